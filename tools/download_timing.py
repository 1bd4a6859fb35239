"""What getting a cloud out of the device costs (msplat_download_cloud_device, msplat_download_attributes_device,
msplat_download_ply_vertices_device and msplat_export_ply) beside the only route there was before them, on the
BASELINE config 2 cloud: 1 M splats with full SH.

usage (GPU box, repo root):
    python tools/download_timing.py [--n 1000000] [--storages fp32,sh_fp16,sh_q8] [--repeats 5] [--out FILE]

Per cloud storage and spatial_order (OFF: the store is in upload order; ON: in Morton order, rows are gathered through the inverse
order) one JSON line on stdout (and appended to --out):
    kernel .......... per device route -- `records` = unpack_kernel, `attributes` = egress_kernel<AttrWriter>, `vertices` =
                      egress_kernel<VertexWriter> with write_ply's 248-byte layout -- the kernel alone between two stream events
                      (msplat_debug_upload_kernel_ms on a context with enable_timing; on a reordered store invert_order_kernel is in
                      it), median of --repeats calls after one warm-up: ms, the bytes it must move (stored records read once, rows
                      written once, + 8 B a splat for the order on a reordered store), GB/s, and that as a fraction of what a plain copy
                      gets on this box (`hbm_delivered`: bench.py's own measurement, taken here once; tools/ubench_stream.hip measures
                      the same)
    call_ms ......... the same calls by the host clock (each returns after the stream has drained)
    export_ply_ms ... msplat_export_ply to a file in --dir, end to end, median
    host_route_ms ... the route the parent commit offers to the same file: msplat_download_cloud into host memory, then
                      GaussianCloud.ExportPly of those records (the eigen-decomposition on one host thread, the write); `download`
                      and `export` apart, median of min(--repeats, 3)
    files_equal ..... the two files hold the same header; `max_rot_diff` / `scale_rtol`: how far their vertices are apart
A run without a GPU fails at the first context."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None, help="splats (default: the cfg2 workload's 1 000 000)")
    ap.add_argument("--storages", default="fp32,sh_fp16,sh_q8")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the PLY files go (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()

    import bench                                    # (sets GPU_MAX_HW_QUEUES before the HIP runtime starts, as bench.py does)
    import numpy as np
    import torch
    from splatapult_amd import SplatRenderer, _capi, synthetic
    from splatapult_amd.scene import GaussianCloud

    wl = bench.WORKLOADS["cfg2"]
    n = args.n or wl["n"]
    a = synthetic.generate(n, seed=wl["seed"], full_sh=True, pos_sigma=wl["pos_sigma"])
    gc = GaussianCloud(GaussianCloud.Options(True, True))
    if not gc.FromAttributes(a["xyz"], a["f_dc"], a["f_rest"], a["opacity"], a["log_scale"], a["rot"]):
        raise SystemExit("FromAttributes failed")
    aos = np.ascontiguousarray(gc.as_array(), np.float32)
    off = _capi.AttrOffsets(0, 16, 32, 48, 64, 76, 88, 100, 116, 132, 148, 164, 180, 196, 212, 228)
    d_rec = torch.empty(n * 244, dtype=torch.uint8, device="cuda:0")
    d_vtx = torch.empty(n * 248, dtype=torch.uint8, device="cuda:0")
    d_attr = [torch.empty((n, k), dtype=torch.float32, device="cuda:0") for k in (3, 3, 45, 1, 3, 4)]
    torch.cuda.synchronize()
    hbm = bench.hbm_delivered("cuda:0")
    lib = _capi.lib()
    L = _capi.PlyLayout()                           # synthetic.write_ply's 62-float vertex, which is ExportPly's
    L.vertex_size, L.x, L.y, L.z, L.opacity = 248, 0, 4, 8, 216
    for i in range(45):
        L.f_rest[i] = 36 + 4 * i
    for i in range(4):
        L.rot[i] = 232 + 4 * i
        if i < 3:
            L.f_dc[i], L.scale[i] = 24 + 4 * i, 220 + 4 * i
    tmp = args.dir or tempfile.mkdtemp(prefix="msplat_download_")
    dev_path, host_path = os.path.join(tmp, "device.ply"), os.path.join(tmp, "host.ply")

    def timed(call, ctx, kernel, repeats):
        ms, kms = [], []
        for k in range(repeats + 1):                # the first call is the warm-up: code objects, the order on the device
            t0 = time.perf_counter()
            rc = call()
            t1 = time.perf_counter()
            if rc != _capi.OK:
                raise SystemExit("the call failed: " + lib.msplat_last_error(ctx).decode())
            if k:
                ms.append(1e3 * (t1 - t0))
                if kernel:
                    v = C.c_float(-1.0)
                    lib.msplat_debug_upload_kernel_ms(ctx, C.byref(v))
                    kms.append(v.value)
        return float(np.median(ms)), (float(np.median(kms)) if kernel else None)

    def kernel_row(ms, nbytes):
        gbps = nbytes / (ms * 1e-3) / 1e9
        copy = hbm.get("copy_GBps")
        return {"ms": ms, "bytes": nbytes, "GBps": gbps, "frac_of_hbm_delivered": (gbps / copy) if copy else None}

    for storage in [s for s in args.storages.split(",") if s]:
        for spatial, sname in ((_capi.SPATIAL_OFF, "off"), (_capi.SPATIAL_ON, "on")):
            r = SplatRenderer(device=0, cloud_storage=storage, spatial_order=spatial, enable_timing=True)
            if not r._create(False):
                raise SystemExit("msplat_create failed: " + r.last_error())
            ctx = r._ctx
            if lib.msplat_upload_cloud(ctx, aos.ctypes.data, n, 244, C.byref(off), 1) != _capi.OK:
                raise SystemExit("upload failed: " + r.last_error())
            r._n = n
            read = n * 16 * {"fp32": 16, "sh_fp16": 10, "sh_q8": 8}[storage] + (8 * n if sname == "on" else 0)
            rec_ms, rec_k = timed(lambda: lib.msplat_download_cloud_device(ctx, C.c_void_p(d_rec.data_ptr()), n * 244), ctx, True, args.repeats)
            att_ms, att_k = timed(lambda: lib.msplat_download_attributes_device(ctx, n, *[C.c_void_p(t.data_ptr()) for t in d_attr]), ctx, True,
                                  args.repeats)
            vtx_ms, vtx_k = timed(lambda: lib.msplat_download_ply_vertices_device(ctx, C.c_void_p(d_vtx.data_ptr()), n * 248, C.byref(L)), ctx, True,
                                  args.repeats)
            exp_ms, _ = timed(lambda: lib.msplat_export_ply(ctx, dev_path.encode()), ctx, False, args.repeats)
            # the parent commit's route to the same file
            down, export = [], []
            host = GaussianCloud(GaussianCloud.Options(True, True))
            host.FromAttributes(*[a[k] for k in ("xyz", "f_dc", "f_rest", "opacity", "log_scale", "rot")])      # (a shell of n records)
            for _ in range(min(args.repeats, 3)):
                t0 = time.perf_counter()
                got = r.download_cloud(True)
                t1 = time.perf_counter()
                C.memmove(host.GetRawDataPtr(), got.ctypes.data, n * 244)
                if not host.ExportPly(host_path):
                    raise SystemExit("GaussianCloud.ExportPly failed")
                t2 = time.perf_counter()
                down.append(1e3 * (t1 - t0))
                export.append(1e3 * (t2 - t1))
            raw_d, raw_h = open(dev_path, "rb").read(), open(host_path, "rb").read()
            end = raw_d.index(b"end_header\n") + 11
            vd = np.frombuffer(raw_d, "<f4", n * 62, end).reshape(n, 62)
            vh = np.frombuffer(raw_h, "<f4", n * 62, end).reshape(n, 62)
            fin = np.isfinite(vh[:, 54:58]) & (vh[:, 54:58] != 0)
            line = {"tool": "download_timing", "splats": n, "cloud_storage": storage, "spatial_order": sname,
                    "kernel": {"records": kernel_row(rec_k, read + n * 244), "attributes": kernel_row(att_k, read + n * 59 * 4),
                               "vertices": kernel_row(vtx_k, read + n * 248)},
                    "call_ms": {"records": rec_ms, "attributes": att_ms, "vertices": vtx_ms},
                    "export_ply_ms": exp_ms,
                    "host_route_ms": {"download": float(np.median(down)), "export": float(np.median(export)),
                                      "total": float(np.median(down) + np.median(export))},
                    "files_equal": {"header": raw_d[:end] == raw_h[:end], "copies": bool(np.array_equal(vd[:, :54].view(np.uint32), vh[:, :54].view(np.uint32))),
                                    "max_rot_diff": float(np.abs(vd[:, 58:62] - vh[:, 58:62]).max()),
                                    "scale_rtol": float((np.abs(vd[:, 54:58] - vh[:, 54:58])[fin] / np.abs(vh[:, 54:58])[fin]).max())},
                    "repeats": args.repeats, "hbm_delivered": hbm}
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
            r.close()
    for p in (dev_path, host_path):
        if os.path.exists(p):
            os.remove(p)


if __name__ == "__main__":
    main()
