"""What msplat_append_cloud costs beside the route through the host it replaces.

usage (GPU box, repo root):
    python tools/append_timing.py [--sizes 1000000,6000000] [--sources 100000,1000000] [--storages fp32,sh_q8] [--out FILE]

Synthetic full-SH clouds; every splat of the source is appended (d_select = NULL).  The destination is stored as --storages names it,
the source once in the same kind and once in the other one of fp32 / sh_q8 (converting).  Every (size, storage) pair is a child
process under its own `timeout`; the first failure ends the run.  One JSON line per (size, source size, storage, source storage) on
stdout (and appended to --out), host clock unless named otherwise:

  append_ms             msplat_append_cloud, the call, on a context that holds the N-splat cloud again (the second of two: the
                        first pays the one-time allocations)
  append_kernels_ms     of it: the two gathers, or the gather and append_convert_kernel, between two stream events (enable_timing;
                        msplat_debug_upload_kernel_ms); the scan is not in it
  append_rest_ms        the difference: the scan and the readback of K, the new store's allocation, the per-cloud buffers and
                        spatial_reorder (Morton storage from 2^18 splats on)
  moved_bytes           N x 2 x (16 + 16 F4) + K x ((16 + 16 F4 of the source) + (16 + 16 F4)): what the kernels read and write
  moved_gb_s            moved_bytes / append_kernels_ms
  frac_of_hbm_delivered moved_gb_s against bench.py's roofline.hbm_delivered (a plain 1-GiB copy, taken once in the child)
  host_route_ms         what exists without the call: msplat_download_cloud of both contexts, numpy.concatenate, Init of the result
                        (same-kind lines only: the route does not depend on the source's kind but for its download)
  n, ns, f4, src_f4     N, Ns, float4s per stored record of either store
A run without a GPU fails at the first context."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_TIMEOUT = 420
F4 = {"fp32": 16, "sh_fp16": 10, "sh_q8": 8}
OTHER = {"fp32": "sh_q8", "sh_q8": "fp32", "sh_fp16": "fp32"}


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def child(n, storage, sources, out):
    import bench  # (sets the queue count before the HIP runtime starts, as bench.py does)
    import ctypes as C
    import numpy as np
    import torch  # noqa: F401  (the process's HIP runtime is torch's: loaded before the library's first call)
    from splatapult_amd import SplatRenderer, synthetic

    def rows(count, seed):
        return np.ascontiguousarray(synthetic.make_cloud(count, seed=seed, full_sh=True, pos_sigma=1.5).as_array()[:count], np.float32)

    def renderer(aos, kind):
        r = SplatRenderer(device=0, enable_timing=1000, cloud_storage=kind)
        if not r.Init(aos, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        r.synchronize()
        return r

    def kernels_ms(r):
        ms = C.c_float(-1.0)
        r._lib.msplat_debug_upload_kernel_ms(r._ctx, C.byref(ms))
        return ms.value

    copy = bench.hbm_delivered("cuda:0").get("copy_GBps")
    aos = rows(n, 0xC0 + n % 251)
    r = renderer(aos, storage)
    for ns in sources:
        src_aos = rows(ns, 0xA0 + ns % 251)
        for src_storage in (storage, OTHER[storage]):
            s = renderer(src_aos, src_storage)
            line = dict(kind="append", n=n, ns=ns, storage=storage, src_storage=src_storage, f4=F4[storage], src_f4=F4[src_storage])
            for k in range(2):                                   # untimed: the first call
                if r.stats()["num_splats"] != n and not r.Init(aos, False, False):
                    raise SystemExit("Init failed: " + r.last_error())
                r.synchronize()
                t0 = time.perf_counter()
                added, _ = r.AppendCloud(s)
                line["append_ms"] = (time.perf_counter() - t0) * 1e3
                assert added == ns, (added, ns)
            line["append_kernels_ms"] = kernels_ms(r)
            line["append_rest_ms"] = line["append_ms"] - line["append_kernels_ms"]
            line["moved_bytes"] = n * 2 * (16 + 16 * F4[storage]) + ns * ((16 + 16 * F4[src_storage]) + (16 + 16 * F4[storage]))
            line["moved_gb_s"] = line["moved_bytes"] / (line["append_kernels_ms"] * 1e6) if line["append_kernels_ms"] > 0 else None
            line["frac_of_hbm_delivered"] = line["moved_gb_s"] / copy if copy and line["moved_gb_s"] else None
            if src_storage == storage:
                # the route without the call, on a context that holds the N-splat cloud again
                if not r.Init(aos, False, False):
                    raise SystemExit("Init failed: " + r.last_error())
                r.synchronize()
                t0 = time.perf_counter()
                merged = np.concatenate([r.download_cloud(True), s.download_cloud(True)])
                if not r.Init(merged, False, False):
                    raise SystemExit("Init failed: " + r.last_error())
                r.synchronize()
                line["host_route_ms"] = (time.perf_counter() - t0) * 1e3
                del merged
            s.close()
            emit(line, out)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--sources", default="100000,1000000")
    ap.add_argument("--storages", default="fp32,sh_q8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sources = [int(s) for s in args.sources.split(",")]
    if args.child:
        child(int(args.child[0]), args.child[1], sources, args.out)
        return
    for n in (int(s) for s in args.sizes.split(",")):
        for storage in args.storages.split(","):
            cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", str(n), storage,
                   "--sources", args.sources] + (["--out", args.out] if args.out else [])
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                raise SystemExit("child (%d, %s) ended with status %d: nothing more is started" % (n, storage, rc))


if __name__ == "__main__":
    main()
