"""What selection by position costs (msplat_mark_volume, msplat_mark_view, msplat_measure_cloud).

usage (GPU box, repo root):
    python tools/select_timing.py [--sizes 1000000,6000000] [--reps 30] [--parent-lib LIB] [--out FILE]

Per size and storage order (upload, Morton) two child processes, each under its own `timeout`; the first failure ends the run.  One
JSON line per child on stdout (and appended to --out):

  kernels  the child runs under `rocprofv3 --kernel-trace --stats`, so every kernel is timed the same way, by its own dispatch:
           --reps calls each of MarkVolume (a sphere that holds ~10 % of the cloud), MarkView (the whole 1920 x 1080 viewport),
           MeasureCloud of the marked selection, and a Sort that starts with visibility_kernel because SetCrop of the SAME matrix was
           called just before -- the yardstick of mark_volume_kernel: the same plane and order table, 16 B + the boxes more written.
           Average microseconds of mark_volume_kernel, mark_view_kernel, measure_cloud_kernel, rows_finish_kernel,
           visibility_kernel and, where the upload ran them (Morton storage), cloud_moments_kernel / cloud_moments_finish.
           With --parent-lib a third child times visibility_kernel on that build (the parent commit's) the same way.
  clock    no profiler: msplat_measure_cloud by the host clock (the stream drain and the 112-byte copy included) and between its own
           stream events (msplat_debug_upload_kernel_ms), MarkVolume + synchronize by the host clock, and the route these calls
           replace: download_cloud to the host, the crop expression and the count / box / mean in numpy.
A run without a GPU fails at the first context."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_TIMEOUT = 300
KERNELS = ("mark_volume_kernel", "mark_view_kernel", "measure_cloud_kernel", "rows_finish_kernel", "visibility_kernel",
           "cloud_moments_kernel", "cloud_moments_finish")
W, H = 1920, 1080


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def setup(n, order):
    """(renderer, records, the sphere's matrix, the view) of a synthetic SH-degree-0 cloud stored in `order`"""
    import bench  # noqa: F401  (sets the queue count before the HIP runtime starts, as bench.py does)
    import numpy as np
    from splatapult_amd import SplatRenderer, _capi, camera, synthetic
    from splatapult_amd.scene import GaussianCloud

    a = synthetic.generate(n, seed=0x5EED1234, full_sh=False, pos_sigma=1.5)
    gc = GaussianCloud(GaussianCloud.Options(False, False))
    if not gc.FromAttributes(a["xyz"], a["f_dc"], None, a["opacity"], a["log_scale"], a["rot"]):
        raise SystemExit("FromAttributes failed")
    aos = np.ascontiguousarray(gc.as_array(), np.float32)
    radius = float(np.quantile(np.linalg.norm(a["xyz"].astype(np.float64), axis=1), 0.10))
    M = np.ascontiguousarray(np.diag([1.0 / radius] * 3 + [1.0]).reshape(16), np.float32)
    view = (camera.pose((0.0, 0.0, 7.0)), camera.perspective(camera.FOVY, W / H), [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR])
    r = SplatRenderer(device=0, spatial_order=_capi.SPATIAL_ON if order == "morton" else _capi.SPATIAL_OFF, enable_timing=True)
    if not r.Init(aos, False, False):
        raise SystemExit("Init failed: " + r.last_error())
    return r, aos, M, view


def child_kernels(n, order, reps, crop_only):
    import torch
    r, _, M, view = setup(n, order)
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(reps + 2):
        if not crop_only:
            r.MarkVolume(M, mask, 1, "sphere")
            r.MarkView(*view, mask, 2)
            r.MeasureCloud(mask)
        r.SetCrop(M, "sphere")                          # the next Sort starts with visibility_kernel
        r.Sort(*view)
        r.synchronize()
    r.close()


def child_clock(n, order, reps, out):
    import numpy as np
    import torch
    r, aos, M, view = setup(n, order)
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    mark, measure, measure_kernels = [], [], []
    ms = C.c_float()
    for k in range(reps + 2):
        t0 = time.perf_counter()
        r.MarkVolume(M, mask, 1, "sphere")
        r.synchronize()
        t1 = time.perf_counter()
        m = r.MeasureCloud(mask)
        t2 = time.perf_counter()
        r._lib.msplat_debug_upload_kernel_ms(r._ctx, C.byref(ms))
        if k >= 2:
            mark.append(1e3 * (t1 - t0)), measure.append(1e3 * (t2 - t1)), measure_kernels.append(ms.value)
    route = []
    for k in range(3):
        t0 = time.perf_counter()
        rows = r.download_cloud(False)
        q = rows[:, 0:3] * M[0]
        sel = (q * q).sum(axis=1) <= 1.0
        chosen = rows[sel, 0:3]
        box = (chosen.min(axis=0), chosen.max(axis=0), chosen.mean(axis=0, dtype=np.float64))
        route.append(1e3 * (time.perf_counter() - t0))
    assert int(sel.sum()) == m["selected"], (int(sel.sum()), m["selected"])
    med = lambda v: float(np.median(v))
    emit({"tool": "select_timing", "kind": "clock", "splats": n, "storage_order": order, "selected": m["selected"],
          "mark_volume_and_sync_ms": med(mark), "measure_call_ms": med(measure), "measure_kernels_ms": med(measure_kernels),
          "host_route_ms": med(route), "host_route_box_lo": [float(v) for v in box[0]]}, out)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None, help="libmsplat.so built from the parent commit: its visibility_kernel, timed the same way")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, n, order = args.child[0], int(args.child[1]), args.child[2]
        if kind == "clock":
            child_clock(n, order, args.reps, args.out)
        else:
            child_kernels(n, order, args.reps, kind == "crop_only")
        return

    def spawn(child, profile_dir=None, lib=None):
        env = dict(os.environ)
        env.pop("MSPLAT_LIB_PATH", None)
        if lib:
            env["MSPLAT_LIB_PATH"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child"] + child
        if args.out and not profile_dir:
            cmd += ["--out", args.out]
        if profile_dir:             # (the program itself goes after `--`)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", profile_dir, "-o", "run", "--output-format", "csv", "--"] + cmd
        rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT)] + cmd, cwd=ROOT, env=env,
                            stdout=subprocess.DEVNULL if profile_dir else None).returncode
        if rc != 0:
            raise SystemExit("child %s ended with status %d: nothing more is started" % (child, rc))

    def kernel_stats(profile_dir):
        found = glob.glob(os.path.join(profile_dir, "**", "run_kernel_stats.csv"), recursive=True)
        if not found:
            raise SystemExit("rocprofv3 left no run_kernel_stats.csv under " + profile_dir)
        stats = {}
        for row in csv.DictReader(open(found[0])):
            for k in KERNELS:
                if k + "(" in row["Name"] or row["Name"].endswith(k) or ("::" + k) in row["Name"]:
                    stats[k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                "min_us": float(row.get("MinNs") or "nan") / 1e3, "max_us": float(row.get("MaxNs") or "nan") / 1e3}
        return stats

    for n in [int(s) for s in args.sizes.split(",") if s]:
        for order in ("upload", "morton"):
            for kind, lib in (("kernels", None),) + ((("crop_only", args.parent_lib),) if args.parent_lib else ()):
                tmp = tempfile.mkdtemp(prefix="msplat_select_")
                try:
                    spawn([kind, str(n), order], profile_dir=tmp, lib=lib)
                    emit({"tool": "select_timing", "kind": "kernels" if lib is None else "parent_visibility_kernel", "splats": n,
                          "storage_order": order, "reps": args.reps, "kernels": kernel_stats(tmp)}, args.out)
                finally:
                    shutil.rmtree(tmp, ignore_errors=True)
            spawn(["clock", str(n), order])


if __name__ == "__main__":
    main()
