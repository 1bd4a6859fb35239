"""What selection by attribute costs (msplat_cloud_values, msplat_mark_values, msplat_histogram_values).

usage (GPU box, repo root):
    python tools/values_timing.py [--sizes 1000000,6000000] [--storages fp32,sh_fp16,sh_q8] [--reps 20] [--out FILE]

Synthetic full-SH clouds (bench.py's generator).  Per size, storage kind and storage order (upload, Morton) two child processes,
each under its own `timeout`; the first failure ends the run.  One JSON line per child on stdout (and appended to --out):

  kernels  the child runs under `rocprofv3 --kernel-trace --stats`, so every kernel is timed the same way, by its own dispatch:
           --reps calls each of CloudValues("x"), ("alpha"), ("colour_dist2"), ("scale_max"), MarkValues, and the two yardsticks of
           the parent commit in the same run, as many calls each: MarkVolume (mark_volume_kernel: the position plane read, a byte
           written -- the traffic shape of the position kinds and of mark_values_kernel) and AdjustCloud with opacity alone (adjust_kernel: the whole record
           read and written -- what a head kind has to beat).  Average microseconds per kernel name, template arguments included:
           cloud_values_kernel<full SH, storage, group> with group 0 position, 1 alpha, 2 colour, 3 scale.
  clock    no profiler: msplat_histogram_values between its own stream events (msplat_debug_upload_kernel_ms) for uniform values,
           for values in three neighbouring bins of 4096 and for all values equal (one hot bin), at 256 and 4096 bins; the whole
           loop -- CloudValues("alpha"), HistogramValues of 256 bins, MarkValues, synchronize -- by the host clock; the route it replaces, download_cloud and the same in numpy; and what
           this box's HBM delivers to a copy (bench.hbm_delivered, same process) and kind_bytes_over_hbm_us, the time the bytes a kind
           touches per splat would take at that rate.
A run without a GPU fails at the first context."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_TIMEOUT = 300
KERNELS = ("cloud_values_kernel", "mark_values_kernel", "histogram_values_kernel", "rows_finish_kernel", "mark_volume_kernel", "adjust_kernel")
# bytes of the store the rule of a kind needs per splat (+ 4 written, + 4 of the order table in Morton order)
KIND_BYTES = {"x": 16, "alpha": 4, "colour_dist2": 12, "scale_max": 36}
KINDS = {"colour_dist2": (0.1, 0.8, 0.2)}


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def setup(n, storage, order):
    import bench  # noqa: F401  (sets the queue count before the HIP runtime starts, as bench.py does)
    import numpy as np
    from splatapult_amd import SplatRenderer, _capi, synthetic

    aos = np.ascontiguousarray(synthetic.make_cloud(n, seed=0xC0 + n % 251, full_sh=True, pos_sigma=1.5).as_array()[:n], np.float32)
    r = SplatRenderer(device=0, spatial_order=_capi.SPATIAL_ON if order == "morton" else _capi.SPATIAL_OFF, enable_timing=1000,
                      cloud_storage=storage)
    if not r.Init(aos, False, False):
        raise SystemExit("Init failed: " + r.last_error())
    return r, aos


def child_kernels(n, storage, order, reps):
    import numpy as np
    import torch
    r, _ = setup(n, storage, order)
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(n, dtype=torch.float32, device="cuda:0")
    M = np.ascontiguousarray(np.diag([0.5, 0.5, 0.5, 1.0]).reshape(16), np.float32)
    torch.cuda.synchronize()
    for _ in range(reps + 2):
        for kind in ("x", "alpha", "colour_dist2", "scale_max"):
            r.CloudValues(kind, KINDS.get(kind), out=out)
        r.MarkValues(out, 0.01, 0.05, mask, 1)
        r.MarkVolume(M, mask, 1, "sphere")
        r.AdjustCloud(None, 1.0)                        # opacity alone, every splat: the cloud keeps its values
        r.synchronize()
    r.close()


def child_clock(n, storage, order, reps, out):
    import bench
    import numpy as np
    import torch
    r, _ = setup(n, storage, order)
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))
    ms = C.c_float()
    rng = np.random.default_rng(n % 1009)
    inputs = {"uniform": torch.from_numpy(rng.uniform(0.0, 1.0, n).astype(np.float32)).to(dev),
              "three_bins": torch.from_numpy(rng.uniform(0.5, 0.5 + 3.0 / 4096, n).astype(np.float32)).to(dev),     # (three bins of 4096, one of 256)
              "one_bin": torch.full((n,), 0.7, dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    line = {"tool": "values_timing", "kind": "clock", "splats": n, "storage": storage, "storage_order": order, "reps": reps}
    for name, v in inputs.items():
        for bins in (256, 4096):
            got = []
            for k in range(reps + 2):
                h = r.HistogramValues(v, bins, 0.0, 1.0)
                r._lib.msplat_debug_upload_kernel_ms(r._ctx, C.byref(ms))
                if k >= 2:
                    got.append(1e3 * ms.value)
            assert int(h["counts"].sum()) == n
            line["histogram_%s_%d_kernels_us" % (name, bins)] = med(got)
            line["histogram_%s_%d_spread" % (name, bins)] = (max(got) - min(got)) / max(med(got), 1e-9)
    mask = torch.ones(n, dtype=torch.uint8, device=dev)
    vals = torch.empty(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    loop = []
    for k in range(reps + 2):
        t0 = time.perf_counter()
        r.CloudValues("alpha", out=vals)
        h = r.HistogramValues(vals, 256, 0.0, 1.0)
        r.MarkValues(vals, 0.05, float("inf"), mask, 0, outside=True)
        r.synchronize()
        if k >= 2:
            loop.append(1e3 * (time.perf_counter() - t0))
    route = []
    for k in range(3):
        t0 = time.perf_counter()
        rows = r.download_cloud(True)
        counts = np.histogram(rows[:, 3], 256, (0.0, 1.0))[0]
        keep = rows[:, 3] >= 0.05
        route.append(1e3 * (time.perf_counter() - t0))
    assert int(keep.sum()) == int(mask.sum().item()) and int(counts.sum()) == int(h["counts"].sum())
    hbm = bench.hbm_delivered(dev)
    # what the bytes of a kind would take at the rate a plain copy gets here: the store's bytes the rule needs, the order table of a
    # Morton store and the 4 bytes written, per splat
    extra = 4 + (4 if order == "morton" else 0)
    floor_us = {k: 1e6 * n * (b + extra) / (hbm["copy_GBps"] * 1e9) for k, b in KIND_BYTES.items()} if hbm.get("copy_GBps") else None
    line.update(loop_ms=med(loop), host_route_ms=med(route), hidden=int(n - keep.sum()), kind_bytes=KIND_BYTES, hbm_delivered=hbm,
                kind_bytes_over_hbm_us=floor_us)
    emit(line, out)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--storages", default="fp32,sh_fp16,sh_q8")
    ap.add_argument("--orders", default="upload,morton")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, n, storage, order = args.child[0], int(args.child[1]), args.child[2], args.child[3]
        if kind == "clock":
            child_clock(n, storage, order, args.reps, args.out)
        else:
            child_kernels(n, storage, order, args.reps)
        return

    def spawn(child, profile_dir=None):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child"] + child
        if args.out and not profile_dir:
            cmd += ["--out", args.out]
        if profile_dir:             # (the program itself goes after `--`)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", profile_dir, "-o", "run", "--output-format", "csv", "--"] + cmd
        rc = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT)] + cmd, cwd=ROOT, stdout=subprocess.DEVNULL if profile_dir else None).returncode
        if rc != 0:
            raise SystemExit("child %s ended with status %d: nothing more is started" % (child, rc))

    def kernel_stats(profile_dir):
        found = glob.glob(os.path.join(profile_dir, "**", "run_kernel_stats.csv"), recursive=True)
        if not found:
            raise SystemExit("rocprofv3 left no run_kernel_stats.csv under " + profile_dir)
        stats = {}
        for row in csv.DictReader(open(found[0])):
            if any(k in row["Name"] for k in KERNELS):
                name = re.sub(r"\(.*", "", row["Name"]).replace("void ", "").replace("msplat::", "").strip()
                stats[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                               "min_us": float(row.get("MinNs") or "nan") / 1e3, "max_us": float(row.get("MaxNs") or "nan") / 1e3}
        return stats

    for n in [int(s) for s in args.sizes.split(",") if s]:
        for storage in [s for s in args.storages.split(",") if s]:
            for order in [s for s in args.orders.split(",") if s]:
                tmp = tempfile.mkdtemp(prefix="msplat_values_")
                try:
                    spawn(["kernels", str(n), storage, order], profile_dir=tmp)
                    emit({"tool": "values_timing", "kind": "kernels", "splats": n, "storage": storage, "storage_order": order,
                          "reps": args.reps, "kernels": kernel_stats(tmp)}, args.out)
                finally:
                    shutil.rmtree(tmp, ignore_errors=True)
                spawn(["clock", str(n), storage, order])


if __name__ == "__main__":
    main()
