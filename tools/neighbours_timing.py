"""What selection by neighbourhood costs (msplat_neighbour_values): the grid's build, the search, and the search
rate in candidate tests per second that the default budget (max_tests = 0) is derived from.

usage (GPU box, repo root):
    python tools/neighbours_timing.py [--sizes 1000000] [--neighbours 4,32,256] [--orders upload,morton] [--reps 5] [--out FILE]

The scene-like synthetic cloud of the other timing tools (bench.py's generator, pos_sigma 1.5).  Per size, storage order and radius
-- one radius per requested mean neighbour count, from the cloud's mean density; the mean that was MEASURED is reported -- two child
processes, each under its own `timeout`; the first failure ends the run.  One JSON line per child on stdout (and appended to --out):

  kernels  the child runs under `rocprofv3 --kernel-trace --stats`: --reps calls of NeighbourValues("count") and of ("dist2"); average
           microseconds per kernel name (neighbour_search_kernel<0> counts, <1> takes the minimum).
  clock    no profiler, the host clock around the synchronous call: total_ms of "count", of "dist2" and of "count" with cap = 4;
           build_ms = a call refused by max_tests = 1, which builds the grid, counts the tests, reads them back and stops;
           search_ms = total - build; tests (msplat_neighbour_info.tests), tests_per_s = tests / search time, pairs_per_s likewise for
           the pairs inside the radius, and the grid's numbers.
A run without a GPU fails at the first context."""
import argparse
import csv
import glob
import json
import math
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
POS_SIGMA = 1.5
BUDGET = 1 << 40            # explicit: the tool measures what the default is derived from


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def radius_for(n, neighbours):
    """the radius at which a centre of an isotropic Gaussian cloud of n centres has `neighbours` others on average: the mean of
    the density over the cloud's own centres is n / (8 pi^1.5 sigma^3)"""
    density = n / (8.0 * math.pi ** 1.5 * POS_SIGMA ** 3)
    return (neighbours / (density * 4.0 / 3.0 * math.pi)) ** (1.0 / 3.0)


def setup(n, order):
    import bench  # noqa: F401  (sets the queue count before the HIP runtime starts, as bench.py does)
    import numpy as np
    from splatapult_amd import SplatRenderer, _capi, synthetic

    aos = np.ascontiguousarray(synthetic.make_cloud(n, seed=0xC0 + n % 251, full_sh=True, pos_sigma=POS_SIGMA).as_array()[:n], np.float32)
    r = SplatRenderer(device=0, spatial_order=_capi.SPATIAL_ON if order == "morton" else _capi.SPATIAL_OFF)
    if not r.Init(aos, False, False):
        raise SystemExit("Init failed: " + r.last_error())
    return r


def child_kernels(n, order, radius, reps):
    import torch
    r = setup(n, order)
    out = torch.empty(n, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(reps + 1):
        r.NeighbourValues(radius, "count", max_tests=BUDGET, out=out)
        r.NeighbourValues(radius, "dist2", max_tests=BUDGET, out=out)
    r.close()


def child_clock(n, order, neighbours, radius, reps, out_path):
    import numpy as np
    import torch
    from splatapult_amd import MsplatError, _capi
    r = setup(n, order)
    out = torch.empty(n, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    med = lambda v: float(np.median(v))

    def timed(**kw):
        got = []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            res = r.NeighbourValues(radius, max_tests=BUDGET, out=out, info=True, **kw)
            if k >= 1:
                got.append(1e3 * (time.perf_counter() - t0))
        return got, res[1]

    total, info = timed(kind="count")
    mean_found = float(out.mean().item())
    dist2, _ = timed(kind="dist2")
    capped, _ = timed(kind="count", cap=4)
    build = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        try:
            r.NeighbourValues(radius, "count", max_tests=1, out=out)
            raise SystemExit("a budget of one test was not refused")
        except MsplatError as e:
            assert e.code == _capi.ERR_UNSUPPORTED, e
        if k >= 1:
            build.append(1e3 * (time.perf_counter() - t0))
    search_ms = max(med(total) - med(build), 1e-6)
    emit({"tool": "neighbours_timing", "kind": "clock", "splats": n, "storage_order": order, "reps": reps, "neighbours_wanted": neighbours,
          "radius": radius, "neighbours_mean": mean_found, "total_count_ms": med(total), "total_dist2_ms": med(dist2), "total_count_cap4_ms": med(capped),
          "build_ms": med(build), "search_ms": search_ms, "spread": (max(total) - min(total)) / max(med(total), 1e-9), "tests": info["tests"],
          "tests_per_query": info["tests"] / max(info["queries"], 1), "tests_per_s": info["tests"] / (1e-3 * search_ms),
          "pairs_per_s": mean_found * n / (1e-3 * search_ms), "buckets": info["buckets"], "max_bucket": info["max_bucket"],
          "device_bytes": r.stats()["device_bytes"]}, out_path)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000")
    ap.add_argument("--neighbours", default="4,32,256")
    ap.add_argument("--orders", default="upload,morton")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, n, order, neighbours = args.child[0], int(args.child[1]), args.child[2], float(args.child[3])
        radius = radius_for(n, neighbours)
        if kind == "clock":
            child_clock(n, order, neighbours, radius, args.reps, args.out)
        else:
            child_kernels(n, order, radius, args.reps)
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
            if "neighbour_" in row["Name"] or "compact_offsets_kernel" in row["Name"] or "rows_finish_kernel" in row["Name"]:
                name = re.sub(r"\(.*", "", row["Name"]).replace("void ", "").replace("msplat::", "").strip()
                stats[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                               "min_us": float(row.get("MinNs") or "nan") / 1e3, "max_us": float(row.get("MaxNs") or "nan") / 1e3}
        return stats

    for n in [int(s) for s in args.sizes.split(",") if s]:
        for order in [s for s in args.orders.split(",") if s]:
            for neighbours in [s for s in args.neighbours.split(",") if s]:
                spawn(["clock", str(n), order, neighbours])
                tmp = tempfile.mkdtemp(prefix="msplat_neighbours_")
                try:
                    spawn(["kernels", str(n), order, neighbours], profile_dir=tmp)
                    emit({"tool": "neighbours_timing", "kind": "kernels", "splats": n, "storage_order": order, "reps": args.reps,
                          "neighbours_wanted": float(neighbours), "radius": radius_for(n, float(neighbours)), "kernels": kernel_stats(tmp)}, args.out)
                finally:
                    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
