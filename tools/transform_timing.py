"""What msplat_transform_cloud costs beside the route through the host it replaces, and beside an all-kept
msplat_compact_cloud of the same cloud, which moves the same bytes.

usage (GPU box, repo root):
    python tools/transform_timing.py [--sizes 1000000,6000000] [--storages fp32,sh_q8] [--shares 1.0,0.1] [--out FILE]

Synthetic full-SH clouds, a rotation plus a uniform scale, a random selection of the given share (1.0: d_select = NULL).  Every
(size, storage) pair is a child process under its own `timeout`; the first failure ends the run.  One JSON line per (size, storage,
share) on stdout (and appended to --out), host clock unless named otherwise:

  transform_ms          msplat_transform_cloud, the call (the second of two: the first pays the one-time allocations)
  transform_kernels_ms  of it: transform_kernel between two stream events (enable_timing; msplat_debug_upload_kernel_ms)
  transform_rest_ms     the difference: the new store's allocation, the per-cloud buffers and spatial_reorder (Morton storage from
                        2^18 splats on)
  pass_bytes            N x 2 x (16 + 16 F4): what the pass reads and writes of positions and records
  pass_gb_s             pass_bytes / transform_kernels_ms
  compact_kernels_ms    an all-kept msplat_compact_cloud of the same context, its kernels (flags, scan, the allocation, the gather):
                        the same bytes moved without the arithmetic -- a transform pass much slower than this is not memory-bound
  host_route_ms         what exists without the call: msplat_download_cloud, the rule in numpy (centres and covariances only, the
                        45 x 45 SH rotation per splat left out: a lower bound), Init of the result
  n, f4                 N, float4s per stored record
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


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def similarity():
    """column-major float32[16]: a rotation about (1, 2, 0.5) by 0.7 rad times 0.37, plus a translation"""
    import numpy as np
    a = np.array([1.0, 2.0, 0.5]) / np.linalg.norm([1.0, 2.0, 0.5])
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = (np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K) * 0.37
    m[:3, 3] = (0.4, -0.25, 0.6)
    return np.ascontiguousarray(m.T.reshape(16), np.float32)


def child(n, storage, shares, out):
    import bench  # noqa: F401  (sets the queue count before the HIP runtime starts, as bench.py does)
    import ctypes as C
    import numpy as np
    import torch
    from splatapult_amd import SplatRenderer, synthetic

    aos = np.ascontiguousarray(synthetic.make_cloud(n, seed=0xC0 + n % 251, full_sh=True, pos_sigma=1.5).as_array()[:n], np.float32)
    M = similarity()

    def kernels_ms(r):
        ms = C.c_float(-1.0)
        r._lib.msplat_debug_upload_kernel_ms(r._ctx, C.byref(ms))
        return ms.value

    for share in shares:
        select = None
        if share < 1.0:
            select = torch.from_numpy((np.random.default_rng(int(share * 1000) + n % 997).random(n) < share).view(np.uint8)).to("cuda:0")
            torch.cuda.synchronize()
        r = SplatRenderer(device=0, enable_timing=1000, cloud_storage=storage)
        if not r.Init(aos, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        line = dict(kind="transform", n=n, storage=storage, share=share, f4=F4[storage])
        r.TransformCloud(M, select)                              # untimed: the first call
        r.synchronize()
        t0 = time.perf_counter()
        r.TransformCloud(M, select)
        line["transform_ms"] = (time.perf_counter() - t0) * 1e3
        line["transform_kernels_ms"] = kernels_ms(r)
        line["transform_rest_ms"] = line["transform_ms"] - line["transform_kernels_ms"]
        line["pass_bytes"] = n * 2 * (16 + 16 * F4[storage])
        line["pass_gb_s"] = line["pass_bytes"] / (line["transform_kernels_ms"] * 1e6) if line["transform_kernels_ms"] > 0 else None
        assert r.CompactCloud() == n                             # nothing set: every splat is kept
        line["compact_kernels_ms"] = kernels_ms(r)
        # the route without the call, on a context that holds the cloud again
        if not r.Init(aos, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        r.synchronize()
        A = M.reshape(4, 4)[:3, :3].T
        t0 = time.perf_counter()
        rows = r.download_cloud(True)
        rows[:, 0:3] = rows[:, 0:3] @ A.T + M[12:15]
        S = rows[:, 16:25].reshape(-1, 3, 3)                     # (symmetric: the storage order of S does not matter here)
        rows[:, 16:25] = (A @ S @ A.T).reshape(-1, 9)
        if not r.Init(rows, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        r.synchronize()
        line["host_route_ms"] = (time.perf_counter() - t0) * 1e3
        r.close()
        emit(line, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--storages", default="fp32,sh_q8")
    ap.add_argument("--shares", default="1.0,0.1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    shares = [float(s) for s in args.shares.split(",")]
    if args.child:
        child(int(args.child[0]), args.child[1], shares, args.out)
        return
    for n in (int(s) for s in args.sizes.split(",")):
        for storage in args.storages.split(","):
            cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", str(n), storage,
                   "--shares", args.shares] + (["--out", args.out] if args.out else [])
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                raise SystemExit("child (%d, %s) ended with status %d: nothing more is started" % (n, storage, rc))


if __name__ == "__main__":
    main()
