"""What msplat_adjust_cloud costs beside msplat_transform_cloud of the same cloud in the same run -- the same
bytes moved with less arithmetic -- and beside the route through the host it replaces.

usage (GPU box, repo root):
    python tools/adjust_timing.py [--sizes 1000000] [--storages fp32,sh_fp16,sh_q8] [--shares 1.0,0.01] [--reps 5] [--out FILE]

Synthetic full-SH clouds, a tint of weight 0.1 and a fade to 0.9, a random selection of the given share (1.0: d_select = NULL).
Every (size, storage) pair is a child process under its own `timeout`; the first failure ends the run.  One JSON line per (size,
storage, share) on stdout (and appended to --out).  The *_kernels_ms are the one kernel of a call between two stream events
(enable_timing; msplat_debug_upload_kernel_ms), the MEDIAN over --reps calls after one untimed call, which pays the one-time
allocations -- transform_timing.py's protocol, repeated:

  adjust_kernels_ms          adjust_kernel with MSPLAT_ADJUST_COLOUR | MSPLAT_ADJUST_OPACITY
  adjust_colour_kernels_ms   ... with MSPLAT_ADJUST_COLOUR alone
  adjust_opacity_kernels_ms  ... with MSPLAT_ADJUST_OPACITY alone: nothing behind a compact record's head is decoded
  transform_kernels_ms       transform_kernel on the same context and selection (a rotation, SH included): the median of the
                             samples taken before and after the adjust calls (transform_before_after_ms: the two medians)
  adjust_over_transform      adjust_kernels_ms / transform_kernels_ms
  spread                     (max - min) / median of the adjust_kernels_ms samples
  adjust_ms                  the whole call, host clock (the last one): + the new store's allocation, the per-cloud buffers and
                             spatial_reorder (Morton storage from 2^18 splats on)
  pass_bytes, pass_gb_s      N x 2 x (16 + 16 F4), what the pass reads and writes of positions and records; over adjust_kernels_ms
  host_route_ms              what exists without the call: msplat_download_cloud, the rule in numpy on the selected rows, Init of
                             the result (which drops the mask and the overlay classes, and quantises an sh_q8 cloud again)
  n, f4                      N, float4s per stored record
A run without a GPU fails at the first context."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CHILD_TIMEOUT = 420
F4 = {"fp32": 16, "sh_fp16": 10, "sh_q8": 8}


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def child(n, storage, shares, reps, out):
    import bench  # noqa: F401  (sets the queue count before the HIP runtime starts, as bench.py does)
    import ctypes as C
    import numpy as np
    import torch
    from splatapult_amd import SplatRenderer, synthetic, tint_matrix
    from transform_timing import similarity

    aos = np.ascontiguousarray(synthetic.make_cloud(n, seed=0xC0 + n % 251, full_sh=True, pos_sigma=1.5).as_array()[:n], np.float32)
    M = similarity()
    s = np.cbrt(np.linalg.det(M.reshape(4, 4)[:3, :3].astype(np.float64)))
    M[:12] = (M[:12].reshape(3, 4) / s).reshape(12).astype(np.float32)      # a rotation: repeated calls keep the covariances' size
    tint, fade = tint_matrix((1.0, 0.55, 0.1), 0.1), 0.9

    def kernels_ms(r):
        ms = C.c_float(-1.0)
        r._lib.msplat_debug_upload_kernel_ms(r._ctx, C.byref(ms))
        return ms.value

    def samples(call):
        call()                                                   # untimed: the first call
        got = []
        for _ in range(reps):
            call()
            got.append(kernels_ms(r))
        return got

    for share in shares:
        select = sel_host = None
        if share < 1.0:
            sel_host = np.random.default_rng(int(share * 1000) + n % 997).random(n) < share
            select = torch.from_numpy(sel_host.view(np.uint8)).to("cuda:0")
            torch.cuda.synchronize()
        r = SplatRenderer(device=0, enable_timing=1000, cloud_storage=storage)
        if not r.Init(aos, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        line = dict(kind="adjust", n=n, storage=storage, share=share, f4=F4[storage], reps=reps)
        before = samples(lambda: r.TransformCloud(M, select))
        both = samples(lambda: r.AdjustCloud(tint, fade, select))
        r.synchronize()
        t0 = time.perf_counter()
        r.AdjustCloud(tint, fade, select)
        line["adjust_ms"] = (time.perf_counter() - t0) * 1e3
        line["adjust_kernels_ms"] = statistics.median(both)
        line["spread"] = (max(both) - min(both)) / line["adjust_kernels_ms"] if line["adjust_kernels_ms"] > 0 else None
        line["adjust_colour_kernels_ms"] = statistics.median(samples(lambda: r.AdjustCloud(colour=tint, select=select)))
        line["adjust_opacity_kernels_ms"] = statistics.median(samples(lambda: r.AdjustCloud(opacity=fade, select=select)))
        after = samples(lambda: r.TransformCloud(M, select))
        line["transform_kernels_ms"] = statistics.median(before + after)
        line["transform_before_after_ms"] = [statistics.median(before), statistics.median(after)]
        line["adjust_over_transform"] = line["adjust_kernels_ms"] / line["transform_kernels_ms"] if line["transform_kernels_ms"] > 0 else None
        line["pass_bytes"] = n * 2 * (16 + 16 * F4[storage])
        line["pass_gb_s"] = line["pass_bytes"] / (line["adjust_kernels_ms"] * 1e6) if line["adjust_kernels_ms"] > 0 else None
        # the route without the call, on a context that holds the cloud again
        if not r.Init(aos, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        r.synchronize()
        G, o = tint[:, :3], tint[:, 3]
        t0 = time.perf_counter()
        rows = r.download_cloud(True)
        pick = slice(None) if sel_host is None else sel_host
        sh = np.stack([rows[pick][:, [4 + 4 * c + k if k < 4 else 25 + 12 * c + (k - 4) for k in range(16)]] for c in range(3)], axis=1)
        new = np.einsum("cj,sjk->sck", G, sh)
        new[:, :, 0] += ((0.5 * G.sum(axis=1) + o - 0.5) / 0.28209479177387814).astype(np.float32)
        for c in range(3):
            rows[pick, 4 + 4 * c:8 + 4 * c] = new[:, c, :4]
            rows[pick, 25 + 12 * c:37 + 12 * c] = new[:, c, 4:]
        rows[pick, 3] = np.clip(np.float32(fade) * rows[pick, 3], 0.0, 1.0)
        if not r.Init(rows, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        r.synchronize()
        line["host_route_ms"] = (time.perf_counter() - t0) * 1e3
        r.close()
        emit(line, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000")
    ap.add_argument("--storages", default="fp32,sh_fp16,sh_q8")
    ap.add_argument("--shares", default="1.0,0.01")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    shares = [float(s) for s in args.shares.split(",")]
    if args.child:
        child(int(args.child[0]), args.child[1], shares, args.reps, args.out)
        return
    for n in (int(s) for s in args.sizes.split(",")):
        for storage in args.storages.split(","):
            cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", str(n), storage,
                   "--shares", args.shares, "--reps", str(args.reps)] + (["--out", args.out] if args.out else [])
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                raise SystemExit("child (%d, %s) ended with status %d: nothing more is started" % (n, storage, rc))


if __name__ == "__main__":
    main()
