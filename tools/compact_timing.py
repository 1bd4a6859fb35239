"""What msplat_compact_cloud costs beside the route through the host it replaces, and what the smaller cloud
saves per frame.

usage (GPU box, repo root):
    python tools/compact_timing.py [--sizes 1000000,6000000] [--storages fp32,sh_q8] [--shares 0.5,0.9] [--frames 50] [--out FILE]

Synthetic full-SH clouds, a random mask that keeps the given share, a 1920 x 1080 fp32 target, serial frames (Sort + Render, device
output, one synchronise per frame).  Every (size, storage) pair is a child process under its own `timeout`; the first failure ends
the run.  One JSON line per (size, storage, share) on stdout (and appended to --out), host clock unless named otherwise:

  masked_frame_ms      Sort + Render of the masked context (the mask set, the cloud whole)
  compact_ms           msplat_compact_cloud, the call
  compact_kernels_ms   of it: flags, count, offsets, index, the 4-byte readback of K, the allocation of the new store and the gather,
                       between two stream events (enable_timing; msplat_debug_upload_kernel_ms)
  compact_rest_ms      the difference: the per-cloud buffers for K and spatial_reorder (Morton storage from 2^18 splats on)
  gather_bytes         K x 2 x (16 + 16 F4): what the gather reads and writes of positions and records
  compacted_frame_ms   Sort + Render of the compacted context
  host_route_ms        what exists without the call: msplat_download_cloud, numpy take of the kept rows, Init of the result
  kept, n, f4          K, N, float4s per stored record
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
W, H = 1920, 1080
F4 = {"fp32": 16, "sh_fp16": 10, "sh_q8": 8}


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def child(n, storage, shares, frames, out):
    import bench  # noqa: F401  (sets the queue count before the HIP runtime starts, as bench.py does)
    import ctypes as C
    import math
    import numpy as np
    import torch
    from splatapult_amd import SplatRenderer, camera, synthetic

    aos = np.ascontiguousarray(synthetic.make_cloud(n, seed=0xC0 + n % 251, full_sh=True, pos_sigma=1.5).as_array()[:n], np.float32)
    proj = camera.perspective(camera.FOVY, W / H)
    nf = [camera.Z_NEAR, camera.Z_FAR]
    views = [(camera.orbit(7.0, 2.0 * math.pi * k / 16.0), proj, [0, 0, W, H], nf) for k in range(16)]
    fb = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def frame_ms(r):
        for v in views:                                          # every pose once, untimed
            r.Sort(*v)
            r.Render(*v, out_ptr=fb.data_ptr())
        r.synchronize()
        t0 = time.perf_counter()
        for k in range(frames):
            v = views[k % len(views)]
            r.Sort(*v)
            r.Render(*v, out_ptr=fb.data_ptr())
            r.synchronize()
        return (time.perf_counter() - t0) * 1e3 / frames

    for share in shares:
        mask = np.random.default_rng(int(share * 1000) + n % 997).random(n) < share
        r = SplatRenderer(device=0, enable_timing=1000, cloud_storage=storage)     # (events on every 1000th frame only)
        if not r.Init(aos, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        r.SetVisibility(mask)
        line = dict(kind="compact", n=n, storage=storage, share=share, f4=F4[storage], frames=frames)
        line["masked_frame_ms"] = frame_ms(r)
        r.synchronize()
        t0 = time.perf_counter()
        k = r.CompactCloud()
        line["compact_ms"] = (time.perf_counter() - t0) * 1e3
        ms = C.c_float(-1.0)
        r._lib.msplat_debug_upload_kernel_ms(r._ctx, C.byref(ms))
        line["compact_kernels_ms"] = ms.value
        line["compact_rest_ms"] = line["compact_ms"] - ms.value
        line["kept"] = k
        line["gather_bytes"] = k * 2 * (16 + 16 * F4[storage])
        line["compacted_frame_ms"] = frame_ms(r)
        # the route without the call, on a context that holds the whole cloud again
        if not r.Init(aos, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        r.synchronize()
        t0 = time.perf_counter()
        rows = r.download_cloud(True)
        if not r.Init(np.ascontiguousarray(rows[mask]), False, False):
            raise SystemExit("Init failed: " + r.last_error())
        r.synchronize()
        line["host_route_ms"] = (time.perf_counter() - t0) * 1e3
        r.close()
        emit(line, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--storages", default="fp32,sh_q8")
    ap.add_argument("--shares", default="0.5,0.9")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    shares = [float(s) for s in args.shares.split(",")]
    if args.child:
        child(int(args.child[0]), args.child[1], shares, args.frames, args.out)
        return
    for n in (int(s) for s in args.sizes.split(",")):
        for storage in args.storages.split(","):
            cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", str(n), storage,
                   "--shares", args.shares, "--frames", str(args.frames)] + (["--out", args.out] if args.out else [])
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                raise SystemExit("child (%d, %s) ended with status %d: nothing more is started" % (n, storage, rc))


if __name__ == "__main__":
    main()
