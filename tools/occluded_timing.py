#!/usr/bin/env python3
"""usage (GPU box): python tools/occluded_timing.py [--frames 256] [--out FILE]

What does the occluder test cost, and what does a plane that hides splats save?  On BASELINE config 2 (1 M splats, 1920x1080 fp32,
64-step orbit), one frame at a time, on one box in one run:
  plain   msplat_render,
  open    msplat_render_occluded with a plane of +inf: every splat passes -- the price of the test,
  half    a plane that closes the left half of the screen at the median z_w of the splats inside the frustum (the right half is open),
  closed  a plane of 0.0: nothing passes anywhere.
The median is taken on the host from the first pose (view and projection in float64, the geometry stage's ndc window): the orbit keeps
its distance to a cloud that is symmetric about the axis, so it serves every pose.
Every measurement is a child process of its own under its own `timeout`; the first child that fails, faults or runs out of time ends
the run -- nothing more is started on the GPU after it.  The number is frames per second of Sort + Render over --frames frames after
a warm-up, wall clock around a synchronised block, best of three blocks.  Prints a markdown table and one JSON line."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOAD = dict(n=1_000_000, seed=0x5EED1234, pos_sigma=1.5, cam_z=7.0, desc="1 M splats, 1920x1080 (BASELINE config 2)")
W, H = 1920, 1080
KINDS = ("plain", "open", "half", "closed")


def median_window_depth(xyz, cam, proj):
    """median of 0.5 ndc.z + 0.5 over the splats whose centre the geometry stage keeps (0.25 <= ndc.z <= 1, |ndc.xy| <= 1)"""
    import numpy as np
    view = np.linalg.inv(np.asarray(cam, np.float64).reshape(4, 4).T)
    P = np.asarray(proj, np.float64).reshape(4, 4).T
    clip = (P @ view @ np.concatenate([xyz.astype(np.float64), np.ones((xyz.shape[0], 1))], axis=1).T).T
    front = clip[:, 3] > 0
    ndc = clip[front, :3] / clip[front, 3:4]
    seen = (np.abs(ndc[:, 0]) <= 1) & (np.abs(ndc[:, 1]) <= 1) & (ndc[:, 2] >= 0.25) & (ndc[:, 2] <= 1)
    return float(np.median(0.5 * ndc[seen, 2] + 0.5))


def worker(args):
    """one measurement in this process: prints one JSON line"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from splatapult_amd import SplatRenderer, camera, synthetic
    wl = WORKLOAD
    cloud = synthetic.make_cloud(wl["n"], seed=wl["seed"], full_sh=True, pos_sigma=wl["pos_sigma"])
    r = SplatRenderer(device=0, fb_format="fp32")
    assert r.Init(cloud, False, False), r.last_error()
    dev = torch.device("cuda:0")
    fb = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    proj = camera.perspective(camera.FOVY, W / H)
    vp, nf = [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR]
    poses = [camera.orbit(wl["cam_z"], 2.0 * math.pi * k / 64.0) for k in range(64)]
    level = None
    plane = None
    if args.kind != "plain":
        host = np.full((H, W), np.inf if args.kind != "closed" else 0.0, np.float32)
        if args.kind == "half":
            level = median_window_depth(cloud.as_array()[:, :3], poses[0], proj)
            host[:, :W // 2] = level
        plane = torch.from_numpy(host).to(dev)
    torch.cuda.synchronize()

    def block(frames, start):
        t0 = time.perf_counter()
        for k in range(frames):
            c = poses[(start + k) % 64]
            r.Sort(c, proj, vp, nf)
            if plane is None:
                r.Render(c, proj, vp, nf, out_ptr=fb.data_ptr(), pitch_bytes=W * 16)
            else:
                r.Render(c, proj, vp, nf, out_ptr=fb.data_ptr(), pitch_bytes=W * 16, occluder_ptr=plane.data_ptr())
        r.synchronize()
        return frames / (time.perf_counter() - t0)

    block(args.warmup, 0)
    fps = [block(args.frames, 64 * i) for i in range(3)]
    touched = float((fb[..., :3] != 0).any(dim=-1).float().mean().item())        # share of pixels the last frame coloured
    r.close()
    print(json.dumps(dict(kind=args.kind, fps=max(fps), ms=1000.0 / max(fps), blocks=[round(f, 1) for f in fps], level=level,
                          coloured=round(touched, 4))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a single measurement may take")
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kind", default="plain", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    results = {}
    lines = ["| %s, serial frames | frames/s | ms per frame | against plain |" % WORKLOAD["desc"], "|---|---|---|---|"]
    for kind in KINDS:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--kind", kind,
               "--frames", str(args.frames), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:          # a failure, a fault or the time limit: nothing more is started
            print("measurement %s ended with status %d: stopping" % (kind, p.returncode), file=sys.stderr)
            sys.exit(p.returncode or 1)
        results[kind] = json.loads(p.stdout.strip().splitlines()[-1])
        print("%s: %s" % (kind, results[kind]), file=sys.stderr, flush=True)
        lines.append("| %s | %.1f | %.3f | %.3f |" % (kind, results[kind]["fps"], results[kind]["ms"], results[kind]["fps"] / results["plain"]["fps"]))
    text = "\n".join(lines) + "\n" + json.dumps({"occluded_timing": results})
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
