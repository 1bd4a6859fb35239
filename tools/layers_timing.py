#!/usr/bin/env python3
"""usage (GPU box): python tools/layers_timing.py [--frames 512] [--rounds 5] [--parent-lib PATH] [--out FILE]

What do the planes cost in a VR frame, and does the one-chain stereo path survive them?  On BASELINE config 5 (1 M splats,
2 x 2016 x 2240 fp16, one Sort per frame with the first eye, 64-step orbit), one frame at a time, on one box in one run:
  stereo_plain   msplat_render_stereo                                   two_plain   two msplat_render calls
  stereo_occ     msplat_render_stereo_layers with occluders             two_occ     two msplat_render_occluded calls        (a)
  stereo_both    msplat_render_stereo_layers, occluders + depth planes  two_both    two msplat_render_layers calls          (b)
  mono_occ       msplat_render_occluded, first eye only                 mono_both   msplat_render_layers with both planes   (c)
The occluder of each eye closes the left half of the screen at the median z_w of the splats inside the frustum of the first pose
(tools/occluded_timing.py's "half" plane); the depth planes are separate buffers.
One child process measures all kinds, a block of --frames frames per kind and round, the kinds alternating inside every round, so
that a drift of the box hits them alike; the number per kind is the median over the rounds of the block's ms per frame (wall clock
around a synchronised block), with the rounds' minimum and maximum as the spread.  --parent-lib: a second child loads that build of
libmsplat.so (MSPLAT_LIB_PATH) and measures the kinds it has entry points for -- the parent commit's only way to draw frame (a) is
two_occ.  Every child runs under its own `timeout`; the first that fails, faults or runs out of time ends the run -- nothing more is
started on the GPU after it.  Prints a markdown table and one JSON line."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
WORKLOAD = dict(n=1_000_000, seed=0x5EED1234, pos_sigma=1.5, cam_z=7.0, desc="1 M splats, 2 x 2016 x 2240 fp16 (BASELINE config 5)")
W, H = 2016, 2240
KINDS = ("stereo_plain", "two_plain", "stereo_occ", "two_occ", "stereo_both", "two_both", "mono_occ", "mono_both")
OLD_KINDS = ("stereo_plain", "two_plain", "two_occ", "mono_occ")          # what a build without the layers entry points can run


def worker(args):
    """all of args.kinds in this process, alternating: prints one JSON line"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from occluded_timing import median_window_depth
    from splatapult_amd import SplatRenderer, camera, synthetic
    wl = WORKLOAD
    cloud = synthetic.make_cloud(wl["n"], seed=wl["seed"], full_sh=True, pos_sigma=wl["pos_sigma"])
    r = SplatRenderer(device=0, fb_format="fp16")
    assert r.Init(cloud, False, False), r.last_error()
    dev = torch.device("cuda:0")
    fbs = [torch.zeros((H, W, 4), dtype=torch.float16, device=dev) for _ in range(2)]
    proj = camera.perspective(camera.FOVY, W / H)
    vp, nf = [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR]
    poses = [camera.orbit(wl["cam_z"], 2.0 * math.pi * k / 64.0) for k in range(64)]
    eyes = [[camera.translate_local(c, dx=-0.032), camera.translate_local(c, dx=+0.032)] for c in poses]
    level = median_window_depth(cloud.as_array()[:, :3], eyes[0][0], proj)
    host = np.full((H, W), np.inf, np.float32)
    host[:, :W // 2] = level
    occ = [torch.from_numpy(host).to(dev) for _ in range(2)]
    dep = [torch.zeros((H, W), dtype=torch.float32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    out = [f.data_ptr() for f in fbs]
    po, pd = [o.data_ptr() for o in occ], [d.data_ptr() for d in dep]
    pitch = W * 8

    def frame(kind, e):
        r.Sort(e[0], proj, vp, nf)
        if kind == "stereo_plain":
            r.RenderStereo(e, [proj, proj], vp, nf, out_ptrs=out, pitch_bytes=pitch)
        elif kind == "two_plain":
            for k in range(2):
                r.Render(e[k], proj, vp, nf, out_ptr=out[k], pitch_bytes=pitch)
        elif kind == "stereo_occ":
            r.RenderStereoLayers(e, [proj, proj], vp, nf, out_ptrs=out, pitch_bytes=pitch, occluder_ptrs=po)
        elif kind == "two_occ":
            for k in range(2):
                r.Render(e[k], proj, vp, nf, out_ptr=out[k], pitch_bytes=pitch, occluder_ptr=po[k])
        elif kind == "stereo_both":
            r.RenderStereoLayers(e, [proj, proj], vp, nf, out_ptrs=out, pitch_bytes=pitch, depth_ptrs=pd, occluder_ptrs=po)
        elif kind == "two_both":
            for k in range(2):
                r.RenderLayers(e[k], proj, vp, nf, out_ptr=out[k], pitch_bytes=pitch, depth_ptr=pd[k], occluder_ptr=po[k])
        elif kind == "mono_occ":
            r.Render(e[0], proj, vp, nf, out_ptr=out[0], pitch_bytes=pitch, occluder_ptr=po[0])
        elif kind == "mono_both":
            r.RenderLayers(e[0], proj, vp, nf, out_ptr=out[0], pitch_bytes=pitch, depth_ptr=pd[0], occluder_ptr=po[0])
        else:
            raise KeyError(kind)

    def block(kind, frames, start):
        t0 = time.perf_counter()
        for k in range(frames):
            frame(kind, eyes[(start + k) % 64])
        r.synchronize()
        return 1000.0 * (time.perf_counter() - t0) / frames

    kinds = args.kinds.split(",")
    for kind in kinds:
        block(kind, args.warmup, 0)
    ms = {kind: [] for kind in kinds}
    for i in range(args.rounds):
        for kind in (kinds if i % 2 == 0 else kinds[::-1]):          # alternating, and in alternating order
            ms[kind].append(block(kind, args.frames, 64 * i))
    r.close()
    print(json.dumps(dict(level=level, ms={k: [round(v, 4) for v in vs] for k, vs in ms.items()})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--parent-lib", default=None, help="another build of libmsplat.so (the parent commit's) to measure beside the tree's")
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kinds", default=",".join(KINDS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    runs = [("tree", None, KINDS)] + ([("parent", os.path.abspath(args.parent_lib), OLD_KINDS)] if args.parent_lib else [])
    results = {}
    for name, lib, kinds in runs:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--kinds", ",".join(kinds),
               "--frames", str(args.frames), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        env = dict(os.environ)
        env.pop("MSPLAT_LIB_PATH", None)
        if lib:
            env["MSPLAT_LIB_PATH"] = lib
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
        if p.returncode != 0:          # a failure, a fault or the time limit: nothing more is started
            print("the %s build's measurement ended with status %d: stopping" % (name, p.returncode), file=sys.stderr)
            sys.exit(p.returncode or 1)
        results[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print("%s: %s" % (name, results[name]), file=sys.stderr, flush=True)
    lines = ["| %s, serial frames | build | ms per frame (median of %d) | min .. max |" % (WORKLOAD["desc"], args.rounds), "|---|---|---|---|"]
    for name, _, kinds in runs:
        for kind in kinds:
            v = results[name]["ms"][kind]
            lines.append("| %s | %s | %.4f | %.4f .. %.4f |" % (kind, name, statistics.median(v), min(v), max(v)))
    text = "\n".join(lines) + "\n" + json.dumps({"layers_timing": results})
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
