#!/usr/bin/env python3
"""usage (GPU box): python tools/fb8_timing.py [--parent-lib PATH/libmsplat.so] [--frames 256] [--in-flight 4] [--out FILE]

What does an 8-bit render target buy on one GPU, and did the fp32 frame change?  On BASELINE config 2 (1 M splats, 1920x1080, 64-step
orbit) and on the 6 M / 1080p workload rendered in two passes (msplat_config.two_pass = ON), one frame at a time and with frames in
flight, msplat_render into device memory:
  (a) the fp32 frame of the PARENT commit's library (--parent-lib: a libmsplat.so built from the parent; skipped without it),
  (b) the fp32 frame of this tree's library,
  (c) MSPLAT_FB_RGBA8, (d) MSPLAT_FB_SRGB8_ALPHA8 of this tree's library.
Every measurement is a child process of its own (MSPLAT_LIB_PATH selects the library) under its own `timeout`; the first child that
fails, faults or runs out of time ends the run -- nothing more is started on the GPU after it.  The number is frames per second of
Sort + Render over --frames frames after a warm-up, wall clock around a synchronised block, best of three blocks.
(b) against (a) has to lie inside the pool's box-to-box spread (README: 2-3 %); (c) and (d) against (b) are reported, not gated: the
framebuffer is 33 MB of about 620 MB of traffic per config-2 frame, so little is to be expected on one GPU -- the bytes saved are the
gather's, which one GPU cannot measure.
Prints a markdown table and one JSON line."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {
    "cfg2": dict(n=1_000_000, seed=0x5EED1234, pos_sigma=1.5, cam_z=7.0, two_pass=False, desc="1 M splats, 1920x1080 (BASELINE config 2)"),
    "6m": dict(n=6_000_000, seed=0x5EED6000, pos_sigma=3.0, cam_z=12.0, two_pass=True, desc="6 M splats, 1920x1080, two-pass frames"),
}
W, H = 1920, 1080


def worker(args):
    """one measurement in this process: prints one JSON line"""
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    import torch
    sys.path.insert(0, ROOT)
    from splatapult_amd import SplatRenderer, _capi, camera, synthetic
    wl = WORKLOADS[args.workload]
    P = args.in_flight
    cloud = synthetic.make_cloud(wl["n"], seed=wl["seed"], full_sh=True, pos_sigma=wl["pos_sigma"])
    r = SplatRenderer(device=0, fb_format=args.kind, frames_in_flight=P, two_pass=_capi.TWO_PASS_ON if wl["two_pass"] else _capi.TWO_PASS_AUTO)
    assert r.Init(cloud, False, False), r.last_error()
    dev = torch.device("cuda:0")
    tdt = torch.float32 if args.kind == "fp32" else torch.uint8
    fbs = [torch.zeros((H, W, 4), dtype=tdt, device=dev) for _ in range(P)]
    pitch = W * 4 * fbs[0].element_size()
    torch.cuda.synchronize()
    proj = camera.perspective(camera.FOVY, W / H)
    vp, nf = [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR]
    poses = [camera.orbit(wl["cam_z"], 2.0 * math.pi * k / 64.0) for k in range(64)]

    def block(frames, start):
        t0 = time.perf_counter()
        for k in range(frames):
            c = poses[(start + k) % 64]
            r.Sort(c, proj, vp, nf)
            s = r.frame_slot
            r.Render(c, proj, vp, nf, out_ptr=fbs[s].data_ptr(), pitch_bytes=pitch)
        r.synchronize()
        return frames / (time.perf_counter() - t0)

    block(args.warmup, 0)
    fps = [block(args.frames, 64 * i) for i in range(3)]
    two_pass_frames = r.two_pass_state()[0]
    r.close()
    print(json.dumps(dict(workload=args.workload, kind=args.kind, in_flight=P, fps=max(fps), blocks=[round(f, 1) for f in fps],
                          two_pass_frames=int(two_pass_frames), lib=os.environ.get("MSPLAT_LIB_PATH") or "in-tree")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libmsplat.so built from the parent commit: measurement (a)")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a single measurement may take")
    ap.add_argument("--workloads", default="cfg2,6m")
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--workload", default="cfg2", help=argparse.SUPPRESS)
    ap.add_argument("--kind", default="fp32", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    legs = [("b", "fp32", None), ("c", "rgba8", None), ("d", "srgb8", None)]
    if args.parent_lib:
        legs.insert(0, ("a", "fp32", os.path.abspath(args.parent_lib)))
    else:
        print("no --parent-lib: measurement (a) is skipped", file=sys.stderr)
    results = {}
    lines = ["| workload | frames in flight | (a) parent, fp32 (frames/s) | (b) fp32 | (c) RGBA8 | (d) SRGB8_ALPHA8 | (b)/(a) | (c)/(b) | (d)/(b) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for wl in args.workloads.split(","):
        for P in (1, args.in_flight):
            row = {}
            for leg, kind, lib in legs:
                env = dict(os.environ)
                env.pop("MSPLAT_LIB_PATH", None)
                if lib:
                    env["MSPLAT_LIB_PATH"] = lib
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--workload", wl,
                       "--kind", kind, "--in-flight", str(P), "--frames", str(args.frames), "--warmup", str(args.warmup)]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
                if p.returncode != 0:          # a failure, a fault or the time limit: nothing more is started
                    print("measurement (%s) %s P=%d ended with status %d: stopping" % (leg, wl, P, p.returncode), file=sys.stderr)
                    sys.exit(p.returncode or 1)
                row[leg] = json.loads(p.stdout.strip().splitlines()[-1])
                print("(%s) %s P=%d: %s" % (leg, wl, P, row[leg]), file=sys.stderr, flush=True)
            fa = row["a"]["fps"] if "a" in row else None
            fb, fc, fd = row["b"]["fps"], row["c"]["fps"], row["d"]["fps"]
            lines.append("| %s | %d | %s | %.1f | %.1f | %.1f | %s | %.3f | %.3f |" % (
                WORKLOADS[wl]["desc"], P, "%.1f" % fa if fa else "-", fb, fc, fd, "%.3f" % (fb / fa) if fa else "-", fc / fb, fd / fb))
            results["%s/P%d" % (wl, P)] = row
    text = "\n".join(lines) + "\n" + json.dumps({"fb8_timing": results})
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
