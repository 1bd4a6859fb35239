#!/usr/bin/env python3
"""usage (GPU box): python tools/target_mode_timing.py [--frames 256] [--in-flight 4] [--out FILE]

What does reading the target cost the compositor?  BASELINE config 2 (1 M splats, 1920x1080 fp32, 64-step orbit), one frame at a
time and with frames in flight, in the three target modes of msplat_set_target_mode -- all in ONE process, on one renderer per
shape, the modes taking turns block by block so that clock and thermal drift hit them alike.  The number is the compositor
KERNEL's time (dispatch begin / end events, msplat_get_timings): a block is the frames between two reads of the timings (one
frame when serial, four per context in flight), a sample its mean, and the table shows the median / quartiles over the samples
of at least --frames frames per mode after a warm-up.  LOAD blends over the previous frame's pixels in the same framebuffer
(finite: every frame's alpha is 1 and T < 1 wherever a splat lands), which is what an integrator's frame loop does after it
has drawn its own geometry.  Prints a markdown table and one JSON line."""
import argparse
import json
import math
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splatapult_amd import SplatRenderer, camera, synthetic  # noqa: E402

MODES = ("clear", "load", "premultiplied")


def measure(cloud, W, H, P, frames, warmup):
    """{mode: [compositor kernel ms per block]} for P frames in flight (1 = one frame at a time)"""
    dev = torch.device("cuda:0")
    r = SplatRenderer(device=0, fb_format="fp32", frames_in_flight=P, enable_timing=1)
    assert r.Init(cloud, False, False), r.last_error()
    fbs = [torch.rand((((H + 31) // 32) * 32, W, 4), dtype=torch.float32, device=dev) for _ in range(P)]
    torch.cuda.synchronize()
    proj = camera.perspective(camera.FOVY, W / H)
    vp, nf = [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR]
    poses = [camera.orbit(7.0, 2.0 * math.pi * k / 64.0) for k in range(64)]
    block = 1 if P == 1 else 4 * P
    step = 0

    def run_block():
        nonlocal step
        for _ in range(block):
            c = poses[step % 64]
            step += 1
            r.Sort(c, proj, vp, nf)
            r.Render(c, proj, vp, nf, out_ptr=fbs[r.frame_slot].data_ptr(), pitch_bytes=W * 16)
        r.synchronize()
        return r.timings()["composite_kernel"]

    samples = {m: [] for m in MODES}
    for m in MODES:                      # warm-up: every mode's kernel has run, the pools have grown
        r.set_target_mode(m)
        for _ in range(max(1, warmup // block)):
            run_block()
    turns = 8                            # the modes take turns: `turns` rounds of frames / turns frames each
    per_turn = max(1, -(-frames // (turns * block)))
    for _ in range(turns):
        for m in MODES:
            r.set_target_mode(m)
            run_block()                  # (the first block after a switch is not kept)
            for _ in range(per_turn):
                samples[m].append(run_block())
    r.close()
    return samples, block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256, help="timed frames per mode and shape (at least 200 for a quotable table)")
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--in-flight", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    W, H = 1920, 1080
    cloud = synthetic.make_cloud(1_000_000, seed=0x5EED1234, full_sh=True, pos_sigma=1.5)
    lines = ["| shape | mode | compositor kernel, median (us) | quartiles (us) | vs clear | samples x frames |", "|---|---|---|---|---|---|"]
    result = {}
    for label, P in (("one frame at a time", 1), ("%d frames in flight" % args.in_flight, args.in_flight)):
        samples, block = measure(cloud, W, H, P, args.frames, args.warmup)
        base = float(np.median(samples["clear"]))
        for m in MODES:
            a = np.asarray(samples[m], np.float64) * 1e3
            q1, med, q3 = np.percentile(a, [25, 50, 75])
            lines.append("| %s | %s | %.1f | %.1f - %.1f | %+.1f %% | %d x %d |" % (label, m, med, q1, q3, 100.0 * (med / (base * 1e3) - 1.0), a.size, block))
            result["%s/%s" % ("serial" if P == 1 else "in_flight", m)] = dict(median_us=round(float(med), 2), q1_us=round(float(q1), 2),
                                                                             q3_us=round(float(q3), 2), frames=int(a.size * block))
    text = "\n".join(lines) + "\n" + json.dumps({"target_mode_timing": result})
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
