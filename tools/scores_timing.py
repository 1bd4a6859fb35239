"""What a score frame costs (msplat_render_scores) beside the id frame and the Render of the same context.

usage (GPU box, repo root):
    python tools/scores_timing.py [--config cfg2|sparse] [--parent-lib LIB] [--frames 200] [--rounds 3] [--out FILE]

Serial frames, device output, one synchronise per frame, the host clock around `frames` frames after every pose has run once.
--config cfg2: BASELINE config 2 (bench.py's cfg2: 1 M synthetic splats, 1920 x 1080 fp32, the 64-step orbit); sparse: the 20 k-splat,
517 x 293 view the tests use.  Every measurement is a child process under its own `timeout`; the first failure ends the run.  One
JSON line per child on stdout (and appended to --out):

  tree     this tree's library, one Sort per pose kept out of the timed window (the four frames draw the same Sort):
             render_ms          msplat_render
             ids_ms             msplat_render_ids over the whole viewport, both planes
             scores_ms          msplat_render_scores over the whole viewport, d_pixels == NULL
             scores_pixels_ms   the same with the hit counts
           The arrays are accumulated into across the frames (zeroing them is the caller's, and not part of the frame).
  parent   --parent-lib (a build of the parent commit, same ABI): render_ms and ids_ms, alternating with `tree` over --rounds.  The
           claim to check: both are the same on both.
A run without a GPU fails at the first context."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_TIMEOUT = 420


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def workload(config):
    """(cloud, W, H, views)"""
    import bench
    from splatapult_amd import camera, synthetic
    nf = [camera.Z_NEAR, camera.Z_FAR]
    if config == "sparse":
        W, H = 517, 293
        cloud = synthetic.make_cloud(20000, seed=302, full_sh=True, log_scale_mean=-4.2)
        return cloud, W, H, [(camera.pose((0.0, 0.0, 7.0)), camera.perspective(camera.FOVY, W / H), [0, 0, W, H], nf)]
    wl = bench.WORKLOADS["cfg2"]
    W, H = wl["W"], wl["H"]
    cloud = synthetic.make_cloud(wl["n"], seed=wl["seed"], full_sh=True, pos_sigma=wl["pos_sigma"])
    proj = camera.perspective(camera.FOVY, W / H)
    return cloud, W, H, [(camera.orbit(wl["cam_z"], 2.0 * math.pi * k / 64.0), proj, [0, 0, W, H], nf) for k in range(64)]


def child(label, config, frames, out):
    import torch
    from splatapult_amd import SplatRenderer, _capi

    cloud, W, H, views = workload(config)
    r = SplatRenderer(device=0, frame_mode=_capi.FRAMES_SERIAL)
    if not r.Init(cloud, False, False):
        raise SystemExit("Init failed: " + r.last_error())
    n = r._n
    fb = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    ids = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
    zw = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    score = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    hits = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    L = _capi.lib()

    def scores(v, d_pixels):
        _capi.check(r._ctx, L.msplat_render_scores(r._ctx, *r._args.load(*v), None, None, 0, C.c_void_p(score.data_ptr()), d_pixels, n))

    kinds = {"render_ms": lambda v: r.Render(*v, out_ptr=fb.data_ptr())}
    if hasattr(L, "msplat_render_ids"):
        kinds["ids_ms"] = lambda v: r.RenderIds(*v, out_ptr=ids.data_ptr(), depth_ptr=zw.data_ptr())
    if hasattr(L, "msplat_render_scores"):
        kinds["scores_ms"] = lambda v: scores(v, None)
        kinds["scores_pixels_ms"] = lambda v: scores(v, C.c_void_p(hits.data_ptr()))

    def run(call, count):
        spent = 0.0
        for k in range(count):
            v = views[k % len(views)]
            r.Sort(*v)
            r.synchronize()
            t0 = time.perf_counter()
            call(v)
            r.synchronize()
            spent += time.perf_counter() - t0
        return 1e3 * spent / count

    line = {"tool": "scores_timing", "config": config, "library": label, "lib_path": _capi.LIB_PATH, "splats": n, "viewport": [W, H],
            "frames": frames}
    for name, call in kinds.items():
        run(call, 64)                                   # every pose once: code objects, the pair buffer's growth
        line[name] = run(call, frames)
    line["scored_splats"] = int((score != 0).sum())
    emit(line, out)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=("cfg2", "sparse"))
    ap.add_argument("--parent-lib", default=None, help="libmsplat.so built from the parent commit (same ABI), measured beside the tree's")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.config, args.frames, args.out)
        return

    def spawn(label, lib=None):
        env = dict(os.environ)
        env.pop("MSPLAT_LIB_PATH", None)
        if lib:
            env["MSPLAT_LIB_PATH"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--config", args.config,
               "--frames", str(args.frames), "--child", label]
        if args.out:
            cmd += ["--out", args.out]
        rc = subprocess.run(cmd, cwd=ROOT, env=env).returncode
        if rc != 0:
            raise SystemExit("child %s ended with status %d: nothing more is started" % (label, rc))

    for _ in range(args.rounds):
        if args.parent_lib:
            spawn("parent", args.parent_lib)
        spawn("tree")


if __name__ == "__main__":
    main()
