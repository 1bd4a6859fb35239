"""What an id frame costs (msplat_render_ids) beside the Render of the same context.

usage (GPU box, repo root):
    python tools/ids_timing.py [--parent-lib LIB] [--frames 200] [--rounds 3] [--out FILE]

Serial frames at BASELINE config 2 (bench.py's cfg2: 1 M synthetic splats, 1920 x 1080 fp32, the 64-step orbit), device output, one
synchronise per frame, the host clock around `frames` frames after every pose has run once.  Every measurement is a child process
under its own `timeout`; the first failure ends the run.  One JSON line per child on stdout (and appended to --out):

  tree     this tree's library, one Sort per pose kept out of the timed window (the three frames draw the same Sort):
             render_ms     msplat_render
             ids_ms        msplat_render_ids over the whole viewport, both planes
             pick_ms       msplat_render_ids through a 1 x 1 window in the middle of the viewport (the projection and the binning
                           of the whole frame, the id kernel over one tile)
           and, from the context's stream events (enable_timing) of the Renders alone, their project / binning / composite split:
           ids_ms - (project + binning) can be read against the compositor's time.
  parent   --parent-lib (a build of the parent commit, same ABI): render_ms only, alternating with `tree` over --rounds.  The
           claim to check: render_ms is the same on both.
A run without a GPU fails at the first context."""
import argparse
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


def child(label, frames, out):
    import bench
    import torch
    from splatapult_amd import SplatRenderer, _capi, camera, synthetic

    wl = bench.WORKLOADS["cfg2"]
    W, H = wl["W"], wl["H"]
    cloud = synthetic.make_cloud(wl["n"], seed=wl["seed"], full_sh=True, pos_sigma=wl["pos_sigma"])
    proj = camera.perspective(camera.FOVY, W / H)
    views = [(camera.orbit(wl["cam_z"], 2.0 * math.pi * k / 64.0), proj, [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR]) for k in range(64)]
    r = SplatRenderer(device=0, frame_mode=_capi.FRAMES_SERIAL, enable_timing=True)
    if not r.Init(cloud, False, False):
        raise SystemExit("Init failed: " + r.last_error())
    fb = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    ids = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
    zw = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    has_ids = hasattr(_capi.lib(), "msplat_render_ids")
    pick = (W // 2, H // 2, 1, 1)
    kinds = {"render_ms": lambda v: r.Render(*v, out_ptr=fb.data_ptr())}
    if has_ids:
        kinds["ids_ms"] = lambda v: r.RenderIds(*v, out_ptr=ids.data_ptr(), depth_ptr=zw.data_ptr())
        kinds["pick_ms"] = lambda v: r.RenderIds(*v, window=pick, out_ptr=ids.data_ptr(), depth_ptr=zw.data_ptr())

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

    line = {"tool": "ids_timing", "library": label, "lib_path": _capi.LIB_PATH, "splats": wl["n"], "viewport": [W, H], "frames": frames}
    for name, call in kinds.items():
        run(call, 64)                                   # every pose once: code objects, the pair buffer's growth
        r.timings()
        line[name] = run(call, frames)
        if name == "render_ms":
            t = r.timings()
            line["render_stages_ms"] = {k: t[k] for k in ("render_total", "project", "binning", "composite", "composite_kernel")}
    emit(line, out)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libmsplat.so built from the parent commit (same ABI), measured beside the tree's")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.frames, args.out)
        return

    def spawn(label, lib=None):
        env = dict(os.environ)
        env.pop("MSPLAT_LIB_PATH", None)
        if lib:
            env["MSPLAT_LIB_PATH"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--frames", str(args.frames), "--child", label]
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
