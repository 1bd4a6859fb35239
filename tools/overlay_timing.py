"""What the render-time overlay costs (msplat_set_overlay* / msplat_set_overlay_palette).

usage (GPU box, repo root):
    python tools/overlay_timing.py [--parent-lib LIB] [--frames 256] [--rounds 3] [--out FILE]

BASELINE config 2 (bench.py's cfg2: its 1 M-splat cloud, its 64-step orbit, 1920 x 1080 fp32), Sort + Render per frame into device
memory, timed by the host clock.  Every measurement is a child process under its own `timeout`; the first failure ends the run.
One JSON line per child on stdout (and appended to --out):

  frames   mode "serial" (one context, one synchronise per frame) and "flight4" (four frames in flight, one synchronise at the end):
           ms per frame of the plain frame on --parent-lib (a build of the parent commit, same ABI) and on this tree's library,
           the two alternating over --rounds; on this tree's library also with the overlay INACTIVE (classes set, a palette of
           a == 0 only: nothing may be launched or read that was not before) and ACTIVE with 0 %, 1 %, 50 % and 100 % of the splats
           in a class with a != 0 (0 %: the kernel runs and touches no record).  An active overlay is a one-pass frame; so are
           the serial frames of this workload, while with frames in flight two_pass = AUTO probes two passes now and then
           (two_pass_frames counts them; the pixels are the same).
  stage    serial frames with stage events on every frame (enable_timing): the projection stage of msplat_get_timings, which includes
           overlay_kernel, per share -- the kernel by difference against the inactive overlay.
A run without a GPU fails at the first context."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_TIMEOUT = 420
SHARES = (0.0, 0.01, 0.5, 1.0)


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def workload():
    import bench
    import math
    from splatapult_amd import camera
    wl = bench.WORKLOADS["cfg2"]
    W, H = wl["W"], wl["H"]
    proj = camera.perspective(camera.FOVY, W / H)
    views = [(camera.orbit(wl["cam_z"], 2.0 * math.pi * k / 64.0), proj, [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR]) for k in range(64)]
    return wl, W, H, views


def variants(r, n):
    """(name, set-up) per measured variant; the overlay ones exist where the library has the entry points"""
    import numpy as np
    yield "plain", lambda: None
    if not hasattr(r._lib, "msplat_set_overlay"):
        return
    rng = np.random.default_rng(7)
    pick = rng.random(n)
    tint = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 0.6, 0.1, 0.5]], np.float32)
    blank = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 0.6, 0.1, 0.0]], np.float32)
    yield "inactive", lambda: r.SetOverlay((pick < 0.5).astype(np.uint8), blank)
    for share in SHARES:
        yield "active_%g%%" % (100 * share), (lambda s=share: r.SetOverlay((pick < s).astype(np.uint8), tint))
    yield "plain_again", lambda: r.SetOverlay(None, None)


def child_frames(cloud_path, label, mode, frames, out):
    import bench  # noqa: F401  (sets the queue count before the HIP runtime starts, as bench.py does)
    import numpy as np
    import torch
    from splatapult_amd import SplatRenderer, _capi

    wl, W, H, views = workload()
    aos = np.load(cloud_path, mmap_mode="r")
    n = int(aos.shape[0])
    P = 4 if mode == "flight4" else 1
    r = SplatRenderer(device=0, frames_in_flight=P)
    if not r.Init(aos, False, False):
        raise SystemExit("Init failed: " + r.last_error())
    fbs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(P)]
    torch.cuda.synchronize()

    def run(count):
        t0 = time.perf_counter()
        for k in range(count):
            v = views[k % len(views)]
            r.Sort(*v)
            r.Render(*v, out_ptr=fbs[k % P].data_ptr())
            if P == 1:
                r.synchronize()
        r.synchronize()
        return 1e3 * (time.perf_counter() - t0) / count

    line = {"tool": "overlay_timing", "kind": "frames", "mode": mode, "library": label, "lib_path": _capi.LIB_PATH, "splats": n, "frames": frames,
            "ms_per_frame": {}}
    run(128)                                                # every pose twice: code objects, the pair buffer's growth
    for name, setup in variants(r, n):
        setup()
        run(64)
        line["ms_per_frame"][name] = min(run(frames) for _ in range(3))
    line["two_pass_frames"] = r.two_pass_state()[0]
    emit(line, out)
    r.close()


def child_stage(cloud_path, frames, out):
    import bench  # noqa: F401
    import numpy as np
    import torch
    from splatapult_amd import SplatRenderer, _capi

    wl, W, H, views = workload()
    aos = np.load(cloud_path, mmap_mode="r")
    n = int(aos.shape[0])
    r = SplatRenderer(device=0, enable_timing=True)
    if not r.Init(aos, False, False):
        raise SystemExit("Init failed: " + r.last_error())
    fb = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def run(count):
        for k in range(count):
            v = views[k % len(views)]
            r.Sort(*v)
            r.Render(*v, out_ptr=fb.data_ptr())
            r.synchronize()

    line = {"tool": "overlay_timing", "kind": "stage", "library": "tree", "lib_path": _capi.LIB_PATH, "splats": n, "frames": frames,
            "project_ms": {}, "render_ms": {}}
    run(128)
    for name, setup in variants(r, n):
        setup()
        run(64)
        r.timings()
        run(frames)
        t = r.timings()
        line["project_ms"][name], line["render_ms"][name] = t["project"], t["render_total"]
    base = line["project_ms"].get("inactive")
    if base is not None:
        line["overlay_kernel_us_by_difference"] = {k: 1e3 * (v - base) for k, v in line["project_ms"].items() if k.startswith("active")}
    emit(line, out)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libmsplat.so built from the parent commit (same ABI), measured beside the tree's")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        if args.child[0] == "stage":
            child_stage(args.child[1], args.frames, args.out)
        else:
            child_frames(args.child[1], args.child[2], args.child[3], args.frames, args.out)
        return

    def spawn(child, lib=None):
        env = dict(os.environ)
        env.pop("MSPLAT_LIB_PATH", None)
        if lib:
            env["MSPLAT_LIB_PATH"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--frames", str(args.frames), "--child"] + child
        if args.out:
            cmd += ["--out", args.out]
        rc = subprocess.run(cmd, cwd=ROOT, env=env).returncode
        if rc != 0:
            raise SystemExit("child %s ended with status %d: nothing more is started" % (child, rc))

    # the workload's cloud, built once (host only) and shared with the children through a file
    import numpy as np
    import bench
    from splatapult_amd import synthetic
    wl = bench.WORKLOADS["cfg2"]
    cloud = synthetic.make_cloud(wl["n"], seed=wl["seed"], full_sh=True, pos_sigma=wl["pos_sigma"])
    tmp = tempfile.mkdtemp(prefix="msplat_ov_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = os.path.join(tmp, "cloud.npy")
    try:
        np.save(path, np.ascontiguousarray(cloud.as_array(), np.float32))
        del cloud
        for _ in range(args.rounds):
            for mode in ("serial", "flight4"):
                if args.parent_lib:
                    spawn(["frames", path, "parent", mode], args.parent_lib)
                spawn(["frames", path, "tree", mode])
        spawn(["stage", path])
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
