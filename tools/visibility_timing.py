"""What per-splat visibility costs and saves (msplat_set_visibility / msplat_set_crop).

usage (GPU box, repo root):
    python tools/visibility_timing.py [--parent-lib LIB] [--frames 100] [--rounds 3] [--sizes 1000000,6000000] [--out FILE]

Two kinds of measurement, every one a child process under its own `timeout`; the first failure ends the run.  One JSON line per
child on stdout (and appended to --out):

  kernel   visibility_kernel at each of --sizes (synthetic clouds, SH degree 0, stored in upload order and in Morton order): the
           context's sort_total (stream events around msplat_sort's launches, enable_timing) of a Sort that starts with the kernel
           -- the crop or the mask was set just before -- and of the next Sort, which does not; the difference of the medians is
           the kernel plus its 4-byte memset.  Bytes from the shapes: 16 read + 16 written per splat, + 1 with a mask, + 4 with a
           mask on a Morton-ordered store.  A difference of two event spans carries both spans' noise: the spread is printed.
  frames   the scene-like 6 M workload of bench.py (cfg3s: its cloud, its 64 cameras, 1920 x 1080, serial frames, one
           synchronise per frame): ms per frame by the host clock and sort_total by stream events, uncropped, on --parent-lib (a
           build of the parent commit, same ABI) and on this tree's library, the two alternating over --rounds; on this tree's also
           with a sphere crop around the first camera that keeps ~10 % of the splats.  The claim to check: the uncropped Sort and
           frame cost the same on both libraries (nothing is launched or read that was not before).
A run without a GPU fails at the first context."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
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


def spread(v):
    import numpy as np
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def sphere(centre, radius):
    """world -> crop: the sphere becomes the unit sphere"""
    import numpy as np
    s = 1.0 / radius
    m = np.diag([s, s, s, 1.0])
    m[:3, 3] = -np.asarray(centre, np.float64) * s
    return np.ascontiguousarray(m.T.reshape(16), np.float32)


def child_kernel(n, out):
    import bench  # noqa: F401  (sets the queue count before the HIP runtime starts, as bench.py does)
    import numpy as np
    from splatapult_amd import SplatRenderer, _capi, camera, synthetic
    from splatapult_amd.scene import GaussianCloud

    a = synthetic.generate(n, seed=0x5EED1234, full_sh=False, pos_sigma=1.5)
    gc = GaussianCloud(GaussianCloud.Options(False, False))
    if not gc.FromAttributes(a["xyz"], a["f_dc"], None, a["opacity"], a["log_scale"], a["rot"]):
        raise SystemExit("FromAttributes failed")
    aos = np.ascontiguousarray(gc.as_array(), np.float32)
    W, H = 1920, 1080
    view = (camera.pose((0.0, 0.0, 7.0)), camera.perspective(camera.FOVY, W / H), [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR])
    dist = np.linalg.norm(a["xyz"].astype(np.float64), axis=1)
    M = sphere((0.0, 0.0, 0.0), float(np.quantile(dist, 0.10)))
    mask = np.random.default_rng(1).random(n) < 0.10
    for spatial, sname in ((_capi.SPATIAL_OFF, "upload"), (_capi.SPATIAL_ON, "morton")):
        r = SplatRenderer(device=0, spatial_order=spatial, enable_timing=True)
        if not r.Init(aos, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        for kind in ("crop", "mask"):
            with_kernel, without = [], []
            for k in range(44):
                if kind == "crop":
                    r.SetCrop(M, "sphere")
                else:
                    r.SetVisibility(mask)
                for dst in (with_kernel, without):
                    r.Sort(*view)
                    r.synchronize()
                    t = _capi.Timings()             # (SplatRenderer.timings() weights by rendered frames: there are none here)
                    _capi.check(r._ctx, r._lib.msplat_get_timings(r._ctx, C.byref(t)))
                    ms = float(t.sort_total)
                    if k >= 4:                          # (the first rounds warm up: code objects, the listed pass 0)
                        dst.append(ms)
            hidden = r.visibility()["hidden"]
            nbytes = n * (32 + (1 if kind == "mask" else 0) + (4 if kind == "mask" and sname == "morton" else 0))
            d = float(np.median(with_kernel) - np.median(without))
            emit({"tool": "visibility_timing", "kind": "kernel", "splats": n, "storage_order": sname, "what": kind, "hidden": hidden,
                  "sort_ms_with_visibility_kernel": spread(with_kernel), "sort_ms_without": spread(without),
                  "visibility_kernel_ms_by_difference": d, "bytes": nbytes, "GBps": (nbytes / (d * 1e-3) / 1e9) if d > 0 else None}, out)
            r.SetCrop(None)
            r.SetVisibility(None)
        r.close()


def child_frames(cloud_path, label, frames, out):
    import bench
    import numpy as np
    import torch
    from splatapult_amd import SplatRenderer, _capi, camera, synthetic

    wl = bench.WORKLOADS["cfg3s"]
    W, H = wl["W"], wl["H"]
    aos = np.load(cloud_path, mmap_mode="r")
    cams = synthetic.scene_cameras(64)
    proj = camera.perspective(camera.FOVY, W / H)
    views = [(c, proj, [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR]) for c in cams]
    r = SplatRenderer(device=0, enable_timing=True)
    if not r.Init(aos, False, False):
        raise SystemExit("Init failed: " + r.last_error())
    fb = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def run(count):
        t0 = time.perf_counter()
        for k in range(count):
            v = views[k % len(views)]
            r.Sort(*v)
            r.Render(*v, out_ptr=fb.data_ptr())
            r.synchronize()
        return 1e3 * (time.perf_counter() - t0) / count

    def measure():
        run(64)                                         # every pose once: code objects, the pair buffer's growth, the listed pass 0
        r.timings()
        ms = run(frames)
        return {"frame_ms": ms, "sort_ms": r.timings()["sort_total"], "sort_count_last": r.sort_count()}

    line = {"tool": "visibility_timing", "kind": "frames", "library": label, "lib_path": _capi.LIB_PATH, "splats": int(aos.shape[0]),
            "frames": frames, "uncropped": measure()}
    if hasattr(_capi.lib(), "msplat_set_crop"):
        eye = np.asarray(cams[0], np.float32).reshape(16)[12:15]
        dist = np.linalg.norm(np.asarray(aos[:, 0:3], np.float64) - eye, axis=1)
        r.SetCrop(sphere(eye, float(np.quantile(dist, 0.10))), "sphere")
        line["cropped_10_percent"] = measure()
        line["cropped_10_percent"]["hidden"] = r.visibility()["hidden"]
        r.SetCrop(None)
        line["uncropped_again"] = measure()
    emit(line, out)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libmsplat.so built from the parent commit (same ABI), measured beside the tree's")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-frames", action="store_true")
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        if args.child[0] == "kernel":
            child_kernel(int(args.child[1]), args.out)
        else:
            child_frames(args.child[1], args.child[2], args.frames, args.out)
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

    for n in [int(s) for s in args.sizes.split(",") if s]:
        spawn(["kernel", str(n)])
    if args.skip_frames:
        return
    # the workload's cloud, built once (host only) and shared with the children through a file
    import numpy as np
    import bench
    from splatapult_amd import synthetic
    from splatapult_amd.scene import GaussianCloud
    wl = bench.WORKLOADS["cfg3s"]
    a = synthetic.generate_scene(wl["n"], seed=wl["seed"])
    gc = GaussianCloud(GaussianCloud.Options(True, True))
    if not gc.FromAttributes(a["xyz"], a["f_dc"], a["f_rest"], a["opacity"], a["log_scale"], a["rot"]):
        raise SystemExit("FromAttributes failed")
    tmp = tempfile.mkdtemp(prefix="msplat_vis_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = os.path.join(tmp, "cloud.npy")
    try:
        np.save(path, np.ascontiguousarray(gc.as_array(), np.float32))
        del a, gc
        for _ in range(args.rounds):
            if args.parent_lib:
                spawn(["frames", path, "parent"], args.parent_lib)
            spawn(["frames", path, "tree"])
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
