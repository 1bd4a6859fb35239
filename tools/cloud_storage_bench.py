"""FP32 against SH_FP16 and SH_Q8 cloud storage (msplat_set_cloud_storage) under bench.py's own protocol.

usage (GPU box, repo root):
    python tools/cloud_storage_bench.py [--workloads cfg2,cfg3,cfg4,cfg5] [--storages fp32,sh_fp16,sh_q8] [--steps 20]
                                        [--warmup 200] [--plain] [--out FILE]

Every (workload, storage) runs `bench.py --gpus 1 --workload W --steps S --warmup K --full --no-cpu-baseline` in a child process
(four frames in flight, cu_partition auto, median of S-frame blocks, the serial phase) with the renderer's cloud_storage default
set to the storage under test: bench.py itself is imported, not edited.  A second child renders the workload's first view with
FP32 storage of C and, per compact storage, with that storage of C and with FP32 storage of the cloud it stands for -- round16(C)
(f_rest rounded to fp16) for SH_FP16, deq(C) (tests/sh_q8_rule.py: f_rest = code * step) for SH_Q8 -- and reports whether the
last two agree bit for bit (`bit_exact`) and max|pixel difference| against FP32 storage of C (`max|diff|`).
One JSON line per (workload, storage) on stdout (and appended to --out).

Child modes (also what a profiler wraps: rocprofv3 ... -- python tools/cloud_storage_bench.py --child sh_fp16 -- <bench args>):
    --child STORAGE -- <bench.py arguments>       one bench.py run with that storage
    --check WORKLOAD [STORAGES]                   the render check of one workload
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# f_rest columns of the reference record (61 floats)
REST = [5, 6, 7, 9, 10, 11, 13, 14, 15] + list(range(25, 61))


def run_child_bench(storage, bench_args):
    import bench                                    # (sets GPU_MAX_HW_QUEUES before the HIP runtime starts, as bench.py does)
    import splatapult_amd
    base = splatapult_amd.SplatRenderer

    class StorageRenderer(base):
        def __init__(self, *a, **kw):
            kw.setdefault("cloud_storage", storage)
            super().__init__(*a, **kw)

    splatapult_amd.SplatRenderer = StorageRenderer     # bench.measure imports it from the package at call time
    sys.argv = [os.path.join(ROOT, "bench.py")] + bench_args
    return bench.main()


LABELS = {"fp32": ("fp32", None), "sh_fp16": ("SH fp16", "f32 (SH storage fp16)"), "sh_q8": ("SH q8", "f32 (SH storage q8)")}


def run_check(key, storages):
    import bench
    import numpy as np
    from splatapult_amd import SplatRenderer, camera, synthetic
    from tests.sh_q8_rule import deq

    wl = bench.WORKLOADS[key]
    aos = synthetic.make_cloud(wl["n"], seed=wl["seed"], full_sh=True, pos_sigma=wl["pos_sigma"]).as_array()

    def round16(a):
        out = a.copy()
        out[:, REST] = a[:, REST].astype(np.float16).astype(np.float32)
        return out

    stands_for = {"sh_fp16": round16, "sh_q8": deq}
    W, H = wl["W"], wl["H"]
    proj = camera.perspective(camera.FOVY, W / H)
    vp, nf = [0, 0, W, H], [camera.Z_NEAR, camera.Z_FAR]
    cams = [camera.pose((0.0, 0.0, wl["cam_z"]), 0.3)] if wl["views"] == 1 else \
        [camera.pose((-0.032, 0.0, wl["cam_z"]), 0.3), camera.pose((0.032, 0.0, wl["cam_z"]), 0.3)]

    def render(storage, a):
        r = SplatRenderer(device=0, fb_format=wl["fb"], cloud_storage=storage)
        if not r.Init(a, False, False):
            raise SystemExit("Init failed: " + r.last_error())
        r.Sort(cams[0], proj, vp, nf)
        out = [r.Render(c, proj, vp, nf) for c in cams]
        r.close()
        return out

    u = (lambda x: x.view(np.uint16 if x.dtype == np.float16 else np.uint32))
    ref = render("fp32", aos)
    res = {"workload": key}
    for storage in storages:
        if storage == "fp32":
            continue
        got, want = render(storage, aos), render("fp32", stands_for[storage](aos))
        exact = all(np.array_equal(u(a), u(b)) for a, b in zip(got, want))
        diff = max(float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) for a, b in zip(got, ref))
        res[storage] = {"bit_exact": bool(exact), "max|diff|": diff}
    print(json.dumps(res))


def last_json(text):
    for line in reversed(text.splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    return None


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        args = sys.argv[3:]
        return run_child_bench(sys.argv[2], args[1:] if args[:1] == ["--"] else args)
    if len(sys.argv) > 2 and sys.argv[1] == "--check":
        return run_check(sys.argv[2], (sys.argv[3] if len(sys.argv) > 3 else "sh_fp16").split(","))
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg2,cfg3,cfg4,cfg5")
    ap.add_argument("--storages", default="fp32,sh_fp16,sh_q8")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--plain", action="store_true", help="bench.py's plain run (one timed block, no serial phase) instead of --full")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child process")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    me = os.path.abspath(__file__)
    for key in [k for k in args.workloads.split(",") if k]:
        chk = subprocess.run([sys.executable, me, "--check", key, args.storages], cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
        check = last_json(chk.stdout)
        if chk.returncode != 0 or check is None:
            sys.stderr.write(chk.stdout[-3000:] + chk.stderr[-3000:])
            raise SystemExit("check of %s failed (exit %d)" % (key, chk.returncode))
        for storage in [s for s in args.storages.split(",") if s]:
            bargs = ["--gpus", "1", "--workload", key, "--steps", str(args.steps), "--warmup", str(args.warmup)]
            if not args.plain:
                bargs += ["--full", "--no-cpu-baseline"]
            p = subprocess.run([sys.executable, me, "--child", storage, "--"] + bargs, cwd=ROOT, capture_output=True, text=True,
                               timeout=args.timeout)
            out = last_json(p.stdout)
            if p.returncode != 0 or out is None:
                sys.stderr.write(p.stdout[-3000:] + p.stderr[-3000:])
                raise SystemExit("bench.py child for %s / %s failed (exit %d)" % (key, storage, p.returncode))
            cfg = out.setdefault("config", {})
            label, dtype = LABELS[storage]
            cfg["workload"] = cfg.get("workload", key) + " [cloud storage: %s]" % label
            if storage != "fp32":
                out["dtype"] = dtype
                out["bit_exact"] = check[storage]["bit_exact"]
                out["max|diff|"] = check[storage]["max|diff|"]
            else:
                out["bit_exact"] = True                  # (the reference itself)
                out["max|diff|"] = 0.0
            out["cloud_storage"] = storage
            line = json.dumps(out)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
