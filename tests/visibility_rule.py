"""What the visibility tests share (numpy only; no device, no torch): the crop rule of include/msplat.h restated in numpy float32 in
the header's operation order, its float64 form, the crop matrices and the centres placed on and just outside the surfaces, the mask
cases, and the clouds and the view.  Nothing here is measured: the tests compare a masked or cropped context with a context that was
uploaded the visible splats only."""
import functools

import numpy as np

from tests import scenes

F = np.float32
W, H = 256, 160
SIZES = (255, 256, 257, 4097)            # one box short of a splat, one box, one box and a splat, 17 boxes (the last holds one splat)
BOX = 256                                # kBoxSplats: stored splats per cull box and per workgroup of visibility_kernel
N_CROP = 4097
TIE_FREE = (4097, 24)                    # (n, seed) of a cloud whose keys are pairwise distinct in view(): most seeds have a tie or two (tests/test_visibility.py)


def view():
    return scenes.default_view(W, H, z=7.0, yaw=0.2)


@functools.lru_cache(maxsize=None)
def cloud_aos(n, seed=21):
    """(n, 61) float32 records of a synthetic cloud, read-only"""
    aos = np.ascontiguousarray(scenes.synth_cloud(n, seed, log_scale_mean=-3.0).as_array()[:n], F)
    aos.setflags(write=False)
    return aos


# ---- the crop rule ----------------------------------------------------------------------------------------------------------

def crop_q(xyz, M, dtype=F):
    """q = M (x, y, z, 1), rows 0..2, as msplat.h states it: ((M[0] x + M[4] y) + M[8] z) + M[12], every operation in `dtype`"""
    M = np.asarray(M, dtype).reshape(16)
    x, y, z = (np.asarray(xyz)[:, k].astype(dtype) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        return [((M[r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r] for r in range(3)]


def crop(xyz, M, shape, invert=False, dtype=F):
    """bool per centre: the splat takes part under msplat_set_crop(M, shape | invert).  A NaN centre is never inside"""
    qx, qy, qz = crop_q(xyz, M, dtype)
    one = dtype(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        if shape == "sphere":
            inside = (qx * qx + qy * qy) + qz * qz <= one
        else:
            assert shape == "box", shape
            inside = (np.abs(qx) <= one) & (np.abs(qy) <= one) & (np.abs(qz) <= one)
    return ~inside if invert else inside


def surface_distance(xyz, M, shape):
    """float64: how far each centre is from the crop surface, in crop-space units (|q| - 1 per axis for the box, |q|^2 - 1)"""
    qx, qy, qz = crop_q(xyz, M, np.float64)
    if shape == "sphere":
        return np.abs(qx * qx + qy * qy + qz * qz - 1.0)
    return np.minimum(np.minimum(np.abs(np.abs(qx) - 1.0), np.abs(np.abs(qy) - 1.0)), np.abs(np.abs(qz) - 1.0))


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def matrices():
    """name -> float32[16], column-major world -> crop.  identity and scaled: q is exact for every float32 centre (a power of two
    per axis, no translation); rotated: a rotation, a shear, a scale and a translation -- q is rounded"""
    ident = np.eye(4)
    scaled = np.diag([0.5, 0.25, 1.0, 1.0])
    A = _rotation((1.0, 2.0, 0.5), 0.7) @ np.array([[1.0, 0.3, 0.0], [0.0, 1.0, -0.2], [0.0, 0.0, 1.0]]) * 0.45
    rotated = np.eye(4)
    rotated[:3, :3], rotated[:3, 3] = A, (0.21, -0.13, 0.32)
    return {k: np.ascontiguousarray(m.T.reshape(16), F) for k, m in (("identity", ident), ("scaled", scaled), ("rotated", rotated))}


def on_surface(name):
    """(centres ON the surface, the same centres moved one float outward) of box and sphere under matrices()[name], name =
    "identity" or "scaled": axis points of the sphere are face points of the box; q is exact, so `on` is inside and `out` is not"""
    sx, sy = (1.0, 1.0) if name == "identity" else (2.0, 4.0)        # q = 1 at x = sx, y = sy, z = 1
    on = np.array([[sx, 0, 0], [-sx, 0, 0], [0, sy, 0], [0, -sy, 0], [0, 0, 1], [0, 0, -1]], F)
    out = np.where(on != 0, np.nextafter(on, np.where(on > 0, F(np.inf), F(-np.inf))), on).astype(F)
    return on, out


@functools.lru_cache(maxsize=None)
def crop_cloud():
    """the cloud of the crop tests: the first 24 splats moved onto / just off the surfaces of the exact matrices (read-only).  The
    fixtures share depths, so this cloud HAS equal keys: the crop tests store it in upload order, where ties keep that order"""
    aos = cloud_aos(*TIE_FREE).copy()
    k = 0
    for name in ("identity", "scaled"):
        for pts in on_surface(name):
            aos[k:k + 6, 0:3] = pts
            k += 6
    aos.setflags(write=False)
    return aos


CROPS = [(m, s, inv) for m in ("identity", "scaled", "rotated") for s in ("box", "sphere") for inv in (False, True)]


# ---- masks ------------------------------------------------------------------------------------------------------------------

def mask_cases(n):
    """name -> the mask, bool or uint8, in upload numbering"""
    rng = np.random.default_rng(1000 + n)
    bytes_ = rng.choice(np.array([0, 2, 255], np.uint8), n)
    every_other = np.arange(n) % 2 == 0
    one = np.zeros(n, bool)
    one[n // 3] = True
    cases = {"all_visible": np.ones(n, bool), "all_hidden": np.zeros(n, bool), "one_visible": one, "every_other": every_other,
             "random_30": rng.random(n) < 0.3, "bytes_2_255": bytes_}
    if n >= 2 * BOX:                     # exactly the slots of one whole box (with the cloud stored in upload order)
        hidden = np.ones(n, bool)
        hidden[BOX:2 * BOX] = False
        cases["one_box_hidden"], cases["one_box_visible"] = hidden, ~hidden
    return cases


def random_mask(n, seed=3, share=0.5):
    return np.random.default_rng(seed).random(n) < share
