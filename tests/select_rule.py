"""What the selection tests share (numpy only; no device, no torch): msplat_mark_view's rule of include/msplat.h restated in numpy
float32 in the header's operation order and in float64, the cameras whose MVP is exact in fp32 with the centres designed for them,
the random-camera comparison set, the measure in numpy, and the hostile inputs of msplat_measure_box.  msplat_mark_volume's rule is
tests/visibility_rule.py's crop().  Nothing here is measured."""
import ctypes as C
import functools
import math

import numpy as np

from splatapult_amd import _capi
from tests import cull_cases
from tests import visibility_rule as vr

F = np.float32
_P = C.POINTER(C.c_float)


def mvp_of(cam, proj):
    """float32[16]: msplat_mat4_mul(projMat, msplat_mat4_inverse(cameraMat)), the library's own host functions -- what msplat_sort
    and msplat_mark_view build"""
    L = _capi.lib()
    f = lambda a: np.ascontiguousarray(np.asarray(a, F).reshape(16))
    view, mvp = np.zeros(16, F), np.zeros(16, F)
    L.msplat_mat4_inverse(f(cam).ctypes.data_as(_P), view.ctypes.data_as(_P))
    L.msplat_mat4_mul(f(proj).ctypes.data_as(_P), view.ctypes.data_as(_P), mvp.ctypes.data_as(_P))
    return mvp


def centre_px(xyz, mvp, W, H, dtype=F):
    """(cx, cy, depth) per centre, every operation rounded to `dtype`, nothing fused, in msplat.h's order"""
    m = np.asarray(mvp, dtype).reshape(16)
    x, y, z = (np.asarray(xyz)[:, k].astype(dtype) for k in range(3))
    W, H, half = dtype(W), dtype(H), dtype(0.5)
    with np.errstate(all="ignore"):
        px = ((m[0] * x + m[4] * y) + m[8] * z) + m[12]
        py = ((m[1] * x + m[5] * y) + m[9] * z) + m[13]
        pw = ((m[3] * x + m[7] * y) + m[11] * z) + m[15]
        xx, yy = px / pw, py / pw
        return half * (W + (xx * W)), half * (H + (yy * H)), pw


def view_inside(xyz, mvp, W, H, window=None, region=None, dtype=F):
    """bool per centre: msplat_mark_view marks it.  window = (x0, y0, w, h) or None; region = (h, w) array or None"""
    cx, cy, depth = centre_px(xyz, mvp, W, H, dtype)
    x0, y0, w, h = window if window is not None else (0, 0, int(W), int(H))
    with np.errstate(invalid="ignore"):
        inside = (depth > 0) & (cx >= x0) & (cx < x0 + w) & (cy >= y0) & (cy < y0 + h)
    if region is not None:
        region = np.asarray(region)
        assert region.shape == (h, w), (region.shape, h, w)
        col = np.where(inside, cx, x0).astype(np.int64) - x0          # (int)cx: truncation of a value known to lie in the window
        row = np.where(inside, cy, y0).astype(np.int64) - y0
        inside &= region[row, col] != 0
    return inside


def marked(mask, inside, value):
    """what a mark leaves in `mask` (a copy is returned): `value` where inside, the other bytes as they were"""
    out = np.array(mask, np.uint8)
    out[inside] = value
    return out


# ---- cameras whose MVP is exact in fp32 (the idea of tests/sort_limit_cases.py): an identity or axis-permuting camera-to-world
# matrix with power-of-two translations and a projection with power-of-two entries; pw = the distance along the view axis -----------
EW, EH = 32, 16                          # the exact cases' viewport: powers of two, so xx W and 0.5 (W + xx W) are exact


def _proj_pow2(sx, sy):
    p = np.zeros((4, 4))
    p[0, 0], p[1, 1], p[2, 2], p[2, 3], p[3, 2] = sx, sy, -1.0, -0.25, -1.0
    return np.ascontiguousarray(p.T.reshape(16), F)


def exact_cameras():
    """name -> (cameraMat, projMat, (sx, sy), R, t): camera-to-world = [R | t], R a signed permutation (columns = the camera's axes
    in the world)"""
    ident = np.eye(3)
    perm = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])        # camera x -> world y, y -> z, z -> x
    flip = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])       # a quarter turn about the view axis
    out = {}
    for name, R, t, s in (("identity", ident, (0.0, 0.0, 0.0), (1.0, 1.0)), ("permuted", perm, (2.0, -0.5, 4.0), (2.0, 0.5)),
                          ("quarter_turn", flip, (-1.0, 8.0, 0.25), (0.5, 1.0))):
        cam = np.eye(4)
        cam[:3, :3], cam[:3, 3] = R, t
        out[name] = (np.ascontiguousarray(cam.T.reshape(16), F), _proj_pow2(*s), s, R, np.asarray(t))
    return out


def exact_mvp64(name):
    """the same MVP in float64 from the closed form: proj * [R^T | -R^T t]"""
    cam, proj, s, R, t = exact_cameras()[name]
    view = np.eye(4)
    view[:3, :3], view[:3, 3] = R.T, -R.T @ t
    return (proj.astype(np.float64).reshape(4, 4).T @ view).T.reshape(16)


EXACT_WINDOWS = {"viewport": None, "inner": (5, 3, 17, 9), "edge": (20, 0, 12, 16), "one_pixel": (7, 6, 1, 1)}


@functools.lru_cache(maxsize=None)
def exact_centres(name):
    """(xyz float32 (n, 3), cx, cy, depth float64) for exact_cameras()[name]: every half-integer pixel coordinate from one pixel
    left of / below the viewport to one pixel beyond it -- pixel centres (k + 0.5), pixel borders (k), hence every edge and
    corner of every window of EXACT_WINDOWS -- at depths 1, 2 and 4 in turn; then the same lattice thinned at depth 0 and behind
    the camera, and centres with x = NaN.  Every value is exact in fp32, and so is every operation of the rule on them"""
    cam, proj, (sx, sy), R, t = exact_cameras()[name]
    gx, gy = np.meshgrid(np.arange(-2, 2 * EW + 3) / 2.0, np.arange(-2, 2 * EH + 3) / 2.0)
    cx, cy = gx.ravel(), gy.ravel()
    depth = np.array([1.0, 2.0, 4.0])[np.arange(cx.size) % 3]
    ex_cx, ex_cy = cx[::7], cy[::7]                                   # depth 0 and behind the camera
    cx = np.concatenate([cx, ex_cx, ex_cx])
    cy = np.concatenate([cy, ex_cy, ex_cy])
    depth = np.concatenate([depth, np.zeros(ex_cx.size), -2.0 * np.ones(ex_cx.size)])
    d = np.where(depth == 0.0, 1.0, depth)                            # (depth 0: any camera-space x, y; these keep pw = 0)
    xc = (2.0 * cx - EW) / EW * d / sx                                # camera space: px = sx xc, pw = -zc
    yc = (2.0 * cy - EH) / EH * d / sy
    world = np.stack([xc, yc, -depth], axis=1) @ R.T + t
    xyz = world.astype(F)
    assert (xyz.astype(np.float64) == world).all(), "a designed centre is not a float32"
    k = xyz.shape[0]
    xyz = np.concatenate([xyz, xyz[5:k:97]])                          # ... and NaN centres, copies of inside ones
    xyz[k:, 0] = np.nan
    pad = lambda a: np.concatenate([a, np.full(xyz.shape[0] - k, np.nan)])
    xyz.setflags(write=False)
    return xyz, pad(cx), pad(cy), pad(depth)


def region_for(window, seed):
    """(h, w) uint8 of 0, 1 and 255 for a window of the exact viewport"""
    x0, y0, w, h = window if window is not None else (0, 0, EW, EH)
    return np.random.default_rng(seed).choice(np.array([0, 0, 1, 255], np.uint8), (h, w))


def splat_rows(xyz):
    """(n, 61) records of small, opaque-ish splats at the given centres (tests/visibility_rule.py's cloud with its centres replaced)"""
    n = xyz.shape[0]
    aos = vr.cloud_aos(max(n, 255))[:n].copy()
    aos[:, 0:3] = xyz
    return aos


# ---- general cameras: the rule in float64 wherever fp32 cannot decide differently -----------------------------------------------
GW, GH = 256, 160
GENERAL_N, GENERAL_SEED = 4097, 77
GENERAL_WINDOW = (31, 17, 160, 90)
BORDER_PX = 1e-3                         # the issue's margin: a centre nearer than this to a pixel border may fall on either side
MAX_LEFT_OUT = 0.01


def general_views():
    return {"default": vr.view(), "rolled": cull_cases.CAMERAS["rolled"](GW, GH), "asymmetric": cull_cases.CAMERAS["asymmetric"](GW, GH)}


@functools.lru_cache(maxsize=None)
def general_cloud():
    aos = vr.cloud_aos(GENERAL_N, GENERAL_SEED).copy()
    aos[:, 0:3] *= F(1.6)                # some of it outside every window, some of it behind the "inside"-style near planes
    aos.setflags(write=False)
    return aos


def general_region():
    """a lasso-like plane of GENERAL_WINDOW: a disc with a hole, bytes 0 / 1 / 200"""
    x0, y0, w, h = GENERAL_WINDOW
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = ((xx - w / 2.0) / (w / 2.0)) ** 2 + ((yy - h / 2.0) / (h / 2.0)) ** 2
    return np.where((r2 <= 1.0) & (r2 >= 0.05), np.where((xx + yy) % 3 == 0, 200, 1), 0).astype(np.uint8)


def decidable(xyz, mvp, W, H):
    """bool per centre: its float64 pixel is farther than BORDER_PX from every pixel border (the window's and the region's edges
    are pixel borders) and its float64 depth is not within 1e-6 of 0 relative to its terms -- or it is so far outside the viewport
    that no window contains it either way.  (fp32 evaluates cx of these clouds, two or more units in front of the camera, to
    about 1e-4 px: tests/test_select.py checks that numpy's fp32 rule and the float64 rule agree on this set)"""
    cx, cy, depth = centre_px(xyz, mvp, W, H, np.float64)
    m = np.asarray(mvp, np.float64).reshape(16)
    x, y, z = (np.asarray(xyz)[:, k].astype(np.float64) for k in range(3))
    scale = np.abs(m[3] * x) + np.abs(m[7] * y) + np.abs(m[11] * z) + np.abs(m[15])
    with np.errstate(invalid="ignore"):
        far = (depth < -1e-6 * scale) | (cx < -1.0) | (cx > W + 1.0) | (cy < -1.0) | (cy > H + 1.0)
        near_border = (np.abs(cx - np.rint(cx)) < BORDER_PX) | (np.abs(cy - np.rint(cy)) < BORDER_PX)
        ok = (np.abs(depth) > 1e-6 * scale) & ~near_border
    return far | ok


# ---- the measure ---------------------------------------------------------------------------------------------------------------
MEASURE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 4097)
MEASURE_N = 4097
SUM2_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


@functools.lru_cache(maxsize=None)
def measure_rows():
    """(4097, 61) records for the measure tests: a synthetic cloud with, spread over the upload indices, NaN and +-inf centres,
    centres of magnitude 1e18, alpha 0 (footprint bound 0) and an infinite covariance (footprint bound inf)"""
    aos = vr.cloud_aos(MEASURE_N).copy()
    aos[3::61, 0] = np.nan
    aos[7::127, 1] = np.inf
    aos[11::131, 2] = -np.inf
    aos[13::97, 0:3] = F(1e18) * np.sign(aos[13::97, 0:3])
    aos[17::89, 1] = F(-1e18)
    aos[19::53, 3] = 0.0                 # alpha 0: pos4.w = 0
    aos[23::211, 16] = np.inf            # covariance xx = inf: pos4.w = inf
    aos.setflags(write=False)
    return aos


def measure_selection(count, n=MEASURE_N):
    """uint8[n] with `count` nonzero bytes (1 or 255) spread over the upload indices, the hostile rows among them"""
    sel = np.zeros(n, np.uint8)
    if count:
        idx = np.unique(np.linspace(0, n - 1, count).astype(np.int64)) if count < n else np.arange(n)
        if count == 1:
            idx = np.array([n // 2])
        assert idx.size == count, (idx.size, count)
        sel[idx] = np.where(idx % 2 == 0, 1, 255)
    return sel


def measure(pos4, select=None):
    """msplat_measure_cloud in numpy over the position plane (n, 4) in upload numbering: the exact fields, and for each of the nine
    sums (sum x y z, then SUM2_PAIRS) the exactly rounded sum of the exact terms (math.fsum) with the bound finite * 2^-53 * S"""
    pos4 = np.asarray(pos4, F)
    chosen = np.ones(pos4.shape[0], bool) if select is None else np.asarray(select) != 0
    p = pos4[chosen]
    fin = np.isfinite(p[:, 0:3]).all(axis=1)
    q = p[fin]
    out = dict(selected=int(chosen.sum()), finite=int(fin.sum()))
    out["lo"] = q[:, 0:3].min(axis=0) if q.shape[0] else np.full(3, np.inf, F)
    out["hi"] = q[:, 0:3].max(axis=0) if q.shape[0] else np.full(3, -np.inf, F)
    w = q[:, 3]
    w = w[np.isfinite(w) & (w > 0)]
    out["reach2_max"] = w.max() if w.size else F(0.0)
    d = q[:, 0:3].astype(np.float64)
    terms = [d[:, k] for k in range(3)] + [d[:, a] * d[:, b] for a, b in SUM2_PAIRS]     # (a product of two floats is exact in double)
    out["sums"] = np.array([math.fsum(t) for t in terms])
    out["bounds"] = np.array([out["finite"] * 2.0 ** -53 * math.fsum(np.abs(t)) for t in terms])
    return out


# ---- msplat_measure_box's hostile measures: name -> (lo, hi) float32[3] -------------------------------------------------------
def box_cases():
    f = lambda *v: np.array(v, F)
    big = F(1e6)
    return {
        "single_point": (f(0.3, -7.25, 1e-3), f(0.3, -7.25, 1e-3)),
        "single_point_at_zero": (f(0, 0, 0), f(0, 0, 0)),
        "extent_1e-30": (f(0.0, -5e-31, 1.0), f(1e-30, 5e-31, F(1.0) + F(2.0 ** -23))),
        "extent_1e18": (f(-5e17, 0.0, -1e18), f(5e17, 1e18, 1.0)),
        "far_and_thin": (f(big, -big, big), f(big + F(1e-3), -big + F(0.0625), np.nextafter(big, F(np.inf)))),
        "far_and_ten_wide": (f(big, -big - F(10.0), -3.0), f(big + F(10.0), -big, 7.0)),
        # (a corner of this one leaves the box that a relative widening alone gives: tests/test_select.py shows it)
        "far_and_eight_wide": (f(86474.828125, -2885316.25, 906.6351318359375), f(86482.546875, -2885295.25, 907.1133422851562)),
        "denormal": (f(1e-40, -1e-45, 0.0), f(2e-40, 1e-45, 1e-42)),
    }


def box_cloud(lo, hi, seed=5, n=2000):
    """float32 centres inside [lo, hi] per axis: the eight corners, the face centres' neighbours and a uniform draw clipped to the box"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    rng = np.random.default_rng(seed)
    u = rng.random((n, 3))
    pts = (lo.astype(np.float64) * (1.0 - u) + hi.astype(np.float64) * u).astype(F)
    pts = np.clip(pts, lo, hi)
    corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], F)
    inner = np.clip(np.stack([np.nextafter(lo, hi), np.nextafter(hi, lo)]), lo, hi).astype(F)
    return np.concatenate([corners, inner, pts])
