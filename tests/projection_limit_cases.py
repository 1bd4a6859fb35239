"""Inputs for the limits tests of the projection (tests/test_projection_limits_fixtures.py on the CPU, tests/test_gpu_projection_limits.py
on the device): clouds and views designed for project_kernel's thresholds.  Inputs only -- no expected values, no device, no torch;
what a fixture claims to hit is checked by the CPU test with the oracle alone.

Every case has at most 4097 splats and a viewport of at most 353 x 301 pixels (12 x 10 bins, the last column 1 px wide and the top
row 13 px high)."""
import functools
import math

import numpy as np

from oracle import oracle as orc
from splatapult_amd import camera, synthetic
from tests import cull_cases as cc
from tests import scenes

F = np.float32
N, W, H = 4097, 353, 301
NF = scenes.NF
LADDER_CAMERAS = ("default", "squashed", "sheared", "asymmetric", "offset_viewport", "inside")
IDENT = np.array([1.0, 0.0, 0.0, 0.0], F)


def view(name, W=W, H=H):
    """(cam, proj, viewport, nearFar): the default rigid camera at (0, 0, 7), or one of tests/cull_cases.py's"""
    return scenes.default_view(W, H) if name == "default" else cc.CAMERAS[name](W, H)


def view_space(cam, xyz):
    """float64 view-space positions (n, 3) under the camera-to-world matrix cam"""
    m = np.linalg.inv(np.asarray(cam, np.float64).reshape(4, 4).T)
    return np.asarray(xyz, np.float64) @ m[:3, :3].T + m[:3, 3]


def oracle_splats(aos, full_sh, vw, srgb=False):
    """the oracle's Sort + projection of a view: dict(V, sorted_idx, sorted_keys, splats)"""
    cam, proj, vp, nf = vw
    return orc.render_frame(aos, full_sh, cam, proj, vp, nf, srgb=srgb, nthreads=8, want_image=False, want_splats=True)


# ---- the conditioning ladder --------------------------------------------------------------------------------------------------

def ladder_attrs(name, n=N, seed=71, W=W, H=H):
    """needles and sheets whose long-axis screen variance L under camera `name` runs from 1e3 to 1e8 px^2 (a third of the splats
    log-uniform in 1e3 .. 3e6, two thirds in 3e6 .. 1e8, where the fp32 covariance loses its sign; the camera's own stretch and
    the needle's angle to the view axis move single splats off the target).  The short axes lie four to seven decades below the
    long one.  By upload index mod 4: 0, 1 needles turned at random, 2 needles along world x, y, z in turn (identity rotation),
    3 sheets with two long axes (every other one unrotated).  The generator over-produces: the CPU test counts the classes."""
    a = synthetic.generate(n, seed=seed, pos_sigma=1.2, log_scale_mean=-3.0, log_scale_sigma=0.3, workers=1)
    cam, proj, vp, nf = view(name, W, H)
    depth = np.maximum(-view_space(cam, a["xyz"])[:, 2], 0.05)
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    u = np.where(i % 3 == 0, rng.uniform(3.0, 6.5, n), rng.uniform(6.5, 8.0, n))
    f_px = float(proj[5]) * vp[3] / 2.0
    long_ls = np.log(np.sqrt(10.0 ** u) * depth / f_px)
    short_ls = long_ls[:, None] - rng.uniform(4.0, 7.0, (n, 3)) * math.log(10.0)
    ls = short_ls.copy()
    kind = i % 4
    axis = (i // 4) % 3
    ls[i, np.where(kind == 2, axis, 0)] = long_ls
    sheet = kind == 3
    ls[sheet, 1] = long_ls[sheet] - rng.uniform(0.0, 1.0, int(sheet.sum()))
    a["log_scale"] = ls.astype(F)
    a["rot"][(kind == 2) | (sheet & (i % 8 == 3))] = IDENT
    a["opacity"] = rng.uniform(-3.0, 3.0, n).astype(F)
    return a


@functools.lru_cache(maxsize=None)
def ladder_cloud(name, W=W, H=H):
    return scenes.cloud_from_attrs(ladder_attrs(name, W=W, H=H))


# ---- ordinary splats and single records ----------------------------------------------------------------------------------------

def plain_aos(n, seed, pos_sigma=1.0, log_scale_mean=-3.5):
    """n ordinary splats around the origin as the reference's 61-float records (the oracle's own load-time arithmetic)"""
    a = synthetic.generate(n, seed=seed, pos_sigma=pos_sigma, pos_clip=2.0, log_scale_mean=log_scale_mean, workers=1)
    return orc.build_cloud(a["xyz"], a["f_dc"], a["f_rest"], a["opacity"], a["log_scale"], a["rot"], True)


def records(xyz, alpha=0.5, var=1e-4, seed=5):
    """one record per position: isotropic covariance var (a scalar or one per splat), the given stored alpha, ordinary SH"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    aos = plain_aos(xyz.shape[0], seed)
    aos[:, 0:3] = xyz
    aos[:, 3] = alpha
    aos[:, 16:25] = 0.0
    aos[:, 16] = aos[:, 20] = aos[:, 24] = var
    return aos


def _ord(x):
    """float32 -> an integer that ascends with the value (nextafter is +-1)"""
    i = int(np.asarray(x, F).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def _from_ord(k):
    return np.array(k if k >= 0 else (-k) | 0x80000000, np.uint32).view(F)[()]


def pred(x):
    return np.nextafter(F(x), F(-np.inf))


def succ(x):
    return np.nextafter(F(x), F(np.inf))


def project_points(xyz, vw):
    """the oracle's projection of ordinary records at the positions xyz, in the given order"""
    cam, proj, vp, nf = vw
    aos = records(xyz)
    return orc.project(np.arange(aos.shape[0], dtype=np.uint32), aos, True, False, orc.mat4_inverse(cam), proj, vp, nf, cam[12:15])


def threshold_coordinates(value_of, lo, hi, target, window=24):
    """coordinates c (float32, between lo and hi) at which the oracle's own fp32 value_of(c) -- monotone in c -- equals
    pred(target), target and succ(target): dict name -> c, for the names that some c reaches.  value_of takes an array."""
    klo, khi = sorted((_ord(lo), _ord(hi)))
    vlo, vhi = value_of(np.array([_from_ord(klo), _from_ord(khi)], F))
    rising = vhi > vlo
    a, b = klo, khi                                   # invariant: value(a) < target <= value(b) when rising
    while b - a > 1:
        m = (a + b) // 2
        v = value_of(np.array([_from_ord(m)], F))[0]
        if (v >= F(target)) == rising:
            b = m
        else:
            a = m
    cs = np.array([_from_ord(k) for k in range(max(a - window, klo), min(b + window, khi) + 1)], F)
    vs = value_of(cs)
    out = {}
    for name, t in (("pred", pred(target)), ("exact", F(target)), ("succ", succ(target))):
        hit = np.flatnonzero(vs == t)
        if hit.size:
            out[name] = cs[hit[0]]
    return out


# ---- threshold neighbours ------------------------------------------------------------------------------------------------------

# Near planes of the render camera.  Around ndc.z = 0.25 one ulp of the depth moves ndc.z = (P10 tz + P14) / -tz by three ulps, so
# one projection reaches at most one or two of pred(0.25), 0.25 and succ(0.25); these three reach all of them between them (found by
# trying near planes 0.100, 0.101, ...; tests/test_projection_limits_fixtures.py asserts that every value is hit)
THRESHOLD_NEARS = (0.1, 0.101, 0.129)
THRESHOLD_FAR = 8.0


def threshold_views(near=THRESHOLD_NEARS[0], W=W, H=H):
    """(sort view, render view).  Sort's cull keeps |ndc.xy| < 1.5, so a splat on the render camera's guard band |ndc.xy| = 2 is
    reached with another camera for Sort: the default one at (0, 0, 7).  The render camera sits at the origin and looks down -z
    (its view matrix is the identity: t = the position, bit for bit) with a far plane at 8."""
    sort = scenes.default_view(W, H)
    nf = [near, THRESHOLD_FAR]
    render = (camera.pose((0.0, 0.0, 0.0)), camera.perspective(camera.FOVY, W / H, *nf), [0, 0, W, H], nf)
    return sort, render


@functools.lru_cache(maxsize=None)
def threshold_case(near=THRESHOLD_NEARS[0]):
    """(aos, labels): splats whose oracle ndc.z lands on pred / exact / succ of 0.25 and of 1, ndc.x and ndc.y on those of +-2
    (searched over several depths: one depth need not reach all three), and centres at p.w = 0: the eye itself (len = 0), one
    denormal in front of and behind it, and tz = -1e-23, -1e-19 whose square underflows.  labels[i] = (threshold, which); only
    what the render camera of this near plane reaches is there."""
    _, render = threshold_views(near)
    pos, labels = [], []

    def ndc(axis, make):
        return lambda c: project_points(make(c), render)["ndc"][:, axis]

    along_z = lambda c: np.stack([np.zeros_like(c), np.zeros_like(c), c], axis=1)
    # (near ndc.z = 1 forty ulps of the depth move ndc.z by one: a wide window)
    for name, target, lo, hi, window in (("ndc.z=0.25", 0.25, -2.0 * near, -4.0 * near, 8), ("ndc.z=1", 1.0, -7.0, -9.0, 400)):
        for which, c in threshold_coordinates(ndc(2, along_z), lo, hi, target, window).items():
            pos.append([0.0, 0.0, c]); labels.append((name, which))
    for axis in (0, 1):
        for sign in (1.0, -1.0):
            name = "ndc.%s=%+d" % ("xy"[axis], int(2 * sign))
            found = {}
            for z in (-1.0, -1.37, -2.25, -3.1, -0.77, -4.6, -1.9, -2.7):
                def make(c, z=z):
                    p = np.zeros((c.shape[0], 3), F)
                    p[:, axis], p[:, 2] = c, z
                    return p
                for which, c in threshold_coordinates(ndc(axis, make), sign * 0.3 * -z, sign * 1.5 * -z, 2.0 * sign).items():
                    found.setdefault(which, make(np.array([c], F))[0])
                if len(found) == 3:
                    break
            for which, p in found.items():
                pos.append(list(p)); labels.append((name, which))
    tiny = np.array(1, np.uint32).view(F)[()]
    for which, z in (("exact", 0.0), ("pred", -tiny), ("succ", tiny), ("tz*tz underflows", -1e-23), ("tz*tz underflows", -1e-19)):
        pos.append([0.0, 0.0, z]); labels.append(("p.w=0", which))
    # ordinary neighbours in the same wave, in front of the render camera
    rng = np.random.default_rng(3)
    k = 64 - len(pos) % 64 + 64
    plain = np.stack([rng.uniform(-0.5, 0.5, k), rng.uniform(-0.4, 0.4, k), rng.uniform(-5.0, -1.5, k)], axis=1)
    aos = records(np.concatenate([np.array(pos, F), plain.astype(F)]), alpha=0.6, var=4e-4)
    aos.setflags(write=False)
    return aos, tuple(labels) + (("plain", ""),) * k


ALPHAS = (("pred", pred(1.0 / 256.0)), ("exact", F(1.0 / 256.0)), ("succ", succ(1.0 / 256.0)), ("one", F(1.0)))


@functools.lru_cache(maxsize=None)
def alpha_case():
    """(aos, view): four splats of zero covariance on the view axis of the default camera, W and H odd -- each centre is the
    centre of pixel (W // 2, H // 2) exactly -- with STORED alpha pred(1/256), 1/256, succ(1/256) and 1, nearest first, among
    ordinary splats of the same wave.  The splat of succ(1/256) lights exactly that pixel."""
    assert W % 2 == 1 and H % 2 == 1
    aos = plain_aos(64, 9)
    for j, (_, alpha) in enumerate(ALPHAS):
        aos[j, 0:3] = (0.0, 0.0, 2.0 - j)
        aos[j, 3] = alpha
        aos[j, 16:25] = 0.0
    aos.setflags(write=False)
    return aos, scenes.default_view(W, H)


# ---- rectangle edges -----------------------------------------------------------------------------------------------------------

EDGE_TARGETS = {0: (100, 96, 0, W - 1), 1: (100, 64, 0, H - 1)}      # per axis: an integer, a bin edge, the first and the last pixel
EDGE_DELTA = 5e-4


def footprint_edges(sp):
    """float64 (x0, x1, y0, y1) per oracle splat: px -+ ex - 0.5 and py -+ ey - 0.5 with e = sqrt(rho2 cov), rho2 = 2 ln(256 alpha):
    what ceil / floor turn into the first and last pixel of the footprint (tests/render_cases.py: oracle_rects)"""
    rho2 = 2.0 * np.log(256.0 * sp["alpha"].astype(np.float64))
    ex, ey = np.sqrt(rho2 * sp["cov"][:, 0]), np.sqrt(rho2 * sp["cov"][:, 3])
    px, py = sp["px"].astype(np.float64), sp["py"].astype(np.float64)
    return px - ex - 0.5, px + ex - 0.5, py - ey - 0.5, py + ey - 0.5


@functools.lru_cache(maxsize=None)
def rect_edges_case():
    """(aos, view, wanted): isotropic splats under the default camera whose footprint edge px - ex - 0.5 (side -1) or
    px + ex - 0.5 (side +1), and the same in y, lies EDGE_DELTA above or below an integer, a bin edge, the first and the last
    pixel of the viewport: wanted[i] = (axis, side, target + delta) for the first len(wanted) splats.  Then: 16 small splats
    wholly off screen with the centre inside the guard band (1.2 <= |ndc.x| or |ndc.y| < 1.45), 4 that cover the whole viewport,
    4 of zero covariance (the 0.3 px low-pass term alone), and ordinary splats up to 128."""
    vw = cam, proj, vp, nf = scenes.default_view(W, H)
    tan_y = 1.0 / float(proj[5])
    tan_x = 1.0 / float(proj[0])
    wanted, pos = [], []
    for axis in (0, 1):
        size = (W, H)[axis]
        for side in (-1, 1):
            for k in EDGE_TARGETS[axis]:
                for delta in (-EDGE_DELTA, EDGE_DELTA):
                    j = len(wanted)
                    depth = 4.0 + 0.125 * j
                    centre = k + 0.5 - side * 19.8                     # the footprint is about 19.8 px to either side
                    p = [0.0, 0.0, 7.0 - depth]
                    p[axis] = (2.0 * centre / size - 1.0) * (tan_x, tan_y)[axis] * depth
                    p[1 - axis] = 0.1 * ((j % 5) - 2) * depth * 0.2
                    pos.append(p)
                    wanted.append((axis, side, k + delta))
    aos = records(np.array(pos, F), alpha=0.7, var=1e-2, seed=13)
    n = len(wanted)
    view_m = orc.mat4_inverse(cam)
    for _ in range(12):
        sp = orc.project(np.arange(n, dtype=np.uint32), aos, True, False, view_m, proj, vp, nf, cam[12:15])
        edges = footprint_edges(sp)
        rho2 = 2.0 * np.log(256.0 * sp["alpha"].astype(np.float64))
        for j, (axis, side, t) in enumerate(wanted):
            cov = float(sp["cov"][j, 0 if axis == 0 else 3])
            e = math.sqrt(rho2[j] * cov)
            got = edges[2 * axis + (0 if side < 0 else 1)][j]
            e_new = e + side * (t - got)                               # side -1: the edge is centre - e
            scale = (e_new * e_new / rho2[j] - 0.3) / (cov - 0.3)
            aos[j, 16] = aos[j, 20] = aos[j, 24] = F(aos[j, 16] * scale)
    rng = np.random.default_rng(21)
    extra = []
    for j in range(16):                                                # wholly off screen, centre inside the guard band
        depth = 3.0 + 0.2 * j
        u = (1.2 + 0.25 * (j // 4) / 4.0) * (1.0 if j % 2 == 0 else -1.0)
        p = [0.0, 0.0, 7.0 - depth]
        p[(j // 2) % 2] = u * (tan_x, tan_y)[(j // 2) % 2] * depth
        extra.append(p)
    off = records(np.array(extra, F), alpha=0.9, var=1e-5, seed=14)
    whole = records(np.array([[0.0, 0.0, 1.0], [0.3, 0.2, 0.5], [-0.4, 0.1, 0.0], [0.0, -0.3, -1.0]], F), alpha=0.3, var=25.0, seed=15)
    zero = records(np.array([[0.2, 0.1, 1.5], [-0.3, 0.3, 1.0], [0.5, -0.4, 0.2], [-0.6, -0.2, -0.5]], F), alpha=0.95, var=0.0, seed=16)
    out = np.concatenate([aos, off, whole, zero, plain_aos(128 - n - 24, 17)])
    out.setflags(write=False)
    return out, vw, tuple(wanted)


# ---- colour --------------------------------------------------------------------------------------------------------------------

def _look(axis, sign):
    """camera-to-world matrix of a camera at the origin whose viewing direction (-z of the camera) is sign * world axis: a signed
    permutation, exact in float32"""
    back = np.zeros(3); back[axis] = -sign
    right = np.zeros(3); right[(axis + 1) % 3] = 1.0
    up = np.cross(back, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = right, up, back
    return m.T.astype(F).reshape(16).copy(), np.stack([right, up, back], axis=1)


COLOUR_LOOKS = tuple((axis, sign) for axis in range(3) for sign in (1.0, -1.0))
SRGB_EDGE = F(0.04045)
B0 = 0.28209479177387814


@functools.lru_cache(maxsize=None)
def colour_case(look):
    """(aos, view, directions) for one of the six axis-aligned cameras at the origin with a 100-degree field of view: per camera-
    space direction (a, b, -1), a, b in {-1, 0, 1} -- world directions along an axis, a face diagonal or a space diagonal, where
    single SH basis functions vanish -- two splats (at 2 and 4 times the direction) whose 48 SH coefficients have magnitudes
    1e-3 .. 1e2 and mixed signs; then, on the view axis, splats whose only non-zero coefficients are the three constant terms,
    chosen so that 0.5 + SH runs from -2 to 4, and nine more a few ulps around the sRGB curve's knee 0.04045 (which 0.5 + s
    reaches only on a grid of 2^-25, so `exact` may not exist: the CPU test says which neighbours are hit)."""
    axis, sign = COLOUR_LOOKS[look]
    cam, R = _look(axis, sign)
    vw = (cam, camera.perspective(math.radians(100.0), W / H), [0, 0, W, H], NF)
    rng = np.random.default_rng(100 + look)
    dirs = [(a, b, -1.0) for a in (-1.0, 0.0, 1.0) for b in (-1.0, 0.0, 1.0)]
    pos = [R @ np.array(d) * r for d in dirs for r in (2.0, 4.0)]
    ramp = np.linspace(-2.0, 4.0, 25)
    knee_c = F((float(SRGB_EDGE) - 0.5) / B0)
    knee = [_from_ord(_ord(knee_c) + j) for j in range(-4, 5)]
    n_sh, n_axis = len(pos), len(ramp) + len(knee)
    pos += [R @ np.array([0.0, 0.0, -1.0]) * (1.0 + 0.05 * j) for j in range(n_axis)]
    aos = records(np.array(pos, F), alpha=0.5, var=1e-3, seed=30 + look)
    sh = np.r_[4:16, 25:61]
    aos[:n_sh, sh] = (rng.choice([-1.0, 1.0], (n_sh, 48)) * 10.0 ** rng.uniform(-3.0, 2.0, (n_sh, 48))).astype(F)
    aos[n_sh:, sh] = 0.0
    for ch, base in enumerate((4, 8, 12)):
        aos[n_sh:n_sh + len(ramp), base] = (np.roll(ramp, 7 * ch) - 0.5) / B0
        aos[n_sh + len(ramp):, base] = knee
    aos.setflags(write=False)
    return aos, vw, tuple(tuple(R @ np.array(d)) for d in dirs)


# ---- non-finite attributes -----------------------------------------------------------------------------------------------------

NONFINITE = (np.nan, np.inf, -np.inf)
GEOMETRY_FIELDS = (("x", 0), ("y", 1), ("z", 2), ("cov00", 16), ("cov01", 17), ("cov22", 24), ("alpha", 3))
COLOUR_FIELDS = (("sh0", 4), ("sh1", 9), ("sh3", 40))


def _poisoned(fields, seed, spare_alpha_inf=False):
    aos = plain_aos(256, seed, pos_sigma=0.8)
    where = []
    for j, (name, off) in enumerate(fields):
        for k, v in enumerate(NONFINITE):
            if spare_alpha_inf and name == "alpha" and v == np.inf:
                continue
            i = 5 + 11 * (3 * j + k)                                  # 11 apart: two or three per wave, neighbours ordinary
            aos[i, off] = v
            where.append((i, name, v))
    aos.setflags(write=False)
    return aos, tuple(where)


@functools.lru_cache(maxsize=None)
def nonfinite_geometry_case():
    """(aos, view, where): 256 ordinary splats; where[k] = (upload index, field, value): NaN, +inf and -inf, one at a time, in the
    position, the covariance and the stored alpha.  (alpha = +inf is in nonfinite_colour_case: it is drawn.)"""
    aos, where = _poisoned(GEOMETRY_FIELDS, 41, spare_alpha_inf=True)
    return aos, scenes.default_view(W, H), where


@functools.lru_cache(maxsize=None)
def nonfinite_colour_case():
    """the same with NaN, +inf and -inf in SH coefficients of degree 0, 1 and 3, and alpha = +inf: splats the reference draws, with
    a colour or a weight that is not finite"""
    aos, where = _poisoned(COLOUR_FIELDS, 42)
    aos = aos.copy()
    aos[200, 3] = np.inf
    aos.setflags(write=False)
    return aos, scenes.default_view(W, H), where + ((200, "alpha", np.inf),)


# ---- visible counts ------------------------------------------------------------------------------------------------------------

COUNTS = (1, 63, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def count_case(V, stride=1, rem=0):
    """(aos, view): V * stride splats of which exactly the V with upload index = rem mod stride are in front of the default
    camera (the others sit behind it): stride 8 makes all sorted indices equal modulo 8"""
    aos = plain_aos(V * stride, 50 + V, pos_sigma=0.7).copy()
    hidden = np.arange(V * stride) % stride != rem
    aos[hidden, 2] += 20.0
    aos.setflags(write=False)
    return aos, scenes.default_view(W, H)
