"""Inputs and references the render tests share (numpy, the oracle and host code only: no device, no torch): scenes and views,
destinations, occluder planes, the oracle recipes of the target modes, the depth output, the occluder test and the layers frame
with their float64 definitions, and a few fixtures of the point, covariance and cloud-storage tests.

The recipes never change the oracle.  The blend is linear in colour, so a frame over a destination is C_ref + T_ref dst with
T_ref = 1 - the oracle's frame of the same splats in white (composite_pair); window depth is composited as one more colour; and
behind a plane with a few distinct levels the pixels of level v are those of the frame of the splats with z_w < v
(levels_in_front).  tests/test_depth_output.py, tests/test_occluded.py and tests/test_layers.py pin the recipes against the
definitions.  Every cached result is computed once per process and is read-only."""
import functools

import numpy as np

from oracle import oracle as orc
from splatapult_amd import _capi, camera
from tests import scenes

MODES = ("clear", "load", "premultiplied")
NP_DTYPES = {"fp32": np.float32, "fp16": np.float16, "rgba8": np.uint8, "srgb8": np.uint8}


# ---- scenes and views --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene(name):
    """(cloud, W, H, view kwargs): ragged edge tiles and many empty tiles / the nasty attributes / saturated tiles and early exit"""
    if name == "sparse":
        return scenes.synth_cloud(20000, 302, log_scale_mean=-4.2), 517, 293, dict(z=7.0)
    if name == "hard":
        return scenes.cloud_from_attrs(scenes.hard_attrs(6000, 17)), 400, 300, dict(z=6.0, yaw=0.7)
    if name == "dense":
        return scenes.synth_cloud(120000, 301, log_scale_mean=-2.6), 640, 360, dict(z=0.8, yaw=2.0)
    raise KeyError(name)


def view_of(name, **over):
    cloud, W, H, kw = scene(name)
    return cloud, W, H, scenes.default_view(W, H, **dict(kw, **over))


def spread_view():
    """the "hard" scene between near / far planes that hug it: z_w of what the pixels see runs from the near cull (0.625) to the
    far plane instead of crowding towards 1 (chosen on the CPU with the oracle; test_depth_matches_the_oracle asserts the spread)"""
    cloud, W, H, _ = scene("hard")
    zn, zf = 5.02, 6.33
    return cloud, W, H, (camera.pose((0.0, 0.0, 5.75), 0.524, 0.037), camera.perspective(camera.FOVY, W / H, zn, zf), [0, 0, W, H], [zn, zf])


def case(name):
    return spread_view() if name == "spread" else view_of(name)


def stereo_eyes(W, H):
    """two eyes as tests/test_gpu_target_mode.py::test_render_stereo_equals_two_renders builds them"""
    proj = camera.perspective(camera.FOVY, W / H)
    return [camera.pose((-0.1, 0.0, 6.0), 0.65), camera.pose((0.1, 0.0, 6.0), 0.75)], proj, [0, 0, W, H], scenes.NF


def hand_placed():
    """eight splats in front of a camera at z = 4 looking down -Z: overlapping footprints at distinct depths, one opaque, one faint,
    one off to the side that overlaps nothing; near / far = 1 / 8 so that z_w covers most of [0.625, 1]"""
    xyz = np.array([[0.0, 0.0, 1.6], [0.15, 0.05, 0.8], [-0.2, 0.1, 0.0], [0.1, -0.15, -1.0], [0.0, 0.0, -2.5],
                    [0.9, 0.5, 0.5], [-0.1, 0.0, 1.2], [0.3, 0.2, -3.4]], np.float32)
    n = xyz.shape[0]
    f_dc = np.linspace(-1.0, 1.0, n * 3, dtype=np.float32).reshape(n, 3)
    opacity = np.array([0.5, 2.0, -1.0, 30.0, 1.0, 0.0, -4.5, 3.0], np.float32)            # logits: alpha 0.01 .. 1
    log_scale = np.log(np.array([[0.12, 0.2, 0.1], [0.3, 0.1, 0.1], [0.25, 0.25, 0.25], [0.4, 0.2, 0.1], [0.8, 0.6, 0.3],
                                 [0.1, 0.1, 0.1], [0.5, 0.05, 0.1], [1.0, 1.0, 0.2]], np.float32))
    rot = np.array([[1, 0, 0, 0], [0.9, 0.1, 0.3, 0.2], [1, 0, 0, 0], [0.7, 0.0, 0.0, 0.7], [1, 0, 0, 0], [1, 0, 0, 0],
                    [0.6, 0.5, 0.4, 0.3], [1, 0, 0, 0]], np.float32)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    aos = orc.build_cloud(xyz, f_dc, None, opacity, log_scale, rot, False)
    W, H, zn, zf = 96, 64, 1.0, 8.0
    view = (camera.pose((0.0, 0.0, 4.0)), camera.perspective(camera.FOVY, W / H, zn, zf), [0, 0, W, H], [zn, zf])
    return aos, W, H, view


@functools.lru_cache(maxsize=None)
def hand_placed_splats():
    aos, W, H, (cam, proj, vp, nf) = hand_placed()
    ref = orc.render_frame(aos, False, cam, proj, vp, nf, nthreads=4, want_image=False, want_splats=True)
    splats = ref["splats"]
    assert ref["V"] == aos.shape[0] and (splats["reject"] == 0).all(), "not all eight hand-placed splats are drawn"
    splats.setflags(write=False)
    return splats


@functools.lru_cache(maxsize=None)
def scene_splats(name):
    """the oracle's projected splats of a scene's view in draw order (read-only), V"""
    cloud, W, H, (cam, proj, vp, nf) = view_of(name)
    ref = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=16, want_image=False, want_splats=True)
    ref["splats"].setflags(write=False)
    return ref["splats"], ref["V"]


BIN = 32      # msplat_tile_size(): the bin edge in pixels (asserted against the library by tests/test_gpu_bin_grid_limits.py)

# name -> (W, H, yaw, n, seed, hard): the five strips of tests/test_gpu_bin_grid_limits.py (tests/test_bin_grid_fixtures.py checks
# their reach on the CPU)
STRIPS = {
    "wide_synth": (8192, 64, 0.0, 40000, 5, False),
    "tall_synth": (64, 8192, 0.0, 40000, 6, False),
    "wide_hard": (8192, 64, 0.1, 20000, 7, True),
    "tall_hard": (64, 8192, 0.0, 20000, 8, True),
    "ragged_hard": (8191, 33, 0.0, 20000, 9, True),
}


@functools.lru_cache(maxsize=None)
def strip_cloud(name):
    W, H, yaw, n, seed, hard = STRIPS[name]
    return scenes.cloud_from_attrs(scenes.strip_attrs(n, seed, W, H, hard))


def strip_case(name):
    """(cloud, W, H, view) of a named strip"""
    W, H, yaw = STRIPS[name][:3]
    return strip_cloud(name), W, H, scenes.strip_view(W, H, yaw)


def oracle_rects(sp, W, H, bin_px=BIN):
    """(drawn, tx0, ty0, tx1, ty1) per sorted splat from the oracle's projection: drawn = some pixel centre of the viewport lies
    inside the bounding box of the w > 1/256 footprint (every such pixel lies within rho sqrt(cov) of the centre); the box in bins"""
    alpha = sp["alpha"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho2 = 2.0 * np.log(256.0 * alpha)
    vis = (sp["reject"] == 0) & (rho2 > 0)
    ex = np.sqrt(np.maximum(rho2, 0) * sp["cov"][:, 0])
    ey = np.sqrt(np.maximum(rho2, 0) * sp["cov"][:, 3])
    x0 = np.ceil(sp["px"] - ex - 0.5); x1 = np.floor(sp["px"] + ex - 0.5)
    y0 = np.ceil(sp["py"] - ey - 0.5); y1 = np.floor(sp["py"] + ey - 0.5)
    drawn = vis & (x1 >= 0) & (y1 >= 0) & (x0 <= W - 1) & (y0 <= H - 1) & (x0 <= x1) & (y0 <= y1)
    c = lambda v, hi: (np.clip(np.nan_to_num(v), 0, hi - 1) // bin_px).astype(np.int64)
    return drawn, c(x0, W), c(y0, H), c(x1, W), c(y1, H)


# ---- destinations ------------------------------------------------------------------------------------------------------------

def random_dst(H, W, seed, dtype=np.float32, lo=0.0, hi=2.0):
    """finite destination pixels, alpha included"""
    return np.random.default_rng(seed).uniform(lo, hi, (H, W, 4)).astype(np.float32).astype(dtype)


def const_dst(H, W, rgba, dtype=np.float32):
    return np.broadcast_to(np.asarray(rgba, np.float32), (H, W, 4)).astype(dtype)


def random_bytes(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 4), dtype=np.uint8)


def dst_for(fmt, H, W, seed):
    """finite destination pixels in the format's host dtype"""
    if NP_DTYPES[fmt] == np.uint8:
        return np.random.default_rng(seed).integers(0, 256, (H, W, 4)).astype(np.uint8)
    return random_dst(H, W, seed, NP_DTYPES[fmt])


def empty_frame(mode, dst):
    """what a Render with nothing visible leaves in `mode` over dst (any format's host dtype)"""
    if mode == "load":
        return dst
    one = 255 if dst.dtype == np.uint8 else 1
    return np.broadcast_to(np.array([0, 0, 0, one if mode == "clear" else 0], dst.dtype), dst.shape)


def junk_plane(H, W, seed):
    """what a caller's plane may hold: NaN, infinities, huge and negative values"""
    z = (np.random.default_rng(seed).standard_normal((H, W)) * 1e6).astype(np.float32)
    z[::2, ::3] = np.nan
    z[1::4, 1::5] = np.inf
    return z


# ---- occluder planes ---------------------------------------------------------------------------------------------------------

# The GPU's z_w may differ from the oracle's in the last bits (z_w < 1: an ulp is <= 2^-24); a splat on the wrong side of a level
# is not a rounding error, so every level keeps this distance from every drawn splat's z_w
MARGIN = 2.0 ** -20
BORDER_X, BORDER_Y = 37, 21          # the four-level plane's region borders: inside a 16 x 4 strip of the compositor's tiles
SMALL_VIEWPORTS = [(70, 45), (33, 17), (16, 16)]      # no multiples of 16 / smaller than a bin / a single tile


def window_depth(splats):
    """z_w per orc.project'ed splat: project_kernel's arithmetic, an exact product and one rounded sum"""
    zw = np.float32(0.5) * splats["ndc"][:, 2] + np.float32(0.5)
    assert zw.dtype == np.float32, zw.dtype
    return zw


def choose_levels(splats, quantiles=(0.2, 0.4, 0.6, 0.8)):
    """one plane level per quantile of the drawn splats' z_w: the midpoint of a gap of more than 2.5 MARGIN between two
    neighbouring z_w values, the gap nearest to the quantile among those that show and hide at least 10 % of the drawn splats"""
    zw = np.sort(window_depth(splats)[splats["reject"] == 0].astype(np.float64))
    n = zw.shape[0]
    gaps = np.flatnonzero(np.diff(zw) > 2.5 * MARGIN)            # gap i lies between zw[i] and zw[i + 1]: i + 1 splats are in front
    shown = (gaps + 1) / n
    gaps, shown = gaps[(shown >= 0.1) & (shown <= 0.9)], shown[(shown >= 0.1) & (shown <= 0.9)]
    levels = []
    for q in quantiles:
        assert gaps.size, "no gap of 2.5 * 2^-20 left in the drawn z_w between the 10 % and 90 % quantiles"
        k = int(np.argmin(np.abs(shown - q)))
        levels.append(np.float32(0.5 * (zw[gaps[k]] + zw[gaps[k] + 1])))
        gaps, shown = np.delete(gaps, k), np.delete(shown, k)
    return np.array(levels, np.float32)


def four_level_plane(levels, W, H):
    """quadrants around (BORDER_X, BORDER_Y), one level each"""
    assert len(levels) == 4 and W > BORDER_X and H > BORDER_Y, (len(levels), W, H)
    plane = np.empty((H, W), np.float32)
    plane[:BORDER_Y, :BORDER_X], plane[:BORDER_Y, BORDER_X:] = levels[0], levels[1]
    plane[BORDER_Y:, :BORDER_X], plane[BORDER_Y:, BORDER_X:] = levels[2], levels[3]
    return plane


def ramp_plane(lo, hi, W, H):
    """a smooth ramp in x from lo (left) to hi (right): one value per column"""
    col = (np.float64(lo) + (np.float64(hi) - np.float64(lo)) * (np.arange(W) + 0.5) / W).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(col, (H, W)))


def blocks_plane(levels, W, H):
    """the four-level plane with a NaN, a 0, a +inf and a 2.0 block in it: d0 = 0, 0, 1, 1"""
    plane = four_level_plane(levels, W, H)
    plane[4:12, 6:30] = np.nan
    plane[30:41, 10:22] = 0.0
    plane[25:52, 50:70] = np.inf
    plane[2:20, 60:90] = 2.0
    return plane


def assert_plane_is_testable(splats, plane, shares=True):
    """for every value the plane holds: MARGIN away from every drawn splat's z_w and (shares) hiding 10 % .. 90 % of them"""
    zw = window_depth(splats)[splats["reject"] == 0].astype(np.float64)
    for v in np.unique(plane):
        assert np.abs(zw - np.float64(v)).min() >= MARGIN, "level %.9g is within 2^-20 of a drawn splat's z_w" % v
        if shares:
            hidden = (~(zw < np.float64(v))).mean()
            assert 0.1 <= hidden <= 0.9, "level %.9g hides %.3f of the drawn splats" % (v, hidden)


def hand_placed_ramp():
    """the ramp of the hand-placed scene: from in front of the nearest splat to behind the farthest, no column within 2^-20 of a z_w"""
    _, W, H, _ = hand_placed()
    zw = window_depth(hand_placed_splats())
    plane = ramp_plane(zw.min() - np.float32(0.01), zw.max() + np.float32(0.01), W, H)
    assert_plane_is_testable(hand_placed_splats(), plane, shares=False)
    return plane


@functools.lru_cache(maxsize=None)
def four_levels(name):
    """(plane, levels) of a scene's view: the four-level plane whose levels tests/test_occluded.py found testable"""
    _, W, H, _ = view_of(name)
    splats, _ = scene_splats(name)
    levels = choose_levels(splats)
    plane = four_level_plane(levels, W, H)
    assert_plane_is_testable(splats, plane)
    plane.setflags(write=False)
    return plane, levels


@functools.lru_cache(maxsize=None)
def small_viewport_case(W, H):
    """the "sparse" cloud in a small viewport behind a plane of two levels, left and right of the middle column: (cloud, view,
    the oracle's splats, plane, levels); the levels are testable (asserted here, on the CPU)"""
    cloud = scene("sparse")[0]
    view = cam, proj, vp, nf = scenes.default_view(W, H, z=7.0)
    ref = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=4, want_image=False, want_splats=True)
    splats = ref["splats"]
    levels = choose_levels(splats, (0.3, 0.7))
    plane = np.empty((H, W), np.float32)
    plane[:, :W // 2], plane[:, W // 2:] = levels[0], levels[1]
    assert_plane_is_testable(splats, plane)
    splats.setflags(write=False)
    plane.setflags(write=False)
    return cloud, view, splats, plane, levels


def d0_of(plane):
    """what the depth attachment holds, as the depth plane's destination: the 8-bit targets' clamp rule, NaN -> 0 (float32 in and out)"""
    o = np.asarray(plane, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(o > 0, np.where(o > 1, np.float32(1), o), np.float32(0)).astype(np.float32)


# ---- the oracle recipes ------------------------------------------------------------------------------------------------------

def read_only(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def composite_pair(splats, W, H, rgb=None, nthreads=16):
    """The oracle's frame of orc.project'ed splats in draw order -- in their own colours, or recoloured with `rgb` -- and its frame
    of the same splats in white: (colour frame, white frame = 1 - T_ref in every colour channel, T_ref in float64, the colour
    frame's threshold-flip budget, the white frame's)"""
    if rgb is not None:
        splats = splats.copy()
        splats["rgb"] = rgb
    C, bud_c = orc.composite_flip(splats, W, H, nthreads=nthreads)
    white = splats.copy()
    white["rgb"] = 1.0
    cover, bud_w = orc.composite_flip(white, W, H, nthreads=nthreads)
    return C, cover, 1.0 - cover[..., 0].astype(np.float64), bud_c, bud_w


def levels_in_front(splats, plane):
    """per level v of a plane with few distinct values: (the pixels that hold v, the splats with z_w < v in draw order).  A NaN
    hides everything and a level with nothing in front shows nothing: those pixels keep what the caller started from"""
    zw = window_depth(splats)
    for v in np.unique(plane[~np.isnan(plane)]):
        front = splats[zw < v]
        if front.shape[0]:
            yield plane == v, front


@functools.lru_cache(maxsize=None)
def oracle_layers(name):
    """C_ref (with alpha 1 - T_ref), T_ref and the two threshold-flip budgets of a scene's view, computed once"""
    _, W, H, _ = view_of(name)
    splats, V = scene_splats(name)
    C_ref, cover, T_ref, bud_c, bud_w = composite_pair(splats, W, H)
    layer = C_ref.astype(np.float64)
    layer[..., 3] = cover[..., 0]                           # 1 - T_ref
    return read_only(dict(V=V, layer=layer, T=T_ref, bud_c=bud_c.astype(np.float64), bud_w=bud_w.astype(np.float64), cover=cover))


def depth_layers(splats, W, H, nthreads=16):
    """The reference depth plane of orc.project'ed splats in draw order (orc.render_frame(..., want_splats=True)["splats"]):
    D_ref = the oracle's composite of the splats recoloured with their window depth, T_ref = 1 - its composite of the splats
    recoloured white; the plane is D_ref + T_ref.  Also: z_w per splat, the coverage 1 - T_ref and both threshold-flip budgets."""
    zw = window_depth(splats)
    D, cover, T, bud_d, bud_w = composite_pair(splats, W, H, rgb=zw[:, None], nthreads=nthreads)
    return read_only(dict(zw=zw, plane=D[..., 0].astype(np.float64) + T, T=T, cover=cover[..., 0].astype(np.float64),
                          bud_d=bud_d.astype(np.float64), bud_w=bud_w.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def oracle_plane(name):
    cloud, W, H, (cam, proj, vp, nf) = case(name)
    ref = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=16, want_image=False, want_splats=True)
    L = dict(depth_layers(ref["splats"], W, H, nthreads=16))
    L["V"] = ref["V"]
    L["visible"] = ref["splats"]["reject"] == 0
    return L


def occluded_reference(splats, plane, W, H, nthreads=16):
    """The reference frame of orc.project'ed splats in draw order behind `plane` (few distinct values): per level the pair of the
    splats in front of it, stitched by region.  Returns what tests/checks.check_over takes: layer = (C_ref, 1 - T_ref),
    T = T_ref, the two threshold-flip budgets."""
    assert plane.shape == (H, W) and plane.dtype == np.float32, (plane.shape, plane.dtype)
    layer, T = np.zeros((H, W, 4)), np.ones((H, W))
    bud_c, bud_w = np.zeros((H, W)), np.zeros((H, W))
    for region, front in levels_in_front(splats, plane):
        C, cover, t, bc, bw = composite_pair(front, W, H, nthreads=nthreads)
        layer[region, :3] = C[region, :3]
        layer[region, 3] = cover[region, 0]
        T[region] = t[region]
        bud_c[region], bud_w[region] = bc[region], bw[region]
    return read_only(dict(layer=layer, T=T, bud_c=bud_c, bud_w=bud_w))


def layers_reference(splats, plane, W, H, nthreads=16):
    """The reference depth plane of orc.project'ed splats in draw order behind `plane` (few distinct values), in the form
    tests/checks.check_plane takes: per level depth_layers (the pair with the window depth as the colour) of the splats in front
    of it, plane = D_ref + T_ref * d0 per region, T, and the two threshold-flip budgets (the white frame's scaled by d0 <= 1,
    like |dst| in check_over)."""
    assert plane.shape == (H, W) and plane.dtype == np.float32, (plane.shape, plane.dtype)
    d0 = d0_of(plane).astype(np.float64)
    out_plane, T = d0.copy(), np.ones((H, W))                    # (where nothing is seen the plane keeps d0, T 1)
    bud_d, bud_w = np.zeros((H, W)), np.zeros((H, W))
    for region, front in levels_in_front(splats, plane):
        L = depth_layers(front, W, H, nthreads=nthreads)
        D = L["plane"] - L["T"]                                  # depth_layers hands out D + T
        out_plane[region] = D[region] + L["T"][region] * d0[region]
        T[region] = L["T"][region]
        bud_d[region], bud_w[region] = L["bud_d"][region], L["bud_w"][region] * d0[region]
    return read_only(dict(plane=out_plane, T=T, bud_d=bud_d, bud_w=bud_w, d0=d0))


@functools.lru_cache(maxsize=None)
def reference_layers(name):
    _, W, H, _ = view_of(name)
    return occluded_reference(scene_splats(name)[0], four_levels(name)[0].copy(), W, H)


@functools.lru_cache(maxsize=None)
def reference_plane(name):
    _, W, H, _ = view_of(name)
    return layers_reference(scene_splats(name)[0], four_levels(name)[0].copy(), W, H)


def definition_f64(splats, plane, W, H):
    """the definition, in float64, front to back over the draw order reversed (the array is far -> near); w and its discard as
    splat_frag.glsl:18-42 define them, GL_LESS against the plane per pixel.  Returns (layer = (C, 1 - T), T)."""
    fx, fy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    zw = window_depth(splats)
    C, T = np.zeros((H, W, 3)), np.ones((H, W))
    for s, z in zip(splats[::-1], zw[::-1]):
        dx, dy = fx - float(s["px"]), fy - float(s["py"])
        inv = s["inv"].astype(np.float64)
        q = dx * (inv[0] * dx + inv[2] * dy) + dy * (inv[1] * dx + inv[3] * dy)
        w = float(s["alpha"]) * np.exp(-0.5 * q)
        w[w <= 1.0 / 256.0] = 0.0
        w[~(z < plane)] = 0.0                                    # float32 against float32, NaN included
        C += (T * w)[..., None] * s["rgb"].astype(np.float64)
        T *= 1.0 - w
    return np.concatenate([C, (1.0 - T)[..., None]], axis=-1), T


def definition_depth_f64(splats, plane, W, H):
    """the definition of the combined depth plane, in float64: definition_f64's walk with the window depth as the colour, over
    d0.  Returns (depth, T)."""
    z = splats.copy()
    z["rgb"] = window_depth(splats)[:, None]
    layer, T = definition_f64(z, plane, W, H)
    return np.minimum(layer[..., 0] + T * d0_of(plane).astype(np.float64), 1.0), T


# ---- fixtures of the point, covariance and cloud-storage tests ---------------------------------------------------------------

def smooth_sprite(w, h, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.hypot((xx + 0.5) / w * 2 - 1, (yy + 0.5) / h * 2 - 1)
    t = np.zeros((h, w, 4), np.float64)
    t[..., 0] = 0.5 + 0.5 * np.sin(xx * 0.3)
    t[..., 1] = (yy + 0.5) / h                       # vertical gradient: catches a missing row flip
    t[..., 2] = 0.5 + 0.5 * np.cos(d * 5)
    t[..., 3] = np.clip((1 - d) * 6, 0, 1)
    t[..., :3] = np.clip(t[..., :3] + rng.normal(0, 0.02, size=(h, w, 3)), 0, 1)
    return (t * 255 + 0.5).astype(np.uint8)


def random_points(n, seed):
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 8), np.float32)
    pts[:, :3] = rng.normal(0, 1.2, size=(n, 3))
    pts[:, 3] = 1.0
    pts[:, 4:7] = rng.integers(0, 256, size=(n, 3)).astype(np.float32) / np.float32(255.0)
    pts[:, 7] = 1.0
    return pts


def _covariance_by_rodrigues(rot, log_scale):
    """Sigma = sum_i s_i^2 (R e_i)(R e_i)^T with R e_i from Rodrigues' rotation formula about the quaternion's axis, in float64 --
    no quaternion-to-matrix closed form, no matrix products: independent of the restatements of glm's mat3_cast it checks"""
    q = np.asarray(rot, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)                 # glm::normalize (gaussiancloud.cpp:88-89); rot = (w, x, y, z)
    w, v = q[:, 0], q[:, 1:]
    sin_half = np.linalg.norm(v, axis=1)
    angle = 2.0 * np.arctan2(sin_half, w)
    axis = v / np.maximum(sin_half, 1e-300)[:, None]
    s2 = np.exp(np.asarray(log_scale, np.float64)) ** 2              # scale = exp(log_scale) (gaussiancloud.cpp:254-361)
    sigma = np.zeros((q.shape[0], 3, 3))
    for i in range(3):
        e = np.zeros((q.shape[0], 3)); e[:, i] = 1.0
        c, s = np.cos(angle)[:, None], np.sin(angle)[:, None]
        re = e * c + np.cross(axis, e) * s + axis * (axis * e).sum(1, keepdims=True) * (1.0 - c)
        sigma += s2[:, i, None, None] * re[:, :, None] * re[:, None, :]
    return sigma


# byte offsets of the 16 attributes in the reference's 61-float record
AOS_OFF = (0, 16, 32, 48, 64, 76, 88, 100, 116, 132, 148, 164, 180, 196, 212, 228)


def ply_layout():
    """msplat_ply_layout of synthetic.write_ply's 62-float vertex"""
    L = _capi.PlyLayout()
    L.vertex_size = 62 * 4
    L.x, L.y, L.z = 0, 4, 8
    for i in range(3):
        L.f_dc[i] = 24 + 4 * i
    for i in range(45):
        L.f_rest[i] = 36 + 4 * i
    L.opacity = 216
    for i in range(3):
        L.scale[i] = 220 + 4 * i
    for i in range(4):
        L.rot[i] = 232 + 4 * i
    return L


def sh_basis_bounds():
    """beta_k = max over unit v of |b_k(v)| for project_block's 16 basis functions (dense sphere sampling, 1e-3 margin)"""
    th = np.linspace(0.0, np.pi, 1201)[:, None]
    ph = np.linspace(0.0, 2 * np.pi, 2401)[None, :]
    vx, vy, vz = np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th) * np.ones_like(ph)
    k1, k2, k3, k4 = 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
    k5, k6, k7, k8, k9 = 0.5900435899266435, 2.8906114426405543, 0.4570457994644658, 0.37317633259011546, 1.4453057213202771
    b = [np.full_like(vx, 0.28209479177387814), -k1 * vy, k1 * vz, -k1 * vx,
         k2 * vy * vx, -k2 * vy * vz, k3 * (3 * vz * vz - 1), -k2 * vx * vz, k4 * (vx * vx - vy * vy),
         -k5 * vy * (3 * vx * vx - vy * vy), k6 * vy * vx * vz, -k7 * vy * (5 * vz * vz - 1), k8 * vz * (5 * vz * vz - 3),
         -k7 * vx * (5 * vz * vz - 1), k9 * vz * (vx * vx - vy * vy), -k5 * vx * (vx * vx - 3 * vy * vy)]
    return np.array([np.abs(x).max() for x in b]) * 1.001
