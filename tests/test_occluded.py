"""CPU side of msplat_render_occluded: the entry point is exported and bound, refuses a NULL context without touching a device, and
the oracle recipe the GPU tests compare against (tests/test_gpu_occluded.py imports the helpers below) is pinned by a float64 numpy
restatement of the definition:

    per pixel p the frame is msplat_render's with every splat i with !(z_i < plane[p]) absent at p,   z_i = 0.5 ndc.z + 0.5.

The recipe never changes the oracle: for a plane with a few distinct levels, the pixels of level v are those of the oracle's frame
of the splats with z_w < v (orc.composite_flip on a subset of the orc.project'ed splats), and the white frame of the same subset
gives 1 - T, as tests/test_gpu_target_mode.py does for MSPLAT_TARGET_LOAD.  The conditions the GPU tests lean on -- every level
well away from every drawn splat's z_w, every level hiding and showing a fair share of the splats -- are asserted here, where they
can fail without a GPU."""
import functools
import inspect
import os
import re

import numpy as np

from oracle import oracle as orc
from splatapult_amd import MsplatError, SplatRenderer, SplatRendererGroup, _capi, camera
from tests.test_depth_output import depth_layers, hand_placed
from tests.test_gpu_target_mode import view_of          # (importing the module needs no GPU: the scenes are built on the host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The GPU's z_w may differ from the oracle's in the last bits (z_w < 1: an ulp is <= 2^-24); a splat on the wrong side of a level
# is not a rounding error, so every level keeps this distance from every drawn splat's z_w
MARGIN = 2.0 ** -20
BORDER_X, BORDER_Y = 37, 21          # the four-level plane's region borders: inside a 16 x 4 strip of the compositor's tiles


def window_depth(splats):
    """z_w per orc.project'ed splat, as tests/test_depth_output.depth_layers computes it (project_kernel's arithmetic)"""
    zw = np.float32(0.5) * splats["ndc"][:, 2] + np.float32(0.5)
    assert zw.dtype == np.float32
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
    assert len(levels) == 4 and W > BORDER_X and H > BORDER_Y
    plane = np.empty((H, W), np.float32)
    plane[:BORDER_Y, :BORDER_X], plane[:BORDER_Y, BORDER_X:] = levels[0], levels[1]
    plane[BORDER_Y:, :BORDER_X], plane[BORDER_Y:, BORDER_X:] = levels[2], levels[3]
    return plane


def ramp_plane(lo, hi, W, H):
    """a smooth ramp in x from lo (left) to hi (right): one value per column"""
    col = (np.float64(lo) + (np.float64(hi) - np.float64(lo)) * (np.arange(W) + 0.5) / W).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(col, (H, W)))


def assert_plane_is_testable(splats, plane, shares=True):
    """the conditions above for every value the plane holds"""
    zw = window_depth(splats)[splats["reject"] == 0].astype(np.float64)
    for v in np.unique(plane):
        assert np.abs(zw - np.float64(v)).min() >= MARGIN, "level %.9g is within 2^-20 of a drawn splat's z_w" % v
        if shares:
            hidden = (~(zw < np.float64(v))).mean()
            assert 0.1 <= hidden <= 0.9, "level %.9g hides %.3f of the drawn splats" % (v, hidden)


def occluded_reference(splats, plane, W, H, nthreads=16):
    """The reference frame of orc.project'ed splats in draw order behind `plane` (few distinct values): per level v the oracle's
    composite of the splats with z_w < v and of the same splats recoloured white, stitched by region.  Returns what
    tests/test_gpu_target_mode.check_over takes: layer = (C_ref, 1 - T_ref), T = T_ref, the two threshold-flip budgets."""
    assert plane.shape == (H, W) and plane.dtype == np.float32
    zw = window_depth(splats)
    layer, T = np.zeros((H, W, 4)), np.ones((H, W))
    bud_c, bud_w = np.zeros((H, W)), np.zeros((H, W))
    levels = np.unique(plane[~np.isnan(plane)])
    for v in levels:                                             # (a NaN hides everything: the region keeps layer 0, T 1)
        region = plane == v
        front = splats[zw < v]                                   # draw order kept
        if front.shape[0] == 0:
            continue
        C, bc = orc.composite_flip(front, W, H, nthreads=nthreads)
        white = front.copy()
        white["rgb"] = 1.0
        cover, bw = orc.composite_flip(white, W, H, nthreads=nthreads)
        layer[region, :3] = C[region, :3]
        layer[region, 3] = cover[region, 0]
        T[region] = 1.0 - cover[region, 0].astype(np.float64)
        bud_c[region], bud_w[region] = bc[region], bw[region]
    out = dict(layer=layer, T=T, bud_c=bud_c, bud_w=bud_w)
    for a in out.values():
        a.setflags(write=False)
    return out


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


@functools.lru_cache(maxsize=None)
def hand_placed_splats():
    aos, W, H, (cam, proj, vp, nf) = hand_placed()
    ref = orc.render_frame(aos, False, cam, proj, vp, nf, nthreads=4, want_image=False, want_splats=True)
    splats = ref["splats"]
    assert ref["V"] == aos.shape[0] and (splats["reject"] == 0).all()         # all eight are drawn
    splats.setflags(write=False)
    return splats


def hand_placed_ramp():
    """the ramp of the hand-placed scene: from in front of the nearest splat to behind the farthest, no column within 2^-20 of a z_w"""
    _, W, H, _ = hand_placed()
    zw = window_depth(hand_placed_splats())
    plane = ramp_plane(zw.min() - np.float32(0.01), zw.max() + np.float32(0.01), W, H)
    assert_plane_is_testable(hand_placed_splats(), plane, shares=False)
    return plane


# ------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    assert re.search(r"\bint msplat_render_occluded\(msplat_ctx\* ctx,", header)
    bound = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    assert "msplat_render_occluded" in bound
    res, args = bound["msplat_render_occluded"]
    assert res is _capi.C.c_int and len(args) == 10          # msplat_render's eight + the plane and its pitch
    fn = _capi.lib().msplat_render_occluded                  # the in-tree library exports it
    assert fn.argtypes == args
    for cls in (SplatRenderer, SplatRendererGroup):
        assert {"occluder", "occluder_ptr", "occluder_pitch_bytes"} <= set(inspect.signature(cls.Render).parameters)


def test_a_null_context_is_an_invalid_argument():
    f = np.zeros(16, np.float32)
    p = f.ctypes.data_as(_capi.C.POINTER(_capi.C.c_float))
    img, z = np.zeros((4, 4, 4), np.float32), np.ones((4, 4), np.float32)
    L = _capi.lib()
    assert L.msplat_render_occluded(None, p, p, p, p, img.ctypes.data, 0, z.ctypes.data, 0, 0) == _capi.ERR_INVALID_ARG
    assert L.msplat_last_error(None)
    assert L.msplat_render_occluded(None, p, p, p, p, img.ctypes.data, 0, None, 0, 0) == _capi.ERR_INVALID_ARG   # msplat_render's answer


def test_the_group_refuses_an_occluder_plane_before_it_touches_a_device():
    g = SplatRendererGroup([0])
    view = (camera.pose((0.0, 0.0, 4.0)), camera.perspective(camera.FOVY, 1.5), [0, 0, 48, 32], [0.1, 100.0])
    for kw in (dict(occluder=np.ones((32, 48), np.float32)), dict(out_ptr=1, occluder_ptr=1), dict(occluder_ptr=1, occluder_pitch_bytes=256)):
        try:
            g.Render(*view, **kw)
        except MsplatError as e:
            assert e.code == _capi.ERR_UNSUPPORTED and "occluder" in str(e)
        else:
            raise AssertionError("the group took %s" % sorted(kw))


def test_the_oracle_recipe_is_the_definition():
    _, W, H, _ = hand_placed()
    splats = hand_placed_splats()
    zw = window_depth(splats)
    levels = choose_levels(splats)
    four = four_level_plane(levels, W, H)
    assert_plane_is_testable(splats, four)
    assert np.unique(four).size == 4
    ramp = hand_placed_ramp()
    assert np.unique(ramp).size == W and (ramp[0, 0] < zw).all() and (ramp[0, -1] > zw).all()      # from all hidden to all shown
    for plane in (four, ramp):
        L = occluded_reference(splats, plane, W, H, nthreads=4)
        layer, T = definition_f64(splats, plane, W, H)
        # tests/test_depth_output's tolerance: float32 against float64 over at most eight blends of values <= 1, and a fragment
        # within 1e-4 of the discard threshold may fall on either side: the oracle's own flip budgets cover that
        tol = 8 * 4 * 2.0 ** -24 + L["bud_c"] + L["bud_w"]
        assert (np.abs(L["T"] - T) <= tol).all(), np.abs(L["T"] - T).max()
        assert (np.abs(L["layer"] - layer) <= tol[..., None]).all(), np.abs(L["layer"] - layer).max()
    # the plane matters: the four-level frame differs from the unoccluded one where splats were hidden, and equals it nowhere by accident
    open_layer, _ = definition_f64(splats, np.full((H, W), np.inf, np.float32), W, H)
    four_layer, _ = definition_f64(splats, four, W, H)
    assert np.abs(open_layer - four_layer).max() > 0.05
    closed_layer, closed_T = definition_f64(splats, np.full((H, W), np.nan, np.float32), W, H)
    assert (closed_layer == 0).all() and (closed_T == 1).all()
    # an open plane is the plain recipe (depth_layers' white frame)
    full = occluded_reference(splats, np.full((H, W), 2.0, np.float32), W, H, nthreads=4)
    np.testing.assert_array_equal(full["T"], depth_layers(splats, W, H, nthreads=4)["T"])


@functools.lru_cache(maxsize=None)
def scene_splats(name):
    """the oracle's projected splats of a scene's view in draw order (read-only), V"""
    cloud, W, H, (cam, proj, vp, nf) = view_of(name)
    ref = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=16, want_image=False, want_splats=True)
    ref["splats"].setflags(write=False)
    return ref["splats"], ref["V"]


def test_the_scenes_of_the_gpu_tests_have_testable_levels():
    for name in ("sparse", "hard", "dense"):
        _, W, H, _ = view_of(name)
        splats, V = scene_splats(name)
        levels = choose_levels(splats)
        assert np.unique(levels).size == 4
        assert_plane_is_testable(splats, four_level_plane(levels, W, H))
        drawn = int((splats["reject"] == 0).sum())
        print("%s: V %d, drawn %d, levels %s" % (name, V, drawn, levels))
