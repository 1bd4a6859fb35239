"""CPU side of msplat_render_layers / msplat_render_stereo_layers: the entry points are declared, exported and bound, refuse a NULL
context without touching a device, the group refuses, and the oracle recipe the GPU tests compare the combined depth plane against
(tests/render_cases.layers_reference) is pinned by a float64 restatement of the definition:

    depth[p] = min(fma(T, d0, sum_{i: z_i < o} T_i w_i z_i), 1),   o = occluder[p],  d0 = o > 0 ? (o > 1 ? 1 : o) : 0  (NaN -> 0)

-- the expected window depth of the splats that pass GL_LESS against the plane, blended over what the depth attachment holds.
The recipe never changes the oracle: per level v of a plane with a few distinct values, tests/render_cases.depth_layers of the
splats with z_w < v gives D and T, and the region of v reads D + T * d0(v).  The conditions the GPU tests lean on (every level well
away from every drawn splat's z_w) are asserted here, where they can fail without a GPU."""
import inspect
import os
import re

import numpy as np

from splatapult_amd import MsplatError, SplatRenderer, SplatRendererGroup, _capi, camera
from tests.render_cases import (SMALL_VIEWPORTS, assert_plane_is_testable, blocks_plane, choose_levels, d0_of, definition_depth_f64,
                                definition_f64, depth_layers, four_level_plane, hand_placed, hand_placed_ramp, hand_placed_splats,
                                layers_reference, small_viewport_case, window_depth)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------

N_ARGS = {"msplat_render_layers": 12, "msplat_render_stereo_layers": 17}


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    bound = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    for name, nargs in N_ARGS.items():
        assert re.search(r"\bint %s\(msplat_ctx\*" % name, header), name
        assert name in bound, name
        res, args = bound[name]
        assert res is _capi.C.c_int and len(args) == nargs
        fn = getattr(_capi.lib(), name)                      # the in-tree library exports it
        assert fn.argtypes == args
    # msplat_render's eight + two planes with their pitches; msplat_render_stereo's eleven + two pairs of planes with their pitches
    assert N_ARGS["msplat_render_layers"] == 8 + 4 and N_ARGS["msplat_render_stereo_layers"] == 11 + 6
    for cls in (SplatRenderer, SplatRendererGroup):
        assert callable(cls.RenderLayers) and callable(cls.RenderStereoLayers)
    want = {"depth", "depth_ptr", "depth_pitch_bytes", "occluder", "occluder_ptr", "occluder_pitch_bytes", "out", "out_ptr", "pitch_bytes"}
    assert want <= set(inspect.signature(SplatRenderer.RenderLayers).parameters)
    want = {"out_ptrs", "pitch_bytes", "depth_ptrs", "depth_pitch_bytes", "occluder_ptrs", "occluder_pitch_bytes"}
    assert want <= set(inspect.signature(SplatRenderer.RenderStereoLayers).parameters)
    # the header no longer calls the combination out of scope
    assert "msplat_render_depth's output in the same frame, seeding" not in header
    shim = open(os.path.join(ROOT, "splatapult_amd", "host", "msplat_host.hpp")).read()
    assert "void RenderLayers(" in shim and "void RenderStereoLayers(" in shim


def test_a_null_context_is_an_invalid_argument():
    f = np.zeros(16, np.float32)
    p = f.ctypes.data_as(_capi.C.POINTER(_capi.C.c_float))
    img, z, o = np.zeros((4, 4, 4), np.float32), np.zeros((4, 4), np.float32), np.ones((4, 4), np.float32)
    L = _capi.lib()
    for d, oc in ((z.ctypes.data, o.ctypes.data), (None, o.ctypes.data), (z.ctypes.data, None), (None, None)):
        assert L.msplat_render_layers(None, p, p, p, p, img.ctypes.data, 0, d, 0, oc, 0, 0) == _capi.ERR_INVALID_ARG
        assert L.msplat_last_error(None)
        assert L.msplat_render_stereo_layers(None, p, p, p, p, p, p, img.ctypes.data, img.ctypes.data, 0, d, d, 0, oc, oc, 0, 0) == _capi.ERR_INVALID_ARG
        assert L.msplat_render_stereo_layers(None, p, p, p, p, p, p, img.ctypes.data, img.ctypes.data, 0, d, d, 0, oc, oc, 0, 1) == _capi.ERR_INVALID_ARG
    assert (img == 0).all() and (z == 0).all() and (o == 1).all()


def test_the_group_refuses_before_it_touches_a_device():
    g = SplatRendererGroup([0])
    view = (camera.pose((0.0, 0.0, 4.0)), camera.perspective(camera.FOVY, 1.5), [0, 0, 48, 32], [0.1, 100.0])
    plane = np.ones((32, 48), np.float32)
    calls = [lambda: g.RenderLayers(*view, depth=True, occluder=plane), lambda: g.RenderLayers(*view, out_ptr=1, depth_ptr=1, occluder_ptr=1),
             lambda: g.RenderLayers(*view), lambda: g.RenderStereoLayers([view[0]] * 2, [view[1]] * 2, view[2], view[3], out_ptrs=[1, 1],
                                                                         depth_ptrs=[1, 1], occluder_ptrs=[1, 1])]
    for call in calls:
        try:
            call()
        except MsplatError as e:
            assert e.code == _capi.ERR_UNSUPPORTED and "layers" in str(e)
        else:
            raise AssertionError("the group took a layers frame")


def test_render_keeps_refusing_both_planes_and_names_the_call_that_takes_them():
    r = SplatRenderer()
    view = (camera.pose((0.0, 0.0, 4.0)), camera.perspective(camera.FOVY, 1.5), [0, 0, 48, 32], [0.1, 100.0])
    try:
        r.Render(*view, depth=True, occluder=np.ones((32, 48), np.float32))
    except MsplatError as e:
        assert e.code == _capi.ERR_UNSUPPORTED and "occluder" in str(e) and "RenderLayers" in str(e)
    else:
        raise AssertionError("Render took both planes")


def test_d0_is_the_clamp_rule():
    o = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 2.0 ** -130, 0.25, 1.0, np.nextafter(np.float32(1), np.float32(2)), 2.0, np.inf], np.float32)
    want = np.array([0, 0, 0, 0, 0, 2.0 ** -130, 0.25, 1, 1, 1, 1], np.float32)
    got = d0_of(o)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()


def test_the_oracle_recipe_is_the_definition():
    _, W, H, _ = hand_placed()
    splats = hand_placed_splats()
    zw = window_depth(splats)
    levels = choose_levels(splats)
    assert_plane_is_testable(splats, four_level_plane(levels, W, H))
    blocks = blocks_plane(levels, W, H)
    finite = blocks[np.isfinite(blocks) & (blocks != 0.0) & (blocks != 2.0)]
    assert np.unique(finite).size == 4 and np.isnan(blocks).any() and (blocks == 0).any() and np.isposinf(blocks).any() and (blocks == 2).any()
    # every value the plane holds keeps its distance from every z_w (NaN holds none; 0, 2 and +inf are far from [0.625, 1])
    assert_plane_is_testable(splats, blocks[~np.isnan(blocks)], shares=False)
    ramp = hand_placed_ramp()
    assert np.unique(ramp).size == W and (ramp[0, 0] < zw).all() and (ramp[0, -1] > zw).all()      # from all hidden to all shown
    for plane in (blocks, ramp):
        L = layers_reference(splats, plane, W, H, nthreads=4)
        depth, T = definition_depth_f64(splats, plane, W, H)
        # tests/test_depth_output.py's tolerance: float32 against float64 over at most eight blends of values <= 1, and a fragment
        # within 1e-4 of the discard threshold may fall on either side: the oracle's own flip budgets cover that
        tol = 8 * 4 * 2.0 ** -24 + L["bud_d"] + L["bud_w"]
        assert (np.abs(L["T"] - T) <= tol).all(), np.abs(L["T"] - T).max()
        assert (np.abs(L["plane"] - depth) <= tol).all(), np.abs(L["plane"] - depth).max()
        assert L["plane"].min() >= 0.0 and L["plane"].max() <= 1.0
        untouched = L["T"] == 1.0
        assert untouched.any() and (L["plane"][untouched] == L["d0"][untouched]).all() and (depth[untouched] == L["d0"][untouched]).all()
    # the closed blocks read exactly 0, the open ones msplat_render_depth's plane
    L = layers_reference(splats, blocks, W, H, nthreads=4)
    closed = np.isnan(blocks) | (blocks == 0.0)
    assert (L["plane"][closed] == 0.0).all() and (L["T"][closed] == 1.0).all()
    full = depth_layers(splats, W, H, nthreads=4)
    opened = np.isposinf(blocks) | (blocks == 2.0)
    np.testing.assert_array_equal(L["plane"][opened], full["plane"][opened])
    assert (full["T"][opened] < 0.5).any()                                     # ... where splats are seen
    # an open plane everywhere is msplat_render_depth's recipe, a closed one the plane of zeros
    everywhere = layers_reference(splats, np.full((H, W), np.inf, np.float32), W, H, nthreads=4)
    np.testing.assert_array_equal(everywhere["plane"], full["plane"])
    np.testing.assert_array_equal(layers_reference(splats, np.full((H, W), np.nan, np.float32), W, H, nthreads=4)["plane"], np.zeros((H, W)))
    # the plane matters, and so does d0: the four-level depth differs from both the unoccluded plane and the occluded sum over 1.0
    four = four_level_plane(levels, W, H)
    depth4, T4 = definition_depth_f64(splats, four, W, H)
    assert np.abs(depth4 - full["plane"]).max() > 0.05
    z = splats.copy()
    z["rgb"] = zw[:, None]
    over_one = definition_f64(z, four, W, H)[0][..., 0] + T4
    assert np.abs(depth4 - over_one).max() > 0.05


def test_the_small_viewports_of_the_gpu_tests_have_testable_levels():
    for W, H in SMALL_VIEWPORTS:
        _, _, splats, plane, levels = small_viewport_case(W, H)
        assert np.unique(plane).size == 2 and levels[0] != levels[1]
        print("%d x %d: drawn %d, levels %s" % (W, H, int((splats["reject"] == 0).sum()), levels))
