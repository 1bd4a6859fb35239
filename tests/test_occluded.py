"""CPU side of msplat_render_occluded: the entry point is exported and bound, refuses a NULL context without touching a device, and
the oracle recipe the GPU tests compare against (tests/render_cases.occluded_reference) is pinned by a float64 numpy restatement
of the definition:

    per pixel p the frame is msplat_render's with every splat i with !(z_i < plane[p]) absent at p,   z_i = 0.5 ndc.z + 0.5.

The recipe never changes the oracle: for a plane with a few distinct levels, the pixels of level v are those of the oracle's frame
of the splats with z_w < v (orc.composite_flip on a subset of the orc.project'ed splats), and the white frame of the same subset
gives 1 - T, as tests/render_cases.oracle_layers does for MSPLAT_TARGET_LOAD.  The conditions the GPU tests lean on -- every level
well away from every drawn splat's z_w, every level hiding and showing a fair share of the splats -- are asserted here, where they
can fail without a GPU."""
import inspect
import os
import re

import numpy as np

from splatapult_amd import MsplatError, SplatRenderer, SplatRendererGroup, _capi, camera
from tests.render_cases import (assert_plane_is_testable, choose_levels, definition_f64, depth_layers, four_level_plane, hand_placed,
                                hand_placed_ramp, hand_placed_splats, occluded_reference, scene_splats, view_of, window_depth)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
        # tests/test_depth_output.py's tolerance: float32 against float64 over at most eight blends of values <= 1, and a fragment
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


def test_the_scenes_of_the_gpu_tests_have_testable_levels():
    for name in ("sparse", "hard", "dense"):
        _, W, H, _ = view_of(name)
        splats, V = scene_splats(name)
        levels = choose_levels(splats)
        assert np.unique(levels).size == 4
        assert_plane_is_testable(splats, four_level_plane(levels, W, H))
        drawn = int((splats["reject"] == 0).sum())
        print("%s: V %d, drawn %d, levels %s" % (name, V, drawn, levels))
