"""CPU side of msplat_render_depth: the entry point is exported and bound, refuses a NULL context without touching a device, and the
oracle recipe the GPU tests compare against (tests/render_cases.depth_layers) is pinned by a numpy restatement of the
definition

    depth = sum_i T_i w_i z_i + T * 1.0,      z_i = 0.5 ndc.z + 0.5,  T_i = prod_{j nearer} (1 - w_j),  T = the product over all

on a handful of hand-placed splats.  The recipe never changes the oracle: window depth is composited as one more colour (the blend
is linear in colour) and the white frame gives 1 - T, as tests/render_cases.oracle_layers does for MSPLAT_TARGET_LOAD."""
import inspect
import os
import re

import numpy as np

from oracle import oracle as orc
from splatapult_amd import MsplatError, SplatRenderer, SplatRendererGroup, _capi, camera
from tests.render_cases import depth_layers, hand_placed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    assert re.search(r"\bint msplat_render_depth\(msplat_ctx\* ctx,", header)
    bound = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    assert "msplat_render_depth" in bound
    res, args = bound["msplat_render_depth"]
    assert res is _capi.C.c_int and len(args) == 10          # msplat_render's eight + the plane and its pitch
    fn = _capi.lib().msplat_render_depth                      # the in-tree library exports it
    assert fn.argtypes == args
    for cls in (SplatRenderer, SplatRendererGroup):
        assert {"depth", "depth_ptr", "depth_pitch_bytes"} <= set(inspect.signature(cls.Render).parameters)


def test_a_null_context_is_an_invalid_argument():
    f = np.zeros(16, np.float32)
    p = f.ctypes.data_as(_capi.C.POINTER(_capi.C.c_float))
    img, z = np.zeros((4, 4, 4), np.float32), np.zeros((4, 4), np.float32)
    L = _capi.lib()
    assert L.msplat_render_depth(None, p, p, p, p, img.ctypes.data, 0, z.ctypes.data, 0, 0) == _capi.ERR_INVALID_ARG
    assert L.msplat_last_error(None)
    assert L.msplat_render_depth(None, p, p, p, p, img.ctypes.data, 0, None, 0, 0) == _capi.ERR_INVALID_ARG      # msplat_render's answer


def test_the_group_refuses_a_depth_plane_before_it_touches_a_device():
    g = SplatRendererGroup([0])
    view = (camera.pose((0.0, 0.0, 4.0)), camera.perspective(camera.FOVY, 1.5), [0, 0, 48, 32], [0.1, 100.0])
    for kw in (dict(depth=True), dict(depth=np.zeros((32, 48), np.float32)), dict(out_ptr=1, depth_ptr=1)):
        try:
            g.Render(*view, **kw)
        except MsplatError as e:
            assert e.code == _capi.ERR_UNSUPPORTED and "depth" in str(e)
        else:
            raise AssertionError("the group took %s" % sorted(kw))


def test_the_oracle_recipe_is_the_definition():
    aos, W, H, (cam, proj, vp, nf) = hand_placed()
    ref = orc.render_frame(aos, False, cam, proj, vp, nf, nthreads=4, want_image=False, want_splats=True)
    splats = ref["splats"]
    assert ref["V"] == aos.shape[0] and (splats["reject"] == 0).all()         # all eight are drawn
    L = depth_layers(splats, W, H, nthreads=4)
    assert L["zw"].min() >= 0.625 and L["zw"].max() <= 1.0 and L["zw"].max() - L["zw"].min() > 0.25
    # the definition, in float64, front to back over the draw order reversed (the array is far -> near); w and its discard as
    # splat_frag.glsl:18-42 define them
    fx, fy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    depth, T = np.zeros((H, W)), np.ones((H, W))
    for s in splats[::-1]:
        dx, dy = fx - float(s["px"]), fy - float(s["py"])
        inv = s["inv"].astype(np.float64)
        q = dx * (inv[0] * dx + inv[2] * dy) + dy * (inv[1] * dx + inv[3] * dy)
        w = float(s["alpha"]) * np.exp(-0.5 * q)
        w[w <= 1.0 / 256.0] = 0.0
        z = 0.5 * float(s["ndc"][2]) + 0.5
        depth += T * w * z
        T *= 1.0 - w
    want = depth + T * 1.0
    # float32 against float64 over at most eight blends of values <= 1, and a fragment within 1e-4 of the discard threshold may
    # fall on either side: the oracle's own flip budgets (colour z over dst 1) cover that
    tol = 8 * 4 * 2.0 ** -24 + L["bud_d"] + L["bud_w"]
    assert (np.abs(L["T"] - T) <= tol).all(), np.abs(L["T"] - T).max()
    assert (np.abs(L["plane"] - want) <= tol).all(), np.abs(L["plane"] - want).max()
    untouched = L["cover"] == 0.0
    assert untouched.any() and (L["plane"][untouched] == 1.0).all() and (want[untouched] == 1.0).all()
    assert (L["cover"] > 0.99).any() and L["plane"].min() < 0.8                # an opaque splat in front: the plane reads its z_w
    assert L["plane"].min() >= 0.0 and L["plane"].max() <= 1.0
