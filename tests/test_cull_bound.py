"""The footprint bound of the conservative culls, on the host: FrameParams::view_scale2 as the library computes it
(msplat_debug_view_scale2: no context, no device) against the squared spectral norm it has to bound, and the per-splat bound
built on it (tests/cull_bound_rule.py, float64) against the footprint the projection defines -- for the hostile clouds and
every camera of tests/cull_cases.py.  A bound below the true extent is a splat missing from a frame."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import _capi
from tests import cull_cases as cc
from tests import scenes
from tests.cull_bound_rule import spectral2, splat_bound, true_extents

_FP = C.POINTER(C.c_float)
SLACK = 1e-5            # what view_scale2 may lie above sigma_max^2, relative: footprint_bound's own inflation, a decade above
                        # float32 rounding (6e-8) and the closed form's error in double


def library_view(cam):
    """inverse(cameraMat) as every frame computes it (float32)"""
    cam = np.ascontiguousarray(cam, np.float32)
    out = np.zeros(16, np.float32)
    _capi.lib().msplat_mat4_inverse(cam.ctypes.data_as(_FP), out.ctypes.data_as(_FP))
    return out


def library_view_scale2(view):
    view = np.ascontiguousarray(view, np.float32)
    out = np.full(1, -1.0, np.float32)
    assert _capi.lib().msplat_debug_view_scale2(view.ctypes.data_as(_FP), out.ctypes.data_as(_FP)) == _capi.OK
    return float(out[0])


def view_with(m3):
    """a view matrix with the upper-left 3x3 m3 (rows x columns) and some translation"""
    v = np.eye(4)
    v[:3, :3] = m3
    v[:3, 3] = (0.5, -2.0, 7.0)
    return v.T.astype(np.float32).reshape(16).copy()


def special_views():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(3), rng.standard_normal(3)
    g = rng.standard_normal((3, 3))
    yield "identity", view_with(np.eye(3))
    yield "rank 1", view_with(np.outer(a, b))
    yield "rank 1, one entry", view_with(np.outer([0.0, 1.0, 0.0], [0.0, 0.0, 3.0]))
    yield "entries of 1e-15", view_with(1e-15 * g)
    yield "entries of 1e+15", view_with(1e15 * g)
    yield "1e-15 next to 1e+15", view_with(g * np.array([[1e-15, 1.0, 1e15]]))
    yield "diag(1e-15, 1, 1e+15)", view_with(np.diag([1e-15, 1.0, 1e15]))
    yield "symmetric, two equal singular values", view_with(np.diag([2.0, 2.0, 1.0]))
    yield "three equal singular values, not symmetric", view_with(3.0 * np.linalg.qr(g)[0])


def test_the_header_declares_the_entry_and_the_binding_lists_it():
    import os
    import re
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, "include", "msplat_debug.h")).read()
    assert re.search(r"\bint\s+msplat_debug_view_scale2\s*\(\s*const\s+float\s+viewMat\[16\]\s*,\s*float\s*\*\s*out\s*\)\s*;", text)
    assert "msplat_debug_view_scale2" in {n for n, _, _ in _capi.SYMBOLS}
    one = np.zeros(1, np.float32)
    L = _capi.lib()
    assert L.msplat_debug_view_scale2(None, one.ctypes.data_as(_FP)) == _capi.ERR_INVALID_ARG
    assert L.msplat_debug_view_scale2(view_with(np.eye(3)).ctypes.data_as(_FP), None) == _capi.ERR_INVALID_ARG


def test_view_scale2_bounds_the_squared_spectral_norm_from_above_and_tightly():
    views = [(name, library_view(make(cc.W, cc.H)[0])) for name, make in cc.CAMERAS.items()] + list(special_views())
    assert len(views) == len(cc.CAMERA_NAMES) + 9
    for name, view in views:
        got, want = library_view_scale2(view), spectral2(view)
        print("view_scale2 %-45s library %.9g  sigma_max^2 %.9g  ratio - 1 = %.3g" % (name, got, want, got / want - 1.0))
        assert np.isfinite(got) and want > 0.0, (name, got, want)
        assert got >= want, "%s: view_scale2 %.9g is below sigma_max^2 %.9g" % (name, got, want)
        assert got <= want * (1.0 + SLACK), "%s: view_scale2 %.9g is more than 1e-5 above sigma_max^2 %.9g" % (name, got, want)


def test_view_scale2_of_a_zero_matrix_is_zero_and_junk_never_gives_a_finite_number():
    assert library_view_scale2(view_with(np.zeros((3, 3)))) == 0.0
    g = np.random.default_rng(6).standard_normal((3, 3))
    for bad in (np.nan, np.inf, -np.inf):
        for r in range(3):
            for c in range(3):
                for base in (g, np.eye(3), np.zeros((3, 3))):
                    m = base.copy()
                    m[r, c] = bad
                    got = library_view_scale2(view_with(m))
                    assert not np.isfinite(got), "a 3x3 with %s at (%d, %d) gives view_scale2 %.9g" % (bad, r, c, got)
    for bad in (np.nan, np.inf):
        assert not np.isfinite(library_view_scale2(view_with(np.full((3, 3), bad))))


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_the_per_splat_bound_covers_the_true_footprint(name):
    """spare = bound - true extent >= 0 on both axes for every drawable splat.  The formula's own margin is 0.2 % + 1.5 px, so a
    sound view_scale2 leaves about 1.5 px; the least spare is printed per camera and seed"""
    cam, proj, vp, nf = cc.CAMERAS[name](cc.W, cc.H)
    view = library_view(cam)
    vs2 = library_view_scale2(view)
    for seed in cc.SEEDS:
        aos = scenes.cloud_from_attrs(cc.hostile_attrs(cc.N, seed)).as_array()
        assert aos.shape[0] == cc.N
        _, ex, ey, ok = true_extents(aos, view, proj, vp, near=nf[0])
        bx, by = splat_bound(aos, view, proj, vp, vs2)
        assert ok.sum() >= 256, "%s: only %d drawable splats" % (name, ok.sum())
        sx, sy = (bx - ex)[ok], (by - ey)[ok]
        print("cull bound %-17s seed %d: view_scale2 %.6g (sigma_max^2 %.6g), %4d drawable, least spare x %.4g px, y %.4g px, "
              "splats below the bound %d" % (name, seed, vs2, spectral2(view), ok.sum(), sx.min(), sy.min(), ((sx < 0) | (sy < 0)).sum()))
        assert np.isfinite(sx).all() and np.isfinite(sy).all(), name
        assert sx.min() >= 0.0, "%s, seed %d: %d splat(s) reach up to %.4g px beyond the bound in x" % (name, seed, (sx < 0).sum(), -sx.min())
        assert sy.min() >= 0.0, "%s, seed %d: %d splat(s) reach up to %.4g px beyond the bound in y" % (name, seed, (sy < 0).sum(), -sy.min())
