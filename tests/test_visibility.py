"""CPU tests of per-splat visibility (msplat_set_visibility[_device], msplat_set_crop, msplat_get_visibility):
the entry points exist, what they refuse without a device, and that the fixtures of tests/test_gpu_visibility.py are what they
claim -- the centres on the crop surfaces are inside and their float neighbours outside under the header's fp32 rule, no centre of
the cropped cloud is so close to a rotated surface that a last-bit difference could flip it, and the tie-free cloud has no ties."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle
from splatapult_amd import SplatRenderer, _capi
from tests import visibility_rule as vr
from tests.conftest import ROOT

NEW = ("msplat_set_visibility", "msplat_set_visibility_device", "msplat_set_crop", "msplat_get_visibility")
IDENT = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))


def test_the_library_exports_the_entry_points_and_the_wrappers_exist():
    L = C.CDLL(_capi.LIB_PATH)
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), "libmsplat.so does not export " + name
        assert name in bound, "no ctypes prototype for " + name
    for method in ("SetVisibility", "SetCrop", "visibility"):
        assert callable(getattr(SplatRenderer, method, None)), "SplatRenderer has no " + method
    assert (_capi.CROP_NONE, _capi.CROP_BOX, _capi.CROP_SPHERE, _capi.CROP_INVERT) == (0, 1, 2, 0x100)
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    assert "MSPLAT_CROP_NONE = 0, MSPLAT_CROP_BOX = 1, MSPLAT_CROP_SPHERE = 2, MSPLAT_CROP_INVERT = 0x100" in header


def test_refusals_that_need_no_device():
    L = _capi.lib()
    err = lambda: L.msplat_last_error(None).decode()
    mask = np.ones(4, np.uint8)
    assert L.msplat_set_visibility(None, mask.ctypes.data, 4) == _capi.ERR_INVALID_ARG and "NULL" in err()
    assert L.msplat_set_visibility_device(None, None, 0) == _capi.ERR_INVALID_ARG and "NULL" in err()
    assert L.msplat_get_visibility(None, None, None, None) == _capi.ERR_INVALID_ARG and "NULL" in err()
    assert L.msplat_set_crop(None, IDENT, _capi.CROP_BOX) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    assert L.msplat_set_crop(None, None, _capi.CROP_NONE) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    # the shape and the matrix are judged before the context is looked at
    for shape in (3, 7, -1, _capi.CROP_INVERT, _capi.CROP_BOX | 0x200, _capi.CROP_SPHERE | 0x1000):
        assert L.msplat_set_crop(None, IDENT, shape) == _capi.ERR_INVALID_ARG and "shape" in err(), shape
    for k, bad in ((0, np.nan), (5, np.inf), (14, -np.inf), (8, np.nan)):
        m = np.eye(4, dtype=np.float32).reshape(16)
        m[k] = bad
        rc = L.msplat_set_crop(None, m.ctypes.data_as(C.POINTER(C.c_float)), _capi.CROP_SPHERE | _capi.CROP_INVERT)
        assert rc == _capi.ERR_INVALID_ARG and "worldToCrop[%d] is not finite" % k in err(), (k, err())
    # the fourth row is not read: it may hold anything
    m = np.eye(4, dtype=np.float32).reshape(16)
    m[3] = m[7] = m[11] = m[15] = np.nan
    assert L.msplat_set_crop(None, m.ctypes.data_as(C.POINTER(C.c_float)), _capi.CROP_BOX) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()


def test_set_visibility_checks_length_and_dtype_before_the_library():
    class Lib:                      # any call on it is a failure of this test
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    r = SplatRenderer()
    r._lib, r._n = Lib(), 10
    for bad in (np.ones(9, bool), np.ones(11, np.uint8), np.ones((10, 1), bool), np.ones((2, 5), np.uint8)):
        with pytest.raises(ValueError, match="shape"):
            r.SetVisibility(bad)
    for bad in (np.ones(10, np.float32), np.ones(10, np.int8), np.ones(10, np.int32), [1] * 10, b"\x01" * 10):
        with pytest.raises(ValueError, match="bool / uint8"):
            r.SetVisibility(bad)

    class Tensor:                   # a device tensor, duck-typed as renderer.SetVisibility reads it
        def __init__(self, n, dtype="torch.bool", device="cuda", contiguous=True):
            self.shape, self.dtype, self._c = (n,), dtype, contiguous
            self.device = type("D", (), {"type": device, "__str__": lambda s: device})()

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            raise AssertionError("the pointer was taken")

    for bad, why in ((Tensor(9), "shape"), (Tensor(10, "torch.float32"), "bool or uint8"), (Tensor(10, contiguous=False), "contiguous"),
                     (Tensor(10, device="cpu"), "device memory")):
        with pytest.raises(ValueError, match=why):
            r.SetVisibility(bad)
    with pytest.raises(ValueError, match="shape must be one of"):
        r.SetCrop(np.eye(4), shape="cylinder")
    with pytest.raises(AssertionError, match="16 floats"):
        r.SetCrop(np.eye(3))
    r._lib, r._ctxs = _capi.lib(), []        # (what __del__ uses)


@pytest.mark.parametrize("name", ["identity", "scaled"])
def test_centres_on_the_surface_are_inside_and_their_neighbours_outside(name):
    M = vr.matrices()[name]
    on, out = vr.on_surface(name)
    assert (np.abs(out) >= np.abs(on)).all() and ((out != on).sum(axis=1) == 1).all()
    for shape in ("box", "sphere"):
        q = np.stack(vr.crop_q(on, M), axis=1)
        assert (np.abs(q).max(axis=1) == 1.0).all() and (np.abs(q).sum(axis=1) == 1.0).all()      # q is exactly a face centre
        assert vr.crop(on, M, shape).all() and not vr.crop(on, M, shape, invert=True).any()
        assert not vr.crop(out, M, shape).any() and vr.crop(out, M, shape, invert=True).all()
        # exact: float64 says the same
        assert vr.crop(on, M, shape, dtype=np.float64).all() and not vr.crop(out, M, shape, dtype=np.float64).any()


def test_a_nan_centre_is_outside_with_and_without_invert():
    xyz = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.nan] * 3, [0.1, 0.2, 0.3]], np.float32)
    for name, M in vr.matrices().items():
        for shape in ("box", "sphere"):
            inside = vr.crop(xyz, M, shape)
            assert not inside[:4].any(), (name, shape)
            # "not inside" is all INVERT asks: the rule lets a NaN centre through, and the presort cull rejects it anyway
            assert vr.crop(xyz, M, shape, invert=True)[:4].all(), (name, shape)
    assert vr.crop(xyz, vr.matrices()["identity"], "box")[4]


def test_the_cropped_cloud_holds_the_surface_fixtures_and_no_centre_near_a_rounded_surface():
    aos = vr.crop_cloud()
    xyz = aos[:, 0:3]
    assert aos.shape == (vr.N_CROP, 61) and np.isfinite(xyz).all()
    k = 0
    for name in ("identity", "scaled"):
        on, out = vr.on_surface(name)
        np.testing.assert_array_equal(xyz[k:k + 6], on)
        np.testing.assert_array_equal(xyz[k + 6:k + 12], out)
        k += 12
    # fp32 evaluation of q: |error| <= 4 ulp of sum |M_rc x_c| < 2^-21 |q|_1 here; 1e-5 is twenty times that for |q| ~ 1
    for name, M in vr.matrices().items():
        for shape in ("box", "sphere"):
            d = vr.surface_distance(xyz, M, shape)
            exact = name != "rotated"
            near = d < 1e-5
            if exact:
                assert near.sum() >= 6                       # the fixtures: on the surface or one float off it
            else:
                assert not near.any(), "%s %s: %d centre(s) within 1e-5 of the surface" % (name, shape, near.sum())
            got, want = vr.crop(xyz, M, shape), vr.crop(xyz, M, shape, dtype=np.float64)
            assert (got == want)[~near].all()
            assert (got == want).all(), (name, shape)        # (q exact, or nothing near: the two agree everywhere)
            assert 0.02 < got.mean() < 0.98, (name, shape, got.mean())       # the crop keeps some and hides some


def test_the_tie_free_cloud_has_pairwise_distinct_keys():
    L = _capi.lib()
    cam, proj, vp, nf = vr.view()
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32).reshape(16))
    p16 = C.POINTER(C.c_float)
    view, mvp = np.zeros(16, np.float32), np.zeros(16, np.float32)
    L.msplat_mat4_inverse(f(cam).ctypes.data_as(p16), view.ctypes.data_as(p16))
    L.msplat_mat4_mul(f(proj).ctypes.data_as(p16), view.ctypes.data_as(p16), mvp.ctypes.data_as(p16))
    vis, key = np_oracle.cull_keys(vr.cloud_aos(*vr.TIE_FREE)[:, 0:3], mvp, nf[1])
    assert vis.sum() > 3000, vis.sum()
    assert np.unique(key[vis]).size == vis.sum(), "%d visible splats share a key" % (vis.sum() - np.unique(key[vis]).size)
    # (the other sizes' clouds and the crop cloud do have ties: they are compared where ties keep the upload order, or as sets)
    vis, key = np_oracle.cull_keys(vr.crop_cloud()[:, 0:3], mvp, nf[1])
    assert vis[:24].all(), "a surface fixture is outside the view"


def test_the_shim_with_the_visibility_methods_compiles_with_gxx(tmp_path):
    src = tmp_path / "vis_shim.cpp"
    src.write_text("""
#include <vector>
#include "splatapult_amd/host/msplat_host.hpp"
int main()
{
    SplatRenderer r;
    std::vector<uint8_t> mask(4, 1);
    const float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    // no context yet: nothing to set, every call succeeds on zero contexts
    bool ok = r.SetVisibility(mask.data(), mask.size()) && r.SetVisibilityDevice(nullptr, 0) && r.SetCrop(m, MSPLAT_CROP_SPHERE | MSPLAT_CROP_INVERT);
    ok = ok && r.SetCrop(nullptr, MSPLAT_CROP_NONE) && msplat_set_crop(nullptr, m, MSPLAT_CROP_BOX) == MSPLAT_ERR_INVALID_ARG;
    ok = ok && msplat_get_visibility(nullptr, nullptr, nullptr, nullptr) == MSPLAT_ERR_INVALID_ARG;
    return ok ? 0 : 1;
}
""")
    exe, libdir = str(tmp_path / "vis_shim"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, cwd=ROOT)
    assert subprocess.run([exe]).returncode == 0
