"""CPU tests of the render-time overlay (msplat_set_overlay[_device], msplat_set_overlay_palette, msplat_get_overlay; INTEGRATION.md
26): the entry points exist, what they refuse without a device, the numpy restatement of the rule against a float64 evaluation,
that the fixtures of tests/test_gpu_overlay.py are what they claim, and SetOverlay's checks before the library is called."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle
from splatapult_amd import SplatRenderer, _capi
from tests import overlay_rule as ov
from tests.conftest import ROOT

NEW = ("msplat_set_overlay", "msplat_set_overlay_device", "msplat_set_overlay_palette", "msplat_get_overlay")


def test_the_library_exports_the_entry_points_and_the_wrappers_exist():
    L = C.CDLL(_capi.LIB_PATH)
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), "libmsplat.so does not export " + name
        assert name in bound, "no ctypes prototype for " + name
    for method in ("SetOverlay", "overlay"):
        assert callable(getattr(SplatRenderer, method, None)), "SplatRenderer has no " + method
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    for name in NEW:
        assert "int %s(msplat_ctx* ctx, " % name in header, name
    shim = open(os.path.join(ROOT, "splatapult_amd", "host", "msplat_host.hpp")).read()
    for method in ("SetOverlay(", "SetOverlayDevice(", "SetOverlayPalette("):
        assert "bool " + method in shim, method


def test_refusals_that_need_no_device():
    L = _capi.lib()
    err = lambda: L.msplat_last_error(None).decode()
    cls = np.ones(4, np.uint8)
    pal = ov.palette(3)
    assert L.msplat_set_overlay(None, cls.ctypes.data, 4) == _capi.ERR_INVALID_ARG and "NULL" in err()
    assert L.msplat_set_overlay_device(None, None, 0) == _capi.ERR_INVALID_ARG and "NULL" in err()
    assert L.msplat_set_overlay_palette(None, pal.ctypes.data, 3) == _capi.ERR_INVALID_ARG and "NULL" in err()
    assert L.msplat_get_overlay(None, None, None, None) == _capi.ERR_INVALID_ARG and "NULL" in err()


def test_the_rule_is_two_roundings_away_from_float64():
    """c' = fl(fl(t c) + fl(a h)), t = 1 - a.  For the palettes' a (0, 2^-8, 0.5, 1) t is exact and at most one of the products is
    rounded (a = 2^-8: a h is a scaling by a power of two; a = 0.5: both are; a = 1: t c = 0 and a h = h), so two roundings remain:
    a product, within 0.5 ulp of the larger term L, and the sum, within 0.5 ulp of a value <= 2 L, that is 1 ulp(L): 1.5 ulp(L)"""
    rng = np.random.default_rng(5)
    n = 20000
    c = np.concatenate([rng.uniform(-0.5, 1.5, (n - 6, 3)), [[0.0] * 3, [-0.0] * 3, [1e-30] * 3, [1.0] * 3, [0.5] * 3, [3e4] * 3]]).astype(np.float32)
    for count in ov.COUNTS:
        pal = ov.palette(count)
        cls = rng.integers(0, 256, n).astype(np.uint8)
        cls[: n // 2] = rng.integers(0, count, n // 2)
        got = ov.tint(c, cls, pal)
        want, tc, ah = ov.tint_f64(c, cls, pal)
        h, a = ov.entries(cls, pal)
        on = a != 0
        assert on.any() and (count == 1 or (~on).any())
        np.testing.assert_array_equal(got[~on].view(np.uint32), c[~on].view(np.uint32))          # untouched: the bits stay
        assert ((np.float32(1.0) - a).astype(np.float64) == 1.0 - a.astype(np.float64)).all()      # t is exact
        larger = np.maximum(tc, ah)
        ulp = np.spacing(np.maximum(larger, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)
        print("count %d: worst error %.3f ulp of the larger term" % (count, (err[on] / ulp[on]).max()))
        assert (err[on] <= 1.5 * ulp[on]).all(), (err[on] / ulp[on]).max()
        full = a == 1
        if full.any():                                          # a == 1: exactly h for a finite c
            np.testing.assert_array_equal(got[full], h[full])


def test_untinted_lanes_keep_their_bits_also_a_nan():
    c = np.array([[np.nan, 1.0, -0.0], [np.inf, 2.0, 3.0]], np.float32)
    c.view(np.uint32)[0, 0] = 0x7FC12345                        # a NaN with a payload
    pal = ov.palette(3)
    got = ov.tint(c, np.array([0, 200], np.uint8), pal)          # a == 0, and a class beyond the palette
    np.testing.assert_array_equal(got.view(np.uint32), c.view(np.uint32))
    pal = ov.palette(256)
    assert pal[3, 3] == 1.0
    got = ov.tint(c, np.array([3, 3], np.uint8), pal)            # a == 1 on non-finite lanes: 0 * inf and 0 * NaN are NaN
    assert np.isnan(got[0, 0]) and np.isnan(got[1, 0]) and got[0, 1] == pal[3, 1] and got[1, 2] == pal[3, 2]


def test_the_palettes_and_classes_are_what_they_claim():
    for count in ov.COUNTS:
        pal = ov.palette(count)
        assert pal.shape == (count, 4) and pal.dtype == np.float32 and np.isfinite(pal).all()
        assert set(pal[:, 3].tolist()) <= set(ov.A_VALUES)
        assert pal[ov.tinted_class(count), 3] != 0
        if count == 256:
            assert set(pal[:, 3].tolist()) == set(ov.A_VALUES)
        for n in ov.SIZES:
            aos = ov.cloud(n)
            cls = ov.classes(aos, count)
            assert cls.shape == (n,) and cls.dtype == np.uint8
            if n >= 63:
                hist = np.bincount(cls, minlength=256)
                for k in (0, 1, count - 1, min(count, 255), 255):
                    assert hist[k] > 0, "n %d, count %d: no splat of class %d" % (n, count, k)
                _, a = ov.entries(cls, pal)
                assert (a != 0).any() and (count == 1 and n < 2 * ov.RUN + 64 or (a == 0).any())
    assert (ov.GREY[1] == [0.5, 0.5, 0.5, 1.0]).all() and ov.GREY[0, 3] == 0


def test_the_largest_cloud_has_a_block_of_64_ranks_without_a_tint_and_one_all_tinted():
    """the draw order of the view the GPU tests use, from the oracle's keys: ranks are the visible splats far to near"""
    L = _capi.lib()
    cam, proj, vp, nf = ov.view()
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32).reshape(16))
    p16 = C.POINTER(C.c_float)
    viewm, mvp = np.zeros(16, np.float32), np.zeros(16, np.float32)
    L.msplat_mat4_inverse(f(cam).ctypes.data_as(p16), viewm.ctypes.data_as(p16))
    L.msplat_mat4_mul(f(proj).ctypes.data_as(p16), viewm.ctypes.data_as(p16), mvp.ctypes.data_as(p16))
    aos = ov.cloud(4097)
    vis, key = np_oracle.cull_keys(aos[:, 0:3], mvp, nf[1])
    ranks = np.flatnonzero(vis)[np.argsort(key[vis], kind="stable")]
    assert ranks.size > 3000 and ranks.size % 64 != 0, ranks.size          # (and V is no multiple of 64: the stereo chain has a gap)
    for count in ov.COUNTS:
        _, a = ov.entries(ov.classes(aos, count)[ranks], ov.palette(count))
        blocks = (a[: ranks.size // 64 * 64] != 0).reshape(-1, 64)
        assert blocks.all(axis=1).any(), "count %d: no block of 64 ranks is all tinted" % count
        assert (~blocks.any(axis=1)).any(), "count %d: no block of 64 ranks is free of tints" % count


def test_the_sh_free_clouds():
    for full_sh in (True, False):
        aos = ov.cloud(257, full_sh=full_sh)
        sel = ov.selection(257)
        z = ov.zero_sh(aos, sel)
        cols = ov.sh_floats(aos.shape[1])
        rest = np.setdiff1d(np.arange(aos.shape[1]), cols)
        assert cols.size == (48 if full_sh else 12)
        assert (z[np.ix_(np.flatnonzero(sel), cols)] == 0).all() and (z[~sel] == aos[~sel]).all() and (z[:, rest] == aos[:, rest]).all()
        assert (aos[np.ix_(np.flatnonzero(sel), cols)] != 0).any()
        base = ov.dc_only(aos)
        assert (base[:, ov.dc_columns()] == aos[:, ov.dc_columns()]).all() and (base[:, rest] == aos[:, rest]).all()
        assert (base[:, np.setdiff1d(cols, ov.dc_columns())] == 0).all()
        # the recoloured cloud's colours are the rule's, to the rounding of the DC term: |d| <= SH_C0 ulp(dc') / 2 + the sum's ulp
        cls, pal = ov.classes(aos, 256), ov.palette(256)
        base2, rec = ov.recoloured(aos, cls, pal)
        assert (base2 == base).all()
        c = np.float32(0.5) + np.float32(ov.SH_C0) * base[:, ov.dc_columns()]
        back = np.float32(0.5) + np.float32(ov.SH_C0) * rec[:, ov.dc_columns()]
        assert np.abs(back.astype(np.float64) - ov.tint(c, cls, pal)).max() < 1e-6


def test_set_overlay_checks_its_arguments_before_the_library():
    class Lib:                      # any call on it is a failure of this test
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    r = SplatRenderer()
    r._lib, r._n = Lib(), 10
    for bad in (np.ones(9, np.uint8), np.ones(11, bool), np.ones((10, 1), np.uint8), np.ones((2, 5), np.uint8)):
        with pytest.raises(ValueError, match="shape"):
            r.SetOverlay(bad)
    for bad in (np.ones(10, np.float32), np.ones(10, np.int8), np.ones(10, np.int32), [1] * 10, b"\x01" * 10):
        with pytest.raises(ValueError, match="uint8 / bool"):
            r.SetOverlay(bad)

    class Tensor:                   # a device tensor, duck-typed as renderer.SetOverlay reads it
        def __init__(self, n, dtype="torch.uint8", device="cuda", contiguous=True):
            self.shape, self.dtype, self._c = (n,), dtype, contiguous
            self.device = type("D", (), {"type": device, "__str__": lambda s: device})()

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            raise AssertionError("the pointer was taken")

    for bad, why in ((Tensor(9), "shape"), (Tensor(10, "torch.float32"), "uint8 or bool"), (Tensor(10, contiguous=False), "contiguous"),
                     (Tensor(10, device="cpu"), "device memory")):
        with pytest.raises(ValueError, match=why):
            r.SetOverlay(bad)
    good = np.zeros(10, np.uint8)
    for bad in (np.zeros((257, 4)), np.zeros((3, 3)), np.zeros(4), np.zeros((2, 2, 4))):
        with pytest.raises(ValueError, match=r"\(count, 4\)"):
            r.SetOverlay(good, bad)
    for k, v in ((0, np.nan), (5, np.inf), (3, -0.5), (7, 1.5), (3, np.nan)):
        pal = ov.palette(3).copy()
        pal.reshape(-1)[k] = v
        with pytest.raises(ValueError, match="finite with a in"):
            r.SetOverlay(good, pal)
        with pytest.raises(ValueError, match="finite with a in"):
            r.SetOverlay(palette=pal)
    r.SetOverlay()                  # nothing given, nothing done
    r._lib, r._ctxs = _capi.lib(), []        # (what __del__ uses)


def test_the_shim_with_the_overlay_methods_compiles_with_gxx(tmp_path):
    src = tmp_path / "overlay_shim.cpp"
    src.write_text("""
#include <vector>
#include "splatapult_amd/host/msplat_host.hpp"
int main()
{
    SplatRenderer r;
    std::vector<uint8_t> classes(4, 1);
    const float palette[8] = {0, 0, 0, 0, 1.0f, 0.5f, 0.25f, 0.5f};
    // no context yet: the classes have nothing to be set on, the palette is kept for the contexts Init creates
    bool ok = r.SetOverlay(classes.data(), classes.size()) && r.SetOverlayDevice(nullptr, 0) && r.SetOverlayPalette(palette, 2);
    ok = ok && r.SetOverlayPalette(nullptr, 0) && msplat_set_overlay(nullptr, classes.data(), 4) == MSPLAT_ERR_INVALID_ARG;
    ok = ok && msplat_set_overlay_palette(nullptr, palette, 2) == MSPLAT_ERR_INVALID_ARG;
    ok = ok && msplat_get_overlay(nullptr, nullptr, nullptr, nullptr) == MSPLAT_ERR_INVALID_ARG;
    return ok ? 0 : 1;
}
""")
    exe, libdir = str(tmp_path / "overlay_shim"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, cwd=ROOT)
    assert subprocess.run([exe]).returncode == 0
