"""CPU tests of selection by attribute (msplat_cloud_values, msplat_mark_values, msplat_histogram_values), no
device: the names exist in the header, the library and the bindings; the refusals that need no device; the numpy histogram rule
(tests/values_rule.py) conserves what it counts and is monotone; the rule's SCALE_MAX agrees with an independent eigenvalue solver;
the fixtures of the GPU tests hold what they claim and the thresholds the SCALE kinds are marked at are decidable."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from tests import values_rule as vl
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "msplat.h")
NEW = ("msplat_cloud_values", "msplat_mark_values", "msplat_histogram_values")
F = np.float32


def test_the_header_declares_the_calls_the_library_exports_them_and_the_bindings_have_them():
    header = open(HEADER).read()
    for decl in ("int msplat_cloud_values(msplat_ctx* ctx, int32_t kind, const float param[4], float* d_values, uint64_t n);",
                 "int msplat_mark_values(msplat_ctx* ctx, const float* d_values, uint64_t n, float lo, float hi, int32_t op, uint8_t* d_mask, uint8_t value);",
                 "int msplat_histogram_values(msplat_ctx* ctx, const float* d_values, const uint8_t* d_select, uint64_t n, float lo, float hi, uint32_t bins,",
                 "typedef struct msplat_value_summary { uint32_t struct_size;", "} msplat_value_summary;",
                 "MSPLAT_VALUE_COLOUR_DIST2 = 9", "MSPLAT_VALUE_SCALE_MAX = 12", "enum { MSPLAT_RANGE_INSIDE = 0, MSPLAT_RANGE_OUTSIDE = 1 };"):
        assert decl in header, decl
    for said in ("0.5f + (0.28209479177387814f * g[4 + 4c])", "a NaN value is never inside", "b = t >= (float)bins ? bins - 1 : (uint32_t)t",
                 "81 952 bytes", "Out of scope: the device group; host-memory arrays"):
        assert said in header, said
    assert len(header.splitlines()) <= 300
    L = C.CDLL(_capi.LIB_PATH)
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), "libmsplat.so does not export %s" % name
        assert name in bound, "no ctypes prototype for %s" % name
    for method in ("CloudValues", "MarkValues", "HistogramValues"):
        assert callable(getattr(SplatRenderer, method, None)), "SplatRenderer has no %s" % method
    assert tuple(sorted(_capi.VALUE_KINDS, key=_capi.VALUE_KINDS.get)) == vl.KINDS and sorted(_capi.VALUE_KINDS.values()) == list(range(13))
    for name, code in _capi.VALUE_KINDS.items():
        assert "MSPLAT_VALUE_%s = %d" % (name.upper(), code) in header, name
    # the struct as the compiler lays it out (the shim test asserts the same numbers in C++)
    assert C.sizeof(_capi.ValueSummary) == 56 and _capi.ValueSummary.selected.offset == 8 and _capi.ValueSummary.vmax.offset == 52


def test_refusals_that_need_no_device():
    L = _capi.lib()
    err = lambda: L.msplat_last_error(None).decode()
    s = _capi.ValueSummary(struct_size=C.sizeof(_capi.ValueSummary))
    assert L.msplat_cloud_values(None, _capi.VALUE_KINDS["alpha"], None, None, 0) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    assert L.msplat_mark_values(None, None, 0, 0.0, 1.0, _capi.RANGE_INSIDE, None, 1) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    assert L.msplat_histogram_values(None, None, None, 0, 0.0, 1.0, 0, None, C.byref(s)) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    assert L.msplat_histogram_values(None, None, None, 0, 0.0, 1.0, 4, None, None) == _capi.ERR_INVALID_ARG
    # the Python layer refuses what cannot be right before it asks for a device
    r = SplatRenderer()
    for call in (lambda: SplatRenderer.CloudValues(r, "hue"), lambda: SplatRenderer.CloudValues(r, 13),
                 lambda: SplatRenderer.CloudValues(r, "alpha", param=(0, 0, 0)), lambda: SplatRenderer.CloudValues(r, "distance2"),
                 lambda: SplatRenderer.CloudValues(r, "colour_dist2", param=(0, np.nan, 0)),
                 lambda: SplatRenderer.MarkValues(r, None, np.nan, 1.0, None, 1),
                 lambda: SplatRenderer.HistogramValues(r, None, bins=4097, lo=0, hi=1), lambda: SplatRenderer.HistogramValues(r, None, bins=4),
                 lambda: SplatRenderer.HistogramValues(r, None, bins=0, lo=0.0), lambda: SplatRenderer.HistogramValues(r, None, bins=4, lo=1, hi=1),
                 lambda: SplatRenderer.HistogramValues(r, None, bins=4, lo=0, hi=np.inf)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("bins", [1, 2, 1000, 4096])
def test_the_histogram_rule_conserves_the_selection_closes_both_ends_and_is_monotone(bins):
    for name, (v, lo, hi) in vl.hist_inputs().items():
        for select in (None, vl.hist_select()):
            h = vl.histogram(v, select, bins, lo, hi)
            assert int(h["counts"].sum()) + h["below"] + h["above"] + h["nan"] == h["selected"], (name, bins)
            assert h["selected"] == (v.shape[0] if select is None else int((select != 0).sum()))
            assert h["finite"] <= h["selected"] - h["nan"]
    lo, hi = F(-2.0), F(3.0)
    assert vl.bin_of(np.array([lo, hi]), bins, lo, hi).tolist() == [0, bins - 1]
    ends = vl.histogram(np.array([lo, hi, np.nextafter(lo, F(-9)), np.nextafter(hi, F(9))], F), None, bins, lo, hi)
    assert ends["counts"][0] >= 1 and ends["counts"][bins - 1] >= 1 and int(ends["counts"].sum()) == 2 and ends["below"] == ends["above"] == 1
    # monotone in v: over a sorted sweep of [lo, hi] -- the neighbours of every bin edge included -- the bin never decreases,
    # starts at 0, ends at bins - 1 and stays inside [0, bins)
    edges = (np.float64(lo) + np.arange(bins + 1) * ((np.float64(hi) - np.float64(lo)) / bins)).astype(F)
    sweep = np.concatenate([edges, np.nextafter(edges, F(-9)), np.nextafter(edges, F(9)), np.linspace(lo, hi, 5001, dtype=F)])
    sweep = np.sort(sweep[(sweep >= lo) & (sweep <= hi)])
    b = vl.bin_of(sweep, bins, lo, hi)
    assert b[0] == 0 and b[-1] == bins - 1 and (np.diff(b) >= 0).all() and b.min() >= 0 and b.max() <= bins - 1
    assert len(np.unique(b)) == bins                                   # ... and every bin is reached
    # a range whose scale is not a normal fp32 number is one the call refuses
    assert not vl.bin_scale(1, -3e38, 3e38)[1] and vl.bin_scale(4096, -3e38, 3e38)[1] and not vl.bin_scale(1, 0.0, 1e-45)[1]


def test_the_range_rule_is_closed_and_a_nan_is_never_inside():
    v = np.array([0.0, 1.0, np.nextafter(F(1.0), F(2.0)), -0.0, np.nan, np.inf, -np.inf], F)
    assert vl.inside(v, 0.0, 1.0).tolist() == [True, True, False, True, False, False, False]
    assert vl.inside(v, -np.inf, np.inf).tolist() == [True] * 4 + [False, True, True]
    assert not vl.inside(v, 1.0, 0.0).any()
    base = np.full(7, 7, np.uint8)
    assert vl.marked(base, v, 0.0, 1.0, False, 9).tolist() == [9, 9, 7, 9, 7, 7, 7]
    assert vl.marked(base, v, 0.0, 1.0, True, 9).tolist() == [7, 7, 9, 7, 9, 9, 9]           # the NaN is marked under OUTSIDE


def test_the_fixture_rows_hold_the_hostile_families_and_the_planted_values():
    rec = vl.rows()
    assert rec.shape == (4097, 61) and (rec[0, 16:25] == 0).all() and rec[2, 3] == 0 and rec[3, 3] == 1 and rec[4, 17] != rec[4, 19]
    assert np.isnan(rec[5, 3]) and np.isposinf(rec[6, 3]) and np.isneginf(rec[7, 3])
    assert np.isnan(rec[8, 4]) and np.isposinf(rec[9, 8]) and np.isneginf(rec[10, 12])
    assert np.isnan(rec[11, 0]) and np.isposinf(rec[12, 1]) and np.isneginf(rec[13, 2])
    fam = vl.family_of_row()
    assert set(fam[:63]) == {-1, 0, 1, 2}, "the first 63 rows hold every family"
    s = vl.scales(rec)
    assert (s[0] == 0).all() and np.isfinite(s).all() and (np.diff(s, axis=1) >= 0).all()
    ratio = s[:, 2] / np.maximum(s[:, 0], 1e-30)
    assert (ratio[fam == 0] > 100).any() and np.allclose(ratio[fam == 1], 1, rtol=1e-4)
    # every kind of the rule gives one float per row, and the kinds with an argument depend on it
    pos4 = np.concatenate([rec[:, 0:3], np.abs(rec[:, 16:17])], axis=1)
    for kind in vl.KINDS:
        v = vl.values(rec, pos4, kind, vl.PARAMS.get(kind))
        assert v.dtype == F and v.shape == (rec.shape[0],), kind
    assert np.isnan(vl.values(rec, pos4, "distance2", vl.PARAMS["distance2"])[11]) and np.isnan(vl.values(rec, pos4, "red")[8])
    assert np.isposinf(vl.values(rec, pos4, "colour_dist2", vl.PARAMS["colour_dist2"])[[9, 10]]).all()
    assert vl.values(rec, pos4, "green")[20] == F(0.5) + F(F(0.28209479177387814) * rec[20, 8])


def test_scale_max_squared_agrees_with_an_independent_eigenvalue_solver():
    """np.linalg.eigvalsh (LAPACK, float64) of the symmetrised covariance shares no code with the Jacobi sweeps: the squared
    SCALE_MAX is within 2^-21 of the largest |Sigma| entry of it, the bound covariance_error sets for the same eigenvalues"""
    rec = vl.rows()
    S = rec[:, 16:25].astype(np.float64).reshape(-1, 3, 3)
    S = 0.5 * (S + S.transpose(0, 2, 1))
    top = np.abs(S).max(axis=(1, 2))
    want = np.maximum(np.linalg.eigvalsh(S)[:, 2], 0.0)
    got = vl.values(rec, rec[:, 0:4], "scale_max").astype(np.float64) ** 2
    err = np.abs(got - want)
    print("worst |SCALE_MAX^2 - lambda_max| / max |Sigma|: %.3g (bound %.3g)" % (float((err[top > 0] / top[top > 0]).max()), 2.0 ** -21))
    assert (err <= 2.0 ** -21 * top).all(), int((err > 2.0 ** -21 * top).sum())
    lo = vl.values(rec, rec[:, 0:4], "scale_min").astype(np.float64) ** 2
    assert (np.abs(lo - np.maximum(np.linalg.eigvalsh(S)[:, 0], 0.0)) <= 2.0 ** -21 * top).all()


@pytest.mark.parametrize("kind", vl.SCALE_KINDS)
def test_the_scale_thresholds_of_the_gpu_tests_are_decidable(kind):
    """the GPU marks and the rule's are compared on every row: no rule value may lie within 1e-5 (relative) of a threshold, ten
    times the rtol 1e-6 the device's values are held to, and every threshold splits its family"""
    rec = vl.rows()
    v = vl.scales(rec)[:, vl.SCALE_KINDS.index(kind)]
    fam = vl.family_of_row()
    for f, (name, t) in enumerate(vl.scale_thresholds(kind).items()):
        assert name == vl.FAMILIES[f] and np.isfinite(t) and t > 0
        near = vl.undecidable(v, t)
        assert not near.any(), "%s, %s: %d value(s) within 1e-5 of the threshold %.9g" % (kind, name, int(near.sum()), t)
        share = float((v[fam == f] <= t).mean())
        assert 0.25 <= share <= 0.75, (kind, name, share)
        for n in vl.SIZES[1:]:
            assert 0 < int((v[:n] <= t).sum()) < n, (kind, name, n)


def test_the_shim_with_the_value_methods_compiles_with_gxx(tmp_path):
    src = tmp_path / "values_shim.cpp"
    src.write_text("""
#include <cstddef>
#include "splatapult_amd/host/msplat_host.hpp"
static_assert(sizeof(msplat_value_summary) == 56 && offsetof(msplat_value_summary, selected) == 8 && offsetof(msplat_value_summary, vmax) == 52,
              "the layout the ctypes binding assumes");
static_assert(MSPLAT_VALUE_X == 0 && MSPLAT_VALUE_ALPHA == 5 && MSPLAT_VALUE_SCALE_MAX == 12 && MSPLAT_RANGE_OUTSIDE == 1, "the kinds");
int main()
{
    SplatRenderer r;
    msplat_value_summary out;
    const float p[4] = {0, 0, 0, 0};
    uint32_t counts[4];
    // no context yet: every call on the renderer is refused, none crashes
    bool ok = !r.CloudValues(MSPLAT_VALUE_DISTANCE2, p, nullptr, 0) && !r.MarkValues(nullptr, 0, 0.0f, 1.0f, MSPLAT_RANGE_INSIDE, nullptr, 1) &&
              !r.HistogramValues(nullptr, nullptr, 0, 0.0f, 1.0f, 4, counts, &out) && out.struct_size == sizeof(msplat_value_summary);
    ok = ok && msplat_cloud_values(nullptr, MSPLAT_VALUE_ALPHA, nullptr, nullptr, 0) == MSPLAT_ERR_INVALID_ARG;
    ok = ok && msplat_mark_values(nullptr, nullptr, 0, 0.0f, 1.0f, MSPLAT_RANGE_OUTSIDE, nullptr, 0) == MSPLAT_ERR_INVALID_ARG;
    ok = ok && msplat_histogram_values(nullptr, nullptr, nullptr, 0, 0.0f, 1.0f, 0, nullptr, &out) == MSPLAT_ERR_INVALID_ARG;
    return ok ? 0 : 1;
}
""")
    exe, libdir = str(tmp_path / "values_shim"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, cwd=ROOT)
    assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 0
