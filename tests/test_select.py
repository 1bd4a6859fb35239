"""CPU tests of the selection calls (msplat_mark_volume, msplat_mark_view, msplat_measure_cloud, msplat_measure_box; INTEGRATION.md
28), no device: the names exist in the header, the library and the bindings; the refusals that need no device; msplat_measure_box on
hostile measures, proved with the crop rule in fp32; and that the fixtures of the GPU tests (tests/select_rule.py) are what they
claim -- the exact cameras' MVP is exact, the designed centres sit where they were designed to sit, the random-camera comparison
leaves out less than it may, and the measure's selections hold the hostile rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi, measure_box
from tests import select_rule as sr
from tests import visibility_rule as vr
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "msplat.h")
NEW = ("msplat_mark_volume", "msplat_mark_view", "msplat_measure_cloud", "msplat_measure_box")
_P = C.POINTER(C.c_float)
F = np.float32


def test_the_header_declares_the_calls_the_library_exports_them_and_the_bindings_have_them():
    header = open(HEADER).read()
    for decl in ("int msplat_mark_volume(msplat_ctx* ctx, const float worldToVolume[16], int32_t shape, uint8_t* d_mask, uint64_t n, uint8_t value);",
                 "const int32_t window[4], const uint8_t* d_region, uint64_t region_pitch_bytes, uint8_t* d_mask, uint64_t n, uint8_t value);",
                 "int msplat_measure_cloud(msplat_ctx* ctx, const uint8_t* d_select, uint64_t n, msplat_cloud_measure* out);",
                 "int msplat_measure_box(const msplat_cloud_measure* m, float pad, float worldToVolume[16]);",
                 "} msplat_cloud_measure;"):
        assert decl in header, decl
    for said in ("a NaN centre is outside and therefore marked under INVERT", "cx = 0.5f * (W + (xx * W))", "finite * 2^-53 * S",
                 "229 488 bytes", "A * 2^-21"):
        assert said in header, said
    assert len(header.splitlines()) <= 300
    L = C.CDLL(_capi.LIB_PATH)
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), "libmsplat.so does not export %s" % name
        assert name in bound, "no ctypes prototype for %s" % name
    for method in ("MarkVolume", "MarkView", "MeasureCloud"):
        assert callable(getattr(SplatRenderer, method, None)), "SplatRenderer has no %s" % method
    assert callable(measure_box)
    # the struct as the compiler lays it out (the shim test asserts the same numbers in C++): padding behind struct_size and reach2_max
    assert C.sizeof(_capi.CloudMeasure) == 128 and _capi.CloudMeasure.sum2.offset == 80 and _capi.CloudMeasure.selected.offset == 8


def test_refusals_that_need_no_device():
    L = _capi.lib()
    err = lambda: L.msplat_last_error(None).decode()
    ident = np.eye(4, dtype=F).reshape(16)
    m = _capi.CloudMeasure(struct_size=C.sizeof(_capi.CloudMeasure))
    assert L.msplat_mark_volume(None, ident.ctypes.data_as(_P), _capi.CROP_BOX, None, 0, 1) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    vp, nf = (C.c_float * 4)(0, 0, 8, 8), (C.c_float * 2)(0.1, 10.0)
    assert L.msplat_mark_view(None, ident.ctypes.data_as(_P), ident.ctypes.data_as(_P), vp, nf, None, None, 0, None, 0, 1) == _capi.ERR_INVALID_ARG
    assert "ctx is NULL" in err()
    assert L.msplat_measure_cloud(None, None, 0, C.byref(m)) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    out = np.zeros(16, F)
    assert L.msplat_measure_box(None, 0.0, out.ctypes.data_as(_P)) == _capi.ERR_INVALID_ARG
    assert L.msplat_measure_box(C.byref(m), 0.0, None) == _capi.ERR_INVALID_ARG
    assert L.msplat_measure_box(C.byref(m), 0.0, out.ctypes.data_as(_P)) == _capi.ERR_INVALID_ARG and "no finite centre" in err()
    m.finite, m.selected = 1, 1
    for k in range(3):
        m.lo[k] = m.hi[k] = 1.0
    for pad in (-1.0, float("nan"), float("inf")):
        assert L.msplat_measure_box(C.byref(m), pad, out.ctypes.data_as(_P)) == _capi.ERR_INVALID_ARG and "pad" in err(), pad
    assert not out.any(), "a refused call wrote the matrix"
    assert L.msplat_measure_box(C.byref(m), 0.0, out.ctypes.data_as(_P)) == _capi.OK
    m.lo[1], m.hi[1] = 2.0, 1.0
    assert L.msplat_measure_box(C.byref(m), 0.0, out.ctypes.data_as(_P)) == _capi.ERR_INVALID_ARG and "not a box" in err()
    m.lo[1] = float("-inf")
    assert L.msplat_measure_box(C.byref(m), 0.0, out.ctypes.data_as(_P)) == _capi.ERR_INVALID_ARG


def test_a_context_without_a_device_refuses_null_out_before_anything_else():
    # (NULL ctx comes first; NULL out needs a context, so it is checked on the GPU: tests/test_gpu_select.py)
    L = _capi.lib()
    assert L.msplat_measure_cloud(None, None, 0, None) == _capi.ERR_INVALID_ARG


@pytest.mark.parametrize("pad", [0.0, 0.37, 1e3])
@pytest.mark.parametrize("name", list(sr.box_cases()))
def test_measure_box_holds_every_centre_of_hostile_measures(name, pad):
    lo, hi = sr.box_cases()[name]
    M = measure_box(dict(selected=1, finite=1, lo=lo, hi=hi, reach2_max=0.0), pad)
    assert np.isfinite(M).all() and M[15] == 1 and (M[[1, 2, 3, 4, 6, 7, 8, 9, 11]] == 0).all(), M
    pts = sr.box_cloud(lo, hi)
    assert (pts >= lo).all() and (pts <= hi).all()
    inside = vr.crop(pts, M, "box")
    q = np.abs(np.stack(vr.crop_q(pts, M))).max()
    print("%s, pad %g: max |q| in fp32 %.9g over %d centres" % (name, pad, q, pts.shape[0]))
    assert inside.all(), "%s: %d of %d centres of [lo, hi] are outside the box; max |q| %.9g" % (name, (~inside).sum(), pts.shape[0], q)
    # ... and the box is no wider than the formula says: a centre beyond the half-extent, widened by 1e-5 relative, is outside
    c = 0.5 * lo.astype(np.float64) + 0.5 * hi.astype(np.float64)
    A = np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64)
    h = np.maximum(0.5 * hi.astype(np.float64) - 0.5 * lo.astype(np.float64), 2.0 ** -100) * (1 + 2.0 ** -20) + A * 2.0 ** -21 + pad
    for axis in range(3):
        for sign in (-1.0, 1.0):
            far = c.copy()
            far[axis] += sign * h[axis] * (1 + 1e-5) + sign * A[axis] * 2.0 ** -20
            p = far.astype(F)[None, :]
            if np.isfinite(p).all() and abs(float(p[0, axis]) - c[axis]) > h[axis] * (1 + 1e-6) + A[axis] * 2.0 ** -21:
                assert not vr.crop(p, M, "box", dtype=np.float64)[0], (name, axis, sign)


def test_the_relative_widening_alone_does_not_hold_far_from_the_origin():
    """why the header's half-extent has the additive term A * 2^-21: with max((hi - lo) / 2, floor) * (1 + 2^-20) + pad alone, a box
    eight units wide at 1e5 loses its own corners to fp32 cancellation in q = x / h - c / h (one random box in five does)"""
    lo, hi = sr.box_cases()["far_and_eight_wide"]
    c = 0.5 * lo.astype(np.float64) + 0.5 * hi.astype(np.float64)
    h = np.maximum(0.5 * hi.astype(np.float64) - 0.5 * lo.astype(np.float64), 2.0 ** -100) * (1 + 2.0 ** -20)
    M = np.zeros(16, F)
    M[[0, 5, 10]], M[12:15], M[15] = (1.0 / h).astype(F), (-c / h).astype(F), 1.0
    assert not vr.crop(sr.box_cloud(lo, hi), M, "box").all()


def test_the_exact_cameras_mvp_is_exact_and_the_designed_centres_sit_where_designed():
    for name, (cam, proj, _, _, _) in sr.exact_cameras().items():
        mvp = sr.mvp_of(cam, proj)
        want = sr.exact_mvp64(name)
        assert (mvp.astype(np.float64) == want).all(), (name, mvp, want)
        xyz, cx, cy, depth = sr.exact_centres(name)
        gx, gy, gd = sr.centre_px(xyz, mvp, sr.EW, sr.EH)
        ok = np.isfinite(xyz[:, 0]) & (depth != 0)
        assert (gd[ok] == depth[ok]).all() and (gx[ok] == cx[ok]).all() and (gy[ok] == cy[ok]).all(), name
        assert (gd[depth == 0] == 0).all() and np.isnan(gx[~np.isfinite(xyz[:, 0])]).all()
        front = ok & (depth > 0)
        # pixel centres, pixel borders, outside on every side
        assert (cx[front] % 1 == 0.5).any() and (cx[front] % 1 == 0).any() and (cx[front] < 0).any() and (cx[front] >= sr.EW).any()
        for wname, win in sr.EXACT_WINDOWS.items():
            x0, y0, w, h = win if win is not None else (0, 0, sr.EW, sr.EH)
            for ex in (x0, x0 + w):                 # centres exactly on the four edges and corners of the window
                for ey in (y0, y0 + h):
                    assert (front & (cx == ex) & (cy == ey)).any(), (name, wname, ex, ey)
            inside = sr.view_inside(xyz, mvp, sr.EW, sr.EH, win)
            want = front & (cx >= x0) & (cx < x0 + w) & (cy >= y0) & (cy < y0 + h)
            assert (inside == want).all() and 0 < inside.sum() < xyz.shape[0], (name, wname)
            # the rule in float64 agrees on every designed centre: nothing here is decided by rounding
            assert (sr.view_inside(xyz, mvp, sr.EW, sr.EH, win, dtype=np.float64) == inside).all(), (name, wname)
            region = sr.region_for(win, 3)
            with_region = sr.view_inside(xyz, mvp, sr.EW, sr.EH, win, region)
            assert not (with_region & ~inside).any() and (w * h == 1 or 0 < with_region.sum() < inside.sum()), (name, wname)
        assert xyz.shape[0] <= 4096


def test_the_random_camera_comparison_leaves_out_less_than_one_percent():
    xyz = sr.general_cloud()[:, 0:3]
    region = sr.general_region()
    for name, (cam, proj, vp, nf) in sr.general_views().items():
        W, H = vp[2], vp[3]
        assert (W, H) == (sr.GW, sr.GH)
        mvp = sr.mvp_of(cam, proj)
        ok = sr.decidable(xyz, mvp, W, H)
        share = 1.0 - ok.mean()
        whole = sr.view_inside(xyz, mvp, W, H)
        lasso = sr.view_inside(xyz, mvp, W, H, sr.GENERAL_WINDOW, region)
        print("%s: %.3f %% of the splats left out; %d in the viewport, %d in the lasso" % (name, 100 * share, whole.sum(), lasso.sum()))
        assert share <= sr.MAX_LEFT_OUT, (name, share)
        assert 0.2 < whole.mean() < 0.98 and 0.02 < lasso.mean() < whole.mean(), (name, whole.mean(), lasso.mean())
        # numpy's fp32 rule agrees with the float64 rule wherever the comparison is made
        for win, reg in ((None, None), (sr.GENERAL_WINDOW, None), (sr.GENERAL_WINDOW, region)):
            a = sr.view_inside(xyz, mvp, W, H, win, reg)
            b = sr.view_inside(xyz, mvp, W, H, win, reg, dtype=np.float64)
            assert (a == b)[ok].all(), (name, win, int((a != b)[ok].sum()))


def test_the_measure_fixtures_hold_the_hostile_rows():
    rows = sr.measure_rows()
    xyz = rows[:, 0:3]
    assert np.isnan(xyz).any() and np.isposinf(xyz).any() and np.isneginf(xyz).any() and (np.abs(xyz[np.isfinite(xyz)]) >= 1e18).any()
    for count in sr.MEASURE_COUNTS:
        sel = sr.measure_selection(count)
        assert int((sel != 0).sum()) == count and set(np.unique(sel)) <= {0, 1, 255}
        if count >= 255:
            chosen = rows[sel != 0]
            assert (~np.isfinite(chosen[:, 0:3]).all(axis=1)).any() and (chosen[:, 3] == 0).any(), count
            assert (np.abs(chosen[:, 0:3][np.isfinite(chosen[:, 0:3])]) >= 1e18).any(), count
    # the numpy measure on a plane made up here: counts, box, bound and the sums' reference
    pos4 = np.concatenate([xyz, np.linspace(-1, 3, rows.shape[0], dtype=F)[:, None]], axis=1)
    pos4[5, 3], pos4[6, 3] = np.inf, np.nan
    m = sr.measure(pos4, sr.measure_selection(4097))
    fin = np.isfinite(xyz).all(axis=1)
    assert m["selected"] == 4097 and m["finite"] == fin.sum() < 4097
    assert (m["lo"] == xyz[fin].min(axis=0)).all() and m["reach2_max"] == F(3.0) and np.isfinite(m["sums"]).all() and (m["bounds"] > 0).all()
    empty = sr.measure(pos4, sr.measure_selection(0))
    assert empty["selected"] == 0 and empty["finite"] == 0 and np.isposinf(empty["lo"]).all() and np.isneginf(empty["hi"]).all()
    assert empty["reach2_max"] == 0 and not empty["sums"].any()


def test_the_shim_with_the_selection_methods_compiles_with_gxx(tmp_path):
    src = tmp_path / "select_shim.cpp"
    src.write_text("""
#include <cstddef>
#include "splatapult_amd/host/msplat_host.hpp"
static_assert(sizeof(msplat_cloud_measure) == 128 && offsetof(msplat_cloud_measure, sum2) == 80 && offsetof(msplat_cloud_measure, selected) == 8,
              "the layout the ctypes binding assumes");
int main()
{
    SplatRenderer r;
    const float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    msplat::mat4 cam{}, proj{};
    msplat::vec4 vp{{0, 0, 8, 8}};
    msplat::vec2 nf{{0.1f, 10.0f}};
    msplat_cloud_measure out;
    // no context yet: every call on the renderer is refused, none crashes
    bool ok = !r.MarkVolume(m, MSPLAT_CROP_SPHERE | MSPLAT_CROP_INVERT, nullptr, 0, 1) && !r.MarkView(cam, proj, vp, nf, nullptr, nullptr, 0, 1) &&
              !r.MeasureCloud(nullptr, 0, &out) && out.struct_size == sizeof(msplat_cloud_measure);
    out.finite = out.selected = 1;
    for (int k = 0; k < 3; ++k) { out.lo[k] = -1.0f; out.hi[k] = 3.0f; }
    float box[16];
    ok = ok && SplatRenderer::MeasureBox(out, 0.5f, box) && box[0] > 0.39f && box[0] < 0.4f && box[12] < -0.39f && box[15] == 1.0f;
    ok = ok && msplat_mark_volume(nullptr, m, MSPLAT_CROP_BOX, nullptr, 0, 0) == MSPLAT_ERR_INVALID_ARG;
    ok = ok && msplat_measure_cloud(nullptr, nullptr, 0, &out) == MSPLAT_ERR_INVALID_ARG;
    return ok ? 0 : 1;
}
""")
    exe, libdir = str(tmp_path / "select_shim"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, cwd=ROOT)
    assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 0
