"""GPU tests of selection by position (msplat_mark_volume, msplat_mark_view, msplat_measure_cloud, msplat_measure_box; INTEGRATION.md
28).  The marks are compared byte for byte with the header's rules restated in numpy float32 (tests/visibility_rule.py's crop(),
tests/select_rule.py's view_inside()), with msplat_set_crop itself, and -- for general cameras -- with the rule in float64 wherever
rounding cannot decide; the measure's exact fields with numpy over the position plane the kernels read
(msplat_debug_get_positions), its sums with math.fsum inside the header's bound.  Clouds hold at most 4097 splats, viewports at most
256 x 160 pixels; tests/test_select.py checks the fixtures on the CPU."""
import ctypes as C
import math

import numpy as np
import pytest

from splatapult_amd import MsplatError, _capi, measure_box
from tests import scenes
from tests import select_rule as sr
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import make_renderer, sorted_frame

pytestmark = pytest.mark.gpu

OFF, ON = _capi.SPATIAL_OFF, _capi.SPATIAL_ON
ORDERS = pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
DEV = "cuda:0"
F = np.float32
_P = C.POINTER(C.c_float)


def filled(n, value):
    import torch
    t = torch.full((n,), value, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    return t


def to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    torch.cuda.synchronize()
    return t


def host(r, t):
    r.synchronize()
    return t.cpu().numpy()


def fptr(a):
    return np.ascontiguousarray(np.asarray(a, F).reshape(-1)).ctypes.data_as(_P)


# ---- 1. mark_volume is the crop rule ------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("n", vr.SIZES)
def test_mark_volume_is_the_crop_rule(n, spatial):
    aos = vr.crop_cloud()[:n].copy()
    aos[30, 0], aos[n - 1, 2] = np.nan, np.nan                        # NaN centres: outside, so marked only under INVERT
    r = make_renderer(aos, spatial_order=spatial)
    assert (r.storage_order() is not None) == (spatial == ON)
    xyz = aos[:, 0:3]
    for matrix, shape, invert in vr.CROPS:
        M = vr.matrices()[matrix]
        mask = filled(n, 7)
        r.MarkVolume(M, mask, 9, shape, invert)
        want = np.where(vr.crop(xyz, M, shape, invert), 9, 7).astype(np.uint8)
        got = host(r, mask)
        same_bits(got, want, "n %d, %s %s%s" % (n, matrix, shape, " inverted" if invert else ""))
        assert got[30] == (9 if invert else 7) and got[n - 1] == (9 if invert else 7)
        assert 0 < (got == 9).sum() < n
    r.close()


# ---- 2. mark_volume closes the loop with the crop --------------------------------------------------------------------------------
def test_a_marked_mask_hides_what_the_crop_hides():
    aos = vr.crop_cloud()
    n, view = aos.shape[0], vr.view()
    a, b = make_renderer(aos, spatial_order=OFF), make_renderer(aos, spatial_order=OFF)
    L = _capi.lib()
    for k, (matrix, shape, invert) in enumerate(vr.CROPS):
        what = "%s %s%s" % (matrix, shape, " inverted" if invert else "")
        M = vr.matrices()[matrix]
        a.SetCrop(M, shape, invert)
        mask = filled(n, 1)
        if k % 4 == 1:            # the two calls back to back on the context's stream, nothing between them
            code = _capi.CROP_SHAPES[shape] | (0 if invert else _capi.CROP_INVERT)
            assert L.msplat_mark_volume(b._ctx, fptr(M), code, C.c_void_p(mask.data_ptr()), n, 0) == _capi.OK, b.last_error()
            assert L.msplat_set_visibility_device(b._ctx, C.c_void_p(mask.data_ptr()), n) == _capi.OK, b.last_error()
        else:
            b.MarkVolume(M, mask, 0, shape, invert=not invert)      # 0 where the crop hides
            b.SetVisibility(mask)
        fa, fb = sorted_frame(a, view), sorted_frame(b, view)
        va, vb = a.visibility(), b.visibility()
        assert va["hidden"] == vb["hidden"] == n - int(vr.crop(aos[:, 0:3], M, shape, invert).sum()), (what, va, vb)
        assert vb["has_mask"] and vb["crop"] is None and va["crop"] == (shape, invert)
        for key in ("keys", "idx", "img"):
            same_bits(fb[key], fa[key], "%s: %s" % (what, key))
        assert 0 < fa["V"] < n
    a.close(), b.close()


# ---- 3. mark_view, exact cases ---------------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("camera", list(sr.exact_cameras()))
def test_mark_view_on_designed_centres(camera, spatial):
    import torch
    cam, proj = sr.exact_cameras()[camera][:2]
    xyz = sr.exact_centres(camera)[0]
    n = xyz.shape[0]
    r = make_renderer(sr.splat_rows(xyz), spatial_order=spatial)
    mvp = sr.mvp_of(cam, proj)
    vp = [0, 0, sr.EW, sr.EH]
    for wname, win in sr.EXACT_WINDOWS.items():
        x0, y0, w, h = win if win is not None else (0, 0, sr.EW, sr.EH)
        region = sr.region_for(win, 11)
        wide = torch.zeros((h, w + 5), dtype=torch.uint8, device=DEV)          # a region plane with a pitch > w
        wide[:, :w] = torch.from_numpy(region).to(DEV)
        one = np.zeros((h, w), np.uint8)                                       # a one-pixel region
        one[h // 2, w // 3] = 3
        torch.cuda.synchronize()
        for rname, reg_arg, reg in (("no region", None, None), ("tight region", region, region), ("pitched region", wide[:, :w], region),
                                    ("one-pixel region", one, one)):
            mask = filled(n, 7)
            if reg_arg is None:
                raw_mark_view(r, cam, proj, vp, win, None, 0, mask, 9)          # the C call, nearFar NULL
            else:
                r.MarkView(cam, proj, vp, [0.1, 100.0], mask, 9, window=win, region=reg_arg)
            want = sr.marked(np.full(n, 7, np.uint8), sr.view_inside(xyz, mvp, sr.EW, sr.EH, win, reg), 9)
            same_bits(host(r, mask), want, "%s, window %s, %s" % (camera, wname, rname))
            assert (want == 9).any() or w * h == 1, (camera, wname, rname)      # (the random region of the 1 x 1 window may be 0)
    r.close()


def raw_mark_view(r, cam, proj, vp, win, region_ptr, pitch, mask, value, near_far=None, n=None):
    """msplat_mark_view itself, nearFar NULL unless given; the call's return code is asserted OK"""
    w = (C.c_int32 * 4)(*win) if win is not None else None
    rc = r._lib.msplat_mark_view(r._ctx, fptr(cam), fptr(proj), fptr(vp), fptr(near_far) if near_far is not None else None, w,
                                 C.c_void_p(region_ptr) if region_ptr else None, pitch, C.c_void_p(mask.data_ptr()), r._n if n is None else n, value)
    assert rc == _capi.OK, r.last_error()


# ---- 4. mark_view, general cameras -----------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("name", list(sr.general_views()))
def test_mark_view_follows_the_float64_rule_and_marks_a_subset_of_the_sort(name, spatial):
    aos = sr.general_cloud()
    n, xyz = aos.shape[0], aos[:, 0:3]
    cam, proj, vp, nf = sr.general_views()[name]
    mvp = sr.mvp_of(cam, proj)
    ok = sr.decidable(xyz, mvp, sr.GW, sr.GH)
    assert 1.0 - ok.mean() <= sr.MAX_LEFT_OUT
    r = make_renderer(aos, spatial_order=spatial)
    region = sr.general_region()
    whole = None
    for win, reg in ((None, None), (sr.GENERAL_WINDOW, None), (sr.GENERAL_WINDOW, region)):
        mask = filled(n, 0)
        r.MarkView(cam, proj, vp, nf, mask, 1, window=win, region=reg)
        got = host(r, mask) != 0
        want = sr.view_inside(xyz, mvp, sr.GW, sr.GH, win, reg, dtype=np.float64)
        wrong = (got != want) & ok
        print("%s, window %s, region %s: %d marked, %d compared, %d differ from the float64 rule, %d differ from numpy's fp32 rule"
              % (name, win, reg is not None, got.sum(), ok.sum(), wrong.sum(), (got != sr.view_inside(xyz, mvp, sr.GW, sr.GH, win, reg)).sum()))
        assert not wrong.any(), np.flatnonzero(wrong)[:10]
        assert 0 < got.sum() < n
        whole = got if win is None else whole
    r.Sort(cam, proj, vp, nf)
    seen = np.zeros(n, bool)
    seen[r.sorted_indices()] = True
    assert not (whole & ~seen).any(), "%d marked splat(s) are not in the Sort's visible set" % (whole & ~seen).sum()
    assert whole.sum() < seen.sum()                                    # (the Sort keeps a guard band around the viewport)
    r.close()


# ---- 5. select-through reaches what the frame does not show ----------------------------------------------------------------------
def wall_and_cluster():
    """(records, the cluster's upload indices): five dense sheets of opaque splats at z = 4.0 .. 3.6 in front of a cluster of
    small splats around z = 0.5, seen from z = 7: every pixel the cluster covers has lost its transmittance to the wall"""
    g = np.arange(-12, 13) * 0.1
    gx, gy = np.meshgrid(g, g)
    wall = np.concatenate([np.stack([gx.ravel() + 0.05 * (k % 2), gy.ravel(), np.full(gx.size, 4.0 - 0.1 * k)], axis=1) for k in range(5)])
    rng = np.random.default_rng(8)
    cluster = np.stack([rng.uniform(-0.5, 0.5, 200), rng.uniform(-0.5, 0.5, 200), rng.uniform(0.0, 1.0, 200)], axis=1)
    xyz = np.concatenate([cluster[:100], wall, cluster[100:]]).astype(F)
    idx = np.concatenate([np.arange(100), np.arange(100 + wall.shape[0], xyz.shape[0])])
    aos = sr.splat_rows(xyz)
    aos[:, 3] = 1.0
    aos[:, 16:25] = 0.0
    s2 = np.full(xyz.shape[0], 0.1 ** 2, F)
    s2[idx] = 0.03 ** 2
    aos[:, 16] = aos[:, 20] = aos[:, 24] = s2
    return aos, idx


def test_mark_view_marks_the_cluster_behind_the_wall():
    aos, cluster = wall_and_cluster()
    n = aos.shape[0]
    cam, proj, vp, nf = scenes.default_view(256, 160, z=7.0)
    cx, cy, _ = sr.centre_px(aos[cluster, 0:3], sr.mvp_of(cam, proj), 256, 160, np.float64)
    x0, y0 = int(cx.min()) - 2, int(cy.min()) - 2
    win = (x0, y0, int(cx.max()) + 3 - x0, int(cy.max()) + 3 - y0)
    lasso = np.ones((win[3], win[2]), np.uint8)
    lasso[0, 0] = lasso[-1, -1] = 0
    r = make_renderer(aos)
    r.Sort(cam, proj, vp, nf)
    assert np.isin(cluster, r.sorted_indices()).all(), "the cluster is in the view"
    score = host(r, r.RenderScores(cam, proj, vp, nf, window=win, region=lasso))
    assert (score[cluster] == 0).all(), "%d cluster splat(s) show through the wall" % (score[cluster] != 0).sum()
    assert (score > 0).sum() > 20                                      # the wall is what the lasso shows
    seen = filled(n, 0)
    r.MarkScores(r.RenderScores(cam, proj, vp, nf, window=win, region=lasso), "at_least", 1, seen, 1)
    through = filled(n, 0)
    r.MarkView(cam, proj, vp, nf, through, 1, window=win, region=lasso)
    seen, through = host(r, seen) != 0, host(r, through) != 0
    assert not seen[cluster].any() and through[cluster].all()
    assert (through & seen).any() and not through.all()               # wall splats under the lasso are marked by both
    r.close()


# ---- 6. measure_cloud ------------------------------------------------------------------------------------------------------------
def raw_measure(r, select):
    m = _capi.CloudMeasure(struct_size=C.sizeof(_capi.CloudMeasure))
    rc = r._lib.msplat_measure_cloud(r._ctx, C.c_void_p(select.data_ptr()) if select is not None else None, r._n, C.byref(m))
    assert rc == _capi.OK, r.last_error()
    return bytes(m)


@ORDERS
@pytest.mark.parametrize("grid_cap", [None, 1, 5], ids=["default_grid", "one_workgroup", "five_workgroups"])
def test_measure_cloud_counts_boxes_and_sums(grid_cap, spatial, monkeypatch):
    if grid_cap is not None:
        monkeypatch.setenv("MSPLAT_GRID_CAP", str(grid_cap))          # read when the context is created
    aos = sr.measure_rows()
    n = aos.shape[0]
    r = make_renderer(aos, spatial_order=spatial)
    pos4 = r.debug_positions()
    same_bits(pos4[:, 0:3], aos[:, 0:3], "the position plane holds the uploaded centres")
    w = pos4[:, 3]
    assert (w == 0).any() and np.isposinf(w).any() and (np.isfinite(w) & (w > 0)).any(), "footprint bounds of 0, inf and in between"
    for count in sr.MEASURE_COUNTS + (None,):
        sel = None if count is None else sr.measure_selection(count)
        want = sr.measure(pos4, sel)
        t = None if sel is None else to_device(sel)
        got = r.MeasureCloud(t)
        what = "%s selected, grid cap %s" % (count, grid_cap)
        assert got["selected"] == want["selected"] == (n if count is None else count), what
        assert got["finite"] == want["finite"], what
        assert (got["lo"] == want["lo"]).all() and (got["hi"] == want["hi"]).all(), (what, got["lo"], want["lo"], got["hi"], want["hi"])
        assert got["reach2_max"] == want["reach2_max"] and np.isfinite(got["reach2_max"]), (what, got["reach2_max"], want["reach2_max"])
        sums = np.concatenate([got["sum"], got["sum2"]])
        err = np.abs(sums - want["sums"])
        print("%s: finite %d, worst |sum - fsum| / bound %.3g" % (what, want["finite"], float((err / np.maximum(want["bounds"], 1e-300)).max())))
        assert (err <= want["bounds"]).all(), (what, err, want["bounds"])
        if want["finite"]:
            assert (got["mean"] == got["sum"] / got["finite"]).all() and got["covariance"].shape == (3, 3)
            assert (got["covariance"] == got["covariance"].T).all()
        else:
            assert got["mean"] is None and got["covariance"] is None
        assert raw_measure(r, t) == raw_measure(r, t), "%s: the same call twice returned different bytes" % what
    r.close()


PINNED = "select_pinned_bytes.npz"       # tests/golden: recorded by pinned_results() (see test_measure_and_summary_bytes_are_pinned)


def pinned_results(setenv):
    """{name: array}: the raw msplat_cloud_measure of every selection of the designed cloud, and the raw msplat_value_summary and the
    counts of every designed value array at 64 bins with and without d_select -- at grid caps 1 and 5 (the two that fix the summation
    tree) and in both storage orders.  setenv(name, value) sets MSPLAT_GRID_CAP, which a context reads when it is created"""
    from tests import values_rule as vl
    out = {}
    for cap in (1, 5):
        setenv("MSPLAT_GRID_CAP", str(cap))
        for spatial, order in ((OFF, "upload_order"), (ON, "morton_order")):
            r = make_renderer(sr.measure_rows(), spatial_order=spatial)
            for count in sr.MEASURE_COUNTS + (None,):
                t = None if count is None else to_device(sr.measure_selection(count))
                out["measure/cap%d/%s/%s" % (cap, order, count)] = np.frombuffer(raw_measure(r, t), np.uint8).copy()
            r.close()
            r = make_renderer(vl.cloud(vl.HIST_N), spatial_order=spatial)
            for name, (v, lo, hi) in vl.hist_inputs().items():
                d_v = to_device(v)
                for sname, sel in (("all", None), ("d_select", to_device(vl.hist_select()))):
                    counts = np.full(64, 0xAAAAAAAA, np.uint32)
                    key = "cap%d/%s/%s/%s" % (cap, order, name, sname)
                    s = _capi.ValueSummary(struct_size=C.sizeof(_capi.ValueSummary))
                    rc = r._lib.msplat_histogram_values(r._ctx, C.c_void_p(d_v.data_ptr()), C.c_void_p(sel.data_ptr()) if sel is not None else None,
                                                        r._n, lo, hi, 64, counts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(s))
                    assert rc == _capi.OK, r.last_error()
                    out["summary/" + key] = np.frombuffer(bytes(s), np.uint8).copy()
                    out["counts/" + key] = counts
            r.close()
    return out


def test_measure_and_summary_bytes_are_pinned(monkeypatch, golden_dir):
    """msplat_measure_cloud and msplat_histogram_values return the bytes they returned when the fixture was recorded (with
    pinned_results(), at the commit before the row reductions were folded into msplat_rows.hip.h): the order of every
    floating-point addition -- lane loop, wave butterfly, waves in wave order, finish rows in lane stride -- is part of the result"""
    import os
    want = np.load(os.path.join(golden_dir, PINNED))
    got = pinned_results(monkeypatch.setenv)
    assert sorted(got) == sorted(want.files) and len(got) == 2 * 2 * (len(sr.MEASURE_COUNTS) + 1 + 2 * 2 * 5)
    for name in sorted(got):
        kind = name.split("/")[0]
        assert got[name].size == {"counts": 64, "measure": C.sizeof(_capi.CloudMeasure), "summary": C.sizeof(_capi.ValueSummary)}[kind], name
        same_bits(got[name], want[name], name)


# ---- 7. measure -> box -> mark ---------------------------------------------------------------------------------------------------
@ORDERS
def test_the_measured_box_marks_the_selection(spatial):
    aos = sr.general_cloud().copy()
    aos[77, 1] = np.nan
    n, xyz = aos.shape[0], aos[:, 0:3]
    r = make_renderer(aos, spatial_order=spatial)
    sel = filled(n, 0)
    r.MarkVolume(vr.matrices()["rotated"], sel, 1, "sphere")
    sel[77] = 1                                                        # ... and the NaN centre: selected, not finite
    chosen = host(r, sel) != 0
    m = r.MeasureCloud(sel)
    fin = chosen & np.isfinite(xyz).all(axis=1)
    assert m["selected"] == chosen.sum() and m["finite"] == fin.sum() == m["selected"] - 1 and 100 < m["finite"] < n - 100
    for pad in (0.0, float(np.sqrt(m["reach2_max"]))):
        M = measure_box(m, pad)
        mask = filled(n, 0)
        r.MarkVolume(M, mask, 1, "box")
        got = host(r, mask) != 0
        assert got[fin].all(), "pad %g: %d selected centre(s) are outside their own box" % (pad, (~got[fin]).sum())
        lo, hi = m["lo"].astype(np.float64), m["hi"].astype(np.float64)
        c, h = 0.5 * (lo + hi), (0.5 * (hi - lo) + pad) * (1.0 + 1e-5)
        with np.errstate(invalid="ignore"):
            beyond = (np.abs(xyz.astype(np.float64) - c) > h).any(axis=1)
        assert not (got & beyond).any(), "pad %g: %d centre(s) beyond the padded box are marked" % (pad, (got & beyond).sum())
        assert not got[77] and got.sum() < n
    assert pad > 0
    r.close()


# ---- 8. downstream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edit, storage", [("transform", "sh_fp16"), ("adjust", "sh_q8")])
def test_a_marked_mask_selects_for_the_cloud_edits(edit, storage):
    aos = vr.crop_cloud()[:1025]
    n = aos.shape[0]
    M = vr.matrices()["rotated"]
    rule = vr.crop(aos[:, 0:3], M, "box")
    move = np.eye(4, dtype=F)
    move[3, 0:3] = (0.5, -0.25, 2.0)                                  # column-major: a translation
    out = []
    for route in ("marked", "uploaded"):
        r = make_renderer(aos, cloud_storage=storage)
        if route == "marked":
            sel = filled(n, 0)
            r.MarkVolume(M, sel, 255, "box")
        else:
            sel = rule
        if edit == "transform":
            r.TransformCloud(move.reshape(16), sel)
        else:
            r.AdjustCloud(colour=np.array([[0.5, 0.1, 0, 0.2], [0, 0.75, 0, 0], [0.25, 0, 1, -0.1]], F), opacity=0.5, select=sel)
        assert r.cloud_storage() == storage
        out.append(r.download_cloud(True))
        r.close()
    same_bits(out[0], out[1], "%s of the marked selection against the rule's mask" % edit)
    assert 0 < rule.sum() < n and (out[0][rule] != aos[rule]).any() and (out[0][~rule, 0:4] == aos[~rule, 0:4]).all()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_context_as_it_was():
    import torch
    L = _capi.lib()
    n, view = 257, vr.view()
    aos = vr.cloud_aos(n)
    r = make_renderer(aos)
    before = sorted_frame(r, view)
    cam, proj, vp, nf = view
    W, H = vp[2], vp[3]
    mask = filled(n + 1, 5)
    region = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    host_bytes = np.ones(W * H + 16, np.uint8)
    at = host_bytes.ctypes.data
    ident = np.eye(4, dtype=F).reshape(16)
    bad = ident.copy()
    bad[9] = np.inf
    d_mask, p = C.c_void_p(mask.data_ptr()), lambda v: C.c_void_p(v) if v else None
    m = _capi.CloudMeasure(struct_size=C.sizeof(_capi.CloudMeasure))

    def refused(rc, code, who, words):
        msg = r.last_error()
        assert rc == code and who in msg and all(w in msg for w in words), (rc, code, msg)

    volume = lambda M=ident, shape=_capi.CROP_BOX, ptr=d_mask, k=n: L.msplat_mark_volume(r._ctx, fptr(M) if M is not None else None, shape, ptr, k, 9)
    for kw, words in ((dict(M=None), ["worldToVolume is NULL"]), (dict(shape=_capi.CROP_NONE), ["shape"]), (dict(shape=5), ["shape"]),
                      (dict(shape=_capi.CROP_INVERT), ["shape"]), (dict(M=bad), ["worldToVolume[9]", "not finite"]), (dict(k=n - 1), ["mask bytes"]),
                      (dict(k=n + 1), ["mask bytes"]), (dict(k=0), ["mask bytes"]), (dict(ptr=None), ["d_mask is NULL"]),
                      (dict(ptr=p(at)), ["d_mask", "not device memory"])):
        refused(volume(**kw), _capi.ERR_INVALID_ARG, "msplat_mark_volume", words)

    def view_call(cam_=cam, vp_=vp, win=None, reg=None, pitch=0, ptr=d_mask, k=n):
        w = (C.c_int32 * 4)(*win) if win is not None else None
        return L.msplat_mark_view(r._ctx, fptr(cam_) if cam_ is not None else None, fptr(proj), fptr(vp_) if vp_ is not None else None, None, w,
                                  p(reg), pitch, ptr, k, 9)

    for kw, words in ((dict(cam_=None), ["NULL"]), (dict(vp_=None), ["NULL"]), (dict(k=n + 1), ["mask bytes"]), (dict(ptr=None), ["d_mask is NULL"]),
                      (dict(ptr=p(at)), ["d_mask", "not device memory"]), (dict(reg=at), ["d_region", "not device memory"]),
                      (dict(reg=region.data_ptr(), pitch=W - 1), ["region pitch"]),
                      (dict(win=(0, 0, 40, 9), reg=region.data_ptr(), pitch=39), ["region pitch"])):
        refused(view_call(**kw), _capi.ERR_INVALID_ARG, "msplat_mark_view", words)
    for win in ((0, 0, 0, 4), (0, 0, 4, 0), (-1, 0, 4, 4), (W - 3, 0, 4, 4), (0, H - 3, 4, 4), (0, 0, W + 1, H), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)):
        refused(view_call(win=win), _capi.ERR_INVALID_ARG, "msplat_mark_view", ["window", "not inside"])
    refused(view_call(vp_=[0, 0, 8193, 8]), _capi.ERR_UNSUPPORTED, "msplat_mark_view", ["8193"])

    measure = lambda ptr=None, k=n, out=C.byref(m): L.msplat_measure_cloud(r._ctx, ptr, k, out)
    refused(measure(out=None), _capi.ERR_INVALID_ARG, "msplat_measure_cloud", ["out is NULL"])
    refused(measure(k=n - 1), _capi.ERR_INVALID_ARG, "msplat_measure_cloud", ["mask bytes"])
    refused(measure(ptr=p(at)), _capi.ERR_INVALID_ARG, "msplat_measure_cloud", ["d_select", "not device memory"])
    m.struct_size = _capi.CloudMeasure.sum2.offset + 40
    refused(measure(), _capi.ERR_INVALID_ARG, "msplat_measure_cloud", ["struct_size"])
    m.struct_size = C.sizeof(_capi.CloudMeasure)
    assert measure() == _capi.OK and m.selected == n                  # d_select NULL: every splat

    r.synchronize()
    assert (mask.cpu().numpy() == 5).all() and (host_bytes == 1).all(), "a refused call wrote"
    after = sorted_frame(r, view)
    for key in ("keys", "idx", "img"):
        same_bits(after[key], before[key], "after the refusals: %s" % key)
    with pytest.raises(ValueError):
        r.MarkVolume(ident, mask, 1)                                   # n + 1 bytes
    with pytest.raises(ValueError):
        r.MarkView(cam, proj, vp, nf, mask[:n], 1, window=(0, 0, W + 1, 1))
    with pytest.raises(ValueError):
        r.MarkVolume(ident, mask[:n], 1, shape="cone")
    r.close()

    # before an upload; with a point cloud (which still renders)
    cfg = _capi.Config()
    cfg.struct_size = C.sizeof(_capi.Config)
    cfg.t_epsilon = -1.0
    h = C.c_void_p()
    assert L.msplat_create(C.byref(h), C.byref(cfg)) == _capi.OK
    fp = [fptr(x) for x in (cam, proj, vp, nf)]
    assert L.msplat_mark_volume(h, fptr(ident), _capi.CROP_BOX, d_mask, n, 9) == _capi.ERR_NO_CLOUD and b"msplat_mark_volume" in L.msplat_last_error(h)
    assert L.msplat_mark_view(h, *fp, None, None, 0, d_mask, n, 9) == _capi.ERR_NO_CLOUD and b"msplat_mark_view" in L.msplat_last_error(h)
    assert L.msplat_measure_cloud(h, None, n, C.byref(m)) == _capi.ERR_NO_CLOUD and b"msplat_measure_cloud" in L.msplat_last_error(h)
    pts = np.random.default_rng(81).uniform(-1, 1, (500, 8)).astype(F)
    pts[:, 3] = 1.0
    pts[:, 4:] = np.abs(pts[:, 4:])
    assert L.msplat_upload_points(h, pts.ctypes.data, pts.shape[0], 32, 0, 16) == _capi.OK
    assert L.msplat_sort(h, *fp) == _capi.OK
    img0, img1 = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    assert L.msplat_render(h, *fp, img0.ctypes.data, 0, 0) == _capi.OK
    assert L.msplat_mark_volume(h, fptr(ident), _capi.CROP_BOX, d_mask, 500, 9) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    assert L.msplat_mark_view(h, *fp, None, None, 0, d_mask, 500, 9) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    assert L.msplat_measure_cloud(h, None, 500, C.byref(m)) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    assert L.msplat_render(h, *fp, img1.ctypes.data, 0, 0) == _capi.OK
    same_bits(img1, img0, "the point context renders what it rendered")
    L.msplat_destroy(h)
    torch.cuda.synchronize()
    assert (mask.cpu().numpy() == 5).all()


def test_example_render_selects_a_sphere_prints_its_measure_and_highlights_it(tmp_path, golden_dir):
    """SplatRenderer::MarkVolume / MeasureCloud (msplat_host.hpp) through example_render --select-sphere: the printed count is the
    rule's, the printed box lies inside the sphere's, and with --highlight the frame changes where without it it does not"""
    import os
    import re
    import subprocess
    from splatapult_amd import GaussianCloud
    from tests.conftest import ROOT
    exe, libdir = str(tmp_path / "example_render"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-I", ROOT, os.path.join(ROOT, "splatapult_amd", "host", "example_render.cpp"),
                    "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    W, H = 320, 200
    ply = os.path.join(golden_dir, "test.ply")
    gc = GaussianCloud()
    assert gc.ImportPly(ply)
    xyz = gc.as_array()[:, 0:3]
    centre = np.median(xyz, axis=0).astype(F)
    radius = F(np.quantile(np.linalg.norm(xyz - centre, axis=1), 0.4))
    s = F(1.0) / radius
    M = np.array([s, 0, 0, 0, 0, s, 0, 0, 0, 0, s, 0, -centre[0] * s, -centre[1] * s, -centre[2] * s, 1], F)     # the tool's fp32 matrix
    inside = vr.crop(xyz, M, "sphere")
    assert 0 < inside.sum() < xyz.shape[0]
    arg = "%.9g,%.9g,%.9g,%.9g" % (centre[0], centre[1], centre[2], radius)
    outs = [str(tmp_path / ("o%d.f32" % k)) for k in range(3)]
    subprocess.run([exe, ply, outs[0], str(W), str(H)], check=True, timeout=120)
    said = subprocess.run([exe, ply, outs[1], str(W), str(H), "--select-sphere", arg], check=True, timeout=120, capture_output=True, text=True).stdout
    m = re.search(r"select sphere: (\d+) of (\d+) splats, box \(([^)]*)\) \.\. \(([^)]*)\), centroid \(([^)]*)\)", said)
    assert m, said
    assert (int(m.group(1)), int(m.group(2))) == (int(inside.sum()), xyz.shape[0]), said
    lo, hi, mean = (np.array([float(v) for v in m.group(k).split(",")]) for k in (3, 4, 5))
    assert np.allclose(lo, xyz[inside].min(axis=0), rtol=1e-5) and np.allclose(hi, xyz[inside].max(axis=0), rtol=1e-5), said
    assert np.allclose(mean, xyz[inside].astype(np.float64).mean(axis=0), rtol=1e-4, atol=1e-6), said
    said = subprocess.run([exe, ply, outs[2], str(W), str(H), "--select-sphere", arg, "--highlight", "1,0,0,0.8"], check=True, timeout=120,
                          capture_output=True, text=True).stdout
    assert "the selection is highlighted" in said, said
    plain, selected, tinted = (np.fromfile(p, np.float32).reshape(H, W, 4) for p in outs)
    same_bits(selected, plain, "selecting and measuring changes no pixel")
    assert np.abs(tinted - plain).max() > 0.05


def test_an_empty_cloud_is_marked_and_measured():
    r = make_renderer(np.zeros((0, 61), F))
    import torch
    empty = torch.zeros(0, dtype=torch.uint8, device=DEV)
    L = _capi.lib()
    assert L.msplat_mark_volume(r._ctx, fptr(np.eye(4)), _capi.CROP_SPHERE, None, 0, 1) == _capi.OK
    cam, proj, vp, nf = vr.view()
    assert L.msplat_mark_view(r._ctx, fptr(cam), fptr(proj), fptr(vp), None, None, None, 0, None, 0, 1) == _capi.OK
    m = r.MeasureCloud(empty)
    assert m["selected"] == 0 and m["finite"] == 0 and np.isposinf(m["lo"]).all() and np.isneginf(m["hi"]).all() and m["mean"] is None
    with pytest.raises(MsplatError) as e:
        measure_box(m)
    assert e.value.code == _capi.ERR_INVALID_ARG
    r.close()
