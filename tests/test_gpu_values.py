"""GPU tests of selection by attribute (msplat_cloud_values, msplat_mark_values, msplat_histogram_values).  The
values are compared with the header's rule restated in numpy float32 (tests/values_rule.py) applied to what msplat_download_cloud and
the position plane return -- copies and fp32 kinds bit for bit, the SCALE kinds within rtol 1e-6 --, the marks byte for byte, the
histogram's counts and every summary field exactly.  Clouds hold at most 4097 splats; tests/test_values.py checks the fixtures and
the decidable thresholds on the CPU."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import MsplatError, _capi
from tests import values_rule as vl
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import make_renderer, sorted_frame

pytestmark = pytest.mark.gpu

OFF, ON = _capi.SPATIAL_OFF, _capi.SPATIAL_ON
ORDERS = pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
# (cloud_storage, full SH): FP32 full and degree-1, SH_FP16 full and degree-1, SH_Q8 full
STORES = {"fp32": ("fp32", True), "fp32_degree1": ("fp32", False), "sh_fp16": ("sh_fp16", True), "sh_fp16_degree1": ("sh_fp16", False),
          "sh_q8": ("sh_q8", True)}
DEV = "cuda:0"
F = np.float32
_P = C.POINTER(C.c_float)
SENTINEL = F(-12345.5)
PAD = 19            # floats of sentinel on both sides of d_values: the array starts 4-byte aligned and no better


def filled(n, value):
    import torch
    t = torch.full((n,), value, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    return t


def to_device(a):
    import torch
    t = torch.from_numpy(np.array(a)).to(DEV)                          # (a copy: the fixtures are read-only)
    torch.cuda.synchronize()
    return t


def host(r, t):
    r.synchronize()
    return t.cpu().numpy()


def padded_values(n):
    import torch
    buf = torch.full((n + 2 * PAD,), float(SENTINEL), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    return buf, buf[PAD:PAD + n]


def close_scales(got, want, what):
    """rtol 1e-6 with equal zeros (the bound close_to_rule sets for the same eigenvalues); returns the rows that are not bit-equal"""
    assert ((got == 0) == (want == 0)).all(), "%s: other zeros" % what
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=what)
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())


# ---- 1. the values are the rule's ----------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("n", vl.SIZES)
def test_values_equal_the_rule(n, store, spatial):
    storage, full_sh = STORES[store]
    aos = vl.cloud(n, full_sh)
    r = make_renderer(aos, cloud_storage=storage, spatial_order=spatial)
    assert (r.storage_order() is not None) == (spatial == ON and n > 1) and r.cloud_storage() == storage      # (one splat has no order)
    rec, pos4 = r.download_cloud(full_sh), r.debug_positions()
    head = [0, 1, 2, 3, 4, 8, 12] + list(range(16, 25))
    same_bits(rec[:, head], aos[:, head], "the head of every storage kind holds the uploaded floats")
    same_bits(pos4[:, 0:3], aos[:, 0:3], "the position plane holds the uploaded centres")
    not_bit_equal = 0
    for kind in vl.KINDS:
        what = "n %d, %s, %s" % (n, store, kind)
        buf, out = padded_values(n)
        got_t = r.CloudValues(kind, vl.PARAMS.get(kind), out=out)
        assert got_t.data_ptr() == out.data_ptr()
        whole = host(r, buf)
        got, want = whole[PAD:PAD + n], vl.values(rec, pos4, kind, vl.PARAMS.get(kind))
        assert (whole[:PAD] == SENTINEL).all() and (whole[PAD + n:] == SENTINEL).all(), "%s: the padding around d_values was written" % what
        if kind in vl.SCALE_KINDS:
            not_bit_equal += close_scales(got, want, what)
        else:
            same_bits(got, want, what)
    print("n %d, %s, order %d: %d of %d SCALE values are not bit-equal to the numpy rule" % (n, store, spatial, not_bit_equal, 3 * n))
    # by number, and into a tensor of its own
    same_bits(host(r, r.CloudValues(_capi.VALUE_KINDS["alpha"])), rec[:, 3].copy(), "alpha by number")
    r.close()


# ---- 2. mark_values --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", vl.SIZES)
def test_mark_values_is_the_range_rule(n):
    aos = vl.cloud(n)
    r = make_renderer(aos, spatial_order=ON if n > 64 else OFF)
    rec, pos4 = r.download_cloud(True), r.debug_positions()
    checked = 0
    for kind in ("alpha", "colour_dist2", "x") + vl.SCALE_KINDS:
        values = r.CloudValues(kind, vl.PARAMS.get(kind))
        want_v = vl.values(rec, pos4, kind, vl.PARAMS.get(kind))
        if kind in vl.SCALE_KINDS:
            ranges = []
            for t in vl.scale_thresholds(kind).values():       # decidable: no rule value within 1e-5 of t, the device's within 1e-6
                ranges += [(-np.inf, t), (t, np.inf), (t, t)]
        else:
            same_bits(host(r, values), want_v, kind)
            fin = np.sort(want_v[np.isfinite(want_v)])
            a, b = (fin[fin.shape[0] // 4], fin[(3 * fin.shape[0]) // 4]) if fin.shape[0] else (F(0.0), F(1.0))
            # everything; an empty range; thresholds equal to values (closed ends); one value alone; one-sided
            ranges = [(-np.inf, np.inf), (b, a) if a != b else (1.0, 0.0), (a, b), (a, a), (-np.inf, a), (np.nextafter(b, F(np.inf)), np.inf)]
        for lo, hi in ranges:
            for outside in (False, True):
                mask = filled(n, 7)
                r.MarkValues(values, lo, hi, mask, 9, outside=outside)
                want = vl.marked(np.full(n, 7, np.uint8), want_v, lo, hi, outside, 9)
                same_bits(host(r, mask), want, "n %d, %s in [%r, %r], outside %s" % (n, kind, lo, hi, outside))
                checked += 1
        if kind == "alpha" and n >= 63:
            nan = np.isnan(want_v)
            assert nan.any() and np.isinf(want_v).any()
            inside_all, outside_all = filled(n, 0), filled(n, 0)
            r.MarkValues(values, -np.inf, np.inf, inside_all, 1)
            r.MarkValues(values, -np.inf, np.inf, outside_all, 1, outside=True)
            assert (host(r, inside_all) == ~nan).all() and (host(r, outside_all) == nan).all(), "a NaN value is marked under OUTSIDE only"
    assert checked >= 60
    r.close()


# ---- 3. the histogram ------------------------------------------------------------------------------------------------------------
def raw_histogram(r, values, select, bins, lo, hi, counts):
    s = _capi.ValueSummary(struct_size=C.sizeof(_capi.ValueSummary))
    rc = r._lib.msplat_histogram_values(r._ctx, C.c_void_p(values.data_ptr()), C.c_void_p(select.data_ptr()) if select is not None else None,
                                        r._n, lo, hi, bins, counts.ctypes.data_as(C.POINTER(C.c_uint32)) if counts is not None else None, C.byref(s))
    assert rc == _capi.OK, r.last_error()
    return bytes(s)


@pytest.mark.parametrize("selected", [False, True], ids=["all", "d_select"])
@pytest.mark.parametrize("grid_cap", [None, 1, 5], ids=["default_grid", "one_workgroup", "five_workgroups"])
@pytest.mark.parametrize("bins", [1, 2, 64, 1000, 4096])
def test_histogram_counts_and_summary_equal_the_rule(bins, grid_cap, selected, monkeypatch):
    if grid_cap is not None:
        monkeypatch.setenv("MSPLAT_GRID_CAP", str(grid_cap))          # read when the context is created
    r = make_renderer(vl.cloud(vl.HIST_N), spatial_order=ON)
    sel = vl.hist_select() if selected else None
    d_sel = to_device(sel) if selected else None
    for name, (v, lo, hi) in vl.hist_inputs().items():
        what = "%s, %d bins, grid cap %s, %s" % (name, bins, grid_cap, "selected" if selected else "all")
        d_v = to_device(v)
        want = vl.histogram(v, sel, bins, lo, hi)
        got = r.HistogramValues(d_v, bins, lo, hi, select=d_sel)
        print("%s: selected %d finite %d nan %d below %d above %d, largest bin %d" % (
            what, got["selected"], got["finite"], got["nan"], got["below"], got["above"], int(got["counts"].max())))
        assert vl.summary_fields(got) == vl.summary_fields(want), (what, vl.summary_fields(got), vl.summary_fields(want))
        same_bits(got["counts"], want["counts"], what)
        assert int(got["counts"].sum()) + got["below"] + got["above"] + got["nan"] == got["selected"], what
        # the same call twice returns the same bytes
        c1, c2 = np.full(bins, 0xAAAAAAAA, np.uint32), np.full(bins, 0x55555555, np.uint32)
        assert raw_histogram(r, d_v, d_sel, bins, lo, hi, c1) == raw_histogram(r, d_v, d_sel, bins, lo, hi, c2), what
        same_bits(c1, c2, what + ": counts of two calls")
        same_bits(c1, want["counts"], what + ": counts of the C call")
    if bins == 1:
        eq = r.HistogramValues(to_device(vl.hist_inputs()["equal"][0]), 4096, 0.0, 1.0)
        assert eq["counts"].max() == vl.HIST_N and (eq["counts"] != 0).sum() == 1, "one hot bin"
    r.close()


def test_histogram_without_bins_returns_the_summary_alone():
    r = make_renderer(vl.cloud(vl.HIST_N))
    for name, (v, lo, hi) in vl.hist_inputs().items():
        d_v = to_device(v)
        for sel in (None, vl.hist_select()):
            want = vl.histogram(v, sel)
            got = r.HistogramValues(d_v, select=None if sel is None else to_device(sel))
            assert vl.summary_fields(got) == vl.summary_fields(want) and got["counts"].shape == (0,) and got["below"] == got["above"] == 0, name
        counts = np.full(8, 0xAAAAAAAA, np.uint32)
        raw_histogram(r, d_v, None, 0, float("nan"), float("nan"), counts)          # lo, hi and counts are not read
        assert (counts == 0xAAAAAAAA).all(), "bins == 0 wrote counts"
    nothing = to_device(np.zeros(vl.HIST_N, np.uint8))
    got = r.HistogramValues(d_v, 4, -1.0, 1.0, select=nothing)
    assert got["selected"] == 0 and got["finite"] == 0 and np.isposinf(got["vmin"]) and np.isneginf(got["vmax"]) and not got["counts"].any()
    # the values of a cloud: the histogram of a kind is the rule's of the rule's values
    alpha = r.CloudValues("alpha")
    want = vl.histogram(vl.rows()[:, 3], None, 64, 0.0, 1.0)
    got = r.HistogramValues(alpha, 64, 0.0, 1.0)
    assert vl.summary_fields(got) == vl.summary_fields(want) and got["nan"] == 1 and got["above"] == 1 and got["below"] == 1
    same_bits(got["counts"], want["counts"], "alpha of the fixture rows")
    r.close()


# ---- 4. closing the loop -----------------------------------------------------------------------------------------------------------
def test_alpha_marked_to_zero_hides_what_an_upload_without_those_rows_lacks():
    aos = vr.cloud_aos(*vr.TIE_FREE)
    n, view = aos.shape[0], vr.view()
    t = F(np.median(aos[:, 3]))
    keep = np.flatnonzero(aos[:, 3] >= t)
    assert 0 < keep.shape[0] < n and (aos[:, 3] == t).any()            # a value equal to the threshold is kept: the range is closed
    untouched = make_renderer(aos, spatial_order=OFF, enable_timing=1)
    a, b = make_renderer(aos, spatial_order=OFF), make_renderer(aos[keep], spatial_order=OFF)
    before = sorted_frame(untouched, view)
    mask = filled(n, 1)
    a.MarkValues(a.CloudValues("alpha"), t, np.inf, mask, 0, outside=True)
    a.SetVisibility(mask)
    fa, fb = sorted_frame(a, view), sorted_frame(b, view)
    assert fa["V"] == fb["V"] and a.visibility()["hidden"] == n - keep.shape[0]
    same_bits(fa["idx"], keep[fb["idx"]].astype(fa["idx"].dtype), "sorted indices")
    same_bits(fa["keys"], fb["keys"], "sorted keys")
    # every call of the feature on a context that is otherwise left alone: its next frame is the frame before, without another Sort
    for kind in vl.KINDS:
        v = untouched.CloudValues(kind, vl.PARAMS.get(kind))
        untouched.HistogramValues(v, 64, -1.0, 2.0)
        untouched.MarkValues(v, 0.0, 1.0, filled(n, 0), 1)
    tm = untouched.timings()                                           # (a read clears them: the one frame above is still all there is)
    assert tm["frames_averaged"] == 1.0 and tm["render_total"] > 0 and tm["sort_total"] > 0, tm
    same_bits(untouched.Render(*view), before["img"], "a Render after the value calls, no new Sort")
    after = sorted_frame(untouched, view)
    for key in ("keys", "idx", "img"):
        same_bits(after[key], before[key], "after the value calls: %s" % key)
    untouched.close(), a.close(), b.close()


@pytest.mark.parametrize("edit, storage, kind", [("transform", "sh_fp16", "scale_max"), ("adjust", "sh_q8", "colour_dist2")])
def test_a_value_mark_selects_for_the_cloud_edits(edit, storage, kind):
    n = 1025
    aos = vl.cloud(n)
    r = make_renderer(aos, cloud_storage=storage, spatial_order=ON)
    before, pos4 = r.download_cloud(True), r.debug_positions()
    rule_v = vl.values(before, pos4, kind, vl.PARAMS.get(kind))
    if kind == "scale_max":
        lo, hi = vl.scale_thresholds(kind)["needles"], np.inf
    else:
        lo, hi = -np.inf, F(np.median(rule_v[np.isfinite(rule_v)]))
    rule = vl.inside(rule_v, lo, hi)
    sel = filled(n, 0)
    r.MarkValues(r.CloudValues(kind, vl.PARAMS.get(kind)), lo, hi, sel, 255)
    same_bits(host(r, sel), np.where(rule, 255, 0).astype(np.uint8), "the mark")
    if edit == "transform":
        move = np.eye(4, dtype=F)
        move[3, 0:3] = (0.5, -0.25, 2.0)                              # column-major: a translation
        r.TransformCloud(move.reshape(16), sel)
    else:
        r.AdjustCloud(colour=np.array([[0.5, 0.1, 0, 0.2], [0, 0.75, 0, 0], [0.25, 0, 1, -0.1]], F), opacity=0.5, select=sel)
    assert r.cloud_storage() == storage
    after = r.download_cloud(True)
    same_bits(after[~rule], before[~rule], "%s: the unselected rows" % edit)
    assert 100 < rule.sum() < n - 100 and (after[rule] != before[rule]).any(axis=1).sum() > 0.9 * rule.sum()
    r.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_say_why_and_leave_the_context_as_it_was():
    import torch
    L = _capi.lib()
    n, view = 257, vr.view()
    aos = vr.cloud_aos(n)
    r = make_renderer(aos)
    before = sorted_frame(r, view)
    cam, proj, vp, nf = view
    mask = filled(n + 1, 5)
    vals = torch.full((n + 2,), 0.25, dtype=torch.float32, device=DEV)
    vals2 = torch.full((n + 2,), 0.25, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    host_floats = np.ones(n + 16, F)
    at = host_floats.ctypes.data
    d_mask, d_vals = C.c_void_p(mask.data_ptr()), C.c_void_p(vals.data_ptr())
    p = lambda v: C.c_void_p(v) if v else None
    three = (C.c_float * 4)(0.0, 0.0, 0.0, float("nan"))              # [3] is never read
    bad = (C.c_float * 4)(0.0, float("inf"), 0.0, 0.0)
    s = _capi.ValueSummary(struct_size=C.sizeof(_capi.ValueSummary))
    counts = np.full(4096, 0xAAAAAAAA, np.uint32)
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))
    K = _capi.VALUE_KINDS

    def refused(rc, code, who, words):
        msg = r.last_error()
        assert rc == code and who in msg and all(w in msg for w in words), (rc, code, msg)

    values = lambda kind=K["alpha"], param=None, ptr=d_vals, k=n: L.msplat_cloud_values(r._ctx, kind, param, ptr, k)
    for kw, words in ((dict(kind=13), ["kind 13"]), (dict(kind=-1), ["kind -1"]), (dict(kind=K["distance2"]), ["param is NULL"]),
                      (dict(kind=K["colour_dist2"], param=bad), ["param[1]", "not finite"]), (dict(k=n - 1), ["for a cloud of"]),
                      (dict(k=n + 1), ["for a cloud of"]), (dict(k=0), ["for a cloud of"]), (dict(ptr=None), ["d_values is NULL"]),
                      (dict(ptr=p(at)), ["d_values", "not device memory"]), (dict(ptr=p(vals.data_ptr() + 2)), ["d_values", "4-byte aligned"])):
        refused(values(**kw), _capi.ERR_INVALID_ARG, "msplat_cloud_values", words)
    assert values(kind=K["distance2"], param=three, ptr=C.c_void_p(vals2.data_ptr())) == _capi.OK, r.last_error()

    mark = lambda v=d_vals, k=n, lo=0.0, hi=1.0, op=_capi.RANGE_INSIDE, ptr=d_mask: L.msplat_mark_values(r._ctx, v, k, lo, hi, op, ptr, 9)
    for kw, words in ((dict(op=2), ["op 2"]), (dict(op=-1), ["op -1"]), (dict(lo=float("nan")), ["lo is NaN"]), (dict(hi=float("nan")), ["hi is NaN"]),
                      (dict(k=n + 1), ["for a cloud of"]), (dict(ptr=None), ["d_mask is NULL"]), (dict(ptr=p(at)), ["d_mask", "not device memory"]),
                      (dict(v=None), ["d_values is NULL"]), (dict(v=p(at)), ["d_values", "not device memory"]),
                      (dict(v=p(vals.data_ptr() + 1)), ["d_values", "4-byte aligned"])):
        refused(mark(**kw), _capi.ERR_INVALID_ARG, "msplat_mark_values", words)

    def hist(v=d_vals, sel=None, k=n, lo=0.0, hi=1.0, bins=4, c=cp, out=C.byref(s)):
        return L.msplat_histogram_values(r._ctx, v, sel, k, lo, hi, bins, c, out)

    for kw, words in ((dict(out=None), ["out is NULL"]), (dict(bins=4097), ["4097 bins"]), (dict(c=None), ["counts is NULL"]),
                      (dict(lo=1.0, hi=1.0), ["lo < hi"]), (dict(lo=2.0, hi=1.0), ["lo < hi"]), (dict(lo=float("nan")), ["lo < hi"]),
                      (dict(hi=float("inf")), ["lo < hi"]), (dict(lo=-3e38, hi=3e38, bins=1), ["not a normal fp32 number"]),
                      (dict(k=n - 1), ["for a cloud of"]), (dict(v=None), ["d_values is NULL"]), (dict(v=p(at)), ["d_values", "not device memory"]),
                      (dict(v=p(vals.data_ptr() + 2)), ["4-byte aligned"]), (dict(sel=p(at)), ["d_select", "not device memory"])):
        refused(hist(**kw), _capi.ERR_INVALID_ARG, "msplat_histogram_values", words)
    s.struct_size = _capi.ValueSummary.vmax.offset
    refused(hist(), _capi.ERR_INVALID_ARG, "msplat_histogram_values", ["struct_size"])
    s.struct_size = C.sizeof(_capi.ValueSummary)
    assert (counts == 0xAAAAAAAA).all(), "a refused call wrote counts"
    assert hist() == _capi.OK and s.selected == n and counts[1] == n and counts[4] == 0xAAAAAAAA          # 0.25 of [0, 1] in four bins

    r.synchronize()
    assert (mask.cpu().numpy() == 5).all() and (host_floats == 1).all(), "a refused call wrote"
    assert (vals.cpu().numpy() == F(0.25)).all(), "a refused call wrote"
    got = vals2.cpu().numpy()
    assert (got[n:] == F(0.25)).all() and (got[:n] != F(0.25)).any(), "the one accepted call wrote behind its n values"
    after = sorted_frame(r, view)
    for key in ("keys", "idx", "img"):
        same_bits(after[key], before[key], "after the refusals: %s" % key)
    with pytest.raises(ValueError):
        r.CloudValues("alpha", out=vals)                               # n + 2 floats
    with pytest.raises(ValueError):
        r.MarkValues(vals[:n], 0.0, 1.0, mask, 1)                      # n + 1 bytes
    with pytest.raises(ValueError):
        r.HistogramValues(vals[:n].double(), 4, 0.0, 1.0)
    with pytest.raises(MsplatError) as e:
        r.HistogramValues(vals[:n], 1, -3e38, 3e38)
    assert e.value.code == _capi.ERR_INVALID_ARG
    r.close()

    # before an upload; with a point cloud (which still renders)
    cfg = _capi.Config()
    cfg.struct_size = C.sizeof(_capi.Config)
    cfg.t_epsilon = -1.0
    h = C.c_void_p()
    assert L.msplat_create(C.byref(h), C.byref(cfg)) == _capi.OK
    fptr = lambda a: np.ascontiguousarray(np.asarray(a, F).reshape(-1)).ctypes.data_as(_P)
    fp = [fptr(x) for x in (cam, proj, vp, nf)]
    assert L.msplat_cloud_values(h, K["alpha"], None, d_vals, n) == _capi.ERR_NO_CLOUD and b"msplat_cloud_values" in L.msplat_last_error(h)
    assert L.msplat_mark_values(h, d_vals, n, 0.0, 1.0, 0, d_mask, 9) == _capi.ERR_NO_CLOUD and b"msplat_mark_values" in L.msplat_last_error(h)
    assert L.msplat_histogram_values(h, d_vals, None, n, 0.0, 1.0, 4, cp, C.byref(s)) == _capi.ERR_NO_CLOUD
    assert b"msplat_histogram_values" in L.msplat_last_error(h)
    pts = np.random.default_rng(81).uniform(-1, 1, (n, 8)).astype(F)
    pts[:, 3] = 1.0
    pts[:, 4:] = np.abs(pts[:, 4:])
    W, H = int(vp[2]), int(vp[3])
    assert L.msplat_upload_points(h, pts.ctypes.data, pts.shape[0], 32, 0, 16) == _capi.OK
    assert L.msplat_sort(h, *fp) == _capi.OK
    img0, img1 = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    assert L.msplat_render(h, *fp, img0.ctypes.data, 0, 0) == _capi.OK
    assert L.msplat_cloud_values(h, K["x"], None, d_vals, n) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    assert L.msplat_mark_values(h, d_vals, n, 0.0, 1.0, 0, d_mask, 9) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    assert L.msplat_histogram_values(h, d_vals, None, n, 0.0, 1.0, 4, cp, C.byref(s)) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    assert L.msplat_render(h, *fp, img1.ctypes.data, 0, 0) == _capi.OK
    same_bits(img1, img0, "the point context renders what it rendered")
    L.msplat_destroy(h)
    torch.cuda.synchronize()
    assert (mask.cpu().numpy() == 5).all()


def test_an_empty_cloud_succeeds_and_launches_nothing():
    import torch
    r = make_renderer(np.zeros((0, 61), F))
    L = _capi.lib()
    s = _capi.ValueSummary(struct_size=C.sizeof(_capi.ValueSummary))
    counts = np.full(4, 7, np.uint32)
    assert L.msplat_cloud_values(r._ctx, _capi.VALUE_KINDS["scale_max"], None, None, 0) == _capi.OK
    assert L.msplat_mark_values(r._ctx, None, 0, 0.0, 1.0, _capi.RANGE_OUTSIDE, None, 1) == _capi.OK
    assert L.msplat_histogram_values(r._ctx, None, None, 0, 0.0, 1.0, 4, counts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(s)) == _capi.OK
    assert (s.selected, s.finite, s.nan, s.below, s.above) == (0, 0, 0, 0, 0) and s.vmin == np.inf and s.vmax == -np.inf and not counts.any()
    empty = torch.zeros(0, dtype=torch.float32, device=DEV)
    got = r.HistogramValues(r.CloudValues("alpha", out=empty))
    assert got["selected"] == 0 and np.isposinf(got["vmin"])
    r.close()
