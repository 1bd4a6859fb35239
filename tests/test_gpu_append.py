"""GPU tests of msplat_append_cloud: the selected splats of a source context's cloud appended on the device to
a context's own.  The reference of every comparison is merged behaviour, never the code under test -- a context that was uploaded
the concatenated rows (tests/append_rule.py) in the same storage and with the same spatial_order, or the contexts before the call
-- and every comparison is same_bits: num_splats, the storage kind, the downloaded records, the storage order, the cull boxes after
a Sort and the frame's sort_count, keys, indices, pixels, drawn and pair counts.  Because a second SH_Q8 round may move a value, the
reference rows are the destination's ORIGINAL rows followed by the source's original rows where the two storage kinds match and
by its downloaded rows where they differ.  Views are 256 x 160; the clouds have at most 8194 splats but for the one that crosses
2^18.  tests/test_append.py checks the rule on the CPU.  No test hands a host address to msplat_append_cloud: its pointer guards
(check_device_source, before anything is launched) are checked by reading."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from splatapult_amd.points import PointRenderer
from tests import append_rule as ar
from tests import compact_harness as ch
from tests import sh_q8_rule as sq
from tests import transform_harness as th
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import make_renderer, sorted_frame
from tests.render_cases import random_points

pytestmark = pytest.mark.gpu

VIEW = vr.view()
OFF, ON, AUTO = _capi.SPATIAL_OFF, _capi.SPATIAL_ON, _capi.SPATIAL_AUTO
ORDER = {False: OFF, True: ON}
# (cloud_storage, full SH): the three storages of a full-SH cloud, and the two of an SH-degree-0 cloud (25-float rows)
STORES = {"fp32": ("fp32", True), "sh_fp16": ("sh_fp16", True), "sh_q8": ("sh_q8", True), "degree0": ("fp32", False),
          "degree0_fp16": ("sh_fp16", False)}
FULL, DEGREE0 = ("fp32", "sh_fp16", "sh_q8"), ("degree0", "degree0_fp16")
PAIRS = [(d, s) for group in (FULL, DEGREE0) for d in group for s in group]          # 9 + 4: (destination, source)


def cloud(n, full_sh=True):
    aos = vr.cloud_aos(n, vr.TIE_FREE[1]) if n == vr.TIE_FREE[0] else vr.cloud_aos(n)
    return aos if full_sh else np.ascontiguousarray(aos[:, :25])


def stored(rows, storage):
    """what a store of that kind returns for uploaded rows: the decode of its encode"""
    if storage == "sh_q8":
        return sq.deq(rows)
    out = rows.copy()
    if storage == "sh_fp16":
        rest = [c for c in sq.REST if c < rows.shape[1]]
        with np.errstate(over="ignore"):
            out[:, rest] = rows[:, rest].astype(np.float16).astype(np.float32)
    return out


def raw_append(r, s, d_select=None, n=None, d_map=None, k=None):
    """msplat_append_cloud on the renderers' contexts, the return code"""
    return _capi.lib().msplat_append_cloud(r._ctx, s._ctx if s is not None else None, d_select, s._n if n is None else n, d_map,
                                           C.byref(k) if k is not None else None)


def append(r, s, select):
    """AppendCloud(index_map=True) with the map as numpy uint32 (MSPLAT_ID_NONE where a splat was not selected)"""
    k, m = r.AppendCloud(s, select, index_map=True)
    return k, m.cpu().numpy().view(np.uint32)


def reference_rows(own_aos, src_aos, src_download, same_kind, select):
    return ar.merged_rows(own_aos, src_aos if same_kind else src_download, select)


def appended_equals_the_upload(own_aos, src_aos, select, dst, src, own_order, src_order, what, make=make_renderer):
    """a context uploaded own_aos that was appended the selection of a context uploaded src_aos, against a context uploaded the
    merged rows; the source afterwards against itself before"""
    (dstorage, full_sh), (sstorage, _) = STORES[dst], STORES[src]
    n, ns = own_aos.shape[0], src_aos.shape[0]
    s = make(src_aos, cloud_storage=sstorage, spatial_order=src_order)
    src_before = ch.context_state(s, VIEW, full_sh)
    r = make(own_aos, cloud_storage=dstorage, spatial_order=own_order)
    before = r.download_cloud(full_sh)
    storage = r.cloud_storage()
    k, m = append(r, s, select)
    want_map, want_k = ar.index_map(select, ns, n)
    assert k == want_k, "%s: K %d, the rule's %d" % (what, k, want_k)
    same_bits(m, want_map, "%s: the index map" % what)
    with pytest.raises(_capi.MsplatError) as e:                  # has_sort is cleared: Sort first
        r.Render(*VIEW)
    assert e.value.code == _capi.ERR_NO_SORT, what
    got = ch.context_state(r, VIEW, full_sh)
    assert r.cloud_storage() == storage and got["n"] == n + k, what
    same_kind = s.cloud_storage() == storage
    rows = reference_rows(own_aos, src_aos, src_before["cloud"], same_kind, select)
    ch.assert_same_context(got, th.uploaded_state(rows, VIEW, cloud_storage=dstorage, spatial_order=own_order), what)
    # per row: the old rows as they were, the new ones the source's download, encoded in the destination's kind where it differs
    sel = ar.picked(select, ns)
    same_bits(got["cloud"][:n], before, "%s: the destination's own rows" % what)
    new = src_before["cloud"][sel]
    same_bits(got["cloud"][n:], new if same_kind else stored(new, dstorage), "%s: the appended rows" % what)
    th.assert_same_context_again(ch.context_state(s, VIEW, full_sh), src_before, "%s: the source afterwards" % what)
    r.close(), s.close()


# ---- 1. the merged context equals the upload of the concatenation; 2. per row ---------------------------------------------------
@pytest.mark.parametrize("d", range(len(vr.SIZES)), ids=["n%d" % n for n in vr.SIZES])
@pytest.mark.parametrize("dst,src", PAIRS, ids=["%s<-%s" % p for p in PAIRS])
def test_an_appended_context_equals_the_upload_of_the_merged_rows(dst, src, d):
    n, full_sh = vr.SIZES[d], STORES[dst][1]
    for ns, name, own_on, src_on in ar.plan(d):
        appended_equals_the_upload(cloud(n, full_sh), ar.source_aos(ns, full_sh), ar.select_cases(ns)[name], dst, src, ORDER[own_on],
                                   ORDER[src_on], "n %d, %s <- %d of %s, %s, orders %d %d" % (n, dst, ns, src, name, own_on, src_on))


@pytest.mark.parametrize("src_order", [OFF, ON], ids=["src_upload_order", "src_morton_order"])
@pytest.mark.parametrize("own_order", [OFF, ON], ids=["upload_order", "morton_order"])
def test_both_storage_orders_on_either_side_at_4097_splats(own_order, src_order):
    n = ns = 4097
    select = ar.select_cases(ns)["random_30"]
    for dst, src in (("sh_q8", "sh_q8"), ("sh_q8", "fp32"), ("fp32", "sh_fp16"), ("degree0_fp16", "degree0")):
        full_sh = STORES[dst][1]
        appended_equals_the_upload(cloud(n, full_sh), ar.source_aos(ns, full_sh), select, dst, src, own_order, src_order,
                                   "%s <- %s, orders %d %d" % (dst, src, own_order, src_order))


# ---- 3. src == ctx ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
@pytest.mark.parametrize("store", ["fp32", "sh_fp16", "sh_q8", "degree0"])
def test_a_context_appended_to_itself_duplicates_the_selection(store, spatial):
    storage, full_sh = STORES[store]
    n = 1000
    aos, select = cloud(n, full_sh), vr.random_mask(n, seed=5, share=0.5)
    r = make_renderer(aos, cloud_storage=storage, spatial_order=spatial)
    before = r.download_cloud(full_sh)
    k, m = append(r, r, select)
    assert k == int(select.sum())
    same_bits(m, ar.index_map(select, n, n)[0], "the index map")
    got = ch.context_state(r, VIEW, full_sh)
    assert got["n"] == n + k
    same_bits(got["cloud"][:n], before, "%s: the originals" % store)
    same_bits(got["cloud"][n:], before[select], "%s: the duplicates" % store)
    ref = th.uploaded_state(ar.merged_rows(aos, aos, select), VIEW, cloud_storage=storage, spatial_order=spatial)
    ch.assert_same_context(got, ref, "%s: the doubled rows" % store)
    k, _ = r.AppendCloud(r)                                      # ... and once more, every splat
    assert k == n + int(select.sum()) and r.stats()["num_splats"] == 2 * k
    r.close()


# ---- 4. empty cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst,src", [("fp32", "fp32"), ("sh_q8", "sh_q8"), ("sh_q8", "fp32"), ("fp32", "sh_q8"), ("degree0", "degree0_fp16")])
def test_an_empty_destination_extracts_the_selection_into_a_cloud_of_its_own(dst, src):
    full_sh = STORES[dst][1]
    ns = 4097
    src_aos, select = ar.source_aos(ns, full_sh), ar.select_cases(ns)["random_30"]
    for order in (OFF, ON):
        appended_equals_the_upload(np.zeros((0, src_aos.shape[1]), np.float32), src_aos, select, dst, src, order, ON,
                                   "an empty %s destination <- %s, order %d" % (dst, src, order))


@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
def test_appending_nothing_leaves_records_order_and_boxes_as_they_were(spatial):
    n = 4097
    aos = cloud(n)
    empty = make_renderer(np.zeros((0, 61), np.float32), spatial_order=spatial)            # Ns = 0
    other = make_renderer(ar.source_aos(257), cloud_storage="sh_fp16", spatial_order=spatial)
    for storage in ("fp32", "sh_q8"):
        r = make_renderer(aos, cloud_storage=storage, spatial_order=spatial)
        before = ch.context_state(r, VIEW, True)
        for s, select in ((other, np.zeros(257, bool)), (empty, None), (empty, np.zeros(0, bool))):
            k, m = append(r, s, select)
            assert k == 0 and m.shape == (s._n,) and (m == ar.ID_NONE).all()
            with pytest.raises(_capi.MsplatError) as e:          # the same postconditions as any other K: Sort first
                r.Render(*VIEW)
            assert e.value.code == _capi.ERR_NO_SORT
            th.assert_same_context_again(ch.context_state(r, VIEW, True), before, "%s, K = 0" % storage)
        r.close()
    k, _ = empty.AppendCloud(empty)                              # nothing appended to nothing
    assert k == 0 and empty.stats()["num_splats"] == 0
    ch.assert_same_context(ch.context_state(empty, VIEW, True), ch.subset_state(aos, np.zeros(0, np.int64), VIEW, spatial_order=spatial),
                           "empty <- empty")
    empty.close(), other.close()


# ---- 5. mask and crop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["fp32", "sh_fp16"])
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
def test_the_mask_is_kept_and_every_appended_splat_is_visible(spatial, src):
    n, ns = vr.TIE_FREE[0], 1000
    aos, src_aos = cloud(n), ar.source_aos(ns)
    mask, select = vr.random_mask(n, seed=8, share=0.5), vr.random_mask(ns, seed=6, share=0.4)
    s = make_renderer(src_aos, cloud_storage=src, spatial_order=spatial)
    r = make_renderer(aos, spatial_order=spatial)
    r.SetVisibility(mask)
    k, _ = r.AppendCloud(s, select)
    assert r.visibility()["has_mask"]
    got = ch.context_state(r, VIEW, True)
    merged = ar.merged_mask(mask, k)
    assert r.visibility() == dict(has_mask=True, crop=None, hidden=int((~merged).sum())), r.visibility()
    assert int((~merged).sum()) == int((~mask).sum())
    rows = reference_rows(aos, src_aos, s.download_cloud(True), src == "fp32", select)
    ch.assert_same_context(got, th.uploaded_state(rows, VIEW, mask=merged, spatial_order=spatial), "a mask set before the call")
    idx = got["frame"]["idx"]
    assert 0 < got["frame"]["V"] < n + k and merged[idx].all() and (idx >= n).any()
    r.close(), s.close()


def test_a_crop_set_before_the_call_hides_by_the_merged_centres():
    aos, src_aos = vr.crop_cloud(), ar.source_aos(1000)
    n, crop = aos.shape[0], (vr.matrices()["scaled"], "box", False)
    s = make_renderer(src_aos, spatial_order=ON)
    r = make_renderer(aos, spatial_order=OFF)
    r.SetCrop(*crop)
    old_hidden = int((~vr.crop(aos[:, 0:3], crop[0], "box")).sum())
    r.Sort(*VIEW)
    assert r.visibility()["hidden"] == old_hidden
    k, _ = r.AppendCloud(s)
    rows = ar.merged_rows(aos, src_aos, None)
    hidden = int((~vr.crop(rows[:, 0:3], crop[0], "box")).sum())
    assert k == 1000 and old_hidden < hidden < n + k
    got = ch.context_state(r, VIEW, True)
    assert r.visibility() == dict(has_mask=False, crop=("box", False), hidden=hidden), r.visibility()
    ch.assert_same_context(got, th.uploaded_state(rows, VIEW, crop=crop, spatial_order=OFF), "a crop set before the call")
    r.close(), s.close()


# ---- 6. frames in flight and an attached context --------------------------------------------------------------------------------
def test_four_frames_in_flight_all_render_the_merged_cloud_under_the_mask():
    n, ns = 4097, 1000
    aos, src_aos, mask = cloud(n), ar.source_aos(ns), vr.random_mask(4097, seed=8, share=0.5)
    select = vr.random_mask(ns, seed=6, share=0.4)
    ref = make_renderer(ar.merged_rows(aos, src_aos, select), spatial_order=OFF)
    ref.SetVisibility(ar.merged_mask(mask, int(select.sum())))
    want = sorted_frame(ref, VIEW)
    ref.close()
    s = make_renderer(src_aos, spatial_order=ON, frames_in_flight=2)
    fly = make_renderer(aos, spatial_order=OFF, frames_in_flight=4)
    fly.SetVisibility(mask)
    for _ in range(2):                                           # two frames are in flight on either side when the call comes
        fly.Sort(*VIEW)
        s.Sort(*VIEW)
    k, _ = fly.AppendCloud(s, select)
    assert k == int(select.sum())
    seen = set()
    for f in range(4):
        ch.assert_same_frame(sorted_frame(fly, VIEW), want, "frame %d after the call" % f)
        assert fly.visibility()["has_mask"], f
        seen.add(fly._ctx.value)
    assert len(seen) == 4                                        # one frame per context
    fly.close(), s.close()


def test_an_attached_context_renders_the_old_cloud_until_it_is_attached_again_and_may_be_the_source():
    L = _capi.lib()
    n, ns = 4097, 257
    aos, src_aos = cloud(n), ar.source_aos(ns)
    a = make_renderer(aos, spatial_order=ON)                     # the owner
    b = SplatRenderer(device=0, spatial_order=ON)
    assert b._create(False), b.last_error()
    assert L.msplat_attach_cloud(b._ctx, a._ctx) == _capi.OK, b.last_error()
    b._n = n
    s = make_renderer(src_aos, spatial_order=OFF)
    whole = ch.context_state(a, VIEW, True)
    a.AppendCloud(s)
    merged = th.uploaded_state(ar.merged_rows(aos, src_aos, None), VIEW, spatial_order=ON)
    th.assert_same_context_again(ch.context_state(a, VIEW, True), merged, "the owner")
    th.assert_same_context_again(ch.context_state(b, VIEW, True), whole, "the attached context of a store its owner appended to")
    # the attached context, which still holds the old cloud, as the source
    k, _ = s.AppendCloud(b)
    assert k == n
    th.assert_same_context_again(ch.context_state(s, VIEW, True),
                                 th.uploaded_state(ar.merged_rows(src_aos, aos, None), VIEW, spatial_order=OFF), "an attached source")
    th.assert_same_context_again(ch.context_state(b, VIEW, True), whole, "the attached source afterwards")
    assert L.msplat_attach_cloud(b._ctx, a._ctx) == _capi.OK, b.last_error()
    b._n = n + ns
    th.assert_same_context_again(ch.context_state(b, VIEW, True), merged, "attached again")
    a.close(), b.close(), s.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    n, ns = 257, 65
    r = make_renderer(cloud(n), spatial_order=ON)
    r.SetVisibility(vr.mask_cases(n)["every_other"])
    s = make_renderer(ar.source_aos(ns), spatial_order=ON)
    low = make_renderer(ar.source_aos(ns, False), spatial_order=ON)         # another full_sh
    before, src_before, low_before = (ch.context_state(x, VIEW, f) for x, f in ((r, True), (s, True), (low, False)))
    k = C.c_uint64(99)
    assert raw_append(r, low, k=k) == _capi.ERR_UNSUPPORTED and "SH" in r.last_error()
    assert raw_append(low, r, k=k) == _capi.ERR_UNSUPPORTED
    same_bits(r.Render(*VIEW), before["frame"]["img"], "a Render after the refusal draws the latest Sort")
    assert raw_append(r, s, n=ns - 1, k=k) == _capi.ERR_INVALID_ARG
    assert raw_append(r, s, n=ns + 1, k=k) == _capi.ERR_INVALID_ARG
    assert raw_append(r, None, n=0, k=k) == _capi.ERR_INVALID_ARG
    assert _capi.lib().msplat_append_cloud(None, s._ctx, None, ns, None, C.byref(k)) == _capi.ERR_INVALID_ARG
    import torch
    t = torch.zeros(ns + 1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert raw_append(r, s, d_map=C.c_void_p(t.data_ptr() + 1), k=k) == _capi.ERR_INVALID_ARG and "aligned" in r.last_error()
    with pytest.raises(ValueError):
        r.AppendCloud(s, np.ones(ns - 1, bool))
    with pytest.raises(ValueError):
        r.AppendCloud(s, np.ones(ns, np.float32))
    # a point cloud on either side: refused, and it still renders
    p = PointRenderer(device=0)
    assert p.Init(random_points(500, 3)), p.last_error()
    want = p.Render(*VIEW)
    assert _capi.lib().msplat_append_cloud(p._ctx, s._ctx, None, ns, None, C.byref(k)) == _capi.ERR_UNSUPPORTED
    assert _capi.lib().msplat_append_cloud(r._ctx, p._ctx, None, 500, None, C.byref(k)) == _capi.ERR_UNSUPPORTED
    same_bits(p.Render(*VIEW), want, "the points after the refusal")
    p.close()
    # no cloud on either side
    c = SplatRenderer(device=0)
    assert c._create(False), c.last_error()
    assert _capi.lib().msplat_append_cloud(c._ctx, s._ctx, None, ns, None, C.byref(k)) == _capi.ERR_NO_CLOUD
    assert _capi.lib().msplat_append_cloud(r._ctx, c._ctx, None, 0, None, C.byref(k)) == _capi.ERR_NO_CLOUD
    c.close()
    assert k.value == 99 and not t.cpu().numpy().any()           # (nothing was written)
    assert r.visibility()["has_mask"]
    same_bits(r.Render(*VIEW), before["frame"]["img"], "a Render after the refusals")
    for x, st, f in ((r, before, True), (s, src_before, True), (low, low_before, False)):
        th.assert_same_context_again(ch.context_state(x, VIEW, f), st, "after the refusals")
    r.close(), s.close(), low.close()


# ---- 8. over-range conversion ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst,value,word", [("sh_fp16", 1e5, "fp16"), ("sh_q8", np.inf, "finite"), ("sh_q8", np.nan, "finite")])
def test_an_over_range_conversion_fails_and_changes_nothing(dst, value, word):
    n, ns = 300, 130
    src_aos = ar.source_aos(ns).copy()
    src_aos[70, sq.REST[7]] = value
    s = make_renderer(src_aos, spatial_order=ON)                 # an FP32 store holds any value
    r = make_renderer(cloud(n), cloud_storage=dst, spatial_order=ON)
    before = ch.context_state(r, VIEW, True)
    k = C.c_uint64(99)
    assert raw_append(r, s, k=k) == _capi.ERR_UNSUPPORTED and k.value == 99
    assert word in r.last_error() and "unchanged" in r.last_error()
    same_bits(r.Render(*VIEW), before["frame"]["img"], "a Render after the failure draws the latest Sort")
    same_bits(r.download_cloud(True), before["cloud"], "the download after the failure")
    th.assert_same_context_again(ch.context_state(r, VIEW, True), before, "after the failure")
    sel = np.ones(ns, bool)
    sel[70] = False
    k, _ = r.AppendCloud(s, sel)                                 # without that splat the call goes through
    assert k == ns - 1 and r.stats()["num_splats"] == n + ns - 1
    r.close(), s.close()


# ---- 9. small grids -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 5])
def test_a_small_grid_changes_nothing(cap, monkeypatch):
    n = ns = 4097                # 65 waves of 64 records, two scan chunks: 65 and 13 turns of the conversion's grid-stride loop
    make = lambda aos, **kw: ch.capped_renderer(aos, monkeypatch, cap, **kw)
    select = ar.select_cases(ns)["random_30"]
    for dst, src in (("fp32", "fp32"), ("sh_fp16", "fp32"), ("fp32", "sh_q8"), ("sh_q8", "sh_fp16")):
        appended_equals_the_upload(cloud(n), ar.source_aos(ns), select, dst, src, ON, ON, "MSPLAT_GRID_CAP=%d, %s <- %s" % (cap, dst, src),
                                   make=make)


# ---- 10. entering Morton storage under AUTO -----------------------------------------------------------------------------------
def test_a_cloud_that_reaches_2_to_the_18_enters_morton_storage_under_auto():
    from tests import scenes
    n, ns = (1 << 18) - 1, 2
    aos = np.ascontiguousarray(scenes.synth_cloud(n, 5, log_scale_mean=-4.5).as_array()[:n, :25], np.float32)
    src_aos = ar.source_aos(ns, False)
    s = make_renderer(src_aos, spatial_order=AUTO)
    r = make_renderer(aos, spatial_order=AUTO)
    assert r.storage_order() is None                             # one splat short of Morton storage
    k, _ = r.AppendCloud(s)
    assert k == ns
    got = ch.context_state(r, VIEW, False)
    assert got["n"] == n + ns > 1 << 18 and got["order"] is not None
    ch.assert_same_context(got, th.uploaded_state(ar.merged_rows(aos, src_aos, None), VIEW, spatial_order=AUTO), "N + K crosses 2^18")
    r.close(), s.close()
