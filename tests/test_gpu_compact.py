"""GPU tests of msplat_compact_cloud: the context's cloud reduced on the device to the splats its mask and
crop let through.  The reference of every comparison is merged behaviour, never the code under test -- a context that was uploaded
aos[keep] in the same storage and with the same spatial_order, or the masked context before the compaction -- and every comparison
is same_bits: K, num_splats, the storage kind, the downloaded records, the storage order, the cull boxes after a Sort and the
frame's sort_count, keys, indices, pixels, drawn and pair counts.  The index map is tests/compact_rule.py's.  Views are 256 x 160;
the clouds have at most 8193 splats but for the MSPLAT_GRID_CAP case (163 917) and the one that leaves Morton storage (2^18 + 256,
SH degree 0).  tests/test_compact.py checks the fixtures on the CPU.  No test hands a host address to msplat_compact_cloud: its
pointer guard (check_device_source, before anything is launched) is checked by reading."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from splatapult_amd.points import PointRenderer
from splatapult_amd.renderer import _aos_upload
from tests import compact_harness as ch
from tests import compact_rule as cr
from tests import sort_limit_cases as slc
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import make_renderer, sorted_frame
from tests.render_cases import random_points

pytestmark = pytest.mark.gpu

VIEW = vr.view()
OFF, ON, AUTO = _capi.SPATIAL_OFF, _capi.SPATIAL_ON, _capi.SPATIAL_AUTO
# (cloud_storage, full SH): the three storages of a full-SH cloud, and an SH-degree-0 cloud
STORES = {"fp32": ("fp32", True), "sh_fp16": ("sh_fp16", True), "sh_q8": ("sh_q8", True), "degree0": ("fp32", False)}


def cloud(n, full_sh=True):
    aos = vr.cloud_aos(n, vr.TIE_FREE[1]) if n == vr.TIE_FREE[0] else vr.cloud_aos(n)
    return aos if full_sh else np.ascontiguousarray(aos[:, :25])


# ---- 1. a compacted context equals the subset upload --------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("n", cr.SIZES)
def test_a_compacted_context_equals_the_subset_upload(n, store, spatial):
    storage, full_sh = STORES[store]
    aos = cloud(n, full_sh)
    for name, mask in cr.mask_cases(n).items():
        r, _ = ch.mask_then_compact(aos, mask, VIEW, "n %d, %s, %s" % (n, store, name), cloud_storage=storage, spatial_order=spatial)
        assert r.cloud_storage() == storage
        r.close()


# ---- 2. masked before, compacted after ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "sh_fp16", "sh_q8"])
def test_the_compacted_frame_is_the_masked_frame_renumbered(storage):
    n = vr.TIE_FREE[0]
    aos, mask = cloud(n), vr.random_mask(n, seed=8, share=0.5)
    r = make_renderer(aos, cloud_storage=storage, spatial_order=OFF)
    r.SetVisibility(mask)
    before = sorted_frame(r, VIEW)
    assert 0 < before["V"] < n
    k, m = ch.compact(r)
    ch.assert_map(m, k, mask, storage)
    after = sorted_frame(r, VIEW)
    assert after["V"] == before["V"]
    same_bits(after["keys"], before["keys"], "%s: keys" % storage)
    same_bits(after["img"], before["img"], "%s: the frame" % storage)
    same_bits(after["idx"], m[before["idx"]], "%s: indices = map[indices before]" % storage)
    assert (after["drawn"], after["pairs"]) == (before["drawn"], before["pairs"])
    r.close()


# ---- 3. crops -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,shape,invert", vr.CROPS, ids=["%s-%s%s" % (m, s, "-inverted" if i else "") for m, s, i in vr.CROPS])
def test_a_crop_is_compacted_by_the_rule_of_the_header(matrix, shape, invert):
    aos = vr.crop_cloud()
    n, xyz, M = aos.shape[0], aos[:, 0:3], vr.matrices()[matrix]
    what = "%s %s%s" % (matrix, shape, " inverted" if invert else "")
    keep = vr.crop(xyz, M, shape, invert)
    r = make_renderer(aos, spatial_order=OFF)
    r.SetCrop(M, shape, invert)
    before = sorted_frame(r, VIEW)
    k, m = ch.compact(r)
    ch.assert_map(m, k, keep, what)
    assert 0 < k < n
    if matrix != "rotated":                                      # the centres ON the surface are inside, their float neighbours not
        at = 0 if matrix == "identity" else 12
        on, out = m[at:at + 6] != cr.ID_NONE, m[at + 6:at + 12] != cr.ID_NONE
        assert (out.all() and not on.any()) if invert else (on.all() and not out.any()), (what, m[:24])
    got = ch.context_state(r, VIEW, True)
    # the crop stays and is evaluated on the new cloud: it hides nothing there
    assert r.visibility() == dict(has_mask=False, crop=(shape, invert), hidden=0), (what, r.visibility())
    same_bits(got["frame"]["keys"], before["keys"], "%s: keys" % what)
    same_bits(got["frame"]["img"], before["img"], "%s: the frame" % what)
    same_bits(got["frame"]["idx"], m[before["idx"]], "%s: indices" % what)
    r.SetCrop(None)
    ch.assert_same_context(ch.context_state(r, VIEW, True), ch.subset_state(aos, keep, VIEW, spatial_order=OFF), what)
    r.close()


@pytest.mark.parametrize("matrix,shape,invert", [("rotated", "box", False), ("scaled", "sphere", True)])
def test_mask_and_crop_together_keep_their_and(matrix, shape, invert):
    aos = vr.crop_cloud()
    n, M = aos.shape[0], vr.matrices()[matrix]
    keep = vr.random_mask(n, seed=9, share=0.6) & vr.crop(aos[:, 0:3], M, shape, invert)
    r = make_renderer(aos, spatial_order=ON)
    r.SetCrop(M, shape, invert)
    r.SetVisibility(vr.random_mask(n, seed=9, share=0.6))
    k, m = ch.compact(r)
    ch.assert_map(m, k, keep, "mask and %s %s" % (matrix, shape))
    r.SetCrop(None)
    ch.assert_same_context(ch.context_state(r, VIEW, True), ch.subset_state(aos, keep, VIEW, spatial_order=ON), "mask and crop")
    r.close()


def test_a_nan_centre_is_kept_by_a_mask_dropped_by_a_crop_and_kept_by_an_inverted_crop():
    n = 300
    aos = cloud(n).copy()
    aos[[7, 256], 0] = np.nan
    aos[100, 1] = np.inf
    odd = np.array([7, 100, 256])
    M = vr.matrices()["identity"]
    for shape in ("box", "sphere"):
        for invert in (False, True):
            keep = vr.crop(aos[:, 0:3], M, shape, invert)
            assert keep[odd].all() == invert and keep[odd].any() == invert
            r = make_renderer(aos, spatial_order=OFF)
            r.SetCrop(M, shape, invert)
            k, m = ch.compact(r)
            ch.assert_map(m, k, keep, "%s inverted %s" % (shape, invert))
            r.close()
    mask = np.arange(n) % 3 != 2                                 # keeps 7, 100 and 256
    assert mask[odd].all()
    r = make_renderer(aos, spatial_order=OFF)
    r.SetVisibility(mask)
    k, m = ch.compact(r)
    ch.assert_map(m, k, mask, "a mask alone")
    same_bits(r.download_cloud(True), aos[mask], "the NaN centres' records")
    r.close()


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------
def test_all_hidden_leaves_an_empty_cloud_and_init_works_afterwards():
    n = 257
    aos = cloud(n)
    r = make_renderer(aos, spatial_order=ON)
    want = sorted_frame(r, VIEW)
    r.SetVisibility(np.zeros(n, bool))
    k, m = ch.compact(r)
    assert k == 0 and (m == cr.ID_NONE).all() and r.stats()["num_splats"] == 0
    ch.assert_same_context(ch.context_state(r, VIEW, True), ch.subset_state(aos, np.zeros(0, np.int64), VIEW, spatial_order=ON), "K = 0")
    assert r.CompactCloud() == 0                                 # ... and the empty cloud compacts to itself
    assert r.Init(aos, False, False), r.last_error()
    ch.assert_same_frame(sorted_frame(r, VIEW), want, "Init after K = 0")
    r.close()


@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
def test_nothing_set_is_the_identity(spatial):
    n = 4097
    aos = cloud(n)
    r = make_renderer(aos, spatial_order=spatial)
    before = ch.context_state(r, VIEW, True)
    k, m = ch.compact(r)
    assert k == n
    same_bits(m, np.arange(n, dtype=np.uint32), "the identity map")
    with pytest.raises(_capi.MsplatError) as e:                  # has_sort is cleared: Sort first
        r.Render(*VIEW)
    assert e.value.code == _capi.ERR_NO_SORT
    ch.assert_same_context(ch.context_state(r, VIEW, True), before, "nothing set")
    r.close()


def test_compacting_twice_is_the_subset_of_the_subset():
    n = cr.CHUNK + 1
    aos = cloud(n)
    first = vr.random_mask(n, seed=11, share=0.7)
    r = make_renderer(aos, spatial_order=ON)
    r.SetVisibility(first)
    k1 = r.CompactCloud()                                        # (d_index_map NULL)
    assert k1 == int(first.sum()) and isinstance(k1, int)
    second = vr.random_mask(k1, seed=12, share=0.4)              # in the NEW numbering
    r.SetVisibility(second)
    k2, m = ch.compact(r)
    ch.assert_map(m, k2, second, "the second compaction")
    keep = np.flatnonzero(first)[second]
    ch.assert_same_context(ch.context_state(r, VIEW, True), ch.subset_state(aos, keep, VIEW, spatial_order=ON), "twice")
    r.close()


# ---- 5. the storage kind is the store's ---------------------------------------------------------------------------------------
def test_the_store_keeps_its_storage_and_the_next_upload_takes_the_configured_one():
    n = 1000
    aos, mask = cloud(n), vr.random_mask(n, seed=13)
    L = _capi.lib()
    r = make_renderer(aos, spatial_order=OFF)
    before = r.download_cloud(True)
    assert L.msplat_set_cloud_storage(r._ctx, _capi.STORAGE_SH_Q8) == _capi.OK
    r.SetVisibility(mask)
    assert r.CompactCloud() == int(mask.sum())
    assert r.cloud_storage() == "fp32"
    same_bits(r.download_cloud(True), before[mask], "an FP32 store with SH_Q8 pending")
    same_bits(r.download_cloud(True), aos[mask], "FP32 records are the source's")
    held, args = _aos_upload(aos)                                # (held: the memory args points into)
    assert L.msplat_upload_cloud(r._ctx, *args) == _capi.OK, r.last_error()
    r._n = n
    assert r.cloud_storage() == "sh_q8"
    r.close()


# ---- 6. leaving Morton storage under AUTO -------------------------------------------------------------------------------------
def test_a_cloud_leaves_morton_storage_when_k_falls_below_2_to_18():
    n = (1 << 18) + 256
    aos = np.ascontiguousarray(vr.cloud_aos(n)[:, :25])
    mask = vr.random_mask(n, share=0.5)
    assert mask.sum() < (1 << 18)
    r = make_renderer(aos, spatial_order=AUTO)
    assert r.storage_order() is not None
    before = r.download_cloud(False)
    r.SetVisibility(mask)
    k, m = ch.compact(r)
    ch.assert_map(m, k, mask, "2^18 + 256")
    assert r.storage_order() is None
    got = ch.context_state(r, VIEW, False)
    same_bits(got["cloud"], before[mask], "the download against the kept rows of the download before")
    ch.assert_same_context(got, ch.subset_state(aos, mask, VIEW, spatial_order=AUTO), "2^18 + 256")
    r.close()


# ---- 7. frames in flight ------------------------------------------------------------------------------------------------------
def test_four_frames_in_flight_all_render_the_compacted_cloud():
    n = 4097
    aos, mask = cloud(n), vr.random_mask(n, seed=8, share=0.5)
    s = make_renderer(np.ascontiguousarray(aos[mask]), spatial_order=OFF)
    want = sorted_frame(s, VIEW)
    s.close()
    fly = make_renderer(aos, spatial_order=OFF, frames_in_flight=4)
    fly.SetVisibility(mask)
    for _ in range(2):                                           # two frames are in flight when the compaction comes
        fly.Sort(*VIEW)
    k, m = ch.compact(fly)
    ch.assert_map(m, k, mask, "four frames in flight")
    seen = set()
    for f in range(4):
        ch.assert_same_frame(sorted_frame(fly, VIEW), want, "frame %d after the compaction" % f)
        assert fly.visibility() == dict(has_mask=False, crop=None, hidden=0), (f, fly.visibility())
        seen.add(fly._ctx.value)
    assert len(seen) == 4                                        # one frame per context
    fly.close()


@pytest.mark.parametrize("who", ["owner", "attached"])
def test_a_shared_store_is_not_modified(who):
    """two contexts on one store through the C ABI: the one that compacts gets a store of its own, the other renders the old cloud
    until it is attached again"""
    L = _capi.lib()
    n = 4097
    aos, mask = cloud(n), vr.random_mask(n, seed=15, share=0.5)
    a = make_renderer(aos, spatial_order=ON)                     # the owner
    b = SplatRenderer(device=0, spatial_order=ON)
    assert b._create(False), b.last_error()
    assert L.msplat_attach_cloud(b._ctx, a._ctx) == _capi.OK, b.last_error()
    b._n = n
    whole = ch.context_state(a, VIEW, True)
    ch.assert_same_context(ch.context_state(b, VIEW, True), whole, "attached, before")
    c, other = (a, b) if who == "owner" else (b, a)
    c.SetVisibility(mask)
    k, m = ch.compact(c)
    ch.assert_map(m, k, mask, who)
    ch.assert_same_context(ch.context_state(c, VIEW, True), ch.subset_state(aos, mask, VIEW, spatial_order=ON), "%s compacted" % who)
    ch.assert_same_context(ch.context_state(other, VIEW, True), whole, "the other context of a store the %s compacted" % who)
    assert L.msplat_attach_cloud(other._ctx, c._ctx) == _capi.OK, other.last_error()
    other._n = k
    ch.assert_same_context(ch.context_state(other, VIEW, True), ch.context_state(c, VIEW, True), "attached again")
    a.close(), b.close()


# ---- 8. MSPLAT_GRID_CAP -------------------------------------------------------------------------------------------------------
def test_grid_cap_changes_nothing(monkeypatch):
    n = slc.GRID_CAP_N
    aos = np.ascontiguousarray(vr.cloud_aos(n)[:, :25])
    mask = vr.mask_cases(n)["random_30"]

    def run(cap):
        r = ch.capped_renderer(aos, monkeypatch, cap, spatial_order=ON)
        r.SetVisibility(mask)
        k, m = ch.compact(r)
        out = (k, m, r.download_cloud(False), r.storage_order())
        r.close()
        return out

    want = run(None)
    ch.assert_map(want[1], want[0], mask, "uncapped")
    same_bits(want[2], aos[cr.keep_of(mask)], "uncapped: FP32 records are the source's")
    for cap in (1, 5):
        got = run(cap)
        assert got[0] == want[0]
        for a, b, part in zip(got[1:], want[1:], ("the map", "the download", "the storage order")):
            same_bits(a, b, "MSPLAT_GRID_CAP=%d: %s" % (cap, part))


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    import torch
    L = _capi.lib()
    k = C.c_uint64(99)
    # a point cloud: refused, and it still renders
    p = PointRenderer(device=0)
    assert p.Init(random_points(500, 3)), p.last_error()
    want = p.Render(*VIEW)
    assert L.msplat_compact_cloud(p._ctx, None, C.byref(k)) == _capi.ERR_UNSUPPORTED and k.value == 99
    same_bits(p.Render(*VIEW), want, "the points after the refusal")
    p.close()
    # no cloud
    c = SplatRenderer(device=0)
    assert c._create(False), c.last_error()
    assert L.msplat_compact_cloud(c._ctx, None, C.byref(k)) == _capi.ERR_NO_CLOUD and k.value == 99
    c.close()
    # a device pointer off its 4-byte boundary: nothing changes, the mask included
    n = 257
    aos, mask = cloud(n), vr.mask_cases(n)["every_other"]
    r = make_renderer(aos, spatial_order=OFF)
    r.SetVisibility(mask)
    before = sorted_frame(r, VIEW)
    t = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert L.msplat_compact_cloud(r._ctx, C.c_void_p(t.data_ptr() + 1), C.byref(k)) == _capi.ERR_INVALID_ARG and k.value == 99
    assert "4-byte" in r.last_error()
    assert r.stats()["num_splats"] == n and r.visibility()["has_mask"]
    same_bits(r.Render(*VIEW), before["img"], "a Render after the refusal draws the latest Sort")
    ch.assert_same_frame(sorted_frame(r, VIEW), before, "after the refusal")
    assert (t == 0).all()
    r.close()


# ---- 10. ids and scores speak the new numbering -------------------------------------------------------------------------------
def test_ids_and_scores_are_in_the_new_numbering():
    n = vr.TIE_FREE[0]
    aos, mask = cloud(n), vr.random_mask(n, seed=14, share=0.5)
    r, _ = ch.mask_then_compact(aos, mask, VIEW, "ids and scores", spatial_order=ON)
    s = make_renderer(np.ascontiguousarray(aos[mask]), spatial_order=ON)
    out = []
    for x in (r, s):
        x.Sort(*VIEW)
        ids, z = x.RenderIds(*VIEW, depth=True)
        score, hits = x.RenderScores(*VIEW, pixels=True)
        out.append((ids, z, score.cpu().numpy(), hits.cpu().numpy()))
    assert out[0][2].shape == (int(mask.sum()),) and (out[0][0] != cr.ID_NONE).any()
    for a, b, part in zip(out[0], out[1], ("ids", "id depth", "scores", "hit counts")):
        same_bits(a, b, part)
    r.close(), s.close()
