"""GPU tests of msplat_transform_cloud: the selected splats of a context's cloud moved, rotated and scaled on
the device.  The reference of every comparison is merged behaviour, never the code under test -- a context that was uploaded the
rule's rows (tests/transform_rule.py, with the D msplat_sh_rotation returns) in the same storage and with the same spatial_order,
or the context before the call -- and every comparison is same_bits: num_splats, the storage kind, the downloaded records, the
storage order, the cull boxes after a Sort and the frame's sort_count, keys, indices, pixels, drawn and pair counts.  Views are
256 x 160; the clouds have at most 4097 splats.  tests/test_transform.py checks the rule and msplat_sh_rotation on the CPU.  No
test hands a host address to msplat_transform_cloud: its pointer guard (check_device_source, before anything is launched) is
checked by reading."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from splatapult_amd.points import PointRenderer
from tests import compact_harness as ch
from tests import sh_q8_rule as sq
from tests import transform_harness as th
from tests import transform_rule as tr
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import make_renderer, sorted_frame
from tests.render_cases import random_points

pytestmark = pytest.mark.gpu

VIEW = vr.view()
OFF, ON = _capi.SPATIAL_OFF, _capi.SPATIAL_ON
MATS = tr.matrices()
# (cloud_storage, full SH): the three storages of a full-SH cloud, and an SH-degree-0 cloud (25-float rows)
STORES = {"fp32": ("fp32", True), "sh_fp16": ("sh_fp16", True), "sh_q8": ("sh_q8", True), "degree0": ("fp32", False)}
_P = C.POINTER(C.c_float)


def cloud(n, full_sh=True):
    aos = vr.cloud_aos(n, vr.TIE_FREE[1]) if n == vr.TIE_FREE[0] else vr.cloud_aos(n)
    return aos if full_sh else np.ascontiguousarray(aos[:, :25])


def raw_transform(r, M, d_select=None, n=None, flags=0):
    """msplat_transform_cloud on the renderer's context, the return code"""
    m = np.ascontiguousarray(np.asarray(M, np.float32).reshape(16))
    return _capi.lib().msplat_transform_cloud(r._ctx, m.ctypes.data_as(_P), d_select, r._n if n is None else n, flags)


def transformed_equals_the_upload(aos, M, select, keep_sh, what, make=make_renderer, **kw):
    """a context uploaded `aos` and transformed, against a context uploaded the rule's rows of its download"""
    full_sh = aos.shape[1] == 61
    r = make(aos, **kw)
    before = r.download_cloud(full_sh)
    storage = r.cloud_storage()
    r.TransformCloud(M, select, keep_sh=keep_sh)
    with pytest.raises(_capi.MsplatError) as e:                  # has_sort is cleared: Sort first
        r.Render(*VIEW)
    assert e.value.code == _capi.ERR_NO_SORT, what
    got = ch.context_state(r, VIEW, full_sh)
    assert r.cloud_storage() == storage, what
    rows = th.rule_rows(before, M, select, keep_sh)
    ch.assert_same_context(got, th.uploaded_state(rows, VIEW, cloud_storage=storage, spatial_order=kw["spatial_order"]), what)
    if select is not None:
        same_bits(got["cloud"][np.asarray(select) == 0], before[np.asarray(select) == 0], "%s: the unselected rows" % what)
    r.close()


# ---- 1. the transformed context equals the upload of the rule's rows ----------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("n", vr.SIZES)
def test_a_transformed_context_equals_the_upload_of_the_rules_rows(n, store, spatial):
    storage, full_sh = STORES[store]
    aos = cloud(n, full_sh)
    # (sh_q8: a second Q8 round may move the untouched rows of a re-upload: every splat is selected)
    cases = {"none": None} if store == "sh_q8" else tr.select_cases(n)
    for name, select in cases.items():
        for m in ("rigid", "similarity"):
            transformed_equals_the_upload(aos, MATS[m], select, False, "n %d, %s, %s, %s" % (n, store, name, m), cloud_storage=storage,
                                          spatial_order=spatial)
    transformed_equals_the_upload(aos, MATS["affine"], cases.get("random_30"), True, "n %d, %s, affine with keep_sh" % (n, store),
                                  cloud_storage=storage, spatial_order=spatial)


def test_a_quarter_turn_is_exact_and_four_of_them_are_the_identity_on_the_centres():
    n = 257
    aos = cloud(n)
    turn = MATS["quarter_turn"].copy()
    turn[12:15] = 0.0
    r = make_renderer(aos, spatial_order=ON)
    for _ in range(4):
        r.TransformCloud(turn)
    got = r.download_cloud(True)
    # signed permutations and exact products: only the sign of a zero can differ (-0 + 0 = +0)
    np.testing.assert_array_equal(got, aos)
    r.close()


# ---- 2. per row, in every storage ---------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
@pytest.mark.parametrize("store", list(STORES))
def test_unselected_rows_keep_their_bits_and_selected_rows_are_the_stores_encoding_of_the_rule(store, spatial):
    storage, full_sh = STORES[store]
    n = 1000
    aos, select = cloud(n, full_sh), vr.random_mask(n, seed=5, share=0.5)
    r = make_renderer(aos, cloud_storage=storage, spatial_order=spatial)
    before = r.download_cloud(full_sh)
    for m, keep_sh in (("similarity", False), ("affine", True)):
        r.TransformCloud(MATS[m], select, keep_sh=keep_sh)
        got = r.download_cloud(full_sh)
        assert r.cloud_storage() == storage and r.stats()["num_splats"] == n
        same_bits(got[~select], before[~select], "%s, %s: the unselected rows" % (store, m))
        want = stored(th.rule_rows(before, MATS[m], select, keep_sh), storage)
        same_bits(got[select], want[select], "%s, %s: the selected rows" % (store, m))
        assert (got[select, 0:3] != before[select, 0:3]).any(axis=1).all()
        before = got
    r.close()


# ---- 3. mask and crop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
def test_the_mask_is_kept_and_hides_the_same_upload_indices(spatial):
    n = vr.TIE_FREE[0]
    aos, mask, select = cloud(n), vr.random_mask(n, seed=8, share=0.5), vr.random_mask(n, seed=6, share=0.4)
    r = make_renderer(aos, spatial_order=spatial)
    before = r.download_cloud(True)
    r.SetVisibility(mask)
    r.TransformCloud(MATS["rigid"], select)
    assert r.visibility()["has_mask"]
    got = ch.context_state(r, VIEW, True)
    assert r.visibility() == dict(has_mask=True, crop=None, hidden=int((~mask).sum())), r.visibility()
    rows = th.rule_rows(before, MATS["rigid"], select)
    ref = th.uploaded_state(rows, VIEW, mask=mask, spatial_order=spatial)
    ch.assert_same_context(got, ref, "a mask set before the call")
    assert 0 < got["frame"]["V"] < n and mask[got["frame"]["idx"]].all()
    r.close()


def test_a_crop_set_before_the_call_hides_by_the_new_centres():
    aos = vr.crop_cloud()
    n, M, crop = aos.shape[0], MATS["similarity"], (vr.matrices()["scaled"], "box", False)
    r = make_renderer(aos, spatial_order=OFF)
    r.SetCrop(*crop)
    old_hidden = int((~vr.crop(aos[:, 0:3], crop[0], "box")).sum())
    r.Sort(*VIEW)
    assert r.visibility()["hidden"] == old_hidden
    r.TransformCloud(M)
    rows = th.rule_rows(aos, M)
    hidden = int((~vr.crop(rows[:, 0:3], crop[0], "box")).sum())
    assert hidden != old_hidden and 0 < hidden < n
    got = ch.context_state(r, VIEW, True)
    assert r.visibility() == dict(has_mask=False, crop=("box", False), hidden=hidden), r.visibility()
    ch.assert_same_context(got, th.uploaded_state(rows, VIEW, crop=crop, spatial_order=OFF), "a crop set before the call")
    r.close()


def test_four_frames_in_flight_all_render_the_moved_cloud_under_the_mask():
    n = 4097
    aos, mask = cloud(n), vr.random_mask(n, seed=8, share=0.5)
    rows = th.rule_rows(aos, MATS["rigid"])
    s = make_renderer(rows, spatial_order=OFF)
    s.SetVisibility(mask)
    want = sorted_frame(s, VIEW)
    s.close()
    fly = make_renderer(aos, spatial_order=OFF, frames_in_flight=4)
    fly.SetVisibility(mask)
    for _ in range(2):                                           # two frames are in flight when the call comes
        fly.Sort(*VIEW)
    fly.TransformCloud(MATS["rigid"])
    seen = set()
    for f in range(4):
        ch.assert_same_frame(sorted_frame(fly, VIEW), want, "frame %d after the call" % f)
        assert fly.visibility()["has_mask"], f
        seen.add(fly._ctx.value)
    assert len(seen) == 4                                        # one frame per context
    fly.close()


# ---- 4. refusals and failures -------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    n = 257
    aos = cloud(n)
    r = make_renderer(aos, spatial_order=ON)
    r.SetVisibility(vr.mask_cases(n)["every_other"])
    before = ch.context_state(r, VIEW, True)
    assert raw_transform(r, MATS["affine"]) == _capi.ERR_UNSUPPORTED           # no similarity, no KEEP_SH
    assert "MSPLAT_TRANSFORM_KEEP_SH" in r.last_error()
    same_bits(r.Render(*VIEW), before["frame"]["img"], "a Render after the refusal draws the latest Sort")
    assert raw_transform(r, MATS["rigid"], n=n - 1) == _capi.ERR_INVALID_ARG
    assert raw_transform(r, MATS["rigid"], n=n + 1) == _capi.ERR_INVALID_ARG
    bad = MATS["rigid"].copy()
    bad[9] = np.nan
    assert raw_transform(r, bad) == _capi.ERR_INVALID_ARG
    assert raw_transform(r, bad, flags=tr.KEEP_SH) == _capi.ERR_INVALID_ARG
    assert raw_transform(r, MATS["rigid"], flags=2) == _capi.ERR_INVALID_ARG
    assert raw_transform(r, MATS["rigid"], flags=tr.KEEP_SH | 0x100) == _capi.ERR_INVALID_ARG
    assert _capi.lib().msplat_transform_cloud(r._ctx, None, None, n, 0) == _capi.ERR_INVALID_ARG
    with pytest.raises(_capi.MsplatError) as e:
        r.TransformCloud(MATS["affine"])
    assert e.value.code == _capi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        r.TransformCloud(MATS["rigid"], np.ones(n - 1, bool))
    with pytest.raises(ValueError):
        r.TransformCloud(MATS["rigid"], np.ones(n, np.float32))
    assert r.visibility()["has_mask"]
    same_bits(r.Render(*VIEW), before["frame"]["img"], "a Render after the refusals")
    th.assert_same_context_again(ch.context_state(r, VIEW, True), before, "after the refusals")
    r.close()
    # a point cloud: refused, and it still renders
    p = PointRenderer(device=0)
    assert p.Init(random_points(500, 3)), p.last_error()
    want = p.Render(*VIEW)
    m = np.ascontiguousarray(MATS["rigid"])
    assert _capi.lib().msplat_transform_cloud(p._ctx, m.ctypes.data_as(_P), None, 500, 0) == _capi.ERR_UNSUPPORTED
    same_bits(p.Render(*VIEW), want, "the points after the refusal")
    p.close()
    # no cloud
    c = SplatRenderer(device=0)
    assert c._create(False), c.last_error()
    assert _capi.lib().msplat_transform_cloud(c._ctx, m.ctypes.data_as(_P), None, 0, 0) == _capi.ERR_NO_CLOUD
    c.close()


def test_an_fp16_overflow_after_the_rotation_fails_and_changes_nothing():
    n = 300
    aos = cloud(n).copy()
    for c in range(3):
        aos[5, [tr.sh_col(c, k) for k in (1, 2, 3)]] = 60000.0
    M = tr.summing_rotation()
    rows = th.rule_rows(aos, M)
    assert np.abs(rows[5, [tr.sh_col(c, 2) for c in range(3)]]).min() > 65520.0      # 60000 sqrt 3
    assert np.abs(np.delete(rows, 5, axis=0)[:, sq.REST]).max() < 100.0
    r = make_renderer(aos, cloud_storage="sh_fp16", spatial_order=ON)
    before = ch.context_state(r, VIEW, True)
    assert raw_transform(r, M) == _capi.ERR_UNSUPPORTED
    assert "fp16" in r.last_error()
    same_bits(r.Render(*VIEW), before["frame"]["img"], "a Render after the failure draws the latest Sort")
    same_bits(r.download_cloud(True), before["cloud"], "the download after the failure")
    th.assert_same_context_again(ch.context_state(r, VIEW, True), before, "after the failure")
    sel = np.ones(n, bool)
    sel[5] = False
    r.TransformCloud(M, sel)                                     # without that splat the call goes through
    same_bits(r.download_cloud(True)[5], before["cloud"][5], "the unselected splat")
    r.close()


# ---- 5. an attached context ---------------------------------------------------------------------------------------------------
def test_an_attached_context_renders_the_old_cloud_until_it_is_attached_again():
    L = _capi.lib()
    n = 4097
    aos = cloud(n)
    a = make_renderer(aos, spatial_order=ON)                     # the owner
    b = SplatRenderer(device=0, spatial_order=ON)
    assert b._create(False), b.last_error()
    assert L.msplat_attach_cloud(b._ctx, a._ctx) == _capi.OK, b.last_error()
    b._n = n
    whole = ch.context_state(a, VIEW, True)
    a.TransformCloud(MATS["rigid"])
    moved = th.uploaded_state(th.rule_rows(aos, MATS["rigid"]), VIEW, spatial_order=ON)
    th.assert_same_context_again(ch.context_state(a, VIEW, True), moved, "the owner")
    th.assert_same_context_again(ch.context_state(b, VIEW, True), whole, "the attached context of a store its owner transformed")
    assert L.msplat_attach_cloud(b._ctx, a._ctx) == _capi.OK, b.last_error()
    th.assert_same_context_again(ch.context_state(b, VIEW, True), moved, "attached again")
    a.close(), b.close()


# ---- 6. a small grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 5])
def test_a_small_grid_changes_nothing(cap, monkeypatch):
    n = 4097                                                     # 65 waves of 64 records: 65 and 13 turns of the grid-stride loop
    make = lambda aos, **kw: ch.capped_renderer(aos, monkeypatch, cap, **kw)
    for store in ("fp32", "sh_fp16"):
        transformed_equals_the_upload(cloud(n), MATS["similarity"], vr.mask_cases(n)["random_30"], False,
                                      "MSPLAT_GRID_CAP=%d, %s" % (cap, store), make=make, cloud_storage=store, spatial_order=ON)
