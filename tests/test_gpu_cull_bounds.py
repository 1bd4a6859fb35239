"""The conservative culls at hostile geometry, on the device: cull_key's band test, box_live's band branch and the two-pass gate
(occ_box_kernel, occ_gate_kernel) drop work on the strength of a footprint bound, and a bound that is too small loses a splat
silently.  Every test compares a frame that culls with the frame of a context that does not -- unbanded, band cull off, one
pass -- for the hostile cloud and every camera of tests/cull_cases.py (tests/test_cull_bound.py checks the bound's arithmetic on
the host), and the band cull also against the oracle's own footprints: a splat whose true footprint reaches an owned bin row
must be in the rank's sorted list, which shows a drop even where a saturated pixel would hide it.

Shapes: 4097 splats (17 cull boxes, the last with one splat), 352 x 300 pixels (11 x 10 bins, the top row 12 px high), fp32."""
import functools

import numpy as np
import pytest

from splatapult_amd import _capi
from tests import cull_cases as cc
from tests import scenes
from tests.checks import check_image
from tests.gpu_harness import bin_px, make_renderer, oracle_frame
from tests.render_cases import oracle_rects

pytestmark = pytest.mark.gpu

N, W, H = cc.N, cc.W, cc.H
ROWS = (H + 31) // 32
SHARES = (1.0 / 64.0, 0.3)

@functools.lru_cache(maxsize=None)
def hostile_cloud():
    return scenes.cloud_from_attrs(cc.hostile_attrs(N, cc.SEEDS[0]))


@functools.lru_cache(maxsize=None)
def walled_cloud():
    return scenes.cloud_from_attrs(cc.join_attrs(cc.wall_attrs(), cc.hostile_attrs(N, cc.SEEDS[0])))


@functools.lru_cache(maxsize=None)
def reference(name):
    """the hostile cloud seen by camera `name` through a context that culls nothing but what the reference culls -- upload
    order, unbanded, one pass: frame, keys, indices (read-only), and the oracle's frame with the bin rectangle of every splat
    whose true footprint reaches a pixel"""
    assert bin_px() == 32
    cloud = hostile_cloud()
    view = cam, proj, vp, nf = cc.CAMERAS[name](W, H)
    r = make_renderer(cloud, spatial_order=_capi.SPATIAL_OFF, two_pass=_capi.TWO_PASS_OFF)
    r.Sort(*view)
    full = r.Render(*view)
    keys, idx = r.sorted_keys(), r.sorted_indices()
    ref = oracle_frame(cloud.as_array(), True, cam, proj, vp, nf, r=r)
    r.close()
    drawn, _, ty0, _, ty1 = oracle_rects(ref["splats"], W, H, 32)
    key_of = np.zeros(N, np.uint32)
    key_of[idx] = keys
    rank_of = np.full(N, -1, np.int64)
    rank_of[idx] = np.arange(idx.shape[0])
    out = dict(view=view, full=full, keys=keys, idx=idx, key_of=key_of, rank_of=rank_of, oracle=ref, drawn=drawn, ty0=ty0, ty1=ty1)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def owned(lay):
    """(the bin rows a layout owns, the mask of the pixel rows in them)"""
    mine = np.array(_capi.band_rows(*lay, rows_full=ROWS), np.int64)
    return mine, np.isin(np.arange(H) // 32, mine)


def assert_sorted_like_the_reference(r, R, what):
    """the context's visible splats carry the reference's keys and come in the reference's order"""
    idx, keys = r.sorted_indices(), r.sorted_keys()
    assert (R["rank_of"][idx] >= 0).all(), "%s: %d splat(s) the reference's cull drops" % (what, (R["rank_of"][idx] < 0).sum())
    np.testing.assert_array_equal(keys, R["key_of"][idx], err_msg="%s: keys" % what)
    assert (np.diff(R["rank_of"][idx]) > 0).all(), "%s: not in the reference's draw order" % what
    return idx


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_the_reference_frame_is_the_oracles(name):
    """what the culled frames are compared with is itself right: visible set, order and pixels of the oracle -- for the cameras
    that are no rotation too (the projection takes mat3(view) as it is).  Under "squashed" one visible splat (upload index 70) has a
    projected covariance whose minor-axis variance is negative in fp32 although det > 0: class Q of the footprint rule
    (include/msplat.h), which the reference, the oracle and the projection all draw nothing for"""
    R = reference(name)
    ref = R["oracle"]
    assert R["idx"].shape[0] == ref["V"], (R["idx"].shape[0], ref["V"])
    np.testing.assert_array_equal(R["idx"], ref["sorted_idx"])
    print("reference %-17s V = %d of %d, %d splat(s) whose footprint reaches a pixel" % (name, ref["V"], N, R["drawn"].sum()))
    assert ref["V"] >= 256 and R["drawn"].sum() >= 128, (ref["V"], R["drawn"].sum())
    check_image(R["full"], ref["image"], budget=ref["budget"])


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_band_cull_per_splat_keeps_every_splat_that_reaches_an_owned_row(name):
    """spatial_order OFF: pass 0 runs cull_key<BAND> on every splat"""
    R = reference(name)
    view, full, ref = R["view"], R["full"], R["oracle"]
    V = R["idx"].shape[0]
    rb = make_renderer(hostile_cloud(), spatial_order=_capi.SPATIAL_OFF, two_pass=_capi.TWO_PASS_OFF)
    for kind, k, G in cc.LAYOUTS:
        acc, covered, ratios = np.zeros_like(full), np.zeros(H, bool), []
        for g in range(G):
            what = "%s, %s x %d rank %d" % (name, kind, G, g)
            lay = rb.set_band_plan(kind, ROWS, G, g, block_rows=k, band_cull=True)
            mine, rows = owned(lay)
            rb.Sort(*view)
            idx = assert_sorted_like_the_reference(rb, R, what)
            ratios.append(idx.shape[0] / V)
            # the oracle's footprint of splat s spans the bin rows ty0 .. ty1: it must be kept if one of them is owned
            reach = R["drawn"] & ((R["ty0"][:, None] <= mine[None, :]) & (mine[None, :] <= R["ty1"][:, None])).any(axis=1)
            lost = np.setdiff1d(ref["sorted_idx"][reach], idx)
            assert lost.size == 0, "%s: the band cull dropped %d splat(s) whose footprint reaches an owned row, e.g. upload index %s" % (
                what, lost.size, lost[:8])
            part = rb.Render(*view)
            assert (part[~rows] == 0).all() and not (covered & rows).any(), what
            covered |= rows
            acc[rows] = part[rows]
        assert covered.all()
        print("band cull per splat, %-17s %-11s x %d: V / V_unbanded per rank %s" % (name, kind, G, " ".join("%.2f" % x for x in ratios)))
        np.testing.assert_array_equal(acc, full, err_msg="%s, %s x %d" % (name, kind, G))
        if name == "rigid_pitched" and (kind, G) == ("contiguous", 8):
            assert min(ratios) < 0.7, "the band cull drops nothing worth the name: %s" % ratios
    rb.close()


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_band_cull_at_box_level_keeps_what_the_per_splat_test_keeps(name):
    """spatial_order ON: the second Sort of a rank that sees less than 70 % of the cloud walks the boxes box_live lists.  Splats
    with equal depth keys are drawn in ascending storage slot (the hostile cloud has them: positions clipped to one plane, seen
    along its normal), so the frame the ranks reassemble is the unbanded frame of the same storage order; visible set and keys
    are those of the per-splat test in upload order"""
    view = reference(name)["view"]
    r = make_renderer(hostile_cloud(), spatial_order=_capi.SPATIAL_ON, two_pass=_capi.TWO_PASS_OFF)
    off = make_renderer(hostile_cloud(), spatial_order=_capi.SPATIAL_OFF, two_pass=_capi.TWO_PASS_OFF)
    assert r.storage_order() is not None and off.storage_order() is None
    r.Sort(*view)
    full = r.Render(*view)
    np.testing.assert_array_equal(r.sorted_keys(), reference(name)["keys"])
    for kind, k, G in cc.LAYOUTS:
        acc, lives = np.zeros_like(full), []
        for g in range(G):
            what = "%s, %s x %d rank %d" % (name, kind, G, g)
            lay = r.set_band_plan(kind, ROWS, G, g, block_rows=k, band_cull=True)
            off.set_band_plan(kind, ROWS, G, g, block_rows=k, band_cull=True)
            _, rows = owned(lay)
            off.Sort(*view)
            V = off.sort_count()
            for f in range(2):
                r.Sort(*view)
                assert r.sort_count() == V, "%s, Sort %d: V %d, per-splat test %d" % (what, f, r.sort_count(), V)
                np.testing.assert_array_equal(r.sorted_keys(), off.sorted_keys(), err_msg="%s, Sort %d: keys" % (what, f))
                assert np.array_equal(np.sort(r.sorted_indices()), np.sort(off.sorted_indices())), "%s, Sort %d: another visible set" % (what, f)
                part = r.Render(*view)
            live, total, listed = r.cull_boxes()
            assert total == (N + 255) // 256 == 17, total
            if 0 < V < 0.7 * N:
                assert listed, "%s: V = %d of %d and the second Sort did not walk the listed boxes" % (what, V, N)
            lives.append((live, int(listed)))
            acc[rows] = part[rows]
        print("band cull at box level, %-17s %-11s x %d: (live boxes of 17, listed) per rank %s" % (name, kind, G, lives))
        np.testing.assert_array_equal(acc, full, err_msg="%s, %s x %d" % (name, kind, G))
    r.close()
    off.close()


@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_two_pass_gate_drops_only_what_cannot_be_seen(name):
    """a wall in front of the hostile cloud: pass 1 finishes the bins over it, the gate (per box with spatial_order ON, per splat
    always) drops the splats behind the cut that reach finished bins only -- pixels and depth plane of the single pass, bit for
    bit.  The cut between the passes falls on a multiple of 1024 ranks: at a share of 1/64 pass 1 holds fewer splats than the wall
    has and need not finish a bin, so the gate is asked to have dropped someone at 0.3"""
    view = cc.CAMERAS[name](W, H)
    for spatial in (_capi.SPATIAL_ON, _capi.SPATIAL_OFF):
        a = make_renderer(walled_cloud(), spatial_order=spatial, two_pass=_capi.TWO_PASS_OFF)
        b = make_renderer(walled_cloud(), spatial_order=spatial, two_pass=_capi.TWO_PASS_ON)
        for n_frames, share in enumerate(SHARES, 1):
            what = "%s, spatial_order %d, share %.3g" % (name, spatial, share)
            b.two_pass_state(share)
            a.Sort(*view); b.Sort(*view)
            assert a.sort_count() == b.sort_count()
            ia, za = a.Render(*view, depth=True)
            ib, zb = b.Render(*view, depth=True)
            np.testing.assert_array_equal(ib, ia, err_msg="%s: pixels" % what)
            np.testing.assert_array_equal(zb, za, err_msg="%s: depth plane" % what)
            info = b.two_pass_info()
            print("two-pass gate, %s: %s" % (what, info))
            assert b.two_pass_state(share)[0] == n_frames and a.two_pass_state()[0] == 0, what
            if name == "rigid_pitched":
                assert info is not None, what
                if share == SHARES[1]:
                    assert info["bins_unfinished"] < info["bins"], "%s: the wall finished no bin: %s" % (what, info)
                    assert info["splats_pass2"] < info["visible"] - info["splats_pass1"], "%s: the gate dropped nobody: %s" % (what, info)
        a.close()
        b.close()


@pytest.mark.parametrize("name", ["squashed", "wide"])
def test_all_culls_together_reassemble_the_plain_frame(name):
    """two passes + blocks of 2 rows x 4 ranks + band cull + spatial_order ON against one pass, unbanded (same storage order:
    equal depth keys are drawn in ascending storage slot).  The cut between the passes falls on a multiple of 1024 ranks, so a
    rank that sees about a thousand splats has someone behind it at the small share only"""
    view = cc.CAMERAS[name](W, H)
    plain = make_renderer(walled_cloud(), spatial_order=_capi.SPATIAL_ON, two_pass=_capi.TWO_PASS_OFF)
    plain.Sort(*view)
    full = plain.Render(*view)
    plain.close()
    r = make_renderer(walled_cloud(), spatial_order=_capi.SPATIAL_ON, two_pass=_capi.TWO_PASS_ON)
    for n_share, share in enumerate(SHARES, 1):
        r.two_pass_state(share)
        acc, seen = np.zeros_like(full), []
        for g in range(4):
            lay = r.set_band_plan("block", ROWS, 4, g, block_rows=2, band_cull=True)
            _, rows = owned(lay)
            for f in range(2):                                        # the second Sort may walk the listed boxes
                r.Sort(*view)
                part = r.Render(*view)
            info = r.two_pass_info() or {}
            seen.append((r.sort_count(), int(r.cull_boxes()[2]), info.get("splats_pass1"), info.get("splats_pass2"), info.get("bins_unfinished")))
            assert (part[~rows] == 0).all(), (name, share, g)
            acc[rows] = part[rows]
        print("all culls together, %s, share %.3g: (V, listed, splats in pass 1, in pass 2, bins unfinished) per rank %s" % (name, share, seen))
        assert r.two_pass_state(share)[0] == 8 * n_share
        np.testing.assert_array_equal(acc, full, err_msg="%s, share %.3g" % (name, share))
    r.close()
