"""GPU tests of the id frame (msplat_render_ids, msplat_mark_ids).  The planes are compared with the float64
definition of tests/ids_rule.py on the pixels that definition DECIDES (tests/test_ids.py holds the cases to at most 1 % undecided
pixels), and with the library's own other execution shapes bit for bit: windows against the crop of the whole plane, contexts that
differ in everything the plane must not depend on, masked and cropped contexts against contexts that were uploaded the visible
splats only, compact storages against an FP32 context of their download.  msplat_mark_ids is compared with numpy on the host, exactly.
Views are at most 517 x 293 with at most 20 k splats.  No test hands msplat_mark_ids a host address: its pointer guard
(check_device_source, before anything is launched) is checked by reading."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import _capi
from splatapult_amd._capi import MsplatError
from tests import ids_rule, scenes
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import SENTINEL, Pitched, make_renderer
from tests.render_cases import MARGIN, window_depth

pytestmark = pytest.mark.gpu

NONE = ids_rule.NONE
ID_FILL = 0xABCDEF01          # what an id plane holds where a frame must not write: no splat, not NONE


def case_renderer(name, **kw):
    aos, _, W, H, view = ids_rule.case(name)
    r = make_renderer(aos, **kw)
    r.Sort(*view)
    return r, W, H, view


def planes_of(r, view, window=None):
    ids, z = r.RenderIds(*view, window=window, depth=True)
    assert ids.dtype == np.uint32 and z.dtype == np.float32 and ids.shape == z.shape
    return ids, z


@pytest.fixture(scope="module")
def sparse_planes():
    """the whole-viewport planes of a default context on the sparse case, computed once, read-only"""
    r, W, H, view = case_renderer("sparse")
    ids, z = planes_of(r, view)
    r.close()
    ids.setflags(write=False)
    z.setflags(write=False)
    return ids, z


def assert_same_planes(got, want, what):
    same_bits(got[0], want[0], "%s: ids" % what)
    same_bits(got[1], want[1], "%s: id_depth" % what)


# ---- 1. against the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ids_rule.CASES)
def test_the_planes_match_the_definition_on_decided_pixels(name):
    ref = ids_rule.reference(name)
    r, W, H, view = case_renderer(name)
    assert r.sort_count() == ref["V"]
    ids, z = planes_of(r, view)
    assert ids.shape == (H, W)
    d = ref["decided"]
    wrong = d & (ids != ref["id"])
    print("%s: %d of %d decided pixels differ; %d undecided, %d of them differ from the reference"
          % (name, wrong.sum(), d.sum(), (~d).sum(), (~d & (ids != ref["id"])).sum()))
    assert not wrong.any(), "%d decided pixel(s) differ, first at %s" % (wrong.sum(), tuple(np.argwhere(wrong)[0]))
    r.set_target_mode("premultiplied")
    alpha = r.Render(*view)[..., 3]
    # an undecided pixel holds the reference's id, or one of the frame's splats whose bin rectangle covers the pixel (NONE only where
    # a fragment sits on the discard threshold)
    _, rect = r.debug_projected()
    order = r.sorted_indices()
    n = ids_rule.case(name)[0].shape[0]
    rank_of = np.full(n, -1, np.int64)
    rank_of[order] = np.arange(order.shape[0])
    T = _capi.lib().msplat_tile_size()
    for y, x in np.argwhere(~d & (ids != ref["id"])):
        if ids[y, x] == NONE:
            assert ref["near"][y, x], "pixel (%d, %d): NONE, the reference names %d and no fragment is near the threshold" % (x, y, ref["id"][y, x])
            continue
        assert ids[y, x] < n and rank_of[ids[y, x]] >= 0, "pixel (%d, %d) names %d, which is not in the Sort" % (x, y, ids[y, x])
        rc = int(rect[rank_of[ids[y, x]]])
        tx0, ty0, tx1, ty1 = rc & 255, (rc >> 8) & 255, (rc >> 16) & 255, rc >> 24
        assert tx0 <= x // T <= tx1 and ty0 <= y // T <= ty1, "pixel (%d, %d) names %d, whose bins do not cover it" % (x, y, ids[y, x])
    # NONE exactly where the premultiplied frame of the same context is empty
    differ = ((ids == NONE) != (alpha == 0.0)) & ~ref["near"]
    assert not differ.any(), "%d pixel(s): NONE and alpha == 0 disagree, first at %s" % (differ.sum(), tuple(np.argwhere(differ)[0]))
    assert (ids == NONE).any() and (ids != NONE).any()
    # the depth plane: the named splat's window depth, exactly 1.0 at NONE
    zw_of = np.full(n, np.nan)
    zw_of[ref["splats"]["index"]] = window_depth(ref["splats"])
    hit = ids != NONE
    assert (z[~hit] == 1.0).all()
    err = np.abs(z[hit].astype(np.float64) - zw_of[ids[hit]])
    print("%s: max |id_depth - z_w| = %.3g (bound %.3g)" % (name, err.max(), MARGIN))
    assert (err <= MARGIN).all(), err.max()
    r.close()


# ---- 2. windows ------------------------------------------------------------------------------------------------------------------
def test_a_window_is_the_crop_of_the_whole_plane(sparse_planes):
    r, W, H, view = case_renderer("sparse")
    whole = planes_of(r, view)
    assert_same_planes(whole, sparse_planes, "a second context")
    L, f = r._lib, r._args.load(*view)
    for window in ids_rule.windows(W, H):
        x0, y0, w, h = window
        want = (np.ascontiguousarray(ids_rule.crop(whole[0], window)), np.ascontiguousarray(ids_rule.crop(whole[1], window)))
        assert_same_planes(planes_of(r, view, window), want, "host, window %s" % (window,))
        # host output into pitched arrays (the C ABI): the padding keeps its bytes
        hi, hz = np.full((h, w + 3), ID_FILL, np.uint32), np.full((h, w + 5), SENTINEL, np.float32)
        win = (C.c_int32 * 4)(*window)
        assert L.msplat_render_ids(r._ctx, *f, win, hi.ctypes.data, 4 * (w + 3), hz.ctypes.data, 4 * (w + 5), 0) == _capi.OK, r.last_error()
        assert (hi[:, w:] == ID_FILL).all() and (hz[:, w:] == SENTINEL).all(), "host padding written, window %s" % (window,)
        assert_same_planes((np.ascontiguousarray(hi[:, :w]), np.ascontiguousarray(hz[:, :w])), want, "host pitched, window %s" % (window,))
        # device output, tight and pitched
        for pad, rows in ((0, 0), (7, 2)):
            di = Pitched(h, w, np.uint32, ID_FILL, pad=pad, rows=rows, plane=True)
            dz = Pitched(h, w, np.float32, SENTINEL, pad=pad + 4 if pad else 0, rows=rows, plane=True)
            assert r.RenderIds(*view, window=window, out_ptr=di.ptr, pitch_bytes=di.pitch if pad else 0, depth_ptr=dz.ptr,
                               depth_pitch_bytes=dz.pitch if pad else 0) is None
            r.synchronize()
            got = (di.read("ids, window %s" % (window,)), dz.read("id_depth, window %s" % (window,)))
            assert_same_planes(got, want, "device, pad %d, window %s" % (pad, window))
        # the ids alone (id_depth == NULL)
        same_bits(r.RenderIds(*view, window=window), want[0], "ids alone, window %s" % (window,))
    for x, y in ((0, 0), (31, 31), (32, 32), (W - 1, H - 1), (W // 2, H // 2), (200, 150)):
        i, zw = r.Pick(*view, x, y)
        assert (NONE if i is None else i) == whole[0][y, x] and np.float32(zw) == whole[1][y, x], (x, y, i, zw)
    hits = np.argwhere(whole[0] != NONE)
    y, x = hits[len(hits) // 2]
    assert r.Pick(*view, int(x), int(y)) == (int(whole[0][y, x]), float(whole[1][y, x]))
    r.close()


# ---- 3. what the planes do not depend on -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(t_epsilon=0.0), dict(compositor_waves=64), dict(frame_mode=_capi.FRAMES_SERIAL),
                                dict(frame_mode=_capi.FRAMES_IN_FLIGHT), dict(fb_format="fp16"), dict(fb_format="rgba8")],
                         ids=["t_epsilon_0", "64_waves", "serial", "in_flight", "fp16", "rgba8"])
def test_the_planes_do_not_depend_on_the_context(kw, sparse_planes):
    r, W, H, view = case_renderer("sparse", **kw)
    assert_same_planes(planes_of(r, view), sparse_planes, str(kw))
    for mode in ("premultiplied", "load"):                      # nor on the target mode: the frame has no colour target
        r.set_target_mode(mode)
        assert_same_planes(planes_of(r, view), sparse_planes, "%s, target mode %s" % (kw, mode))
    r.close()


def test_two_pass_contexts_run_the_id_frame_in_one_pass(sparse_planes):
    r, W, H, view = case_renderer("sparse", two_pass=_capi.TWO_PASS_ON)
    before = r.Render(*view)
    info = r.two_pass_info()
    assert info is not None, "two_pass = ON did not run the Render as two passes"
    assert_same_planes(planes_of(r, view), sparse_planes, "two_pass = ON")
    assert r.two_pass_info() == info, "the id frame changed msplat_get_two_pass_info"
    same_bits(r.Render(*view), before, "the Render after the id frame")
    r.close()


def test_an_async_submit_context_queues_the_device_frame(sparse_planes):
    r, W, H, view = case_renderer("sparse", async_submit=True)
    di, dz = Pitched(H, W, np.uint32, ID_FILL, pad=3, plane=True), Pitched(H, W, np.float32, SENTINEL, pad=1, plane=True)
    r.RenderIds(*view, out_ptr=di.ptr, pitch_bytes=di.pitch, depth_ptr=dz.ptr, depth_pitch_bytes=dz.pitch)
    r.synchronize()
    assert_same_planes((di.read("ids"), dz.read("id_depth")), sparse_planes, "async_submit, device output")
    assert_same_planes(planes_of(r, view), sparse_planes, "async_submit, host output")
    r.close()


def test_renders_around_an_id_frame_are_what_they_were():
    r, W, H, view = case_renderer("sparse", enable_timing=True)
    s, _, _, _ = case_renderer("sparse")
    want = s.Render(*view)                                       # a context that never runs an id frame
    s.close()
    same_bits(r.Render(*view), want, "the Render before")
    r.synchronize()
    assert r.timings()["frames_averaged"] == 1                   # that Render's set (msplat_get_timings restarts the average)
    planes_of(r, view)
    planes_of(r, view, (13, 27, 40, 9))
    r.synchronize()
    assert r.timings()["frames_averaged"] == 0, "an id frame recorded a timing set"
    same_bits(r.Render(*view), want, "the Render after")
    r.close()


# ---- 4. numbering ----------------------------------------------------------------------------------------------------------------
def tie_free():
    return vr.cloud_aos(*vr.TIE_FREE), vr.view()


def sorted_planes(aos, view, **kw):
    r = make_renderer(np.ascontiguousarray(aos), **kw)
    r.Sort(*view)
    got = planes_of(r, view)
    r.close()
    return got


def test_morton_and_upload_order_give_the_same_plane():
    aos, view = tie_free()
    off = sorted_planes(aos, view, spatial_order=_capi.SPATIAL_OFF)
    r = make_renderer(aos, spatial_order=_capi.SPATIAL_ON)
    order = r.storage_order()
    assert order is not None and (order != np.arange(order.shape[0])).any(), "the cloud was not reordered"
    r.Sort(*view)
    on = planes_of(r, view)
    assert_same_planes(on, off, "spatial_order ON against OFF")
    assert np.unique(on[0]).size > 1000, "the view shows too few splats to tell the numberings apart"
    shown = on[0][on[0] != NONE]
    assert np.isin(shown, r.sorted_indices()).all()
    r.close()


@pytest.mark.parametrize("spatial", [_capi.SPATIAL_OFF, _capi.SPATIAL_ON], ids=["upload_order", "morton_order"])
def test_masked_and_cropped_contexts_equal_the_subset_upload(spatial):
    aos, view = tie_free()
    n = aos.shape[0]
    r = make_renderer(aos, spatial_order=spatial)
    M = vr.matrices()["scaled"]                                  # q is exact for every float32 centre
    in_box = vr.crop(aos[:, 0:3], M, "box")
    assert 0.1 * n < in_box.sum() < 0.9 * n
    for what, keep_mask, apply in (("mask", vr.random_mask(n), lambda m: r.SetVisibility(m)),
                                   ("crop", in_box, lambda m: (r.SetVisibility(None), r.SetCrop(M, "box")))):
        apply(keep_mask)
        r.Sort(*view)
        got = planes_of(r, view)
        keep = np.flatnonzero(keep_mask)
        sub = sorted_planes(aos[keep], view, spatial_order=spatial)
        want = np.where(sub[0] == NONE, np.uint32(NONE), keep[np.minimum(sub[0], keep.shape[0] - 1)].astype(np.uint32))
        assert_same_planes(got, (want, sub[1]), "%s against the subset upload" % what)
        shown = got[0][got[0] != NONE]
        assert shown.size and keep_mask[shown].all(), "%s: a hidden splat appears" % what
    r.close()


# ---- 5. storage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["sh_fp16", "sh_q8"])
def test_compact_storages_give_the_plane_of_their_download(storage):
    aos, view = tie_free()
    r = make_renderer(aos, cloud_storage=storage)
    assert r.cloud_storage() == storage
    r.Sort(*view)
    got = planes_of(r, view)
    stored = r.download_cloud(True)
    r.close()
    assert_same_planes(got, sorted_planes(stored, view), storage)


# ---- 6. mark_ids -----------------------------------------------------------------------------------------------------------------
def device_bytes(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def test_mark_ids_against_numpy(sparse_planes):
    import torch
    r, W, H, view = case_renderer("sparse")
    n = ids_rule.case("sparse")[0].shape[0]
    plane = Pitched(H, W, np.uint32, ID_FILL, pad=5, plane=True)
    r.RenderIds(*view, out_ptr=plane.ptr, pitch_bytes=plane.pitch)
    ids = sparse_planes[0]
    rng = np.random.default_rng(5)
    region = rng.choice(np.array([0, 2, 255], np.uint8), (H, W))
    GUARD = 16                                                   # bytes behind the mask: an id >= n stored through would land here

    def marked(start, value, d_ids, pitch, w, h, d_region=None, region_pitch=0):
        host = np.concatenate([start, np.full(GUARD, 0x5A, np.uint8)])
        m = device_bytes(host)
        r.MarkIds(d_ids, pitch, w, h, m.data_ptr(), value, region_ptr=d_region, region_pitch_bytes=region_pitch)
        r.synchronize()
        out = m.cpu().numpy()
        assert (out[n:] == 0x5A).all(), "bytes behind the mask were written"
        return out[:n]

    ones, zeros = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    # the whole plane, behind the frame that writes it on the same stream; both values
    same_bits(marked(ones, 0, plane.ptr, plane.pitch, W, H), ids_rule.mark_reference(ids, ones, 0), "whole plane, value 0")
    same_bits(plane.read("the id plane"), ids, "the device plane")
    sel = marked(zeros, 1, plane.ptr, plane.pitch, W, H)
    same_bits(sel, ids_rule.mark_reference(ids, zeros, 1), "whole plane, value 1")
    assert sel.sum() == np.unique(ids[ids != NONE]).size and np.isin(np.flatnonzero(sel), ids).all()
    # a region of bytes 0 / 2 / 255, tight and pitched; any value is stored as it is
    d_region = device_bytes(region)
    same_bits(marked(ones, 0, plane.ptr, plane.pitch, W, H, d_region.data_ptr()), ids_rule.mark_reference(ids, ones, 0, region), "region")
    wide = np.full((H, W + 9), 255, np.uint8)                    # padding that would select everything
    wide[:, :W] = region
    d_wide = device_bytes(wide)
    same_bits(marked(zeros, 7, plane.ptr, plane.pitch, W, H, d_wide.data_ptr(), W + 9), ids_rule.mark_reference(ids, zeros, 7, region),
              "pitched region, value 7")
    # a window of the plane: a rectangle through pointer and pitch
    x0, y0, w, h = 100, 60, 150, 90
    rect_ptr = plane.ptr + y0 * plane.pitch + 4 * x0
    same_bits(marked(ones, 0, rect_ptr, plane.pitch, w, h), ids_rule.mark_reference(ids[y0:y0 + h, x0:x0 + w], ones, 0), "a rectangle")
    # a plane of NONE, and a hand-made plane of ids >= n: every byte stays
    start = rng.integers(0, 256, n, dtype=np.uint8)
    none = device_bytes(np.full((9, 33), NONE, np.uint32))
    same_bits(marked(start, 0, none.data_ptr(), 0, 33, 9), start, "a plane of NONE")
    beyond_host = (n + np.arange(12 * 8) % GUARD).astype(np.uint32).reshape(8, 12)
    beyond_host[3, 4], beyond_host[7, 11] = 0xFFFFFFFE, 1 << 31
    beyond = device_bytes(beyond_host)
    same_bits(marked(start, 255, beyond.data_ptr(), 0, 12, 8), start, "ids beyond the cloud")
    # n must be the cloud's
    m = device_bytes(ones)
    rc = r._lib.msplat_mark_ids(r._ctx, C.c_void_p(plane.ptr), plane.pitch, W, H, None, 0, C.c_void_p(m.data_ptr()), n - 1, 0)
    assert rc == _capi.ERR_INVALID_ARG and "mask bytes" in r.last_error()
    rc = r._lib.msplat_mark_ids(r._ctx, C.c_void_p(plane.ptr), 4 * W - 4, W, H, None, 0, C.c_void_p(m.data_ptr()), n, 0)
    assert rc == _capi.ERR_INVALID_ARG and "pitch" in r.last_error()
    same_bits(m.cpu().numpy(), ones, "a refused call wrote the mask")

    # the loop: brush a rectangle away.  mark -> SetVisibility from the device mask -> Sort: none of the brushed splats is left
    V = r.sort_count()
    brushed = np.unique(ids[y0:y0 + h, x0:x0 + w])
    brushed = brushed[brushed != NONE]
    assert 100 < brushed.size < V
    mask = torch.ones(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    r.MarkIds(rect_ptr, plane.pitch, w, h, mask.data_ptr(), 0)
    r.SetVisibility(mask)
    r.Sort(*view)
    after, _ = planes_of(r, view)
    assert r.sort_count() == V - brushed.size, (r.sort_count(), V, brushed.size)
    assert not np.isin(after, brushed).any(), "a brushed splat is still shown"
    assert (after[y0:y0 + h, x0:x0 + w] != ids[y0:y0 + h, x0:x0 + w])[ids[y0:y0 + h, x0:x0 + w] != NONE].all()
    r.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def raw_ids(r, f, window, ids, pitch=0, depth=None, depth_pitch=0, dev=0):
    win = (C.c_int32 * 4)(*window) if window is not None else None
    return r._lib.msplat_render_ids(r._ctx, *f, win, ids, pitch, depth, depth_pitch, dev)


def test_refusals_say_why_and_leave_the_context_usable():
    r, W, H, view = case_renderer("hand_placed")
    want = planes_of(r, view)
    f = r._args.load(*view)
    ids, z = np.full((H, W), ID_FILL, np.uint32), np.full((H, W), SENTINEL, np.float32)

    def refused(code, words, **kw):
        rc = raw_ids(r, f, kw.pop("window", None), kw.pop("ids", ids.ctypes.data), depth=z.ctypes.data, **kw)
        msg = r.last_error()
        assert rc == code and "msplat_render_ids" in msg and all(w in msg for w in words), (rc, code, msg)
        assert (ids == ID_FILL).all() and (z == SENTINEL).all(), "a refused frame wrote its planes"

    refused(_capi.ERR_INVALID_ARG, ["ids is NULL"], ids=None)
    for window in ((0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -3, 4), (-1, 0, 4, 4), (0, -1, 4, 4), (W - 3, 0, 4, 4), (0, H - 3, 4, 4),
                   (0, 0, W + 1, H), (W, H, 1, 1), (0, 0, 2 ** 31 - 1, 1), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)):
        refused(_capi.ERR_INVALID_ARG, ["window", "not inside"], window=window)
    for pitch in (4 * W - 4, 4 * W + 2, 3):
        refused(_capi.ERR_INVALID_ARG, ["ids pitch"], pitch=pitch)
        refused(_capi.ERR_INVALID_ARG, ["id_depth pitch"], depth_pitch=pitch)
    refused(_capi.ERR_INVALID_ARG, ["ids pitch"], window=(0, 0, 40, 9), pitch=4 * 39)      # 4 w of the window
    assert raw_ids(r, f, (0, 0, 40, 9), ids.ctypes.data, pitch=4 * W, depth=z.ctypes.data, depth_pitch=4 * W) == _capi.OK
    same_bits(np.ascontiguousarray(ids[:9, :40]), np.ascontiguousarray(want[0][:9, :40]), "a window into the viewport's array")
    assert (ids[9:] == ID_FILL).all() and (ids[:9, 40:] == ID_FILL).all()
    ids[...], z[...] = ID_FILL, SENTINEL

    switches = [("msplat_set_depth_test", lambda on: r.set_depth_test(24 if on else 0)),
                ("msplat_set_target_emulation", lambda on: r.set_target_emulation("rgba8" if on else None)),
                ("probe", lambda on: r.set_tile_probe(on)),
                ("banded", lambda on: r.set_band(2 if on else 1, 0))]
    for word, switch in switches:
        switch(True)
        refused(_capi.ERR_UNSUPPORTED, [word])
        with pytest.raises(MsplatError) as e:
            r.Pick(*view, 3, 3)
        assert e.value.code == _capi.ERR_UNSUPPORTED
        r.Render(*view)                                          # the Render of that configuration still works
        switch(False)
        assert_same_planes(planes_of(r, view), want, "after %s" % word)
    r.close()

    # before a Sort, before an upload, with a point cloud
    aos, _, W, H, view = ids_rule.case("hand_placed")
    r = make_renderer(aos)
    with pytest.raises(MsplatError) as e:
        r.RenderIds(*view)
    assert e.value.code == _capi.ERR_NO_SORT and "msplat_render_ids" in r.last_error()
    r.Sort(*view)
    assert_same_planes(planes_of(r, view), want, "after the refusal before the Sort")
    r.close()
    L = _capi.lib()
    cfg = _capi.Config()
    cfg.struct_size = C.sizeof(_capi.Config)
    cfg.t_epsilon = -1.0
    h = C.c_void_p()
    assert L.msplat_create(C.byref(h), C.byref(cfg)) == _capi.OK
    p = [np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)) for x in scenes.default_view(W, H, z=4.0)]
    fp = [x.ctypes.data_as(C.POINTER(C.c_float)) for x in p]
    assert L.msplat_render_ids(h, *fp, None, ids.ctypes.data, 0, None, 0, 0) == _capi.ERR_NO_CLOUD and b"msplat_render_ids" in L.msplat_last_error(h)
    assert L.msplat_mark_ids(h, None, 0, 4, 4, None, 0, None, 0, 0) == _capi.ERR_NO_CLOUD and b"msplat_mark_ids" in L.msplat_last_error(h)
    pts = np.random.default_rng(81).uniform(-1, 1, (500, 8)).astype(np.float32)
    pts[:, 3] = 1.0
    pts[:, 4:] = np.abs(pts[:, 4:])
    assert L.msplat_upload_points(h, pts.ctypes.data, pts.shape[0], 32, 0, 16) == _capi.OK
    assert L.msplat_sort(h, *fp) == _capi.OK
    assert L.msplat_render_ids(h, *fp, None, ids.ctypes.data, 0, None, 0, 0) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    assert L.msplat_mark_ids(h, None, 0, 4, 4, None, 0, None, 500, 0) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    img = np.zeros((H, W, 4), np.float32)
    assert L.msplat_render(h, *fp, img.ctypes.data, 0, 0) == _capi.OK         # the point context still renders
    assert (ids == ID_FILL).all()
    L.msplat_destroy(h)
