"""GPU tests of per-splat visibility (msplat_set_visibility[_device], msplat_set_crop).  The reference of every
comparison is a context that was uploaded ONLY the visible splats, in the full cloud's upload order -- merged behaviour, never the
code under test -- and every comparison is exact: hiding a splat is defined as the presort cull rejecting it, so sort_count, the
sorted keys, the sorted indices (mapped back through the kept indices) and the frame's bits must be the subset context's.  A crop is
compared with the mask tests/visibility_rule.py computes from the header's fp32 rule.  Views are 256 x 160, clouds at most 4097
splats; tests/test_visibility.py checks the fixtures on the CPU.  No test hands a host address to msplat_set_visibility_device: its
pointer guard (check_device_source, before anything is copied) is checked by reading."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi, synthetic
from splatapult_amd.points import PointRenderer
from splatapult_amd.renderer import _aos_upload
from tests import scenes
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import Pitched, device_frame, host_frame, make_renderer, mixed_plane, sorted_frame, stereo_frame
from tests.render_cases import random_dst, random_points, stereo_eyes

pytestmark = pytest.mark.gpu

VIEW = vr.view()
OFF, ON = _capi.SPATIAL_OFF, _capi.SPATIAL_ON
EMPTY = np.zeros((0, 61), np.float32)


def cloud(n):
    return vr.cloud_aos(n, vr.TIE_FREE[1]) if n == vr.TIE_FREE[0] else vr.cloud_aos(n)


def kept(mask):
    return np.flatnonzero(np.asarray(mask) != 0)


def subset_frame(aos, keep, view=VIEW, **kw):
    """the reference: Sort + Render of a context that holds only aos[keep]"""
    s = make_renderer(np.ascontiguousarray(aos[keep]), **kw)
    f = sorted_frame(s, view)
    s.close()
    return f


def assert_is_the_subset(got, ref, keep, what, ordered=True):
    """got: a masked context's frame; ref: the subset context's.  ordered = False: the two store their splats in different
    (Morton) orders, so indices are compared inside runs of equal keys as sets, and the frame only when there is no such run"""
    assert got["V"] == ref["V"], "%s: sort_count %d, the subset's %d" % (what, got["V"], ref["V"])
    same_bits(got["keys"], ref["keys"], "%s: sorted keys" % what)
    want = keep[ref["idx"]].astype(np.uint32)
    ties = np.unique(got["keys"]).size != got["V"]
    if ordered or not ties:
        same_bits(got["idx"], want, "%s: sorted indices" % what)
        same_bits(got["img"], ref["img"], "%s: the frame" % what)
        assert (got["drawn"], got["pairs"]) == (ref["drawn"], ref["pairs"]), what
    else:
        by_run = lambda idx: np.lexsort((idx, got["keys"]))
        same_bits(got["idx"][by_run(got["idx"])], want[by_run(want)], "%s: sorted indices inside equal-key runs" % what)


# ---- 1. masks against the subset upload -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
@pytest.mark.parametrize("n", vr.SIZES)
def test_a_masked_context_equals_the_subset_upload(n, spatial):
    aos = cloud(n)
    r = make_renderer(aos, spatial_order=spatial)
    assert (r.storage_order() is not None) == (spatial == ON)
    before = sorted_frame(r, VIEW)
    assert r.visibility() == dict(has_mask=False, crop=None, hidden=0)
    for name, mask in vr.mask_cases(n).items():
        keep = kept(mask)
        r.SetVisibility(mask)
        got = sorted_frame(r, VIEW)
        assert r.visibility() == dict(has_mask=True, crop=None, hidden=n - keep.size), (name, r.visibility())
        ref = subset_frame(aos, keep, spatial_order=spatial)
        # the tie-free cloud: exact in either storage order
        assert_is_the_subset(got, ref, keep, "n %d, %s" % (n, name), ordered=spatial == OFF or n == vr.TIE_FREE[0])
        if name == "all_visible":
            for k in ("keys", "idx", "img"):
                same_bits(got[k], before[k], "all visible against no mask: %s" % k)
        if name == "all_hidden":
            assert got["V"] == 0 and got["idx"].size == 0
            same_bits(got["img"], subset_frame(EMPTY, np.zeros(0, np.int64))["img"], "all hidden against the empty cloud")
    r.SetVisibility(None)
    after = sorted_frame(r, VIEW)
    assert r.visibility() == dict(has_mask=False, crop=None, hidden=0)
    for k in ("keys", "idx", "img"):
        same_bits(after[k], before[k], "mask cleared: %s" % k)
    r.close()


# ---- 2. the context's cull boxes ------------------------------------------------------------------------------------------------
def test_cull_boxes_are_built_over_the_visible_splats():
    n = vr.TIE_FREE[0]
    aos = cloud(n)
    r = make_renderer(aos, spatial_order=ON)
    order = r.storage_order()
    r.Sort(*VIEW)
    live0, total0, _ = r.cull_boxes()
    assert total0 == (n + vr.BOX - 1) // vr.BOX and 0 < live0 <= total0
    r.SetVisibility(np.zeros(n, bool))
    r.Sort(*VIEW)
    assert r.cull_boxes()[:2] == (0, total0) and r.sort_count() == 0
    # (one_box_visible: upload numbers 256..511, scattered over the Morton boxes)
    for name in ("random_30", "one_box_visible"):
        mask = vr.mask_cases(n)[name]
        r.SetVisibility(mask)
        first = sorted_frame(r, VIEW)
        live, total, _ = r.cull_boxes()
        holding = np.unique(np.flatnonzero(mask[order]) // vr.BOX).size
        assert total == total0 and live <= live0 and live <= holding, (name, live, live0, holding)
        # an earlier Sort saw less than 70 % of the cloud: pass 0 now walks the listed boxes -- the context's -- only
        assert first["V"] * 10 < n * 7
        second = sorted_frame(r, VIEW)
        assert r.cull_boxes() == (live, total, True), (name, r.cull_boxes())
        for k in ("keys", "idx", "img"):
            same_bits(second[k], first[k], "%s, listed pass 0: %s" % (name, k))
        assert_is_the_subset(second, subset_frame(aos, kept(mask), spatial_order=ON), kept(mask), name)
    r.close()


# ---- 3. the crop ----------------------------------------------------------------------------------------------------------------
def test_a_crop_equals_the_mask_of_the_rule():
    aos = vr.crop_cloud()
    n, xyz = aos.shape[0], aos[:, 0:3]
    a, b = make_renderer(aos, spatial_order=OFF), make_renderer(aos, spatial_order=OFF)
    extra = vr.random_mask(n, seed=9, share=0.6)
    for matrix, shape, invert in vr.CROPS:
        what = "%s %s%s" % (matrix, shape, " inverted" if invert else "")
        M = vr.matrices()[matrix]
        expected = vr.crop(xyz, M, shape, invert)
        a.SetCrop(M, shape, invert)
        b.SetVisibility(expected)
        fa, fb = sorted_frame(a, VIEW), sorted_frame(b, VIEW)
        assert a.visibility() == dict(has_mask=False, crop=(shape, invert), hidden=n - int(expected.sum())), (what, a.visibility())
        for k in ("keys", "idx", "img"):
            same_bits(fa[k], fb[k], "%s: %s" % (what, k))
        assert 0 < fa["V"] < n
        if matrix != "rotated":                                  # the centres ON the surface are inside, their float neighbours not
            at = 0 if matrix == "identity" else 12
            shown = np.isin(np.arange(24), fa["idx"])
            on, out = shown[at:at + 6], shown[at + 6:at + 12]
            assert (out.all() and not on.any()) if invert else (on.all() and not out.any()), (what, shown)
        # mask and crop together: the AND
        a.SetVisibility(extra)
        b.SetVisibility(extra & expected)
        fa, fb = sorted_frame(a, VIEW), sorted_frame(b, VIEW)
        assert a.visibility() == dict(has_mask=True, crop=(shape, invert), hidden=n - int((extra & expected).sum())), what
        for k in ("keys", "idx", "img"):
            same_bits(fa[k], fb[k], "%s and a mask: %s" % (what, k))
        a.SetVisibility(None)
    # ... and the subset upload itself, once per shape
    for matrix, shape, invert in (("rotated", "box", False), ("scaled", "sphere", True)):
        M = vr.matrices()[matrix]
        a.SetCrop(M, shape, invert)
        keep = kept(vr.crop(xyz, M, shape, invert))
        assert_is_the_subset(sorted_frame(a, VIEW), subset_frame(aos, keep, spatial_order=OFF), keep, "%s %s" % (matrix, shape))
    a.close(), b.close()


# ---- 4. routes and refusals -----------------------------------------------------------------------------------------------------
def test_a_device_mask_equals_the_host_mask():
    import torch
    n = 4097
    aos, mask = cloud(n), vr.random_mask(4097, seed=4, share=0.4)
    r = make_renderer(aos, spatial_order=ON)
    r.SetVisibility(mask)
    host = sorted_frame(r, VIEW)
    r.SetVisibility(None)
    for t in (torch.from_numpy(mask).to("cuda:0"), torch.from_numpy(mask.astype(np.uint8) * 255).to("cuda:0")):
        torch.cuda.synchronize()
        r.SetVisibility(t)
        got = sorted_frame(r, VIEW)
        assert r.visibility()["hidden"] == n - int(mask.sum())
        for k in ("keys", "idx", "img"):
            same_bits(got[k], host[k], "device route (%s): %s" % (t.dtype, k))
        r.SetVisibility(None)
    r.close()


def test_refusals_leave_the_context_as_it_was():
    import torch
    L = _capi.lib()
    n = 257
    aos, mask = cloud(n), vr.mask_cases(257)["every_other"]
    r = make_renderer(aos)
    before = sorted_frame(r, VIEW)
    m8 = np.ones(n + 1, np.uint8)
    t8 = torch.ones(n + 1, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for wrong in (n - 1, n + 1, 0):
        assert L.msplat_set_visibility(r._ctx, m8.ctypes.data, wrong) == _capi.ERR_INVALID_ARG
        assert L.msplat_set_visibility_device(r._ctx, C.c_void_p(t8.data_ptr()), wrong) == _capi.ERR_INVALID_ARG
    assert L.msplat_set_crop(r._ctx, np.eye(4, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float)), 5) == _capi.ERR_INVALID_ARG
    assert r.visibility() == dict(has_mask=False, crop=None, hidden=0)
    after = sorted_frame(r, VIEW)
    for k in ("keys", "idx", "img"):
        same_bits(after[k], before[k], "after the refusals: %s" % k)
    r.close()
    # no cloud: no numbering for a mask to speak; the crop is world space and may come first
    c = SplatRenderer(device=0, spatial_order=OFF)
    assert c._create(False), c.last_error()
    assert L.msplat_set_visibility(c._ctx, m8.ctypes.data, 0) == _capi.ERR_NO_CLOUD
    assert L.msplat_set_visibility_device(c._ctx, C.c_void_p(t8.data_ptr()), n) == _capi.ERR_NO_CLOUD
    M = vr.matrices()["scaled"]
    c.SetCrop(M, "box")
    aos_c = vr.crop_cloud()
    held, args = _aos_upload(aos_c)                              # (held: the memory args points into)
    rc = L.msplat_upload_cloud(c._ctx, *args)
    assert rc == _capi.OK, c.last_error()
    c._n = aos_c.shape[0]
    keep = kept(vr.crop(aos_c[:, 0:3], M, "box"))
    assert_is_the_subset(sorted_frame(c, VIEW), subset_frame(aos_c, keep, spatial_order=OFF), keep, "a crop set before the upload")
    c.close()


def test_a_point_cloud_context_is_refused_and_still_renders():
    pts = random_points(500, 3)
    p = PointRenderer(device=0)
    assert p.Init(pts), p.last_error()
    want = p.Render(*VIEW)
    with pytest.raises(_capi.MsplatError) as e:
        p.SetVisibility(np.ones(500, bool))
    assert e.value.code == _capi.ERR_UNSUPPORTED
    with pytest.raises(_capi.MsplatError) as e:
        p.SetCrop(np.eye(4), "sphere")
    assert e.value.code == _capi.ERR_UNSUPPORTED
    assert p.visibility() == dict(has_mask=False, crop=None, hidden=0)
    same_bits(p.Render(*VIEW), want, "the points after the refusals")
    assert (want[..., :3] != 0).any()
    p.close()


# ---- 5. lifetime ----------------------------------------------------------------------------------------------------------------
def test_a_change_shows_at_the_next_sort_and_frames_are_ordered_on_the_stream():
    n = 4097
    aos = cloud(n)
    A, B = vr.random_mask(n, seed=5, share=0.5), vr.random_mask(n, seed=6, share=0.2)
    want_a = subset_frame(aos, kept(A), spatial_order=OFF)["img"]
    want_b = subset_frame(aos, kept(B), spatial_order=OFF)["img"]
    r = make_renderer(aos, spatial_order=OFF)
    unmasked = sorted_frame(r, VIEW)["img"]
    # mask A, Sort + Render, mask B, Sort + Render, nothing synchronises in between
    tg = [Pitched(vr.H, vr.W, np.float32, 0.0) for _ in range(2)]
    for mask, t in ((A, tg[0]), (B, tg[1])):
        r.SetVisibility(mask)
        r.Sort(*VIEW)
        r.Render(*VIEW, out_ptr=t.ptr, pitch_bytes=t.pitch)
    r.synchronize()
    same_bits(tg[0].read("frame A"), want_a, "mask A's frame")
    same_bits(tg[1].read("frame B"), want_b, "mask B's frame")
    # a Render draws the latest Sort: a new mask without a new Sort changes nothing
    r.SetVisibility(A)
    same_bits(r.Render(*VIEW), want_b, "mask A set, no Sort since mask B's")
    assert r.visibility()["hidden"] == n - int(B.sum())          # (the latest Sort's plane)
    r.Sort(*VIEW)
    same_bits(r.Render(*VIEW), want_a, "mask A after its Sort")
    # both cleared: the unmasked frame
    r.SetCrop(vr.matrices()["identity"], "sphere")
    r.SetVisibility(None)
    r.SetCrop(None)
    r.Sort(*VIEW)
    same_bits(r.Render(*VIEW), unmasked, "mask and crop cleared")
    assert r.visibility() == dict(has_mask=False, crop=None, hidden=0)
    r.close()


def test_an_upload_drops_the_mask_and_keeps_the_crop():
    import torch
    n = 1000
    a = synthetic.generate(n, seed=0xC0, full_sh=True, log_scale_mean=-3.0)
    names = ("xyz", "f_dc", "f_rest", "opacity", "log_scale", "rot")
    dev = lambda arr: torch.from_numpy(np.array(arr, order="C")).to("cuda:0")
    M = vr.matrices()["rotated"]
    moved = (a["xyz"] + np.array([0.4, -0.3, 0.2], np.float32)).astype(np.float32)
    for xyz in (a["xyz"], moved):
        assert (vr.surface_distance(xyz, M, "box") > 1e-5).all()  # (no centre a last bit could flip)
    r = SplatRenderer(device=0, spatial_order=OFF)
    assert r.InitFromTensors(*[dev(a[k]) for k in names]), r.last_error()
    r.SetCrop(M, "box")
    r.SetVisibility(vr.random_mask(n, seed=7))
    r.Sort(*VIEW)
    assert r.visibility()["has_mask"] and r.visibility()["hidden"] > 0
    assert r.UpdateFromTensors(*[dev(moved if k == "xyz" else a[k]) for k in names]), r.last_error()
    assert r.visibility() == dict(has_mask=False, crop=("box", False), hidden=0)
    got = sorted_frame(r, VIEW)
    expected = vr.crop(moved, M, "box")
    assert expected.sum() != vr.crop(a["xyz"], M, "box").sum()   # the crop was evaluated on the NEW positions
    assert r.visibility() == dict(has_mask=False, crop=("box", False), hidden=n - int(expected.sum()))
    s = SplatRenderer(device=0, spatial_order=OFF)
    keep = kept(expected)
    assert s.InitFromTensors(*[dev((moved if k == "xyz" else a[k])[keep]) for k in names]), s.last_error()
    assert_is_the_subset(got, sorted_frame(s, VIEW), keep, "the crop after UpdateFromTensors")
    r.close(), s.close()


# ---- 6. everything downstream of the Sort ----------------------------------------------------------------------------------------
N_DOWN = 4097
MASK = vr.random_mask(N_DOWN, seed=8, share=0.5)


def pair(aos=None, prepare=None, **kw):
    """(the masked context, the subset context) under the same settings, the cloud stored in upload order"""
    aos = cloud(N_DOWN) if aos is None else aos
    m = make_renderer(aos, spatial_order=OFF, **kw)
    s = make_renderer(np.ascontiguousarray(aos[kept(MASK)]), spatial_order=OFF, **kw)
    for r in (m, s):
        if prepare:
            prepare(r)
    m.SetVisibility(MASK)
    return m, s


@pytest.mark.parametrize("kw", [dict(cloud_storage="sh_fp16"), dict(cloud_storage="sh_q8"), dict(fb_format="fp16"), dict(fb_format="rgba8"),
                                dict(async_submit=True)], ids=lambda kw: "-".join("%s" % v for v in kw.values()))
def test_downstream_storage_targets_and_async_submit(kw):
    m, s = pair(**kw)
    assert_is_the_subset(sorted_frame(m, VIEW), sorted_frame(s, VIEW), kept(MASK), str(kw))
    m.close(), s.close()


def test_downstream_sh_degree_0():
    m, s = pair(aos=np.ascontiguousarray(cloud(N_DOWN)[:, :25]))
    assert_is_the_subset(sorted_frame(m, VIEW), sorted_frame(s, VIEW), kept(MASK), "SH degree 0")
    m.close(), s.close()


def test_downstream_lsd8_sort(monkeypatch):
    monkeypatch.setenv("MSPLAT_SORT", "lsd8")
    m, s = pair()
    assert_is_the_subset(sorted_frame(m, VIEW), sorted_frame(s, VIEW), kept(MASK), "MSPLAT_SORT=lsd8")
    m.close(), s.close()


@pytest.mark.parametrize("mode", ["load", "premultiplied"])
def test_downstream_target_modes(mode):
    m, s = pair()
    dst = random_dst(vr.H, vr.W, 12)
    imgs = []
    for r in (m, s):
        r.Sort(*VIEW)
        imgs.append(host_frame(r, VIEW, mode, dst, call=r.Render))
    same_bits(imgs[0], imgs[1], mode)
    m.close(), s.close()


def test_downstream_layers_frame():
    m, s = pair()
    s.Sort(*VIEW)
    plane = mixed_plane(s, VIEW)
    out = []
    for r in (m, s):
        r.Sort(*VIEW)
        out.append(device_frame(r, VIEW, "clear", None, call=r.RenderLayers, depth=True, occluder=plane))
    same_bits(out[0][0], out[1][0], "RenderLayers: colour")
    same_bits(out[0][1], out[1][1], "RenderLayers: the depth plane")
    m.close(), s.close()


def test_downstream_stereo_chain():
    cams, proj, vp, nf = stereo_eyes(vr.W, vr.H)
    m, s = pair()
    out = []
    for r in (m, s):
        r.Sort(cams[0], proj, vp, nf)
        out.append(stereo_frame(r, cams, [proj, proj], vp, nf, None, None, call=r.RenderStereo))
    for eye in range(2):
        same_bits(out[0][eye], out[1][eye], "RenderStereo: eye %d" % eye)
    m.close(), s.close()


def test_downstream_two_pass_frame():
    m, s = pair(two_pass=_capi.TWO_PASS_ON)
    out = []
    for r in (m, s):
        r.two_pass_state(share=0.2)
        r.Sort(*VIEW)
        out.append(device_frame(r, VIEW, None, None, call=r.Render))
        assert r.two_pass_state()[0] > 0, "the frame did not run in two passes"
    same_bits(out[0], out[1], "a two-pass frame")
    m.close(), s.close()


def test_downstream_band_layout_with_band_cull():
    m, s = pair(prepare=lambda r: r.set_band_layout(1, 0, 3, 4, band_cull=True))      # bin rows 1..3 of 5
    fm, fs = sorted_frame(m, VIEW), sorted_frame(s, VIEW)
    assert 0 < fm["V"] < int(MASK.sum())
    assert_is_the_subset(fm, fs, kept(MASK), "band layout with band_cull")
    m.close(), s.close()


def test_downstream_four_frames_in_flight_with_the_mask_changed_at_frame_4():
    aos = cloud(N_DOWN)
    other = vr.random_mask(N_DOWN, seed=10, share=0.3)
    views = [scenes.default_view(vr.W, vr.H, z=7.0, yaw=0.2 + 0.15 * k) for k in range(8)]
    want = []
    for mask, vs in ((MASK, views[:4]), (other, views[4:])):
        s = make_renderer(np.ascontiguousarray(aos[kept(mask)]), spatial_order=OFF)
        for v in vs:
            s.Sort(*v)
            want.append(s.Render(*v))
        s.close()
    fly = make_renderer(aos, spatial_order=OFF, frames_in_flight=4)
    fly.SetVisibility(MASK)
    tg = [Pitched(vr.H, vr.W, np.float32, 0.0) for _ in views]
    for k, v in enumerate(views):
        if k == 4:
            fly.SetVisibility(other)                             # every context of the rotation, frames 0..3 still in flight
        fly.Sort(*v)
        fly.Render(*v, out_ptr=tg[k].ptr, pitch_bytes=tg[k].pitch)
    fly.synchronize()
    for k in range(len(views)):
        same_bits(tg[k].read("frame %d" % k), want[k], "frame %d of eight, four in flight" % k)
    fly.close()
