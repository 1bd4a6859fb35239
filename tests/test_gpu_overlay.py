"""GPU tests of the render-time overlay (msplat_set_overlay[_device], msplat_set_overlay_palette, msplat_get_overlay; INTEGRATION.md
26).  Three references, none of them the code under test: the rule of tests/overlay_rule.py applied to the records the same context
projected without the overlay (exact); the plain frame of a context that was uploaded the cloud with the tinted splats' SH zeroed,
which project_kernel turns into exactly the colour the grey palette entry sets (exact, through every render path); and the CPU
oracle's frame of the recoloured cloud (check_image's bounds).  Views are 256 x 160, clouds at most 4097 splats;
tests/test_overlay.py checks the fixtures on the CPU.  No test hands a host address to msplat_set_overlay_device: its pointer guard
(check_device_source, before anything is copied) is checked by reading."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi, camera, synthetic
from splatapult_amd.points import PointRenderer
from splatapult_amd.renderer import _aos_upload
from tests import overlay_rule as ov
from tests.checks import check_image, same_bits
from tests.compact_harness import assert_same_frame, capped_renderer
from tests.gpu_harness import (device_frame, host_frame, make_renderer, mixed_plane, oracle_frame, sorted_frame, stereo_frame)
from tests.render_cases import random_bytes, random_dst, random_points

pytestmark = pytest.mark.gpu

VIEW = ov.view()
W, H = ov.W, ov.H
ON, OFF = _capi.SPATIAL_ON, _capi.SPATIAL_OFF
N = 4097
# (full SH, storage, srgb, palette entries): both SH degrees, both storages, both colour spaces, every palette size
KINDS = [(True, "fp32", False, 256), (False, "fp32", True, 3), (True, "sh_q8", True, 1), (True, "sh_q8", False, 256)]


def frame_of(r, view=VIEW):
    """Render (no Sort) and what the frame's lists were"""
    img = r.Render(*view)
    st = r.stats()
    return dict(img=img, keys=r.sorted_keys(), idx=r.sorted_indices(), V=r.sort_count(), drawn=st["drawn"], pairs=st["pairs"])


def check_records(r, cls, pal, what):
    """item 1 on a sorted context without classes: the overlaid Render's records are the rule applied to the plain Render's"""
    plain = frame_of(r)
    rec0, rect0 = r.debug_projected()
    r.SetOverlay(cls, pal)
    _, a = ov.entries(cls, pal)
    assert r.overlay() == dict(has_classes=True, palette_count=pal.shape[0], active=bool((pal[:, 3] != 0).any())), "%s: %s" % (what, r.overlay())
    tinted = frame_of(r)
    rec1, rect1 = r.debug_projected()
    idx = plain["idx"]
    assert rec0.shape == (plain["V"], 12) and rec0.dtype == np.float32, (rec0.shape, rec0.dtype)
    want = rec0.copy()
    want[:, 6:9] = ov.tint(rec0[:, 6:9], cls[idx], pal)
    drawn = (rect0 & 255) <= ((rect0 >> 16) & 255)
    same_bits(rec1[drawn], want[drawn], "%s: the records of the ranks with a rectangle" % what)
    same_bits(np.delete(rec1, [6, 7, 8], axis=1), np.delete(rec0, [6, 7, 8], axis=1), "%s: the lanes that are no colour" % what)
    same_bits(rect1, rect0, "%s: the rectangles" % what)
    for k in ("keys", "idx"):
        same_bits(tinted[k], plain[k], "%s: %s" % (what, k))
    assert (tinted["V"], tinted["drawn"], tinted["pairs"]) == (plain["V"], plain["drawn"], plain["pairs"]), what
    changed = (a[idx] != 0) & drawn
    if changed.any() and pal.shape[0] > 1:
        assert (rec1[changed, 6:9] != rec0[changed, 6:9]).any(), "%s: no colour changed" % what
    return plain, tinted


# ------------------------------------------------------------------------------------------------
# 1. records, exact
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton"])
@pytest.mark.parametrize("n", ov.SIZES)
def test_the_records_are_the_rule_applied_to_the_plain_records(n, spatial):
    for full_sh, storage, srgb, count in KINDS:
        aos = ov.cloud(n, full_sh=full_sh)
        r = make_renderer(aos, srgb=srgb, spatial_order=spatial, cloud_storage=storage)
        if n >= 255:
            assert (r.storage_order() is not None) == (spatial == ON), (n, spatial, r.storage_order() is None)
        r.Sort(*VIEW)
        check_records(r, ov.classes(aos, count), ov.palette(count), "n %d, %s, sh %s, srgb %s, %d entries" % (n, storage, full_sh, srgb, count))
        r.close()


def test_device_classes_a_bool_selection_and_every_a():
    """the device route with the tensor msplat_mark_ids would have written, and one palette entry per a of A_VALUES on a Morton store"""
    import torch
    aos = ov.cloud(N)
    r = make_renderer(aos, spatial_order=ON)
    assert r.storage_order() is not None
    r.Sort(*VIEW)
    assert r.sort_count() % 64 != 0
    sel = ov.selection(N)
    t = torch.from_numpy(sel).to("cuda:0")
    plain = frame_of(r)
    rec0, _ = r.debug_projected()
    for a in ov.A_VALUES:
        pal = np.array([[9.0, 9.0, 9.0, 0.0], [0.25, 1.0, -0.5, a]], np.float32)
        r.SetOverlay(t, pal)
        tinted = frame_of(r)
        rec1, _ = r.debug_projected()
        want = rec0.copy()
        want[:, 6:9] = ov.tint(rec0[:, 6:9], sel[plain["idx"]].astype(np.uint8), pal)
        same_bits(rec1, want, "a = %g: the records" % a)
        assert r.overlay()["active"] == (a != 0)
        if a == 0:
            assert_same_frame(tinted, plain, "a = 0")
        if a == 1:
            on = sel[plain["idx"]]
            assert (rec1[on, 6:9] == pal[1, :3]).all() and on.any()
    r.close()


# ------------------------------------------------------------------------------------------------
# 2. frames, exact: the grey entry against the context whose tinted splats have no SH
# ------------------------------------------------------------------------------------------------

def grey_pair(fmt="fp32", view=VIEW, **kw):
    """(the context of cloud X with the selection tinted grey, the plain context of X with the selection's SH zeroed), both sorted"""
    aos, sel = ov.cloud(N), ov.selection(N)
    a = make_renderer(aos, fb_format=fmt, **kw)
    a.SetOverlay(sel, ov.GREY)
    b = make_renderer(ov.zero_sh(aos, sel), fb_format=fmt, **{k: v for k, v in kw.items() if k != "frames_in_flight"})
    a.Sort(*view)
    b.Sort(*view)
    assert a.overlay()["active"] and not b.overlay()["active"]
    return a, b


@pytest.mark.parametrize("fmt", ["fp32", "fp16", "rgba8"])
def test_grey_frames_host_device_and_load(fmt):
    a, b = grey_pair(fmt)
    dst = random_bytes(H, W, 3) if fmt == "rgba8" else random_dst(H, W, 3, np.float16 if fmt == "fp16" else np.float32)
    for mode, d in (("clear", None), ("load", dst)):
        want = host_frame(b, VIEW, mode, d, call=b.Render)
        same_bits(host_frame(a, VIEW, mode, d, call=a.Render), want, "%s %s: host target" % (fmt, mode))
        same_bits(device_frame(a, VIEW, mode, d, call=a.Render, dtype=want.dtype, fill=77), want, "%s %s: pitched device target" % (fmt, mode))
    if fmt == "fp32":
        a.SetOverlay(None)
        assert not np.array_equal(host_frame(a, VIEW, "clear", call=a.Render), host_frame(b, VIEW, "clear", call=b.Render)), "the tint shows nothing"
    a.close()
    b.close()


def test_grey_layers_and_the_depth_plane():
    a, b = grey_pair()
    plane = mixed_plane(b, VIEW)
    plain = make_renderer(ov.cloud(N))
    plain.Sort(*VIEW)
    _, z_plain = host_frame(plain, VIEW, "clear", call=plain.RenderLayers, depth=True, occluder=plane)
    want, z_want = host_frame(b, VIEW, "clear", call=b.RenderLayers, depth=True, occluder=plane)
    img, z = host_frame(a, VIEW, "clear", call=a.RenderLayers, depth=True, occluder=plane)
    same_bits(img, want, "layers: colour")
    same_bits(z, z_want, "layers: depth")
    same_bits(z, z_plain, "layers: the depth plane against the context without an overlay")
    img, z = device_frame(a, VIEW, "clear", None, call=a.RenderLayers, depth=True, occluder=plane)
    same_bits(img, want, "layers, device: colour")
    same_bits(z, z_plain, "layers, device: depth")
    for r in (a, b, plain):
        r.close()


def test_grey_stereo_with_a_gap_between_the_views():
    eyes = [camera.pose((-0.1, 0.0, 7.0), 0.02), camera.pose((0.1, 0.0, 7.0), -0.02)]
    cam, proj, vp, nf = VIEW
    first = (eyes[0], proj, vp, nf)
    a, b = grey_pair(view=first)
    assert a.sort_count() % 64 != 0, a.sort_count()
    want = stereo_frame(b, eyes, [proj, proj], vp, nf, "clear", None, call=b.RenderStereo)
    got = stereo_frame(a, eyes, [proj, proj], vp, nf, "clear", None, call=a.RenderStereo)
    for e in range(2):
        same_bits(got[e], want[e], "stereo: eye %d" % e)
        same_bits(got[e], host_frame(a, (eyes[e], proj, vp, nf), "clear", call=a.Render), "stereo: eye %d against the mono call" % e)
    assert not np.array_equal(got[0], got[1])
    plane = mixed_plane(b, first)
    wl, wz = stereo_frame(b, eyes, [proj, proj], vp, nf, "clear", None, call=b.RenderStereoLayers, depth=True, occluders=[plane, plane])
    gl, gz = stereo_frame(a, eyes, [proj, proj], vp, nf, "clear", None, call=a.RenderStereoLayers, depth=True, occluders=[plane, plane])
    for e in range(2):
        same_bits(gl[e], wl[e], "stereo layers: eye %d" % e)
        same_bits(gz[e], wz[e], "stereo layers: depth of eye %d" % e)
    a.close()
    b.close()


def test_grey_banded_rows():
    T = _capi.lib().msplat_tile_size()
    first, count, block, stride = 1, 0, 1, 2
    owned = np.isin(np.arange(H) // T, _capi.band_rows(first, count, block, stride, (H + T - 1) // T))
    assert owned.any() and not owned.all()
    a, b = grey_pair()
    want = host_frame(b, VIEW, "clear", call=b.Render)
    same_bits(host_frame(a, VIEW, "clear", call=a.Render), want, "unbanded")
    band = make_renderer(ov.cloud(N))
    band.set_band_layout(first, count, block, stride)
    band.SetOverlay(ov.selection(N), ov.GREY)
    band.Sort(*VIEW)
    dst = random_dst(H, W, 9)
    got = host_frame(band, VIEW, "load", dst, call=band.Render)
    want = host_frame(b, VIEW, "load", dst, call=b.Render)
    same_bits(np.ascontiguousarray(got[owned]), np.ascontiguousarray(want[owned]), "the band's rows")
    assert got[~owned].tobytes() == dst[~owned].tobytes(), "the band touched rows of another band"
    for r in (a, b, band):
        r.close()


def test_grey_four_frames_in_flight():
    import torch
    views = [ov.view(yaw=0.3 * k) for k in range(6)]
    fly, one = grey_pair(frames_in_flight=4)
    fbs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in views]
    torch.cuda.synchronize()
    for k, (cam, proj, vp, nf) in enumerate(views):
        fly.Sort(cam, proj, vp, nf)
        fly.Render(cam, proj, vp, nf, out_ptr=fbs[k].data_ptr(), pitch_bytes=W * 16)
    fly.synchronize()
    for k, view in enumerate(views):
        one.Sort(*view)
        same_bits(fbs[k].cpu().numpy(), host_frame(one, view, "clear", call=one.Render), "frame %d of four in flight" % k)
    fly.close()
    one.close()


# ------------------------------------------------------------------------------------------------
# 3. frames against the oracle, general palettes
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [3, 256])
def test_the_overlaid_frame_matches_the_oracle_of_the_recoloured_cloud(count):
    aos = ov.cloud(N)
    cls, pal = ov.classes(aos, count), ov.palette(count)
    base, rec = ov.recoloured(aos, cls, pal)
    cam, proj, vp, nf = VIEW
    r = make_renderer(base)
    r.SetOverlay(cls, pal)
    r.Sort(*VIEW)
    img = r.Render(*VIEW)
    ref = oracle_frame(rec, True, cam, proj, vp, nf, r=r)
    assert r.sort_count() == ref["V"]
    check_image(img, ref["image"], budget=ref["budget"])
    r.SetOverlay(None)
    plain = r.Render(*VIEW)
    assert np.abs(plain - img).max() > 0.05, "the palette shows nothing"
    r.close()


# ------------------------------------------------------------------------------------------------
# 4. inactive means plain
# ------------------------------------------------------------------------------------------------

def test_an_inactive_overlay_is_a_plain_context():
    aos = ov.cloud(N)
    cls = ov.classes(aos, 3)
    never = make_renderer(aos, two_pass=_capi.TWO_PASS_ON)
    want = sorted_frame(never, VIEW)
    assert never.overlay() == dict(has_classes=False, palette_count=0, active=False)
    blank = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]], np.float32)
    r = make_renderer(aos, two_pass=_capi.TWO_PASS_ON)
    r.Sort(*VIEW)
    frames = r.two_pass_state()[0]

    def plain(what, **state):
        nonlocal frames
        assert r.overlay() == dict(active=False, **state), "%s: %s" % (what, r.overlay())
        assert_same_frame(frame_of(r), want, what)
        assert r.two_pass_info() is not None and r.two_pass_state()[0] == frames + 1, "%s: not a two-pass frame" % what
        frames += 1

    r.SetOverlay(cls)
    plain("classes without a palette", has_classes=True, palette_count=0)
    r.SetOverlay(None, ov.palette(3))
    plain("a palette without classes", has_classes=False, palette_count=3)
    r.SetOverlay(cls, blank)
    plain("a palette of a == 0 only", has_classes=True, palette_count=2)
    r.SetOverlay(palette=ov.palette(3))
    assert r.overlay() == dict(has_classes=True, palette_count=3, active=True)
    assert not np.array_equal(r.Render(*VIEW), want["img"])
    r.SetOverlay(None, None)
    plain("SetOverlay(None, None) after an active overlay", has_classes=False, palette_count=0)
    never.close()
    r.close()


# ------------------------------------------------------------------------------------------------
# 5. two-pass
# ------------------------------------------------------------------------------------------------

def test_an_overlaid_frame_is_a_one_pass_frame_with_the_same_pixels():
    aos = ov.cloud(N)
    cls, pal = ov.classes(aos, 256), ov.palette(256)
    off = make_renderer(aos, two_pass=_capi.TWO_PASS_OFF)
    off.SetOverlay(cls, pal)
    want = sorted_frame(off, VIEW)
    off.SetOverlay(None)
    plain = frame_of(off)
    on = make_renderer(aos, two_pass=_capi.TWO_PASS_ON)
    on.Sort(*VIEW)
    assert_same_frame(frame_of(on), plain, "two passes, no overlay")
    assert on.two_pass_state()[0] == 1
    on.SetOverlay(cls, pal)
    for k in range(3):
        assert_same_frame(frame_of(on), want, "overlaid frame %d on a two_pass = ON context" % k)
        assert on.two_pass_state()[0] == 1 and on.two_pass_info() is None, (k, on.two_pass_state())
    on.SetOverlay(None)
    assert_same_frame(frame_of(on), plain, "two passes again")
    assert on.two_pass_state()[0] == 2 and on.two_pass_info() is not None
    off.close()
    on.close()


# ------------------------------------------------------------------------------------------------
# 6. lifecycle
# ------------------------------------------------------------------------------------------------

def test_uploads_and_compaction_drop_the_classes_and_keep_the_palette():
    import torch
    aos = ov.cloud(257)
    cls, pal = ov.classes(aos, 3), ov.palette(3)
    r = make_renderer(aos)
    r.SetOverlay(cls, pal)
    assert r.overlay() == dict(has_classes=True, palette_count=3, active=True)
    assert r.Init(aos, False, False), r.last_error()
    assert r.overlay() == dict(has_classes=False, palette_count=3, active=False), "Init: %s" % r.overlay()
    want = sorted_frame(r, VIEW)
    r.SetOverlay(cls)
    assert r.overlay()["active"]
    a = synthetic.generate(257, seed=3)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda:0")
    assert r.UpdateFromTensors(dev(a["xyz"]), dev(a["f_dc"]), dev(a["f_rest"]), dev(a["opacity"]), dev(a["log_scale"]), dev(a["rot"])), r.last_error()
    assert r.overlay() == dict(has_classes=False, palette_count=3, active=False), "UpdateFromTensors: %s" % r.overlay()
    assert r.Init(aos, False, False), r.last_error()
    r.SetOverlay(cls)
    mask = np.arange(257) % 3 != 0
    r.SetVisibility(mask)
    assert r.CompactCloud() == int(mask.sum())
    assert r.overlay() == dict(has_classes=False, palette_count=3, active=False), "CompactCloud: %s" % r.overlay()
    sub = make_renderer(np.ascontiguousarray(aos[mask]))
    assert_same_frame(sorted_frame(r, VIEW), sorted_frame(sub, VIEW), "the compacted cloud renders plain")
    # a palette set before the first upload is handed to the contexts Init creates
    early = SplatRenderer(device=0)
    early.SetOverlay(palette=pal)
    assert early.Init(aos, False, False), early.last_error()
    assert early.overlay() == dict(has_classes=False, palette_count=3, active=False)
    assert_same_frame(sorted_frame(early, VIEW), want, "a palette alone")
    early.SetOverlay(cls)
    tinted = early.Render(*VIEW)
    r2 = make_renderer(aos)
    r2.SetOverlay(cls, pal)
    r2.Sort(*VIEW)
    same_bits(tinted, r2.Render(*VIEW), "the palette set before Init")
    for x in (r, sub, early, r2):
        x.close()


@pytest.mark.parametrize("flight", [1, 2])
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton"])
def test_transform_keeps_the_tint_and_append_leaves_the_new_splats_untinted(spatial, flight):
    aos, sel = ov.cloud(N), ov.selection(N)
    M = np.eye(4, dtype=np.float32)
    M[3, :3] = (0.25, -0.125, 0.5)                               # column-major: a translation
    a = make_renderer(aos, spatial_order=spatial, frames_in_flight=flight)
    a.SetOverlay(sel, ov.GREY)
    b = make_renderer(ov.zero_sh(aos, sel), spatial_order=spatial)
    for r in (a, b):
        r.TransformCloud(M.reshape(16))
    assert a.overlay() == dict(has_classes=True, palette_count=2, active=True), a.overlay()
    for k in range(flight):                                       # every context of the rotation
        assert_same_frame(sorted_frame(a, VIEW), sorted_frame(b, VIEW), "after TransformCloud, frame %d" % k)
    extra = ov.cloud(300, seed=5)
    src = make_renderer(extra)
    for r in (a, b):
        k, _ = r.AppendCloud(src)
        assert k == 300
    assert a.overlay() == dict(has_classes=True, palette_count=2, active=True), a.overlay()
    for k in range(flight):
        got = sorted_frame(a, VIEW)
        assert_same_frame(got, sorted_frame(b, VIEW), "after AppendCloud, frame %d" % k)
    rec, _ = a.debug_projected()
    new = got["idx"] >= N
    assert new.any() and not (rec[new, 6:9] == 0.5).all(axis=1).all(), "the appended splats are tinted"
    old = sel[np.minimum(got["idx"], N - 1)] & ~new
    assert (rec[old, 6:9] == 0.5).all()
    for r in (a, b, src):
        r.close()


def test_id_and_score_frames_ignore_the_overlay():
    aos = ov.cloud(N)
    r = make_renderer(aos)
    r.Sort(*VIEW)
    ids0, z0 = r.RenderIds(*VIEW, depth=True)
    s0, p0 = r.RenderScores(*VIEW, pixels=True)
    r.SetOverlay(ov.classes(aos, 256), ov.palette(256))
    img = r.Render(*VIEW)
    rec_tinted, _ = r.debug_projected()
    ids1, z1 = r.RenderIds(*VIEW, depth=True)
    rec_ids, _ = r.debug_projected()
    s1, p1 = r.RenderScores(*VIEW, pixels=True)
    same_bits(ids1, ids0, "ids")
    same_bits(z1, z0, "id depth")
    same_bits(s1.cpu().numpy(), s0.cpu().numpy(), "scores")
    same_bits(p1.cpu().numpy(), p0.cpu().numpy(), "hit counts")
    assert not np.array_equal(rec_ids, rec_tinted), "the id frame ran the overlay kernel"
    same_bits(r.Render(*VIEW), img, "the Render after the id and score frames")
    r.close()


# ------------------------------------------------------------------------------------------------
# 7. grid-stride
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton"])
def test_one_workgroup_walks_every_rank(monkeypatch, spatial):
    aos = ov.cloud(N)
    cls, pal = ov.classes(aos, 256), ov.palette(256)
    free = make_renderer(aos, spatial_order=spatial)
    free.SetOverlay(cls, pal)
    want = sorted_frame(free, VIEW)
    r = capped_renderer(aos, monkeypatch, cap=1, spatial_order=spatial)
    r.Sort(*VIEW)
    _, tinted = check_records(r, cls, pal, "MSPLAT_GRID_CAP=1")
    assert_same_frame(tinted, want, "MSPLAT_GRID_CAP=1 against the uncapped context")
    free.close()
    r.close()


# ------------------------------------------------------------------------------------------------
# 8. refusals
# ------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_as_it_was():
    import torch
    L = _capi.lib()
    aos = ov.cloud(257)
    cls, pal = ov.classes(aos, 3), ov.palette(3)
    r = make_renderer(aos)
    r.SetOverlay(cls, pal)
    want = sorted_frame(r, VIEW)
    state = r.overlay()
    t = torch.from_numpy(cls).to("cuda:0")
    torch.cuda.synchronize()

    def unchanged(what):
        assert r.overlay() == state, "%s: %s" % (what, r.overlay())
        assert_same_frame(frame_of(r), want, what)

    for n in (256, 258, 0):
        assert L.msplat_set_overlay(r._ctx, cls.ctypes.data, n) == _capi.ERR_INVALID_ARG and "class bytes" in r.last_error(), n
        assert L.msplat_set_overlay_device(r._ctx, C.c_void_p(t.data_ptr()), n) == _capi.ERR_INVALID_ARG, n
    unchanged("n != N")
    big = np.zeros((257, 4), np.float32)
    assert L.msplat_set_overlay_palette(r._ctx, big.ctypes.data, 257) == _capi.ERR_INVALID_ARG and "at most 256" in r.last_error()
    for k, v in ((0, np.nan), (6, np.inf), (3, -2.0 ** -20), (7, np.float32(1.0) + np.float32(2.0 ** -23)), (11, np.nan)):
        bad = pal.copy()
        bad.reshape(-1)[k] = v
        assert L.msplat_set_overlay_palette(r._ctx, bad.ctypes.data, 3) == _capi.ERR_INVALID_ARG, (k, v)
    unchanged("a refused palette")
    # at a Render with an active overlay
    for on, off, why in ((lambda: r.set_depth_test(24), lambda: r.set_depth_test(0), "msplat_set_depth_test"),
                         (lambda: r.set_target_emulation("rgba8"), lambda: r.set_target_emulation(None), "msplat_set_target_emulation"),
                         (lambda: r.set_tile_probe(True), lambda: r.set_tile_probe(False), "tile probe")):
        on()
        with pytest.raises(_capi.MsplatError) as e:
            r.Render(*VIEW)
        assert e.value.code == _capi.ERR_UNSUPPORTED and why in r.last_error(), (why, r.last_error())
        r.SetOverlay(None)
        r.Render(*VIEW)                                            # inactive: the frame those settings always gave
        r.SetOverlay(cls)
        off()
        unchanged("after " + why)
    r.close()
    # classes before the upload; a palette may come first and survives the upload
    c = SplatRenderer(device=0)
    assert c._create(False), c.last_error()
    assert L.msplat_set_overlay(c._ctx, cls.ctypes.data, 257) == _capi.ERR_NO_CLOUD
    assert L.msplat_set_overlay_device(c._ctx, C.c_void_p(t.data_ptr()), 257) == _capi.ERR_NO_CLOUD
    assert L.msplat_set_overlay_palette(c._ctx, pal.ctypes.data, 3) == _capi.OK, c.last_error()
    held, args = _aos_upload(aos)                                # (held: the memory args points into)
    assert L.msplat_upload_cloud(c._ctx, *args) == _capi.OK, c.last_error()
    c._n = 257
    assert c.overlay() == dict(has_classes=False, palette_count=3, active=False)
    c.SetOverlay(cls)
    assert_same_frame(sorted_frame(c, VIEW), want, "a palette set before the upload")
    c.close()
    # a point cloud
    p = PointRenderer(device=0)
    assert p.Init(random_points(500, 3)), p.last_error()
    img = p.Render(*VIEW)
    with pytest.raises(_capi.MsplatError) as e:
        p.SetOverlay(np.ones(500, np.uint8))
    assert e.value.code == _capi.ERR_UNSUPPORTED
    p.SetOverlay(palette=pal)                                    # a palette alone is no overlay
    assert p.overlay() == dict(has_classes=False, palette_count=3, active=False)
    same_bits(p.Render(*VIEW), img, "the points after the refusal")
    p.close()
