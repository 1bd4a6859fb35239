"""GPU tests of the 8-bit render targets MSPLAT_FB_RGBA8 ("rgba8") and MSPLAT_FB_SRGB8_ALPHA8 ("srgb8").

Only the compositors' final store (and MSPLAT_TARGET_LOAD's destination read) knows the format: the accumulators are those of an
MSPLAT_FB_RGBA32F context, bit for bit.  So every check here is the rule of tests/fb8_rule.py applied to the fp32 context's frame of
the same Sort -- RGBA8 byte for byte; SRGB8_ALPHA8 alpha byte for byte and r g b within 0.5 + 2^-10 of a code of the float64
encode -- or, for the execution shapes, the plain 8-bit frame byte for byte.  Scenes and helpers are those of
tests/render_cases.py and tests/gpu_harness.py."""
import numpy as np
import pytest

from splatapult_amd import MsplatError, SplatRenderer, SplatRendererGroup, _capi, camera
from tests import fb8_rule, scenes
from tests.gpu_harness import bin_px, device_frame, fp32_frame, host_frame, make_renderer, sorted_renderer
from tests.render_cases import const_dst, random_bytes, view_of

pytestmark = pytest.mark.gpu

FORMATS = ["rgba8", "srgb8"]
SENTINEL = 0xA5


def is_srgb(fmt):
    return fmt == "srgb8"


def fp32_load(name, dst):
    """the fp32 context's LOAD frame over the float destination dst"""
    cloud, W, H, view = view_of(name)
    r = make_renderer(cloud)
    r.Sort(*view)
    return host_frame(r, view, "load", dst, call=r.Render)


# ------------------------------------------------------------------------------------------------
# 1. the store
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["sparse", "hard", "dense"])
def test_the_store_is_the_rule_applied_to_the_fp32_frame(name, fmt):
    r, W, H, view = sorted_renderer(name, fmt)
    assert _capi.lib().msplat_get_fb_format(r._ctx) == _capi.FB_FORMATS[fmt]
    x = fp32_frame(name, "clear")
    if name == "sparse":                                    # the scene that reaches both clamps (tests/test_fb8.py, on the oracle)
        assert (x[..., :3] > 1).any() and (x[..., :3] < 0).any() and (x[..., :3] == 0).any()
    host = host_frame(r, view, "clear", call=r.Render)
    assert host.dtype == np.uint8 and host.shape == (H, W, 4)
    fb8_rule.check_frame(host, x, is_srgb(fmt), "%s host" % name)
    dev = device_frame(r, view, "clear", random_bytes(H, W, 1), call=r.Render, fill=SENTINEL)          # (asserts that the padding keeps its bytes)
    fb8_rule.check_frame(dev, x, is_srgb(fmt), "%s device" % name)
    np.testing.assert_array_equal(dev, host)
    assert (host[..., 3] == 255).all()                      # CLEAR's alpha


# ------------------------------------------------------------------------------------------------
# 2. target modes
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["sparse", "hard", "dense"])
def test_target_modes(name, fmt):
    r, W, H, view = sorted_renderer(name, fmt)
    srgb = is_srgb(fmt)
    junk = random_bytes(H, W, 5)
    clear = host_frame(r, view, "clear", junk, call=r.Render)
    pre = host_frame(r, view, "premultiplied", junk, call=r.Render)
    xpre = fp32_frame(name, "premultiplied")
    fb8_rule.check_frame(pre, xpre, srgb, "%s premultiplied" % name)
    np.testing.assert_array_equal(pre[..., :3], clear[..., :3])
    # LOAD over random bytes: the fp32 LOAD frame over the decoded destination
    dst = random_bytes(H, W, 6)
    xload = fp32_load(name, fb8_rule.decode(dst, srgb))
    for got in (host_frame(r, view, "load", dst, call=r.Render), device_frame(r, view, "load", dst, call=r.Render, fill=SENTINEL)):
        fb8_rule.check_frame(got, xload, srgb, "%s load" % name)
        if name == "sparse":
            # a pixel no splat reaches keeps its four bytes (the fp32 PREMULTIPLIED alpha is 1 - T: exactly 0 where T == 1)
            untouched = xpre[..., 3] == 0
            assert untouched.mean() >= 0.01
            assert (got[untouched] == dst[untouched]).all(), "%d untouched pixel(s) changed" % (got[untouched] != dst[untouched]).any(axis=-1).sum()
            assert (got[~untouched] != dst[~untouched]).any()
    np.testing.assert_array_equal(host_frame(r, view, "load", const_dst(H, W, (0, 0, 0, 0), np.uint8), call=r.Render), pre)
    np.testing.assert_array_equal(host_frame(r, view, "load", const_dst(H, W, (0, 0, 0, 255), np.uint8), call=r.Render), clear)
    np.testing.assert_array_equal(host_frame(r, view, "clear", junk, call=r.Render), clear)      # and back


# ------------------------------------------------------------------------------------------------
# 3. execution shapes, against the plain 8-bit frame byte for byte
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_two_pass_frames_and_the_persistent_wave_queue(fmt):
    cloud, W, H, view = view_of("dense", z=5.0, yaw=0.3)          # from outside: saturated centre, unfinished rim
    a = make_renderer(cloud, fb_format=fmt, two_pass=_capi.TWO_PASS_OFF)
    b = make_renderer(cloud, fb_format=fmt, two_pass=_capi.TWO_PASS_ON)
    q = make_renderer(cloud, fb_format=fmt, two_pass=_capi.TWO_PASS_OFF, compositor_waves=64)
    b.two_pass_state(0.3)
    dst = random_bytes(H, W, 21)
    for r in (a, b, q):
        r.Sort(*view)
    for mode in ("clear", "load", "premultiplied"):
        want = host_frame(a, view, mode, dst, call=a.Render)
        np.testing.assert_array_equal(host_frame(b, view, mode, dst, call=b.Render), want, err_msg="two passes, " + mode)
        np.testing.assert_array_equal(host_frame(q, view, mode, dst, call=q.Render), want, err_msg="64 persistent waves, " + mode)
    assert b.two_pass_state(0.3)[0] == 3 and a.two_pass_state()[0] == 0
    items, grid = q.compositor_launch()[:2]
    assert grid == 64 < items, (items, grid)                 # persistent waves on the work queue


@pytest.mark.parametrize("fmt", FORMATS)
def test_render_stereo_equals_two_renders(fmt):
    import torch
    cloud = scenes.synth_cloud(10000, 61, log_scale_mean=-3.2)
    W, H = 504, 560                                              # test_two_views_share_one_sort's views
    cam0 = camera.pose((0.0, 0.0, 7.0))
    eyes = [camera.translate_local(cam0, dx=-0.032), camera.translate_local(cam0, dx=+0.032)]
    projs = [camera.create_projection(-1.0, 0.8, 0.95, -0.95), camera.create_projection(-0.8, 1.0, 0.95, -0.95)]
    vp, nf = [0, 0, W, H], scenes.NF
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(eyes[0], projs[0], vp, nf)
    dsts = [random_bytes(H, W, 31), random_bytes(H, W, 32)]
    for mode in ("clear", "load"):
        want = [device_frame(r, (eyes[k], projs[k], vp, nf), mode, dsts[k], call=r.Render, fill=SENTINEL, pad=0) for k in range(2)]
        fbs = [torch.from_numpy(dsts[k].copy()).to("cuda:0") for k in range(2)]
        torch.cuda.synchronize()
        r.RenderStereo(eyes, projs, vp, nf, out_ptrs=[f.data_ptr() for f in fbs], pitch_bytes=W * 4)
        r.synchronize()
        for k in range(2):
            np.testing.assert_array_equal(fbs[k].cpu().numpy(), want[k], err_msg="%s eye %d" % (mode, k))
        assert not np.array_equal(want[0], want[1])
    # host targets go view by view
    r.set_target_mode("clear")
    outs = r.RenderStereo(eyes, projs, vp, nf)
    for k in range(2):
        assert outs[k].dtype == np.uint8
        np.testing.assert_array_equal(outs[k], host_frame(r, (eyes[k], projs[k], vp, nf), "clear", call=r.Render))


@pytest.mark.parametrize("fmt", FORMATS)
def test_four_frames_in_flight_equal_one_context(fmt):
    import torch
    cloud, W, H, _ = view_of("sparse")
    views = [scenes.default_view(W, H, z=7.0, yaw=0.3 * k) for k in range(6)]
    dsts = [random_bytes(H, W, 40 + k) for k in range(len(views))]
    one = make_renderer(cloud, fb_format=fmt)
    fly = make_renderer(cloud, fb_format=fmt, frames_in_flight=4)             # attached contexts, async_submit
    for mode in ("clear", "load"):
        fly.set_target_mode(mode)
        fbs = [torch.from_numpy(d.copy()).to("cuda:0") for d in dsts]
        torch.cuda.synchronize()
        for k, (cam, proj, vp, nf) in enumerate(views):
            fly.Sort(cam, proj, vp, nf)
            fly.Render(cam, proj, vp, nf, out_ptr=fbs[k].data_ptr(), pitch_bytes=W * 4)
        fly.synchronize()
        for k, view in enumerate(views):
            one.Sort(*view)
            np.testing.assert_array_equal(fbs[k].cpu().numpy(), host_frame(one, view, mode, dsts[k], call=one.Render), err_msg="%s frame %d" % (mode, k))


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_banded_context_writes_its_own_rows_only(fmt):
    plain, W, H, view = sorted_renderer("sparse", fmt)
    cloud = view_of("sparse")[0]
    T = bin_px()
    rows_full = (H + T - 1) // T
    first, count, block, stride = 1, 0, 2, 5               # blocks of two bin rows: 1-2, 6-7, ...
    owned_bins = _capi.band_rows(first, count, block, stride, rows_full)
    assert 1 < len(owned_bins) < rows_full
    owned = np.isin(np.arange(H) // T, owned_bins)
    band = make_renderer(cloud, fb_format=fmt)
    band.set_band_layout(first, count, block, stride)
    band.Sort(*view)
    for mode, dst in (("clear", const_dst(H, W, (SENTINEL,) * 4, np.uint8)), ("load", random_bytes(H, W, 51))):
        want = host_frame(plain, view, mode, dst, call=plain.Render)
        for got in (host_frame(band, view, mode, dst, call=band.Render), device_frame(band, view, mode, dst, call=band.Render, fill=SENTINEL)):
            np.testing.assert_array_equal(got[owned], want[owned])
            assert got[~owned].tobytes() == dst[~owned].tobytes(), "mode %s touched rows of another band" % mode


@pytest.mark.parametrize("fmt", FORMATS)
def test_bands_of_every_kind_reassemble_the_unbanded_frame(fmt):
    plain, W, H, view = sorted_renderer("sparse", fmt)
    cloud = view_of("sparse")[0]
    full = host_frame(plain, view, "clear", call=plain.Render)
    T = bin_px()
    rows_full = (H + T - 1) // T
    for kind, k, world, cull in (("contiguous", 1, 3, False), ("interleaved", 1, 4, True), ("block", 2, 3, True), ("weighted", 300, 3, False)):
        acc = np.full_like(full, SENTINEL)
        covered = np.zeros(H, bool)
        for rank in range(world):
            rb = make_renderer(cloud, fb_format=fmt)
            lay = rb.set_band_plan(kind, rows_full, world, rank, k, band_cull=cull)
            rb.Sort(*view)
            rb.Render(*view, out=acc)                        # every band into the same image: only its rows
            covered |= np.isin(np.arange(H) // T, _capi.band_rows(*lay, rows_full=rows_full))
            rb.close()
        assert covered.all(), kind
        np.testing.assert_array_equal(acc, full, err_msg=kind)


@pytest.mark.parametrize("fmt", FORMATS)
def test_render_depth_colour_is_the_plain_frame_and_the_plane_is_the_fp32_one(fmt):
    import torch
    r, W, H, view = sorted_renderer("sparse", fmt)
    f32 = make_renderer(view_of("sparse")[0])
    f32.Sort(*view)
    _, zwant = f32.Render(*view, depth=True)
    assert zwant.dtype == np.float32 and (zwant < 1).any()
    plain = host_frame(r, view, "clear", call=r.Render)
    img, z = r.Render(*view, depth=True)
    np.testing.assert_array_equal(img, plain)
    assert z.dtype == np.float32 and (z.view(np.uint32) == zwant.view(np.uint32)).all()
    # device output, both planes pitched
    fb = torch.full((H, W + 24, 4), SENTINEL, dtype=torch.uint8, device="cuda:0")
    zb = torch.full((H, W + 8), -3.0, dtype=torch.float32, device="cuda:0")
    r.Render(*view, out_ptr=fb.data_ptr(), pitch_bytes=(W + 24) * 4, depth_ptr=zb.data_ptr(), depth_pitch_bytes=(W + 8) * 4)
    r.synchronize()
    got, gz = fb.cpu().numpy(), zb.cpu().numpy()
    np.testing.assert_array_equal(got[:, :W], plain)
    assert (got[:, W:] == SENTINEL).all() and (gz[:, W:] == -3.0).all()
    assert (gz[:, :W].view(np.uint32) == zwant.view(np.uint32)).all()


# ------------------------------------------------------------------------------------------------
# 4. the draw-order compositors
# ------------------------------------------------------------------------------------------------

def test_depth_test_and_target_emulation():
    cloud, W, H, view = view_of("sparse")
    f32 = make_renderer(cloud)
    f32.set_depth_test(24)
    f32.Sort(*view)
    x = host_frame(f32, view, "clear", call=f32.Render)
    xpre = host_frame(f32, view, "premultiplied", call=f32.Render)
    for fmt in FORMATS:
        r = make_renderer(cloud, fb_format=fmt)
        r.set_depth_test(24)
        r.Sort(*view)
        fb8_rule.check_frame(host_frame(r, view, "clear", call=r.Render), x, is_srgb(fmt), "depth test")
        pre = host_frame(r, view, "premultiplied", call=r.Render)
        fb8_rule.check_frame(pre, xpre, is_srgb(fmt), "depth test, premultiplied")
        dst = random_bytes(H, W, 61)
        got = host_frame(r, view, "load", dst, call=r.Render)
        fb8_rule.check_frame(got, host_frame(f32, view, "load", fb8_rule.decode(dst, is_srgb(fmt)), call=f32.Render), is_srgb(fmt), "depth test, load")
        untouched = xpre[..., 3] == 0
        assert untouched.any() and (got[untouched] == dst[untouched]).all()
    # MSPLAT_ROP_RGBA8 on an RGBA8 context: the reference's default window, bytes included -- the emulated values already are codes
    f32.set_target_mode("clear")
    for bits in (0, 24):
        f32.set_depth_test(bits)
        f32.set_target_emulation("rgba8")
        r = make_renderer(cloud, fb_format="rgba8")
        r.set_depth_test(bits)
        r.set_target_emulation("rgba8")
        r.Sort(*view)
        f32.Sort(*view)
        emu = host_frame(f32, view, "clear", call=f32.Render)
        codes = emu * np.float32(255.0)
        assert (codes == np.rint(codes)).all() and codes.min() >= 0 and codes.max() <= 255
        np.testing.assert_array_equal(host_frame(r, view, "clear", call=r.Render), codes.astype(np.uint8))
        f32.set_target_emulation(None)


@pytest.mark.parametrize("fmt", FORMATS)
def test_point_sprites(fmt):
    from splatapult_amd import PointCloud, PointRenderer
    pc = PointCloud(False)
    pc.InitDebugCloud()
    W, H = 320, 240
    cam = camera.pose((0.4, 0.4, 2.5))
    proj = camera.perspective(camera.FOVY, W / H)
    vp, nf = [0, 0, W, H], scenes.NF
    f32 = PointRenderer(device=0)
    assert f32.Init(pc, False)
    x = f32.Render(cam, proj, vp, nf)
    assert x[..., :3].max() > 0.5
    r = PointRenderer(device=0, fb_format=fmt)
    assert r.Init(pc, False)
    got = r.Render(cam, proj, vp, nf)
    fb8_rule.check_frame(got, x, is_srgb(fmt), "sprites")
    assert (got[..., 3] == 255).all() and got[..., :3].max() > 127


# ------------------------------------------------------------------------------------------------
# 5. exchange and group
# ------------------------------------------------------------------------------------------------

def test_band_exchange_moves_four_byte_pixels():
    import torch
    from splatapult_amd.dist import RcclComm, owned_rows
    comm = RcclComm(0, 1, 0)
    T = bin_px()
    dev = torch.device("cuda", 0)
    for fmt in FORMATS:
        r = make_renderer(scenes.synth_cloud(2000, 5), fb_format=fmt)
        W, H = 517, 293
        tiles_y = (H + T - 1) // T
        Hpad = tiles_y * T
        for Ws in (W, W + 24):                               # tight rows: one message per run; a window of a wider surface: row by row
            src = torch.randint(0, 256, (Hpad, Ws, 4), dtype=torch.uint8, device=dev)
            for kind, name, k in ((_capi.BANDS_CONTIGUOUS, "contiguous", 1), (_capi.BANDS_INTERLEAVED, "interleaved", 1),
                                  (_capi.BANDS_BLOCK_INTERLEAVED, "block", 2), (_capi.BANDS_ROOT_WEIGHTED, "weighted", 300)):
                for g in (0, 3, 7):
                    dst = torch.full_like(src, SENTINEL)
                    r.band_exchange(comm.handle, g, 8, 0, kind, k, dst.data_ptr(), Ws * 4, W, Hpad, loopback_src=src.data_ptr())
                    r.synchronize()
                    torch.cuda.synchronize()
                    rows = torch.from_numpy(np.isin(np.arange(Hpad) // T, owned_rows(name, tiles_y, 8, g, k))).to(dev)
                    want = torch.full_like(src, SENTINEL)
                    want[rows, :W] = src[rows, :W]
                    assert torch.equal(dst, want), (fmt, name, g, Ws)
        with pytest.raises(MsplatError) as e:                # the fp16 wire format is for RGBA32F targets
            r.band_exchange(comm.handle, 0, 8, 0, _capi.BANDS_CONTIGUOUS, 1, dst.data_ptr(), Ws * 4, W, Hpad, loopback_src=src.data_ptr(),
                            wire_fp16=True)
        assert "RGBA32F" in str(e.value)
        with pytest.raises(MsplatError):                     # a pitch that is no multiple of the 4-byte pixel
            r.band_exchange(comm.handle, 0, 8, 0, _capi.BANDS_CONTIGUOUS, 1, dst.data_ptr(), W * 4 + 2, W, Hpad, loopback_src=src.data_ptr())
        r.close()
    comm.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_group_reproduces_the_single_context_frame(fmt, monkeypatch):
    import torch
    cloud, W, H, view = view_of("sparse")
    cam, proj, vp, nf = view
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(*view)
    full = host_frame(r, view, "clear", call=r.Render)
    pre = host_frame(r, view, "premultiplied", call=r.Render)
    for devices, layout, k, exchanges in (([0], "contiguous", 1, ("peer", "copy", "rccl")), ([0, 0], "interleaved", 1, ("peer", "copy")),
                                          ([0, 0, 0], "block", 2, ("peer", "copy"))):
        for exchange in exchanges:                           # (RCCL refuses a device listed twice)
            if exchange == "copy":
                monkeypatch.setenv("MSPLAT_GROUP_EXCHANGE", "copy")
            else:
                monkeypatch.delenv("MSPLAT_GROUP_EXCHANGE", raising=False)
            g = SplatRendererGroup(devices, fb_format=fmt, layout=layout, block_rows=k)
            assert g.Init(cloud), g.last_error()
            if exchange == "rccl":
                g.set_exchange("rccl")                       # one device: accepted, nothing to exchange
            if len(devices) > 1:
                assert g.peer_store(1) == (exchange == "peer")
            g.Sort(*view)
            host = g.Render(*view)
            assert host.dtype == np.uint8
            np.testing.assert_array_equal(host, full)
            fb = torch.full((H, W + 24, 4), SENTINEL, dtype=torch.uint8, device="cuda:0")
            g.Render(cam, proj, vp, nf, out_ptr=fb.data_ptr(), pitch_bytes=(W + 24) * 4)
            g.synchronize()
            got = fb.cpu().numpy()
            np.testing.assert_array_equal(got[:, :W], full, err_msg="%s %s" % (devices, exchange))
            assert (got[:, W:] == SENTINEL).all()
            g.set_target_mode("premultiplied")
            np.testing.assert_array_equal(g.Render(*view), pre)
            g.close()


# ------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------

def test_refusals_say_why():
    import torch
    cloud, W, H, view = view_of("hard")
    cam, proj, vp, nf = view
    for fmt in FORMATS:
        r = make_renderer(cloud, fb_format=fmt)
        r.Sort(*view)
        fb = torch.zeros((H + 1, W + 8, 4), dtype=torch.uint8, device="cuda:0")
        for pitch in (W * 4 - 4, W * 4 + 2, W * 4 + 1, 4):
            with pytest.raises(MsplatError) as e:
                r.Render(cam, proj, vp, nf, out_ptr=fb.data_ptr(), pitch_bytes=pitch)
            assert e.value.code == _capi.ERR_INVALID_ARG
            assert "pitch %d" % pitch in r.last_error() and "4-byte pixels" in r.last_error() and str(W * 4) in r.last_error()
        r.synchronize()
        assert not fb.any()                                  # nothing was rendered
        for bad in (np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float16), np.zeros((H, W), np.uint32)):
            with pytest.raises(ValueError, match="uint8"):
                r.Render(cam, proj, vp, nf, out=bad)
    s = make_renderer(cloud, fb_format="srgb8")
    for rop in ("rgba8", "fp16"):
        with pytest.raises(MsplatError) as e:
            s.set_target_emulation(rop)
        assert e.value.code == _capi.ERR_UNSUPPORTED and "MSPLAT_FB_SRGB8_ALPHA8" in s.last_error() and "linear" in s.last_error().lower()
    s.set_target_emulation(None)                             # MSPLAT_ROP_NONE is no emulation
    s.Sort(*view)
    fb8_rule.check_frame(host_frame(s, view, "clear", call=s.Render), fp32_frame("hard", "clear"), True, "after the refusal")
    # everything else is allowed: the fp16 emulation into an RGBA8 target
    u = make_renderer(cloud, fb_format="rgba8")
    u.set_target_emulation("fp16")
    u.Sort(*view)
    f32 = make_renderer(cloud)
    f32.set_target_emulation("fp16")
    f32.Sort(*view)
    fb8_rule.check_frame(host_frame(u, view, "clear", call=u.Render), host_frame(f32, view, "clear", call=f32.Render), False, "fp16 emulation into rgba8")
