"""GPU tests of msplat_render_depth: msplat_render plus a W x H float32 depth plane,

    depth = sum_i T_i w_i z_i + T * 1.0,      z_i = 0.5 ndc.z + 0.5 (window depth),  T = the transmittance where the walk stopped

-- the splats' expected window depth blended over GL's clear depth 1.0: MSPLAT_TARGET_LOAD's formula with colour z and dst = 1.
Checked here: identities that need no oracle (bit for bit), the unchanged oracle (tests/render_cases.depth_layers, pinned by a
numpy restatement in tests/test_depth_output.py), every execution shape against the plain single-pass depth frame (bit for bit),
and the refusals.

Tolerance against the oracle (tests/checks.check_plane), derived as tests/test_gpu_target_mode.py derives LOAD's with |dst| = 1:
both oracle frames (D_ref, the splats coloured with z_w <= 1, and the white frame 1 - T_ref) carry the suite's TIGHT bound, and
early termination leaves T below t_eps instead of at its limit, so  |err| <= 2 TIGHT + t_eps;  check_image's frac / mean
conditions are scaled the same way, and a pixel above the bound has to be explained by the threshold-flip budgets of BOTH frames
(budget_D + budget_white * 1)."""
import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import MsplatError, _capi
from tests import scenes
from tests.checks import T_EPS, TIGHT, assert_is_a_plane, check_plane
from tests.gpu_harness import SENTINEL, device_frame, host_frame, make_renderer
from tests.render_cases import MODES, case, depth_layers, junk_plane, oracle_plane, random_dst, scene, view_of

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# 1. identities that need no oracle
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["sparse", "hard", "dense"])
def test_identities(name, fmt):
    cloud, W, H, view = view_of(name)
    dt = np.float16 if fmt == "fp16" else np.float32
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(*view)
    dst = random_dst(H, W, 5, dt)
    planes = []
    for mode in MODES:
        plain = host_frame(r, view, mode, dst, call=r.Render)
        img, z = host_frame(r, view, mode, dst, call=r.Render, depth=junk_plane(H, W, 6))
        np.testing.assert_array_equal(img, plain, err_msg="%s: the colour of a depth frame differs from msplat_render's" % mode)
        assert_is_a_plane(z)                                 # ... and nothing of the junk is left
        dimg, dz = device_frame(r, view, mode, dst, call=r.Render, depth=True, dpad=8, zfill=junk_plane(H, W, 7))
        np.testing.assert_array_equal(dimg, plain)
        np.testing.assert_array_equal(dz, z, err_msg="%s: device output differs from host output" % mode)
        np.testing.assert_array_equal(host_frame(r, view, mode, dst, call=r.Render), plain)      # and a plain Render after it is still the plain Render
        planes.append(z)
    np.testing.assert_array_equal(planes[1], planes[0], err_msg="the plane depends on the target mode")
    np.testing.assert_array_equal(planes[2], planes[0], err_msg="the plane depends on the target mode")
    pre = host_frame(r, view, "premultiplied", call=r.Render)
    empty = pre[..., 3] == 0
    assert (planes[0][empty] == 1.0).all(), "a pixel no splat reaches must read exactly 1.0"
    assert empty.mean() >= 0.01 or name != "sparse"           # the sparse scene has such pixels
    assert (planes[0] < 1.0).any()


# ------------------------------------------------------------------------------------------------
# 2. against the unchanged oracle
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t_eps", [-1.0, 0.0])
@pytest.mark.parametrize("name", ["sparse", "dense", "spread"])
def test_depth_matches_the_oracle(name, t_eps):
    cloud, W, H, view = case(name)
    L = oracle_plane(name)
    zw = L["zw"][L["visible"]]
    assert zw.size > 0 and zw.min() >= 0.0 and zw.max() <= 1.0           # the window depth of what is drawn
    covered = L["cover"] > 0.5
    spread = L["plane"][covered].std()
    print("%s: z_w of the drawn splats in [%.4f, %.4f], std of the reference plane over covered pixels %.4f" % (name, zw.min(), zw.max(), spread))
    if name == "spread":
        assert covered.mean() > 0.5 and spread >= 20 * TIGHT, spread       # a condition on the input: z_w does not crowd towards 1
    r = make_renderer(cloud, t_epsilon=t_eps)
    r.Sort(*view)
    assert r.sort_count() == L["V"]
    img, z = host_frame(r, view, "clear", call=r.Render, depth=True)
    assert_is_a_plane(z)
    check_plane(z, L, T_EPS if t_eps < 0 else t_eps)
    assert (z[L["cover"] == 0.0] == 1.0).all()
    if name == "dense":
        assert (img[..., 3] == 1).all() and (L["T"] < T_EPS).mean() > 0.5       # the early exit was taken: saturated pixels


# ------------------------------------------------------------------------------------------------
# 3. execution shapes, bit for bit against the plain single-pass depth frame
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("share", [1.0 / 64.0, 0.3, 1.0])
def test_two_pass_frames_equal_the_single_pass(share):
    """the cases of test_two_pass_frames_are_bit_identical_to_single_pass: a dense cloud from outside (saturated centre, unfinished
    rim: tiles carried through the depth state plane), from inside, and a sparse one (pass 2 redoes nearly everything)"""
    cases = [("dense", dict(z=5.0, yaw=0.3)), ("dense", dict(z=0.8, yaw=2.0)), ("sparse", dict(z=7.0, yaw=0.0))]
    for name, over in cases:
        cloud, W, H, view = view_of(name, **over)
        a = make_renderer(cloud, two_pass=_capi.TWO_PASS_OFF)
        b = make_renderer(cloud, two_pass=_capi.TWO_PASS_ON)
        b.two_pass_state(share)
        a.Sort(*view); b.Sort(*view)
        dst = random_dst(H, W, 21)
        for mode in ("clear", "load"):
            ia, za = host_frame(a, view, mode, dst, call=a.Render, depth=True)
            ib, zb = host_frame(b, view, mode, dst, call=b.Render, depth=junk_plane(H, W, 22))
            np.testing.assert_array_equal(ib, ia)
            np.testing.assert_array_equal(zb, za, err_msg="%s %s share %g" % (name, mode, share))
            np.testing.assert_array_equal(ia, host_frame(a, view, mode, dst, call=a.Render))
        assert b.two_pass_state(share)[0] == 2 and a.two_pass_state()[0] == 0
        info = b.two_pass_info()
        print("two-pass, %s share %g: %s" % (name, share, info))


def test_fp16_two_pass_device_output():
    cloud, W, H, view = view_of("dense", z=5.0, yaw=0.3)
    a = make_renderer(cloud, fb_format="fp16", two_pass=_capi.TWO_PASS_OFF)
    b = make_renderer(cloud, fb_format="fp16", two_pass=_capi.TWO_PASS_ON)
    b.two_pass_state(0.2)
    a.Sort(*view); b.Sort(*view)
    dst = random_dst(H, W, 23, np.float16)
    for mode in MODES:
        ia, za = device_frame(a, view, mode, dst, call=a.Render, depth=True, dpad=8)
        ib, zb = device_frame(b, view, mode, dst, call=b.Render, depth=True, dpad=8)
        np.testing.assert_array_equal(ib, ia)
        np.testing.assert_array_equal(zb, za)
    assert b.two_pass_state(0.2)[0] == 3


def test_a_viewport_smaller_than_a_bin():
    cloud, _, _, _ = scene("sparse")
    W, H = 17, 9
    view = cam, proj, vp, nf = scenes.default_view(W, H, z=7.0)
    r = make_renderer(cloud)
    r.Sort(*view)
    plain = r.Render(*view)
    img, z = host_frame(r, view, "clear", call=r.Render, depth=junk_plane(H, W, 31))
    np.testing.assert_array_equal(img, plain)
    assert_is_a_plane(z)
    dimg, dz = device_frame(r, view, "clear", np.zeros((H, W, 4), np.float32), call=r.Render, depth=True, dpad=8)
    np.testing.assert_array_equal(dimg, plain)
    np.testing.assert_array_equal(dz, z)
    ref = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=4, want_image=False, want_splats=True)
    check_plane(z, depth_layers(ref["splats"], W, H, nthreads=4), T_EPS)


def test_a_frame_with_nothing_visible_is_all_ones():
    cloud, W, H, _ = scene("sparse")
    view = scenes.default_view(W, H, z=7.0, yaw=np.pi)          # looking away from the cloud
    r = make_renderer(cloud)
    r.Sort(*view)
    assert r.sort_count() == 0
    plain = r.Render(*view)
    for got in (host_frame(r, view, "clear", call=r.Render, depth=junk_plane(H, W, 32)),
                device_frame(r, view, "clear", random_dst(H, W, 33), call=r.Render, depth=True, dpad=8)):
        np.testing.assert_array_equal(got[0], plain)
        assert (got[1] == 1.0).all()


def test_a_banded_context_writes_its_own_rows_only():
    cloud, W, H, view = view_of("sparse")
    T = _capi.lib().msplat_tile_size()
    rows_full = (H + T - 1) // T
    first, count, block, stride = 1, 0, 2, 5               # blocks of two bin rows: 1-2, 6-7, ...
    owned_bins = _capi.band_rows(first, count, block, stride, rows_full)
    assert 1 < len(owned_bins) < rows_full
    owned = np.isin(np.arange(H) // T, owned_bins)
    plain = make_renderer(cloud)
    plain.Sort(*view)
    band = make_renderer(cloud)
    band.set_band_layout(first, count, block, stride, band_cull=True)
    band.Sort(*view)
    dst = random_dst(H, W, 51)
    for mode in ("clear", "load"):
        want_img, want_z = host_frame(plain, view, mode, dst, call=plain.Render, depth=True)
        sentinel = np.full((H, W), SENTINEL, np.float32)
        for img, z in (host_frame(band, view, mode, dst, call=band.Render, depth=sentinel.copy()),
                       device_frame(band, view, mode, dst, call=band.Render, depth=True, dpad=8)):
            np.testing.assert_array_equal(img[owned], want_img[owned])
            np.testing.assert_array_equal(z[owned], want_z[owned])
            assert (z[~owned] == SENTINEL).all(), "mode %s: the depth plane's rows of another band were touched" % mode
            assert img[~owned].tobytes() == dst[~owned].tobytes()


@pytest.mark.parametrize("shape", ["four_in_flight", "async_submit"])
def test_frames_in_flight_and_queued_calls_equal_one_context(shape):
    import torch
    cloud, W, H, _ = scene("sparse")
    views = [scenes.default_view(W, H, z=7.0, yaw=0.3 * k) for k in range(6)]
    one = make_renderer(cloud)
    fly = make_renderer(cloud, frames_in_flight=4) if shape == "four_in_flight" else make_renderer(cloud, async_submit=True)
    fbs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in views]
    zbs = [torch.full((H, W), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in views]
    torch.cuda.synchronize()
    for k, (cam, proj, vp, nf) in enumerate(views):
        fly.Sort(cam, proj, vp, nf)
        fly.Render(cam, proj, vp, nf, out_ptr=fbs[k].data_ptr(), pitch_bytes=W * 16, depth_ptr=zbs[k].data_ptr())      # tight plane
    fly.synchronize()
    for k, view in enumerate(views):
        one.Sort(*view)
        img, z = host_frame(one, view, "clear", call=one.Render, depth=True)
        np.testing.assert_array_equal(fbs[k].cpu().numpy(), img, err_msg="frame %d" % k)
        np.testing.assert_array_equal(zbs[k].cpu().numpy(), z, err_msg="frame %d" % k)


def test_host_output_survives_a_pair_buffer_overflow():
    """the scene of test_host_output_load_render_survives_a_pair_buffer_overflow: the context's first render overflows the initial
    capacity, grows the buffer and renders again -- the plane handed back is the complete frame's, all of it"""
    cloud = scenes.synth_cloud(12000, 123, log_scale_mean=-0.5, pos_sigma=1.0)      # ~10 M pairs at 1024 x 1024, capacity starts at 4 M
    W = H = 1024
    view = scenes.default_view(W, H, z=4.0)
    r = make_renderer(cloud)                                # automatic capacity
    r.Sort(*view)
    img, z = host_frame(r, view, "clear", call=r.Render, depth=junk_plane(H, W, 71))      # the context's first render
    st = r.stats()
    assert st["pairs"] > (1 << 22) and st["pair_capacity"] >= st["pairs"], st      # it did overflow, and grew
    calm = make_renderer(cloud, pair_capacity=int(st["pairs"]) + 4096)               # never overflows
    calm.Sort(*view)
    cimg, cz = host_frame(calm, view, "clear", call=calm.Render, depth=True)
    np.testing.assert_array_equal(img, cimg)
    np.testing.assert_array_equal(z, cz)
    assert_is_a_plane(z)


# ------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------

def test_refused_combinations_say_why_and_leave_the_context_usable():
    cloud, W, H, view = view_of("hard")
    cam, proj, vp, nf = view
    r = make_renderer(cloud)
    r.Sort(*view)
    plain = r.Render(*view)
    want_z = host_frame(r, view, "clear", call=r.Render, depth=True)[1]
    switches = [("msplat_set_depth_test", lambda on: r.set_depth_test(24 if on else 0)),
                ("msplat_set_target_emulation", lambda on: r.set_target_emulation("rgba8" if on else None)),
                ("probe", lambda on: r.set_tile_probe(on))]
    for word, switch in switches:
        switch(True)
        z = np.full((H, W), SENTINEL, np.float32)
        with pytest.raises(MsplatError) as e:
            r.Render(*view, depth=z)
        assert e.value.code == _capi.ERR_UNSUPPORTED and word in r.last_error() and "msplat_render_depth" in r.last_error()
        assert (z == SENTINEL).all()
        r.Render(*view)                                     # the plain Render of that configuration still works
        switch(False)
        img, z = host_frame(r, view, "clear", call=r.Render, depth=True)
        np.testing.assert_array_equal(img, plain)
        np.testing.assert_array_equal(z, want_z)
    # a bad pitch
    import torch
    fb = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    zb = torch.zeros((H, W + 8), dtype=torch.float32, device="cuda:0")
    for pitch in (4 * W - 4, 4 * W + 2, 3):
        with pytest.raises(MsplatError) as e:
            r.Render(*view, out_ptr=fb.data_ptr(), pitch_bytes=W * 16, depth_ptr=zb.data_ptr(), depth_pitch_bytes=pitch)
        assert e.value.code == _capi.ERR_INVALID_ARG and "pitch" in r.last_error() and "msplat_render_depth" in r.last_error()
    r.Render(*view, out_ptr=fb.data_ptr(), pitch_bytes=W * 16, depth_ptr=zb.data_ptr(), depth_pitch_bytes=4 * W + 32)
    r.synchronize()
    np.testing.assert_array_equal(zb.cpu().numpy()[:, :W], want_z)
    # the plane lives where the colour does
    with pytest.raises(ValueError):
        r.Render(*view, out_ptr=fb.data_ptr(), pitch_bytes=W * 16, depth=True)
    with pytest.raises(ValueError):
        r.Render(*view, depth_ptr=zb.data_ptr())


def test_point_clouds_have_no_depth_output():
    pts = np.random.default_rng(81).uniform(-1, 1, (500, 8)).astype(np.float32)
    pts[:, 3] = 1.0
    pts[:, 4:] = np.abs(pts[:, 4:])
    L = _capi.lib()
    cfg = _capi.Config()
    cfg.struct_size = _capi.C.sizeof(_capi.Config)
    cfg.t_epsilon = -1.0
    h = _capi.C.c_void_p()
    assert L.msplat_create(_capi.C.byref(h), _capi.C.byref(cfg)) == _capi.OK
    assert L.msplat_upload_points(h, pts.ctypes.data, pts.shape[0], 32, 0, 16) == _capi.OK
    W, H = 64, 48
    fp = _capi.C.POINTER(_capi.C.c_float)
    a = [np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)) for x in scenes.default_view(W, H, z=4.0)]
    p = [x.ctypes.data_as(fp) for x in a]
    assert L.msplat_sort(h, *p) == _capi.OK
    img, z = np.zeros((H, W, 4), np.float32), np.full((H, W), SENTINEL, np.float32)
    assert L.msplat_render_depth(h, *p, img.ctypes.data, 0, z.ctypes.data, 0, 0) == _capi.ERR_UNSUPPORTED
    assert b"point cloud" in L.msplat_last_error(h) and (z == SENTINEL).all()
    assert L.msplat_render_depth(h, *p, img.ctypes.data, 0, None, 0, 0) == _capi.OK            # depth == NULL is msplat_render
    L.msplat_destroy(h)


def test_the_group_refuses_the_depth_argument():
    from splatapult_amd import SplatRendererGroup
    cloud, W, H, view = view_of("hard")
    g = SplatRendererGroup([0])
    assert g.Init(cloud), g.last_error()
    g.Sort(*view)
    want = g.Render(*view)
    with pytest.raises(MsplatError) as e:
        g.Render(*view, depth=True)
    assert e.value.code == _capi.ERR_UNSUPPORTED
    np.testing.assert_array_equal(g.Render(*view), want)
    g.close()
