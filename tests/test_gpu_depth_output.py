"""GPU tests of msplat_render_depth: msplat_render plus a W x H float32 depth plane,

    depth = sum_i T_i w_i z_i + T * 1.0,      z_i = 0.5 ndc.z + 0.5 (window depth),  T = the transmittance where the walk stopped

-- the splats' expected window depth blended over GL's clear depth 1.0: MSPLAT_TARGET_LOAD's formula with colour z and dst = 1.
Checked here: identities that need no oracle (bit for bit), the unchanged oracle (tests/test_depth_output.py: depth_layers, pinned
there by a numpy restatement), every execution shape against the plain single-pass depth frame (bit for bit), and the refusals.

Tolerance against the oracle, derived as tests/test_gpu_target_mode.py derives LOAD's with |dst| = 1: both oracle frames (D_ref, the
splats coloured with z_w <= 1, and the white frame 1 - T_ref) carry the suite's TIGHT bound, and early termination leaves T below
t_eps instead of at its limit, so  |err| <= 2 TIGHT + t_eps;  check_image's frac / mean conditions are scaled the same way, and a
pixel above the bound has to be explained by the threshold-flip budgets of BOTH frames (budget_D + budget_white * 1)."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import MsplatError, _capi, camera
from tests import scenes
from tests.test_depth_output import depth_layers
from tests.test_gpu_parity import TIGHT, make_renderer
from tests.test_gpu_target_mode import SENTINEL, T_EPS, random_dst, render_host, scene, view_of

pytestmark = pytest.mark.gpu

MODES = ("clear", "load", "premultiplied")


def spread_view():
    """the "hard" scene between near / far planes that hug it: z_w of what the pixels see runs from the near cull (0.625) to the
    far plane instead of crowding towards 1 (chosen on the CPU with the oracle; test_depth_matches_the_oracle asserts the spread)"""
    cloud, W, H, _ = scene("hard")
    zn, zf = 5.02, 6.33
    return cloud, W, H, (camera.pose((0.0, 0.0, 5.75), 0.524, 0.037), camera.perspective(camera.FOVY, W / H, zn, zf), [0, 0, W, H], [zn, zf])


def case(name):
    return spread_view() if name == "spread" else view_of(name)


def render_depth_host(r, view, mode="clear", dst=None, plane=None):
    """one host-output Render with a depth plane in `mode`: (image, plane); dst: what the colour array holds before"""
    cam, proj, vp, nf = view
    r.set_target_mode(mode)
    out = None if dst is None else np.ascontiguousarray(dst).copy()
    img, z = r.Render(cam, proj, vp, nf, out=out, depth=True if plane is None else plane)
    assert z.dtype == np.float32 and z.shape == img.shape[:2]
    return img, z


def render_depth_device(r, view, mode, dst, pad=24, zpad=8, zfill=None):
    """one device-output Render into pitched targets: (image, plane), both paddings checked against the sentinel they start as;
    zfill: what the plane's pixels hold before (default: the sentinel too)"""
    import torch
    cam, proj, vp, nf = view
    H, W = dst.shape[:2]
    tdt = torch.float16 if dst.dtype == np.float16 else torch.float32
    fb = torch.full((H, W + pad, 4), SENTINEL, dtype=tdt, device="cuda:0")
    fb[:, :W] = torch.from_numpy(np.ascontiguousarray(dst)).to("cuda:0")
    zb = torch.full((H, W + zpad), SENTINEL, dtype=torch.float32, device="cuda:0")
    if zfill is not None:
        zb[:, :W] = torch.from_numpy(np.ascontiguousarray(zfill)).to("cuda:0")
    torch.cuda.synchronize()
    r.set_target_mode(mode)
    r.Render(cam, proj, vp, nf, out_ptr=fb.data_ptr(), pitch_bytes=(W + pad) * 4 * fb.element_size(), depth_ptr=zb.data_ptr(),
             depth_pitch_bytes=(W + zpad) * 4)
    r.synchronize()
    got, z = fb.cpu().numpy(), zb.cpu().numpy()
    assert (got[:, W:] == SENTINEL).all() and (z[:, W:] == SENTINEL).all(), "mode %s wrote into the padding of a pitched target" % mode
    return got[:, :W].copy(), z[:, :W].copy()


def junk_plane(H, W, seed):
    """what a caller's plane may hold: NaN, infinities, huge and negative values"""
    z = (np.random.default_rng(seed).standard_normal((H, W)) * 1e6).astype(np.float32)
    z[::2, ::3] = np.nan
    z[1::4, 1::5] = np.inf
    return z


def assert_is_a_plane(z):
    assert np.isfinite(z).all() and (z >= 0.0).all() and (z <= 1.0).all(), (np.nanmin(z), np.nanmax(z))


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
        plain = render_host(r, view, mode, dst)
        img, z = render_depth_host(r, view, mode, dst, plane=junk_plane(H, W, 6))
        np.testing.assert_array_equal(img, plain, err_msg="%s: the colour of a depth frame differs from msplat_render's" % mode)
        assert_is_a_plane(z)                                 # ... and nothing of the junk is left
        dimg, dz = render_depth_device(r, view, mode, dst, zfill=junk_plane(H, W, 7))
        np.testing.assert_array_equal(dimg, plain)
        np.testing.assert_array_equal(dz, z, err_msg="%s: device output differs from host output" % mode)
        np.testing.assert_array_equal(render_host(r, view, mode, dst), plain)      # and a plain Render after it is still the plain Render
        planes.append(z)
    np.testing.assert_array_equal(planes[1], planes[0], err_msg="the plane depends on the target mode")
    np.testing.assert_array_equal(planes[2], planes[0], err_msg="the plane depends on the target mode")
    pre = render_host(r, view, "premultiplied")
    empty = pre[..., 3] == 0
    assert (planes[0][empty] == 1.0).all(), "a pixel no splat reaches must read exactly 1.0"
    assert empty.mean() >= 0.01 or name != "sparse"           # the sparse scene has such pixels
    assert (planes[0] < 1.0).any()


# ------------------------------------------------------------------------------------------------
# 2. against the unchanged oracle
# ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_plane(name):
    cloud, W, H, (cam, proj, vp, nf) = case(name)
    ref = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=16, want_image=False, want_splats=True)
    L = dict(depth_layers(ref["splats"], W, H, nthreads=16))
    L["V"] = ref["V"]
    L["visible"] = ref["splats"]["reject"] == 0
    return L


def check_plane(z, L, t_eps, max_abs=TIGHT, mean_abs=1e-4, frac=0.999, tol=1e-4):
    """z against D_ref + T_ref: check_over of tests/test_gpu_target_mode.py with |dst| = 1"""
    err = np.abs(z.astype(np.float64) - L["plane"])
    print("check_plane: max |err| %.3g, mean %.3g, t_eps %g" % (err.max(), err.mean(), t_eps))
    within = (err <= tol * 2.0 + t_eps).mean()
    assert within >= frac, "only %.5f of values within the scaled %g (max %.3g)" % (within, tol, err.max())
    assert err.mean() <= mean_abs * 2.0 + t_eps, "mean |err| %.3g" % err.mean()
    bound = max_abs * 2.0 + t_eps
    over = err > bound
    if over.any():
        bad = over & (err > bound + L["bud_d"] + L["bud_w"])
        assert not bad.any(), "%d value(s) above the bound not explained by a w ~ 1/256 flip (max %.3g)" % (bad.sum(), err[bad].max())
        print("check_plane: %d value(s) above the bound, all within the two frames' threshold-flip budgets" % over.sum())


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
    img, z = render_depth_host(r, view)
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
            ia, za = render_depth_host(a, view, mode, dst)
            ib, zb = render_depth_host(b, view, mode, dst, plane=junk_plane(H, W, 22))
            np.testing.assert_array_equal(ib, ia)
            np.testing.assert_array_equal(zb, za, err_msg="%s %s share %g" % (name, mode, share))
            np.testing.assert_array_equal(ia, render_host(a, view, mode, dst))
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
        ia, za = render_depth_device(a, view, mode, dst)
        ib, zb = render_depth_device(b, view, mode, dst)
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
    img, z = render_depth_host(r, view, plane=junk_plane(H, W, 31))
    np.testing.assert_array_equal(img, plain)
    assert_is_a_plane(z)
    dimg, dz = render_depth_device(r, view, "clear", np.zeros((H, W, 4), np.float32))
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
    for got in (render_depth_host(r, view, plane=junk_plane(H, W, 32)), render_depth_device(r, view, "clear", random_dst(H, W, 33))):
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
        want_img, want_z = render_depth_host(plain, view, mode, dst)
        sentinel = np.full((H, W), SENTINEL, np.float32)
        for img, z in (render_depth_host(band, view, mode, dst, plane=sentinel.copy()), render_depth_device(band, view, mode, dst)):
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
        img, z = render_depth_host(one, view)
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
    img, z = render_depth_host(r, view, plane=junk_plane(H, W, 71))      # the context's first render
    st = r.stats()
    assert st["pairs"] > (1 << 22) and st["pair_capacity"] >= st["pairs"], st      # it did overflow, and grew
    calm = make_renderer(cloud, pair_capacity=int(st["pairs"]) + 4096)               # never overflows
    calm.Sort(*view)
    cimg, cz = render_depth_host(calm, view)
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
    want_z = render_depth_host(r, view)[1]
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
        img, z = render_depth_host(r, view)
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
