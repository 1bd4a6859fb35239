"""GPU tests of msplat_set_target_mode: the splat frame as a layer (PREMULTIPLIED) and blended over the target's contents (LOAD).

Per pixel the compositor ends with C (premultiplied colour) and T (transmittance where the walk stopped).  CLEAR stores (C, 1),
PREMULTIPLIED (C, 1 - T), LOAD (fma(T, dst.rgb, C), fma(T, dst.a - 1, 1)).  Checked here:
  identities that need no oracle (bit for bit), untouched pixels, the unchanged oracle (C_ref + T_ref dst with
  T_ref = 1 - white frame: the blend is linear in colour), every execution shape against the plain one (bit for bit), the
  draw-order (depth-test) compositor, a host-output frame whose pair buffer has to grow, and the refused combinations.

Tolerance against the oracle, derived: both oracle frames (C_ref and the white frame 1 - T_ref) carry the suite's TIGHT bound
(tests/checks.py), early termination leaves T below t_eps instead of at its limit, and the alpha channel is the same
blend with "colour" 1 - T, so for all four channels  |err| <= TIGHT (1 + |dst|) + t_eps |dst|;  check_image's frac / mean
conditions are scaled the same way, and a pixel above the bound has to be explained by the threshold-flip budgets of BOTH frames
(budget_C + budget_white |dst|), as check_image does for one: tests/checks.check_over.  The oracle recipe is
tests/render_cases.oracle_layers."""
import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import MsplatError, SplatRenderer, SplatRendererGroup, _capi, camera
from tests import scenes
from tests.checks import T_EPS, TIGHT, check_image, check_over
from tests.gpu_harness import device_frame, host_frame, make_renderer
from tests.render_cases import const_dst, oracle_layers, random_dst, scene, view_of

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------
# 1. identities that need no oracle
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", ["host_fp32", "host_fp16", "device_pitched_fp32", "device_pitched_fp16"])
@pytest.mark.parametrize("name", ["sparse", "hard", "dense"])
def test_identities_between_the_modes(name, target):
    cloud, W, H, view = view_of(name)
    fmt = "fp16" if target.endswith("fp16") else "fp32"
    dt = np.float16 if fmt == "fp16" else np.float32
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(*view)
    zeros, opaque = const_dst(H, W, (0, 0, 0, 0), dt), const_dst(H, W, (0, 0, 0, 1), dt)
    if target.startswith("host"):
        run = lambda mode, dst: host_frame(r, view, mode, dst, call=r.Render)
    else:
        run = lambda mode, dst: device_frame(r, view, mode, dst, call=r.Render)         # (asserts that the padding keeps its bytes)
    junk = random_dst(H, W, 5, dt)                     # CLEAR and PREMULTIPLIED read nothing: what the target held does not matter
    clear = run("clear", junk)
    pre = run("premultiplied", junk)
    assert (clear[..., 3] == 1).all()
    np.testing.assert_array_equal(pre[..., :3], clear[..., :3])
    assert (pre[..., 3] >= 0).all() and (pre[..., 3] <= 1).all()
    # coverage really is written (the dense view saturates every pixel: T < 2^-14, which half rounds to alpha == 1)
    assert (pre[..., 3] < 1).any() or (name == "dense" and fmt == "fp16")
    np.testing.assert_array_equal(run("load", zeros), pre)
    np.testing.assert_array_equal(run("load", opaque), clear)
    assert r.target_mode() == "load"
    np.testing.assert_array_equal(run("clear", junk), clear)       # and back


# ------------------------------------------------------------------------------------------------
# 2. / 3. against the unchanged oracle
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t_eps", [-1.0, 0.0])
@pytest.mark.parametrize("name", ["sparse", "dense"])
def test_load_and_premultiplied_match_the_oracle(name, t_eps):
    cloud, W, H, view = view_of(name)
    L = oracle_layers(name)
    r = make_renderer(cloud, t_epsilon=t_eps)
    r.Sort(*view)
    assert r.sort_count() == L["V"]
    eps = T_EPS if t_eps < 0 else t_eps
    dst = random_dst(H, W, 11)
    check_over(host_frame(r, view, "load", dst, call=r.Render), L, dst, eps)
    zero = np.zeros((H, W, 4), np.float32)
    pre = host_frame(r, view, "premultiplied", call=r.Render)
    check_over(pre, L, zero, eps)                            # |err| <= TIGHT: alpha against 1 - T_ref, colour against C_ref
    if name == "dense":
        assert (pre[..., 3] > 1.0 - 2.0 * T_EPS).mean() > 0.5      # the early exit was taken: saturated pixels


def test_load_leaves_pixels_no_splat_reaches_bit_for_bit():
    cloud, W, H, view = view_of("sparse")
    L = oracle_layers("sparse")
    untouched = L["cover"][..., 0] == 0.0                   # the oracle's white frame: not one fragment passed the discard there
    assert untouched.mean() >= 0.01, untouched.mean()       # (checked on the CPU: the sparse scene has such pixels)
    r = make_renderer(cloud)
    r.Sort(*view)
    # finite, both signs, alpha included and on both sides of 0.5 (dst.a - 1 rounds below it)
    dst = (np.random.default_rng(12).standard_normal((H, W, 4)) * 1.5).astype(np.float32)
    # ... and what arithmetic would not hand through: -0, denormals (the compositor's waves flush them), the largest finite value
    odd = np.array([-0.0, 1e-40, -3e-39, np.finfo(np.float32).max, np.finfo(np.float32).tiny], np.float32)
    dst[::3, ::2] = odd[np.random.default_rng(13).integers(0, odd.size, dst[::3, ::2].shape)]
    assert (untouched[::3, ::2]).any()
    for got in (host_frame(r, view, "load", dst, call=r.Render), device_frame(r, view, "load", dst, call=r.Render)):
        seen = untouched & (got.view(np.uint32) == dst.view(np.uint32)).all(axis=-1)
        assert seen.sum() == untouched.sum(), "%d untouched pixel(s) changed" % (untouched.sum() - seen.sum())
        assert seen.mean() >= 0.01
        assert (got.view(np.uint32) != dst.view(np.uint32)).any()          # and the others were blended


# ------------------------------------------------------------------------------------------------
# 4. bit-identical across execution shapes
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("share", [1.0 / 64.0, 0.3, 1.0])
def test_two_pass_frames_equal_the_single_pass(share):
    """tiles pass 1 finishes are stored (and, in LOAD, read) by pass 1, the carried ones by pass 2: every pixel once"""
    cloud, W, H, view = view_of("dense", z=5.0, yaw=0.3)          # from outside: saturated centre, unfinished rim
    a = make_renderer(cloud, two_pass=_capi.TWO_PASS_OFF)
    b = make_renderer(cloud, two_pass=_capi.TWO_PASS_ON)
    b.two_pass_state(share)
    a.Sort(*view); b.Sort(*view)
    dst = random_dst(H, W, 21)
    for mode in ("load", "premultiplied"):
        np.testing.assert_array_equal(host_frame(b, view, mode, dst, call=b.Render), host_frame(a, view, mode, dst, call=a.Render))
    assert b.two_pass_state(share)[0] == 2 and a.two_pass_state()[0] == 0
    print("two-pass, share %g: %s" % (share, b.two_pass_info()))


@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
def test_render_stereo_equals_two_renders(fmt):
    import torch
    cloud, W, H, _ = scene("hard")
    dt, tdt = (np.float16, torch.float16) if fmt == "fp16" else (np.float32, torch.float32)
    proj = camera.perspective(camera.FOVY, W / H)
    vp, nf = [0, 0, W, H], scenes.NF
    cams = [camera.pose((-0.1, 0.0, 6.0), 0.65), camera.pose((0.1, 0.0, 6.0), 0.75)]
    dsts = [random_dst(H, W, 31, dt), random_dst(H, W, 32, dt)]
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(cams[0], proj, vp, nf)
    for mode in ("load", "premultiplied"):
        want = [device_frame(r, (cams[k], proj, vp, nf), mode, dsts[k], call=r.Render, pad=0) for k in range(2)]
        fbs = [torch.from_numpy(dsts[k].copy()).to("cuda:0") for k in range(2)]
        torch.cuda.synchronize()
        r.RenderStereo(cams, [proj, proj], vp, nf, out_ptrs=[f.data_ptr() for f in fbs], pitch_bytes=W * 4 * fbs[0].element_size())
        r.synchronize()
        for k in range(2):
            np.testing.assert_array_equal(fbs[k].cpu().numpy(), want[k])
        assert not np.array_equal(want[0], want[1])


def test_host_output_stereo_goes_view_by_view_over_each_array():
    """msplat_render_stereo with host targets is two renders, each over its own array; the Python RenderStereo has no out= to take
    the destinations and says so"""
    import ctypes as C
    cloud, W, H, _ = scene("hard")
    proj = camera.perspective(camera.FOVY, W / H)
    vp, nf = [0, 0, W, H], scenes.NF
    cams = [camera.pose((-0.1, 0.0, 6.0), 0.65), camera.pose((0.1, 0.0, 6.0), 0.75)]
    dsts = [random_dst(H, W, 33), random_dst(H, W, 34)]
    r = make_renderer(cloud)
    r.Sort(cams[0], proj, vp, nf)
    want = [host_frame(r, (cams[k], proj, vp, nf), "load", dsts[k], call=r.Render) for k in range(2)]
    with pytest.raises(ValueError):
        r.RenderStereo(cams, [proj, proj], vp, nf)
    fp = C.POINTER(C.c_float)
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))
    a = [f(cams[0]), f(proj), f(cams[1]), f(proj), f(vp), f(nf)]
    outs = [d.copy() for d in dsts]
    rc = _capi.lib().msplat_render_stereo(r._ctx, *[x.ctypes.data_as(fp) for x in a], outs[0].ctypes.data, outs[1].ctypes.data, 0, 0)
    assert rc == _capi.OK, r.last_error()
    for k in range(2):
        np.testing.assert_array_equal(outs[k], want[k])


def test_four_frames_in_flight_equal_one_context():
    import torch
    cloud, W, H, _ = scene("sparse")
    views = [scenes.default_view(W, H, z=7.0, yaw=0.3 * k) for k in range(6)]
    dsts = [random_dst(H, W, 40 + k) for k in range(len(views))]
    one = make_renderer(cloud)
    fly = make_renderer(cloud, frames_in_flight=4)
    for mode in ("load", "premultiplied"):
        fly.set_target_mode(mode)                            # every context of the rotation
        fbs = [torch.from_numpy(d.copy()).to("cuda:0") for d in dsts]
        torch.cuda.synchronize()
        for k, (cam, proj, vp, nf) in enumerate(views):
            fly.Sort(cam, proj, vp, nf)
            fly.Render(cam, proj, vp, nf, out_ptr=fbs[k].data_ptr(), pitch_bytes=W * 16)
        fly.synchronize()
        for k, view in enumerate(views):
            one.Sort(*view)
            np.testing.assert_array_equal(fbs[k].cpu().numpy(), host_frame(one, view, mode, dsts[k], call=one.Render), err_msg="%s frame %d" % (mode, k))


def test_a_banded_context_reads_and_writes_its_own_rows_only():
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
    band.set_band_layout(first, count, block, stride)
    band.Sort(*view)
    dst = random_dst(H, W, 51)
    for mode in ("load", "premultiplied"):
        want = host_frame(plain, view, mode, dst, call=plain.Render)
        for got in (host_frame(band, view, mode, dst, call=band.Render), device_frame(band, view, mode, dst, call=band.Render)):
            np.testing.assert_array_equal(got[owned], want[owned])
            assert got[~owned].tobytes() == dst[~owned].tobytes(), "mode %s touched rows of another band" % mode


def test_a_one_device_group_takes_premultiplied_and_refuses_load():
    cloud, W, H, view = view_of("hard")
    r = make_renderer(cloud)
    r.Sort(*view)
    want = host_frame(r, view, "premultiplied", call=r.Render)
    g = SplatRendererGroup([0])
    assert g.Init(cloud), g.last_error()
    g.set_target_mode("premultiplied")
    g.Sort(*view)
    np.testing.assert_array_equal(g.Render(*view), want)
    with pytest.raises(MsplatError) as e:
        g.set_target_mode("load")
    assert e.value.code == _capi.ERR_UNSUPPORTED and "MSPLAT_TARGET_LOAD" in g.last_error()
    np.testing.assert_array_equal(g.Render(*view), want)               # the refused call changed nothing
    g.set_target_mode("clear")
    assert (g.Render(*view)[..., 3] == 1).all()
    g.close()


# ------------------------------------------------------------------------------------------------
# 5. the draw-order compositor (msplat_set_depth_test)
# ------------------------------------------------------------------------------------------------

def test_depth_test_path_blends_over_the_target():
    """the scene and the bound of test_depth_test_emulation_matches_oracle (check_image's defaults, on the colour channels)"""
    cloud = scenes.synth_cloud(20000, 101, log_scale_mean=-3.0)
    W, H = 640, 360
    view = cam, proj, vp, nf = scenes.default_view(W, H, yaw=0.2)
    r = make_renderer(cloud)
    r.set_depth_test(24)
    r.Sort(*view)
    ref = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=8, want_image=False, want_splats=True)
    C_ref = orc.composite_depth(ref["splats"], W, H, 24, nthreads=8).astype(np.float64)
    white = ref["splats"].copy()
    white["rgb"] = 1.0
    cover = orc.composite_depth(white, W, H, 24, nthreads=8)[..., 0].astype(np.float64)
    dst = random_dst(H, W, 61)
    want = C_ref[..., :3] + (1.0 - cover)[..., None] * dst[..., :3].astype(np.float64)

    def check(img, want_rgb, want_a):
        err = np.abs(img[..., :3].astype(np.float64) - want_rgb)
        print("depth path: max |err| %.3g, mean %.3g" % (err.max(), err.mean()))
        opaque = np.concatenate([img[..., :3], np.ones_like(img[..., 3:])], axis=-1)        # check_image wants alpha == 1; alpha is checked below
        check_image(opaque, np.concatenate([want_rgb, np.ones_like(want_rgb[..., :1])], axis=-1))
        assert np.abs(img[..., 3].astype(np.float64) - want_a).max() <= TIGHT

    check(host_frame(r, view, "load", dst, call=r.Render), want, cover + (1.0 - cover) * dst[..., 3].astype(np.float64))
    pre = host_frame(r, view, "premultiplied", call=r.Render)
    check(pre, C_ref[..., :3], cover)
    clear = host_frame(r, view, "clear", call=r.Render)
    np.testing.assert_array_equal(pre[..., :3], clear[..., :3])
    assert (clear[..., 3] == 1).all()
    np.testing.assert_array_equal(host_frame(r, view, "load", const_dst(H, W, (0, 0, 0, 0)), call=r.Render), pre)
    # an opaque target stays exactly opaque (w + fl(1 - w) rounds to 1 for every w in [0, 1]), the colours are CLEAR's
    np.testing.assert_array_equal(host_frame(r, view, "load", const_dst(H, W, (0, 0, 0, 1)), call=r.Render), clear)


# ------------------------------------------------------------------------------------------------
# 6. host output: the pair buffer grows in the middle of a LOAD render
# ------------------------------------------------------------------------------------------------

def test_host_output_load_render_survives_a_pair_buffer_overflow():
    """LOAD is not idempotent: the retry after the overflow must start from the caller's rows again, not from the attempt's"""
    cloud = scenes.synth_cloud(12000, 123, log_scale_mean=-0.5, pos_sigma=1.0)      # ~10 M pairs at 1024 x 1024, capacity starts at 4 M
    W = H = 1024
    view = scenes.default_view(W, H, z=4.0)
    dst = random_dst(H, W, 71)
    r = make_renderer(cloud)                                # automatic capacity
    r.Sort(*view)
    got = host_frame(r, view, "load", dst, call=r.Render)                 # the context's first render
    st = r.stats()
    assert st["pairs"] > (1 << 22) and st["pair_capacity"] >= st["pairs"], st      # it did overflow, and grew
    calm = make_renderer(cloud, pair_capacity=int(st["pairs"]) + 4096)               # never overflows
    calm.Sort(*view)
    np.testing.assert_array_equal(got, host_frame(calm, view, "load", dst, call=calm.Render))
    assert calm.stats()["pair_capacity"] == int(st["pairs"]) + 4096


# ------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------

def test_refused_combinations_say_why():
    cloud, W, H, view = view_of("hard")
    for mode in ("load", "premultiplied"):
        r = make_renderer(cloud)                            # the mode first, the emulation second
        r.set_target_mode(mode)
        with pytest.raises(MsplatError) as e:
            r.set_target_emulation("rgba8")
        assert e.value.code == _capi.ERR_UNSUPPORTED and "msplat_set_target_mode" in r.last_error()
        r = make_renderer(cloud)                            # and the other way round
        r.set_target_emulation("rgba8")
        with pytest.raises(MsplatError) as e:
            r.set_target_mode(mode)
        assert e.value.code == _capi.ERR_UNSUPPORTED and "msplat_set_target_emulation" in r.last_error()
        assert r.target_mode() == "clear"
        # the tile probe has no instantiation that reads the target: refused by the Render, not rendered as CLEAR
        r = make_renderer(cloud)
        r.Sort(*view)
        r.set_tile_probe(True)
        r.set_target_mode(mode)
        with pytest.raises(MsplatError) as e:
            r.Render(*view, out=np.zeros((H, W, 4), np.float32))
        assert e.value.code == _capi.ERR_UNSUPPORTED and "probe" in r.last_error() and r.last_error().startswith("msplat_render: ")
    # a bad mode
    L = _capi.lib()
    r = make_renderer(cloud)
    assert L.msplat_set_target_mode(r._ctx, 3) == _capi.ERR_INVALID_ARG and L.msplat_set_target_mode(r._ctx, -1) == _capi.ERR_INVALID_ARG
    assert L.msplat_get_target_mode(r._ctx) == _capi.TARGET_CLEAR
    r.set_target_mode("load")
    with pytest.raises(ValueError):
        r.Render(*view)                                     # out=None has no contents to blend over


def test_point_clouds_refuse_the_modes_in_either_order():
    pts = np.random.default_rng(81).uniform(-1, 1, (500, 8)).astype(np.float32)
    pts[:, 3] = 1.0
    pts[:, 4:] = np.abs(pts[:, 4:])
    L = _capi.lib()

    def upload(h):
        return L.msplat_upload_points(h, pts.ctypes.data, pts.shape[0], 32, 0, 16)

    cfg = _capi.Config()
    cfg.struct_size = _capi.C.sizeof(_capi.Config)
    cfg.t_epsilon = -1.0
    for mode in (_capi.TARGET_LOAD, _capi.TARGET_PREMULTIPLIED):
        h = _capi.C.c_void_p()
        assert L.msplat_create(_capi.C.byref(h), _capi.C.byref(cfg)) == _capi.OK
        assert upload(h) == _capi.OK                        # the points first
        assert L.msplat_set_target_mode(h, mode) == _capi.ERR_UNSUPPORTED
        assert b"point cloud" in L.msplat_last_error(h) and L.msplat_get_target_mode(h) == _capi.TARGET_CLEAR
        L.msplat_destroy(h)
        h = _capi.C.c_void_p()
        assert L.msplat_create(_capi.C.byref(h), _capi.C.byref(cfg)) == _capi.OK
        assert L.msplat_set_target_mode(h, mode) == _capi.OK         # the mode first
        assert upload(h) == _capi.ERR_UNSUPPORTED
        assert b"msplat_set_target_mode" in L.msplat_last_error(h)
        assert L.msplat_set_target_mode(h, _capi.TARGET_CLEAR) == _capi.OK and upload(h) == _capi.OK
        L.msplat_destroy(h)
