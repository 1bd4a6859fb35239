"""GPU tests of msplat_render_occluded: the splat frame behind a caller's plane of window depths (GL_LESS, app.cpp:160-163).

Per pixel p the frame is msplat_render's with every splat i with !(z_i < plane[p]) absent at p.  Checked here:
  planes that hide nothing / everything (bit for bit against msplat_render / the empty frame), the exact partition (a region of
  one level equals msplat_render of a context that holds only the splats in front of it, bit for bit at t_epsilon = 0), the
  unchanged oracle (tests/render_cases.occluded_reference through tests/checks.check_over, its bounds unchanged),
  the tie rule on a splat whose z_w is exact, every execution shape against the plain occluded frame (bit for bit), refusals.

The planes of the partition and oracle tests keep every level 2^-20 away from every drawn splat's z_w (asserted on the CPU in
tests/test_occluded.py): the GPU's z_w may differ from the oracle's in the last bits."""
import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import MsplatError, _capi, camera
from tests import scenes
from tests.checks import T_EPS, check_over
from tests.gpu_harness import PAD_COLOUR, device_frame, host_frame, make_renderer, mixed_plane, subset_renderer
from tests.render_cases import (MODES, assert_plane_is_testable, choose_levels, const_dst, definition_f64, dst_for, empty_frame, four_levels,
                                hand_placed, hand_placed_ramp, hand_placed_splats, occluded_reference, random_dst, reference_layers, scene,
                                scene_splats, view_of)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# 1. / 2. planes that hide nothing, planes that hide everything
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["fp32", "fp16", "rgba8", "srgb8"])
@pytest.mark.parametrize("name", ["sparse", "dense"])
def test_an_open_plane_gives_the_plain_frame(name, fmt):
    cloud, W, H, view = view_of(name)
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(*view)
    dst = dst_for(fmt, H, W, 5)
    for mode in MODES:
        want = host_frame(r, view, mode, dst, call=r.Render)
        for level in (np.inf, 2.0):
            plane = np.full((H, W), level, np.float32)
            np.testing.assert_array_equal(host_frame(r, view, mode, dst, call=r.Render, occluder=plane), want, err_msg="%s host %g" % (mode, level))
            np.testing.assert_array_equal(device_frame(r, view, mode, dst, call=r.Render, occluder=plane, fill=PAD_COLOUR), want, err_msg="%s device %g" % (mode, level))
        np.testing.assert_array_equal(host_frame(r, view, mode, dst, call=r.Render), want)        # a plain Render afterwards is the plain Render


@pytest.mark.parametrize("fmt", ["fp32", "fp16", "rgba8", "srgb8"])
def test_a_closed_plane_gives_the_empty_frame(fmt):
    cloud, W, H, view = view_of("hard")
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(*view)
    dst = dst_for(fmt, H, W, 6)
    assert not np.array_equal(host_frame(r, view, "clear", dst, call=r.Render), empty_frame("clear", dst))      # the view is not empty
    for mode in MODES:
        for level in (0.0, -1.0, np.nan):
            plane = np.full((H, W), level, np.float32)
            want = empty_frame(mode, dst)
            assert host_frame(r, view, mode, dst, call=r.Render, occluder=plane).tobytes() == np.ascontiguousarray(want).tobytes(), (mode, level)
            assert device_frame(r, view, mode, dst, call=r.Render, occluder=plane, fill=PAD_COLOUR).tobytes() == np.ascontiguousarray(want).tobytes(), (mode, level)


# ------------------------------------------------------------------------------------------------
# 3. exact partition
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hard", "dense"])
def test_each_region_is_the_frame_of_the_splats_in_front_of_its_level(name):
    cloud, W, H, view = view_of(name)
    splats, V = scene_splats(name)
    plane, levels = four_levels(name)
    plane = plane.copy()
    exact = make_renderer(cloud, t_epsilon=0.0)
    early = make_renderer(cloud)
    exact.Sort(*view); early.Sort(*view)
    assert exact.sort_count() == V
    got0 = host_frame(exact, view, "clear", call=exact.Render, occluder=plane)
    got1 = host_frame(early, view, "clear", call=early.Render, occluder=plane)
    plain = host_frame(exact, view, "clear", call=exact.Render)
    if name == "dense":
        assert np.diff(exact.debug_tile_lists(want_pairs=False)[0].astype(np.int64)).max() > 128      # lists longer than two batches
    for v in levels:
        region = plane == v
        sub, n = subset_renderer(name, splats, v, t_epsilon=0.0)
        assert 0 < n < V
        sub.Sort(*view)
        want = host_frame(sub, view, "clear", call=sub.Render)
        sub.close()
        # default t_epsilon: the walk stops at a batch boundary with T < t_epsilon left, the exact one goes on
        err = np.abs(got1[region].astype(np.float64) - want[region]).max()
        print("%s level %.9g: %d of %d splats in front, max |early - exact| %.3g (t_epsilon %.3g)" % (name, v, n, V, err, T_EPS))
        np.testing.assert_array_equal(got0[region], want[region], err_msg="level %.9g" % v)
        assert err <= T_EPS
    # the plane hides something that shows -- in "hard"; inside the dense cloud the nearest fifth of the splats leaves T below an
    # ulp of the colour everywhere, and what lies behind adds nothing even at t_epsilon = 0: there the test is about the long lists
    changed = int((got0 != plain).any(axis=-1).sum())
    print("%s: %d pixel(s) differ from the plain frame" % (name, changed))
    assert changed > 0 or name == "dense"


# ------------------------------------------------------------------------------------------------
# 4. against the unchanged oracle
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t_eps", [-1.0, 0.0])
@pytest.mark.parametrize("name", ["sparse", "dense"])
def test_the_occluded_frame_matches_the_oracle(name, t_eps):
    cloud, W, H, view = view_of(name)
    plane = four_levels(name)[0].copy()
    L = reference_layers(name)
    r = make_renderer(cloud, t_epsilon=t_eps)
    r.Sort(*view)
    assert r.sort_count() == scene_splats(name)[1]
    eps = T_EPS if t_eps < 0 else t_eps
    opaque = const_dst(H, W, (0, 0, 0, 1))                  # CLEAR is the blend over (0, 0, 0, 1)
    check_over(host_frame(r, view, "clear", call=r.Render, occluder=plane), L, opaque, eps)
    dst = random_dst(H, W, 11)
    check_over(host_frame(r, view, "load", dst, call=r.Render, occluder=plane), L, dst, eps)
    check_over(host_frame(r, view, "premultiplied", call=r.Render, occluder=plane), L, np.zeros((H, W, 4), np.float32), eps)


@pytest.mark.parametrize("t_eps", [-1.0, 0.0])
def test_a_ramp_plane_matches_the_definition(t_eps):
    aos, W, H, view = hand_placed()
    splats = hand_placed_splats()
    ramp = hand_placed_ramp()
    layer, T = definition_f64(splats, ramp, W, H)
    bud = occluded_reference(splats, ramp, W, H, nthreads=4)          # one level per column: the flip budgets of each column's frame
    L = dict(layer=layer, T=T, bud_c=bud["bud_c"], bud_w=bud["bud_w"])
    r = make_renderer(aos, t_epsilon=t_eps)
    r.Sort(*view)
    assert r.sort_count() == splats.shape[0]
    eps = T_EPS if t_eps < 0 else t_eps
    check_over(host_frame(r, view, "clear", call=r.Render, occluder=ramp), L, const_dst(H, W, (0, 0, 0, 1)), eps)
    dst = random_dst(H, W, 12)
    check_over(host_frame(r, view, "load", dst, call=r.Render, occluder=ramp), L, dst, eps)
    check_over(host_frame(r, view, "premultiplied", call=r.Render, occluder=ramp), L, np.zeros((H, W, 4), np.float32), eps)
    assert np.abs(host_frame(r, view, "clear", call=r.Render, occluder=ramp) - host_frame(r, view, "clear", call=r.Render)).max() > 0.05      # the ramp hides something


# ------------------------------------------------------------------------------------------------
# 5. the tie rule
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("z, zw, drawn", [(-1.5, 0.5, False), (-2.0, 0.75, True)])
def test_a_splat_at_the_planes_depth_is_hidden(z, zw, drawn):
    """identity camera at the origin, perspective with near / far = 1 / 3: the matrix entries -2 and -3 are exact, so a splat at
    view z has clip z = -2 z - 3 and w = -z.  z = -1.5: clip z = 0, z_w = 0.5 exactly -- but ndc.z = 0 lies in front of the
    geometry stage's ndc.z < 0.25 cull (splat_geom.glsl), so that splat is never drawn and the two comparisons hold with empty
    frames on both sides.  z = -2: clip z = 1, w = 2, ndc.z = 0.5, z_w = 0.75 exactly, and the splat is drawn: there the rule
    is really tested."""
    W, H, zn, zf = 64, 48, 1.0, 3.0
    proj = camera.perspective(camera.FOVY, W / H, zn, zf)
    assert proj.reshape(4, 4)[2, 2] == -2.0 and proj.reshape(4, 4)[3, 2] == -3.0
    view = (camera.pose((0.0, 0.0, 0.0)), proj, [0, 0, W, H], [zn, zf])
    aos = orc.build_cloud(np.array([[0.0, 0.0, z]], np.float32), np.array([[0.8, 0.1, -0.4]], np.float32), None,
                          np.array([3.0], np.float32), np.log(np.full((1, 3), 0.2, np.float32)), np.array([[1, 0, 0, 0]], np.float32), False)
    r = make_renderer(aos)
    r.Sort(*view)
    plain = host_frame(r, view, "clear", call=r.Render)
    empty = empty_frame("clear", plain)
    assert (not np.array_equal(plain, empty)) == drawn
    level = np.float32(zw)
    np.testing.assert_array_equal(host_frame(r, view, "clear", call=r.Render, occluder=np.full((H, W), level, np.float32)), empty)
    np.testing.assert_array_equal(host_frame(r, view, "clear", call=r.Render, occluder=np.full((H, W), np.nextafter(level, np.float32(1)), np.float32)), plain)
    if drawn:
        np.testing.assert_array_equal(host_frame(r, view, "clear", call=r.Render, occluder=np.full((H, W), np.nextafter(level, np.float32(0)), np.float32)), empty)


# ------------------------------------------------------------------------------------------------
# 6. bit-identical across execution shapes
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("share", [1.0 / 64.0, 0.3, 1.0])
def test_two_pass_frames_equal_the_single_pass(share):
    cloud, W, H, view = view_of("dense", z=5.0, yaw=0.3)          # from outside: saturated centre, unfinished rim
    a = make_renderer(cloud, two_pass=_capi.TWO_PASS_OFF)
    b = make_renderer(cloud, two_pass=_capi.TWO_PASS_ON)
    b.two_pass_state(share)
    a.Sort(*view); b.Sort(*view)
    plane = mixed_plane(a, view)
    dst = random_dst(H, W, 21)
    before = b.two_pass_state(share)[0]
    for mode in MODES:
        want = host_frame(a, view, mode, dst, call=a.Render, occluder=plane)
        np.testing.assert_array_equal(host_frame(b, view, mode, dst, call=b.Render, occluder=plane), want)
        np.testing.assert_array_equal(device_frame(b, view, mode, dst, call=b.Render, occluder=plane, fill=PAD_COLOUR), want)
    assert b.two_pass_state(share)[0] == before + 6 and a.two_pass_state()[0] == 0
    assert not np.array_equal(host_frame(a, view, "clear", call=a.Render, occluder=plane), host_frame(a, view, "clear", call=a.Render))
    print("two-pass, share %g: %s" % (share, b.two_pass_info()))


@pytest.mark.parametrize("W, H", [(20, 12), (100, 70)])
def test_small_viewports(W, H):
    """a viewport smaller than a bin and one of a few ragged bins: two levels, left and right of the middle column, each half the
    frame of the splats in front of its level (t_epsilon = 0: bit for bit); device output equals host output"""
    cloud = scene("sparse")[0]
    view = cam, proj, vp, nf = scenes.default_view(W, H, z=7.0)
    ref = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=4, want_image=False, want_splats=True)
    splats = ref["splats"]
    levels = choose_levels(splats, (0.3, 0.7))
    plane = np.empty((H, W), np.float32)
    plane[:, :W // 2], plane[:, W // 2:] = levels[0], levels[1]
    assert_plane_is_testable(splats, plane)
    r = make_renderer(cloud, t_epsilon=0.0)
    r.Sort(*view)
    got = host_frame(r, view, "clear", call=r.Render, occluder=plane)
    dst = random_dst(H, W, 25)
    for mode in MODES:
        np.testing.assert_array_equal(device_frame(r, view, mode, dst, call=r.Render, occluder=plane, fill=PAD_COLOUR),
                                      host_frame(r, view, mode, dst, call=r.Render, occluder=plane))
    for v in levels:
        sub, n = subset_renderer(cloud, splats, v, t_epsilon=0.0)
        sub.Sort(*view)
        np.testing.assert_array_equal(got[plane == v], host_frame(sub, view, "clear", call=sub.Render)[plane == v])
        sub.close()


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
    plane = mixed_plane(plain, view)
    foreign = plane.copy()
    foreign[~owned] = np.nan                                # the other bands' rows of the plane: not this context's to read
    dst = random_dst(H, W, 51)
    for mode in MODES:
        want = host_frame(plain, view, mode, dst, call=plain.Render, occluder=plane)
        assert not np.array_equal(want[owned], host_frame(plain, view, mode, dst, call=plain.Render)[owned])
        for got in (host_frame(band, view, mode, dst, call=band.Render, occluder=foreign),
                    device_frame(band, view, mode, dst, call=band.Render, occluder=foreign, fill=PAD_COLOUR)):
            np.testing.assert_array_equal(got[owned], want[owned])
            assert got[~owned].tobytes() == dst[~owned].tobytes(), "mode %s touched rows of another band" % mode


@pytest.mark.parametrize("shape", ["four_in_flight", "async_submit"])
def test_frames_in_flight_and_queued_calls_equal_one_context(shape):
    import torch
    cloud, W, H, _ = scene("sparse")
    views = [scenes.default_view(W, H, z=7.0, yaw=0.3 * k) for k in range(6)]
    one = make_renderer(cloud)
    planes = []
    for view in views:
        one.Sort(*view)
        planes.append(mixed_plane(one, view))
    fly = make_renderer(cloud, frames_in_flight=4) if shape == "four_in_flight" else make_renderer(cloud, async_submit=True)
    dsts = [random_dst(H, W, 40 + k) for k in range(len(views))]
    for mode in ("load", "clear"):
        fly.set_target_mode(mode)                            # every context of the rotation
        fbs = [torch.from_numpy(d.copy()).to("cuda:0") for d in dsts]
        zbs = [torch.from_numpy(p).to("cuda:0") for p in planes]        # alive until the frames have run
        torch.cuda.synchronize()
        for k, (cam, proj, vp, nf) in enumerate(views):
            fly.Sort(cam, proj, vp, nf)
            fly.Render(cam, proj, vp, nf, out_ptr=fbs[k].data_ptr(), pitch_bytes=W * 16, occluder_ptr=zbs[k].data_ptr())      # tight plane
        fly.synchronize()
        for k, view in enumerate(views):
            one.Sort(*view)
            np.testing.assert_array_equal(fbs[k].cpu().numpy(), host_frame(one, view, mode, dsts[k], call=one.Render, occluder=planes[k]),
                                          err_msg="%s frame %d" % (mode, k))


def test_persistent_waves_on_the_work_queue_equal_one_wave_per_item():
    cloud, W, H, view = view_of("dense")
    a = make_renderer(cloud)
    b = make_renderer(cloud, compositor_waves=64)
    a.Sort(*view); b.Sort(*view)
    plane = mixed_plane(a, view)
    dst = random_dst(H, W, 61)
    for mode in MODES:
        np.testing.assert_array_equal(host_frame(b, view, mode, dst, call=b.Render, occluder=plane), host_frame(a, view, mode, dst, call=a.Render, occluder=plane))
    items, grid = b.compositor_launch()[:2]
    assert grid == 64 and items > grid                       # the work-queue regime


def test_host_output_survives_a_pair_buffer_overflow():
    """the scene of tests/test_gpu_target_mode's overflow test: the context's first render overflows the initial capacity, grows the
    buffer and renders again -- from the plane staged once, over the caller's rows again (LOAD)"""
    cloud = scenes.synth_cloud(12000, 123, log_scale_mean=-0.5, pos_sigma=1.0)      # ~10 M pairs at 1024 x 1024, capacity starts at 4 M
    W = H = 1024
    view = scenes.default_view(W, H, z=4.0)
    # z_w = 1 - 0.1 / d (near 0.1, far 1000) for a cloud of sigma 1 seen from 4: a ramp across the depths 1 .. 7 (the splats are
    # huge: the nearest few hundred saturate the frame, so the ramp has to start in front of them to hide anything that shows)
    col = np.linspace(0.90, 0.986, W, dtype=np.float32)
    plane = np.ascontiguousarray(np.broadcast_to(col, (H, W)))
    dst = random_dst(H, W, 71)
    r = make_renderer(cloud)                                # automatic capacity
    r.Sort(*view)
    got = host_frame(r, view, "load", dst, call=r.Render, occluder=plane)        # the context's first render
    st = r.stats()
    assert st["pairs"] > (1 << 22) and st["pair_capacity"] >= st["pairs"], st      # it did overflow, and grew
    calm = make_renderer(cloud, pair_capacity=int(st["pairs"]) + 4096)               # never overflows
    calm.Sort(*view)
    np.testing.assert_array_equal(got, host_frame(calm, view, "load", dst, call=calm.Render, occluder=plane))
    assert not np.array_equal(got, host_frame(calm, view, "load", dst, call=calm.Render)) and not np.array_equal(got, dst)      # some hidden, some shown


# ------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------

def test_refused_combinations_say_why_and_leave_the_context_usable():
    import torch
    cloud, W, H, view = view_of("hard")
    r = make_renderer(cloud)
    r.Sort(*view)
    plain = r.Render(*view)
    plane = mixed_plane(r, view)
    want = host_frame(r, view, "clear", call=r.Render, occluder=plane)
    switches = [("msplat_set_depth_test", lambda on: r.set_depth_test(24 if on else 0)),
                ("msplat_set_target_emulation", lambda on: r.set_target_emulation("rgba8" if on else None)),
                ("probe", lambda on: r.set_tile_probe(on))]
    for word, switch in switches:
        switch(True)
        out = np.full((H, W, 4), -123.0, np.float32)
        with pytest.raises(MsplatError) as e:
            r.Render(*view, out=out, occluder=plane)
        assert e.value.code == _capi.ERR_UNSUPPORTED and word in r.last_error() and "msplat_render_occluded" in r.last_error()
        assert (out == -123.0).all()
        r.Render(*view)                                     # the plain Render of that configuration still works
        switch(False)
        np.testing.assert_array_equal(r.Render(*view), plain)
        np.testing.assert_array_equal(host_frame(r, view, "clear", call=r.Render, occluder=plane), want)
    # a depth output and an occluder plane in one frame
    for kw in (dict(depth=True, occluder=plane), dict(depth=np.zeros((H, W), np.float32), occluder=plane), dict(out_ptr=1, depth_ptr=1, occluder_ptr=1)):
        with pytest.raises(MsplatError) as e:
            r.Render(*view, **kw)
        assert e.value.code == _capi.ERR_UNSUPPORTED and "occluder" in str(e.value)
    # a bad pitch
    fb = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    zb = torch.from_numpy(np.concatenate([plane, np.zeros((H, 8), np.float32)], axis=1)).to("cuda:0")
    torch.cuda.synchronize()
    for pitch in (4 * W - 4, 4 * W + 2, 3):
        with pytest.raises(MsplatError) as e:
            r.Render(*view, out_ptr=fb.data_ptr(), pitch_bytes=W * 16, occluder_ptr=zb.data_ptr(), occluder_pitch_bytes=pitch)
        assert e.value.code == _capi.ERR_INVALID_ARG and "pitch" in r.last_error() and "msplat_render_occluded" in r.last_error()
    r.Render(*view, out_ptr=fb.data_ptr(), pitch_bytes=W * 16, occluder_ptr=zb.data_ptr(), occluder_pitch_bytes=4 * W + 32)
    r.synchronize()
    np.testing.assert_array_equal(fb.cpu().numpy(), want)
    # the plane lives where the colour does
    with pytest.raises(ValueError):
        r.Render(*view, out_ptr=fb.data_ptr(), pitch_bytes=W * 16, occluder=plane)
    with pytest.raises(ValueError):
        r.Render(*view, occluder_ptr=zb.data_ptr())
    np.testing.assert_array_equal(r.Render(*view), plain)


def test_point_clouds_have_no_occluder_test():
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
    img, z = np.full((H, W, 4), -123.0, np.float32), np.ones((H, W), np.float32)
    assert L.msplat_render_occluded(h, *p, img.ctypes.data, 0, z.ctypes.data, 0, 0) == _capi.ERR_UNSUPPORTED
    assert b"point cloud" in L.msplat_last_error(h) and (img == -123.0).all()
    assert L.msplat_render_occluded(h, *p, img.ctypes.data, 0, None, 0, 0) == _capi.OK         # occluder == NULL is msplat_render
    assert (img[..., 3] == 1.0).all()
    L.msplat_destroy(h)


def test_the_group_refuses_the_occluder_argument():
    from splatapult_amd import SplatRendererGroup
    cloud, W, H, view = view_of("hard")
    g = SplatRendererGroup([0])
    assert g.Init(cloud), g.last_error()
    g.Sort(*view)
    want = g.Render(*view)
    with pytest.raises(MsplatError) as e:
        g.Render(*view, occluder=np.ones((H, W), np.float32))
    assert e.value.code == _capi.ERR_UNSUPPORTED
    np.testing.assert_array_equal(g.Render(*view), want)
    g.close()
