"""GPU tests of msplat_render_layers / msplat_render_stereo_layers: msplat_render_occluded's colour and a depth plane in one frame,

    depth[p] = min(fma(T, d0, sum_{i: z_i < o} T_i w_i z_i), 1),   o = occluder[p],  d0 = o > 0 ? (o > 1 ? 1 : o) : 0  (NaN -> 0)

-- the expected window depth of the splats that pass GL_LESS, blended over what the depth attachment holds -- for one view and for
both eyes of one Sort in one chain of launches.  Checked here: the degradations (a NULL plane gives the call without it, bit for
bit), the combined frame (colour = msplat_render_occluded's bit for bit; the plane against the unchanged oracle,
tests/render_cases.layers_reference through tests/checks.check_plane with its bounds unchanged -- 2 TIGHT + t_eps
carries over because 0 <= d0 <= 1; the exact partition; d0 where nothing is seen; in place), every execution shape against the
plain combined frame (bit for bit), the stereo chain and its fallbacks against one msplat_render_layers per eye (bit for bit), and
the refusals.  The planes of the oracle and partition tests keep every level 2^-20 away from every drawn splat's z_w (asserted on
the CPU in tests/test_occluded.py and tests/test_layers.py)."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import MsplatError, _capi
from tests import scenes
from tests.checks import T_EPS, check_plane, same_bits
from tests.gpu_harness import (JUNK, PAD_COLOUR, SENTINEL, device_frame, host_frame, make_renderer, mixed_plane, stereo_frame,
                               subset_renderer)
from tests.render_cases import (MODES, NP_DTYPES, SMALL_VIEWPORTS, d0_of, dst_for, empty_frame, four_levels, random_dst, reference_plane,
                                scene, scene_splats, small_viewport_case, stereo_eyes, view_of)

pytestmark = pytest.mark.gpu

# the device targets of this module: the colour's padding holds PAD_COLOUR, the depth plane's (like the occluder's) NaN / 0 junk
PITCHED = dict(fill=PAD_COLOUR, dfill=JUNK)


# ------------------------------------------------------------------------------------------------
# 1. degradation, bit for bit
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["fp32", "fp16", "rgba8", "srgb8"])
def test_a_missing_plane_gives_the_call_without_it(fmt):
    cloud, W, H, view = view_of("sparse")
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(*view)
    plane = mixed_plane(r, view)
    dst = dst_for(fmt, H, W, 5)
    cam, proj, vp, nf = view
    for mode in MODES:
        plain = host_frame(r, view, mode, dst, call=r.Render)
        # neither plane: msplat_render
        r.set_target_mode(mode)
        same_bits(r.RenderLayers(cam, proj, vp, nf, out=dst.copy()), plain, "%s: no planes, host" % mode)
        same_bits(device_frame(r, view, mode, dst, call=r.RenderLayers, **PITCHED), plain, "%s: no planes, device" % mode)
        # depth only: msplat_render_depth
        r.set_target_mode(mode)
        want_img, want_z = r.Render(cam, proj, vp, nf, out=dst.copy(), depth=True)
        same_bits(want_img, plain)
        img, z = host_frame(r, view, mode, dst, call=r.RenderLayers, depth=True)
        same_bits(img, want_img, "%s: depth only, host" % mode); same_bits(z, want_z, "%s: depth only, host plane" % mode)
        img, z = device_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, **PITCHED)
        same_bits(img, want_img, "%s: depth only, device" % mode); same_bits(z, want_z, "%s: depth only, device plane" % mode)
        # occluder only: msplat_render_occluded
        want = host_frame(r, view, mode, dst, call=r.Render, occluder=plane)
        r.set_target_mode(mode)
        same_bits(r.RenderLayers(cam, proj, vp, nf, out=dst.copy(), occluder=plane), want, "%s: occluder only, host" % mode)
        same_bits(device_frame(r, view, mode, dst, call=r.RenderLayers, occluder=plane, **PITCHED), want, "%s: occluder only, device" % mode)
        same_bits(device_frame(r, view, mode, dst, call=r.Render, occluder=plane, fill=PAD_COLOUR), want)
        assert not np.array_equal(want, plain)
        # an open plane with a depth output: msplat_render's colour, msplat_render_depth's plane
        for level in (np.inf, 2.0):
            op = np.full((H, W), level, np.float32)
            for img, z in (host_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=op),
                           device_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=op, **PITCHED)):
                same_bits(img, plain, "%s: open plane %g" % (mode, level)); same_bits(z, want_z, "%s: open plane %g, depth" % (mode, level))
        # a closed plane: the empty frame and a depth plane of exactly 0
        for level in (0.0, -1.0, np.nan):
            cl = np.full((H, W), level, np.float32)
            for img, z in (host_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=cl),
                           device_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=cl, **PITCHED)):
                same_bits(img, np.ascontiguousarray(empty_frame(mode, dst)), "%s: closed plane %g" % (mode, level))
                same_bits(z, np.zeros((H, W), np.float32), "%s: closed plane %g, depth" % (mode, level))
        same_bits(host_frame(r, view, mode, dst, call=r.Render), plain)              # a plain Render afterwards is the plain Render


# ------------------------------------------------------------------------------------------------
# 2. the combined frame
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["fp32", "fp16", "rgba8", "srgb8"])
def test_the_colour_is_the_occluded_frames_and_the_plane_ignores_the_target(fmt):
    cloud, W, H, view = view_of("sparse")
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(*view)
    plane = mixed_plane(r, view)
    dst = dst_for(fmt, H, W, 7)
    planes = []
    for mode in MODES:
        want = host_frame(r, view, mode, dst, call=r.Render, occluder=plane)
        img, z = host_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=plane)
        same_bits(img, want, "%s host" % mode)
        dimg, dz = device_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=plane, **PITCHED)
        same_bits(dimg, want, "%s device" % mode); same_bits(dz, z, "%s: device plane differs from host plane" % mode)
        assert np.isfinite(z).all() and z.min() >= 0.0 and z.max() <= 1.0
        planes.append(z)
    same_bits(planes[1], planes[0], "the plane depends on the target mode"); same_bits(planes[2], planes[0], "the plane depends on the target mode")
    # where no surviving splat reaches a pixel the plane holds d0 exactly
    if fmt == "fp32":
        untouched = host_frame(r, view, "premultiplied", call=r.Render, occluder=plane)[..., 3] == 0
        assert untouched.mean() > 0.01 and (~untouched).mean() > 0.01
        same_bits(planes[0][untouched], d0_of(plane)[untouched], "a pixel no surviving splat reaches must read d0")
        _, plain_z = host_frame(r, view, "clear", call=r.Render, depth=True)
        assert not np.array_equal(planes[0], plain_z)            # the occluder matters to the plane


@pytest.mark.parametrize("t_eps", [-1.0, 0.0])
@pytest.mark.parametrize("name", ["sparse", "dense"])
def test_the_plane_matches_the_oracle(name, t_eps):
    cloud, W, H, view = view_of(name)
    plane = four_levels(name)[0].copy()
    L = reference_plane(name)
    r = make_renderer(cloud, t_epsilon=t_eps)
    r.Sort(*view)
    assert r.sort_count() == scene_splats(name)[1]
    eps = T_EPS if t_eps < 0 else t_eps
    img, z = host_frame(r, view, "clear", call=r.RenderLayers, depth=True, occluder=plane)
    same_bits(img, host_frame(r, view, "clear", call=r.Render, occluder=plane))
    check_plane(z, L, eps)
    _, dz = device_frame(r, view, "load", random_dst(H, W, 11), call=r.RenderLayers, depth=True, occluder=plane, **PITCHED)
    same_bits(dz, z)


@pytest.mark.parametrize("name", ["hard", "dense"])
def test_each_region_of_the_plane_is_that_of_the_splats_in_front_of_its_level(name):
    """the check that a hidden splat feeds neither cz nor T: at t_epsilon = 0 the full cloud's plane equals, in the region of level
    v, the plane of a context that holds only the splats in front of v, rendered through the same call with the same occluder"""
    cloud, W, H, view = view_of(name)
    splats, V = scene_splats(name)
    plane, levels = four_levels(name)
    plane = plane.copy()
    exact = make_renderer(cloud, t_epsilon=0.0)
    exact.Sort(*view)
    assert exact.sort_count() == V
    img0, z0 = host_frame(exact, view, "clear", call=exact.RenderLayers, depth=True, occluder=plane)
    if name == "dense":
        assert np.diff(exact.debug_tile_lists(want_pairs=False)[0].astype(np.int64)).max() > 128      # lists longer than two batches
    for v in levels:
        region = plane == v
        sub, n = subset_renderer(name, splats, v, t_epsilon=0.0)
        assert 0 < n < V
        sub.Sort(*view)
        img, z = host_frame(sub, view, "clear", call=sub.RenderLayers, depth=True, occluder=plane)
        sub.close()
        same_bits(z0[region], z[region], "level %.9g: the plane" % v)
        same_bits(img0[region], img[region], "level %.9g: the colour" % v)
    _, zplain = host_frame(exact, view, "clear", call=exact.Render, depth=True)
    changed = int((z0 != zplain).sum())
    print("%s: %d value(s) of the plane differ from msplat_render_depth's" % (name, changed))
    # (inside the dense cloud the nearest fifth of the splats leaves T below an ulp of the plane everywhere: there the test is about
    #  the long lists, as in tests/test_gpu_occluded.py)
    assert changed > 0 or name == "dense"


@pytest.mark.parametrize("name", ["sparse", "dense"])
def test_in_place_equals_separate_buffers(name):
    cloud, W, H, view = view_of(name)
    r = make_renderer(cloud)
    r.Sort(*view)
    plane = mixed_plane(r, view)
    dst = random_dst(H, W, 13)
    for mode in MODES:
        img, z = host_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=plane)
        attachment = plane.copy()
        himg, hz = host_frame(r, view, mode, dst, call=r.RenderLayers, depth=attachment, occluder=attachment)
        assert hz is attachment
        same_bits(himg, img, "%s host in place" % mode); same_bits(hz, z, "%s host in place, plane" % mode)
        dimg, dz = device_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=plane, **PITCHED, in_place=True)
        same_bits(dimg, img, "%s device in place" % mode); same_bits(dz, z, "%s device in place, plane" % mode)


# ------------------------------------------------------------------------------------------------
# 3. bit-identical across execution shapes
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
        img, z = host_frame(a, view, mode, dst, call=a.RenderLayers, depth=True, occluder=plane)
        for got, gz in (host_frame(b, view, mode, dst, call=b.RenderLayers, depth=True, occluder=plane),
                        device_frame(b, view, mode, dst, call=b.RenderLayers, depth=True, occluder=plane, **PITCHED),
                        device_frame(b, view, mode, dst, call=b.RenderLayers, depth=True, occluder=plane, **PITCHED, in_place=True)):
            same_bits(got, img, mode); same_bits(gz, z, mode)
    assert b.two_pass_state(share)[0] == before + 9 and a.two_pass_state()[0] == 0
    print("two-pass, share %g: %s" % (share, b.two_pass_info()))
    a.close(); b.close()
    # fp16 device output
    a = make_renderer(cloud, two_pass=_capi.TWO_PASS_OFF, fb_format="fp16")
    b = make_renderer(cloud, two_pass=_capi.TWO_PASS_ON, fb_format="fp16")
    b.two_pass_state(share)
    a.Sort(*view); b.Sort(*view)
    dst = random_dst(H, W, 22, np.float16)
    for mode in MODES:
        img, z = device_frame(a, view, mode, dst, call=a.RenderLayers, depth=True, occluder=plane, **PITCHED)
        got, gz = device_frame(b, view, mode, dst, call=b.RenderLayers, depth=True, occluder=plane, **PITCHED)
        same_bits(got, img, "fp16 " + mode); same_bits(gz, z, "fp16 " + mode)
    assert b.two_pass_state(share)[0] == 3


def test_three_bands_write_their_own_rows_of_both_planes():
    cloud, W, H, view = view_of("sparse")
    T = _capi.lib().msplat_tile_size()
    rows_full = (H + T - 1) // T
    plain = make_renderer(cloud)
    plain.Sort(*view)
    plane = mixed_plane(plain, view)
    dst = random_dst(H, W, 51)
    want = {mode: host_frame(plain, view, mode, dst, call=plain.RenderLayers, depth=True, occluder=plane) for mode in MODES}
    covered = np.zeros(H, bool)
    for rank in range(3):
        band = make_renderer(cloud)
        lay = band.set_band_plan("contiguous", rows_full, 3, rank)
        owned = np.isin(np.arange(H) // T, _capi.band_rows(*lay, rows_full))
        assert owned.any() and not owned.all() and not (covered & owned).any()
        covered |= owned
        band.Sort(*view)
        foreign = plane.copy()
        foreign[~owned] = np.nan                            # the other bands' rows of the occluder: not this context's to read
        for mode in MODES:
            img, z = want[mode]
            hz = np.full((H, W), SENTINEL, np.float32)
            himg, _ = host_frame(band, view, mode, dst, call=band.RenderLayers, depth=hz, occluder=foreign)
            dimg, dz = device_frame(band, view, mode, dst, call=band.RenderLayers, depth=True, occluder=foreign, **PITCHED)
            for gi, gz in ((himg, hz), (dimg, dz)):
                same_bits(gi[owned], img[owned], "%s rank %d" % (mode, rank)); same_bits(gz[owned], z[owned], "%s rank %d: plane" % (mode, rank))
                assert gi[~owned].tobytes() == dst[~owned].tobytes(), "mode %s touched colour rows of another band" % mode
                assert (gz[~owned] == SENTINEL).all(), "mode %s touched depth rows of another band" % mode
        band.close()
    assert covered.all()


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
        obs = [torch.from_numpy(p).to("cuda:0") for p in planes]        # alive until the frames have run
        dbs = [torch.full((H, W), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in views]
        torch.cuda.synchronize()
        for k, (cam, proj, vp, nf) in enumerate(views):
            fly.Sort(cam, proj, vp, nf)
            # odd frames: the attachment in place
            d = obs[k] if k % 2 else dbs[k]
            fly.RenderLayers(cam, proj, vp, nf, out_ptr=fbs[k].data_ptr(), pitch_bytes=W * 16, depth_ptr=d.data_ptr(), occluder_ptr=obs[k].data_ptr())
        fly.synchronize()
        for k, view in enumerate(views):
            one.Sort(*view)
            img, z = host_frame(one, view, mode, dsts[k], call=one.RenderLayers, depth=True, occluder=planes[k])
            same_bits(fbs[k].cpu().numpy(), img, "%s frame %d" % (mode, k))
            same_bits((obs[k] if k % 2 else dbs[k]).cpu().numpy(), z, "%s frame %d: plane" % (mode, k))


def test_persistent_waves_on_the_work_queue_equal_one_wave_per_item():
    cloud, W, H, view = view_of("dense")
    a = make_renderer(cloud)
    b = make_renderer(cloud, compositor_waves=64)
    a.Sort(*view); b.Sort(*view)
    plane = mixed_plane(a, view)
    dst = random_dst(H, W, 61)
    for mode in MODES:
        img, z = host_frame(a, view, mode, dst, call=a.RenderLayers, depth=True, occluder=plane)
        got, gz = host_frame(b, view, mode, dst, call=b.RenderLayers, depth=True, occluder=plane)
        same_bits(got, img, mode); same_bits(gz, z, mode)
    items, grid = b.compositor_launch()[:2]
    assert grid == 64 and items > grid                       # the work-queue regime


@pytest.mark.parametrize("W, H", SMALL_VIEWPORTS)
def test_small_viewports(W, H):
    """viewports that are no multiple of 16, one smaller than a bin, one of a single tile: device output equals host output, the
    colour is the occluded frame's, and with two levels left and right of the middle column each half of the plane is that of the
    splats in front of its level (t_epsilon = 0: bit for bit)"""
    cloud, view, splats, plane, levels = small_viewport_case(W, H)      # (the levels' conditions: tests/test_layers.py)
    plane = plane.copy()
    r = make_renderer(cloud, t_epsilon=0.0)
    r.Sort(*view)
    dst = random_dst(H, W, 25)
    for mode in MODES:
        img, z = host_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=plane)
        same_bits(img, host_frame(r, view, mode, dst, call=r.Render, occluder=plane), mode)
        for got, gz in (device_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=plane, **PITCHED),
                        device_frame(r, view, mode, dst, call=r.RenderLayers, depth=True, occluder=plane, **PITCHED, in_place=True)):
            same_bits(got, img, mode); same_bits(gz, z, mode)
    _, z = host_frame(r, view, "clear", call=r.RenderLayers, depth=True, occluder=plane)
    for v in levels:
        sub, n = subset_renderer(cloud, splats, v, t_epsilon=0.0)
        sub.Sort(*view)
        same_bits(z[plane == v], host_frame(sub, view, "clear", call=sub.RenderLayers, depth=True, occluder=plane)[1][plane == v], "level %.9g" % v)
        sub.close()


def test_host_output_survives_a_pair_buffer_overflow():
    """the scene of tests/test_gpu_occluded's overflow test: the context's first render overflows the initial capacity, grows the
    buffer and renders again -- from the occluder staged once, over the caller's rows again (LOAD), the attachment in place"""
    cloud = scenes.synth_cloud(12000, 123, log_scale_mean=-0.5, pos_sigma=1.0)      # ~10 M pairs at 1024 x 1024, capacity starts at 4 M
    W = H = 1024
    view = scenes.default_view(W, H, z=4.0)
    col = np.linspace(0.90, 0.986, W, dtype=np.float32)
    plane = np.ascontiguousarray(np.broadcast_to(col, (H, W)))
    dst = random_dst(H, W, 71)
    r = make_renderer(cloud)                                # automatic capacity
    r.Sort(*view)
    attachment = plane.copy()
    got, gz = host_frame(r, view, "load", dst, call=r.RenderLayers, depth=attachment, occluder=attachment)        # the context's first render
    st = r.stats()
    assert st["pairs"] > (1 << 22) and st["pair_capacity"] >= st["pairs"], st      # it did overflow, and grew
    calm = make_renderer(cloud, pair_capacity=int(st["pairs"]) + 4096)               # never overflows
    calm.Sort(*view)
    img, z = host_frame(calm, view, "load", dst, call=calm.RenderLayers, depth=True, occluder=plane)
    same_bits(got, img); same_bits(gz, z)
    same_bits(img, host_frame(calm, view, "load", dst, call=calm.Render, occluder=plane))
    assert not np.array_equal(z, plane) and (z < plane).any()              # splats in front of the attachment were blended into it


# ------------------------------------------------------------------------------------------------
# 4. / 5. both eyes: one chain, and the view-by-view fallbacks
# ------------------------------------------------------------------------------------------------

COMBOS = [(True, False), (False, True), (True, True)]         # (depth, occluder)


def eye_planes(r, cams, proj, vp, nf, swapped):
    """eye 0 closed and eye 1 the mixed plane of its own view, or the other way round: swapped pointers cannot pass"""
    H, W = vp[3], vp[2]
    closed = np.zeros((H, W), np.float32)
    closed[::3, ::2] = np.nan
    mixed = [mixed_plane(r, (cams[e], proj, vp, nf)) for e in range(2)]
    return [mixed[0], closed] if swapped else [closed, mixed[1]]


def with_planes(got, depth):
    """(images, planes or None) of what a frame of both eyes returned"""
    return got if depth else (got, None)


def per_eye(r, cams, proj, vp, nf, mode, dsts, planes, depth):
    """the same frame as one device-output RenderLayers per eye"""
    out = [device_frame(r, (cams[e], proj, vp, nf), mode, dsts[e], call=r.RenderLayers, depth=depth,
                        occluder=planes[e] if planes is not None else None, **PITCHED) for e in range(2)]
    return ([o[0] for o in out], [o[1] for o in out]) if depth else (out, None)


def assert_eyes(got, want, msg):
    for e in range(2):
        same_bits(got[0][e], want[0][e], "%s: eye %d colour" % (msg, e))
        if want[1] is not None:
            same_bits(got[1][e], want[1][e], "%s: eye %d plane" % (msg, e))


@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
@pytest.mark.parametrize("depth, occluder", COMBOS)
def test_stereo_layers_in_one_chain_equal_one_call_per_eye(depth, occluder, fmt):
    """70 x 45: view 0's partial top bin row sits under view 1's first row"""
    cloud = scene("hard")[0]
    W, H = 70, 45
    cams, proj, vp, nf = stereo_eyes(W, H)
    r = make_renderer(cloud, fb_format=fmt)
    r.Sort(cams[0], proj, vp, nf)
    dsts = [random_dst(H, W, 31, NP_DTYPES[fmt]), random_dst(H, W, 32, NP_DTYPES[fmt])]
    for swapped in (False, True):
        planes = eye_planes(r, cams, proj, vp, nf, swapped) if occluder else None
        for mode in MODES:                                   # LOAD: over random destinations
            want = per_eye(r, cams, proj, vp, nf, mode, dsts, planes, depth)
            mono_items = r.compositor_launch()[0]
            got = with_planes(stereo_frame(r, cams, [proj, proj], vp, nf, mode, dsts, call=r.RenderStereoLayers, depth=depth, occluders=planes, **PITCHED), depth)
            assert r.compositor_launch()[0] == 2 * mono_items, "the single chain did not run"
            assert_eyes(got, want, "%s swapped %d" % (mode, swapped))
            if depth and occluder:
                got = stereo_frame(r, cams, [proj, proj], vp, nf, mode, dsts, call=r.RenderStereoLayers, depth=depth, occluders=planes, **PITCHED, in_place=True)
                assert_eyes(with_planes(got, depth), want, "%s in place" % mode)
        assert not np.array_equal(want[0][0], want[0][1])
        if depth:
            assert not np.array_equal(want[1][0], want[1][1])
    # a mono frame on the same context afterwards is unaffected
    mono = device_frame(r, (cams[1], proj, vp, nf), "clear", dsts[1], call=r.RenderLayers, depth=depth, occluder=planes[1] if occluder else None, **PITCHED)
    same_bits(mono[0] if depth else mono, per_eye(r, cams, proj, vp, nf, "clear", dsts, planes, depth)[0][1])


@pytest.mark.parametrize("depth, occluder", COMBOS)
def test_stereo_layers_on_the_work_queue_and_in_flight(depth, occluder):
    import torch
    cloud, W, H, _ = scene("hard")
    cams, proj, vp, nf = stereo_eyes(W, H)
    one = make_renderer(cloud)
    one.Sort(cams[0], proj, vp, nf)
    dsts = [random_dst(H, W, 33), random_dst(H, W, 34)]
    planes = eye_planes(one, cams, proj, vp, nf, False) if occluder else None
    want = per_eye(one, cams, proj, vp, nf, "load", dsts, planes, depth)
    # persistent waves on the work queue
    q = make_renderer(cloud, compositor_waves=64)
    q.Sort(cams[0], proj, vp, nf)
    got = stereo_frame(q, cams, [proj, proj], vp, nf, "load", dsts, call=q.RenderStereoLayers, depth=depth, occluders=planes, **PITCHED)
    assert_eyes(with_planes(got, depth), want, "compositor_waves=64")
    items, grid = q.compositor_launch()[:2]
    assert grid == 64 and items > grid and items == 2 * one.compositor_launch()[0]
    # four contexts in flight: six frames, each with its own targets
    fly = make_renderer(cloud, frames_in_flight=4)
    fly.set_target_mode("load")
    n = 6
    fbs = [[torch.from_numpy(dsts[e].copy()).to("cuda:0") for e in range(2)] for _ in range(n)]
    obs = [[torch.from_numpy(planes[e]).to("cuda:0") for e in range(2)] for _ in range(n)] if occluder else None
    dbs = [[torch.full((H, W), SENTINEL, dtype=torch.float32, device="cuda:0") for e in range(2)] for _ in range(n)] if depth else None
    torch.cuda.synchronize()
    for k in range(n):
        fly.Sort(cams[0], proj, vp, nf)
        fly.RenderStereoLayers(cams, [proj, proj], vp, nf, out_ptrs=[f.data_ptr() for f in fbs[k]], pitch_bytes=W * 16,
                               depth_ptrs=[d.data_ptr() for d in dbs[k]] if depth else None,
                               occluder_ptrs=[o.data_ptr() for o in obs[k]] if occluder else None)
    fly.synchronize()
    for k in range(n):
        got = ([f.cpu().numpy() for f in fbs[k]], [d.cpu().numpy() for d in dbs[k]] if depth else None)
        assert_eyes(got, want, "in flight, frame %d" % k)


@pytest.mark.parametrize("depth, occluder", COMBOS)
def test_stereo_layers_fall_back_view_by_view(depth, occluder):
    cloud, W, H, _ = scene("hard")
    cams, proj, vp, nf = stereo_eyes(W, H)
    r = make_renderer(cloud)
    r.Sort(cams[0], proj, vp, nf)
    planes = eye_planes(r, cams, proj, vp, nf, True) if occluder else None
    dsts = [random_dst(H, W, 35), random_dst(H, W, 36)]
    want = per_eye(r, cams, proj, vp, nf, "clear", dsts, planes, depth)
    mono_items = r.compositor_launch()[0]
    # host arrays
    r.set_target_mode("clear")
    got = with_planes(r.RenderStereoLayers(cams, [proj, proj], vp, nf, depth=depth, occluders=planes), depth)
    assert_eyes(got, want, "host arrays")
    assert r.compositor_launch()[0] == mono_items
    # a banded context: owned rows of each eye
    T = _capi.lib().msplat_tile_size()
    band = make_renderer(cloud)
    band.set_band(2, 1)
    band.Sort(cams[0], proj, vp, nf)
    owned = np.arange(H) // T % 2 == 1
    gi, gz = with_planes(stereo_frame(band, cams, [proj, proj], vp, nf, "clear", dsts, call=band.RenderStereoLayers, depth=depth, occluders=planes, **PITCHED), depth)
    for e in range(2):
        same_bits(gi[e][owned], want[0][e][owned], "banded: eye %d" % e)
        assert gi[e][~owned].tobytes() == dsts[e][~owned].tobytes()
        if depth:
            same_bits(gz[e][owned], want[1][e][owned], "banded: eye %d plane" % e)
            assert (gz[e][~owned] == SENTINEL).all()
    assert band.compositor_launch()[0] < 2 * mono_items


@pytest.mark.parametrize("depth, occluder", COMBOS)
def test_stereo_layers_beyond_128_bin_rows_go_view_by_view(depth, occluder):
    cloud = scene("hard")[0]
    W, H = 64, 4128                                          # 129 bin rows per view
    cams, proj, vp, nf = stereo_eyes(W, H)
    r = make_renderer(cloud)
    r.Sort(cams[0], proj, vp, nf)
    planes = eye_planes(r, cams, proj, vp, nf, False) if occluder else None
    dsts = [random_dst(H, W, 37), random_dst(H, W, 38)]
    want = per_eye(r, cams, proj, vp, nf, "load", dsts, planes, depth)
    mono_items = r.compositor_launch()[0]
    assert mono_items == 4 * 2 * 129
    got = stereo_frame(r, cams, [proj, proj], vp, nf, "load", dsts, call=r.RenderStereoLayers, depth=depth, occluders=planes, **PITCHED)
    assert_eyes(with_planes(got, depth), want, "64 x 4128")
    assert r.compositor_launch()[0] == mono_items            # two renders, not one chain


# ------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------

def test_refused_combinations_say_why_and_leave_the_context_usable():
    import torch
    cloud = scene("hard")[0]
    W, H = 70, 45
    cams, proj, vp, nf = stereo_eyes(W, H)
    view = (cams[0], proj, vp, nf)
    r = make_renderer(cloud)
    r.Sort(*view)
    plain = r.Render(*view)
    plane = mixed_plane(r, view)
    want = host_frame(r, view, "clear", call=r.RenderLayers, depth=True, occluder=plane)
    fbs = [torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    zbs = [torch.full((H, W + 8), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    obs = [torch.from_numpy(plane).to("cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    ptrs = lambda ts: [t.data_ptr() for t in ts]

    def untouched():
        torch.cuda.synchronize()
        return all((t == SENTINEL).all().item() for t in fbs + zbs)

    switches = [("msplat_set_depth_test", lambda on: r.set_depth_test(24 if on else 0)),
                ("msplat_set_target_emulation", lambda on: r.set_target_emulation("rgba8" if on else None)),
                ("probe", lambda on: r.set_tile_probe(on))]
    for word, switch in switches:
        switch(True)
        for kw in (dict(depth=True, occluder=plane), dict(depth=True), dict(occluder=plane)):
            out = np.full((H, W, 4), SENTINEL, np.float32)
            with pytest.raises(MsplatError) as e:
                r.RenderLayers(*view, out=out, **kw)
            assert e.value.code == _capi.ERR_UNSUPPORTED and word in r.last_error() and "msplat_render_layers" in r.last_error()
            assert (out == SENTINEL).all()
        for kw in (dict(depth_ptrs=ptrs(zbs), depth_pitch_bytes=(W + 8) * 4, occluder_ptrs=ptrs(obs)), dict(depth_ptrs=ptrs(zbs), depth_pitch_bytes=(W + 8) * 4),
                   dict(occluder_ptrs=ptrs(obs))):
            with pytest.raises(MsplatError) as e:
                r.RenderStereoLayers(cams, [proj, proj], vp, nf, out_ptrs=ptrs(fbs), pitch_bytes=W * 16, **kw)
            assert e.value.code == _capi.ERR_UNSUPPORTED and word in r.last_error() and "msplat_render_stereo_layers" in r.last_error()
            assert untouched()
        r.RenderLayers(*view)                               # without planes it is the plain Render of that configuration: it works
        switch(False)
        same_bits(r.Render(*view), plain)
        got = host_frame(r, view, "clear", call=r.RenderLayers, depth=True, occluder=plane)
        same_bits(got[0], want[0]); same_bits(got[1], want[1])
    # half-given pairs of stereo planes
    for kw in (dict(depth_ptrs=[zbs[0].data_ptr(), None]), dict(depth_ptrs=[None, zbs[1].data_ptr()]), dict(occluder_ptrs=[obs[0].data_ptr(), None]),
               dict(occluder_ptrs=[None, obs[1].data_ptr()]), dict(depth_ptrs=ptrs(zbs), occluder_ptrs=[None, obs[1].data_ptr()])):
        with pytest.raises(MsplatError) as e:
            r.RenderStereoLayers(cams, [proj, proj], vp, nf, out_ptrs=ptrs(fbs), pitch_bytes=W * 16, depth_pitch_bytes=(W + 8) * 4, **kw)
        assert e.value.code == _capi.ERR_INVALID_ARG and "msplat_render_stereo_layers" in r.last_error() and "both" in r.last_error()
        assert untouched()
    # bad pitches of either plane, one view and two
    for pitch in (4 * W - 4, 4 * W + 2, 3):
        for kw, word in ((dict(depth_pitch_bytes=pitch), "depth pitch"), (dict(occluder_pitch_bytes=pitch), "occluder pitch")):
            with pytest.raises(MsplatError) as e:
                r.RenderLayers(*view, out_ptr=fbs[0].data_ptr(), pitch_bytes=W * 16, depth_ptr=zbs[0].data_ptr(), occluder_ptr=obs[0].data_ptr(), **kw)
            assert e.value.code == _capi.ERR_INVALID_ARG and word in r.last_error() and "msplat_render_layers" in r.last_error()
            with pytest.raises(MsplatError) as e:
                r.RenderStereoLayers(cams, [proj, proj], vp, nf, out_ptrs=ptrs(fbs), pitch_bytes=W * 16, depth_ptrs=ptrs(zbs), occluder_ptrs=ptrs(obs), **kw)
            assert e.value.code == _capi.ERR_INVALID_ARG and word in r.last_error() and "msplat_render_stereo_layers" in r.last_error()
            assert untouched()
    # the planes live where the colour does
    with pytest.raises(ValueError):
        r.RenderLayers(*view, out_ptr=fbs[0].data_ptr(), pitch_bytes=W * 16, occluder=plane)
    with pytest.raises(ValueError):
        r.RenderLayers(*view, occluder_ptr=obs[0].data_ptr())
    with pytest.raises(ValueError):
        r.RenderStereoLayers(cams, [proj, proj], vp, nf, depth_ptrs=ptrs(zbs))
    # Render itself keeps refusing both planes
    with pytest.raises(MsplatError) as e:
        r.Render(*view, depth=True, occluder=plane)
    assert e.value.code == _capi.ERR_UNSUPPORTED
    # and afterwards everything still works
    r.RenderLayers(*view, out_ptr=fbs[0].data_ptr(), pitch_bytes=W * 16, depth_ptr=zbs[0].data_ptr(), depth_pitch_bytes=(W + 8) * 4,
                   occluder_ptr=obs[0].data_ptr())
    r.synchronize()
    same_bits(fbs[0].cpu().numpy(), want[0]); same_bits(zbs[0].cpu().numpy()[:, :W].copy(), want[1])
    assert (zbs[0].cpu().numpy()[:, W:] == SENTINEL).all()
    same_bits(r.Render(*view), plain)


def test_point_clouds_have_no_layers_frame():
    pts = np.random.default_rng(81).uniform(-1, 1, (500, 8)).astype(np.float32)
    pts[:, 3] = 1.0
    pts[:, 4:] = np.abs(pts[:, 4:])
    L = _capi.lib()
    cfg = _capi.Config()
    cfg.struct_size = C.sizeof(_capi.Config)
    cfg.t_epsilon = -1.0
    h = C.c_void_p()
    assert L.msplat_create(C.byref(h), C.byref(cfg)) == _capi.OK
    assert L.msplat_upload_points(h, pts.ctypes.data, pts.shape[0], 32, 0, 16) == _capi.OK
    W, H = 64, 48
    fp = C.POINTER(C.c_float)
    a = [np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)) for x in scenes.default_view(W, H, z=4.0)]
    p = [x.ctypes.data_as(fp) for x in a]
    assert L.msplat_sort(h, *p) == _capi.OK
    img = [np.full((H, W, 4), SENTINEL, np.float32) for _ in range(2)]
    z, o = np.full((H, W), SENTINEL, np.float32), np.ones((H, W), np.float32)
    for d, oc in ((z.ctypes.data, o.ctypes.data), (z.ctypes.data, None), (None, o.ctypes.data)):
        assert L.msplat_render_layers(h, *p, img[0].ctypes.data, 0, d, 0, oc, 0, 0) == _capi.ERR_UNSUPPORTED
        assert b"point cloud" in L.msplat_last_error(h) and b"msplat_render_layers" in L.msplat_last_error(h)
        rc = L.msplat_render_stereo_layers(h, p[0], p[1], p[0], p[1], p[2], p[3], img[0].ctypes.data, img[1].ctypes.data, 0, d, d, 0, oc, oc, 0, 0)
        assert rc == _capi.ERR_UNSUPPORTED
        assert b"point cloud" in L.msplat_last_error(h) and b"msplat_render_stereo_layers" in L.msplat_last_error(h)
        assert (img[0] == SENTINEL).all() and (img[1] == SENTINEL).all() and (z == SENTINEL).all()
    assert L.msplat_render_layers(h, *p, img[0].ctypes.data, 0, None, 0, None, 0, 0) == _capi.OK         # no planes: msplat_render
    assert (img[0][..., 3] == 1.0).all()
    L.msplat_destroy(h)


def test_the_group_has_no_layers_frame():
    from splatapult_amd import SplatRendererGroup
    cloud, W, H, view = view_of("hard")
    g = SplatRendererGroup([0])
    assert g.Init(cloud), g.last_error()
    g.Sort(*view)
    want = g.Render(*view)
    with pytest.raises(MsplatError) as e:
        g.RenderLayers(*view, depth=True, occluder=np.ones((H, W), np.float32))
    assert e.value.code == _capi.ERR_UNSUPPORTED
    same_bits(g.Render(*view), want)
    g.close()
