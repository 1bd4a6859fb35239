"""The bin grid at its 8-bit limits: viewports of up to 8192 px = 256 bins of 32 px per axis.

Bin coordinates are bytes everywhere in the render path (a rectangle is tx0 | ty0 << 8 | tx1 << 16 | ty1 << 24, kRectEmpty is
"tx0 = 255 > tx1 = 0", the column pass has one thread and one LDS counter per bin column, its ballot rank sums nine bit planes of a
weight of up to 256 rows, the two-pass frames' summed-area table has (tiles_x + 1)(tiles_y + 1) <= 24576 uint16 entries, both
eyes share one chain while 2 tiles_y <= 256), and no other module renders a frame wider or taller than 4096 px.  Everything here
reaches index 255 with small frames: strips of 8192 x 64 and 64 x 8192 px (256 x 2 bins, 0.5 M pixels: scenes.strip_view /
scenes.strip_attrs, whose reach is asserted on the CPU by tests/test_bin_grid_fixtures.py), 64 x 4096 / 4128 for the stereo chain,
4160 x 4160 (130 x 130 bins: both coordinates above 127 at once, bin ids up to 16899) and 8192 x 3008 / 3040 (the largest
summed-area table and the first viewport beyond it).

References: the CPU oracle through check_image / check_fp16_image (tests/checks.py) and _check_projection / _expected_tile_lists
(tests/gpu_harness.py) with their caps unchanged, the depth oracle and tolerance of tests/test_gpu_depth_output.py, the point
oracle at the tolerance of test_point_renderer_matches_oracle; every other comparison is bit for bit.  Which regime ran (own waves /
persistent waves, one chain / two renders, one pass / two passes) is read from the library's taps and asserted, never assumed.

Measured image differences (-rP prints them per case):
  CPU, tiled front-to-back renderer vs the back-to-front oracle on the five strips: 100 % of values within 1e-4, mean |diff|
  2.1e-5, max 7.4e-5.
  MI355X, this module, fp32 frames of the four 8192-long strips: worst max |diff| 2.47e-3 (tall_synth; 1.40e-3 wide_synth, 1.2e-4
  and 7.9e-6 on the hard strips), worst mean 1.27e-6, >= 99.999 % of values within 1e-4; no pixel needed the flip budget.
  fp16 frames against the fp32 oracle: max |diff| 2.78e-4 on the strips, 5.81e-4 on rows 4096..4159 of the 4160 x 4160 frame.
  Depth plane: max |err| 2.75e-5.  Points on the tall strip: max |diff| 1.2e-7."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import MsplatError, _capi, camera, synthetic
from tests import scenes
from tests.checks import T_EPS, assert_is_a_plane, check_fp16_image, check_image, check_plane, same_bits
from tests.gpu_harness import (QUEUE_SENTINEL as SENTINEL, _check_projection, _expected_tile_lists, bin_edge, bin_px, device_frame, make_renderer,
                               no_sentinel, oracle_frame, stereo_frame, tap)
from tests.render_cases import BIN, NP_DTYPES, STRIPS, const_dst, depth_layers, random_dst, random_points, smooth_sprite, strip_case

pytestmark = pytest.mark.gpu

WORST = {"fp32_max": 0.0, "fp32_mean": 0.0, "fp16_max": 0.0}
STRIP_ITEMS = 4 * 256 * 2            # (bin, quadrant) work items of a 256 x 2 strip


def frozen(ref):
    for k in ("image", "budget", "splats", "sorted_idx", "sorted_keys"):
        ref[k].setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def strip_oracle(name):
    """oracle Sort + Render of a named strip, computed once and read-only (the clouds are small: stored in upload order, which
    every user asserts)"""
    cloud, W, H, (cam, proj, vp, nf) = strip_case(name)
    return frozen(oracle_frame(cloud.as_array(), True, cam, proj, vp, nf))


def sorted_strip(name, **kw):
    """(renderer after Sort, W, H, view)"""
    cloud, W, H, view = strip_case(name)
    r = make_renderer(cloud, **kw)
    assert r.storage_order() is None
    r.Sort(*view)
    return r, W, H, view


def decode(rect):
    rect = rect.astype(np.int64)
    return rect & 255, (rect >> 8) & 255, (rect >> 16) & 255, rect >> 24


def report(what, img, ref_image, key):
    d = np.abs(img[..., :3].astype(np.float64) - ref_image[..., :3])
    WORST[key + "_max"] = max(WORST[key + "_max"], d.max())
    if key == "fp32":
        WORST["fp32_mean"] = max(WORST["fp32_mean"], d.mean())
    print("%s: max |diff| %.3g, mean %.3g, within 1e-4: %.5f (module so far: fp32 max %.3g / mean %.3g, fp16 max %.3g)"
          % (what, d.max(), d.mean(), (d <= 1e-4).mean(), WORST["fp32_max"], WORST["fp32_mean"], WORST["fp16_max"]))


def test_the_bin_is_32_px():
    assert bin_px() == BIN


# ------------------------------------------------------------------------------------------------
# 1. projection, rectangles and tile lists, exact
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wide_hard", "tall_hard", "ragged_hard"])
def test_projection_rectangles_and_tile_lists_exact(name, monkeypatch):
    """8192 x 64, 64 x 8192 and 8191 x 33 (a ragged last bin at index 255 and a ragged second row: the smallest frames with 256 bins
    on an axis); the hard clouds hold rectangles over all 256 bins and rectangles that START in bin 255.  The lists of the default
    context (ranks from LDS atomics, scan-free passes) against the rectangles; those of the ballot ranking (rank_mode =
    MSPLAT_RANK_BALLOT: nine bit planes of a weight of up to 256 rows) and of the scan kernels against the default's"""
    r, W, H, view = sorted_strip(name)
    img = r.Render(*view)
    ref = strip_oracle(name)
    assert r.sort_count() == ref["V"]
    rect = _check_projection(r, ref, W, H)
    tx0, ty0, tx1, ty1 = decode(rect)
    drawn = tx0 <= tx1
    st = r.stats()
    tiles_x, tiles_y = st["tiles_x"], st["tiles_y"]
    assert (tiles_x, tiles_y) == ((W + BIN - 1) // BIN, (H + BIN - 1) // BIN) and max(tiles_x, tiles_y) == 256
    lo, hi = (tx0, tx1) if W > H else (ty0, ty1)
    starts_last = drawn & (lo == 255)
    print("%s: %d x %d bins, %d drawn of %d, highest bin index %d, widest rectangle %d bins, %d rectangle(s) start in bin 255, %d pairs"
          % (name, tiles_x, tiles_y, drawn.sum(), rect.size, hi[drawn].max(), (hi - lo + 1)[drawn].max(), starts_last.sum(), st["pairs"]))
    assert hi[drawn].max() == 255
    assert ((hi - lo)[drawn] == 255).any()              # bit 8 of the column pass's weight / all 256 columns of one rectangle
    assert starts_last.any()                            # tx0 = 255 with tx1 = 255 is a rectangle, not kRectEmpty
    assert not (rect[drawn] == 0x000000FF).any()
    ts, pairs = r.debug_tile_lists()
    exp = _expected_tile_lists(rect, tiles_x, tiles_y)
    assert st["pairs"] == sum(len(e) for e in exp)
    assert ts[-1] == st["pairs"]
    for t, e in enumerate(exp):
        got = pairs[ts[t]:ts[t + 1]] & 0xFFFFFF
        assert got.tolist() == e, "tile %d" % t
    for rank in np.flatnonzero(starts_last):            # ... and the binning did not take them for empty
        t = int(ty0[rank]) * tiles_x + int(tx0[rank])
        assert rank in (pairs[ts[t]:ts[t + 1]] & 0xFFFFFF)
    assert r.verify_order() == (0, 0)
    for kw, env in (({"rank_mode": _capi.RANK_BALLOT}, {}), ({"rank_mode": _capi.RANK_BALLOT}, {"MSPLAT_SCAN_KERNELS": "1"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rb, _, _, _ = sorted_strip(name, **kw)
        for k in env:
            monkeypatch.delenv(k)
        np.testing.assert_array_equal(rb.Render(*view), img)
        tsb, pairsb = rb.debug_tile_lists()
        np.testing.assert_array_equal(tsb, ts)
        np.testing.assert_array_equal(pairsb, pairs)
        assert rb.verify_order() == (0, 0)
        rb.close()


# ------------------------------------------------------------------------------------------------
# 2. frames against the oracle
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wide_synth", "tall_synth", "wide_hard", "tall_hard"])
def test_frames_match_the_oracle(name):
    """the four 8192-long strips in fp32 (check_image's caps as they are), the two hard ones also on an fp16 target; visible set,
    keys and draw order exact"""
    r, W, H, view = sorted_strip(name)
    img = r.Render(*view)
    ref = strip_oracle(name)
    assert r.sort_count() == ref["V"]
    np.testing.assert_array_equal(r.sorted_keys(), ref["sorted_keys"])
    np.testing.assert_array_equal(r.sorted_indices(), ref["sorted_idx"])
    report("%s fp32 %dx%d" % (name, W, H), img, ref["image"], "fp32")
    check_image(img, ref["image"], budget=ref["budget"])
    assert (img[..., :3] != 0).any(axis=-1).reshape(H // BIN, BIN, W // BIN, BIN).any(axis=(1, 3)).all()      # every bin drew something
    if STRIPS[name][5]:
        r16, _, _, _ = sorted_strip(name, fb_format="fp16")
        img16 = r16.Render(*view)
        report("%s fp16 %dx%d" % (name, W, H), img16, ref["image"], "fp16")
        check_fp16_image(img16, ref["image"], ref["budget"])


# ------------------------------------------------------------------------------------------------
# 3. everything that must be bit-identical, on one wide and one tall hard strip, device output
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wide_hard", "tall_hard"])
def test_short_pool_frames_equal_the_own_wave_frames(name):
    """compositor_waves = 64 against the default pool (2048 items: every item its own wave) for the splat compositor and the
    draw-order compositor of set_depth_test(24) (the point compositor: test_points_on_the_strips); the tap proves the regime"""
    cloud, W, H, view = strip_case(name)
    for depth_bits, kind in ((0, 0), (24, 1)):
        want = None
        for pool in (None, 64):
            r = make_renderer(cloud, compositor_waves=pool)
            r.set_depth_test(depth_bits)
            r.Sort(*view)
            for rep in range(2):
                img = device_frame(r, view, None, None, call=r.Render, **bin_edge())
                assert tap(r, pool, kind=kind, items=STRIP_ITEMS) == (pool is not None)
                no_sentinel(img)
                if want is None:
                    want = img
                same_bits(img, want, "%s depth %d pool %s frame %d" % (name, depth_bits, pool, rep))
            print("%s, depth test %d, pool %s: compositor launch (items, grid, ordered, kind) = %s" % (name, depth_bits, pool, r.compositor_launch()))
            r.close()
        assert (want[..., :3] != 0).any()


@functools.lru_cache(maxsize=None)
def dense_strip_cloud(W, H, seed):
    """a variant of the plain strip cloud for the two-pass tests: 120 000 splats, every one nearly opaque (logit 8), the half of
    the cloud on the high bin indices of the long axis 0.6 x its size, the other half 0.11 x.  The hard strips are no use there:
    their huge near splats finish EVERY bin in pass 1 at any share, and the tests want some bins finished and some carried over.
    Pass 1 composites whole batches of 64 list entries only, so a share of 1/64 has to put more than 64 splats on a bin before it
    can finish one -- hence the size.  Emulated on the CPU from the oracle's projection (the nearest whole batches of every bin's
    list, T < 2^-14 over the whole bin): 224 / 259 / 259 of the 512 bins of the wide strip finish with 1/64 / 0.3 / all of the
    visible splats in pass 1 (tall strip: 182 / 259 / 260), all of them at indices >= 126."""
    a = scenes.strip_attrs(120000, seed, W, H, False)
    high = a["xyz"][:, 0 if W > H else 1] > 0
    a["log_scale"][high] -= 0.5
    a["log_scale"][~high] -= 2.2
    a["opacity"][:] = 8.0
    return scenes.cloud_from_attrs(a)


@functools.lru_cache(maxsize=None)
def thin_strip_cloud(W, H, seed):
    """the plain strip cloud at 0.14 x its size: 71 % of the pixels keep a coverage below 0.99 (oracle, on the CPU), so what LOAD
    reads from the destination shows in the frame; the hard strips saturate nearly every pixel"""
    a = scenes.strip_attrs(40000, seed, W, H, False)
    a["log_scale"] -= 2.0
    return scenes.cloud_from_attrs(a)


@pytest.mark.parametrize("W,H,seed", [(8192, 64, 21), (64, 8192, 22)])
def test_forced_two_passes_equal_one_pass(W, H, seed):
    """pinned shares 1/64, 0.3 and 1.0 on the dense strip cloud (condition on the input, asserted from the library's own report:
    some bins finished by pass 1, some carried over -- the summed-area table has 257 columns or rows -- and at one share at least
    pass 2 dropped splats), and on the hard strip, where pass 1 finishes everything"""
    hard = strip_case("wide_hard" if W > H else "tall_hard")
    for what, cloud, view in (("dense", dense_strip_cloud(W, H, seed), scenes.strip_view(W, H)), ("hard", hard[0], hard[3])):
        a = make_renderer(cloud, two_pass=_capi.TWO_PASS_OFF)
        a.Sort(*view)
        want = device_frame(a, view, None, None, call=a.Render, **bin_edge())
        no_sentinel(want)
        assert a.two_pass_state()[0] == 0 and a.two_pass_info() is None
        dropped = []
        for share in (1.0 / 64.0, 0.3, 1.0):
            b = make_renderer(cloud, two_pass=_capi.TWO_PASS_ON)
            b.two_pass_state(share)
            b.Sort(*view)
            img = device_frame(b, view, None, None, call=b.Render, **bin_edge())
            same_bits(img, want, "%s %dx%d share %g" % (what, W, H, share))
            assert b.two_pass_state(share)[0] == 1
            info = b.two_pass_info()
            print("two passes, %s %dx%d, share %g: %s" % (what, W, H, share, info))
            assert info is not None and info["bins"] == 512 and info["visible"] == a.sort_count()
            if what == "dense":
                assert 0 < info["bins_unfinished"] < info["bins"], info
                dropped.append(info["splats_pass2"] < info["visible"] - info["splats_pass1"])
            assert b.verify_order() == (0, 0)
            b.close()
        assert what != "dense" or any(dropped)
        a.close()


BAND_LAYOUTS = {"tall_hard": [("interleaved", 1, 3), ("interleaved", 1, 7), ("interleaved", 1, 13), ("contiguous", 1, 8),
                              ("contiguous", 1, 16), ("block", 5, 3)],
                "wide_hard": [("interleaved", 1, 2)]}


@pytest.mark.parametrize("name", ["tall_hard", "wide_hard"])
def test_row_bands_reassemble_the_strip_bit_for_bit(name):
    """256 bin rows dealt to 3 ... 16 ranks (the tall strip; the wide one has two rows for two ranks), with and without the band
    cull: the loop of test_row_bands_reassemble_bit_exact on device targets -- a rank leaves the sentinel in every foreign row"""
    cloud, W, H, view = strip_case(name)
    R = (H + BIN - 1) // BIN
    base = make_renderer(cloud)
    base.Sort(*view)
    want = device_frame(base, view, None, None, call=base.Render, **bin_edge())
    no_sentinel(want)
    for kind, k, G in BAND_LAYOUTS[name]:
        for cull in (False, True):
            rb = make_renderer(cloud)
            got = np.full_like(want, SENTINEL)
            covered = np.zeros(H, bool)
            vs = []
            for g in range(G):
                lay = rb.set_band_plan(kind, R, G, g, block_rows=k, band_cull=cull)
                mine = _capi.band_rows(*lay, rows_full=R)
                rb.Sort(*view)
                vs.append(rb.sort_count())
                part = device_frame(rb, view, None, None, call=rb.Render, **bin_edge())
                rows = np.isin(np.arange(H) // BIN, mine)
                assert (part[~rows] == SENTINEL).all() and not (covered & rows).any()
                assert rb.stats()["tiles_y"] == len(mine)
                covered |= rows
                got[rows] = part[rows]
            assert covered.all()
            same_bits(got, want, "%s %s k %d G %d cull %s" % (name, kind, k, G, cull))
            print("%s: %s, blocks of %d, %d ranks, band cull %s: visible per rank %d ... %d of %d" % (name, kind, k, G, cull, min(vs), max(vs), base.sort_count()))
            rb.close()
    base.close()


@pytest.mark.parametrize("name", ["wide_hard", "tall_hard", "wide_thin", "tall_thin"])
def test_target_modes_on_a_pitched_target(name):
    """the identities of tests/test_gpu_target_mode.py::test_identities_between_the_modes (device_pitched_fp32), also on the thin
    strip cloud, most of whose pixels stay translucent"""
    if name.endswith("hard"):
        r, W, H, view = sorted_strip(name)
    else:
        W, H, seed = (8192, 64, 21) if name == "wide_thin" else (64, 8192, 22)
        view = scenes.strip_view(W, H)
        r = make_renderer(thin_strip_cloud(W, H, seed))
        r.Sort(*view)

    run = lambda mode, dst: device_frame(r, view, mode, dst, call=r.Render)         # (asserts that the padding keeps its bytes)
    zeros, opaque = const_dst(H, W, (0, 0, 0, 0)), const_dst(H, W, (0, 0, 0, 1))
    junk = random_dst(H, W, 5)
    clear = run("clear", junk)
    pre = run("premultiplied", junk)
    assert (clear[..., 3] == 1).all()
    np.testing.assert_array_equal(pre[..., :3], clear[..., :3])
    assert (pre[..., 3] >= 0).all() and (pre[..., 3] <= 1).all() and (pre[..., 3] < 1).any()
    print("%s: share of pixels with coverage below 0.99: %.3f" % (name, (pre[..., 3] < 0.99).mean()))
    assert name.endswith("hard") or (pre[..., 3] < 0.99).mean() > 0.5
    np.testing.assert_array_equal(run("load", zeros), pre)
    np.testing.assert_array_equal(run("load", opaque), clear)
    np.testing.assert_array_equal(run("clear", junk), clear)
    np.testing.assert_array_equal(clear, r.Render(*view))          # (the host frame of the same Sort)


@functools.lru_cache(maxsize=None)
def strip_depth_layers(name):
    _, W, H, _ = strip_case(name)
    return depth_layers(strip_oracle(name)["splats"], W, H, nthreads=16)


@pytest.mark.parametrize("name", ["wide_hard", "tall_hard"])
def test_depth_plane(name):
    """msplat_render_depth: the colour of msplat_render bit for bit; the plane against the depth oracle, check_plane's tolerance"""
    r, W, H, view = sorted_strip(name)
    plain = device_frame(r, view, None, None, call=r.Render, **bin_edge())
    img, z = device_frame(r, view, None, None, call=r.Render, depth=True, **bin_edge())
    same_bits(img, plain, "%s: the colour of a depth frame" % name)
    no_sentinel(z)
    assert_is_a_plane(z)
    L = strip_depth_layers(name)
    check_plane(z, L, T_EPS)
    assert (z[L["cover"] == 0.0] == 1.0).all() and (z < 1.0).any()


# ------------------------------------------------------------------------------------------------
# 4. stereo at the chain's limit
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,batched", [(4096, True), (4128, False)])
def test_stereo_at_the_limit_of_the_chain(H, batched):
    """64 x 4096: 2 x 128 = 256 virtual bin rows, the tallest viewport whose eyes share one chain; 64 x 4128: 129 rows per view,
    two renders.  Eyes 0.065 apart, a hard cloud squeezed into the strip (rectangles over all rows of a view, rectangles that start
    in its last row).  RenderStereo into device targets against one Render per eye, fp32 and fp16"""
    W = 64
    cloud = scenes.cloud_from_attrs(scenes.strip_attrs(20000, 12, W, H, True))
    cam, proj, vp, nf = scenes.strip_view(W, H)
    eyes = [camera.translate_local(cam, dx=-0.0325), camera.translate_local(cam, dx=+0.0325)]
    rows = (H + BIN - 1) // BIN
    one_view = 4 * 2 * rows
    for fmt in ("fp32", "fp16"):
        r = make_renderer(cloud, fb_format=fmt)
        r.Sort(eyes[0], proj, vp, nf)
        want = []
        for e in range(2):
            want.append(device_frame(r, (eyes[0], proj, vp, nf), None, None, call=r.Render, render_cam=eyes[e], **bin_edge(dtype=NP_DTYPES[fmt])))
            assert not tap(r, None, items=one_view)
            no_sentinel(want[-1])
        assert not np.array_equal(want[0], want[1])
        _, ty0, _, ty1 = decode(r.debug_projected()[1])           # (of the latest Render: the second eye)
        assert ty1.max() == rows - 1 and (ty1 - ty0).max() == rows - 1 and ty0.max() == rows - 1
        rs = make_renderer(cloud, fb_format=fmt)
        rs.Sort(eyes[0], proj, vp, nf)
        for rep in range(2):
            imgs = stereo_frame(rs, eyes, [proj, proj], vp, nf, None, None, call=rs.RenderStereo, **bin_edge(dtype=NP_DTYPES[fmt]))
            launch = rs.compositor_launch()
            assert launch[0] == (2 * one_view if batched else one_view) and launch[1] == launch[0], launch
            assert rs.stats()["tiles_y"] == (2 * rows if batched else rows)
            for e in range(2):
                same_bits(imgs[e], want[e], "64x%d %s frame %d eye %d" % (H, fmt, rep, e))
        print("64x%d %s: %s, compositor launch %s, tiles_y %d" % (H, fmt, "one chain" if batched else "two renders", launch, rs.stats()["tiles_y"]))
        assert rs.verify_order() == (0, 0)
        r.close(); rs.close()


# ------------------------------------------------------------------------------------------------
# 5. both coordinates above 127 at once
# ------------------------------------------------------------------------------------------------

def corner_cluster(a, W, H, k=4000, depth=3.0):
    """the first k splats of `a` become a cluster on the centre of the top-right 64 x 64 px of a W x H frame with the strips' focal
    length (4096 px): centres spread with sigma 17 px, nearly opaque, ~14 px in size and NEAR (depth 3 of a cloud around depth 7),
    so that the nearest 30 % of the visible splats hold all of them and pass 1 of a two-pass frame finishes the corner's bins
    (emulated on the CPU from the oracle's projection: 15 bins, those of the last two columns and rows among them)"""
    cx, cy = (W / 2 - 32.0) / 4096.0 * depth, (H / 2 - 32.0) / 4096.0 * depth
    a["xyz"][:k] = a["xyz"][:k] * (17.0 / 4096.0 * depth / 2.5) + np.array([cx, cy, 7.0 - depth], np.float32)
    a["log_scale"][:k] -= 1.0
    a["opacity"][:k] = 8.0
    return a


def corner_scene():
    """4160 x 4160 = 130 x 130 bins, the smallest square with tx >= 128 and ty >= 128: 20 000 splats spread over the frame and the
    4000 of corner_cluster"""
    W = H = 4160
    a = corner_cluster(synthetic.generate(24000, seed=31, pos_sigma=2.5, log_scale_mean=-3.6), W, H)
    view = (camera.pose((0.0, 0.0, 7.0)), camera.create_projection(-W / 8192.0, W / 8192.0, H / 8192.0, -H / 8192.0), [0, 0, W, H], scenes.NF)
    return scenes.cloud_from_attrs(a), W, H, view


def test_both_bin_coordinates_above_127():
    import torch
    cloud, W, H, view = corner_scene()
    cam, proj, vp, nf = view
    dev = torch.device("cuda", 0)

    def render(r):
        t = torch.full((H, W, 4), SENTINEL, dtype=torch.float16, device=dev)          # 138 MB
        torch.cuda.synchronize()
        r.Sort(*view)
        r.Render(*view, out_ptr=t.data_ptr(), pitch_bytes=W * 8)
        r.synchronize()
        return t

    a = make_renderer(cloud, fb_format="fp16", two_pass=_capi.TWO_PASS_OFF)
    assert a.storage_order() is None
    ta = render(a)
    st = a.stats()
    assert (st["tiles_x"], st["tiles_y"]) == (130, 130)
    launch = a.compositor_launch()
    assert launch[0] == 4 * 130 * 130 and launch[1] < launch[0], launch        # 67 600 items: persistent waves
    ref = oracle_frame(cloud.as_array(), True, cam, proj, vp, nf, row0=4096, row1=H)
    assert a.sort_count() == ref["V"]
    np.testing.assert_array_equal(a.sorted_indices(), ref["sorted_idx"])
    rect = _check_projection(a, ref, W, H)
    tx0, ty0, tx1, ty1 = decode(rect)
    drawn = tx0 <= tx1
    inside, reach = drawn & (tx0 >= 128) & (ty0 >= 128), drawn & (tx1 >= 128) & (ty1 >= 128)
    assert inside.sum() >= 100 and reach.sum() >= 2000 and tx1[drawn].max() == 129 and ty1[drawn].max() == 129
    ts, pairs = a.debug_tile_lists()
    exp = _expected_tile_lists(rect, 130, 130)
    assert st["pairs"] == sum(len(e) for e in exp) == ts[-1]
    for t, e in enumerate(exp):
        assert (pairs[ts[t]:ts[t + 1]] & 0xFFFFFF).tolist() == e, "tile %d" % t
    corner = [ty * 130 + tx for ty in (128, 129) for tx in (128, 129)]
    print("4160x4160: %d drawn, %d reach and %d lie inside the corner bins, corner lists %s, highest bin id with a list %d, compositor launch %s"
          % (drawn.sum(), reach.sum(), inside.sum(), [len(exp[t]) for t in corner], max(t for t, e in enumerate(exp) if e), launch))
    assert all(len(exp[t]) >= 100 for t in corner)
    assert a.verify_order() == (0, 0)
    # rows 4096 .. 4159 against the oracle
    got = ta[4096:].cpu().numpy()
    assert not (got == SENTINEL).any()
    report("4160x4160 fp16, rows 4096..4159", got, ref["image"][4096:], "fp16")
    check_fp16_image(got, ref["image"][4096:], ref["budget"][4096:])
    assert (got[:, 4096:, :3] != 0).any(axis=-1).mean() > 0.9
    # forced two passes
    b = make_renderer(cloud, fb_format="fp16", two_pass=_capi.TWO_PASS_ON)
    b.two_pass_state(0.3)
    tb = render(b)
    assert b.two_pass_state(0.3)[0] == 1
    info = b.two_pass_info()
    print("4160x4160 two passes, share 0.3: %s" % info)
    assert info is not None and info["bins"] == 16900
    assert 0 < info["bins_unfinished"] < info["bins"], info                 # the corner's bins finished: the table is not all ones
    assert info["splats_pass2"] < info["visible"] - info["splats_pass1"], info      # ... and the gate dropped splats behind them
    assert torch.equal(ta, tb)
    assert b.verify_order() == (0, 0)


# ------------------------------------------------------------------------------------------------
# 6. the largest summed-area table
# ------------------------------------------------------------------------------------------------

def test_the_largest_summed_area_table_and_the_first_viewport_beyond_it():
    """8192 x 3008 = 256 x 94 bins: 257 x 95 = 24415 <= 24576 entries, forced two passes run; 8192 x 3040: 257 x 96 = 24672, the
    same context renders in one pass.  The plain strip cloud plus corner_cluster at the top-right corner of the 3008-px frame, so
    that pass 1 finishes bins at column 255 / row 93.  Both against a one-pass context, bit for bit on the device (fp16 targets of 197 / 199 MB;
    the shape cannot be smaller: the table's size is the bin count).
    Time on the MI355X: 0.4 s for the test's call (nothing is downloaded and no oracle runs)"""
    import torch
    W = 8192
    cloud = scenes.cloud_from_attrs(corner_cluster(scenes.strip_attrs(40000, 41, W, 3040, False), W, 3008))
    a = make_renderer(cloud, fb_format="fp16", two_pass=_capi.TWO_PASS_OFF)
    b = make_renderer(cloud, fb_format="fp16", two_pass=_capi.TWO_PASS_ON)
    b.two_pass_state(0.3)
    dev = torch.device("cuda", 0)
    for H, two in ((3008, True), (3040, False)):
        view = scenes.strip_view(W, H)
        assert ((W // BIN + 1) * (H // BIN + 1) <= 24576) == two
        before = b.two_pass_state(0.3)[0]
        ts = []
        for r in (a, b):
            t = torch.full((H, W, 4), SENTINEL, dtype=torch.float16, device=dev)
            torch.cuda.synchronize()
            r.Sort(*view)
            r.Render(*view, out_ptr=t.data_ptr(), pitch_bytes=W * 8)
            r.synchronize()
            ts.append(t)
        st = b.stats()
        assert (st["tiles_x"], st["tiles_y"]) == (256, H // BIN)
        frames, info = b.two_pass_state(0.3)[0], b.two_pass_info()
        print("8192x%d: two-pass frames %d -> %d, info %s, compositor launch %s" % (H, before, frames, info, b.compositor_launch()))
        if two:
            assert frames == before + 1 and info is not None and info["frames"] > 0 and info["bins"] == 256 * 94
            # the cluster finished bins around (255, 93): the table's last entries are not simply the bin count
            assert 0 < info["bins_unfinished"] < info["bins"] and info["splats_pass2"] < info["visible"] - info["splats_pass1"], info
        else:
            assert frames == before and info is None
        assert a.two_pass_state()[0] == 0
        assert torch.equal(ts[0], ts[1])
        assert bool((ts[0][..., 3] == 1).all()) and bool((ts[0][..., :3] != 0).any())
        assert bool((ts[0][:, W - BIN:, :3] != 0).any())         # bin column 255 drew something
        del ts
    assert b.verify_order() == (0, 0)


# ------------------------------------------------------------------------------------------------
# 7. points
# ------------------------------------------------------------------------------------------------

def strip_points(W, H):
    """random_points(6000, 111) spread like the strip clouds (sigma 2.64) and squeezed into the strip"""
    pts = random_points(6000, 111)
    pts[:, :3] *= 2.2
    pts[:, 0 if H > W else 1] *= min(W, H) / max(W, H)
    return pts


@pytest.mark.parametrize("W,H", [(64, 8192), (8192, 64)])
def test_points_on_the_strips(W, H):
    """the sprite's size on screen depends on H alone: ~23 px on the tall strip -- compared with the point oracle at the tolerance
    of test_point_renderer_matches_oracle -- and below one pixel on the wide one, where only the draw order (exact) and the
    short-pool frame (equal to the own-wave frame, as on the tall strip) are asserted"""
    from splatapult_amd import PointRenderer
    pts, tex = strip_points(W, H), smooth_sprite(64, 48, seed=2)
    view = cam, proj, vp, nf = scenes.strip_view(W, H)
    ref = orc.points_frame(pts, tex, cam, proj, vp, nf, srgb=False, depth_bits=0)
    p = ref["pts"][ref["pts"]["reject"] == 0]
    along = p["cy"] if H > W else p["cx"]
    reached = np.unique((along[(along >= 0) & (along < 8192)] // BIN).astype(np.int64))
    print("points %dx%d: V %d, bins with a sprite centre %d, highest %d, median half size %.2f px" % (W, H, ref["V"], reached.size, reached.max(), np.median(p["hy"])))
    assert reached.max() == 255 and reached.size >= 250
    want = None
    for pool in (None, 64):
        r = PointRenderer(device=0, compositor_waves=pool)
        assert r.Init(pts, False, sprite=tex), r.last_error()
        for rep in range(2):
            img = device_frame(r, view, None, None, call=r.Render, **bin_edge())
            assert tap(r, pool, kind=2, items=STRIP_ITEMS) == (pool is not None)
            no_sentinel(img)
            if want is None:
                want = img
            same_bits(img, want, "points %dx%d pool %s frame %d" % (W, H, pool, rep))
        assert r.sort_count() == ref["V"]
        np.testing.assert_array_equal(r.sorted_indices(), ref["sorted_idx"])
        r.close()
    if H > W:
        assert (want[..., :3].sum(axis=-1) > 0).mean() > 0.01
        d = np.abs(want - ref["image"])[..., :3]
        print("points %dx%d: max |diff| %.3g, above 1e-5: %.6f" % (W, H, d.max(), (d > 1e-5).mean()))
        assert (d <= 1e-5).mean() >= 0.9999, (d > 1e-5).mean()
        assert d.max() <= 1e-3
        assert np.abs(want[..., 3] - 1.0).max() == 0


# ------------------------------------------------------------------------------------------------
# 8. the accepted edge
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", [True, False])
def test_8192_is_accepted_and_8193_refused(wide):
    """the strips of item 1 cropped to 32 px (256 x 1 bins); one pixel more is MSPLAT_ERR_UNSUPPORTED, by Sort and by Render, says
    why, and leaves the context rendering the valid frame's pixels"""
    name = "wide_hard" if wide else "tall_hard"
    cloud, yaw = strip_case(name)[0], STRIPS[name][2]
    ok = scenes.strip_view(8192, 32, yaw) if wide else scenes.strip_view(32, 8192, yaw)
    bad = scenes.strip_view(8193, 32, yaw) if wide else scenes.strip_view(32, 8193, yaw)
    r = make_renderer(cloud)
    r.Sort(*ok)
    want = r.Render(*ok)
    st = r.stats()
    assert sorted((st["tiles_x"], st["tiles_y"])) == [1, 256]
    _, _, tx1, ty1 = decode(r.debug_projected()[1])
    assert (tx1 if wide else ty1).max() == 255
    assert (want[..., :3] != 0).any() and (want[..., 3] == 1).all()
    for call in (r.Sort, r.Render):
        with pytest.raises(MsplatError) as e:
            call(*bad)
        assert e.value.code == _capi.ERR_UNSUPPORTED
        assert "8192" in r.last_error() and "8193" in r.last_error(), r.last_error()
        np.testing.assert_array_equal(r.Render(*ok), want)             # the latest valid Sort still stands
    r.Sort(*ok)
    np.testing.assert_array_equal(r.Render(*ok), want)
    assert r.verify_order() == (0, 0)
