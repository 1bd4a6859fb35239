"""The compositors' persistent-wave work queue at small shapes.

Every compositor launch runs in one of two regimes (msplat_device.hip: comp_pool, ordered, cgrid): grid >= items -- every (bin, quadrant)
item has its own wave and no queue code runs -- or grid < items: persistent waves take their static item and pull more, composite_kernel
through the 32 sharded heads of queue_next (static share per shard from gridDim.x, two neighbours to steal from, the 8-bins x 4-quadrants
mapping for the first items & ~31 items and the plain one for the tail, bins in storage order), composite_depth_kernel and
composite_points_kernel through the single head of draw_order_walk.  Without msplat_config.compositor_waves the second regime needs
more than 20 480 items (8192 for the draw-order kernels): full-size frames only.  Here a pool of 64 ... items - 1 waves puts viewports
of 128 ... 2288 items on the queue, and the contract of msplat.h -- "pixels, keys and lists do not depend on any field below `stream`"
-- is checked bit for bit against the frame of a plain context (default pool, one frame at a time), which renders over the same target
contents where the mode reads them.

Which regime ran is not assumed: msplat_debug_get_compositor_launch (SplatRenderer.compositor_launch) reports items and grid of the
latest launch, and every test asserts grid < items on the short pool and grid == items on the baseline (96x64 has 24 items, fewer than the
smallest pool the library accepts: there grid == items is the correct answer and asserted instead).

What the targets hold decides what a faulty queue can hide behind.  An item never handed out leaves its pixels alone: the device targets
are filled with a sentinel no pixel can be (alpha is 1 or 1 - T) before EVERY frame, also between the repeated frames of one Sort.  An
item handed out twice writes the same pixels twice under MSPLAT_TARGET_CLEAR; under MSPLAT_TARGET_LOAD it blends twice over a
pseudo-random destination and differs.  The targets are one bin wider and taller than the viewport (pitch), and the padding keeps its
bits.  Nothing here is a measured number: comparisons are bit-exact, or use the tolerance of the test named beside them."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import camera
from tests import scenes
from tests.checks import bits, check_image, same_bits
from tests.gpu_harness import (MIN_POOL, QUEUE_SENTINEL as SENTINEL, Pitched, bin_edge, bin_px, device_frame, items_of, make_renderer, no_sentinel,
                               oracle_frame, pools_of, stereo_frame, tap)
from tests.render_cases import NP_DTYPES, random_points, smooth_sprite

pytestmark = pytest.mark.gpu

# viewport -> why: 308 items = 288 on the XCD mapping + a 20-item tail, ragged right and top tiles; 128 items, no tail; 24 items: fewer
# than 32 and than the minimum pool; 1144 items, the ragged case of test_compositor_both_targets_probe_and_work_counters
VIEWPORTS = [(333, 211), (256, 128), (96, 64), (701, 397)]
ORACLE_VIEWPORTS = [(333, 211), (701, 397)]
@functools.lru_cache(maxsize=None)
def the_cloud():
    return scenes.synth_cloud(30000, 7101, log_scale_mean=-3.0)      # long lists that vary a lot per tile


def view_of(W, H, k=0):
    return scenes.default_view(W, H, z=5.5, yaw=0.2 + 0.45 * k, x=0.05 * k)


@functools.lru_cache(maxsize=None)
def oracle_of(W, H):
    cam, proj, vp, nf = view_of(W, H)
    return oracle_frame(the_cloud().as_array(), True, cam, proj, vp, nf)


def random_target(W, H, fmt, seed):
    """a destination that is neither zero nor constant, in the target's format"""
    T = bin_px()
    a = np.random.default_rng(seed).random((H + T, W + T, 4), np.float32)
    return a.astype(np.float16) if fmt == "fp16" else a


# ------------------------------------------------------------------------------------------------
# the splat compositor (composite_kernel, queue_next)
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", VIEWPORTS)
def test_every_pool_renders_the_own_wave_frame(W, H):
    """viewports x pools, plain fp32 frames: one, two and three frames in a row from one Sort (the queue heads are cleared from inside
    the frame: the second frame tests that), one more after a new Sort with another camera; the pool-64 frame of the ragged viewports
    also against the CPU oracle, as test_compositor_both_targets_probe_and_work_counters does, so that the baseline is not the only
    referee"""
    cloud, items = the_cloud(), items_of(W, H)
    views = [view_of(W, H, 0), view_of(W, H, 1)]
    base = make_renderer(cloud)
    want = []
    for v in views:
        base.Sort(*v)
        want.append(device_frame(base, v, None, None, call=base.Render, **bin_edge()))
        assert not tap(base, None, items=items)
        no_sentinel(want[-1])
        assert (want[-1][..., :3] != 0).any()
    assert not np.array_equal(want[0], want[1])
    for pool in pools_of(items):
        r = make_renderer(cloud, compositor_waves=pool)
        r.Sort(*views[0])
        for rep in range(3):
            img = device_frame(r, views[0], None, None, call=r.Render, **bin_edge())
            assert tap(r, pool, items=items) == (items > MIN_POOL)
            same_bits(img, want[0], "%dx%d pool %d frame %d" % (W, H, pool, rep))
        if pool == 64 and (W, H) in ORACLE_VIEWPORTS:
            ref = oracle_of(W, H)
            check_image(img, ref["image"], budget=ref["budget"])
        r.Sort(*views[1])
        img = device_frame(r, views[1], None, None, call=r.Render, **bin_edge())
        assert tap(r, pool, items=items) == (items > MIN_POOL)
        same_bits(img, want[1], "%dx%d pool %d after a new Sort" % (W, H, pool))
        assert r.verify_order() == (0, 0)
        r.close()
    base.close()


@pytest.mark.parametrize("fmt,mode", [("fp16", "clear"), ("fp32", "premultiplied"), ("fp32", "load"), ("fp16", "load")])
def test_target_formats_and_modes_on_a_short_pool(fmt, mode):
    """pools 64 and 100 at every viewport: the fp16 target, the premultiplied layer, and "load" over a pseudo-random destination --
    the duplicate detector: a tile composited twice blends twice -- rendered twice in a row over the same destination"""
    cloud = the_cloud()
    for W, H in VIEWPORTS:
        items, v = items_of(W, H), view_of(W, H)
        fill = random_target(W, H, fmt, 11 * W + H) if mode == "load" else SENTINEL
        base = make_renderer(cloud, fb_format=fmt)
        base.set_target_mode(mode)
        base.Sort(*v)
        want = device_frame(base, v, None, None, call=base.Render, **bin_edge(fill=fill, dtype=NP_DTYPES[fmt]))
        assert not tap(base, None, items=items)
        no_sentinel(want)
        if mode == "load":
            assert (bits(want) != bits(fill[:H, :W])).mean() > 0.01      # the frame really went over the destination
        for pool in pools_of(items, short=True):
            r = make_renderer(cloud, fb_format=fmt, compositor_waves=pool)
            r.set_target_mode(mode)
            r.Sort(*v)
            for rep in range(2):
                img = device_frame(r, v, None, None, call=r.Render, **bin_edge(fill=fill, dtype=NP_DTYPES[fmt]))
                assert tap(r, pool, items=items) == (items > MIN_POOL)
                same_bits(img, want, "%s %s %dx%d pool %d frame %d" % (fmt, mode, W, H, pool, rep))
            r.close()
        base.close()


def test_depth_output_on_a_short_pool():
    """msplat_render_depth: colour and plane"""
    cloud = the_cloud()
    for W, H in VIEWPORTS:
        items, v = items_of(W, H), view_of(W, H)
        base = make_renderer(cloud)
        base.Sort(*v)
        want, zwant = device_frame(base, v, None, None, call=base.Render, depth=True, **bin_edge())
        assert not tap(base, None, items=items)
        no_sentinel(want)
        no_sentinel(zwant)
        assert zwant.min() >= 0.0 and zwant.max() <= 1.0 and (zwant < 1.0).any()
        for pool in pools_of(items, short=True):
            r = make_renderer(cloud, compositor_waves=pool)
            r.Sort(*v)
            for rep in range(2):
                img, z = device_frame(r, v, None, None, call=r.Render, depth=True, **bin_edge())
                assert tap(r, pool, items=items) == (items > MIN_POOL)
                same_bits(img, want, "colour %dx%d pool %d frame %d" % (W, H, pool, rep))
                same_bits(z, zwant, "depth plane %dx%d pool %d frame %d" % (W, H, pool, rep))
            r.close()
        base.close()


def test_both_eyes_in_one_chain_on_a_short_pool():
    """RenderStereo into device targets: one chain with doubled items (the second view's bin rows stacked on the first's), against one
    Render per eye on the plain context"""
    cloud = the_cloud()
    for W, H in VIEWPORTS:
        cam, proj, vp, nf = view_of(W, H)
        eyes = [camera.translate_local(cam, dx=-0.032), camera.translate_local(cam, dx=+0.032)]
        items = items_of(W, H, views=2)
        base = make_renderer(cloud)
        base.Sort(eyes[0], proj, vp, nf)
        want = []
        for e in range(2):
            want.append(device_frame(base, (eyes[0], proj, vp, nf), None, None, call=base.Render, render_cam=eyes[e], **bin_edge()))
            assert not tap(base, None, items=items // 2)
            no_sentinel(want[-1])
        assert not np.array_equal(want[0], want[1])
        for pool in pools_of(items, short=True) + ([1280] if items > 1280 else []):
            r = make_renderer(cloud, compositor_waves=pool)
            r.Sort(eyes[0], proj, vp, nf)
            for rep in range(2):
                imgs = stereo_frame(r, eyes, [proj, proj], vp, nf, None, None, call=r.RenderStereo, **bin_edge())
                assert tap(r, pool, items=items) == (items > MIN_POOL)
                for e in range(2):
                    same_bits(imgs[e], want[e], "%dx%d pool %d frame %d eye %d" % (W, H, pool, rep, e))
            r.close()
        base.close()


def test_row_bands_on_a_short_pool():
    """a banded context, set_band_plan("block", rows, 3, g, block_rows=2), reassembled as the scheduling lattice does.  A rank's items
    are those of its own rows: every rank runs persistent waves at 701x397 (440 / 352 / 352 items) and, with pool 64, at 333x211
    (132 / 88 / 88); the tap is checked for every rank that owns rows"""
    from splatapult_amd import _capi
    cloud, T = the_cloud(), bin_px()
    for W, H in VIEWPORTS:
        v = view_of(W, H)
        rows_full, tiles_x = (H + T - 1) // T, (W + T - 1) // T
        base = make_renderer(cloud)
        base.Sort(*v)
        want = device_frame(base, v, None, None, call=base.Render, **bin_edge())
        assert not tap(base, None, items=items_of(W, H))
        for pool in pools_of(items_of(W, H), short=True):
            got = np.full_like(want, SENTINEL)
            persistent = []
            for g in range(3):
                r = make_renderer(cloud, compositor_waves=pool)
                lay = r.set_band_plan("block", rows_full, 3, g, block_rows=2)
                mine = _capi.band_rows(*lay, rows_full=rows_full)
                r.Sort(*v)
                part = device_frame(r, v, None, None, call=r.Render, **bin_edge())
                rows = np.isin(np.arange(H) // T, mine)
                assert (part[~rows] == SENTINEL).all()               # a rank writes its own rows only
                got[rows] = part[rows]
                if mine:
                    persistent.append(tap(r, pool, items=4 * tiles_x * len(mine)))
                r.close()
            same_bits(got, want, "%dx%d pool %d" % (W, H, pool))
            if (W, H) == (701, 397) or ((W, H) == (333, 211) and pool == 64):
                assert persistent == [True, True, True], persistent
        base.close()


@pytest.mark.parametrize("share", [0.2, 1.0 / 64.0])
def test_two_pass_frames_on_a_short_pool(share):
    """both passes of a two-pass frame (composite_kernel<OCC = 1> and <OCC = 2>, whose item count is read on the device) on pools 64
    and 100; the tap reports the first pass"""
    from splatapult_amd import _capi
    cloud = the_cloud()
    for W, H in VIEWPORTS:
        items, v = items_of(W, H), view_of(W, H)
        base = make_renderer(cloud)
        base.Sort(*v)
        want = device_frame(base, v, None, None, call=base.Render, **bin_edge())
        assert not tap(base, None, items=items)
        assert base.two_pass_state()[0] == 0
        for pool in pools_of(items, short=True):
            r = make_renderer(cloud, compositor_waves=pool, two_pass=_capi.TWO_PASS_ON)
            r.two_pass_state(share)
            r.Sort(*v)
            for rep in range(2):
                img = device_frame(r, v, None, None, call=r.Render, **bin_edge())
                assert tap(r, pool, items=items) == (items > MIN_POOL)
                same_bits(img, want, "share %g %dx%d pool %d frame %d" % (share, W, H, pool, rep))
            assert r.two_pass_state()[0] > 0                         # both OCC passes ran on the short pool
            r.close()
        base.close()


def test_frames_in_flight_with_an_explicit_small_pool():
    """three contexts sharing the cloud, frames overlapped (nothing synchronises between them), pools 64 and 100"""
    cloud = the_cloud()
    for W, H in VIEWPORTS:
        items = items_of(W, H)
        views = [view_of(W, H, k) for k in range(5)]
        base = make_renderer(cloud)
        want = []
        for v in views:
            base.Sort(*v)
            want.append(device_frame(base, v, None, None, call=base.Render, **bin_edge()))
            assert not tap(base, None, items=items)
        for pool in pools_of(items, short=True):
            r = make_renderer(cloud, frames_in_flight=3, compositor_waves=pool)
            tg = [Pitched(H, W, np.float32, SENTINEL, pad=bin_px(), rows=bin_px()) for _ in views]
            for k, (cam, proj, vp, nf) in enumerate(views):
                r.Sort(cam, proj, vp, nf)
                r.Render(cam, proj, vp, nf, out_ptr=tg[k].ptr, pitch_bytes=tg[k].pitch)
            r.synchronize()
            assert tap(r, pool, items=items) == (items > MIN_POOL)
            for k in range(len(views)):
                same_bits(tg[k].read("frame %d" % k), want[k], "%dx%d pool %d frame %d" % (W, H, pool, k))
            r.close()
        base.close()


def test_probe_counts_the_same_work_on_a_short_pool():
    """the per-item probe at pool 64 and on the own-wave baseline: pixels unchanged, every sum of composite_work() that is not a clock
    equal, and word 7 of every work item whose 16x16 tile lies inside the image non-zero: the item ran.  (The persistent waves walk
    the bins in storage order, so item -> tile is the mapping of composite_kernel: the first items & ~31 items 8 bins x 4 quadrants,
    the tail plain.)"""
    import ctypes as C
    from splatapult_amd import _capi
    cloud, T = the_cloud(), bin_px()
    sums = ("work_items", "list_entries", "pair_words_fetched", "records_fetched", "records_composited", "pixel_evals", "batches",
            "useful_evals")

    def raw_probe(r, items):
        out = np.zeros((2 * items, 8), np.uint32)
        _capi.check(r._ctx, _capi.lib().msplat_debug_get_tile_probe8(r._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.shape[0]))
        assert not out[items:].any()
        return out[:items]

    for W, H in VIEWPORTS:
        items, v = items_of(W, H), view_of(W, H)
        tiles_x = (W + T - 1) // T
        inside_count = ((W + T // 2 - 1) // (T // 2)) * ((H + T // 2 - 1) // (T // 2))
        work = {}
        for pool in (None, 64):
            r = make_renderer(cloud, compositor_waves=pool)
            r.Sort(*v)
            img = device_frame(r, v, None, None, call=r.Render, **bin_edge())
            r.set_tile_probe(True)
            same_bits(device_frame(r, v, None, None, call=r.Render, **bin_edge()), img, "%dx%d pool %s: the probe changed pixels" % (W, H, pool))
            persistent = tap(r, pool, items=items)
            assert persistent == (pool is not None and items > MIN_POOL)
            work[pool] = (r.composite_work(), img)
            ran = raw_probe(r, items)[:, 7] != 0
            assert ran.sum() == inside_count == work[pool][0]["work_items"]
            if persistent:
                q = np.arange(items)
                mapped = q < (items & ~31)
                slot = np.where(mapped, (q >> 5) * 8 + (q & 7), q >> 2)
                quad = np.where(mapped, (q >> 3) & 3, q & 3)
                tx, ty = (slot % tiles_x) * 2 + (quad & 1), (slot // tiles_x) * 2 + (quad >> 1)
                inside = (tx * (T // 2) < W) & (ty * (T // 2) < H)
                assert (ran == inside).all(), "items that did not run: %s" % np.flatnonzero(ran != inside)[:16]
            r.close()
        same_bits(work[64][1], work[None][1], "%dx%d" % (W, H))
        for k in sums:
            assert work[64][0][k] == work[None][0][k], (W, H, k, work[64][0][k], work[None][0][k])
        assert work[None][0]["records_composited"] > 0


# ------------------------------------------------------------------------------------------------
# the draw-order compositors (draw_order_walk: a single queue head)
# ------------------------------------------------------------------------------------------------

DRAW_ORDER_CASES = [(24, None, "clear"), (24, "rgba8", "clear"), (24, "fp16", "clear"), (0, "rgba8", "clear"), (0, "fp16", "clear"),
                    (24, None, "load")]


@pytest.mark.parametrize("depth_bits,rop,mode", DRAW_ORDER_CASES)
def test_draw_order_compositor_on_a_short_pool(depth_bits, rop, mode):
    """emulated depth buffer x render-target rounding, and the depth test blending over a pseudo-random destination; the second eye
    drawn in the first eye's order, as in test_every_combination_of_the_render_target_emulations_gives_the_same_pixels; twice in a row"""
    cloud = the_cloud()
    for W, H in ORACLE_VIEWPORTS:
        items = items_of(W, H)
        cam, proj, vp, nf = view_of(W, H)
        v = (cam, proj, vp, nf)
        eye1 = camera.translate_local(cam, dx=0.064)
        fill = random_target(W, H, "fp32", 13 * W + H) if mode == "load" else SENTINEL
        want = None
        for pool in (None, 64):
            r = make_renderer(cloud, compositor_waves=pool)
            r.set_depth_test(depth_bits)
            r.set_target_emulation(rop)
            r.set_target_mode(mode)
            r.Sort(*v)
            for rep in range(2):
                img = device_frame(r, v, None, None, call=r.Render, render_cam=eye1, **bin_edge(fill=fill))
                assert tap(r, pool, kind=1, items=items) == (pool is not None)
                no_sentinel(img)
                if want is None:
                    want = img
                same_bits(img, want, "depth %d rop %s %s %dx%d pool %s frame %d" % (depth_bits, rop, mode, W, H, pool, rep))
            r.close()
        assert (want[..., :3] != 0).any()


def test_point_compositor_on_a_short_pool():
    """the scene of test_point_renderer_matches_oracle (srgb off, z = 5) with and without the depth test, pool 64 against the default
    pool; the depth-tested pool-64 frame also against the oracle with that test's tolerance"""
    from splatapult_amd import PointRenderer
    pts = random_points(6000, 111)
    tex = smooth_sprite(64, 48, seed=2)
    W, H = 640, 360
    v = scenes.default_view(W, H, z=5.0, yaw=0.3)
    items = items_of(W, H)
    for depth_bits in (0, 24):
        want = None
        for pool in (None, 64):
            r = PointRenderer(device=0, compositor_waves=pool)
            assert r.Init(pts, False, sprite=tex), r.last_error()
            r.set_depth_test(depth_bits)
            for rep in range(2):
                img = device_frame(r, v, None, None, call=r.Render, **bin_edge())      # (PointRenderer.Render sorts, then draws)
                assert tap(r, pool, kind=2, items=items) == (pool is not None)
                no_sentinel(img)
                if want is None:
                    want = img
                same_bits(img, want, "points, depth %d, pool %s, frame %d" % (depth_bits, pool, rep))
            r.close()
        if depth_bits == 24:
            ref = orc.points_frame(pts, tex, v[0], v[1], v[2], v[3], srgb=False, depth_bits=depth_bits)
            d = np.abs(img - ref["image"])[..., :3]
            assert (d <= 1e-5).mean() >= 0.9999, (d > 1e-5).mean()
            assert d.max() <= 1e-3
            assert np.abs(img[..., 3] - 1.0).max() == 0


# ------------------------------------------------------------------------------------------------
# timed contexts (msplat_config.enable_timing, msplat_get_timings: what bench.py reads)
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pool", [None, 64])
def test_timed_context_renders_the_same_pixels_and_reports_its_stages(pool):
    """enable_timing records events around the stages and launches composite_kernel with dispatch begin / end events: the baseline's
    pixels, and after three frames finite, non-negative stage times over >= 1 frame and >= 1 timed compositor launch.  No speed
    threshold"""
    import ctypes as C
    from splatapult_amd import _capi
    cloud = the_cloud()
    W, H = 333, 211
    items, v = items_of(W, H), view_of(W, H)
    base = make_renderer(cloud)
    base.Sort(*v)
    want = device_frame(base, v, None, None, call=base.Render, **bin_edge())
    assert not tap(base, None, items=items)
    base.close()
    r = make_renderer(cloud, enable_timing=True, compositor_waves=pool)
    for rep in range(3):
        r.Sort(*v)
        img = device_frame(r, v, None, None, call=r.Render, **bin_edge())
        assert tap(r, pool, items=items) == (pool is not None)
        same_bits(img, want, "timed context, pool %s, frame %d" % (pool, rep))
    t = _capi.Timings()
    _capi.check(r._ctx, _capi.lib().msplat_get_timings(r._ctx, C.byref(t)))
    for k in ("sort_total", "render_total", "project", "binning", "composite"):
        x = float(getattr(t, k))
        assert np.isfinite(x) and x >= 0.0, (k, x)
    assert t.reserved[0] >= 1 and t.reserved[2] >= 1, list(t.reserved)
    assert np.isfinite(t.reserved[1]) and t.reserved[1] >= 0.0
    r.close()
