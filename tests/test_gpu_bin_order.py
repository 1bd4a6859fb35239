"""Persistent compositor waves walk the bins in the XCD-local order (msplat_bin_order.h): same pixels, and the table follows the geometry.

A context with compositor_waves = 64 runs persistent waves from 65 work items on (tests/test_gpu_compositor_queue.py explains the two
regimes); msplat_debug_get_compositor_launch says which regime ran and msplat_debug_get_bin_order reads back the table that launch
walked.  Every frame is compared bit for bit with a context whose items each have their own wave (heaviest-first order, no table), into
targets one bin wider and taller than the viewport that hold a sentinel: a bin the table lost keeps the sentinel, a bin it names twice
is harmless under CLEAR and so the table itself is compared with the host function's (a permutation: tests/test_bin_order.py).
96 x 64 has 24 items, fewer than the smallest pool the library accepts: there every item has its own wave on both contexts, which is
asserted instead, and the table read back is the heaviest-first one."""
import ctypes as C
import functools

import numpy as np
import pytest

from splatapult_amd import _capi, camera
from tests import scenes
from tests.gpu_harness import MIN_POOL, bin_edge, bin_px, device_frame, items_of, make_renderer, no_sentinel, stereo_frame, tap

pytestmark = pytest.mark.gpu

VIEWPORTS = [(96, 64), (200, 136), (520, 264)]      # 3 x 2, 7 x 5 and 17 x 9 bins


@functools.lru_cache(maxsize=None)
def the_cloud():
    return scenes.synth_cloud(12000, 7101, log_scale_mean=-3.0)


def view_of(W, H):
    return scenes.default_view(W, H, z=5.5, yaw=0.2)


def grid_of(W, H, views=1):
    T = bin_px()
    return (W + T - 1) // T, ((H + T - 1) // T) * views


def host_table(tiles_x, rows):
    out = np.zeros(tiles_x * rows, np.uint32)
    assert _capi.lib().msplat_debug_bin_order(tiles_x, rows, out.ctypes.data_as(C.POINTER(C.c_uint32))) == _capi.OK
    return out


@functools.lru_cache(maxsize=None)
def own_wave_frame(W, H):
    """the frame of a plain context (every item on its own wave), computed once and left unchanged"""
    base, v = make_renderer(the_cloud()), view_of(W, H)
    base.Sort(*v)
    img = device_frame(base, v, None, None, call=base.Render, **bin_edge())
    assert not tap(base, None, items=items_of(W, H))
    no_sentinel(img)
    assert (img[..., :3] != 0).any()
    base.close()
    img.setflags(write=False)
    return img


def check_table(r, W, H, views=1):
    """the table the latest launch walked: the host function's for persistent waves, some permutation otherwise"""
    tiles_x, rows = grid_of(W, H, views)
    got = r.bin_order()
    assert got.shape[0] == tiles_x * rows
    if r.compositor_launch()[2] == 0:
        np.testing.assert_array_equal(got, host_table(tiles_x, rows))
    else:
        np.testing.assert_array_equal(np.sort(got), np.arange(tiles_x * rows, dtype=np.uint32))


@pytest.mark.parametrize("W,H", VIEWPORTS)
def test_persistent_waves_render_the_own_wave_frame(W, H):
    items, v = items_of(W, H), view_of(W, H)
    r = make_renderer(the_cloud(), compositor_waves=64)
    r.Sort(*v)
    for rep in range(2):
        img = device_frame(r, v, None, None, call=r.Render, **bin_edge())
        persistent = tap(r, 64, items=items)
        assert persistent == (items > MIN_POOL)
        assert r.compositor_launch()[2] == (0 if persistent else 1)      # unordered exactly when persistent
        np.testing.assert_array_equal(img, own_wave_frame(W, H))
        check_table(r, W, H)
    r.close()


def test_the_table_follows_the_geometry():
    r = make_renderer(the_cloud(), compositor_waves=64)
    for W, H in [(200, 136), (520, 264), (200, 136)]:
        v = view_of(W, H)
        r.Sort(*v)
        img = device_frame(r, v, None, None, call=r.Render, **bin_edge())
        assert tap(r, 64, items=items_of(W, H))
        np.testing.assert_array_equal(img, own_wave_frame(W, H))
        check_table(r, W, H)
    r.close()


def test_both_eyes_in_one_chain_walk_the_stacked_rows():
    W, H = 200, 136
    cam, proj, vp, nf = view_of(W, H)
    eyes = [camera.translate_local(cam, dx=-0.032), camera.translate_local(cam, dx=+0.032)]
    base = make_renderer(the_cloud())
    base.Sort(eyes[0], proj, vp, nf)
    want = [device_frame(base, (eyes[0], proj, vp, nf), None, None, call=base.Render, render_cam=eyes[e], **bin_edge()) for e in range(2)]
    assert not tap(base, None, items=items_of(W, H))
    base.close()
    assert not np.array_equal(want[0], want[1])
    r = make_renderer(the_cloud(), compositor_waves=64)
    r.Sort(eyes[0], proj, vp, nf)
    imgs = stereo_frame(r, eyes, [proj, proj], vp, nf, None, None, call=r.RenderStereo, **bin_edge())
    assert tap(r, 64, items=items_of(W, H, views=2))
    for e in range(2):
        np.testing.assert_array_equal(imgs[e], want[e])
    check_table(r, W, H, views=2)
    # ... and one view again on the same context: the table of 7 x 5 bins, not of 7 x 10
    img = device_frame(r, (eyes[0], proj, vp, nf), None, None, call=r.Render, **bin_edge())
    assert tap(r, 64, items=items_of(W, H))
    np.testing.assert_array_equal(img, want[0])
    check_table(r, W, H)
    r.close()


def test_two_pass_frame_pass_two_walks_the_unfinished_bins():
    W, H = 520, 264
    items, v = items_of(W, H), view_of(W, H)
    r = make_renderer(the_cloud(), compositor_waves=64, two_pass=_capi.TWO_PASS_ON)
    r.two_pass_state(0.2)
    r.Sort(*v)
    for rep in range(2):
        img = device_frame(r, v, None, None, call=r.Render, **bin_edge())
        assert tap(r, 64, items=items)
        np.testing.assert_array_equal(img, own_wave_frame(W, H))
    assert r.two_pass_state()[0] > 0                    # both passes ran
    info = r.two_pass_info()
    assert info is not None and info["bins"] == items // 4
    check_table(r, W, H)                                # the first pass's table; pass 2 walked its own list of unfinished bins
    r.close()
