"""What the GPU tests share that talks to a device: renderers, the oracle frame in a renderer's storage order, the projection
and tile-list checks, the compositor launch tap, and ONE frame harness -- host_frame, device_frame and stereo_frame issue a frame
through the library call they are handed (Render / RenderLayers, RenderStereo / RenderStereoLayers) and assert what every such
frame owes its caller: a pitched target's padding keeps its bytes, a separate occluder plane is read-only, a depth plane comes
back as float32 of the image's shape.  torch is imported inside the functions that need it.  pytest rewrites `assert` in test
modules only, so every assertion here carries its values in its message."""
import functools
import inspect

import numpy as np

from oracle import oracle as orc
from splatapult_amd import SplatRenderer
from tests.checks import CONIC_FLOOR, CONIC_RTOL, RGB_FLOOR, RGB_RTOL, same_bits
from tests.render_cases import oracle_rects, scene, view_of, window_depth

KK = -0.5 * 1.4426950408889634
WORST = {"conic": 0.0, "rgb": 0.0}      # the worst projection error of every _check_projection call of the process


def bin_px():
    from splatapult_amd import _capi
    return _capi.lib().msplat_tile_size()


def make_renderer(cloud, srgb=False, **kw):
    r = SplatRenderer(device=0, **kw)
    assert r.Init(cloud, srgb, False), r.last_error()
    return r


def sorted_renderer(name, fmt, **kw):
    cloud, W, H, view = view_of(name)
    r = make_renderer(cloud, fb_format=fmt, **kw)
    r.Sort(*view)
    return r, W, H, view


def subset_renderer(name_or_cloud, splats, level, **kw):
    """a context that holds only the splats with (the oracle's) z_w < level, in the upload order of the full cloud"""
    cloud = scene(name_or_cloud)[0] if isinstance(name_or_cloud, str) else name_or_cloud
    aos = cloud.as_array() if hasattr(cloud, "as_array") else cloud
    keep = np.sort(splats["index"][window_depth(splats) < level])
    return make_renderer(np.ascontiguousarray(aos[keep]), **kw), keep.shape[0]


@functools.lru_cache(maxsize=None)
def fp32_frame(name, mode):
    """the fp32 context's CLEAR / PREMULTIPLIED frame of a scene's view, computed once and left unchanged"""
    cloud, W, H, view = view_of(name)
    r = make_renderer(cloud)
    r.Sort(*view)
    img = host_frame(r, view, mode, call=r.Render)
    img.setflags(write=False)
    r.close()
    return img


_STORAGE_CACHE = {}


def storage_aos(r, aos):
    """(the cloud in the renderer's STORAGE order, the permutation slot -> upload index or None).  Large clouds are stored in
    Morton order (msplat_config.spatial_order) and splats with EQUAL depth keys are drawn in ascending storage slot: the
    reference's tie order is undefined (atomic slots, presort_compute.glsl:50); ours is reproduced by feeding the oracle the
    cloud in that order.  Everything the renderer reports is in upload numbering, so oracle indices are mapped with order[idx]."""
    order = r.storage_order()
    if order is None:
        return aos, None
    key = (aos.shape, float(aos[0, 0]), float(aos[-1, 5]), float(aos[aos.shape[0] // 2, 17]), int(order[:97].sum()), int(order[-97:].sum()))
    hit = _STORAGE_CACHE.get("last")
    if hit is None or hit[0] != key:
        _STORAGE_CACHE["last"] = hit = (key, np.ascontiguousarray(aos[order]))
    return hit[1], order


def oracle_frame(aos, full_sh, cam, proj, vp, nf, render_cam=None, render_proj=None, srgb=False, nthreads=16,
                 row0=0, row1=None, r=None):
    """oracle Sort + Render with the per-pixel threshold-flip budget: dict(V, image, budget, splats, sorted_*).
    r: the renderer whose storage order the oracle is to follow (storage_aos); sorted_idx comes back in upload numbering"""
    order = None
    if r is not None:
        aos, order = storage_aos(r, aos)
    ref = orc.render_frame(aos, full_sh, cam, proj, vp, nf, render_cam=render_cam, render_proj=render_proj, srgb=srgb,
                           nthreads=nthreads, want_image=False, want_splats=True)
    if order is not None:
        ref["sorted_idx"] = order[ref["sorted_idx"]]
    W, H = int(vp[2]), int(vp[3])
    ref["image"], ref["budget"] = orc.composite_flip(ref["splats"], W, H, nthreads=nthreads, row0=row0, row1=row1)
    return ref


def run_frame(cloud, view, full_sh=True, srgb=False, **kw):
    cam, proj, vp, nf = view
    r = make_renderer(cloud, srgb=srgb, **kw)
    r.Sort(cam, proj, vp, nf)
    img = r.Render(cam, proj, vp, nf)
    ref = oracle_frame(cloud.as_array(), full_sh, cam, proj, vp, nf, srgb=srgb, r=r)
    return r, img, ref


def sorted_frame(r, view):
    """Sort + Render, and what the frame's lists were"""
    r.Sort(*view)
    img = r.Render(*view)
    st = r.stats()
    return dict(img=img, keys=r.sorted_keys(), idx=r.sorted_indices(), V=r.sort_count(), drawn=st["drawn"], pairs=st["pairs"])


def assert_same_lists(a, b):
    assert a["V"] == b["V"], (a["V"], b["V"])
    np.testing.assert_array_equal(a["keys"], b["keys"])
    np.testing.assert_array_equal(a["idx"], b["idx"])
    assert (a["drawn"], a["pairs"]) == (b["drawn"], b["pairs"]), (a["drawn"], a["pairs"], b["drawn"], b["pairs"])


def mixed_plane(r, view, seed=0):
    """a plane with everything in it, for the bit-for-bit comparisons between execution shapes: four levels from the quantiles of
    the frame's own depth output (one call's output is another's input), that depth plane itself in one quadrant (varies per
    pixel), a NaN block, a +inf block and a closed (0.0) block"""
    r.set_target_mode("clear")
    _, z = r.Render(*view, depth=True)
    H, W = z.shape
    hit = z[z < 1.0]
    levels = np.quantile(hit, [0.2, 0.4, 0.6, 0.8]).astype(np.float32) if hit.size else np.full(4, 0.5, np.float32)
    plane = np.empty((H, W), np.float32)
    plane[:H // 2, :W // 2], plane[:H // 2, W // 2:], plane[H // 2:, :W // 2] = levels[0], levels[2], levels[3]
    plane[H // 2:, W // 2:] = z[H // 2:, W // 2:]
    plane[H // 3:H // 3 + 9, W // 5:W // 5 + 21] = np.nan
    plane[H // 4:H // 4 + 7, W // 2 - 10:W // 2 + 13] = np.inf
    plane[2 * H // 3:2 * H // 3 + 5, W // 3:W // 3 + 40] = 0.0
    plane[::7, ::5] = levels[1]
    return plane


# ---- projection and tile lists against the oracle ----------------------------------------------------------------------------

def _check_projection(r, ref, W, H):
    rec, rect = r.debug_projected()
    sp = ref["splats"]
    assert rec.shape[0] == sp.shape[0], (rec.shape, sp.shape)
    tx0, ty0, tx1, ty1 = rect & 255, (rect >> 8) & 255, (rect >> 16) & 255, rect >> 24
    drawn = tx0 <= tx1
    # a drawn splat is never one the geometry stage rejected
    assert not (drawn & (sp["reject"] != 0)).any(), "%d rejected splat(s) drawn" % (drawn & (sp["reject"] != 0)).sum()
    ok = sp["reject"] == 0
    np.testing.assert_allclose(rec[ok, 0], sp["px"][ok], atol=1e-3, rtol=0)
    np.testing.assert_allclose(rec[ok, 1], sp["py"][ok], atol=1e-3, rtol=0)
    inv = sp["inv"][ok]
    exp_conic = np.stack([KK * inv[:, 0], KK * (inv[:, 1] + inv[:, 2]), KK * inv[:, 3]], axis=1)
    # worst relative error over the splats (|x| below the absolute floor counts from the floor): printed (-rP shows it), so the
    # tolerance below is a measured one, not a guess
    def rel(a, b, floor):
        a, b = a.astype(np.float64), b.astype(np.float64)
        return float((np.abs(a - b) / np.maximum(np.abs(b), floor)).max()) if a.size else 0.0
    rc, rg = rel(rec[ok, 2:5], exp_conic, CONIC_FLOOR), rel(rec[ok, 6:9], sp["rgb"][ok], RGB_FLOOR)
    WORST["conic"], WORST["rgb"] = max(WORST["conic"], rc), max(WORST["rgb"], rg)
    print("projection parity: worst rel conic %.3g, colour %.3g over %d splats (suite so far: %.3g / %.3g)"
          % (rc, rg, int(ok.sum()), WORST["conic"], WORST["rgb"]))
    assert rc <= CONIC_RTOL, "conic rel error %.3g > %g" % (rc, CONIC_RTOL)
    assert rg <= RGB_RTOL, "colour rel error %.3g > %g" % (rg, RGB_RTOL)
    np.testing.assert_array_equal(rec[ok, 9], sp["alpha"][ok])
    # footprint: every pixel with w > 1/256 lies within rho*sqrt(cov_xx) of the centre; anything the oracle can light up must be drawn ...
    m, xs0, ys0, xs1, ys1 = oracle_rects(sp, W, H, bin_px())
    assert drawn[m].all(), "%d splat(s) the oracle can light up are not drawn" % (~drawn[m]).sum()
    covers = (tx0[m] <= xs0[m]) & (tx1[m] >= xs1[m]) & (ty0[m] <= ys0[m]) & (ty1[m] >= ys1[m])
    assert covers.all(), "%d rectangle(s) do not cover the oracle's footprint" % (~covers).sum()
    # ... and the rectangle is tight to within one tile
    tight = (xs0[m] - tx0[m] <= 1) & (tx1[m] - xs1[m] <= 1) & (ys0[m] - ty0[m] <= 1) & (ty1[m] - ys1[m] <= 1)
    assert tight.all(), "%d rectangle(s) are more than one tile wider than the oracle's footprint" % (~tight).sum()
    return rect


def _expected_tile_lists(rect, tiles_x, tiles_y):
    lists = [[] for _ in range(tiles_x * tiles_y)]
    for rank, rc in enumerate(rect.tolist()):
        tx0, ty0, tx1, ty1 = rc & 255, (rc >> 8) & 255, (rc >> 16) & 255, rc >> 24
        if tx0 > tx1:
            continue
        for ty in range(ty0, ty1 + 1):
            for tx in range(tx0, tx1 + 1):
                lists[ty * tiles_x + tx].append(rank)
    return lists


# ---- the compositor launch tap (tests/test_gpu_compositor_queue.py explains the two regimes) ---------------------------------

MIN_POOL = 64                     # msplat_create raises a smaller compositor_waves to this


def items_of(W, H, views=1):
    T = bin_px()
    return 4 * ((W + T - 1) // T) * ((H + T - 1) // T) * views


def pools_of(items, short=False):
    """64: the minimum; 100: no multiple of 32, the shards' static shares differ; items - 1: exactly one wave pulls once; 1280 (what
    contexts with frames in flight use) where it is below the item count.  short: the 64 / 100 cases only"""
    pools = [64, 100] if short else [64, 100, items - 1, 1280]
    return [p for i, p in enumerate(pools) if i < 2 or MIN_POOL < p < items]


def tap(r, pool, kind=0, items=None):
    """checks what the library reports about the context's latest compositor launch against the schedule its pool (None: the default)
    must give; True when the launch ran persistent waves (grid < items)"""
    n, grid, ordered, k = r.compositor_launch()
    assert k == kind, (k, kind)
    if items is not None:
        assert n == items, (n, items)
    want = n if pool is None else min(n, max(pool, MIN_POOL))
    assert grid == want, "items %d, pool %s: grid %d, expected %d" % (n, pool, grid, want)
    persistent = grid < n
    # persistent waves of the splat compositor walk the bins in storage order; everything else heaviest-first
    assert ordered == (0 if kind == 0 and persistent else 1), (n, grid, ordered, k)
    return persistent


# ---- the frame harness -------------------------------------------------------------------------------------------------------

SENTINEL = -123.0             # what float targets and planes hold where a frame must not write (exact in fp16 too)
PAD_COLOUR = 77               # the same for targets of any format, the 8-bit ones included
JUNK = "junk"                 # padding of NaN and 0 columns: what a kernel that read an occluder plane's padding would trip over
QUEUE_SENTINEL = -7.0         # what the work-queue tests' targets hold: no pixel can be it (alpha is 1 or 1 - T)


def bin_edge(fill=QUEUE_SENTINEL, **more):
    """harness arguments for targets one bin wider and taller than the viewport, holding QUEUE_SENTINEL (or `fill`, an array of
    the padded shape): an item never handed out leaves the sentinel in its pixels, an item handed out for pixels outside the
    viewport changes the padding"""
    T = bin_px()
    return dict(pad=T, dpad=T, rows=T, fill=fill, dfill=QUEUE_SENTINEL, **more)


def no_sentinel(img, sentinel=QUEUE_SENTINEL):
    assert not (img == sentinel).any(), "%d value(s) still hold the sentinel" % (img == sentinel).sum()


class Pitched:
    """A device image (H x W x 4) or plane (H x W) in rows of W + pad pixels, with `rows` more rows below.  The padding holds
    `fill`: a value, an array of the padded shape, or JUNK; the viewport's pixels hold `pixels` (an array or a value; None: what
    `fill` holds there).  .ptr and .pitch go to the library; read() returns the viewport's pixels after asserting that the padding
    kept its bytes, unchanged() asserts that for the whole array."""

    def __init__(self, H, W, dtype, fill, pixels=None, pad=0, rows=0, plane=False):
        import torch
        self.H, self.W = H, W
        host = np.zeros((H + rows, W + pad) if plane else (H + rows, W + pad, 4), dtype)
        if isinstance(fill, str):
            assert fill == JUNK and pixels is not None, (fill, pixels is None)
            host[:, W::2] = np.nan
        else:
            host[...] = fill
        if pixels is not None:
            host[:H, :W] = pixels
        self.before = host
        self.t = torch.from_numpy(host).to("cuda:0")
        torch.cuda.synchronize()                                # the upload has finished before the renderer's stream starts
        self.ptr, self.pitch = self.t.data_ptr(), (W + pad) * host.itemsize * (1 if plane else 4)

    def read(self, what):
        a, H, W = self.t.cpu().numpy(), self.H, self.W
        same_bits(a[H:], self.before[H:], "%s: rows beyond the viewport" % what)
        same_bits(a[:H, W:], self.before[:H, W:], "%s: the padding right of the viewport" % what)
        return np.ascontiguousarray(a[:H, :W])

    def unchanged(self, what):
        same_bits(self.t.cpu().numpy(), self.before, what)


def accepted(call, **kw):
    """the keyword arguments `call` takes; one it does not take must be a plane that was not given"""
    takes = inspect.signature(call).parameters
    for k, v in kw.items():
        assert k in takes or v is None or k.endswith("pitch_bytes"), "%s takes no %s" % (call.__name__, k)
    return {k: v for k, v in kw.items() if k in takes}


def host_frame(r, view, mode, dst=None, *, call, depth=None, occluder=None):
    """One host-output frame in `mode` (None: the mode the context is in) through call = r.Render or r.RenderLayers: the image,
    or (image, plane) with depth = True or the array to fill.  dst: what the colour array holds before (LOAD's destination).
    A separate occluder array is read-only; depth may BE the occluder array (in place)."""
    cam, proj, vp, nf = view
    if mode is not None:
        r.set_target_mode(mode)
    kw = {}
    if dst is not None:
        kw["out"] = np.ascontiguousarray(dst).copy()
    if depth is not None:
        kw["depth"] = depth
    if occluder is not None:
        kw["occluder"] = occluder
    keep = None if occluder is None or occluder is depth else occluder.copy()
    got = call(cam, proj, vp, nf, **kw)
    if keep is not None:
        same_bits(occluder, keep, "the occluder plane is read-only")
    if depth is None or depth is False:
        return got
    img, z = got
    assert z.dtype == np.float32 and z.shape == img.shape[:2], "the depth plane is %s %s, the image %s" % (z.dtype, z.shape, img.shape)
    return img, z


def device_targets(dst, dtype, H, W, depth, occluder, pad, zpad, dpad, rows, fill, dfill, zfill, in_place):
    """the pitched colour target, occluder plane (or None) and depth plane (or None; the occluder's memory in place) of one view"""
    if dst is not None:
        dtype = dst.dtype
    elif isinstance(fill, np.ndarray):
        dtype = fill.dtype
    fb = Pitched(H, W, dtype, fill, dst, pad, rows)
    ob = Pitched(H, W, np.float32, JUNK, occluder, zpad, rows, plane=True) if occluder is not None else None
    if in_place:
        assert depth and ob is not None, "in place: the depth plane is written into the occluder's memory"
        return fb, ob, ob
    zb = Pitched(H, W, np.float32, dfill, SENTINEL if zfill is None and isinstance(dfill, str) else zfill, dpad, rows, plane=True) if depth else None
    return fb, ob, zb


def read_targets(fb, ob, zb, what):
    """(image, plane or None) after the padding and read-only checks"""
    img = fb.read("%s: the colour target" % what)
    z = zb.read("%s: the depth plane" % what) if zb is not None else None
    if ob is not None and ob is not zb:
        ob.unchanged("%s: the occluder plane is read-only" % what)
    return img, z


def device_frame(r, view, mode, dst, *, call, depth=False, occluder=None, fill=SENTINEL, dfill=SENTINEL, pad=24, zpad=8, dpad=12,
                 rows=0, zfill=None, in_place=False, dtype=np.float32, render_cam=None):
    """One device-output frame in `mode` (None: the mode the context is in) through call = r.Render or r.RenderLayers, into a
    colour target whose rows are `pad` pixels wider than the image (and `rows` rows taller) and hold `fill` there; dst: the
    viewport's pixels before (None: `fill`, as `dtype`).  occluder: the plane, uploaded with zpad columns of JUNK.  depth: into a
    plane with dpad columns of `dfill`, whose pixels hold zfill before (None: dfill, or SENTINEL over JUNK); in_place: into the
    occluder's memory.  render_cam: the camera to draw with, where it is not the view's.  Returns the image, or (image, plane),
    after asserting that every padding kept its bytes and that a separate occluder plane did not change."""
    cam, proj, vp, nf = view
    fb, ob, zb = device_targets(dst, dtype, vp[3], vp[2], depth, occluder, pad, zpad, dpad, rows, fill, dfill, zfill, in_place)
    if mode is not None:
        r.set_target_mode(mode)
    call(cam if render_cam is None else render_cam, proj, vp, nf, out_ptr=fb.ptr, pitch_bytes=fb.pitch,
         **accepted(call, depth_ptr=zb.ptr if zb else None, depth_pitch_bytes=zb.pitch if zb else (vp[2] + dpad) * 4,
                    occluder_ptr=ob.ptr if ob else None, occluder_pitch_bytes=ob.pitch if ob else (vp[2] + zpad) * 4))
    r.synchronize()
    img, z = read_targets(fb, ob, zb, "mode %s" % mode)
    return (img, z) if depth else img


def stereo_frame(r, cams, projs, vp, nf, mode, dsts, *, call, depth=False, occluders=None, fill=SENTINEL, dfill=SENTINEL, pad=24,
                 zpad=8, dpad=12, rows=0, in_place=False, dtype=np.float32):
    """device_frame for both eyes of one call = r.RenderStereo or r.RenderStereoLayers, with device_frame's targets and checks per
    eye; dsts, occluders: a pair each, or None.  Returns [image0, image1], or ([image0, image1], [plane0, plane1])."""
    H, W = vp[3], vp[2]
    tg = [device_targets(dsts[e] if dsts is not None else None, dtype, H, W, depth, occluders[e] if occluders is not None else None,
                         pad, zpad, dpad, rows, fill, dfill, None, in_place) for e in range(2)]
    if mode is not None:
        r.set_target_mode(mode)
    call(cams, projs, vp, nf, out_ptrs=[t[0].ptr for t in tg], pitch_bytes=tg[0][0].pitch,
         **accepted(call, depth_ptrs=[t[2].ptr for t in tg] if depth else None, depth_pitch_bytes=tg[0][2].pitch if depth else (W + dpad) * 4,
                    occluder_ptrs=[t[1].ptr for t in tg] if occluders is not None else None,
                    occluder_pitch_bytes=tg[0][1].pitch if occluders is not None else (W + zpad) * 4))
    r.synchronize()
    got = [read_targets(*tg[e], "mode %s, eye %d" % (mode, e)) for e in range(2)]
    return ([g[0] for g in got], [g[1] for g in got]) if depth else [g[0] for g in got]
