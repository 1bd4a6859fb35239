"""GPU tests of the opt-in 8-bit storage of the higher-order SH (MSPLAT_STORAGE_SH_Q8).

The contract: an SH_Q8 cloud renders exactly what FP32 storage renders for the dequantised cloud (deq, tests/sh_q8_rule.py) --
same keys, same lists, same pixels bit for bit -- in every frame mode; the download returns deq of the upload on every route; a
non-finite f_rest value fails the upload; a degree-1 cloud stays FP32; and against FP32 storage of the original cloud a pixel
moves by at most the SH basis bound of the quantisation.

Sizes are the smallest that reach the code paths: 20 000 splats (V = 19 500, not a multiple of the 64-rank wave block) and 300 000
(Morton storage order and the box cull start at 262 144), at 640 x 360."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi, camera, synthetic
from splatapult_amd.renderer import SplatRendererGroup
from tests import scenes
from tests.checks import bits, same_bits
from tests.gpu_harness import assert_same_lists, sorted_frame
from tests.render_cases import AOS_OFF, ply_layout, sh_basis_bounds
from tests.sh_q8_rule import PLY_OF_REST, REST, deq, special_rest

pytestmark = pytest.mark.gpu

KEEP = [c for c in range(61) if c not in REST]
Q8 = _capi.STORAGE_SH_Q8


def view(yaw=0.3):
    return scenes.default_view(640, 360, z=7.0, yaw=yaw)


_CLOUDS = {}


def cloud(key):
    """(AoS cloud C, deq(C)), computed once and never written to"""
    if key not in _CLOUDS:
        n, full = {"small": (20_000, True), "reordered": (300_000, True), "deg1": (20_000, False)}[key]
        aos = synthetic.make_cloud(n, seed=0x5EED1234, full_sh=full, pos_sigma=1.5).as_array()
        d = deq(aos)
        aos.setflags(write=False)
        d.setflags(write=False)
        _CLOUDS[key] = (aos, d)
    return _CLOUDS[key]


def three_renders(key, v, make, prepare=None):
    """(SH_Q8 of C, FP32 of deq(C), FP32 of C) frames with renderers from make(cloud_storage=...)"""
    aos, d = cloud(key)
    out = []
    for storage, a in (("sh_q8", aos), ("fp32", d), ("fp32", aos)):
        r = make(cloud_storage=storage)
        assert r.Init(a, False, False), r.last_error()
        assert r.cloud_storage() == storage
        if prepare:
            prepare(r)
        out.append(sorted_frame(r, v))
        r.close()
    return out


# ---- 1. bit identity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,spatial", [("reordered", _capi.SPATIAL_ON), ("reordered", _capi.SPATIAL_OFF),
                                         ("small", _capi.SPATIAL_ON)])
def test_q8_renders_the_fp32_frame_of_the_dequantised_cloud(key, spatial):
    fq, fd, f32 = three_renders(key, view(), lambda **kw: SplatRenderer(device=0, spatial_order=spatial, **kw))
    assert fq["V"] > 1000
    if key == "small":
        assert fq["V"] % 64 != 0          # the last wave block of the projection is partly filled
    same_bits(fq["img"], fd["img"])
    assert_same_lists(fq, f32)
    assert (bits(fq["img"]) != bits(f32["img"])).any()       # (the quantisation is visible: the frames can differ at all)


def test_q8_bit_identity_on_an_rgba16f_target():
    fq, fd, f32 = three_renders("reordered", view(), lambda **kw: SplatRenderer(device=0, fb_format="fp16", **kw))
    assert fq["img"].dtype == np.float16 and fq["V"] > 1000
    same_bits(fq["img"], fd["img"])
    assert_same_lists(fq, f32)


# ---- 2. bit identity in the frame modes -----------------------------------------------------------------------------------
def test_q8_bit_identity_stereo_both_eyes():
    W, H = 256, 320
    proj = camera.perspective(camera.FOVY, W / H)
    cams = [camera.pose((-0.032, 0.0, 7.0), 0.3), camera.pose((0.032, 0.0, 7.0), 0.3)]
    vp = [0, 0, W, H]
    aos, d = cloud("reordered")
    outs = []
    for storage, a in (("sh_q8", aos), ("fp32", d)):
        r = SplatRenderer(device=0, fb_format="fp16", cloud_storage=storage)
        assert r.Init(a, False, False), r.last_error()
        assert r.cloud_storage() == storage
        r.Sort(cams[0], proj, vp, scenes.NF)
        assert r.sort_count() > 1000
        outs.append(r.RenderStereo(cams, [proj, proj], vp, scenes.NF))
        r.close()
    for eye in range(2):
        assert outs[0][eye].dtype == np.float16
        same_bits(outs[0][eye], outs[1][eye])


def test_q8_bit_identity_four_frames_in_flight():
    aos, d = cloud("reordered")
    views = [view(yaw=0.3 + 0.2 * k) for k in range(6)]
    frames = {}
    for name, storage, a in (("q8", "sh_q8", aos), ("deq", "fp32", d), ("c", "fp32", aos)):
        r = SplatRenderer(device=0, frames_in_flight=4, async_submit=True, cloud_storage=storage)
        assert r.Init(a, False, False), r.last_error()
        got = []
        for v in views:
            r.Sort(*v)
            got.append((r.Render(*v), r.sorted_keys(), r.sorted_indices(), r.sort_count()))
            # every context of the rotation renders the owner's storage
            assert r._lib.msplat_get_cloud_storage(r._ctx) == _capi.CLOUD_STORAGE_NAMES[storage]
        if name == "q8":
            assert [r._lib.msplat_get_cloud_storage(h) for h in r._ctxs] == [Q8] * 4
        frames[name] = got
        r.close()
    for k in range(len(views)):
        assert frames["q8"][k][3] > 1000
        same_bits(frames["q8"][k][0], frames["deq"][k][0])
        np.testing.assert_array_equal(frames["q8"][k][1], frames["c"][k][1])
        np.testing.assert_array_equal(frames["q8"][k][2], frames["c"][k][2])


def test_q8_bit_identity_banded_context():
    def prepare(r):
        r.set_band_layout(1, 0, 3, 4, band_cull=True)       # blocks of 3 bin rows from row 1, every 4th block
    fq, fd, f32 = three_renders("reordered", view(), lambda **kw: SplatRenderer(device=0, **kw), prepare)
    assert fq["V"] > 1000
    same_bits(fq["img"], fd["img"])
    assert_same_lists(fq, f32)


def test_q8_bit_identity_one_device_group():
    aos, d = cloud("reordered")
    imgs = []
    for storage, a in (("sh_q8", aos), ("fp32", d)):
        g = SplatRendererGroup([0], cloud_storage=storage)
        assert g.Init(a, False, False), g.last_error()
        assert g._lib.msplat_get_cloud_storage(g.context(0)) == _capi.CLOUD_STORAGE_NAMES[storage]
        g.Sort(*view())
        assert g.sort_count(0) > 1000
        imgs.append(g.Render(*view()))
        g.close()
    same_bits(imgs[0], imgs[1])


def test_q8_bit_identity_with_two_passes():
    # (the reordered cloud is large enough: with the mode forced and the share pinned the frame runs in two passes at
    #  300 000 splats -- pass 1 projects 15 % of the visible splats, pass 2 the listed splats behind the cut)
    aos, d = cloud("reordered")
    out = []
    for storage, a in (("sh_q8", aos), ("fp32", d), ("fp32", aos)):
        r = SplatRenderer(device=0, two_pass=_capi.TWO_PASS_ON, cloud_storage=storage)
        assert r.Init(a, False, False), r.last_error()
        r.two_pass_state(0.15)            # pin the first pass's share
        f = sorted_frame(r, view())
        f["tp"] = r.two_pass_info()
        out.append(f)
        r.close()
    fq, fd, f32 = out
    print("two-pass info:", fq["tp"])
    assert fq["tp"] is not None and fd["tp"] is not None and f32["tp"] is not None, "the frame did not run in two passes"
    assert 0 < fq["tp"]["splats_pass1"] < fq["V"], fq["tp"]
    assert fq["tp"] == f32["tp"]          # the passes split the frame like FP32 storage of C
    assert fq["V"] > 1000
    same_bits(fq["img"], fd["img"])
    # (with two passes, drawn / pairs describe the second pass: they too must match the FP32 frame of C)
    assert_same_lists(fq, f32)


# ---- 3. download ---------------------------------------------------------------------------------------------------------
def special_attrs(n=4096):
    """raw attributes whose f_rest holds special_rest()'s rows (in the record's order), each row at many splats"""
    a = synthetic.generate(n, seed=0x5EED0042, full_sh=True, pos_sigma=1.5)
    sp = special_rest()
    fr = np.array(a["f_rest"], np.float32, copy=True)
    reps = 40
    fr[:sp.shape[0] * reps, PLY_OF_REST] = np.tile(sp, (reps, 1))
    # ... and single special values among ordinary ones, at many f_rest positions
    vals = np.array([2.0 ** -65, -2.0 ** -64, 1e30, -0.0, 0.0, 63.5 / 127.0, -64.5 / 127.0, 1e-40], np.float32)
    tail = fr[sp.shape[0] * reps:sp.shape[0] * reps + 45 * vals.size]
    for k in range(tail.shape[0]):
        tail[k, k % 45] = vals[k // 45]
    a["f_rest"] = fr
    return a


def assert_equal_records(got, want):
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    np.testing.assert_array_equal(bits(got.astype(np.float32)), bits(want.astype(np.float32)))


def test_q8_download_is_deq_of_the_upload_on_every_route(tmp_path):
    a = special_attrs()
    n = a["xyz"].shape[0]
    gc = scenes.cloud_from_attrs(a, True)
    aos = gc.as_array()
    sp = special_rest()
    assert_equal_records(aos[:sp.shape[0], REST], sp)
    want = deq(aos)
    ply = str(tmp_path / "special.ply")
    synthetic.write_ply(ply, a)
    raw = np.fromfile(ply, np.uint8)
    body = raw[len(raw) - n * 248:].copy()

    def upload(route, storage):
        r = SplatRenderer(device=0, cloud_storage=storage)
        if route == "aos":
            assert r.Init(aos, False, False), r.last_error()
        elif route == "gaussian_cloud":
            assert r.Init(gc, False, False), r.last_error()
        elif route == "ply":
            assert r.InitFromPly(ply, True, False), r.last_error()
        else:
            assert r._create(False)
            L = ply_layout()
            _capi.check(r._ctx, r._lib.msplat_upload_ply_vertices(r._ctx, body.ctypes.data, n, C.byref(L), 1))
            r._n = n
        assert r.cloud_storage() == storage
        got = r.download_cloud(True)
        r.close()
        return got

    got = {(route, storage): upload(route, storage) for route in ("aos", "gaussian_cloud", "ply", "ply_vertices")
           for storage in ("sh_q8", "fp32")}
    assert_equal_records(got[("aos", "fp32")], aos)
    for route in ("aos", "gaussian_cloud", "ply", "ply_vertices"):
        q, f = got[(route, "sh_q8")], got[(route, "fp32")]
        assert_equal_records(q, deq(f))                          # the download is deq of what the route uploads
        assert_equal_records(q[:, KEEP], f[:, KEEP])             # the fp32 fields are the FP32 download's, bit for bit
        # the f_rest values are copied, not computed: the host routes and the ingest kernel store the same codes and steps
        assert_equal_records(q[:, REST], want[:, REST])
    assert_equal_records(got[("aos", "sh_q8")], want)
    assert (bits(want[:, REST]) != bits(aos[:, REST])).any()


# ---- 4. non-finite values ------------------------------------------------------------------------------------------------
def test_q8_upload_fails_on_non_finite_f_rest(tmp_path):
    aos = cloud("small")[0].copy()
    aos[7, 30] = np.nan
    aos[9, 6] = -np.inf
    aos[11, 60] = np.inf
    r = SplatRenderer(device=0, cloud_storage="sh_q8")
    assert not r.Init(aos, False, False)
    assert "3 f_rest values" in r.last_error(), r.last_error()
    c, p, v, nf = r._args.load(*view())
    assert r._lib.msplat_sort(r._ctx, c, p, v, nf) == _capi.ERR_NO_CLOUD
    assert r._lib.msplat_get_cloud_storage(r._ctx) == -1
    r.close()
    # the same cloud in FP32 storage is fine
    r = SplatRenderer(device=0)
    assert r.Init(aos, False, False), r.last_error()
    r.close()
    # the ingest route counts on the GPU
    a = synthetic.generate(2000, seed=0x5EED0042, full_sh=True, pos_sigma=1.5)
    a["f_rest"][5, 3] = np.inf
    ply = str(tmp_path / "nonfinite.ply")
    synthetic.write_ply(ply, a)
    r = SplatRenderer(device=0, cloud_storage="sh_q8")
    assert not r.InitFromPly(ply, True, False)
    assert "1 f_rest values" in r.last_error(), r.last_error()
    assert r._lib.msplat_sort(r._ctx, c, p, v, nf) == _capi.ERR_NO_CLOUD
    assert r._lib.msplat_get_cloud_storage(r._ctx) == -1
    r.close()
    r = SplatRenderer(device=0)
    assert r.InitFromPly(ply, True, False), r.last_error()
    r.close()


# ---- 5. degree 1 ---------------------------------------------------------------------------------------------------------
def test_q8_degree1_cloud_is_stored_fp32():
    aos = cloud("deg1")[0]
    assert aos.shape[1] == 25
    got = []
    for storage in ("sh_q8", "fp32"):
        r = SplatRenderer(device=0, cloud_storage=storage)
        assert r.Init(aos, False, False), r.last_error()
        assert r.cloud_storage() == "fp32"
        f = sorted_frame(r, view())
        f["bytes"] = r.stats()["device_bytes"]
        f["dl"] = r.download_cloud(False)
        got.append(f)
        r.close()
    assert got[0]["V"] > 1000
    assert got[0]["bytes"] == got[1]["bytes"]
    same_bits(got[0]["img"], got[1]["img"])
    assert_same_lists(got[0], got[1])
    np.testing.assert_array_equal(bits(got[0]["dl"]), bits(aos))


# ---- 6. reuse of one context ---------------------------------------------------------------------------------------------
def test_storage_switches_on_one_context_through_q8():
    aos = cloud("small")[0]
    n = aos.shape[0]
    fresh = {}
    for storage in ("fp32", "sh_q8", "sh_fp16"):
        r = SplatRenderer(device=0, cloud_storage=storage)
        assert r.Init(aos, False, False), r.last_error()
        fresh[storage] = sorted_frame(r, view())
        r.close()
    r = SplatRenderer(device=0)
    assert r.Init(aos, False, False), r.last_error()
    off = _capi.AttrOffsets(*AOS_OFF)
    seen = {}
    for storage in ("fp32", "sh_q8", "sh_fp16", "fp32"):
        _capi.check(r._ctx, r._lib.msplat_set_cloud_storage(r._ctx, _capi.CLOUD_STORAGE_NAMES[storage]))
        _capi.check(r._ctx, r._lib.msplat_upload_cloud(r._ctx, aos.ctypes.data, n, 61 * 4, C.byref(off), 1))
        assert r.cloud_storage() == storage
        f = sorted_frame(r, view())
        same_bits(f["img"], fresh[storage]["img"])
        assert_same_lists(f, fresh[storage])
        seen.setdefault(storage, []).append(r.stats()["device_bytes"])
    assert seen["fp32"][0] - seen["sh_q8"][0] == 128 * n, (seen, n)
    assert seen["fp32"][1] == seen["fp32"][0]
    assert r._lib.msplat_set_cloud_storage(r._ctx, 2) == _capi.ERR_INVALID_ARG
    assert r.cloud_storage() == "fp32"
    r.close()


def test_point_renderer_reports_fp32_with_kind_3():
    from splatapult_amd import PointRenderer
    rng = np.random.default_rng(5)
    pts = np.zeros((5000, 8), np.float32)
    pts[:, :3] = rng.normal(0.0, 1.0, (5000, 3))
    pts[:, 3] = 1.0
    pts[:, 4:7] = rng.uniform(0.0, 1.0, (5000, 3))
    pts[:, 7] = 1.0
    v = scenes.default_view(640, 360, z=5.0, yaw=0.3)
    imgs = []
    for storage in ("fp32", "sh_q8"):
        r = PointRenderer(device=0, cloud_storage=storage)
        assert r.Init(pts, False), r.last_error()
        assert r.cloud_storage() == "fp32"
        imgs.append(r.Render(*v))
        r.close()
    same_bits(imgs[0], imgs[1])


# ---- 7. colour bound -----------------------------------------------------------------------------------------------------
def colour_bound(aos, d):
    """max over splats and channels of sum_k beta_k |c_k - deq(c)_k|: a pixel is a convex combination of splat colours (and
    the background), each of which moves by at most its own sum"""
    beta = sh_basis_bounds()
    e = np.abs(aos.astype(np.float64) - d.astype(np.float64))
    tot = np.zeros(aos.shape[0])
    for c in range(3):
        # channel c: band 1 at floats 5+4c.., bands 2-3 at 25+12c..
        s = sum(beta[k] * e[:, 4 + 4 * c + k] for k in range(1, 4))
        s = s + sum(beta[k] * e[:, 25 + 12 * c + (k - 4)] for k in range(4, 16))
        tot = np.maximum(tot, s)
    return float(tot.max())


def test_q8_pixels_stay_within_the_sh_bound():
    aos, d = cloud("reordered")
    bound = colour_bound(aos, d) + 2.0 ** -20
    imgs = []
    for storage in ("sh_q8", "fp32"):
        r = SplatRenderer(device=0, cloud_storage=storage)
        assert r.Init(aos, False, False), r.last_error()
        f = sorted_frame(r, view())
        assert f["V"] > 1000
        imgs.append(f["img"].astype(np.float64))
        r.close()
    assert np.isfinite(imgs[0]).all() and np.isfinite(imgs[1]).all()
    moved = np.abs(imgs[0] - imgs[1])
    print("largest pixel movement %.6g, bound %.6g" % (moved.max(), bound))
    assert (moved <= bound).all(), (moved.max(), bound)
    assert moved.max() > 0.0             # the quantisation is visible at all (else the bound says nothing)
