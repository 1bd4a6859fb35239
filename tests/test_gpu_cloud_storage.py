"""GPU tests of the opt-in fp16 storage of the higher-order SH (msplat_set_cloud_storage).

The contract: an SH_FP16 cloud renders exactly what FP32 storage renders for the cloud whose f_rest values were rounded to fp16
(round16 below) -- same keys, same lists, same pixels bit for bit -- in every frame mode; the download returns round16 of the
upload on every route; values fp16 cannot hold fail the upload; and against FP32 storage of the original cloud a pixel moves by
at most the SH basis bound of the rounding."""
import ctypes as C
import os

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi, camera, synthetic
from splatapult_amd.renderer import SplatRendererGroup
from tests import scenes
from tests.checks import bits, same_bits
from tests.gpu_harness import assert_same_lists, sorted_frame
from tests.render_cases import AOS_OFF, ply_layout, sh_basis_bounds

pytestmark = pytest.mark.gpu

# f_rest columns of the reference record (61 floats: pos+alpha, r/g/b_sh0 = DC + band 1, Sigma, r/g/b_sh1..3 = bands 2-3);
# a degree-1 record (25 floats) has the first nine
REST = [5, 6, 7, 9, 10, 11, 13, 14, 15] + list(range(25, 61))


def round16(aos):
    """the cloud SH_FP16 storage renders: f_rest rounded to IEEE fp16 (nearest even), everything else unchanged"""
    out = np.array(aos, np.float32, copy=True)
    cols = REST if out.shape[1] == 61 else REST[:9]
    with np.errstate(over="ignore", invalid="ignore"):
        out[:, cols] = out[:, cols].astype(np.float16).astype(np.float32)
    return out


def cfg2_view(W=1920, H=1080, yaw=0.3):
    return scenes.default_view(W, H, z=7.0, yaw=yaw)


_CLOUDS = {}


def cloud(key):
    """AoS clouds of the benchmark's workloads (bench.WORKLOADS: cfg2 = cfg5's cloud; cfg3's for the two-pass case), cached"""
    if key not in _CLOUDS:
        if key == "cfg2":
            aos = synthetic.make_cloud(1_000_000, seed=0x5EED1234, full_sh=True, pos_sigma=1.5).as_array()
        elif key == "deg1":
            aos = synthetic.make_cloud(300_000, seed=0x5EED0001, full_sh=False, pos_sigma=1.5).as_array()
        elif key == "cfg3":
            aos = synthetic.make_cloud(6_000_000, seed=0x5EED6000, full_sh=True, pos_sigma=3.0).as_array()
        else:
            raise KeyError(key)
        _CLOUDS[key] = aos
    return _CLOUDS[key]


def three_renders(aos, view, make, prepare=None):
    """(SH_FP16 of C, FP32 of round16(C), FP32 of C) frames with renderers from make(cloud_storage=...)"""
    out = []
    for storage, a in (("sh_fp16", aos), ("fp32", round16(aos)), ("fp32", aos)):
        r = make(cloud_storage=storage)
        assert r.Init(a, False, False), r.last_error()
        assert r.cloud_storage() == storage
        if prepare:
            prepare(r)
        out.append(sorted_frame(r, view))
        r.close()
    return out


# ---- 1. bit identity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["cfg2", "deg1"])
@pytest.mark.parametrize("spatial", [_capi.SPATIAL_ON, _capi.SPATIAL_OFF])
def test_sh16_renders_the_fp32_frame_of_the_rounded_cloud(key, spatial):
    f16, fr, f32 = three_renders(cloud(key), cfg2_view(), lambda **kw: SplatRenderer(device=0, spatial_order=spatial, **kw))
    assert f16["V"] > 1000
    same_bits(f16["img"], fr["img"])
    assert_same_lists(f16, f32)


@pytest.mark.parametrize("key", ["cfg2", "deg1"])
def test_sh16_bit_identity_on_an_rgba16f_target(key):
    f16, fr, f32 = three_renders(cloud(key), cfg2_view(), lambda **kw: SplatRenderer(device=0, fb_format="fp16", **kw))
    assert f16["img"].dtype == np.float16
    same_bits(f16["img"], fr["img"])
    assert_same_lists(f16, f32)


def test_sh16_bit_identity_with_two_passes_on_6m():
    view = scenes.default_view(1920, 1080, z=12.0, yaw=0.3)
    out = []
    for storage, a in (("sh_fp16", cloud("cfg3")), ("fp32", round16(cloud("cfg3"))), ("fp32", cloud("cfg3"))):
        r = SplatRenderer(device=0, two_pass=_capi.TWO_PASS_ON, cloud_storage=storage)
        assert r.Init(a, False, False), r.last_error()
        r.two_pass_state(0.15)            # pin the first pass's share: both passes run
        f = sorted_frame(r, view)
        f["tp"] = r.two_pass_info()
        out.append(f)
        r.close()
    _CLOUDS.pop("cfg3")
    f16, fr, f32 = out
    assert f16["tp"] is not None and fr["tp"] is not None, "the frame did not run in two passes"
    same_bits(f16["img"], fr["img"])
    # (with two passes, drawn / pairs describe the second pass: they too must match the FP32 frame of C)
    assert_same_lists(f16, f32)


@pytest.mark.parametrize("key", ["cfg2", "deg1"])
def test_sh16_bit_identity_stereo_both_eyes(key):
    W, H = 2016, 2240
    proj = camera.perspective(camera.FOVY, W / H)
    cams = [camera.pose((-0.032, 0.0, 7.0), 0.3), camera.pose((0.032, 0.0, 7.0), 0.3)]
    vp = [0, 0, W, H]
    outs = []
    for storage, a in (("sh_fp16", cloud(key)), ("fp32", round16(cloud(key)))):
        r = SplatRenderer(device=0, fb_format="fp16", cloud_storage=storage)
        assert r.Init(a, False, False), r.last_error()
        r.Sort(cams[0], proj, vp, scenes.NF)
        outs.append(r.RenderStereo(cams, [proj, proj], vp, scenes.NF))
        r.close()
    for eye in range(2):
        same_bits(outs[0][eye], outs[1][eye])


def test_sh16_bit_identity_four_frames_in_flight():
    aos = cloud("cfg2")
    views = [cfg2_view(yaw=0.3 + 0.2 * k) for k in range(6)]
    frames = {}
    for storage, a in (("sh_fp16", aos), ("fp32", round16(aos)), ("fp32 of C", aos)):
        r = SplatRenderer(device=0, frames_in_flight=4, async_submit=True, cloud_storage=storage.split()[0])
        assert r.Init(a, False, False), r.last_error()
        assert r.cloud_storage() == storage.split()[0]
        got = []
        for v in views:
            r.Sort(*v)
            got.append((r.Render(*v), r.sorted_keys(), r.sorted_indices()))
            # every context of the rotation renders the owner's storage
            assert r._lib.msplat_get_cloud_storage(r._ctx) == _capi.CLOUD_STORAGES[storage.split()[0]]
        frames[storage] = got
        r.close()
    for k in range(len(views)):
        same_bits(frames["sh_fp16"][k][0], frames["fp32"][k][0])
        np.testing.assert_array_equal(frames["sh_fp16"][k][1], frames["fp32 of C"][k][1])
        np.testing.assert_array_equal(frames["sh_fp16"][k][2], frames["fp32 of C"][k][2])


def test_sh16_bit_identity_banded_context():
    def prepare(r):
        r.set_band_layout(1, 0, 3, 4, band_cull=True)       # blocks of 3 bin rows from row 1, every 4th block
    f16, fr, f32 = three_renders(cloud("cfg2"), cfg2_view(), lambda **kw: SplatRenderer(device=0, **kw), prepare)
    same_bits(f16["img"], fr["img"])
    assert_same_lists(f16, f32)


def test_sh16_bit_identity_one_device_group():
    aos = cloud("cfg2")
    view = cfg2_view()
    imgs = []
    for storage, a in (("sh_fp16", aos), ("fp32", round16(aos))):
        g = SplatRendererGroup([0], cloud_storage=storage)
        assert g.Init(a, False, False), g.last_error()
        assert g._lib.msplat_get_cloud_storage(g.context(0)) == _capi.CLOUD_STORAGES[storage]
        g.Sort(*view)
        imgs.append(g.Render(*view))
        g.close()
    same_bits(imgs[0], imgs[1])


# ---- 2. rounding ---------------------------------------------------------------------------------------------------------
SPECIAL = np.array([6e-8, 1e-6, -6e-8, 65504.0, -65504.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.0, 2.0 ** -25,
                    65519.0, np.inf, -np.inf, np.nan, 3.0e-5, -1.7e-7], np.float32)


def special_attrs(n=4096):
    a = synthetic.generate(n, seed=0x5EED0042, full_sh=True, pos_sigma=1.5)
    fr = np.array(a["f_rest"], np.float32, copy=True)
    fr.reshape(-1)[:SPECIAL.size * 40] = np.tile(SPECIAL, 40)       # every special value in many f_rest positions
    a["f_rest"] = fr
    return a


def assert_equal_records(got, want):
    """bit equality; NaN positions must agree (their payload is not part of the contract)"""
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    np.testing.assert_array_equal(bits(np.where(gn, 0, got).astype(np.float32)), bits(np.where(wn, 0, want).astype(np.float32)))


def download(r, full_sh=True):
    return r.download_cloud(full_sh)


def test_sh16_download_is_round16_of_the_upload_on_every_route(tmp_path):
    from splatapult_amd.scene import GaussianCloud
    a = special_attrs()
    gc = scenes.cloud_from_attrs(a, True)
    aos = gc.as_array()
    assert np.isin(SPECIAL[np.isfinite(SPECIAL)], aos[:, REST]).all()
    want = round16(aos)
    routes = {}
    for storage in ("sh_fp16", "fp32"):
        r = SplatRenderer(device=0, cloud_storage=storage)
        assert r.Init(aos, False, False), r.last_error()
        routes[(storage, "aos")] = download(r)
        r.close()
        r = SplatRenderer(device=0, cloud_storage=storage)
        assert r.Init(gc, False, False), r.last_error()
        routes[(storage, "gaussian_cloud")] = download(r)
        r.close()
    assert_equal_records(routes[("fp32", "aos")], aos)
    for route in ("aos", "gaussian_cloud"):
        got = routes[("sh_fp16", route)]
        assert_equal_records(got, want)
        # the fp32 fields are the FP32 download's, bit for bit
        keep = [c for c in range(61) if c not in REST]
        assert_equal_records(got[:, keep], routes[("fp32", route)][:, keep])
    # ... the golden PLY through the ingest kernel, and raw PLY vertices (the special values in f_rest)
    ply = str(tmp_path / "special.ply")
    synthetic.write_ply(ply, a)
    golden = os.path.join(os.path.dirname(__file__), "golden", "test.ply")
    for path in (golden, ply):
        got = {}
        for storage in ("sh_fp16", "fp32"):
            r = SplatRenderer(device=0, cloud_storage=storage)
            assert r.InitFromPly(path, True, False), r.last_error()
            assert r.cloud_storage() == storage
            got[storage] = download(r)
            r.close()
        assert_equal_records(got["sh_fp16"], round16(got["fp32"]))
    raw = np.fromfile(ply, np.uint8)
    body = raw[len(raw) - a["xyz"].shape[0] * 248:].copy()
    got = {}
    for storage in ("sh_fp16", "fp32"):
        r = SplatRenderer(device=0, cloud_storage=storage)
        assert r._create(False)
        L = ply_layout()
        _capi.check(r._ctx, r._lib.msplat_upload_ply_vertices(r._ctx, body.ctypes.data, a["xyz"].shape[0], C.byref(L), 1))
        r._n = a["xyz"].shape[0]
        got[storage] = download(r)
        r.close()
    assert_equal_records(got["sh_fp16"], round16(got["fp32"]))
    # (the f_rest values themselves are copied, not computed: every route stores the same halves)
    assert_equal_records(got["sh_fp16"][:, REST], want[:, REST])


def test_sh16_degree1_download_is_round16():
    aos = scenes.cloud_from_attrs(special_attrs(), False).as_array()
    assert aos.shape[1] == 25
    aos[:, REST[:9]] = np.resize(SPECIAL, (aos.shape[0], 9))
    r = SplatRenderer(device=0, cloud_storage="sh_fp16")
    assert r.Init(aos, False, False), r.last_error()
    assert_equal_records(download(r, False), round16(aos))


# ---- 3. range ------------------------------------------------------------------------------------------------------------
def test_sh16_upload_fails_beyond_the_fp16_range(tmp_path):
    aos = cloud("cfg2")[:20000].copy()
    aos[7, 30] = 7e4
    aos[9, 6] = -7e4
    aos[11, 40] = 65520.0                   # the first finite value that rounds to inf
    r = SplatRenderer(device=0, cloud_storage="sh_fp16")
    assert not r.Init(aos, False, False)
    assert "3 f_rest values" in r.last_error(), r.last_error()
    view = cfg2_view(640, 360)
    c, p, v, nf = r._args.load(*view)
    assert r._lib.msplat_sort(r._ctx, c, p, v, nf) == _capi.ERR_NO_CLOUD
    assert r._lib.msplat_get_cloud_storage(r._ctx) == -1
    r.close()
    # the same cloud in FP32 storage is fine; and the ingest route counts on the GPU
    r = SplatRenderer(device=0)
    assert r.Init(aos, False, False), r.last_error()
    r.close()
    a = special_attrs(2000)
    a["f_rest"][5, 3] = 7e4
    ply = str(tmp_path / "big.ply")
    synthetic.write_ply(ply, a)
    r = SplatRenderer(device=0, cloud_storage="sh_fp16")
    assert not r.InitFromPly(ply, True, False)
    assert "1 f_rest values" in r.last_error(), r.last_error()
    assert r._lib.msplat_sort(r._ctx, c, p, v, nf) == _capi.ERR_NO_CLOUD
    r.close()


# ---- 4. reuse of one context ---------------------------------------------------------------------------------------------
def test_storage_switches_on_one_context():
    aos = cloud("cfg2")
    n = aos.shape[0]
    view = cfg2_view()
    fresh = {}
    for storage in ("fp32", "sh_fp16"):
        r = SplatRenderer(device=0, cloud_storage=storage)
        assert r.Init(aos, False, False), r.last_error()
        fresh[storage] = sorted_frame(r, view)
        r.close()
    r = SplatRenderer(device=0)
    assert r.Init(aos, False, False), r.last_error()
    off = _capi.AttrOffsets(*AOS_OFF)
    seen = []
    for storage in ("fp32", "sh_fp16", "fp32"):
        kind = _capi.CLOUD_STORAGES[storage]
        _capi.check(r._ctx, r._lib.msplat_set_cloud_storage(r._ctx, kind))
        _capi.check(r._ctx, r._lib.msplat_upload_cloud(r._ctx, aos.ctypes.data, n, 61 * 4, C.byref(off), 1))
        assert r.cloud_storage() == storage
        f = sorted_frame(r, view)
        same_bits(f["img"], fresh[storage]["img"])
        assert_same_lists(f, fresh[storage])
        seen.append(r.stats()["device_bytes"])
    assert seen[0] - seen[1] == n * 96, (seen, n)
    assert seen[2] == seen[0]
    assert r._lib.msplat_set_cloud_storage(r._ctx, 2) == _capi.ERR_INVALID_ARG
    assert r.cloud_storage() == "fp32"
    r.close()


# ---- 5. magnitude --------------------------------------------------------------------------------------------------------
def colour_bound(aos):
    beta = sh_basis_bounds()
    d = np.abs(aos - round16(aos)).astype(np.float64)
    tot = np.zeros(aos.shape[0])
    for c in range(3):
        # channel c: band 1 at floats 5+4c.., bands 2-3 at 25+12c..
        s = sum(beta[k] * d[:, 4 + 4 * c + k] for k in range(1, 4))
        s = s + sum(beta[k] * d[:, 25 + 12 * c + (k - 4)] for k in range(4, 16))
        tot = np.maximum(tot, s)
    return float(tot.max())


@pytest.mark.parametrize("cfg", ["cfg2", "cfg5"])
def test_sh16_pixels_stay_within_the_sh_bound(cfg):
    aos = cloud("cfg2")             # (cfg5 renders cfg2's cloud as fp16 stereo 2016 x 2240)
    bound = colour_bound(aos) + 2.0 ** -20
    if cfg == "cfg2":
        view = cfg2_view()
        imgs = []
        for storage in ("sh_fp16", "fp32"):
            r = SplatRenderer(device=0, cloud_storage=storage)
            assert r.Init(aos, False, False), r.last_error()
            imgs.append([sorted_frame(r, view)["img"]])
            r.close()
    else:
        W, H = 2016, 2240
        proj = camera.perspective(camera.FOVY, W / H)
        cams = [camera.pose((-0.032, 0.0, 7.0), 0.3), camera.pose((0.032, 0.0, 7.0), 0.3)]
        imgs = []
        for storage in ("sh_fp16", "fp32"):
            r = SplatRenderer(device=0, fb_format="fp16", cloud_storage=storage)
            assert r.Init(aos, False, False), r.last_error()
            r.Sort(cams[0], proj, [0, 0, W, H], scenes.NF)
            imgs.append(r.RenderStereo(cams, [proj, proj], [0, 0, W, H], scenes.NF))
            r.close()
    for a16, a32 in zip(*imgs):
        a, b = a16.astype(np.float64), a32.astype(np.float64)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        tol = np.full(a.shape, bound)
        if a16.dtype == np.float16:
            # an fp16 target rounds both frames once more: one fp16 spacing at the pixel's magnitude on top
            tol = tol + np.spacing(np.maximum(np.abs(a16), np.abs(a32)).astype(np.float16)).astype(np.float64)
        d = np.abs(a - b)
        assert (d <= tol).all(), (d.max(), bound)
        assert d.max() > 0.0             # the rounding is visible at all (else the bound says nothing)


# ---- 6. point clouds -----------------------------------------------------------------------------------------------------
def test_point_clouds_ignore_the_storage_setting():
    from splatapult_amd import PointRenderer
    rng = np.random.default_rng(5)
    pts = np.zeros((5000, 8), np.float32)
    pts[:, :3] = rng.normal(0.0, 1.0, (5000, 3))
    pts[:, 3] = 1.0
    pts[:, 4:7] = rng.uniform(0.0, 1.0, (5000, 3))
    pts[:, 7] = 1.0
    view = scenes.default_view(640, 360, z=5.0, yaw=0.3)
    imgs = []
    for storage in ("fp32", "sh_fp16"):
        r = PointRenderer(device=0, cloud_storage=storage)
        assert r.Init(pts, False), r.last_error()
        assert r.cloud_storage() == "fp32"
        imgs.append((r.Render(*view), r.sorted_indices()))
        r.close()
    same_bits(imgs[0][0], imgs[1][0])
    np.testing.assert_array_equal(imgs[0][1], imgs[1][1])
