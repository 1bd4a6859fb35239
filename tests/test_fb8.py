"""CPU tests of the 8-bit render targets MSPLAT_FB_RGBA8 / MSPLAT_FB_SRGB8_ALPHA8: the constants in the header and the binding, the
Python mirror's host arrays and constructor strings, and -- so that tests/fb8_rule.py cannot drift from the project's own
definition of the rule -- the rule against PresentRGBA8 (msplat_write_image) and against the scene the GPU tests lean on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, SplatRendererGroup, _capi, camera, renderer
from tests import fb8_rule
from tests.conftest import ROOT, has_gpu


def test_header_declares_the_formats_and_the_binding_mirrors_them():
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    m = re.search(r"enum\s*\{\s*MSPLAT_FB_RGBA32F\s*=\s*(\d+)\s*,\s*MSPLAT_FB_RGBA16F\s*=\s*(\d+)\s*,\s*MSPLAT_FB_RGBA8\s*=\s*(\d+)\s*,"
                  r"\s*MSPLAT_FB_SRGB8_ALPHA8\s*=\s*(\d+)\s*\}", header)
    assert m, "the MSPLAT_FB_* enum lacks the 8-bit formats"
    assert [int(v) for v in m.groups()] == [0, 1, 2, 3]
    assert (_capi.FB_RGBA32F, _capi.FB_RGBA16F, _capi.FB_RGBA8, _capi.FB_SRGB8_ALPHA8) == (0, 1, 2, 3)
    assert _capi.FB_FORMATS == {"fp32": 0, "fp16": 1, "rgba8": 2, "srgb8": 3}
    # the one place bytes per pixel come from
    m = re.search(r"#define MSPLAT_FB_BYTES_PER_PIXEL\(fb_format\) (.*)", header)
    assert m
    expr = m.group(1).replace("?", " and ").replace(":", " or ").replace("u", "")
    for fmt, bpp in ((0, 16), (1, 8), (2, 4), (3, 4)):
        assert eval(expr, {"fb_format": fmt, "MSPLAT_FB_RGBA32F": 0, "MSPLAT_FB_RGBA16F": 1}) == bpp
    # the contract is stated where an integrator reads it
    for word in ("MSPLAT_FB_RGBA8", "MSPLAT_FB_SRGB8_ALPHA8", "255.0f + 0.5f", "2^-10"):
        assert word in header, word
    assert "## 15" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_host_frame_is_uint8_and_refuses_other_arrays():
    vp = [0, 0, 8, 4]
    for fmt in (_capi.FB_RGBA8, _capi.FB_SRGB8_ALPHA8):
        a = renderer._host_frame(fmt, vp)
        assert a.dtype == np.uint8 and a.shape == (4, 8, 4) and not a.any()
        own = np.full((4, 8, 4), 7, np.uint8)
        assert renderer._host_frame(fmt, vp, own) is own and renderer._host_frame(fmt, vp, own, True) is own
        with pytest.raises(ValueError, match="out="):
            renderer._host_frame(fmt, vp, None, True)
        for load in (False, True):
            with pytest.raises(ValueError, match="uint8"):
                renderer._host_frame(fmt, vp, np.zeros((4, 8, 4), np.float32), load)
            with pytest.raises(ValueError, match="uint8"):
                renderer._host_frame(fmt, vp, np.zeros((4, 8, 4), np.int8), load)
            with pytest.raises(ValueError, match=r"\(4, 8, 4\)"):
                renderer._host_frame(fmt, vp, np.zeros((4, 8, 3), np.uint8), load)
            with pytest.raises(ValueError, match=r"\(4, 8, 4\)"):
                renderer._host_frame(fmt, vp, np.zeros((8, 4, 4), np.uint8), load)
            with pytest.raises(ValueError, match="contiguous"):
                renderer._host_frame(fmt, vp, np.zeros((4, 16, 4), np.uint8)[:, ::2], load)
    # the float formats as before, and a uint8 array is no float target
    assert renderer._host_frame(_capi.FB_RGBA32F, vp).dtype == np.float32 and renderer._host_frame(_capi.FB_RGBA16F, vp).dtype == np.float16
    with pytest.raises(ValueError, match="float32"):
        renderer._host_frame(_capi.FB_RGBA32F, vp, np.zeros((4, 8, 4), np.uint8))


def test_constructors_know_the_format_strings():
    for name, code in (("rgba8", _capi.FB_RGBA8), ("srgb8", _capi.FB_SRGB8_ALPHA8)):
        r = SplatRenderer(fb_format=name)
        g = SplatRendererGroup([0], fb_format=name)
        assert r._fb_format == code and g._fb_format == code
        cloud = np.zeros((4, 25), np.float32)
        if has_gpu():
            assert r.Init(cloud), r.last_error()
            assert _capi.lib().msplat_get_fb_format(r._ctx) == code
            r.close()
        else:       # past the argument checks: the existing no-device error
            assert not r.Init(cloud)
            assert "no HIP device" in r.last_error() and "no CPU fallback" in r.last_error()
            assert not g.Init(cloud)
            assert "no HIP device" in g.last_error()
    with pytest.raises(ValueError, match="fb_format"):
        SplatRenderer(fb_format="bgra8")
    # msplat_create knows exactly four formats
    L = _capi.lib()
    for bad in (-1, 4):
        cfg = _capi.Config()
        cfg.struct_size = C.sizeof(_capi.Config)
        cfg.t_epsilon = -1.0
        cfg.fb_format = bad
        h = C.c_void_p()
        rc = L.msplat_create(C.byref(h), C.byref(cfg))
        assert rc in (_capi.ERR_INVALID_ARG, _capi.ERR_NO_DEVICE) and not h.value
        if rc == _capi.ERR_INVALID_ARG:
            assert b"fb_format" in L.msplat_last_error(None)


def _ulp_neighbours(x):
    x = np.asarray(x, np.float32)
    return np.concatenate([np.nextafter(x, np.float32(-1)), x, np.nextafter(x, np.float32(2))])


def nasty_image():
    """values < 0, > 1, NaN, both infinities, exact code centres k / 255, one fp32 ulp either side of every (k + 0.5) / 255 -- and of
    the linear value of every sRGB boundary --, -0 and denormals; as an (H, 16, 4) image with every value in every channel"""
    k = np.arange(256, dtype=np.float32)
    edges = ((k[:255] + np.float32(0.5)) / np.float32(255.0)).astype(np.float32)
    e64 = (np.arange(255) + 0.5) / 255.0
    lin = np.where(e64 <= 0.04045, e64 / 12.92, ((e64 + 0.055) / 1.055) ** 2.4).astype(np.float32)
    vals = np.concatenate([
        np.array([-1.0, -1e-3, -0.0, 0.0, 1e-40, -1e-40, 1.0, 1.0 + 2.0 ** -23, 1.5, 3e38, np.nan, np.inf, -np.inf, 0.0031308, 0.00313081],
                 np.float32),
        (k / np.float32(255.0)).astype(np.float32), _ulp_neighbours(edges), _ulp_neighbours(lin),
        np.random.default_rng(3).uniform(-0.25, 1.25, 2000).astype(np.float32)])
    vals = np.resize(vals, ((vals.size + 15) // 16) * 16)
    img = np.empty((vals.size // 16, 16, 4), np.float32)
    for c in range(4):
        img[..., c] = np.roll(vals, 5 * c).reshape(-1, 16)
    return img


def test_present_rgba8_is_the_unorm_rule_byte_for_byte(tmp_path):
    img = nasty_image()
    camera.write_image(tmp_path / "lin.png", img, encode_srgb=False)
    got = camera.read_image(tmp_path / "lin.png")[::-1]          # the file's first row is the top one
    np.testing.assert_array_equal(got, fb8_rule.unorm8(img))
    # what the rule says about the special values, spelled out
    assert list(fb8_rule.unorm8(np.array([np.nan, -np.inf, np.inf, -0.0, 2.0, 0.4 / 255.0, 0.6 / 255.0], np.float32))) == [0, 0, 255, 0, 255, 0, 1]


def test_present_srgb_passes_the_acceptance_test(tmp_path):
    img = nasty_image()
    camera.write_image(tmp_path / "srgb.png", img, encode_srgb=True)
    got = camera.read_image(tmp_path / "srgb.png")[::-1]
    np.testing.assert_array_equal(got[..., 3], fb8_rule.unorm8(img[..., 3]))          # alpha is linear
    worst = fb8_rule.srgb_accept(got[..., :3], img[..., :3])
    exact = np.rint(255.0 * fb8_rule.srgb_encode64(img[..., :3])).astype(np.uint8)
    differs = got[..., :3] != exact
    near = fb8_rule.near_srgb_boundary(img[..., :3])
    print("PresentRGBA8 sRGB: worst %.6f of a code, %d of %d differ from rint(float64), %d near a boundary" % (
        worst, differs.sum(), differs.size, near.sum()))
    assert near.any() and not (differs & ~near).any()


def test_decode_tables_agree_and_round_trip():
    """the kernels' table (msplat_common.hip.h) is the rule's; a code decoded and encoded again is itself by the rule's own margin
    (the compositors do not rely on it: an untouched pixel of a LOAD frame is not stored at all)"""
    src = open(os.path.join(ROOT, "splatapult_amd", "csrc", "msplat_common.hip.h")).read()
    body = re.search(r"kSrgb8Decode\[256\] = \{(.*?)\};", src, flags=re.S).group(1)
    table = np.array([float(t.strip().rstrip("f")) for t in body.replace("\n", " ").split(",") if t.strip()], np.float64)
    assert table.size == 256
    want = fb8_rule.srgb_decode_table()
    np.testing.assert_array_equal(table.astype(np.float32), want)
    assert want[0] == 0 and want[255] == 1 and (np.diff(want) > 0).all()
    codes = np.arange(256, dtype=np.uint8)
    assert fb8_rule.srgb_error(codes, want).max() < 1e-4
    np.testing.assert_array_equal(fb8_rule.unorm8(fb8_rule.decode(codes[:, None].repeat(4, 1), False)), codes[:, None].repeat(4, 1))


def test_the_sparse_scene_exercises_both_clamps_every_code_and_few_boundaries():
    """fixture honesty: what the GPU tests assume about the "sparse" scene of tests/render_cases.py, on the CPU oracle"""
    from oracle import oracle as orc
    from tests.render_cases import view_of
    cloud, W, H, (cam, proj, vp, nf) = view_of("sparse")
    assert (W, H) == (517, 293)
    rgb = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=8)["image"][..., :3].astype(np.float32)
    above, below, zeros = (rgb > 1).sum(), (rgb < 0).sum(), (rgb == 0).sum()
    codes = np.unique(fb8_rule.unorm8(rgb))
    near = fb8_rule.near_srgb_boundary(rgb).sum()
    print("sparse: %d values above 1, %d below 0, %d zeros, %d codes, %d of %d within 2^-10 of an sRGB boundary" % (
        above, below, zeros, codes.size, near, rgb.size))
    assert above > 0 and below > 0 and zeros > 0 and codes.size == 256
    assert rgb.size == 454443 and near <= 0.005 * rgb.size
    # the fp32 and both formulations of the encode stay far inside the margin on these values
    v = fb8_rule.clamp01(rgb)
    with np.errstate(divide="ignore"):
        forms = (np.float32(1.055) * np.power(v, np.float32(1.0 / 2.4)) - np.float32(0.055),
                 np.float32(1.055) * np.exp2(np.log2(v) * np.float32(1.0 / 2.4)) - np.float32(0.055))
    for e in forms:
        e32 = np.where(v <= np.float32(0.0031308), np.float32(12.92) * v, e).astype(np.float32)
        assert np.abs(255.0 * e32.astype(np.float64) - 255.0 * fb8_rule.srgb_encode64(rgb)).max() < 2.0 ** -10 / 4
    # the other two scenes stay inside (0, 1): they alone would not test the clamps
    for name in ("hard", "dense"):
        cloud, W, H, (cam, proj, vp, nf) = view_of(name)
        img = orc.render_frame(cloud.as_array(), True, cam, proj, vp, nf, nthreads=8)["image"][..., :3]
        assert img.min() >= 0 and img.max() <= 1, (name, img.min(), img.max())
