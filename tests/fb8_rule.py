"""The value contract of the 8-bit render targets MSPLAT_FB_RGBA8 and MSPLAT_FB_SRGB8_ALPHA8 (include/msplat.h)
restated in numpy.  x is the fp32 value an MSPLAT_FB_RGBA32F context stores for the same frame.

  unorm rule (RGBA8: all four channels; SRGB8_ALPHA8: alpha): v = x > 0 ? (x > 1 ? 1 : x) : 0 -- NaN and -inf become 0, +inf
      becomes 1 --, code = (uint8)(v * 255.0f + 0.5f): an fp32 multiply, an fp32 add, truncation.  Exact: byte for byte.
  sRGB rule (SRGB8_ALPHA8: r g b): e = v <= 0.0031308 ? 12.92 v : 1.055 v^(1/2.4) - 0.055, then the same rounding of e.  A margin,
      not bits: with e in float64, |255 e - code| <= 0.5 + 2^-10 (a handful of fp32 roundings and two ~1-ulp transcendentals stay
      far below 64 ulp of a value <= 1, and 64 x 2^-24 x 255 ~ 2^-10 of a code).
  decode (MSPLAT_TARGET_LOAD's destination): d = (float)code / 255.0f; SRGB8_ALPHA8 r g b: c <= 0.04045 ? c / 12.92 :
      ((c + 0.055) / 1.055)^2.4 of that d, evaluated in float64 and rounded to fp32 once (the kernels' 256-entry table)."""
import numpy as np

MARGIN = 0.5 + 2.0 ** -10            # of a code


def clamp01(x):
    """float32 in, float32 out; NaN -> 0 (both comparisons are false for it, as in the C expression)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.where(x > 1, np.float32(1), x), np.float32(0)).astype(np.float32)


def unorm8(x):
    """the unorm rule in float32 arithmetic"""
    v = clamp01(x)
    return (v * np.float32(255.0) + np.float32(0.5)).astype(np.float32).astype(np.uint8)      # truncation: the values are >= 0


def srgb_encode64(x):
    """e of the sRGB rule, float64, from the clamped fp32 value"""
    v = clamp01(x).astype(np.float64)
    return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)


def srgb_error(codes, x):
    """|255 e - code| per value, in codes"""
    return np.abs(255.0 * srgb_encode64(x) - np.asarray(codes).astype(np.float64))


def srgb_accept(codes, x):
    """the sRGB acceptance test: every code within MARGIN of 255 e; returns the worst distance"""
    err = srgb_error(codes, x)
    assert err.max() <= MARGIN, "%d sRGB code(s) off by more than 0.5 + 2^-10 (worst %.6f)" % ((err > MARGIN).sum(), err.max())
    return err.max()


def near_srgb_boundary(x, width=2.0 ** -10):
    """values whose 255 e lies within `width` of a code boundary k + 0.5: the only ones where two evaluations may differ"""
    t = 255.0 * srgb_encode64(x)
    return np.abs(t - np.floor(t) - 0.5) <= width


def srgb_decode_table():
    """linear fp32 value of the 256 sRGB codes"""
    c = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float64)
    return np.where(c <= 0.04045, c / 12.92, np.power((c + 0.055) / 1.055, 2.4)).astype(np.float32)


def decode(codes, srgb):
    """(.., 4) uint8 -> float32 destination as the compositors read it"""
    codes = np.asarray(codes, np.uint8)
    d = (codes.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    if srgb:
        d[..., :3] = srgb_decode_table()[codes[..., :3]]
    return d


def check_frame(got, x, srgb, what=""):
    """an 8-bit frame against the rule applied to the fp32 frame x: RGBA8 byte for byte; SRGB8_ALPHA8 alpha byte for byte and r g b
    by the acceptance test.  Prints the figures before asserting"""
    assert got.dtype == np.uint8 and got.shape == x.shape, (got.dtype, got.shape, x.shape)
    if not srgb:
        want = unorm8(x)
        print("%s rgba8: %d of %d bytes differ" % (what, (got != want).sum(), want.size))
        np.testing.assert_array_equal(got, want, err_msg=what)
        return
    want_a = unorm8(x[..., 3])
    err = srgb_error(got[..., :3], x[..., :3])
    print("%s srgb8: worst |255 e - code| %.6f (margin %.6f), %d alpha bytes differ" % (what, err.max(), MARGIN, (got[..., 3] != want_a).sum()))
    np.testing.assert_array_equal(got[..., 3], want_a, err_msg=what + " alpha")
    srgb_accept(got[..., :3], x[..., :3])
