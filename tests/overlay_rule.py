"""The render-time overlay's rule (msplat_set_overlay*, include/msplat.h) in numpy float32 -- every operation rounded on its own,
nothing fused -- and the fixtures tests/test_overlay.py and tests/test_gpu_overlay.py share: palettes, classes and the SH-free
clouds.  numpy only: no device, no torch.  pytest rewrites `assert` in test modules only, so every assertion here carries its
values in its message."""
import numpy as np

from tests import scenes

SH_C0 = 0.28209479177387814
A_VALUES = (0.0, 2.0 ** -8, 0.5, 1.0)        # the a's of the palettes: no effect, barely there, half, replaced
COUNTS = (1, 3, 256)
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
W, H = 256, 160
RUN = 192                                     # splats in a row along the view axis: holds an aligned block of 64 draw-order ranks


def view(**kw):
    return scenes.default_view(W, H, **kw)


def entries(classes, palette):
    """per class byte the palette entry that applies: (h (n, 3), a (n,)) float32; a class >= count has a = 0"""
    palette = np.asarray(palette, np.float32).reshape(-1, 4)
    full = np.zeros((256, 4), np.float32)
    full[:palette.shape[0]] = palette
    e = full[np.asarray(classes).astype(np.uint8)]
    return e[:, :3], e[:, 3]


def tint(c, classes, palette):
    """the rule over colour lanes c (n, 3) float32 of splats with `classes` (n,): t = 1 - a; c' = (t * c) + (a * h), four float32
    operations; lanes of a splat with a == 0 keep their bits"""
    c = np.asarray(c)
    assert c.dtype == np.float32 and c.ndim == 2 and c.shape[1] == 3, "colour lanes are (n, 3) float32, not %s %s" % (c.dtype, c.shape)
    h, a = entries(classes, palette)
    with np.errstate(all="ignore"):
        t = np.float32(1.0) - a
        p = t[:, None] * c
        q = a[:, None] * h
        out = p + q
    assert t.dtype == p.dtype == q.dtype == out.dtype == np.float32, "the rule left float32"
    return np.where((a != 0)[:, None], out, c)


def tint_f64(c, classes, palette):
    """the same in float64, nothing rounded: (c', |t c|, |a h|)"""
    h, a = entries(classes, palette)
    a, h, c = a.astype(np.float64)[:, None], h.astype(np.float64), np.asarray(c, np.float64)
    return (1.0 - a) * c + a * h, np.abs((1.0 - a) * c), np.abs(a * h)


def palette(count, seed=0):
    """count entries (h_r, h_g, h_b, a): colours in [-0.25, 1.25], a cycling through A_VALUES from entry 0 on (entry 0 has no effect);
    a single entry has a = 0.5"""
    rng = np.random.default_rng(1000 + 7 * count + seed)
    p = rng.uniform(-0.25, 1.25, (count, 4)).astype(np.float32)
    p[:, 3] = np.resize(np.array(A_VALUES, np.float32), count) if count > 1 else 0.5
    return p


GREY = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.5, 1.0]], np.float32)      # class 1: exactly what zero SH project to (non-sRGB)


def classes(aos, count, seed=0):
    """one class per splat of `aos`: random over 0, 1, count - 1, count, 255 and everything between, each of those five present from
    five splats on; from 2 RUN + 64 splats on, the RUN splats farthest down the -z axis have no effect (class `count`, or 0 for a
    full palette) and the RUN after them all have a class with a != 0: seen from +z, a block of 64 ranks of either kind"""
    n = aos.shape[0]
    rng = np.random.default_rng(2000 + 13 * count + seed)
    cls = rng.integers(0, 256, n).astype(np.uint8)
    low = rng.random(n) < 0.6                                  # most splats inside the palette
    cls[low] = rng.integers(0, count, int(low.sum())).astype(np.uint8)
    special = np.array([0, 1, count - 1, min(count, 255), 255], np.int64).clip(0, 255).astype(np.uint8)
    if n >= special.size:
        cls[rng.choice(n, special.size, replace=False)] = special
    if n >= 2 * RUN + 64:
        far = np.argsort(aos[:, 2], kind="stable")
        cls[far[:RUN]] = count if count < 256 else 0
        cls[far[RUN:2 * RUN]] = tinted_class(count)
    return cls


def tinted_class(count):
    """a class whose palette(count) entry has a != 0"""
    return 0 if count == 1 else 1


def selection(n, seed=0, share=0.4):
    """a bool selection, as msplat_mark_ids writes one with value = 1: class 1 of GREY"""
    return np.random.default_rng(3000 + seed).random(n) < share


def cloud(n, seed=0, full_sh=True, **kw):
    """n synthetic splats around the origin as an (n, 61 / 25) float32 array"""
    return np.ascontiguousarray(scenes.synth_cloud(n, 400 + seed + n, full_sh=full_sh, **dict(dict(log_scale_mean=-2.2), **kw)).as_array())


def sh_floats(width):
    """the columns of an AoS record that hold SH coefficients: r g b sh0..3 at floats 4..15, sh4..15 at 25..60 (full SH)"""
    assert width in (25, 61), "records are 25 or 61 floats, not %d" % width
    return np.r_[4:16, 25:width]


def zero_sh(aos, which):
    """`aos` with every SH coefficient of the splats in `which` (bool) zeroed: project_kernel then stores 0.5 + 0 = 0.5 per lane"""
    out = aos.copy()
    rows = np.flatnonzero(which)
    out[np.ix_(rows, sh_floats(aos.shape[1]))] = 0.0
    return out


def dc_only(aos):
    """`aos` with SH bands 1..3 zeroed: the colour 0.5 + SH_C0 dc does not depend on the view"""
    out = aos.copy()
    assert aos.shape[1] in (25, 61), "records are 25 or 61 floats, not %d" % aos.shape[1]
    out[:, np.r_[5:8, 9:12, 13:16, 25:aos.shape[1]]] = 0.0
    return out


def dc_columns():
    return np.array([4, 8, 12])


def recoloured(aos, cls, pal):
    """the cloud whose DC terms give the colours the rule gives the dc_only cloud's: dc' = (c' - 0.5) / SH_C0, c' = tint(0.5 + SH_C0
    dc) in float32 as project_kernel computes it (b[0] * f + 0.5)"""
    base = dc_only(aos)
    c = np.float32(0.5) + np.float32(SH_C0) * base[:, dc_columns()]
    assert c.dtype == np.float32, c.dtype
    c2 = tint(c, cls, pal)
    out = base.copy()
    out[:, dc_columns()] = ((c2.astype(np.float64) - 0.5) / SH_C0).astype(np.float32)
    return base, out
