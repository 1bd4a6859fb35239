"""The suite's comparators and their tolerances, stated once (numpy only; SURVEY.md 8c and the header of tests/test_gpu_parity.py):
image against oracle image (check_image, check_fp16_image), a blended frame against layer + T dst (check_over; check_plane is its
one-channel |dst| = 1 form), and bit equality (same_bits).  pytest rewrites `assert` in test modules only, so every assertion here
carries its values in its message.  tests/test_suite_layout.py pins the bounds."""
import numpy as np

TIGHT = 5e-3                    # max abs per channel
T_EPS = 1.0 / 16384.0           # msplat_config.t_epsilon's default
# SURVEY 8c states rel 1e-5 for conic and colour: asserted as stated, relative to max(|x|, floor) because conic entries and SH
# colours pass through zero.  Measured on the MI355X (r4, every _check_projection call of the suite, 176 k splats): worst relative
# error 0 -- project_kernel evaluates the oracle's operation order without contraction, so these values are bit-identical.
CONIC_RTOL, CONIC_FLOOR = 1e-5, 1e-3
RGB_RTOL, RGB_FLOOR = 1e-5, 1e-3


def check_image(img, ref, max_abs=TIGHT, mean_abs=1e-4, frac=0.999, tol=1e-4, budget=None):
    """budget: per-pixel threshold-flip allowance from orc.composite_flip (None = plain max_abs bound)"""
    assert img.shape == ref.shape, "image %s, reference %s" % (img.shape, ref.shape)
    d = np.abs(img.astype(np.float64) - ref.astype(np.float64))
    rgb = d[..., :3]
    assert np.isfinite(img).all(), "%d value(s) are not finite" % (~np.isfinite(img)).sum()
    within = (rgb <= tol).mean()
    assert within >= frac, "only %.5f of values within %g (max %.3g)" % (within, tol, rgb.max())
    assert rgb.mean() <= mean_abs, "mean |diff| %.3g" % rgb.mean()
    worst = rgb.max(axis=-1)
    over = worst > max_abs
    if over.any():
        assert budget is not None, "max |diff| %.3g in %d pixel(s), no threshold-flip budget given" % (worst.max(), over.sum())
        unexplained = over & (worst > max_abs + budget.astype(np.float64))
        assert not unexplained.any(), "%d pixel(s) above %g not explained by a w ~ 1/256 flip (max %.3g, budget there %.3g)" % (
            unexplained.sum(), max_abs, worst[unexplained].max(), budget[unexplained].max())
        print("check_image: %d pixel(s) above %g, all within the oracle's threshold-flip budget (max %.3g)"
              % (over.sum(), max_abs, worst.max()))
    # the kernels write alpha = 1 exactly (app.cpp:158-160: cleared to 1, blended to 1)
    assert (img[..., 3] == 1.0).all(), "%d pixel(s) with alpha != 1" % (img[..., 3] != 1.0).sum()


def check_fp16_image(img, ref, budget):
    """RGBA16F target against the fp32 oracle: 2e-3 + 1 fp16 ulp (the target is rounded once; the reference's
    ROP rounds after every blend), threshold flips explained like in check_image"""
    assert img.dtype == np.float16, img.dtype
    ulp = np.abs(ref[..., :3]) * 2.0 ** -10
    d = np.abs(img[..., :3].astype(np.float32) - ref[..., :3])
    assert (d <= 2e-3 + ulp + budget[..., None]).all(), "max excess %.3g" % (d - 2e-3 - ulp - budget[..., None]).max()
    within = (d <= 2e-3 + ulp).mean()
    assert within > 0.999, "only %.5f of values within 2e-3 + 1 ulp" % within
    assert (img[..., 3] == 1).all(), "%d pixel(s) with alpha != 1" % (img[..., 3] != 1).sum()


def check_over(img, L, dst, t_eps, max_abs=TIGHT, mean_abs=1e-4, frac=0.999, tol=1e-4):
    """img against layer + T_ref dst on all channels (L: layer, T, bud_c, bud_w); check_image's three conditions, each scaled by
    (1 + |dst|) plus t_eps |dst| for the transmittance the early exit leaves; a value above the bound has to be explained by the
    threshold-flip budgets of both oracle frames, bud_c + bud_w |dst|"""
    d64 = np.abs(dst.astype(np.float64))
    want = L["layer"] + L["T"][..., None] * dst.astype(np.float64)
    err = np.abs(img.astype(np.float64) - want)
    assert np.isfinite(img).all(), "%d value(s) are not finite" % (~np.isfinite(img)).sum()
    print("check_over: max |err| %.3g, mean %.3g, t_eps %g" % (err.max(), err.mean(), t_eps))
    within = (err <= tol * (1.0 + d64) + t_eps * d64).mean()
    assert within >= frac, "only %.5f of values within the scaled %g (max %.3g)" % (within, tol, err.max())
    assert err.mean() <= mean_abs * (1.0 + d64.mean()) + t_eps * d64.mean(), "mean |err| %.3g" % err.mean()
    bound = max_abs * (1.0 + d64) + t_eps * d64
    over = err > bound
    if over.any():
        flips = L["bud_c"][..., None] + L["bud_w"][..., None] * d64
        bad = over & (err > bound + flips)
        assert not bad.any(), "%d value(s) above the bound not explained by a w ~ 1/256 flip (max %.3g)" % (bad.sum(), err[bad].max())
        print("check_over: %d value(s) above the bound, all within the two frames' threshold-flip budgets" % over.sum())


def check_plane(z, L, t_eps):
    """a depth plane against D_ref + T_ref (L: plane, T, bud_d, bud_w): check_over with one channel and |dst| = 1, that is
    2 tol + t_eps, 2 mean_abs + t_eps, 2 TIGHT + t_eps and the flip budgets bud_d + bud_w"""
    layer = dict(layer=(L["plane"] - L["T"])[..., None], T=L["T"], bud_c=L["bud_d"], bud_w=L["bud_w"])
    check_over(z[..., None], layer, np.ones(z.shape + (1,)), t_eps)


def assert_is_a_plane(z):
    assert np.isfinite(z).all() and (z >= 0.0).all() and (z <= 1.0).all(), (np.nanmin(z), np.nanmax(z))


def bits(a):
    """the array's values as unsigned integers of their own width"""
    return np.ascontiguousarray(a).view("u%d" % a.dtype.itemsize)


def same_bits(got, want, what=""):
    """dtype, shape and every bit equal (NaN payloads and the sign of zero included)"""
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    diff = bits(got) != bits(want)
    assert not diff.any(), "%s: %d of %d value(s) differ, first at %s" % (what, diff.sum(), diff.size, tuple(np.argwhere(diff)[0]))
