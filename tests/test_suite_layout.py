"""The suite's own layout: shared test code lives in support modules (tests/*.py whose names do not start with test_), never in
test modules, and the comparators of tests/checks.py sit at the bounds the project states -- 99.9 % of values within 1e-4, mean
1e-4, max TIGHT = 5e-3 unless the oracle's threshold-flip budget explains it, each scaled by (1 + |dst|) plus t_eps |dst| where
a frame is blended over a destination.  Nothing here is measured: every number is one of those, and every case sits a relative
1e-9 inside or outside its bound (float64 rounding of img - ref is 1e-13 of these errors)."""
import ast
import glob
import os

import numpy as np
import pytest

from tests.checks import T_EPS, TIGHT, check_image, check_over, check_plane
from tests.conftest import ROOT

TOL, MEAN_ABS, FRAC = 1e-4, 1e-4, 0.999
DELTA = 1e-9


def test_no_test_module_imports_another():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")))
    assert len(paths) > 30
    for path in paths:
        name, tree = os.path.basename(path), ast.parse(open(path).read(), path)
        support = not name.startswith("test_") and name not in ("conftest.py", "__init__.py")
        for node in ast.walk(tree):                             # imports at any depth, those inside functions included
            if isinstance(node, (ast.Import, ast.ImportFrom)):
                module = getattr(node, "module", None) or ""
                imported = [module] + [a.name for a in node.names] + ["%s.%s" % (module, a.name) for a in node.names]
                assert not getattr(node, "level", 0), "%s:%d: a relative import hides what it imports" % (name, node.lineno)
                for m in imported:
                    assert not m.startswith("tests.test_"), "%s:%d imports the test module %s" % (name, node.lineno, m)
                if support and node in tree.body:
                    assert "torch" not in [m.split(".")[0] for m in imported], "%s imports torch at module level" % name
        for node in tree.body if support else []:               # a support module: nothing pytest would collect or mark
            assert not (isinstance(node, ast.FunctionDef) and node.name.startswith("test_")), "%s defines %s" % (name, node.name)
            assert not (isinstance(node, ast.ClassDef) and node.name.startswith("Test")), "%s defines %s" % (name, node.name)
            assert not (isinstance(node, ast.Assign) and any(getattr(t, "id", "") == "pytestmark" for t in node.targets)), "%s sets pytestmark" % name


# ------------------------------------------------------------------------------------------------

def bounds(d, t_eps):
    """(the share's bound, the maximum's bound) per value and the mean's bound, for values blended over |dst| = d"""
    return TOL * (1.0 + d) + t_eps * d, TIGHT * (1.0 + d) + t_eps * d, MEAN_ABS * (1.0 + d.mean()) + t_eps * d.mean()


def at_the_share(tolb, n_out):
    """n_out values just outside the share's bound, the others just inside it"""
    err = tolb * (1.0 - DELTA)
    err.reshape(-1)[:n_out] = tolb.reshape(-1)[:n_out] * (1.0 + DELTA)
    return err


def at_the_mean(tolb, maxb, mean):
    """the allowed 0.1 % of the values at half their maximum, the others at the one share of their bound that makes the mean `mean`"""
    n_out = int(round(tolb.size * (1.0 - FRAC)))
    err, big = tolb.copy().reshape(-1), 0.5 * maxb.reshape(-1)[:n_out]
    c = (tolb.size * mean - big.sum()) / err[n_out:].sum()
    assert 0.9 < c < 1.0, c
    err[n_out:] *= c
    err[:n_out] = big
    return err.reshape(tolb.shape)


def one_value(shape, where, value):
    err = np.zeros(shape)
    err[where] = value
    return err


def passes(check, err):
    check(err)
    check(-err)                                                 # the bounds are on |err|


def fails(check, err, why):
    for e in (err, -err):
        with pytest.raises(AssertionError, match=why):
            check(e)


def comparator_sits_at_its_bounds(check, d, t_eps, flip, where, without_budget, N):
    """check(err, bud=None): the comparator on a frame that is `err` away from its reference, bud = (colour or depth frame's
    budget, white frame's) at the pixel of `where`; d: |dst| per value (zeros: no destination); flip(bud) = what the budgets allow
    the value at `where`; without_budget: what the comparator says about a value above the maximum when it has no budget"""
    tolb, maxb, meanb = bounds(d, t_eps)
    n_out = int(round(N * (1.0 - FRAC)))
    assert d.size == N and n_out >= 3 and abs(n_out - N * (1.0 - FRAC)) < 1e-6       # 0.1 % of the values is a whole number of them
    # the share within tol: exactly 0.1 % of the values may lie outside
    passes(check, at_the_share(tolb, n_out))
    fails(check, at_the_share(tolb, n_out + 1), "of values within")
    # the mean
    passes(check, at_the_mean(tolb, maxb, meanb * (1.0 - DELTA)))
    fails(check, at_the_mean(tolb, maxb, meanb * (1.0 + DELTA)), "mean")
    # one value at the maximum: without a budget, with one that covers it, with one that does not
    passes(check, one_value(d.shape, where, maxb[where] * (1.0 - DELTA)))
    fails(check, one_value(d.shape, where, maxb[where] * (1.0 + DELTA)), without_budget)
    for bud in ((2.0 ** -8, 0.0), (0.0, 2.0 ** -8), (2.0 ** -9, 2.0 ** -7)):
        if flip(bud) == 0.0:
            continue                                            # (no destination: the white frame's budget buys nothing)
        passes(lambda e: check(e, bud), one_value(d.shape, where, (maxb[where] + flip(bud)) * (1.0 - DELTA)))
        fails(lambda e: check(e, bud), one_value(d.shape, where, (maxb[where] + flip(bud)) * (1.0 + DELTA)), "not explained")
        fails(lambda e: check(e, bud), one_value(d.shape, (0, 0, 0), maxb[0, 0, 0] * (1.0 + DELTA)), "not explained|no threshold")   # the budget is that pixel's


def test_the_comparators_sit_at_their_stated_bounds():
    assert (TIGHT, T_EPS) == (5e-3, 1.0 / 16384.0)
    H, W = 25, 80                                              # 2000 pixels: 6000 colour values, 8000 with alpha
    rng = np.random.default_rng(1)

    # check_image: three colour channels against the oracle's image, alpha == 1 exactly, one budget per pixel
    ref = rng.uniform(0.0, 1.0, (H, W, 4))
    ref[..., 3] = 1.0

    def image(err, bud=None):
        img = ref.copy()
        img[..., :3] += err
        budget = None
        if bud is not None:
            budget = np.zeros((H, W), np.float32)
            budget[7, 11] = bud[0]
        check_image(img, ref, budget=budget)

    comparator_sits_at_its_bounds(image, np.zeros((H, W, 3)), 0.0, lambda bud: bud[0], (7, 11, 2), "no threshold-flip budget given", 6000)
    translucent = ref.copy()
    translucent[3, 4, 3] = np.nextafter(1.0, 0.0)
    with pytest.raises(AssertionError, match="alpha"):
        check_image(translucent, ref)

    # check_over: four channels against layer + T dst, both signs of dst, two values of |dst|
    dst = np.where(rng.random((H, W, 4)) < 0.5, 3.0, -1.0)
    L = dict(layer=rng.uniform(0.0, 1.0, (H, W, 4)), T=rng.uniform(0.0, 1.0, (H, W)))
    for t_eps in (T_EPS, 0.0):
        for where in [tuple(np.argwhere(dst == 3.0)[5]), tuple(np.argwhere(dst == -1.0)[5])]:
            def over(err, bud=None):
                Lb = dict(L, bud_c=np.zeros((H, W)), bud_w=np.zeros((H, W)))
                if bud is not None:
                    Lb["bud_c"][where[:2]], Lb["bud_w"][where[:2]] = bud
                check_over(L["layer"] + L["T"][..., None] * dst + err, Lb, dst, t_eps)

            comparator_sits_at_its_bounds(over, np.abs(dst), t_eps, lambda bud: bud[0] + bud[1] * abs(dst[where]), where, "not explained", 8000)

    # check_plane: check_over's one-channel form with dst = 1, that is 2 tol + t_eps, 2 mean_abs + t_eps, 2 TIGHT + t_eps
    Hp, Wp = 60, 100
    P = dict(plane=rng.uniform(0.0, 1.0, (Hp, Wp)), T=rng.uniform(0.0, 1.0, (Hp, Wp)))
    for t_eps in (T_EPS, 0.0):
        tolb, maxb, meanb = bounds(np.ones((Hp, Wp, 1)), t_eps)
        assert (tolb == 2 * TOL + t_eps).all() and (maxb == 2 * TIGHT + t_eps).all() and meanb == 2 * MEAN_ABS + t_eps

        def plane(err, bud=None):
            Pb = dict(P, bud_d=np.zeros((Hp, Wp)), bud_w=np.zeros((Hp, Wp)))
            if bud is not None:
                Pb["bud_d"][9, 13], Pb["bud_w"][9, 13] = bud
            check_plane(P["plane"] + err[..., 0], Pb, t_eps)

        comparator_sits_at_its_bounds(plane, np.ones((Hp, Wp, 1)), t_eps, lambda bud: bud[0] + bud[1], (9, 13, 0), "not explained", 6000)
    with pytest.raises(AssertionError, match="finite"):
        check_plane(np.where(np.arange(Wp) == 3, np.nan, P["plane"]), dict(P, bud_d=np.zeros((Hp, Wp)), bud_w=np.zeros((Hp, Wp))), T_EPS)
