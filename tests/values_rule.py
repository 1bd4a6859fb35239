"""What the tests of selection by attribute share (numpy only; no device, no torch): the rules of msplat_cloud_values,
msplat_mark_values and msplat_histogram_values of include/msplat.h restated in numpy float32 -- every operation rounded on its own,
nothing fused, in the header's order; the SCALE kinds through tests/egress_rule.jacobi_eigen3 --, the hostile rows the rule and the
kernels are run on, and the thresholds at which the SCALE kinds can be compared with a range without rounding deciding anything."""
import functools

import numpy as np

from tests import egress_rule as er

F = np.float32
KINDS = ("x", "y", "z", "reach2", "distance2", "alpha", "red", "green", "blue", "colour_dist2", "scale_min", "scale_mid", "scale_max")
PARAM_KINDS = ("distance2", "colour_dist2")
SCALE_KINDS = ("scale_min", "scale_mid", "scale_max")
COPY_KINDS = ("x", "y", "z", "reach2", "alpha")
SH_C0 = F(0.28209479177387814)
SIZES = (1, 63, 64, 65, 4097)
PARAMS = {"distance2": np.array([0.25, -0.5, 1.0], F), "colour_dist2": np.array([0.1, 0.8, 0.2], F)}
FAMILIES = ("needles", "isotropic", "two_equal")
BINS_MAX = 4096


# ---- msplat_cloud_values ----------------------------------------------------------------------------------------------------
def _dist2(a, b, c, p):
    p = np.asarray(p, F)
    with np.errstate(all="ignore"):
        da, db, dc = (a - p[0]).astype(F), (b - p[1]).astype(F), (c - p[2]).astype(F)
        return (((da * da).astype(F) + (db * db).astype(F)).astype(F) + (dc * dc).astype(F)).astype(F)


def base_colour(rec):
    """(r, g, b): 0.5f + (0.28209479177387814f * g[4 + 4c])"""
    rec = np.asarray(rec, F)
    with np.errstate(all="ignore"):
        return tuple((F(0.5) + (SH_C0 * rec[:, 4 + 4 * c]).astype(F)).astype(F) for c in range(3))


def scales(rec):
    """(N, 3): sqrtf(max(eval_k, 0.0f)) of JacobiEigen3 of g[16..24], ascending"""
    ev, _ = er.jacobi_eigen3(np.asarray(rec, F)[:, 16:25])
    with np.errstate(all="ignore"):
        return np.sqrt(np.where(ev < 0, F(0.0), ev).astype(F)).astype(F)


def values(rec, pos4, kind, param=None):
    """the rule: rec = the (N, 25 | 61) records msplat_download_cloud returns, pos4 = the (N, 4) position plane -> float32[N]"""
    rec, pos4 = np.asarray(rec, F), np.asarray(pos4, F)
    assert kind in KINDS and (kind in PARAM_KINDS) == (param is not None), (kind, param)
    if kind in ("x", "y", "z", "reach2"):
        return pos4[:, ("x", "y", "z", "reach2").index(kind)].copy()
    if kind == "distance2":
        return _dist2(pos4[:, 0], pos4[:, 1], pos4[:, 2], param)
    if kind == "alpha":
        return rec[:, 3].copy()
    if kind in ("red", "green", "blue"):
        return base_colour(rec)[("red", "green", "blue").index(kind)]
    if kind == "colour_dist2":
        return _dist2(*base_colour(rec), param)
    return np.ascontiguousarray(scales(rec)[:, SCALE_KINDS.index(kind)])


# ---- msplat_mark_values -----------------------------------------------------------------------------------------------------
def inside(v, lo, hi):
    """v >= lo && v <= hi in fp32; a NaN value is never inside"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        return (v >= F(lo)) & (v <= F(hi))


def marked(mask, v, lo, hi, outside, value):
    """the mask after the call"""
    hit = inside(v, lo, hi) != bool(outside)
    return np.where(hit, np.uint8(value), np.asarray(mask, np.uint8)).astype(np.uint8)


# ---- msplat_histogram_values ------------------------------------------------------------------------------------------------
def bin_scale(bins, lo, hi):
    """(float)((double)bins / ((double)hi - (double)lo)), and whether it is a normal fp32 number"""
    with np.errstate(all="ignore"):
        s = F(np.float64(bins) / (np.float64(F(hi)) - np.float64(F(lo))))
    return s, bool(np.isfinite(s) and abs(s) >= np.finfo(F).tiny)


def bin_of(v, bins, lo, hi):
    """the bin of every value with lo <= v <= hi (other entries are meaningless): t = (v - lo) * scale in fp32, b = t >= bins ? bins - 1 : (uint32)t"""
    s, normal = bin_scale(bins, lo, hi)
    assert normal, (bins, lo, hi, s)
    with np.errstate(all="ignore"):
        t = ((np.asarray(v, F) - F(lo)).astype(F) * s).astype(F)
        ok = inside(v, lo, hi)
        return np.where(t >= F(bins), bins - 1, np.where(ok, t, 0).astype(np.int64)).astype(np.int64)


def histogram(v, select=None, bins=0, lo=None, hi=None):
    """dict(selected, finite, nan, below, above, vmin, vmax, counts uint32[bins])"""
    v = np.asarray(v, F)
    sel = np.ones(v.shape[0], bool) if select is None else np.asarray(select) != 0
    v = v[sel]
    fin = np.isfinite(v)
    out = dict(selected=int(sel.sum()), finite=int(fin.sum()), nan=int(np.isnan(v).sum()), below=0, above=0,
               vmin=F(v[fin].min()) if fin.any() else F(np.inf), vmax=F(v[fin].max()) if fin.any() else F(-np.inf),
               counts=np.zeros(bins, np.uint32))
    if bins:
        with np.errstate(invalid="ignore"):
            out["below"], out["above"] = int((v < F(lo)).sum()), int((v > F(hi)).sum())
        ok = inside(v, lo, hi)
        out["counts"] = np.bincount(bin_of(v[ok], bins, lo, hi), minlength=bins).astype(np.uint32)
        assert out["counts"].shape == (bins,)
    return out


def summary_fields(h):
    return tuple(h[k] for k in ("selected", "finite", "nan", "below", "above")) + (F(h["vmin"]).tobytes(), F(h["vmax"]).tobytes())


# ---- the fixtures -----------------------------------------------------------------------------------------------------------
HAND = 5            # rows 0..4: egress_rule.hand_records (zero covariance, 0.005 I, alpha 0, alpha 1, an asymmetric Sigma)
PLANTED = {5: (3, np.nan), 6: (3, np.inf), 7: (3, -np.inf), 8: (4, np.nan), 9: (8, np.inf), 10: (12, -np.inf), 11: (0, np.nan), 12: (1, np.inf),
           13: (2, -np.inf)}      # row: (record float, value) -- alpha, the three DC terms, the centre


@functools.lru_cache(maxsize=None)
def rows():
    """(4097, 61) fp32 records (read-only): the hand rows, then needles, isotropic and two_equal taking turns (so that the first 63
    rows hold every family), with NaN and +-inf planted in alpha, a DC term and a centre of rows 5..13"""
    n = SIZES[-1]
    rec = np.empty((n, 61), F)
    rec[:HAND] = er.family_records("hand")
    fam = [er.family_records(name) for name in FAMILIES]
    k = np.arange(n - HAND)
    for f in range(3):
        mine = k % 3 == f
        rec[HAND:][mine] = fam[f][:int(mine.sum())]
    for row, (col, val) in PLANTED.items():
        rec[row, col] = val
    rec.setflags(write=False)
    return rec


def family_of_row(n=SIZES[-1]):
    """per row: -1 for the hand rows, else the index into FAMILIES"""
    out = np.full(n, -1)
    out[HAND:] = np.arange(n - HAND) % 3
    return out[:n]


def cloud(n, full_sh=True):
    return np.ascontiguousarray(rows()[:n] if full_sh else rows()[:n, :25])


@functools.lru_cache(maxsize=None)
def scale_thresholds(kind):
    """{family: threshold} for a SCALE kind: the midpoint of the widest gap between consecutive sorted rule values in the middle
    half of the family's rows of rows() -- as far from every value as a threshold that splits the family can be"""
    v = scales(rows())[:, SCALE_KINDS.index(kind)].astype(np.float64)
    fam = family_of_row()
    out = {}
    for f, name in enumerate(FAMILIES):
        s = np.sort(v[fam == f])
        q = s[s.shape[0] // 4:s.shape[0] - s.shape[0] // 4]
        gap = np.diff(q)
        at = int(gap.argmax())
        out[name] = F(0.5 * (q[at] + q[at + 1]))
    return out


def undecidable(v, threshold, rel=1e-5):
    """the values within rel (relative) of the threshold"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(v - float(threshold)) <= rel * abs(float(threshold))


HIST_N = 4097


@functools.lru_cache(maxsize=None)
def hist_inputs():
    """{name: (float32[HIST_N] values, lo, hi)} (read-only): uniform values; all values equal (one hot bin); values exactly lo and hi
    among others; values below and above; NaN and +-inf"""
    rng = np.random.default_rng(0x29A1)
    n = HIST_N
    uniform = rng.uniform(-2.0, 3.0, n).astype(F)
    equal = np.full(n, F(0.7))
    ends = rng.uniform(-2.0, 3.0, n).astype(F)
    ends[::5], ends[1::7] = F(-2.0), F(3.0)
    ends[2::11] = np.nextafter(F(3.0), F(0.0))
    ends[3::13] = np.nextafter(F(-2.0), F(0.0))
    outside = rng.uniform(-6.0, 7.0, n).astype(F)
    hostile = rng.uniform(-2.5, 3.5, n).astype(F)
    hostile[::9], hostile[1::10], hostile[2::17] = np.nan, np.inf, -np.inf
    hostile[3], hostile[4] = F(3.4e38), F(-3.4e38)
    hostile[5], hostile[6] = F(1e-45), F(-0.0)
    out = dict(uniform=(uniform, -2.0, 3.0), equal=(equal, 0.0, 1.0), ends=(ends, -2.0, 3.0), outside=(outside, -2.0, 3.0),
               hostile=(hostile, -2.0, 3.0))
    for v, _, _ in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hist_select():
    """a uint8 selection of HIST_N values: about two in three, with values 1 and 255"""
    rng = np.random.default_rng(0x29A2)
    s = rng.integers(0, 3, HIST_N).astype(np.uint8)
    s[s == 2] = 255
    s.setflags(write=False)
    return s
