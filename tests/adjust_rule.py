"""What the tests of msplat_adjust_cloud share (numpy only; no device, no library, no torch): the rule of include/msplat.h restated
in numpy float32 in the header's operation order with the bias computed in float64; the named colour maps, the opacity scales, the
select cases and the clouds the GPU tests use; what a store of each kind returns for uploaded rows.  Nothing here is measured."""
import functools

import numpy as np

from tests import sh_q8_rule as sq
from tests import transform_rule as tr
from tests import visibility_rule as vr

F = np.float32
COLOUR, OPACITY = 1, 2                           # MSPLAT_ADJUST_COLOUR, MSPLAT_ADJUST_OPACITY
MODES = {"colour": COLOUR, "opacity": OPACITY, "both": COLOUR | OPACITY}
B0 = 0.28209479177387814                         # the SH basis' constant b_0
ALPHA_MIN = F(1.0 / 256.0)                       # a splat at or below it is never drawn: its footprint bound is 0
SIZES = (1, 63, 64, 65) + tuple(vr.SIZES)        # one splat; a wave less one, a wave, a wave and a splat; the cull boxes' sizes


# ---- the rule ----------------------------------------------------------------------------------------------------------------

def abi(colour):
    """a (3, 4) map in the row form [G | o] -> the ABI's 12 floats, column-major: colour[3 j + c] = G[c][j], colour[9 + c] = o[c]"""
    g = np.asarray(colour, F)
    assert g.shape == (3, 4), g.shape
    return np.ascontiguousarray(g.T.reshape(12))


def bias(colour12):
    """what the DC term of each channel gains: the header's expression, evaluated in float64 and rounded once"""
    c = np.asarray(colour12, F).astype(np.float64)
    return np.array([(((0.5 * ((c[ch] + c[3 + ch]) + c[6 + ch])) + c[9 + ch]) - 0.5) / B0 for ch in range(3)]).astype(F)


def clamp_alpha(scale, alpha):
    """alpha' = v > 0 ? (v > 1 ? 1 : v) : 0 with v = scale * alpha in float32: a NaN gives 0"""
    with np.errstate(all="ignore"):
        v = F(scale) * np.asarray(alpha, F)
        return np.where(v > 0, np.where(v > 1, F(1.0), v), F(0.0)).astype(F)


def adjust_rows(rows, colour, opacity_scale, flags, select=None):
    """The rule on (n, 25) or (n, 61) float32 records: rows with select (None: all) nonzero adjusted, the others copied.  colour:
    the ABI's 12 floats (read with COLOUR only); every operation in float32, left to right; numpy does not fuse"""
    rows = np.asarray(rows)
    assert rows.dtype == F and rows.ndim == 2 and rows.shape[1] in (25, 61), (rows.dtype, rows.shape)
    assert flags in (COLOUR, OPACITY, COLOUR | OPACITY), flags
    idx = np.arange(rows.shape[0]) if select is None else np.flatnonzero(np.asarray(select) != 0)
    out = rows.copy()
    src = rows[idx]
    with np.errstate(all="ignore"):
        if flags & COLOUR:
            c12 = np.asarray(colour, F).reshape(12)
            b = bias(c12)
            for k in range(16 if rows.shape[1] == 61 else 4):
                r, g, bl = (src[:, tr.sh_col(c, k)] for c in range(3))
                for c in range(3):
                    s = (c12[c] * r + c12[3 + c] * g) + c12[6 + c] * bl
                    if k == 0:
                        s = s + b[c]
                    out[idx, tr.sh_col(c, k)] = s
        if flags & OPACITY:
            out[idx, 3] = clamp_alpha(opacity_scale, src[:, 3])
    assert out.dtype == F
    return out


def colour_of(rows, v):
    """(splat, direction, channel) float64: the pre-clamp colour 0.5 + sum_k b_k(v) sh[c][k] the projection shows"""
    b = tr.basis(v)
    nk = 16 if rows.shape[1] == 61 else 4
    return np.stack([0.5 + rows[:, [tr.sh_col(c, k) for k in range(nk)]].astype(np.float64) @ b[:, :nk].T for c in range(3)], axis=2)


def stored(rows, storage):
    """what a store of that kind returns for uploaded rows: the decode of its encode"""
    if storage == "sh_q8":
        return sq.deq(rows)
    out = rows.copy()
    if storage == "sh_fp16":
        rest = [c for c in sq.REST if c < rows.shape[1]]
        with np.errstate(over="ignore"):
            out[:, rest] = rows[:, rest].astype(np.float16).astype(F)
    return out


# ---- the maps and the scales -------------------------------------------------------------------------------------------------

def tint(rgb, a):
    """[G | o] with G = (1 - a) I, o = a rgb in float64, rounded once"""
    return np.concatenate([(1.0 - a) * np.eye(3), a * np.asarray(rgb, np.float64)[:, None]], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def maps():
    """name -> (3, 4) float32 [G | o].  identity; swap: r <-> b, an exact permutation whose bias is 0 and whose square is the
    identity; grey: Rec. 709 luma in every channel; tint: 35 % towards an orange; negative: gains of both signs (a negative image
    plus a cast); gain4: a gain of 4 with an offset -- band values four times as large, which the fp16 store has to hold"""
    eye, zero = np.eye(3), np.zeros((3, 1))
    luma = np.array([0.2126, 0.7152, 0.0722])
    out = {"identity": np.concatenate([eye, zero], axis=1).astype(F),
           "swap": np.concatenate([np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]), zero], axis=1).astype(F),
           "grey": np.concatenate([np.tile(luma, (3, 1)), zero], axis=1).astype(F),
           "tint": tint((1.0, 0.55, 0.1), 0.35),
           "negative": np.array([[-1.0, 0.0, 0.25, 1.0], [0.5, -0.75, 0.0, 0.9], [0.0, 0.125, -1.5, 1.1]], F),
           "gain4": np.concatenate([4.0 * eye, np.array([[-0.2], [0.05], [0.3]])], axis=1).astype(F)}
    for m in out.values():
        m.setflags(write=False)
    return out


STRADDLE = 2.0 ** -7                             # exact: 0.5 -> 1/256, the float above 0.5 -> just above, the one below -> just below
SCALES = {"zero": 0.0, "2^-9": 2.0 ** -9, "half": 0.5, "one": 1.0, "two": 2.0, "straddle": STRADDLE}
STRADDLE_ALPHAS = np.array([0.5, np.nextafter(F(0.5), F(1.0)), np.nextafter(F(0.5), F(0.0))], F)


@functools.lru_cache(maxsize=None)
def cloud(n, full_sh=True):
    """the GPU tests' cloud of n splats (read-only): visibility_rule's, with the alphas of the first splats of every wave of 64 set
    to STRADDLE_ALPHAS -- under STRADDLE they land on 1/256, one float above it and one float below"""
    aos = (vr.cloud_aos(n, vr.TIE_FREE[1]) if n == vr.TIE_FREE[0] else vr.cloud_aos(n)).copy()
    for k, a in enumerate(STRADDLE_ALPHAS):
        aos[k::64, 3] = a
    aos = aos if full_sh else np.ascontiguousarray(aos[:, :25])
    aos.setflags(write=False)
    return aos


def q8_stable(aos):
    """`aos` with its f_rest values at a fixed point of the SH_Q8 quantiser: a store of that kind returns these rows bit for bit,
    so the upload of a download is the download.  (A second Q8 round may move a value once more -- msplat.h -- and the reference
    of the GPU tests is an upload of downloaded rows: an opacity-only call copies the codes, an upload quantises again.)"""
    rows = sq.deq(aos)
    for _ in range(8):
        again = sq.deq(rows)
        if np.array_equal(again.view(np.uint32), rows.view(np.uint32)):
            rows.setflags(write=False)
            return rows
        rows = again
    raise AssertionError("the SH_Q8 quantiser did not reach a fixed point in 8 rounds")


def overflow_cloud(n=300, row=5):
    """(cloud, row): a band-2 value of 20000 in one row -- gain4 takes it to 80000, beyond fp16 (|c| >= 65520), nothing else near"""
    aos = cloud(n).copy()
    aos[row, tr.sh_col(1, 6)] = 20000.0
    return aos, row


# ---- the selections ----------------------------------------------------------------------------------------------------------

def wave_select(n):
    """For n >= 256 (four whole waves of 64 stored records in a store in upload order): wave 0 with no selected lane, wave 1 with
    all, wave 2 with lane 0 alone, wave 3 with lane 63 alone, the rest at random"""
    assert n >= 256, n
    sel = np.random.default_rng(77 + n).random(n) < 0.5
    sel[0:64], sel[64:128], sel[128:192], sel[192:256] = False, True, False, False
    sel[128], sel[255] = True, True
    return sel


def select_cases(n):
    """name -> the selection (None: every splat): transform_rule's cases, and wave_select where the cloud has the waves for it"""
    cases = dict(tr.select_cases(n))
    if n >= 256:
        cases["waves"] = wave_select(n)
    return cases


def wave_counts(select):
    """selected lanes per wave of 64, and per wave the lane of its only selected splat (-1: not exactly one)"""
    s = np.asarray(select) != 0
    pad = np.concatenate([s, np.zeros(-s.shape[0] % 64, bool)]).reshape(-1, 64)
    cnt = pad.sum(axis=1)
    return cnt, np.where(cnt == 1, pad.argmax(axis=1), -1)
