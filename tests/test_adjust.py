"""CPU tests of msplat_adjust_cloud, no device: the names exist in the header, the library and the binding; the
refusals that need no device; the rule itself (tests/adjust_rule.py) -- the colour a splat shows in any direction follows
col' = G col + o, the channel swap is an exact permutation, the identity returns its input, alpha is clamped as the header says
and unselected rows keep their bits --; that the fixtures of the GPU tests are what they claim; and the Python helpers.

The colour bound is derived, not measured.  The new colour of channel c at direction v is 0.5 + sum_k b_k sh'[c][k]; in exact
arithmetic it is the sum of the `terms` b_k G[c][j] sh[j][k] (3 per coefficient) and b_0 bias[c], plus 0.5, and equals
(G col + o)[c].  Each sh'[c][k] is five or six fp32 operations (three products, two or three sums) on partial sums no larger
than its own terms' magnitudes, and bias is rounded once: an error of at most 6 * 2^-24 sum |terms|.  Asserted:
(terms + 2) * 2^-23 * sum |terms| with the terms evaluated in float64, whose own rounding (2^-53 a term) is far below it."""
import ctypes as C
import os

import numpy as np
import pytest

import splatapult_amd
from splatapult_amd import SplatRenderer, _capi
from tests import adjust_rule as ar
from tests import sh_q8_rule as sq
from tests import transform_rule as tr
from tests.checks import same_bits
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "msplat.h")
MAPS = ar.maps()
_P = C.POINTER(C.c_float)


def test_the_header_declares_the_call_the_library_exports_it_and_the_binding_has_it():
    header = open(HEADER).read()
    assert "enum { MSPLAT_ADJUST_COLOUR = 1, MSPLAT_ADJUST_OPACITY = 2 };" in header
    assert ("int msplat_adjust_cloud(msplat_ctx* ctx, const float colour[12], float opacity_scale, const uint8_t* d_select, uint64_t n, "
            "int32_t flags);") in header
    for said in ("sRGB-encoded under cfg.srgb", "a per-splat or per-class map", "non-linear curves", "host-memory selections"):
        assert said in header, said
    assert len(header.splitlines()) <= 300
    L = C.CDLL(_capi.LIB_PATH)
    assert hasattr(L, "msplat_adjust_cloud"), "libmsplat.so does not export msplat_adjust_cloud"
    assert "msplat_adjust_cloud" in {n for n, _, _ in _capi.SYMBOLS}, "no ctypes prototype for msplat_adjust_cloud"
    assert (_capi.ADJUST_COLOUR, _capi.ADJUST_OPACITY) == (ar.COLOUR, ar.OPACITY) == (1, 2)
    assert callable(getattr(SplatRenderer, "AdjustCloud", None)), "SplatRenderer has no AdjustCloud"


def test_a_null_context_is_refused():
    L = _capi.lib()
    m = ar.abi(MAPS["tint"])
    assert L.msplat_adjust_cloud(None, m.ctypes.data_as(_P), 1.0, None, 0, ar.COLOUR | ar.OPACITY) == _capi.ERR_INVALID_ARG
    assert "ctx is NULL" in L.msplat_last_error(None).decode()


def _records(n, seed, full_sh=True):
    """(n, 61 | 25) records with |sh| <= 1"""
    rng = np.random.default_rng(seed)
    aos = ar.cloud(n).copy()
    for c in range(3):
        for k in range(16):
            aos[:, tr.sh_col(c, k)] = rng.uniform(-1.0, 1.0, n)
    return aos if full_sh else np.ascontiguousarray(aos[:, :25])


@pytest.mark.parametrize("full_sh", [True, False], ids=["full_sh", "degree0"])
@pytest.mark.parametrize("name", list(MAPS))
def test_the_colour_in_every_direction_follows_the_map(name, full_sh):
    rows = _records(40, 3, full_sh)
    m = MAPS[name]
    c12 = ar.abi(m)
    out = ar.adjust_rows(rows, c12, 1.0, ar.COLOUR)
    v = tr.directions(64, 9)
    G, o = m[:, :3].astype(np.float64), m[:, 3].astype(np.float64)
    want = ar.colour_of(rows, v) @ G.T + o                       # (splat, direction, channel): G col + o
    got = ar.colour_of(out, v)
    nk = 16 if full_sh else 4
    b = np.abs(tr.basis(v)[:, :nk])                              # (direction, k)
    sh = np.abs(np.stack([rows[:, [tr.sh_col(j, k) for k in range(nk)]] for j in range(3)], axis=1).astype(np.float64))     # (splat, j, k)
    total = np.einsum("dk,cj,sjk->sdc", b, np.abs(G), sh) + ar.B0 * np.abs(ar.bias(c12).astype(np.float64))
    terms = 3 * nk + 1
    bound = (terms + 2) * 2.0 ** -23 * total
    err = np.abs(got - want)
    print("%s: max |colour' - (G colour + o)| %.3g, the smallest bound %.3g, worst ratio %.3g" % (name, err.max(), bound.min(), (err / bound).max()))
    assert (err <= bound).all(), (name, float((err / bound).max()))
    same_bits(out[:, [0, 1, 2, 3] + list(range(16, 25))], rows[:, [0, 1, 2, 3] + list(range(16, 25))], "centre, alpha, covariance")


def test_the_channel_swap_is_an_exact_permutation_and_its_own_inverse():
    rows = _records(64, 4)
    assert not (np.signbit(rows) & (rows == 0)).any()            # no -0: (0 * r + g) + 0 * b would make it +0
    c12 = ar.abi(MAPS["swap"])
    assert (ar.bias(c12) == 0).all()
    once = ar.adjust_rows(rows, c12, 1.0, ar.COLOUR)
    for k in range(16):
        same_bits(once[:, tr.sh_col(0, k)], rows[:, tr.sh_col(2, k)], "r <- b, k %d" % k)
        same_bits(once[:, tr.sh_col(1, k)], rows[:, tr.sh_col(1, k)], "g, k %d" % k)
        same_bits(once[:, tr.sh_col(2, k)], rows[:, tr.sh_col(0, k)], "b <- r, k %d" % k)
    same_bits(ar.adjust_rows(once, c12, 1.0, ar.COLOUR), rows, "the swap applied twice")


def test_the_identity_returns_its_input_but_not_a_negative_zero():
    rows = _records(64, 5)
    c12 = ar.abi(MAPS["identity"])
    same_bits(ar.adjust_rows(rows, c12, 1.0, ar.COLOUR), rows, "the identity map")
    same_bits(ar.adjust_rows(rows, c12, 1.0, ar.COLOUR | ar.OPACITY), rows, "the identity map and a scale of 1")
    z = rows.copy()
    z[0, tr.sh_col(1, 2)] = -0.0
    out = ar.adjust_rows(z, c12, 1.0, ar.COLOUR)
    assert out[0, tr.sh_col(1, 2)] == 0.0 and not np.signbit(out[0, tr.sh_col(1, 2)])      # -0 + 0 = +0, as the header says


def test_alpha_is_clamped_as_the_header_says():
    F = np.float32
    alpha = np.array([0.0, 1e-30, 0.25, 0.5, 1.0, np.nan, -0.5, np.inf], F)
    same_bits(ar.clamp_alpha(0.0, alpha), np.zeros(8, F), "a scale of 0: 0, NaN (0 * inf) included")
    same_bits(ar.clamp_alpha(2.0, alpha), np.array([0.0, 2e-30, 0.5, 1.0, 1.0, 0.0, 0.0, 1.0], F), "a scale of 2")
    same_bits(ar.clamp_alpha(1.0, alpha), np.array([0.0, 1e-30, 0.25, 0.5, 1.0, 0.0, 0.0, 1.0], F), "a scale of 1: NaN -> 0, inf -> 1")
    same_bits(ar.clamp_alpha(0.5, alpha)[:5], (F(0.5) * alpha[:5]).astype(F), "a scale of 1/2 is the fp32 product")
    rows = _records(16, 6)
    out = ar.adjust_rows(rows, None, 2.0 ** -9, ar.OPACITY)
    same_bits(out[:, 3], (F(2.0 ** -9) * rows[:, 3]).astype(F), "a fade to 2^-9")
    same_bits(np.delete(out, 3, axis=1), np.delete(rows, 3, axis=1), "an opacity-only call leaves every other column alone")


def test_unselected_rows_and_unflagged_parts_keep_their_bits():
    rows = _records(300, 7)
    c12 = ar.abi(MAPS["negative"])
    sh = [tr.sh_col(c, k) for c in range(3) for k in range(16)]
    for name, sel in ar.select_cases(300).items():
        out = ar.adjust_rows(rows, c12, 0.5, ar.COLOUR | ar.OPACITY, sel)
        on = np.ones(300, bool) if sel is None else np.asarray(sel) != 0
        same_bits(out[~on], rows[~on], "%s: the unselected rows" % name)
        same_bits(out[on], ar.adjust_rows(rows, c12, 0.5, ar.COLOUR | ar.OPACITY)[on], "%s: the selected rows" % name)
        assert (out[on][:, sh] != rows[on][:, sh]).any(axis=1).all() and (out[on, 3] != rows[on, 3]).all(), name
    colour_only = ar.adjust_rows(rows, c12, 0.5, ar.COLOUR)
    same_bits(colour_only[:, 3], rows[:, 3], "without OPACITY alpha stays")
    d0 = np.ascontiguousarray(rows[:, :25])                      # an SH degree 0 record: band 1 lives in sh0.yzw and is adjusted
    same_bits(ar.adjust_rows(d0, c12, 0.5, ar.COLOUR | ar.OPACITY), ar.adjust_rows(rows, c12, 0.5, ar.COLOUR | ar.OPACITY)[:, :25], "degree 0")


# ---- the GPU tests' fixtures are what they claim ------------------------------------------------------------------------------

def test_the_alpha_cases_straddle_one_256th():
    F = np.float32
    got = ar.clamp_alpha(ar.STRADDLE, ar.STRADDLE_ALPHAS)
    assert got[0] == ar.ALPHA_MIN and got[1] == np.nextafter(ar.ALPHA_MIN, F(1)) and got[2] == np.nextafter(ar.ALPHA_MIN, F(0)), got
    for n in ar.SIZES:
        for full_sh in (True, False):
            aos = ar.cloud(n, full_sh)
            assert aos.shape == (n, 61 if full_sh else 25) and aos.dtype == F
            a = ar.clamp_alpha(ar.STRADDLE, aos[:, 3])
            assert (a == ar.ALPHA_MIN).any(), n
            if n >= 3:
                assert (a == np.nextafter(ar.ALPHA_MIN, F(1))).any() and (a == np.nextafter(ar.ALPHA_MIN, F(0))).any(), n
    fade = ar.clamp_alpha(ar.SCALES["2^-9"], ar.cloud(4097)[:, 3])
    assert (fade <= ar.ALPHA_MIN).all() and (fade > 0).all()     # a fade to 2^-9 takes every splat out of the frame
    assert set(ar.SCALES.values()) >= {0.0, 2.0 ** -9, 0.5, 1.0, 2.0, ar.STRADDLE}
    assert {1, 63, 64, 65, 4097} <= set(ar.SIZES)


def test_the_sh_q8_cloud_is_a_fixed_point_of_the_quantiser():
    for n in ar.SIZES:
        rows = ar.q8_stable(ar.cloud(n))
        same_bits(sq.deq(rows), rows, "n %d: a second Q8 round" % n)
        keep = [c for c in range(61) if c not in sq.REST]
        same_bits(rows[:, keep], ar.cloud(n)[:, keep], "n %d: everything but f_rest" % n)
        assert np.abs(rows - ar.cloud(n)).max() < 0.05           # still the cloud, to the quantiser's step
        faded = ar.adjust_rows(rows, None, ar.STRADDLE, ar.OPACITY)
        same_bits(sq.deq(faded), faded, "n %d: the faded rows" % n)


def test_the_fp16_overflow_case_exceeds_the_range_in_exactly_one_row():
    aos, row = ar.overflow_cloud()
    out = ar.adjust_rows(aos, ar.abi(MAPS["gain4"]), 1.0, ar.COLOUR)
    over = (np.abs(out[:, sq.REST]) >= 65520.0).any(axis=1)
    assert over[row] and over.sum() == 1, np.flatnonzero(over)
    assert np.abs(np.delete(out, row, axis=0)[:, sq.REST]).max() < 100.0
    assert np.isfinite(out).all()
    for name, m in MAPS.items():                                 # and no named map overflows the GPU tests' clouds
        for n in (257, 4097):
            assert np.abs(ar.adjust_rows(ar.cloud(n), ar.abi(m), 1.0, ar.COLOUR)[:, sq.REST]).max() < 1000.0, (name, n)


def test_the_select_cases_have_the_waves_they_claim():
    for n in ar.SIZES:
        cases = ar.select_cases(n)
        assert set(tr.select_cases(n)) <= set(cases) and cases["none"] is None
        assert ("waves" in cases) == (n >= 256), n
        if n < 256:
            continue
        cnt, lane = ar.wave_counts(cases["waves"])
        rows = np.minimum(64, n - 64 * np.arange(cnt.shape[0]))
        assert cnt[0] == 0 and cnt[1] == 64 == rows[1] and lane[2] == 0 and lane[3] == 63, (n, cnt[:4], lane[:4])
        if n > 256:
            assert (cnt[4:] > 0).any()


# ---- the binding and the helpers, no device -----------------------------------------------------------------------------------

def test_adjust_cloud_refuses_bad_arguments_before_the_library_is_called():
    r = SplatRenderer(device=0)
    with pytest.raises(ValueError):
        r.AdjustCloud()
    with pytest.raises(ValueError):
        r.AdjustCloud(colour=np.eye(4, dtype=np.float32))
    with pytest.raises(ValueError):
        r.AdjustCloud(colour=np.zeros(12, np.float32))
    bad = MAPS["tint"].copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError):
        r.AdjustCloud(colour=bad)
    for scale in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            r.AdjustCloud(opacity=scale)
    with pytest.raises(_capi.MsplatError) as e:                  # good arguments, no cloud
        r.AdjustCloud(colour=MAPS["tint"], opacity=0.5)
    assert e.value.code == _capi.ERR_NO_CLOUD


def test_the_helper_matrices():
    t = splatapult_amd.tint_matrix((1.0, 0.55, 0.1), 0.35)
    assert t.dtype == np.float32 and t.shape == (3, 4)
    same_bits(t, MAPS["tint"], "tint_matrix")
    same_bits(splatapult_amd.tint_matrix((0.2, 0.3, 0.4), 0.0), MAPS["identity"], "a tint of weight 0")
    np.testing.assert_array_equal(splatapult_amd.tint_matrix((0.25, 0.5, 0.75), 1.0), np.array([[0, 0, 0, 0.25], [0, 0, 0, 0.5], [0, 0, 0, 0.75]], np.float32))
    same_bits(splatapult_amd.gain_matrix(1.0), MAPS["identity"], "a gain of 1")
    same_bits(splatapult_amd.gain_matrix(4.0, (-0.2, 0.05, 0.3)), MAPS["gain4"], "gain_matrix")
    np.testing.assert_array_equal(splatapult_amd.gain_matrix((1.0, 2.0, 3.0), 0.5), np.array([[1, 0, 0, 0.5], [0, 2, 0, 0.5], [0, 0, 3, 0.5]], np.float32))
    with pytest.raises(ValueError):
        splatapult_amd.tint_matrix((1.0, 0.5), 0.5)
    # the ABI's order: column-major, G's columns, then o
    np.testing.assert_array_equal(ar.abi(MAPS["gain4"]), np.array([4, 0, 0, 0, 4, 0, 0, 0, 4, -0.2, 0.05, 0.3], np.float32))


def test_the_shim_with_adjust_cloud_compiles_with_gxx_and_refuses_without_a_cloud(tmp_path):
    import subprocess
    src = tmp_path / "adjust_shim.cpp"
    src.write_text("""
#include "splatapult_amd/host/msplat_host.hpp"
int main()
{
    SplatRenderer r;
    const float tint[12] = {0.5f, 0, 0, 0, 0.5f, 0, 0, 0, 0.5f, 0.5f, 0.25f, 0};
    bool ok = !r.AdjustCloud(tint) && !r.AdjustCloud(nullptr, 0.5f) && !r.AdjustCloud(tint, 0.5f, nullptr);      // no cloud (Init first)
    ok = ok && msplat_adjust_cloud(nullptr, tint, 1.0f, nullptr, 0, MSPLAT_ADJUST_COLOUR | MSPLAT_ADJUST_OPACITY) == MSPLAT_ERR_INVALID_ARG;
    return ok ? 0 : 1;
}
""")
    exe, libdir = str(tmp_path / "adjust_shim"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, cwd=ROOT)
    assert subprocess.run([exe], cwd=ROOT, capture_output=True, timeout=60).returncode == 0
