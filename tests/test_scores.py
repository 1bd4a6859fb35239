"""CPU tests of the score frame (msplat_render_scores, msplat_mark_scores): the entry points and the wrappers
exist, what they refuse without a device, what the Python wrappers check before the library is called, the C++ shim compiles, and
tests/scores_rule.py is what tests/test_gpu_scores.py takes it for -- the fp32 restatement of the kernel's walk stays three orders
of magnitude inside the bound, the bound cannot hide a failure, the designed case stack() is what it claims."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from tests import scores_rule as sr
from tests.conftest import ROOT

NEW = ("msplat_render_scores", "msplat_mark_scores")
IDENT = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
VIEW = (np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), [0, 0, 64, 48], [0.1, 10.0])


def test_the_library_exports_the_entry_points_and_the_wrappers_exist():
    L = C.CDLL(_capi.LIB_PATH)
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), "libmsplat.so does not export " + name
        assert name in bound, "no ctypes prototype for " + name
    for method in ("RenderScores", "MarkScores"):
        assert callable(getattr(SplatRenderer, method, None)), "SplatRenderer has no " + method
    assert _capi.SCORE_ONE == sr.ONE == 2 ** 23
    assert (_capi.SCORE_BELOW, _capi.SCORE_AT_LEAST) == (sr.BELOW, sr.AT_LEAST) == (0, 1)
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    assert "#define MSPLAT_SCORE_ONE 8388608u" in header
    assert "enum { MSPLAT_SCORE_BELOW = 0, MSPLAT_SCORE_AT_LEAST = 1 };" in header
    for word in ("the device group", "host-memory arrays", "two views in one chain", "an occluder plane for the score walk"):      # out of scope
        assert word in header, word


def test_refusals_that_need_no_device():
    L = _capi.lib()
    err = lambda: L.msplat_last_error(None).decode()
    vp, nf = (C.c_float * 4)(0, 0, 64, 48), (C.c_float * 2)(0.1, 10.0)
    assert L.msplat_render_scores(None, IDENT, IDENT, vp, nf, None, None, 0, None, None, 0) == _capi.ERR_INVALID_ARG
    assert "ctx is NULL" in err()
    assert L.msplat_render_scores(None, IDENT, IDENT, vp, nf, (C.c_int32 * 4)(0, 0, 1, 1), None, 0, C.c_void_p(4096), None, 4) == _capi.ERR_INVALID_ARG
    assert "ctx is NULL" in err()
    assert L.msplat_mark_scores(None, None, 0, 0, 0, None, 0) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()


class _NoLibrary:                   # any call on it is a failure of the test
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def _renderer(n=10):
    r = SplatRenderer()
    r._lib, r._n, r._ctx = _NoLibrary(), n, 1
    return r


def test_the_wrappers_check_their_arguments_before_the_library():
    import torch
    r = _renderer()
    for window in ((0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 2, 2), (60, 0, 5, 1), (0, 40, 1, 9), (0, 0, 65, 48), (64, 48, 1, 1)):
        with pytest.raises(ValueError, match="not inside"):
            r.RenderScores(*VIEW, window=window)
    for window in ((0, 0, 1), (0.5, 0, 1, 1)):
        with pytest.raises(ValueError, match="four integers"):
            r.RenderScores(*VIEW, window=window)
    for region in (torch.zeros((48, 64), dtype=torch.int32), torch.zeros((64, 48), dtype=torch.uint8), torch.zeros((48, 128), dtype=torch.uint8)[:, ::2],
                   [[0] * 64] * 48):
        with pytest.raises(ValueError, match="region must be a uint8 / bool plane"):
            r.RenderScores(*VIEW, region=region)
    with pytest.raises(ValueError, match=r"shape \(9, 40\)"):                 # the region is the WINDOW's
        r.RenderScores(*VIEW, window=(13, 27, 40, 9), region=torch.zeros((48, 64), dtype=torch.uint8))
    with pytest.raises(ValueError, match="region must live on"):
        r.RenderScores(*VIEW, region=torch.zeros((48, 64), dtype=torch.uint8))
    for score in (torch.zeros(10, dtype=torch.int32), torch.zeros(11, dtype=torch.int64), torch.zeros(20, dtype=torch.int64)[::2], np.zeros(10, np.int64)):
        with pytest.raises(ValueError, match="score must be a contiguous torch int64 tensor"):
            r.RenderScores(*VIEW, score=score)
    with pytest.raises(ValueError, match="score must live on device"):
        r.RenderScores(*VIEW, score=torch.zeros(10, dtype=torch.int64))
    with pytest.raises(ValueError, match="goes with a score tensor"):
        r.RenderScores(*VIEW, pixels=torch.zeros(10, dtype=torch.int32))
    for op in ("above", 1, None):
        with pytest.raises(ValueError, match="op must be one of"):
            r.MarkScores(torch.zeros(10, dtype=torch.int64), op, 0, torch.zeros(10, dtype=torch.uint8), 1)
    for value in (-1, 256):
        with pytest.raises(ValueError, match="one byte"):
            r.MarkScores(torch.zeros(10, dtype=torch.int64), "below", 0, torch.zeros(10, dtype=torch.uint8), value)
    for threshold in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="unsigned 64-bit"):
            r.MarkScores(torch.zeros(10, dtype=torch.int64), "below", threshold, torch.zeros(10, dtype=torch.uint8), 0)
    with pytest.raises(ValueError, match="mask must be a torch uint8 / bool tensor"):
        r.MarkScores(torch.zeros(10, dtype=torch.int64), "below", 1, np.zeros(10, np.uint8), 0)
    with pytest.raises(ValueError, match="score must live on device"):
        r.MarkScores(torch.zeros(10, dtype=torch.int64), "below", 1, torch.zeros(10, dtype=torch.uint8), 0)


def test_the_cpp_shim_has_the_two_calls_and_compiles(tmp_path):
    src = tmp_path / "scores_shim.cpp"
    src.write_text('#include "splatapult_amd/host/msplat_host.hpp"\n'
                   "int main() {\n"
                   "    SplatRenderer r;\n"
                   "    msplat::mat4 m{};\n    msplat::vec4 vp{{0.0f, 0.0f, 64.0f, 48.0f}};\n    msplat::vec2 nf{{0.1f, 10.0f}};\n"
                   "    uint64_t score[4] = {0, 0, 0, 0};\n    uint32_t hits[4] = {0, 0, 0, 0};\n    uint8_t mask[4] = {1, 1, 1, 1};\n"
                   "    const int32_t window[4] = {1, 2, 2, 2};\n"
                   "    bool ok = r.RenderScores(m, m, vp, nf, window, score, 4, hits, nullptr, 0);\n"
                   "    ok = r.RenderScores(m, m, vp, nf, nullptr, score, 4) || ok;\n"
                   "    ok = r.MarkScores(score, 4, MSPLAT_SCORE_BELOW, 3 * (uint64_t)MSPLAT_SCORE_ONE, mask, 0) || ok;\n"
                   "    return ok ? 1 : 0;\n}\n")      # without an Init every call refuses
    exe = str(tmp_path / "scores_shim")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, "-I", os.path.join(ROOT, "splatapult_amd", "host"), str(src),
                    "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe], check=True, cwd=ROOT)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr.count("no cloud (Init first)") == 3, (p.returncode, p.stderr)
    example = open(os.path.join(ROOT, "splatapult_amd", "host", "example_render.cpp")).read()
    assert "--min-score" in example and "renderer.RenderScores(" in example and "renderer.MarkScores(" in example


@pytest.mark.parametrize("name", sr.CASES)
def test_the_fp32_walk_stays_inside_the_bound_and_the_bound_cannot_hide_a_failure(name):
    """The kernel's arithmetic restated in numpy against the float64 definition: worst err / bound 4.2e-5 (hand_placed) and 5.8e-4
    (sparse), so the bound has three orders of magnitude over fp32 rounding.  Conditions on the fixtures, not measurements: the
    flip allowances sum to at most 1e-3 of the scores (1.9e-5, 2.5e-6), and at most 1 % of the drawn splats have a score below
    their own bound, so that 0 would pass for them (0 of 8, 4 of 18 559)."""
    ref = sr.reference(name)
    _, _, W, H, _ = sr.case(name)
    score, pixels = sr.restate_f32(ref["splats"], W, H)
    err = np.abs(score.astype(np.float64) / sr.ONE - ref["S"])
    drawn = ref["A"] > 0
    ratio = (err[drawn] / ref["bound"][drawn]).max()
    share = (ref["S"][drawn] < ref["bound"][drawn]).mean()
    print("%s: worst err / bound %.3g; sum F / sum S %.3g; %d drawn, %.3g %% of them below their bound"
          % (name, ratio, ref["F"].sum() / ref["S"].sum(), drawn.sum(), 100 * share))
    assert (err <= ref["bound"]).all(), ratio
    assert not score[~drawn].any() and not pixels[~drawn].any() and not ref["S"][~drawn].any()
    assert ref["F"].sum() <= 1e-3 * ref["S"].sum()
    assert share <= 0.01, share
    assert (pixels <= ref["A"]).all() and (pixels >= ref["sure"]).all()
    assert (ref["sure"] > 0).sum() >= 0.5 * drawn.sum(), "the lower bound on the hit counts says nothing"


def test_the_stack_is_what_it_claims():
    ref = sr.reference("stack")
    aos, W, H, _ = sr.stack()
    n = aos.shape[0]
    assert (W, H, n, ref["V"]) == (48, 48, 12, 12) and (ref["splats"]["reject"] == 0).all()
    assert (ref["splats"]["index"] == np.arange(n)[::-1]).all(), "twelve distinct depths, the first splat in front"
    S, tile = sr.per_upload_index(ref, ref["S"]), sr.per_upload_index(ref, ref["tile"])
    assert (ref["A"] == W * H).all() and not ref["F"].any()
    # w is the alpha to within 1e-3 over the central 32 x 32 pixels -- here over the whole viewport: T = 0.1^k behind the k-th
    alpha = np.array(sr.STACK_ALPHA)
    T = np.concatenate([[1.0], np.cumprod(1.0 - alpha)])[:n]
    np.testing.assert_allclose(S[:11], (W * H * T * alpha)[:11], rtol=1e-3, atol=0)
    assert T[8] < sr.STOP < T[7] and T[11] == 0.0               # (in float64 the eleventh's w is 1 - 1e-9: the twelfth sees T of 1e-19)
    peak = sr.per_upload_index(ref, ref["peak"])
    assert (peak[[8, 9, 11]] < sr.STOP).all() and peak[7] > sr.STOP, "splats 9, 10 and 12: below 2^-24 per pixel everywhere"
    assert (tile * sr.ONE <= 2.0 ** 31).all() and tile[0] * sr.ONE > 2.0 ** 30, "a central tile of the front splat: above 2^30, at most 2^31"
    # the eleventh splat's w rounds to 1.0f at the centre pixels: alpha and the Gaussian both
    s = ref["splats"][n - 1 - 10]
    assert s["index"] == 10 and np.float32(s["alpha"]) == np.float32(1.0)
    d = np.array([23.5, 24.5]) - float(s["px"])
    assert np.float32(np.exp(-0.5 * float(s["inv"][0]) * 2.0 * (d ** 2).max())) == np.float32(1.0)
    # the fp32 walk: the ninth to twelfth score nothing at all, the first eight on every pixel
    score, pixels = sr.restate_f32(ref["splats"], W, H)
    score, pixels = sr.per_upload_index(ref, score), sr.per_upload_index(ref, pixels)
    assert not score[8:].any() and not pixels[8:].any() and (pixels[:8] == W * H).all()
    assert (np.abs(score / sr.ONE - S) <= sr.per_upload_index(ref, ref["bound"])).all()


def test_mark_reference_on_vectors_written_by_hand():
    score = np.array([0, 1, 5, 5, 6, 2 ** 63, 2 ** 64 - 1], np.uint64)
    ones, zeros = np.ones(7, np.uint8), np.zeros(7, np.uint8)
    np.testing.assert_array_equal(sr.mark_reference(score, sr.BELOW, 5, ones, 0), [0, 0, 1, 1, 1, 1, 1])          # score == threshold stays
    np.testing.assert_array_equal(sr.mark_reference(score, sr.AT_LEAST, 5, zeros, 1), [0, 0, 1, 1, 1, 1, 1])       # ... and is selected
    np.testing.assert_array_equal(sr.mark_reference(score, sr.BELOW, 0, ones, 0), ones)                             # nothing is below 0
    np.testing.assert_array_equal(sr.mark_reference(score, sr.AT_LEAST, 0, zeros, 9), np.full(7, 9))
    np.testing.assert_array_equal(sr.mark_reference(score, sr.BELOW, 2 ** 63, ones, 0), [0, 0, 0, 0, 0, 1, 1])     # unsigned compare
    np.testing.assert_array_equal(sr.mark_reference(score, sr.AT_LEAST, 2 ** 64 - 1, zeros, 1), [0, 0, 0, 0, 0, 0, 1])
    start = np.array([3, 4, 5, 6, 7, 8, 9], np.uint8)
    np.testing.assert_array_equal(sr.mark_reference(score, sr.BELOW, 6, start, 200), [200, 200, 200, 200, 7, 8, 9])  # other bytes stay
    assert start[0] == 3, "the input mask was written"
    int64_view = score.view(np.int64)                               # what the torch tensors hold: the same bits
    np.testing.assert_array_equal(sr.mark_reference(int64_view, sr.BELOW, 2 ** 63, ones, 0), [0, 0, 0, 0, 0, 1, 1])
