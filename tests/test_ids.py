"""CPU tests of the id frame (msplat_render_ids, msplat_mark_ids): the entry points and the wrappers exist, what
they refuse without a device, what the Python wrappers check before the library is called, the C++ shim compiles, and the cases of
tests/test_gpu_ids.py are what they claim -- few undecided pixels, many distinct ids, pixels no splat reaches (tests/ids_rule.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from tests import ids_rule
from tests.conftest import ROOT

NEW = ("msplat_render_ids", "msplat_mark_ids")
IDENT = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
VIEW = (np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), [0, 0, 64, 48], [0.1, 10.0])


def test_the_library_exports_the_entry_points_and_the_wrappers_exist():
    L = C.CDLL(_capi.LIB_PATH)
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), "libmsplat.so does not export " + name
        assert name in bound, "no ctypes prototype for " + name
    for method in ("RenderIds", "Pick", "MarkIds"):
        assert callable(getattr(SplatRenderer, method, None)), "SplatRenderer has no " + method
    assert _capi.ID_NONE == ids_rule.NONE == 0xFFFFFFFF
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    assert "#define MSPLAT_ID_NONE 0xFFFFFFFFu" in header
    for word in ("the device group", "two views in one chain", "an occluder plane for the id walk"):      # said to be out of scope
        assert word in header, word


def test_refusals_that_need_no_device():
    L = _capi.lib()
    err = lambda: L.msplat_last_error(None).decode()
    vp, nf = (C.c_float * 4)(0, 0, 64, 48), (C.c_float * 2)(0.1, 10.0)
    ids = np.zeros((48, 64), np.uint32)
    assert L.msplat_render_ids(None, IDENT, IDENT, vp, nf, None, ids.ctypes.data, 0, None, 0, 0) == _capi.ERR_INVALID_ARG
    assert "ctx is NULL" in err()
    assert L.msplat_render_ids(None, IDENT, IDENT, vp, nf, (C.c_int32 * 4)(0, 0, 1, 1), None, 0, None, 0, 1) == _capi.ERR_INVALID_ARG
    assert "ctx is NULL" in err()
    assert L.msplat_mark_ids(None, None, 0, 0, 0, None, 0, None, 0, 0) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    assert not ids.any()


class _NoLibrary:                   # any call on it is a failure of the test
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def _renderer(n=10):
    r = SplatRenderer()
    r._lib, r._n, r._ctx = _NoLibrary(), n, 1
    return r


def test_render_ids_checks_its_arguments_before_the_library():
    r = _renderer()
    for window in ((0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 2, 2), (0, -1, 2, 2), (60, 0, 5, 1), (0, 40, 1, 9), (0, 0, 65, 48), (64, 48, 1, 1)):
        with pytest.raises(ValueError, match="not inside"):
            r.RenderIds(*VIEW, window=window)
    for window in ((0, 0, 1), (0, 0, 1, 1, 1), (0.5, 0, 1, 1)):
        with pytest.raises(ValueError, match="four integers"):
            r.RenderIds(*VIEW, window=window)
    for out in (np.zeros((48, 64), np.int32), np.zeros((48, 64), np.float32), np.zeros((64, 48), np.uint32), np.zeros((48, 64, 1), np.uint32),
                np.zeros((48, 128), np.uint32)[:, ::2], [[0] * 64] * 48):
        with pytest.raises(ValueError, match="uint32 array of shape"):
            r.RenderIds(*VIEW, out=out)
    with pytest.raises(ValueError, match=r"shape \(9, 40\)"):                 # the planes are the WINDOW's
        r.RenderIds(*VIEW, window=(13, 27, 40, 9), out=np.zeros((48, 64), np.uint32))
    for depth in (np.zeros((48, 64), np.float64), np.zeros((48, 63), np.float32)):
        with pytest.raises(ValueError, match="float32 array of shape"):
            r.RenderIds(*VIEW, depth=depth)
    for pitch in (4 * 64 - 4, 4 * 64 + 2, 3):
        with pytest.raises(ValueError, match="pitch_bytes must be 0"):
            r.RenderIds(*VIEW, out_ptr=4096, pitch_bytes=pitch)
        with pytest.raises(ValueError, match="depth_pitch_bytes must be 0"):
            r.RenderIds(*VIEW, out_ptr=4096, depth_ptr=8192, depth_pitch_bytes=pitch)
    with pytest.raises(ValueError, match="pitch_bytes must be 0"):            # 4 w of the window, not of the viewport
        r.RenderIds(*VIEW, window=(0, 0, 40, 9), out_ptr=4096, pitch_bytes=4 * 39)
    with pytest.raises(ValueError, match="one memory space"):
        r.RenderIds(*VIEW, out_ptr=4096, depth=True)
    with pytest.raises(ValueError, match="one memory space"):
        r.RenderIds(*VIEW, depth_ptr=4096)
    with pytest.raises(ValueError, match="tight rows"):
        r.RenderIds(*VIEW, pitch_bytes=512)


def test_mark_ids_checks_its_arguments_before_the_library():
    r = _renderer()
    with pytest.raises(ValueError, match="negative"):
        r.MarkIds(4096, 0, -1, 4, 8192, 0)
    for value in (-1, 256):
        with pytest.raises(ValueError, match="one byte"):
            r.MarkIds(4096, 0, 4, 4, 8192, value)
    for pitch in (12, 18):
        with pytest.raises(ValueError, match="pitch_bytes must be 0"):
            r.MarkIds(4096, pitch, 4, 4, 8192, 1)
    with pytest.raises(ValueError, match="region_pitch_bytes"):
        r.MarkIds(4096, 0, 4, 4, 8192, 1, region_ptr=12288, region_pitch_bytes=3)
    for ids_ptr, mask_ptr in ((0, 8192), (None, 8192), (4096, 0), (4096, None)):
        with pytest.raises(ValueError, match="device pointers"):
            r.MarkIds(ids_ptr, 0, 4, 4, mask_ptr, 1)
    r._ctx = None
    with pytest.raises(_capi.MsplatError, match="no cloud"):
        r.MarkIds(4096, 0, 4, 4, 8192, 1)


def test_the_cpp_shim_has_the_three_calls_and_compiles(tmp_path):
    src = tmp_path / "ids_shim.cpp"
    src.write_text('#include "splatapult_amd/host/msplat_host.hpp"\n'
                   "int main() {\n"
                   "    SplatRenderer r;\n"
                   "    msplat::mat4 m{};\n    msplat::vec4 vp{{0.0f, 0.0f, 64.0f, 48.0f}};\n    msplat::vec2 nf{{0.1f, 10.0f}};\n"
                   "    uint32_t ids[4] = {0, 0, 0, 0}, index = 0;\n    float z[4], zw = 0.0f;\n    const int32_t window[4] = {1, 2, 2, 2};\n"
                   "    bool ok = r.RenderIds(m, m, vp, nf, window, ids, 0, z, 0, false);\n"
                   "    ok = r.Pick(m, m, vp, nf, 3, 4, &index, &zw) || ok;\n"
                   "    ok = r.MarkIds(ids, 0, 2, 2, (uint8_t*)ids, 4, 1, nullptr, 0) || ok;\n"
                   "    return ok ? 1 : 0;\n}\n")      # without an Init every call refuses
    exe = str(tmp_path / "ids_shim")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, "-I", os.path.join(ROOT, "splatapult_amd", "host"), str(src),
                    "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe], check=True, cwd=ROOT)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr.count("no cloud (Init first)") == 3, (p.returncode, p.stderr)
    example = open(os.path.join(ROOT, "splatapult_amd", "host", "example_render.cpp")).read()
    assert "--pick" in example and "renderer.Pick(" in example


@pytest.mark.parametrize("name,distinct", [("hand_placed", 5), ("sparse", 5000)])
def test_the_cases_are_what_they_claim(name, distinct):
    """Conditions on the fixtures, not measurements: at most 1 % of the pixels undecided (here: 0.16 % and 0.14 %), at least 5 of
    hand_placed's 8 splats and 5000 of sparse's 20 k shown (6 and 10 685), pixels no splat reaches in both"""
    ref = ids_rule.reference(name)
    aos, _, W, H, _ = ids_rule.case(name)
    ids = ref["id"]
    assert ids.shape == (H, W) and ids.dtype == np.uint32
    undecided = 1.0 - ref["decided"].mean()
    shown = np.unique(ids[ids != ids_rule.NONE])
    print("%s: %.3f %% undecided, %d distinct ids, %d pixels no splat reaches" % (name, 100 * undecided, shown.size, (ids == ids_rule.NONE).sum()))
    assert undecided <= 0.01, undecided
    assert shown.size >= distinct and shown.max() < aos.shape[0], (shown.size, shown.max())
    assert (ids == ids_rule.NONE).any() and ((ids == ids_rule.NONE) & ref["decided"]).any()
    # the planes hang together: NONE exactly where nothing contributes, with depth 1.0; a winner is a drawn splat and beats the second
    assert ((ids == ids_rule.NONE) == (ref["best"] == 0.0)).all() and (ref["zw"][ids == ids_rule.NONE] == 1.0).all()
    assert (ref["best"] >= ref["second"]).all() and (ref["second"] >= 0.0).all() and (ref["best"] <= 1.0).all()
    won = ref["rank"][ids != ids_rule.NONE]
    assert (ref["splats"]["reject"][won] == 0).all() and (ref["splats"]["index"][won] == ids[ids != ids_rule.NONE]).all()


def test_the_definition_on_splats_placed_by_hand():
    """definition_f64 against a pixel-by-pixel restatement without the bounding rectangles, and its tie rule: of two identical
    splats the nearer keeps the pixel although the farther contributes as much"""
    splats = ids_rule.reference("hand_placed")["splats"]
    _, _, W, H, _ = ids_rule.case("hand_placed")
    ref = ids_rule.definition_f64(splats, W, H)
    fx, fy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    best, T, ids = np.zeros((H, W)), np.ones((H, W)), np.full((H, W), ids_rule.NONE, np.uint32)
    for s in splats[::-1]:
        dx, dy = fx - float(s["px"]), fy - float(s["py"])
        inv = s["inv"].astype(np.float64)
        w = float(s["alpha"]) * np.exp(-0.5 * (dx * (inv[0] * dx + inv[2] * dy) + dy * (inv[1] * dx + inv[3] * dy)))
        w[w <= 1.0 / 256.0] = 0.0
        better = T * w > best
        best, ids = np.where(better, T * w, best), np.where(better, s["index"], ids)
        T *= 1.0 - w
    np.testing.assert_array_equal(ref["id"], ids)
    np.testing.assert_array_equal(ref["best"], best)
    # the tie: at the shared centre the near splat has w = 0.5, so c = 0.5; the far one has w = 1, so c = 0.5 * 1
    two = splats[:2].copy()
    two["px"], two["py"], two["reject"] = 8.5, 8.5, 0
    two["cov"], two["inv"] = (4.0, 0.0, 0.0, 4.0), (0.25, 0.0, 0.0, 0.25)
    two["alpha"], two["index"] = (1.0, 0.5), (7, 3)          # draw order: the far one first
    tie = ids_rule.definition_f64(two, 17, 17)
    assert tie["best"][8, 8] == 0.5 and tie["second"][8, 8] == 0.5 and tie["id"][8, 8] == 3
    assert not ids_rule.decided(tie)[8, 8]
