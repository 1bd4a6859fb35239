"""CPU tests of the opt-in 8-bit storage of the higher-order SH (MSPLAT_STORAGE_SH_Q8): the ABI is declared,
exported and bound, NULL handles are refused, the Python and C++ surfaces take the option, and the host quantiser -- the
sh8_pack / sh8_unpack pair every upload route and the download use, reached through msplat_debug_sh_q8_round -- equals the
numpy restatement of the contract (tests/sh_q8_rule.py) bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi, synthetic
from splatapult_amd.renderer import SplatRendererGroup
from tests.conftest import ROOT
from tests.sh_q8_rule import BAND, REST, deq, quantise, special_rest


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def q8_round(recs):
    """msplat_debug_sh_q8_round over (n, 61) records -> (rec_out, steps, codes, non-finite counts)"""
    L = _capi.lib()
    recs = np.ascontiguousarray(recs, np.float32)
    n = recs.shape[0]
    out = np.full((n, 61), np.nan, np.float32)
    steps = np.full((n, 3), np.nan, np.float32)
    codes = np.full((n, 45), 99, np.int8)
    bad = np.zeros(n, np.int64)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int8)
    for i in range(n):
        bad[i] = L.msplat_debug_sh_q8_round(recs[i].ctypes.data_as(fp), out[i].ctypes.data_as(fp), steps[i].ctypes.data_as(fp),
                                            codes[i].ctypes.data_as(ip))
    return out, steps, codes, bad


def assert_equals_the_rule(recs):
    out, steps, codes, bad = q8_round(recs)
    want_codes, want_steps = quantise(recs)
    assert (bad == 0).all()
    np.testing.assert_array_equal(codes, want_codes)
    np.testing.assert_array_equal(bits(steps), bits(want_steps))
    np.testing.assert_array_equal(bits(out), bits(deq(recs)))
    keep = [c for c in range(61) if c not in REST]
    np.testing.assert_array_equal(bits(out[:, keep]), bits(np.asarray(recs, np.float32)[:, keep]))
    return out, steps, codes


def test_storage_constant_is_declared_and_matches_the_bindings():
    m = re.search(r"^enum\s*\{\s*MSPLAT_STORAGE_SH_Q8\s*=\s*(\d+)\s*\};", _read("include", "msplat.h"), flags=re.M)
    assert m, "MSPLAT_STORAGE_SH_Q8 missing from msplat.h"
    assert int(m.group(1)) == _capi.STORAGE_SH_Q8 == 3
    assert _capi.CLOUD_STORAGE_NAMES == {"fp32": 0, "sh_fp16": 1, "sh_q8": 3}
    assert _capi.CLOUD_STORAGES == {"fp32": 0, "sh_fp16": 1}


def test_debug_entry_point_is_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _read("include", "msplat_debug.h"), flags=re.S)
    assert re.search(r"\bint\s+msplat_debug_sh_q8_round\s*\(\s*const\s+float\s+rec_in\[61\]\s*,\s*float\s+rec_out\[61\]\s*,"
                     r"\s*float\s+steps_out\[3\]\s*,\s*int8_t\s+codes_out\[45\]\s*\)", code)
    assert hasattr(C.CDLL(_capi.LIB_PATH), "msplat_debug_sh_q8_round")
    assert "msplat_debug_sh_q8_round" in {n for n, _, _ in _capi.SYMBOLS}


def test_entry_points_refuse_a_null_handle_with_kind_3():
    L = _capi.lib()
    assert L.msplat_set_cloud_storage(None, _capi.STORAGE_SH_Q8) == _capi.ERR_INVALID_ARG
    assert L.msplat_group_set_cloud_storage(None, _capi.STORAGE_SH_Q8) == _capi.ERR_INVALID_ARG
    assert L.msplat_get_cloud_storage(None) == -1
    rec = np.zeros(61, np.float32)
    steps, codes = np.zeros(3, np.float32), np.zeros(45, np.int8)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int8)
    args = [rec.ctypes.data_as(fp), rec.copy().ctypes.data_as(fp), steps.ctypes.data_as(fp), codes.ctypes.data_as(ip)]
    for k in range(4):
        a = list(args)
        a[k] = None
        assert L.msplat_debug_sh_q8_round(*a) == _capi.ERR_INVALID_ARG < 0


def test_renderers_take_sh_q8_without_touching_a_device():
    r = SplatRenderer(cloud_storage="sh_q8")
    assert r.cloud_storage() is None
    SplatRendererGroup([0], cloud_storage="sh_q8")
    for name in ("q8", "SH_Q8", "sh_q4", 3):
        with pytest.raises(ValueError):
            SplatRenderer(cloud_storage=name)
        with pytest.raises(ValueError):
            SplatRendererGroup([0], cloud_storage=name)


def test_quantiser_equals_the_rule_on_10000_synthetic_records():
    aos = synthetic.make_cloud(10_000, full_sh=True).as_array()
    assert aos.shape == (10_000, 61)
    out, steps, codes = assert_equals_the_rule(aos)
    assert (steps > 0).all() and (np.abs(codes).max(axis=1) == 127).all()
    # the documented error bound: half a step (plus the roundings of the quotient and of the product)
    err = np.abs(out[:, REST].astype(np.float64) - aos[:, REST])
    assert (err <= (0.5 + 2.0 ** -16) * steps[:, BAND].astype(np.float64)).all()
    assert err.max() > 0


def test_quantiser_equals_the_rule_on_hand_made_records():
    sp = special_rest()
    recs = synthetic.make_cloud(sp.shape[0], seed=3, full_sh=True).as_array()
    recs[:, REST] = sp
    out, steps, codes = assert_equals_the_rule(recs)
    rest = out[:, REST]
    # the cases, spelled out on band 1 (REST[0:9]) of the first rows (special_rest's order)
    assert steps[0, 0] == 0 and (codes[0, :9] == 0).all() and (bits(rest[0, :9]) == 0).all()                  # zeros
    assert list(codes[1, :9]) == [0, 0, 0, 0, 127, 0, 0, 0, 0] and steps[1, 0] == np.float32(0.3) / np.float32(127)
    assert codes[2, 0] == -127 and codes[2, :9].max() < 127                                                    # negative maximum
    for row, scale in ((3, 1.0), (4, 2.0 ** -10)):                                                            # ties to even
        assert steps[row, 0] == np.float32(scale)
        assert list(codes[row, :9]) == [127, 2, 4, -2, -4, 0, 0, 126, 126]
    assert codes[5, 1] == 0 and bits(rest[5, 1:3]).tolist() == [0, 0]                                          # -0.0 -> +0.0
    assert steps[6, 0] == 0 and (codes[6, :9] == 0).all()                                                      # 2^-65
    assert steps[7, 0] == np.float32(2.0 ** -64) / np.float32(127) and codes[7, 1] == -127   # 2^-64
    assert codes[7, 3] == 0
    assert np.isfinite(rest[8]).all() and codes[8, 8] == 127 and np.abs(rest[8, :9]).max() > 9e29              # 1e30


def test_non_finite_f_rest_values_are_counted():
    recs = synthetic.make_cloud(4, seed=5, full_sh=True).as_array()
    recs[0, REST[3]] = np.nan
    recs[1, REST[0]], recs[1, REST[20]], recs[1, REST[44]] = np.inf, -np.inf, np.nan
    recs[2, REST[44]] = -np.inf
    recs[3, 4] = np.nan                   # a DC term is not f_rest
    out, steps, codes, bad = q8_round(recs)
    assert list(bad) == [1, 3, 1, 0]
    keep = [c for c in range(61) if c not in REST]
    np.testing.assert_array_equal(bits(out[:, keep]), bits(recs[:, keep]))
    # bands without a non-finite value are quantised as ever
    want_codes, want_steps = quantise(recs)
    np.testing.assert_array_equal(codes[0][BAND != 0], want_codes[0][BAND != 0])
    np.testing.assert_array_equal(codes[3], want_codes[3])


def test_cpp_shim_with_sh_q8_compiles_with_plain_gxx(tmp_path):
    src = tmp_path / "storage_q8_shim.cpp"
    src.write_text('#include "msplat_host.hpp"\n'
                   '#include "msplat_debug.h"\n'
                   "int main(int argc, char** argv)\n"
                   "{\n"
                   "    static_assert(MSPLAT_STORAGE_SH_Q8 == 3, \"\");\n"
                   "    SplatRenderer r;\n"
                   "    r.SetCloudStorage(MSPLAT_STORAGE_SH_Q8);\n"
                   "    r.ConfigureDevices(std::vector<int>{0, 1});\n"
                   "    if (argc > 1) return r.Init(std::make_shared<GaussianCloud>(GaussianCloud::Options{true}), false, false) ? 0 : 1;\n"
                   "    float in[61] = {}, out[61], steps[3];\n"
                   "    int8_t codes[45];\n"
                   "    in[5] = 1.0f;\n"
                   "    return msplat_debug_sh_q8_round(in, out, steps, codes) == 0 && codes[0] == 127 ? 0 : 2;\n"
                   "}\n")
    exe = str(tmp_path / "storage_q8_shim")
    libdir = os.path.dirname(_capi.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "splatapult_amd", "host"), str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT)
    assert subprocess.run([exe], capture_output=True).returncode == 0
