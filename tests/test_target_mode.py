"""CPU tests of msplat_set_target_mode (include/msplat.h): the three entry points are exported and bound, NULL handles are
refused, msplat_config keeps its size (the mode is a setter, not a field), and the C++ and Python mirrors carry the setter."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, SplatRendererGroup, _capi, renderer
from tests.conftest import ROOT

NAMES = ("msplat_set_target_mode", "msplat_get_target_mode", "msplat_group_set_target_mode")


def test_the_three_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = C.CDLL(_capi.LIB_PATH)
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n + " is not declared in msplat.h"
        assert hasattr(L, n), "libmsplat.so does not export " + n
        assert n in bound, "the ctypes binding lacks " + n
    # the constants of the header and of the binding agree
    m = re.search(r"enum\s*\{\s*MSPLAT_TARGET_CLEAR\s*=\s*(\d+)\s*,\s*MSPLAT_TARGET_LOAD\s*=\s*(\d+)\s*,\s*MSPLAT_TARGET_PREMULTIPLIED\s*=\s*(\d+)\s*\}", code)
    assert m and [int(v) for v in m.groups()] == [0, 1, 2]
    assert (_capi.TARGET_CLEAR, _capi.TARGET_LOAD, _capi.TARGET_PREMULTIPLIED) == (0, 1, 2)
    assert _capi.TARGET_MODES == {"clear": 0, "load": 1, "premultiplied": 2}


def test_null_handles_are_refused():
    L = _capi.lib()
    for mode in (_capi.TARGET_CLEAR, _capi.TARGET_LOAD, _capi.TARGET_PREMULTIPLIED, 3, -1):
        assert L.msplat_set_target_mode(None, mode) == _capi.ERR_INVALID_ARG
        assert L.msplat_group_set_target_mode(None, mode) == _capi.ERR_INVALID_ARG
    assert "NULL" in L.msplat_last_error(None).decode()
    assert L.msplat_get_target_mode(None) == -1


def test_the_mode_is_a_setter_and_msplat_config_keeps_its_size():
    assert C.sizeof(_capi.Config) == 72
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    cfg = re.search(r"typedef struct msplat_config \{(.*?)\} msplat_config;", header, flags=re.S).group(1)
    assert "target" not in re.sub(r"/\*.*?\*/", "", cfg, flags=re.S)


def test_cpp_shim_with_set_target_mode_compiles_with_plain_gxx(tmp_path):
    src = tmp_path / "target_mode.cpp"
    src.write_text('#include "splatapult_amd/host/msplat_host.hpp"\n'
                   "int main()\n{\n"
                   "    SplatRenderer r;\n"
                   "    bool ok = r.SetTargetMode(MSPLAT_TARGET_LOAD) && r.SetTargetMode(MSPLAT_TARGET_PREMULTIPLIED);\n"
                   "    return ok && msplat_get_target_mode(r.GetContext()) == -1 ? 0 : 1;      // no Init: no context yet\n"
                   "}\n")
    libdir = os.path.dirname(_capi.LIB_PATH)
    exe = str(tmp_path / "target_mode")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, "-I", os.path.join(ROOT, "splatapult_amd", "host"), str(src),
                    "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe], check=True, cwd=ROOT)
    assert subprocess.run([exe]).returncode == 0          # a shim without contexts has nothing to set: true, and no crash
    example = open(os.path.join(ROOT, "splatapult_amd", "host", "example_render.cpp")).read()
    assert "SetTargetMode(MSPLAT_TARGET_LOAD)" in example


def test_python_mirrors_carry_the_setter_and_check_their_arguments():
    assert callable(SplatRenderer.set_target_mode) and callable(SplatRendererGroup.set_target_mode)
    r = SplatRenderer()
    for bad in ("over", None, 1):
        with pytest.raises(ValueError):
            r.set_target_mode(bad)
    assert r.target_mode() is None                          # no context yet
    # "load" blends over the target's contents: a host Render without an out= array has none
    with pytest.raises(ValueError, match="out="):
        renderer._host_frame(_capi.FB_RGBA32F, [0, 0, 8, 4], None, True)
    dst = np.ones((4, 8, 4), np.float32)
    assert renderer._host_frame(_capi.FB_RGBA32F, [0, 0, 8, 4], dst, True) is dst
    assert renderer._host_frame(_capi.FB_RGBA32F, [0, 0, 8, 4]).shape == (4, 8, 4)
