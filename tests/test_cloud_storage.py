"""CPU tests of the opt-in fp16 storage of the higher-order SH (msplat_set_cloud_storage): the ABI is
declared, exported and bound, NULL handles and unknown kinds are refused, the Python and C++ surfaces take the option."""
import ctypes as C
import os
import re
import subprocess

import pytest

from splatapult_amd import SplatRenderer, _capi
from splatapult_amd.renderer import SplatRendererGroup
from tests.conftest import ROOT

ENTRY_POINTS = ("msplat_set_cloud_storage", "msplat_get_cloud_storage", "msplat_group_set_cloud_storage")


def _header():
    return open(os.path.join(ROOT, "include", "msplat.h")).read()


def test_storage_enum_is_declared_and_matches_the_bindings():
    m = re.search(r"enum\s*\{\s*MSPLAT_STORAGE_FP32\s*=\s*(\d+)\s*,\s*MSPLAT_STORAGE_SH_FP16\s*=\s*(\d+)\s*\}", _header())
    assert m, "MSPLAT_STORAGE_* enum missing from msplat.h"
    assert (int(m.group(1)), int(m.group(2))) == (_capi.STORAGE_FP32, _capi.STORAGE_SH_FP16) == (0, 1)
    assert _capi.CLOUD_STORAGES == {"fp32": 0, "sh_fp16": 1}


def test_entry_points_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = C.CDLL(_capi.LIB_PATH)
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name + " is not declared in msplat.h"
        assert hasattr(L, name), "libmsplat.so does not export " + name
        assert name in bound, name + " is not bound in _capi.SYMBOLS"


def test_entry_points_refuse_a_null_handle():
    L = _capi.lib()
    for kind in (_capi.STORAGE_FP32, _capi.STORAGE_SH_FP16):
        assert L.msplat_set_cloud_storage(None, kind) == _capi.ERR_INVALID_ARG
        assert L.msplat_group_set_cloud_storage(None, kind) == _capi.ERR_INVALID_ARG
    assert L.msplat_get_cloud_storage(None) == _capi.ERR_INVALID_ARG == -1


@pytest.mark.parametrize("name", ["fp16", "SH_FP16", "bf16", "", None, 1])
def test_renderers_reject_unknown_storage_names(name):
    with pytest.raises(ValueError):
        SplatRenderer(cloud_storage=name)
    with pytest.raises(ValueError):
        SplatRendererGroup([0], cloud_storage=name)


def test_renderers_accept_the_known_storage_names():
    for name in ("fp32", "sh_fp16"):
        r = SplatRenderer(cloud_storage=name)        # nothing touches a device before Init
        assert r.cloud_storage() is None
        SplatRendererGroup([0], cloud_storage=name)


def test_cpp_shim_with_set_cloud_storage_compiles_with_plain_gxx(tmp_path):
    src = tmp_path / "storage_shim.cpp"
    src.write_text('#include "msplat_host.hpp"\n'
                   "int main(int argc, char** argv)\n"
                   "{\n"
                   "    SplatRenderer r;\n"
                   "    r.SetCloudStorage(MSPLAT_STORAGE_SH_FP16);\n"
                   "    r.ConfigureDevices(std::vector<int>{0, 1});\n"
                   "    if (argc > 1) return r.Init(std::make_shared<GaussianCloud>(GaussianCloud::Options{true}), false, false) ? 0 : 1;\n"
                   "    return 0;\n"
                   "}\n")
    exe = str(tmp_path / "storage_shim")
    libdir = os.path.dirname(_capi.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, "-I", os.path.join(ROOT, "splatapult_amd", "host"), str(src),
           "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT)
    assert subprocess.run([exe], capture_output=True).returncode == 0
