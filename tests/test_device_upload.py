"""CPU tests of the uploads from device memory (msplat_upload_cloud_device, msplat_upload_ply_vertices_device,
msplat_upload_attributes_device): the three symbols are exported, declared and bound; each refuses a NULL
context; the C++ shim's InitDevice / InitDeviceAttributes compile with plain g++; the Python mirror refuses tensors that are not
contiguous float32 before it touches a device.  What the calls compute is tests/test_gpu_device_upload.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from tests.conftest import ROOT

NAMES = ("msplat_upload_cloud_device", "msplat_upload_ply_vertices_device", "msplat_upload_attributes_device")


def test_the_three_entry_points_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = C.CDLL(_capi.LIB_PATH)
    bound = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    for name in NAMES:
        assert hasattr(L, name), "libmsplat.so does not export " + name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name + " is not declared in include/msplat.h"
        assert name in bound and bound[name][0] is C.c_int
    assert len(bound["msplat_upload_cloud_device"][1]) == 6
    assert len(bound["msplat_upload_ply_vertices_device"][1]) == 5
    assert len(bound["msplat_upload_attributes_device"][1]) == 9
    assert re.search(r"#define\s+MSPLAT_VERSION\s+1\b", header)


def test_a_null_context_is_an_invalid_argument():
    L = _capi.lib()
    off = _capi.AttrOffsets(0, 16, 32, 48, 64, 76, 88, 100, 116, 132, 148, 164, 180, 196, 212, 228)
    lay = _capi.PlyLayout()
    lay.vertex_size = 248
    assert L.msplat_upload_cloud_device(None, None, 0, 244, C.byref(off), 1) == _capi.ERR_INVALID_ARG
    assert L.msplat_upload_ply_vertices_device(None, None, 0, C.byref(lay), 1) == _capi.ERR_INVALID_ARG
    assert L.msplat_upload_attributes_device(None, 0, None, None, None, None, None, None, 1) == _capi.ERR_INVALID_ARG
    assert b"NULL" in L.msplat_last_error(None)


SHIM_USER = r"""
#include "splatapult_amd/host/msplat_host.hpp"
int main()
{
    SplatRenderer r;
    r.SetFramesInFlight(2);
    r.SetCloudStorage(MSPLAT_STORAGE_SH_FP16);
    msplat_attr_offsets off{};
    bool a = r.InitDevice(nullptr, 0, 244, off, true, false);
    bool b = r.InitDeviceAttributes(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, false);
    SplatRenderer g;
    g.ConfigureDevices({0, 1});
    bool c = g.InitDevice(nullptr, 0, 244, off, true, false);          // refused before a device is touched
    bool d = g.InitDeviceAttributes(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, false);
    return (c || d) ? 2 : ((a && b) ? 0 : 1);
}
"""


def test_the_shim_methods_compile_with_plain_gxx_and_refuse_a_device_group(tmp_path):
    """as tests/test_capi.py compiles the shim: g++ and the C ABI only"""
    src = tmp_path / "shim_user.cpp"
    src.write_text(SHIM_USER)
    exe = str(tmp_path / "shim_user")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir,
                    "-o", exe], check=True, cwd=ROOT)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode in (0, 1), p.stderr                    # 1: no device here (Init -> false after logging); never 2
    assert p.stderr.count("a device group takes no cloud from device memory") == 2, p.stderr


class FakeTensor:
    """the duck-typed surface InitFromTensors reads, over a numpy array (no device needed: the refusals come first)"""

    def __init__(self, a, device_type="cuda"):
        self._a = a
        self.dtype, self.shape = a.dtype, a.shape
        self.device = type("Device", (), {"type": device_type, "index": 0})()

    def is_contiguous(self):
        return bool(self._a.flags["C_CONTIGUOUS"])

    def data_ptr(self):
        raise AssertionError("a refused tensor's pointer is never taken")


def fake_tensors(n=8, **override):
    t = {"xyz": np.zeros((n, 3), np.float32), "f_dc": np.zeros((n, 3), np.float32), "f_rest": np.zeros((n, 45), np.float32),
         "opacity": np.zeros(n, np.float32), "log_scale": np.zeros((n, 3), np.float32), "rot": np.zeros((n, 4), np.float32)}
    t.update(override)
    return [None if v is None else FakeTensor(v) for v in t.values()]


@pytest.mark.parametrize("name", ["xyz", "f_rest", "rot"])
def test_init_from_tensors_refuses_float64_and_strided_input(name):
    good = {"xyz": (8, 3), "f_rest": (8, 45), "rot": (8, 4)}[name]
    r = SplatRenderer()
    with pytest.raises(ValueError, match=name + " must be float32"):
        r.InitFromTensors(*fake_tensors(**{name: np.zeros(good, np.float64)}))
    strided = np.zeros((good[0], 2 * good[1]), np.float32)[:, ::2]
    assert strided.shape == good and not strided.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError, match=name + " must be contiguous"):
        r.InitFromTensors(*fake_tensors(**{name: strided}))
    with pytest.raises(ValueError, match=name + " must have shape"):
        r.InitFromTensors(*fake_tensors(**{name: np.zeros((good[0], good[1] + 1), np.float32)}))
    with pytest.raises(ValueError):
        r.UpdateFromTensors(*fake_tensors(**{name: np.zeros(good, np.float64)}))
    assert r._ctxs == [], "a refused call creates no context"


def test_init_from_tensors_refuses_host_tensors():
    t = fake_tensors()
    t[0] = FakeTensor(np.zeros((8, 3), np.float32), device_type="cpu")
    with pytest.raises(ValueError, match="device memory"):
        SplatRenderer().InitFromTensors(*t)


def test_update_without_a_context_fails_without_raising():
    r = SplatRenderer()
    assert r.UpdateFromDevice(0, 0, 244, [0] * 16, True) is False
    assert "first" in r.last_error()
