"""CPU tests of the downloads into device memory and msplat_export_ply, no device: the four entry points exist
in the header, the library and the binding -- with the header's argument lists -- and refuse a NULL context; the shim's and the
Python class's methods refuse without a context; and the per-splat rule of tests/egress_rule.py, which the GPU tests hold the
kernels to, equals what GaussianCloud.ExportPly writes on every hostile family and sits inside the covariance bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from tests import egress_rule as er
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "msplat.h")
DECLS = (
    "int msplat_download_cloud_device(msplat_ctx* ctx, void* d_aos, uint64_t cap_bytes);",
    "int msplat_download_attributes_device(msplat_ctx* ctx, uint64_t n, float* d_xyz, float* d_f_dc, float* d_f_rest, float* d_opacity, "
    "float* d_log_scale, float* d_rot);",
    "int msplat_download_ply_vertices_device(msplat_ctx* ctx, void* d_vertices, uint64_t cap_bytes, const msplat_ply_layout* layout);",
    "int msplat_export_ply(msplat_ctx* ctx, const char* path);",
)
# how _capi writes the header's argument types
CTYPES = {"msplat_ctx*": C.c_void_p, "void*": C.c_void_p, "float*": C.c_void_p, "uint64_t": C.c_uint64, "const char*": C.c_char_p,
          "const msplat_ply_layout*": C.POINTER(_capi.PlyLayout)}


def test_the_header_declares_the_calls_and_the_binding_has_their_argument_lists():
    header = open(HEADER).read()
    lib = C.CDLL(_capi.LIB_PATH)
    protos = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    for decl in DECLS:
        name = re.match(r"int (\w+)\(", decl).group(1)
        assert decl in header, name
        assert header.index("int msplat_download_cloud(") < header.index(decl)
        assert hasattr(lib, name), "libmsplat.so does not export " + name
        args = [a.strip().rsplit(" ", 1)[0] for a in re.search(r"\((.*?)\);", decl).group(1).split(",")]
        assert protos.get(name) == (C.c_int, [CTYPES[a] for a in args]), (name, args, protos.get(name))
    for method in ("ExportPly", "DownloadTensors", "DownloadDevice"):
        assert callable(getattr(SplatRenderer, method, None)), "SplatRenderer has no " + method
    for word in ("0.5 (V + V^T)", "(0,1), (0,2), (1,2)", "at most 32", "f_rest_0..44", "-logf((1.0f / g[3]) - 1.0f)", "logf(sqrtf(max(eval_k, 0)))"):
        assert word in header, "the header does not state the rule: " + word


def test_a_null_context_is_refused_without_a_device():
    L = _capi.lib()
    lay = _capi.PlyLayout()
    for name, args in (("msplat_download_cloud_device", (None, 0)), ("msplat_download_attributes_device", (0,) + (None,) * 6),
                       ("msplat_download_ply_vertices_device", (None, 0, C.byref(lay))), ("msplat_export_ply", (b"/nonexistent/x.ply",))):
        assert getattr(L, name)(None, *args) == _capi.ERR_INVALID_ARG, name
        assert name + ": ctx is NULL" in L.msplat_last_error(None).decode()
    assert not os.path.exists("/nonexistent/x.ply")


def test_a_renderer_without_a_context_fails_without_raising(tmp_path):
    r = SplatRenderer()
    path = tmp_path / "none.ply"
    assert r.ExportPly(path) is False and "no context" in r.last_error() and not path.exists()
    assert r.DownloadTensors() is None and "no context" in r.last_error()
    assert r.DownloadDevice(0, 0) is False and "no context" in r.last_error()


def test_the_shim_compiles_with_gxx_and_refuses_a_device_group_and_a_missing_cloud(tmp_path):
    src = tmp_path / "download_shim.cpp"
    src.write_text("""
#include "splatapult_amd/host/msplat_host.hpp"
struct Grouped : SplatRenderer {      // a renderer that believes it drives a device group (never dereferenced, never destroyed)
    Grouped() { group = reinterpret_cast<msplat_group*>(this); }
    ~Grouped() { group = nullptr; }
};
int main()
{
    SplatRenderer r;
    float x = 0.0f;
    bool ok = !r.ExportPly("never_written.ply") && !r.DownloadDevice(&x, 4) && !r.DownloadDeviceAttributes(1, &x, &x, nullptr, &x, &x, &x);
    Grouped g;
    ok = ok && !g.ExportPly("never_written.ply") && !g.DownloadDevice(&x, 4) && !g.DownloadDeviceAttributes(1, &x, &x, &x, &x, &x, &x);
    ok = ok && msplat_export_ply(nullptr, "never_written.ply") == MSPLAT_ERR_INVALID_ARG;
    return ok ? 0 : 1;
}
""")
    exe, libdir = str(tmp_path / "download_shim"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, cwd=ROOT)
    run = subprocess.run([exe], cwd=str(tmp_path), capture_output=True, timeout=60)
    assert run.returncode == 0, run.stderr.decode()
    log = run.stderr.decode()
    assert log.count("a device group has no download") == 3 and log.count("no cloud (Init first)") == 3, log
    assert not (tmp_path / "never_written.ply").exists()


@pytest.mark.parametrize("family", er.FAMILIES)
def test_the_rule_is_what_gaussian_cloud_export_ply_writes_and_sits_inside_the_bound(family, tmp_path):
    """xyz, f_dc and f_rest equal as uint32, rot within 2^-22, opacity and scale rtol 1e-6 with equal infinities (numpy's log against
    glibc's); and the rule alone is inside the covariance bound, so the bound cannot hide a rule that drifted"""
    rec = er.family_records(family)
    assert rec.shape == ((5 if family == "hand" else er.N_FAMILY), 61)
    path = str(tmp_path / "host.ply")
    assert er.host_cloud(rec).ExportPly(path)
    header, block = er.read_ply(path)
    assert block.shape == (rec.shape[0], 62) and (block[:, 3:6] == 0).all()
    rule = er.export_rule(rec)
    er.close_to_rule(rule, er.block_attrs(block), family)
    worst = er.check_covariance(rule, rec, family)
    print("%s: the rule's worst covariance error is %.3g of the largest entry" % (family, worst))
    if family == "hand":
        assert (rule["rot"][:2] == np.array([1, 0, 0, 0], np.float32)).all() and (rule["log_scale"][0] == -np.inf).all()
        np.testing.assert_allclose(rule["log_scale"][1], np.log(np.sqrt(np.float32(0.005))), rtol=1e-6)
        assert rule["opacity"][2] == -np.inf and rule["opacity"][3] == np.inf
        assert rec[4, 17] != rec[4, 19]


def test_the_rule_on_records_without_full_sh_and_the_vertex_block_round_trip():
    rec = er.family_records("generate")[:65, :25]
    rule = er.export_rule(rec)
    assert (rule["f_rest"] == 0).all() and rule["xyz"].shape == (65, 3)
    for full in (True, False):
        block = er.vertex_block(rule, full)
        assert block.shape == (65, 62 if full else 17)
        back = er.block_attrs(block)
        for k in er.NAMES:
            np.testing.assert_array_equal(np.asarray(back[k]).reshape(np.asarray(rule[k]).shape), rule[k])
    assert len(er.ply_names(True)) == 62 and len(er.ply_names(False)) == 17
