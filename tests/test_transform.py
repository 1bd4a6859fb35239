"""CPU tests of msplat_transform_cloud and msplat_sh_rotation, no device: the names exist in the header, the
library and the binding; the refusals that need no device; msplat_sh_rotation against a float64 least-squares fit of its defining
identity (tests/transform_rule.py); and the rule itself -- a splat whose SH follow D shows at Q v the colour it showed at v, S' is
A S A^T, and the project's CPU oracle sees the rule-transformed cloud from the moved camera as it saw the original.

Bounds.  |D - D_ref| <= 1e-5 per entry: entries are at most 1 in magnitude, fp32 rounding contributes 3e-8, the fp32 matrix being
orthonormal to 1e-7 only moves D by a few 1e-7, a wrong sign, order or orientation by 0.1 to 1.  Colour: |sh| <= 1, 15 terms of
|b| < 3 and fp32 sums of at most 7 products: a few 1e-7 against the 1e-5 asserted.  S': 6 fp32 roundings per entry of magnitude
<= |A|^2 max |S|, against 1e-5 (1 + max |S|)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import SplatRenderer, _capi
from tests import scenes
from tests import transform_harness as th
from tests import transform_rule as tr
from tests import visibility_rule as vr
from tests.checks import check_image
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "msplat.h")
MATS = tr.matrices()


def test_the_header_declares_the_calls_the_library_exports_them_and_the_binding_has_them():
    header = open(HEADER).read()
    assert "enum { MSPLAT_TRANSFORM_KEEP_SH = 1 };" in header
    assert "int msplat_sh_rotation(const float M[16], float d1[9], float d2[25], float d3[49], float* scale_out);" in header
    assert "int msplat_transform_cloud(msplat_ctx* ctx, const float M[16], const uint8_t* d_select, uint64_t n, int32_t flags);" in header
    assert len(header.splitlines()) <= 300
    L = C.CDLL(_capi.LIB_PATH)
    names = {n for n, _, _ in _capi.SYMBOLS}
    for name in ("msplat_sh_rotation", "msplat_transform_cloud"):
        assert hasattr(L, name), "libmsplat.so does not export %s" % name
        assert name in names, "no ctypes prototype for %s" % name
    assert _capi.TRANSFORM_KEEP_SH == tr.KEEP_SH == 1
    assert callable(getattr(SplatRenderer, "TransformCloud", None)), "SplatRenderer has no TransformCloud"


def test_refusals_that_need_no_device():
    L = _capi.lib()
    m = np.ascontiguousarray(MATS["rigid"])
    assert L.msplat_transform_cloud(None, m.ctypes.data_as(C.POINTER(C.c_float)), None, 0, 0) == _capi.ERR_INVALID_ARG
    assert "ctx is NULL" in L.msplat_last_error(None).decode()
    rc, D, s = th.sh_rotation(MATS["affine"])
    assert rc == _capi.ERR_UNSUPPORTED
    assert all(np.isnan(d).all() for d in D.values()) and np.isnan(s), "the outputs of a refused call were written"
    mirror = MATS["identity"].copy()
    mirror[0] = -1.0                                             # det < 0: an improper rotation
    assert th.sh_rotation(mirror)[0] == _capi.ERR_UNSUPPORTED
    for k in (0, 6, 13):                                         # rows 0-2; the translation is checked too
        bad = MATS["rigid"].copy()
        bad[k] = np.nan
        rc, D, _ = th.sh_rotation(bad)
        assert rc == _capi.ERR_INVALID_ARG and np.isnan(D[1]).all(), k
    row3 = MATS["rigid"].copy()
    row3[[3, 7, 11, 15]] = np.nan                                # row 3 is not read
    assert th.sh_rotation(row3)[0] == _capi.OK
    assert L.msplat_sh_rotation(None, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert th.sh_rotation(MATS["rigid"], scale=False)[0] == _capi.OK      # scale_out may be NULL


def test_the_gate_takes_the_similarities_and_refuses_the_affine_matrix():
    for name in tr.SIMILARITIES:
        ok, s, Q = tr.gate(MATS[name])
        assert ok and abs(s - tr.SCALES[name]) <= 1e-6 * s, (name, s)
        assert np.abs(Q.T @ Q - np.eye(3)).max() < 1e-6, name   # an fp32 rotation: far inside the gate's 1e-4
    ok, _, _ = tr.gate(MATS["affine"])
    assert not ok
    shear = np.eye(4)
    shear[0, 1] = 0.01                                           # a 1 % shear has 1e-2 there
    assert not tr.gate(np.ascontiguousarray(shear.T.reshape(16), np.float32))[0]


@pytest.mark.parametrize("name", tr.SIMILARITIES)
def test_sh_rotation_equals_the_reference_fit(name):
    M = MATS[name]
    rc, D, s = th.sh_rotation(M)
    assert rc == _capi.OK
    _, s_ref, _ = tr.gate(M)
    assert abs(s - s_ref) <= 1e-6 * s_ref and abs(s - tr.SCALES[name]) <= 1e-6 * s_ref, (s, s_ref)
    ref = tr.reference_D(M)
    for band in (1, 2, 3):
        err = np.abs(D[band].astype(np.float64) - ref[band]).max()
        print("%s band %d: max |D - D_ref| %.3g" % (name, band, err))
        assert D[band].dtype == np.float32 and err <= 1e-5, (name, band, err)
        assert np.abs(D[band]).max() <= 1.0 + 1e-6
        if name == "identity":
            np.testing.assert_array_equal(D[band], np.eye(D[band].shape[0], dtype=np.float32))


def test_a_quarter_turn_gives_exact_signed_permutations():
    _, D, s = th.sh_rotation(MATS["quarter_turn"])
    assert s == 1.0
    for band, d in D.items():
        assert set(np.unique(d)) <= {-1.0, 0.0, 1.0}, (band, d)
        assert (np.abs(d).sum(axis=0) == 1.0).all() and (np.abs(d).sum(axis=1) == 1.0).all(), (band, d)
        assert not np.array_equal(d, np.eye(d.shape[0], dtype=np.float32)), band


def _records(n, seed):
    """(n, 61) records with |sh| <= 1 and a symmetric positive covariance"""
    rng = np.random.default_rng(seed)
    aos = vr.cloud_aos(n).copy()
    for c in range(3):
        for k in range(16):
            aos[:, tr.sh_col(c, k)] = rng.uniform(-1.0, 1.0, n)
    return aos


@pytest.mark.parametrize("name", tr.SIMILARITIES)
def test_the_rule_keeps_the_colour_at_the_rotated_direction_and_moves_the_covariance(name):
    M = MATS[name]
    aos = _records(40, 3)
    out = th.rule_rows(aos, M)
    _, _, Q = tr.gate(M)
    v = tr.directions(100, 9)
    b, bq = tr.basis(v), tr.basis(v @ Q.T)                       # row k of v @ Q^T is (Q v_k)^T
    worst = 0.0
    for c in range(3):
        cols = [tr.sh_col(c, k) for k in range(16)]
        before = aos[:, cols].astype(np.float64) @ b.T           # (splat, direction)
        after = out[:, cols].astype(np.float64) @ bq.T
        worst = max(worst, np.abs(after - before).max())
        np.testing.assert_array_equal(out[:, cols[0]], aos[:, cols[0]])      # the DC term is untouched
    print("%s: max colour difference %.3g" % (name, worst))
    assert worst <= 1e-5, worst
    A = tr.upper(M, np.float64).T                                # the proper 3x3
    S = aos[:, 16:25].astype(np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)       # S[c][r] -> [r][c]
    want = A @ S @ A.T
    got = out[:, 16:25].astype(np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)
    assert np.abs(got - want).max() <= 1e-5 * (1.0 + np.abs(S).max()), np.abs(got - want).max()
    R = np.asarray(M, np.float64).reshape(4, 4).T
    np.testing.assert_allclose(out[:, 0:3], aos[:, 0:3].astype(np.float64) @ R[:3, :3].T + R[:3, 3], atol=1e-5, rtol=0)
    np.testing.assert_array_equal(out[:, 3], aos[:, 3])          # alpha is untouched
    if name == "quarter_turn":                                   # every product and sum is exact
        np.testing.assert_array_equal(got, want.astype(np.float32))


def test_select_and_keep_sh_touch_what_they_say():
    aos = _records(64, 4)
    sel = vr.mask_cases(64)["bytes_2_255"]
    M = MATS["similarity"]
    out = th.rule_rows(aos, M, sel)
    np.testing.assert_array_equal(out[sel == 0], aos[sel == 0])
    assert (out[sel != 0, 0:3] != aos[sel != 0, 0:3]).any(axis=1).all()
    np.testing.assert_array_equal(out[sel != 0], th.rule_rows(aos, M)[sel != 0])
    kept = th.rule_rows(aos, MATS["affine"], None, keep_sh=True)
    sh = [tr.sh_col(c, k) for c in range(3) for k in range(16)]
    np.testing.assert_array_equal(kept[:, sh], aos[:, sh])
    assert (kept[:, 16:25] != aos[:, 16:25]).any()
    d0 = np.ascontiguousarray(aos[:, :25])                       # an SH degree 0 record: band 1 lives in sh0.yzw and is rotated
    out0 = th.rule_rows(d0, M)
    np.testing.assert_array_equal(out0, th.rule_rows(aos, M)[:, :25])


def test_the_oracle_sees_the_moved_cloud_from_the_moved_camera_as_it_saw_the_original():
    n, W, H = 300, 64, 40
    aos = vr.cloud_aos(n, 21)
    cam, proj, vp, nf = scenes.default_view(W, H, z=7.0, yaw=0.2)
    M = MATS["rigid"]
    moved = th.rule_rows(aos, M)
    M4 = np.asarray(M, np.float64).reshape(4, 4).T
    cam2 = np.ascontiguousarray((M4 @ np.asarray(cam, np.float64).reshape(4, 4).T).T.reshape(16), np.float32)
    ref = orc.render_frame(aos, True, cam, proj, vp, nf)
    got = orc.render_frame(moved, True, cam2, proj, vp, nf)
    assert ref["V"] > 100 and got["V"] == ref["V"], (got["V"], ref["V"])
    assert (ref["image"][..., :3] > 0.01).mean() > 0.05         # the view shows the cloud
    print("max |diff| %.3g" % np.abs(got["image"] - ref["image"]).max())
    check_image(got["image"], ref["image"])


def test_the_shim_with_transform_cloud_compiles_with_gxx_and_refuses_without_a_cloud(tmp_path):
    import subprocess
    src = tmp_path / "transform_shim.cpp"
    src.write_text("""
#include "splatapult_amd/host/msplat_host.hpp"
struct Mat4 { float m[16]; };
int main()
{
    SplatRenderer r;
    const Mat4 turn = {{0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 1, 0, 0.5f, -2, 0.25f, 1}};
    float d1[9], d2[25], d3[49], s = 0;
    bool ok = !r.TransformCloud(turn) && !r.TransformCloud(turn, nullptr, true);            // no cloud (Init first)
    ok = ok && msplat_transform_cloud(nullptr, turn.m, nullptr, 0, MSPLAT_TRANSFORM_KEEP_SH) == MSPLAT_ERR_INVALID_ARG;
    ok = ok && msplat_sh_rotation(turn.m, d1, d2, d3, &s) == MSPLAT_OK && s == 1.0f;
    for (int k = 0; k < 9; ++k) ok = ok && (d1[k] == 0.0f || d1[k] == 1.0f || d1[k] == -1.0f);
    const Mat4 shear = {{1, 0, 0, 0, 0.3f, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    ok = ok && msplat_sh_rotation(shear.m, d1, d2, d3, nullptr) == MSPLAT_ERR_UNSUPPORTED;
    return ok ? 0 : 1;
}
""")
    exe, libdir = str(tmp_path / "transform_shim"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, cwd=ROOT)
    assert subprocess.run([exe], cwd=ROOT, capture_output=True, timeout=60).returncode == 0
