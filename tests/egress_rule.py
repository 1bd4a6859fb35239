"""What the tests of the device downloads and msplat_export_ply share (numpy only; no device, no torch): the per-splat rule of
include/msplat.h restated -- GaussianCloud::ExportPly of a decoded record, float64 Jacobi and fp32 everywhere else --, the raw reader of
the fixed 62 / 17-float PLY, the covariance bound (the independent check: it shares no formula with the kernel) and the hostile
families the rule and the kernel are run on."""
import ctypes as C
import functools

import numpy as np

from splatapult_amd import synthetic
from tests import scenes
from tests.render_cases import _covariance_by_rodrigues

F32 = np.float32
N_FAMILY = 3000
ATTR_FAMILIES = ("generate", "scene", "needles", "isotropic", "two_equal", "identity")
FAMILIES = ATTR_FAMILIES + ("hand",)
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "log_scale", "rot")


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def jacobi_eigen3(cov9):
    """JacobiEigen3 (splatapult_amd/host/gaussian_scene.cpp) on (N, 9) column-major fp32 covariances, float64 throughout, one lane per
    row: -> (eval (N, 3), evec (N, 3, 3) with evec[:, k, r] = component r of eigenvector k), both rounded once to fp32"""
    V = np.asarray(cov9, F32).astype(np.float64).reshape(-1, 3, 3)             # V[:, c, r]
    n = V.shape[0]
    a = [[0.5 * (V[:, c, r] + V[:, r, c]) for c in range(3)] for r in range(3)]      # a[r][c]
    v = [[np.full(n, 1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    running = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(32):
            off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2]
            running &= ~(off < 1e-30)
            if not running.any():
                break
            for p, q in ((0, 1), (0, 2), (1, 2)):
                do = running & ~(np.abs(a[p][q]) < 1e-300)
                theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q])
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for k in range(3):
                    akp, akq = a[k][p], a[k][q]
                    a[k][p], a[k][q] = np.where(do, c * akp - s * akq, akp), np.where(do, s * akp + c * akq, akq)
                for k in range(3):
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k], a[q][k] = np.where(do, c * apk - s * aqk, apk), np.where(do, s * apk + c * aqk, aqk)
                for k in range(3):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p], v[k][q] = np.where(do, c * vkp - s * vkq, vkp), np.where(do, s * vkp + c * vkq, vkq)
    d = np.stack([a[0][0], a[1][1], a[2][2]], axis=1)
    order = np.argsort(d, axis=1, kind="stable")                               # ascending, ties in index order
    vm = np.stack([np.stack(row, axis=1) for row in v], axis=1)                # vm[:, r, c]
    ev = np.take_along_axis(d, order, axis=1).astype(F32)
    evec = np.stack([np.take_along_axis(vm[:, r, :], order, axis=1) for r in range(3)], axis=2).astype(F32)      # [:, k, r]
    return ev, evec


def quat_from_mat3(R):
    """QuatFromMat3 on (N, 9) column-major fp32 matrices, fp32 operation for operation -> (N, 4) as w x y z"""
    R = np.asarray(R, F32).reshape(-1, 9)
    m = lambda c, r: R[:, c * 3 + r]
    one, two, quarter = F32(1.0), F32(2.0), F32(0.25)
    m00, m11, m22 = R[:, 0], R[:, 4], R[:, 8]
    with np.errstate(all="ignore"):
        tr = m00 + m11 + m22
        s0 = np.sqrt(tr + one) * two
        s1 = np.sqrt(one + m00 - m11 - m22) * two
        s2 = np.sqrt(one + m11 - m00 - m22) * two
        s3 = np.sqrt(one + m22 - m00 - m11) * two
        b0 = [quarter * s0, (m(1, 2) - m(2, 1)) / s0, (m(2, 0) - m(0, 2)) / s0, (m(0, 1) - m(1, 0)) / s0]
        b1 = [(m(1, 2) - m(2, 1)) / s1, quarter * s1, (m(1, 0) + m(0, 1)) / s1, (m(2, 0) + m(0, 2)) / s1]
        b2 = [(m(2, 0) - m(0, 2)) / s2, (m(1, 0) + m(0, 1)) / s2, quarter * s2, (m(2, 1) + m(1, 2)) / s2]
        b3 = [(m(0, 1) - m(1, 0)) / s3, (m(2, 0) + m(0, 2)) / s3, (m(2, 1) + m(1, 2)) / s3, quarter * s3]
        c0, c1, c2 = tr > 0, (m00 > m11) & (m00 > m22), m11 > m22
        w, x, y, z = [np.where(c0, b0[k], np.where(c1, b1[k], np.where(c2, b2[k], b3[k]))).astype(F32) for k in range(4)]
        nrm = np.sqrt(w * w + x * x + y * y + z * z)
        return np.stack([w / nrm, x / nrm, y / nrm, z / nrm], axis=1).astype(F32)


def export_rule(rec):
    """the rule on (N, 25 | 61) fp32 records (what msplat_download_cloud returns) -> the six attribute arrays; f_rest is (N, 45)
    in PLY order, zeros for 25-float records"""
    rec = np.ascontiguousarray(rec, F32)
    n, full = rec.shape[0], rec.shape[1] == 61
    out = dict(xyz=rec[:, 0:3].copy(), f_dc=rec[:, [4, 8, 12]].copy(), f_rest=np.zeros((n, 45), F32))
    if full:
        for c in range(3):
            out["f_rest"][:, 15 * c:15 * c + 3] = rec[:, 5 + 4 * c:8 + 4 * c]
            out["f_rest"][:, 15 * c + 3:15 * c + 15] = rec[:, 25 + 12 * c:37 + 12 * c]
    with np.errstate(all="ignore"):
        out["opacity"] = (-np.log((F32(1.0) / rec[:, 3]) - F32(1.0))).astype(F32)
        ev, evec = jacobi_eigen3(rec[:, 16:25])
        e = evec.reshape(n, 9)
        det = (e[:, 0] * (e[:, 4] * e[:, 8] - e[:, 5] * e[:, 7]) - e[:, 3] * (e[:, 1] * e[:, 8] - e[:, 2] * e[:, 7])
               + e[:, 6] * (e[:, 1] * e[:, 5] - e[:, 2] * e[:, 4]))
        e = np.where((det < 0)[:, None], -e, e)
        out["rot"] = quat_from_mat3(e)
        out["log_scale"] = np.log(np.sqrt(np.where(ev < 0, F32(0.0), ev))).astype(F32)
    return out


def vertex_block(attrs, full):
    """the attributes as GaussianCloud::ExportPly's vertices: (N, 62) floats, (N, 17) without f_rest; nx ny nz are zeros"""
    n = attrs["xyz"].shape[0]
    cols = [attrs["xyz"], np.zeros((n, 3), F32), attrs["f_dc"]] + ([attrs["f_rest"]] if full else [])
    cols += [np.asarray(attrs["opacity"]).reshape(n, 1), attrs["log_scale"], attrs["rot"]]
    return np.ascontiguousarray(np.concatenate(cols, axis=1), "<f4")


def block_attrs(block):
    """the inverse of vertex_block"""
    b, full = np.asarray(block, F32), block.shape[1] == 62
    k = 54 if full else 9
    return dict(xyz=b[:, 0:3], f_dc=b[:, 6:9], f_rest=b[:, 9:54] if full else np.zeros((b.shape[0], 45), F32), opacity=b[:, k],
                log_scale=b[:, k + 1:k + 4], rot=b[:, k + 4:k + 8])


def ply_names(full):
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + (["f_rest_%d" % i for i in range(45)] if full else [])
    return names + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]


def read_ply(path):
    """(header bytes, (N, 62 | 17) fp32 vertex block) of a PLY with ExportPly's fixed float properties"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    n = int(lines[2].split()[-1])
    props = [l.split() for l in lines[3:] if l.startswith("property")]
    assert all(p[1] == "float" for p in props) and [p[2] for p in props] == ply_names(len(props) == 62), props
    assert len(raw) - end == n * len(props) * 4, (len(raw) - end, n, len(props))
    return raw[:end], np.frombuffer(raw, "<f4", n * len(props), end).reshape(n, len(props))


# ---- the covariance bound ---------------------------------------------------------------------------------------------------
def covariance_error(rot, log_scale, cov9):
    """per splat (err, bound, zero): err = max |Sigma' - Sigma|, Sigma' rebuilt in float64 from the exported fp32 rot and log_scale by
    Rodrigues' formula, Sigma the symmetrised (N, 9) covariance of the record; bound = (3 spacing(float32(L)) + 2^-21) max |Sigma| with
    L the largest finite |log_scale_k|: 1/2 ulp for the rule's rounding of log s plus 1 ulp for the device's logf is 1.5 ulp in log s,
    3 ulp relative in s^2; 2^-21 for the fp32 quaternion and eigenvalues.  zero: the rows with max |Sigma| == 0"""
    rot, ls = np.asarray(rot, F32), np.asarray(log_scale, F32)
    S = np.asarray(cov9, F32).astype(np.float64).reshape(-1, 3, 3)
    S = 0.5 * (S + S.transpose(0, 2, 1))
    top = np.abs(S).max(axis=(1, 2))
    zero = top == 0
    with np.errstate(all="ignore"):
        rebuilt = _covariance_by_rodrigues(np.where(zero[:, None], F32(1.0), rot), ls)
        err = np.abs(rebuilt - S).max(axis=(1, 2))
    L = np.where(np.isfinite(ls), np.abs(ls), F32(0.0)).max(axis=1).astype(F32)
    bound = (3.0 * np.spacing(L).astype(np.float64) + 2.0 ** -21) * top
    return err, bound, zero


def check_covariance(attrs, rec, what, extra=0.0):
    """the bound on every splat of attrs (exported values) against the records rec; extra: a further share of max |Sigma| the caller
    accounts for (a second ingest).  Returns the worst err / max |Sigma|"""
    err, bound, zero = covariance_error(attrs["rot"], attrs["log_scale"], rec[:, 16:25])
    top = np.abs(np.asarray(rec[:, 16:25], np.float64)).max(axis=1)
    ok = err[~zero] <= bound[~zero] + extra * top[~zero]
    worst = float((err[~zero] / top[~zero]).max()) if (~zero).any() else 0.0
    assert ok.all(), "%s: %d splats beyond the covariance bound, worst %.3g of the largest entry (row %d)" % (
        what, int((~ok).sum()), worst, int(np.flatnonzero(~zero)[np.argmin(ok)]))
    z = np.flatnonzero(zero)
    assert (np.asarray(attrs["rot"])[z] == np.array([1, 0, 0, 0], F32)).all(), "%s: a zero covariance must export rot = (1, 0, 0, 0)" % what
    assert (np.asarray(attrs["log_scale"])[z] == -np.inf).all(), "%s: a zero covariance must export scale = -inf" % what
    return worst


def close_to_rule(got, want, what):
    """the bounds of the issue between two evaluations of the rule (the device's, glibc's, numpy's): copies equal as uint32, rot
    within 2^-22 per component, opacity and scale rtol 1e-6 with equal infinities"""
    for k in ("xyz", "f_dc", "f_rest"):
        if got.get(k) is not None:
            a, b = np.ascontiguousarray(got[k], F32).view(np.uint32), np.ascontiguousarray(want[k], F32).view(np.uint32)
            assert a.shape == b.shape and (a == b).all(), "%s: %s is not a bit-for-bit copy" % (what, k)
    d = np.abs(np.asarray(got["rot"], np.float64) - np.asarray(want["rot"], np.float64))
    assert (d <= 2.0 ** -22).all(), "%s: rot differs by %.3g (row %d)" % (what, d.max(), int(d.max(axis=1).argmax()))
    for k in ("opacity", "log_scale"):
        a, b = np.asarray(got[k], F32).reshape(np.asarray(want[k]).shape), np.asarray(want[k], F32)
        inf = np.isinf(b)
        assert (np.isinf(a) == inf).all() and (a[inf] == b[inf]).all(), "%s: %s has other infinities" % (what, k)
        np.testing.assert_allclose(a[~inf], b[~inf], rtol=1e-6, atol=0, err_msg="%s: %s" % (what, k))


# ---- the hostile families ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_attrs(name, n=N_FAMILY):
    """attributes (read-only) of an attribute family: colours and positions of one synthetic cloud, scales and rotations per family"""
    assert name in ATTR_FAMILIES, name
    if name == "generate":
        a = synthetic.generate(n, seed=0xE6E55, log_scale_mean=-3.0)
    elif name == "scene":
        a = synthetic.generate_scene(n, seed=0x5CE11E)
    else:
        a = synthetic.generate(n, seed=0xE6E56, log_scale_mean=-3.0)
        rng = np.random.default_rng(["needles", "isotropic", "two_equal", "identity"].index(name) + 2800)
        q = rng.standard_normal((n, 4))
        a["rot"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)
        if name == "needles":
            a["log_scale"] = rng.uniform(-9.0, 0.5, (n, 3)).astype(F32)
        elif name == "isotropic":
            a["log_scale"] = np.repeat(rng.uniform(-6.0, 0.0, (n, 1)), 3, axis=1).astype(F32)
        else:
            a["log_scale"] = rng.uniform(-6.0, 0.0, (n, 3)).astype(F32)
        if name == "two_equal":
            k = np.arange(n) % 3                                            # which axis repeats its neighbour
            a["log_scale"][np.arange(n), k] = a["log_scale"][np.arange(n), (k + 1) % 3]
        if name == "identity":
            a["rot"][:] = (1.0, 0.0, 0.0, 0.0)
    for v in a.values():
        v.setflags(write=False)
    return a


def hand_records():
    """five hand-written records (61 floats): a zero covariance, exactly 0.005 I (the debug cloud's), alpha 0, alpha 1, and a
    covariance that is not symmetric, as MSPLAT_TRANSFORM_KEEP_SH with a shear leaves one"""
    rec = scenes.cloud_from_attrs({k: np.array(v[:5]) for k, v in family_attrs("generate").items()}, True).as_array().copy()
    rec[0, 16:25] = 0.0
    rec[1, 16:25] = 0.0
    rec[1, [16, 20, 24]] = F32(0.005)
    rec[2, 3], rec[3, 3] = 0.0, 1.0
    S = rec[4, 16:25].reshape(3, 3).T.copy()                                  # S[r, c], fp32
    A = np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.25], [0.0, 0.0, 1.0]], F32)
    S2 = ((A @ S).astype(F32) @ A.T).astype(F32)
    S2[0, 1] = S2[1, 0] * F32(1.0 + 2.0 ** -12)                               # certainly not symmetric
    assert S2[0, 1] != S2[1, 0]
    rec[4, 16:25] = S2.T.reshape(9)
    return rec


@functools.lru_cache(maxsize=None)
def family_records(name):
    """(N, 61) fp32 records (read-only) of a family: GaussianCloud.FromAttributes of its attributes, or the hand-written rows"""
    rec = hand_records() if name == "hand" else scenes.cloud_from_attrs({k: np.array(v) for k, v in family_attrs(name).items()}, True).as_array()
    rec.setflags(write=False)
    return rec


def host_cloud(rec):
    """a GaussianCloud (full SH) that holds exactly these records: made of as many rows, then overwritten in place"""
    n = rec.shape[0]
    a = synthetic.generate(max(n, 1), seed=1)
    gc = scenes.cloud_from_attrs({k: v[:n] for k, v in a.items()}, True)
    assert gc.GetNumGaussians() == n and gc.GetStride() == 244
    if n:
        C.memmove(gc.GetRawDataPtr(), np.ascontiguousarray(rec, F32).ctypes.data, n * 244)
    return gc
