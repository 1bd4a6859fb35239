"""What the tests of msplat_transform_cloud share (numpy only; no device, no library, no torch): the rule of include/msplat.h
restated in numpy float32 in the header's operation order, taking the SH matrices D as given; the SH basis of splat_vert.glsl:51-105
in float64; a reference D from a float64 least-squares fit of the defining identity b_l(Q^T v)^T = b_l(v)^T D_l over random
directions; the similarity gate; the matrices and the select cases.  Nothing here is measured."""
import functools

import numpy as np

from tests import visibility_rule as vr

F = np.float32
BANDS = {1: (1, 3), 2: (4, 5), 3: (9, 7)}        # band -> (first coefficient, size)
KEEP_SH = 1                                      # MSPLAT_TRANSFORM_KEEP_SH


def sh_col(c, k):
    """column of the 61-float record (= FP32 record float) that holds SH coefficient k (0..15) of channel c"""
    return 4 + 4 * c + k if k < 4 else 25 + 12 * c + (k - 4)


def upper(M, dtype=F):
    """A[k][r] = M[4k + r]: A[k] is column k of the upper 3x3"""
    return np.asarray(M, dtype).reshape(4, 4)[:3, :3]


# ---- the rule ----------------------------------------------------------------------------------------------------------------

def transform_rows(aos, M, D=None, select=None):
    """The rule on (n, 25) or (n, 61) float32 records: rows with select (None: all) nonzero transformed by M, the others copied.
    D: {1: (3, 3), 2: (5, 5), 3: (7, 7)} float32, what msplat_sh_rotation(M) returned; None: MSPLAT_TRANSFORM_KEEP_SH.  Every
    operation in float32, left to right; numpy does not fuse"""
    aos = np.asarray(aos)
    assert aos.dtype == F and aos.ndim == 2 and aos.shape[1] in (25, 61), (aos.dtype, aos.shape)
    M = np.asarray(M, F).reshape(16)
    A = upper(M)
    rows = np.arange(aos.shape[0]) if select is None else np.flatnonzero(np.asarray(select) != 0)
    out = aos.copy()
    src = aos[rows]
    with np.errstate(all="ignore"):
        x, y, z = src[:, 0], src[:, 1], src[:, 2]
        for r in range(3):
            out[rows, r] = ((M[r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r]
        S = lambda c, r: src[:, 16 + 3 * c + r]
        T = [[(A[0][r] * S(c, 0) + A[1][r] * S(c, 1)) + A[2][r] * S(c, 2) for r in range(3)] for c in range(3)]
        for c in range(3):
            for r in range(3):
                out[rows, 16 + 3 * c + r] = (T[0][r] * A[0][c] + T[1][r] * A[1][c]) + T[2][r] * A[2][c]
        if D is not None:
            for band, (k0, nb) in BANDS.items():
                if band > 1 and aos.shape[1] == 25:
                    continue
                Db = np.asarray(D[band])
                assert Db.dtype == F and Db.shape == (nb, nb), (band, Db.dtype, Db.shape)
                for c in range(3):
                    sh = [src[:, sh_col(c, k0 + j)] for j in range(nb)]
                    for i in range(nb):
                        s = Db[i, 0] * sh[0]
                        for j in range(1, nb):
                            s = s + Db[i, j] * sh[j]
                        out[rows, sh_col(c, k0 + i)] = s
    assert out.dtype == F
    return out


# ---- the SH basis and the reference D ----------------------------------------------------------------------------------------

def basis(v):
    """b[0..15] of splat_vert.glsl:51-105 at the directions v (n, 3), float64, its signs and order"""
    v = np.asarray(v, np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    x2, y2, z2 = x * x, y * y, z * z
    k1, k2, k3, k4 = 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
    k5, k6, k7, k8, k9 = 0.5900435899266435, 2.8906114426405543, 0.4570457994644658, 0.37317633259011546, 1.4453057213202771
    b = [np.full_like(x, 0.28209479177387814), -k1 * y, k1 * z, -k1 * x,
         k2 * y * x, -k2 * y * z, k3 * (3.0 * z2 - 1.0), -k2 * x * z, k4 * (x2 - y2),
         -k5 * y * (3.0 * x2 - y2), k6 * y * x * z, -k7 * y * (5.0 * z2 - 1.0), k8 * z * (5.0 * z2 - 3.0), -k7 * x * (5.0 * z2 - 1.0),
         k9 * z * (x2 - y2), -k5 * x * (x2 - 3.0 * y2)]
    return np.stack(b, axis=1)


def directions(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def gate(M):
    """(is M a similarity, s, Q as a proper 3x3 matrix): s = cbrt(det A), Q = A / s, det A > 0 and max |Q^T Q - I| <= 1e-4"""
    R = upper(M, np.float64).T                   # rows of R are rows of the matrix: R[r][k] = A[k][r]
    det = np.linalg.det(R)
    if not det > 0.0:
        return False, 0.0, None
    s = np.cbrt(det)
    Q = R / s
    return bool(np.abs(Q.T @ Q - np.eye(3)).max() <= 1e-4), float(s), Q


def reference_D(M, n=256, seed=5):
    """{band: D} in float64 from the identity b_l(Q^T v)^T = b_l(v)^T D_l, least squares over n random directions"""
    ok, _, Q = gate(M)
    assert ok and n >= 200
    v = directions(n, seed)
    B, Bq = basis(v), basis(v @ Q)               # row k of v @ Q is (Q^T v_k)^T
    return {band: np.linalg.lstsq(B[:, k0:k0 + nb], Bq[:, k0:k0 + nb], rcond=None)[0] for band, (k0, nb) in BANDS.items()}


# ---- the matrices ------------------------------------------------------------------------------------------------------------

def _column_major(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return np.ascontiguousarray(m.T.reshape(16), F)


def _quaternion(w, x, y, z):
    """the rotation of a unit quaternion, rounded to float32 entry by entry (|Q^T Q - I| ~ 1e-7)"""
    q = np.array([w, x, y, z], np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]).astype(F).astype(np.float64)


@functools.lru_cache(maxsize=None)
def matrices():
    """name -> float32[16], column-major.  identity; quarter_turn: a quarter turn about z, an exact signed permutation, plus a
    power-of-two translation -- every product and sum of the rule is exact, D is a signed permutation; rigid: a quaternion rotation
    plus a translation; similarity: rigid's rotation times 0.37; affine: visibility_rule's `rotated` (a shear in it: no similarity)"""
    quarter = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R = _quaternion(0.81, 0.31, -0.42, 0.27)
    t = (0.4, -0.25, 0.6)
    out = {"identity": _column_major(np.eye(3), (0, 0, 0)), "quarter_turn": _column_major(quarter, (0.5, -2.0, 0.25)),
           "rigid": _column_major(R, t), "similarity": _column_major(R * 0.37, t), "affine": vr.matrices()["rotated"].copy()}
    for m in out.values():
        m.setflags(write=False)
    return out


def summing_rotation():
    """float32[16]: the rotation that turns band-1 coefficients (c, c, c) into (0, sqrt(3) c, 0).  With b[1..3] = k1 (-y, z, -x) the
    band is the linear form k1 g.v, g = (-sh3, -sh1, sh2); the rotation takes g = c (-1, -1, 1) to c sqrt(3) (0, 0, 1)"""
    u = np.array([-1.0, -1.0, 1.0]) / np.sqrt(3.0)
    axis = np.cross(u, (0.0, 0.0, 1.0))
    R = vr._rotation(axis, np.arccos(u[2]))
    assert np.abs(R @ u - (0.0, 0.0, 1.0)).max() < 1e-12
    return _column_major(R.astype(F).astype(np.float64), (0.0, 0.0, 0.0))


SIMILARITIES = ("identity", "quarter_turn", "rigid", "similarity")
SCALES = {"identity": 1.0, "quarter_turn": 1.0, "rigid": 1.0, "similarity": 0.37}


def select_cases(n):
    """name -> the selection (None: every splat), bool or uint8, in upload numbering: visibility_rule's mask cases"""
    return dict({"none": None}, **vr.mask_cases(n))
