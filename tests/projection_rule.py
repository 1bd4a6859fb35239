"""The vertex + geometry stage of one frame (project_kernel; the oracle's project_one) and the footprint rule of include/msplat.h
 restated in numpy float32, operation by operation in the order the literal oracle performs them, so that
its records can be compared with the oracle's bit for bit.  No device, no torch, none of the project's libraries (the sRGB curve
calls the C library's powf, as the oracle does).

The footprint rule.  A splat that passed the geometry stage's guard-band, near and far tests, with fp32 cov2D = (a, b; b', c)
(the +0.3 added; b = cov2D[0][1], column 0 row 1, the record's m01), falls into one of three classes:
  G  drawable: det > 0, a > 0, c > 0 and min >= 0, min = (a + c) / 2 - sqrt(((a - c) / 2)^2 + b b), every operation rounded once;
  Q  !(min >= 0): the geometry shader takes sqrt(min), its quad is NaN, the reference draws nothing -- and so does the product;
  X  min >= 0 but !(det > 0), or a or c not positive: the reference blends exp(+q) or NaN; the product draws nothing."""
import numpy as np

F = np.float32
G, Q, X = 0, 1, 2
CLASS_NAMES = ("G", "Q", "X")
HALF_PI = F(1.57079632679489661923)


def cov2_class(cov):
    """the class per row of cov = (m00, m01, m10, m11), float32"""
    cov = np.asarray(cov, F).reshape(-1, 4)
    a, b, b2, c = cov[:, 0], cov[:, 1], cov[:, 2], cov[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        mn = minor_variance(cov)
        det = a * c - b * b2
        q = ~(mn >= 0)
        x = ~q & (~(det > 0) | ~(a > 0) | ~(c > 0))
    return np.where(q, Q, np.where(x, X, G)).astype(np.int32)


def minor_variance(cov, b_from=1):
    """min of splat_geom.glsl:59-66; b_from = 2 takes the other off-diagonal element (what the rule does NOT do: the tests use it
    to find the splats that tell the two apart)"""
    cov = np.asarray(cov, F).reshape(-1, 4)
    a, b, c = cov[:, 0], cov[:, b_from], cov[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        apco2 = (a + c) / F(2)
        amco2 = (a - c) / F(2)
        term = np.sqrt(amco2 * amco2 + b * b)
        return apco2 - term


def major_variance(cov):
    cov = np.asarray(cov, F).reshape(-1, 4)
    a, b, c = cov[:, 0], cov[:, 1], cov[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        return (a + c) / F(2) + np.sqrt(((a - c) / F(2)) * ((a - c) / F(2)) + b * b)


def _mat3_mul(a, b):
    """column-major 3x3 per row of (n, 9): out[c][r] = (a[0][r] b[c][0] + a[1][r] b[c][1]) + a[2][r] b[c][2]"""
    out = np.empty(np.broadcast_shapes(a.shape, b.shape), F)
    for c in range(3):
        for r in range(3):
            s = a[..., 0 * 3 + r] * b[..., c * 3 + 0]
            s = s + a[..., 1 * 3 + r] * b[..., c * 3 + 1]
            s = s + a[..., 2 * 3 + r] * b[..., c * 3 + 2]
            out[..., c * 3 + r] = s
    return out


def _powf(x, y):
    """the C library's powf, element by element: numpy's float32 power is another implementation and differs from it in the last
    bit for more than half of all colours, and the oracle's sRGB curve calls powf"""
    import ctypes
    import ctypes.util
    f = ctypes.CDLL(ctypes.util.find_library("m")).powf
    f.argtypes, f.restype = [ctypes.c_float, ctypes.c_float], ctypes.c_float
    return np.array([f(float(v), float(y)) for v in np.asarray(x, F).ravel()], F).reshape(np.shape(x))


def _sh_basis(v, full):
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    k1 = F(0.4886025119029199)
    b = [np.full_like(x, F(0.28209479177387814)), -k1 * y, k1 * z, -k1 * x]
    if full:
        x2, y2, z2 = x * x, y * y, z * z
        k2, k3, k4 = F(1.0925484305920792), F(0.31539156525252005), F(0.5462742152960396)
        k5, k6, k7 = F(0.5900435899266435), F(2.8906114426405543), F(0.4570457994644658)
        k8, k9 = F(0.37317633259011546), F(1.4453057213202771)
        b += [k2 * y * x, -k2 * y * z, k3 * (F(3) * z2 - F(1)), -k2 * x * z, k4 * (x2 - y2),
              -k5 * y * (F(3) * x2 - y2), k6 * y * x * z, -k7 * y * (F(5) * z2 - F(1)), k8 * z * (F(5) * z2 - F(3)),
              -k7 * x * (F(5) * z2 - F(1)), k9 * z * (x2 - y2), -k5 * x * (x2 - F(3) * y2)]
    return b


def project(aos, idx, full_sh, srgb, viewMat, projMat, viewport, nearFar, eye, lowpass_first=False):
    """dict of per-splat float32 arrays in idx order: px, py, cov (n, 4), inv (n, 4), rgb (n, 3), alpha, ndc (n, 3), depth,
    reject (bool), cls (G / Q / X of the covariance, whatever the guard tests say).
    lowpass_first: the diagonal of cov2D as Mesa 23.2's llvmpipe evaluates the shaders, ((p0 + 0.3) + p1) + p2 for the three products
    of V_prime's element instead of the source's ((p0 + p1) + p2) + 0.3 -- its compiler moves the constant of `cov2D[i][i] += 0.3f`
    to the front of the sum, which GLSL allows.  With it the geometry shader's inverse covariance, captured with transform feedback,
    is the rule's bit for bit for all 4087 + 3739 splats of the two reference-shader ladders (without: 3214 + 2051).  Only
    tests/test_reference_shaders.py asks for it; the oracle and the kernel evaluate the source's order"""
    rec = np.asarray(aos, F)[np.asarray(idx)]
    n = rec.shape[0]
    vm, pm = np.asarray(viewMat, F).reshape(16), np.asarray(projMat, F).reshape(16)
    vp, nf, eye = np.asarray(viewport, F), np.asarray(nearFar, F), np.asarray(eye, F)
    M = lambda m, c, r: m[c * 4 + r]
    with np.errstate(all="ignore"):
        x, y, z = rec[:, 0], rec[:, 1], rec[:, 2]
        t = []
        for r in range(4):
            s = M(vm, 0, r) * x
            s = s + M(vm, 1, r) * y
            s = s + M(vm, 2, r) * z
            s = s + M(vm, 3, r)
            t.append(s.astype(F))
        X0 = vp[0] * (F(0.00001) * nf[0])
        Y0, WIDTH, HEIGHT = vp[1], vp[2], vp[3]
        SX, SY, WZ = M(pm, 0, 0), M(pm, 1, 1), M(pm, 3, 2)
        tzSq = t[2] * t[2]
        jsx = -(SX * WIDTH) / (F(2) * t[2])
        jsy = -(SY * HEIGHT) / (F(2) * t[2])
        jtx = (SX * t[0] * WIDTH) / (F(2) * tzSq)
        jty = (SY * t[1] * HEIGHT) / (F(2) * tzSq)
        jtz = ((nf[1] - nf[0]) * WZ) / (F(2) * tzSq)
        zero = np.zeros(n, F)
        J = np.stack([jsx, zero, zero, zero, jsy, zero, jtx, jty, jtz], axis=1).astype(F)
        W = np.array([M(vm, 0, 0), M(vm, 0, 1), M(vm, 0, 2), M(vm, 1, 0), M(vm, 1, 1), M(vm, 1, 2),
                      M(vm, 2, 0), M(vm, 2, 1), M(vm, 2, 2)], F)[None, :]
        V = rec[:, 16:25]
        JW = _mat3_mul(J, np.broadcast_to(W, (n, 9)))
        JWt = JW.reshape(n, 3, 3).transpose(0, 2, 1).reshape(n, 9)
        A = _mat3_mul(JW, V)
        Vp = _mat3_mul(A, JWt)
        m00, m01, m10, m11 = Vp[:, 0] + F(0.3), Vp[:, 1], Vp[:, 3], Vp[:, 4] + F(0.3)
        if lowpass_first:
            m00 = ((A[:, 0] * JWt[:, 0] + F(0.3)) + A[:, 3] * JWt[:, 1]) + A[:, 6] * JWt[:, 2]
            m11 = ((A[:, 1] * JWt[:, 3] + F(0.3)) + A[:, 4] * JWt[:, 4]) + A[:, 7] * JWt[:, 5]
        cov = np.stack([m00, m01, m10, m11], axis=1)
        p4 = []
        for r in range(4):
            s = M(pm, 0, r) * t[0]
            s = s + M(pm, 1, r) * t[1]
            s = s + M(pm, 2, r) * t[2]
            s = s + M(pm, 3, r) * t[3]
            p4.append(s.astype(F))
        ndc = np.stack([p4[0] / p4[3], p4[1] / p4[3], p4[2] / p4[3]], axis=1)
        px = F(0.5) * (WIDTH + (ndc[:, 0] * WIDTH) + (F(2) * X0))
        py = F(0.5) * (HEIGHT + (ndc[:, 1] * HEIGHT) + (F(2) * Y0))
        d = [x - eye[0], y - eye[1], z - eye[2]]
        ln = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        b = _sh_basis(np.stack([d[0] / ln, d[1] / ln, d[2] / ln], axis=1), full_sh)
        rgb = np.empty((n, 3), F)
        for ch in range(3):
            s = b[0] * rec[:, 4 + 4 * ch]
            for k in range(1, 4):
                s = s + b[k] * rec[:, 4 + 4 * ch + k]
            if full_sh:
                for k in range(4, 16):
                    s = s + b[k] * rec[:, 25 + 12 * ch + (k - 4)]
            rgb[:, ch] = F(0.5) + s
        if srgb:
            rgb = np.where(rgb <= F(0.04045), rgb / F(12.92), _powf((rgb + F(0.055)) / F(1.055), F(2.4))).astype(F)
        det = m00 * m11 - m01 * m10
        inv = np.stack([m11 / det, -m01 / det, -m10 / det, m00 / det], axis=1).astype(F)
        cls = cov2_class(cov)
        guard = (ndc[:, 2] < F(0.25)) | (ndc[:, 0] > F(2)) | (ndc[:, 0] < F(-2)) | (ndc[:, 1] > F(2)) | (ndc[:, 1] < F(-2)) \
            | ~(ndc[:, 2] <= F(1)) | ~(p4[3] > F(0))
    for a in (px, py, cov, inv, rgb, ndc):
        assert a.dtype == F, a.dtype
    return dict(px=px, py=py, cov=cov, inv=inv, rgb=rgb, alpha=rec[:, 3].copy(), ndc=ndc, depth=p4[3], guard=guard,
                reject=guard | (cls != G), cls=cls)


def compare_with_oracle(rule, sp):
    """names of the record fields whose bits differ from the oracle's orc_splat2d array `sp` (NaN payloads and the sign of a NaN
    are not compared: a NaN equals a NaN)"""
    bad = []
    for name in ("px", "py", "cov", "inv", "rgb", "alpha", "ndc", "depth"):
        a, b = np.ascontiguousarray(rule[name], F), np.ascontiguousarray(sp[name], F)
        same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        if not same.all():
            bad.append("%s (%d)" % (name, int((~same).sum())))
    if not np.array_equal(rule["reject"], sp["reject"] != 0):
        bad.append("reject (%d)" % int((rule["reject"] != (sp["reject"] != 0)).sum()))
    return bad
