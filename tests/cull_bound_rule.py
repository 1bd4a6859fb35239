"""The rule the conservative culls rest on, in numpy and float64, written from DESIGN.md section 2 (the projection's arithmetic
contract) and the comments above cull_key -- it shares no code with the kernels.

A splat's footprint is the ellipse w > 1/256 of w = alpha exp(-q / 2), q the quadratic form of cov^-1 with
cov = M Sigma M^T + 0.3 I, M = J mat3(view); it lies within ex = rho sqrt(cov_xx), ey = rho sqrt(cov_yy) of its centre, with
rho^2 = 2 ln(256 alpha).  The culls replace that by
    e^2 <= |J_row|^2 * view_scale2 * rho^2 lambda_max(Sigma) + 3.4,     |J_row|^2 = js^2 (1 + tr^2),
js = proj[axis][axis] * size / (2 tz), tr = t[axis] / tz, 3.4 >= 0.3 rho^2 for alpha <= 1, and then widen e to 1.002 e + 1.5 px
(per splat).  That holds when view_scale2 >= sigma_max(mat3(view))^2: |J_row W|^2 <= |J_row|^2 sigma_max(W)^2.

Matrices are float[16], column-major; aos is the cloud's record array (x y z alpha, ..., Sigma's columns in floats 16-24)."""
import numpy as np


def _rows(m):
    return np.asarray(m, np.float64).reshape(4, 4).T


def spectral2(view):
    """sigma_max(mat3(view))^2"""
    return float(np.linalg.norm(_rows(view)[:3, :3], 2) ** 2)


def _sigma(aos):
    rec = np.asarray(aos, np.float64)
    S = np.empty((rec.shape[0], 3, 3))
    S[:, :, 0], S[:, :, 1], S[:, :, 2] = rec[:, 16:19], rec[:, 19:22], rec[:, 22:25]
    return S


def _rho2(aos):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 * np.log(256.0 * np.asarray(aos[:, 3], np.float64))


def _eye_space(aos, view):
    xyz1 = np.concatenate([np.asarray(aos[:, :3], np.float64), np.ones((aos.shape[0], 1))], axis=1)
    return xyz1 @ _rows(view).T


def true_extents(aos, view, proj, viewport, near=0.1):
    """(centre (n, 2), ex, ey, drawable) per splat: the footprint's half-extents in pixels as the projection defines them, and
    whether the splat can be drawn at all -- in front of the camera, inside the 1.5 cull band, alpha > 1/256, det(cov) > 0"""
    V, P = _rows(view), _rows(proj)
    Wd, Hd = float(viewport[2]), float(viewport[3])
    t = _eye_space(aos, view)
    clip = t @ P.T
    with np.errstate(divide="ignore", invalid="ignore"):
        ndc = clip[:, :3] / clip[:, 3:4]
        tz = t[:, 2]
        J = np.zeros((aos.shape[0], 2, 3))
        J[:, 0, 0] = -(P[0, 0] * Wd) / (2.0 * tz)
        J[:, 0, 2] = (P[0, 0] * t[:, 0] * Wd) / (2.0 * tz * tz)
        J[:, 1, 1] = -(P[1, 1] * Hd) / (2.0 * tz)
        J[:, 1, 2] = (P[1, 1] * t[:, 1] * Hd) / (2.0 * tz * tz)
        M = J @ V[:3, :3]
        cov = M @ _sigma(aos) @ np.transpose(M, (0, 2, 1))
        a, c, b01, b10 = cov[:, 0, 0] + 0.3, cov[:, 1, 1] + 0.3, cov[:, 1, 0], cov[:, 0, 1]
        det = a * c - b01 * b10
        rho2 = _rho2(aos)
        ex, ey = np.sqrt(np.maximum(rho2, 0.0) * a), np.sqrt(np.maximum(rho2, 0.0) * c)
        centre = np.stack([0.5 * (Wd + ndc[:, 0] * Wd) + float(viewport[0]) * (0.00001 * near),
                           0.5 * (Hd + ndc[:, 1] * Hd) + float(viewport[1])], axis=1)
        drawable = (clip[:, 3] > 0) & (np.abs(ndc[:, 0]) < 1.5) & (np.abs(ndc[:, 1]) < 1.5) & (rho2 > 0) & (det > 0)
    return centre, ex, ey, drawable


def splat_bound(aos, view, proj, viewport, view_scale2):
    """(ex, ey) per splat as the per-splat culls bound them, with the inflations the formula itself writes: 3.4 for the
    low-pass term, 1.002 e + 1.5 px"""
    P = _rows(proj)
    t = _eye_space(aos, view)
    S = _sigma(aos)
    lmax = np.linalg.eigvalsh(0.5 * (S + np.transpose(S, (0, 2, 1))))[:, -1]
    w = np.maximum(_rho2(aos), 0.0) * np.maximum(lmax, 0.0)
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, size in ((0, float(viewport[2])), (1, float(viewport[3]))):
            js = 0.5 * P[axis, axis] * size / t[:, 2]
            tr = t[:, axis] / t[:, 2]
            out.append(np.sqrt(js * js * (1.0 + tr * tr) * float(view_scale2) * w + 3.4) * 1.002 + 1.5)
    return out[0], out[1]
