"""What the score-frame tests share (numpy and the oracle only; no device, no torch): the definition of msplat_render_scores in
float64 over the oracle's projected splats, the bound a device score is held to, an fp32 restatement of the kernel's walk, the
designed case stack() and the numpy form of msplat_mark_scores.

Per pixel centre p, over the drawn splats near to far, with w_i, T_i and c_i = T_i w_i as tests/ids_rule.py defines them: per splat
S_i = sum_p c_i(p) -- what score_i / 2^23 approximates.  A fragment whose weight is within FLIP_REL of the discard threshold 1/256
("near") may land on either side of it in fp32.  That moves its own contribution by at most T / 256 and scales every contribution
behind it at that pixel by 1 - w, a relative change of at most (1/256)(1 + FLIP_REL) / (1 - (1/256)(1 + FLIP_REL)) < 1/254 each.
With m_i(p) the number of near fragments in front of i at p, the flip allowance is
    F_i = sum_p [ c_i(p) m_i(p) / 254 + near_i(p) T_i(p) / 255 ]
and with A_i the number of pixels where w_i > 0 or the fragment is near, a device score is held to
    |score_i / 2^23 - S_i| <= (TOL + 2^-24) A_i + F_i
TOL = 1e-4 is the per-value bound of tests/checks.py (the accuracy the colour frame is held to), 2^-24 the rounding of q.  Nothing
here is measured on a device."""
import functools

import numpy as np

from oracle import oracle as orc
from splatapult_amd import camera
from tests import ids_rule, render_cases
from tests.ids_rule import CASES, FLIP_REL, TOL, case      # noqa: F401  (the cases are the id frame's)

ONE = 8388608                  # MSPLAT_SCORE_ONE
STOP = 2.0 ** -24              # a pixel is finished when T <= STOP
BELOW, AT_LEAST = 0, 1         # MSPLAT_SCORE_BELOW, MSPLAT_SCORE_AT_LEAST
THR = 1.0 / 256.0


def _footprints(splats, W, H):
    """(k, box, dx, dy) of every drawn splat near to far, restricted to the bounding rectangle of its footprint as
    ids_rule.definition_f64 restricts it (outside it w < (1 - 2 FLIP_REL) / 256: neither a fragment nor near the threshold)"""
    for k in range(splats.shape[0] - 1, -1, -1):
        s = splats[k]
        alpha = float(s["alpha"])
        if s["reject"] != 0 or not alpha * 256.0 > 1.0 - 2.0 * FLIP_REL:
            continue
        rho2 = 2.0 * np.log(alpha * 256.0 / (1.0 - 2.0 * FLIP_REL))
        cx, cy = float(s["px"]), float(s["py"])
        ex, ey = np.sqrt(rho2 * float(s["cov"][0])) * 1.001 + 1.0, np.sqrt(rho2 * float(s["cov"][3])) * 1.001 + 1.0
        x0, x1 = max(int(np.floor(cx - ex)), 0), min(int(np.ceil(cx + ex)), W - 1)
        y0, y1 = max(int(np.floor(cy - ey)), 0), min(int(np.ceil(cy + ey)), H - 1)
        if x0 > x1 or y0 > y1:
            continue
        dx, dy = np.meshgrid(np.arange(x0, x1 + 1) + 0.5 - cx, np.arange(y0, y1 + 1) + 0.5 - cy)
        yield k, (slice(y0, y1 + 1), slice(x0, x1 + 1)), dx, dy


def definition_f64(splats, W, H, near_plane=None, want_tile=False):
    """The definition over orc.project'ed splats in draw order (far -> near; walked reversed).  Per splat, in the order of `splats`:
    S, A, F as above, sure = #{p : c_i(p) > 2 TOL and no fragment at p is near} (near_plane: ids_rule's `near`; None: computed
    here), peak = max_p c_i(p), and with want_tile tile = the largest sum of c_i over one 16 x 16 tile.  bound = (TOL + 2^-24) A + F."""
    n = splats.shape[0]
    if near_plane is None:
        near_plane = np.zeros((H, W), bool)
        for k, box, dx, dy in _footprints(splats, W, H):
            inv = splats[k]["inv"].astype(np.float64)
            w = float(splats[k]["alpha"]) * np.exp(-0.5 * (dx * (inv[0] * dx + inv[2] * dy) + dy * (inv[1] * dx + inv[3] * dy)))
            near_plane[box] |= np.abs(w - THR) <= FLIP_REL * THR
    S, F, tile, peak = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    A, sure = np.zeros(n, np.int64), np.zeros(n, np.int64)
    T, m = np.ones((H, W)), np.zeros((H, W))
    for k, box, dx, dy in _footprints(splats, W, H):
        inv = splats[k]["inv"].astype(np.float64)
        w = float(splats[k]["alpha"]) * np.exp(-0.5 * (dx * (inv[0] * dx + inv[2] * dy) + dy * (inv[1] * dx + inv[3] * dy)))
        near = np.abs(w - THR) <= FLIP_REL * THR
        w[w <= THR] = 0.0
        c = T[box] * w
        S[k], A[k], peak[k] = c.sum(), ((w > 0.0) | near).sum(), c.max()
        F[k] = (c * m[box] / 254.0 + near * T[box] / 255.0).sum()
        sure[k] = ((c > 2.0 * TOL) & ~near_plane[box]).sum()
        if want_tile:
            plane = np.zeros((-(-H // 16) * 16, -(-W // 16) * 16))
            plane[:H, :W][box] = c
            tile[k] = plane.reshape(plane.shape[0] // 16, 16, plane.shape[1] // 16, 16).sum(axis=(1, 3)).max()
        m[box] += near
        T[box] *= 1.0 - w
    return dict(S=S, A=A, F=F, sure=sure, tile=tile, peak=peak, bound=(TOL + 2.0 ** -24) * A + F)


def restate_f32(splats, W, H):
    """The kernel's walk restated in numpy float32: w = alpha exp(-q / 2) clamped to 1 and 0 where it is <= 1/256, c = T w,
    q = rint(c 2^23) (nearest even), T = T - c, a pixel finished at T <= 2^-24.  Returns (score uint64, pixels uint32) per splat in
    the order of `splats`."""
    f = np.float32
    n = splats.shape[0]
    score, pixels = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    T = np.ones((H, W), f)
    for k, box, dx, dy in _footprints(splats, W, H):
        dx, dy = dx.astype(f), dy.astype(f)
        inv = splats[k]["inv"].astype(f)
        quad = dx * (inv[0] * dx + inv[2] * dy) + dy * (inv[1] * dx + inv[3] * dy)
        w = np.minimum(f(splats[k]["alpha"]) * np.exp(f(-0.5) * quad), f(1.0)).astype(f)
        w[w <= f(THR)] = 0.0
        live = T[box] > f(STOP)
        c = np.where(live, T[box] * w, f(0.0)).astype(f)
        q = np.rint(c * f(ONE)).astype(np.uint64)
        score[k], pixels[k] = q.sum(), (q != 0).sum()
        T[box] = T[box] - c
    return score, pixels


@functools.lru_cache(maxsize=None)
def reference(name):
    """the definition of a case of ids_rule.CASES or of "stack", computed once and read-only: definition_f64's vectors plus splats
    (the oracle's, draw order), sorted_idx, V, n"""
    if name == "stack":
        aos, W, H, (cam, proj, vp, nf) = stack()
        fr = orc.render_frame(aos, False, cam, proj, vp, nf, nthreads=4, want_image=False, want_splats=True)
        near = None
    else:
        base = ids_rule.reference(name)
        aos, _, W, H, _ = case(name)
        fr, near = base, base["near"]
    ref = definition_f64(fr["splats"], W, H, near, want_tile=name == "stack")
    ref.update(splats=fr["splats"], sorted_idx=fr["sorted_idx"], V=fr["V"], n=aos.shape[0])
    return render_cases.read_only(ref)


def per_upload_index(ref, values, fill=0):
    """a per-splat vector of the definition (draw order) scattered to upload numbering; splats not in the Sort hold `fill`"""
    out = np.full(ref["n"], fill, np.asarray(values).dtype)
    out[ref["splats"]["index"]] = values
    return out


STACK_ALPHA = (0.9,) * 10 + (1.0, 0.9)


def stack():
    """(aos, W, H, view): twelve flat discs on the optical axis of a 48 x 48 view at twelve distinct depths, the first in front,
    each so large (sigma of more than 10^4 pixels) that its Gaussian is 1 to within 1e-6 over the whole viewport: w is its alpha,
    0.9 for the first ten, then 1.0, then 0.9.  T = 0.1^k behind the k-th: below 2^-24 behind the eighth, exactly 0 behind the
    eleventh, whose w rounds to 1.0f."""
    n = len(STACK_ALPHA)
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 2] = 1.5 - 0.25 * np.arange(n)                  # the camera sits at z = 4 and looks down -Z
    f_dc = np.linspace(-1.0, 1.0, n * 3, dtype=np.float32).reshape(n, 3)
    opacity = np.where(np.array(STACK_ALPHA) == 1.0, 30.0, np.log(9.0)).astype(np.float32)      # logits of 1 - 1e-13 and 0.9
    log_scale = np.log(np.tile(np.array([[1000.0, 1000.0, 0.01]], np.float32), (n, 1)))
    rot = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], np.float32), (n, 1))
    aos = orc.build_cloud(xyz, f_dc, None, opacity, log_scale, rot, False)
    W, H, zn, zf = 48, 48, 1.0, 8.0
    view = (camera.pose((0.0, 0.0, 4.0)), camera.perspective(camera.FOVY, W / H, zn, zf), [0, 0, W, H], [zn, zf])
    return aos, W, H, view


def mark_reference(score, op, threshold, mask, value):
    """what msplat_mark_scores leaves in `mask` (a copy is returned): mask[i] = value where score[i] < threshold (BELOW) or
    score[i] >= threshold (AT_LEAST), unsigned 64-bit"""
    assert op in (BELOW, AT_LEAST), op
    s = np.asarray(score).astype(np.uint64)
    hit = (s >= np.uint64(threshold)) == (op == AT_LEAST)
    out = mask.copy()
    out[hit] = value
    return out
