"""What the id-frame tests share (numpy and the oracle only; no device, no torch): the definition of msplat_render_ids in float64 over
the oracle's projected splats, the two cases, and which pixels of them are DECIDED -- the pixels on which the library must name the
reference's splat.

Per pixel centre p, over the drawn splats near to far: w_i = alpha_i exp(-q_i / 2), 0 where w_i <= 1/256 (splat_frag.glsl:18-42);
T_i = prod_{j in front of i}(1 - w_j); c_i = T_i w_i.  id = the splat with the largest c_i, the nearest of equals (strict `>`), NONE
where no splat has w > 0.  `second` is the largest contribution of any OTHER splat, `near` says that some fragment at the pixel has
|w - 1/256| <= FLIP_REL / 256 (the oracle's flip_rel: the fp32 weight may land on the other side of the discard).

A pixel is decided when best - second > 2 TOL and it is not near: TOL = 1e-4 is the per-value bound of tests/checks.py (the
accuracy the colour frame is held to), each of the two contributions may be off by it, and a fragment on the discard threshold may
land on either side and shift every contribution behind it.  Nothing here is measured on a device."""
import functools

import numpy as np

from oracle import oracle as orc
from tests import render_cases

NONE = 0xFFFFFFFF              # MSPLAT_ID_NONE
TOL = 1e-4                     # tests/checks.py: the per-value bound of the colour frame
FLIP_REL = 1e-4                # oracle.composite_flip's flip_rel
CASES = ("hand_placed", "sparse")


def case(name):
    """(aos, full_sh, W, H, view)"""
    if name == "hand_placed":
        aos, W, H, view = render_cases.hand_placed()
        return aos, False, W, H, view
    cloud, W, H, view = render_cases.view_of(name)
    return cloud.as_array(), True, W, H, view


def definition_f64(splats, W, H):
    """The definition over orc.project'ed splats in draw order (far -> near; walked reversed), each restricted to the bounding
    rectangle of its footprint (outside it w < (1 - 2 FLIP_REL) / 256: neither a fragment nor near the threshold).  Returns
    dict(id = splats["index"] of the winner or NONE, rank = its position in `splats` or -1, best, second, near), (H, W) each."""
    ids = np.full((H, W), NONE, np.uint32)
    rank = np.full((H, W), -1, np.int64)
    best, second, T = np.zeros((H, W)), np.zeros((H, W)), np.ones((H, W))
    near = np.zeros((H, W), bool)
    thr = 1.0 / 256.0
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
        box = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        dx, dy = np.meshgrid(np.arange(x0, x1 + 1) + 0.5 - cx, np.arange(y0, y1 + 1) + 0.5 - cy)
        inv = s["inv"].astype(np.float64)
        q = dx * (inv[0] * dx + inv[2] * dy) + dy * (inv[1] * dx + inv[3] * dy)
        w = alpha * np.exp(-0.5 * q)
        near[box] |= np.abs(w - thr) <= FLIP_REL * thr
        w[w <= thr] = 0.0
        c = T[box] * w
        better = c > best[box]                                   # strict: the nearest of equal contributions stays
        second[box] = np.where(better, best[box], np.maximum(second[box], c))
        best[box] = np.where(better, c, best[box])
        ids[box] = np.where(better, s["index"], ids[box])
        rank[box] = np.where(better, k, rank[box])
        T[box] *= 1.0 - w
    return dict(id=ids, rank=rank, best=best, second=second, near=near)


def decided(ref):
    """best - second > 2 TOL and not near.  A pixel without any fragment (best == 0) that is not near is decided too: its answer
    is NONE whatever the rounding (the figures the cases are held to count it so: 40 % of hand_placed shows no splat)"""
    return ((ref["best"] - ref["second"] > 2.0 * TOL) | (ref["best"] == 0.0)) & ~ref["near"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the definition of a case, computed once and read-only: definition_f64's planes plus decided, zw (the winner's window depth,
    1.0 at NONE), splats (the oracle's, draw order), sorted_idx, V.  Ids are upload indices: the oracle is fed the cloud in upload
    order (both clouds are stored in that order: they are smaller than the Morton threshold)"""
    aos, full_sh, W, H, (cam, proj, vp, nf) = case(name)
    fr = orc.render_frame(aos, full_sh, cam, proj, vp, nf, nthreads=8, want_image=False, want_splats=True)
    splats = fr["splats"]
    ref = definition_f64(splats, W, H)
    ref["decided"] = decided(ref)
    zw = render_cases.window_depth(splats)
    ref["zw"] = np.where(ref["rank"] >= 0, zw[np.maximum(ref["rank"], 0)], np.float32(1.0)).astype(np.float32)
    ref.update(splats=splats, sorted_idx=fr["sorted_idx"], V=fr["V"])
    return render_cases.read_only(ref)


def windows(W, H):
    """the windows of the window test: 1 x 1 at the four corners and at a bin corner, a rectangle that straddles tile and bin edges,
    one tile exactly, the whole viewport"""
    return [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (31, 31, 1, 1), (32, 32, 1, 1),
            (13, 27, 40, 9), (16, 32, 16, 16), (0, 0, W, H)]


def crop(plane, window):
    x0, y0, w, h = window
    return plane[y0:y0 + h, x0:x0 + w]


def mark_reference(ids, mask, value, region=None):
    """what msplat_mark_ids leaves in `mask` (a copy is returned): mask[id] = value for the ids of the pixels `region` selects
    (nonzero; None: all) that are splats of the cloud"""
    out = mask.copy()
    sel = ids if region is None else ids[region != 0]
    hit = np.unique(sel)
    out[hit[hit < mask.shape[0]]] = value
    return out
