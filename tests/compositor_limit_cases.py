"""Named inputs for composite_kernel's blend at its limits (inputs and models only, numpy; tests/test_compositor_limits_fixtures.py
checks every claim made here on the CPU, tests/test_gpu_compositor_limits.py renders the cases on the GPU).

Lists are DESIGNED the way binning_limit_cases.py designs rectangles: its camera (view: the identity pose, focal length max(W, H) / 2
px), its depths (descending_depths: rank = upload index, the last splat is the nearest and the first entry the compositor walks), its
z scale of e^-16.  A splat is given in PIXELS -- centre, long and short sigma, the angle of the long axis (a rotation about the view
axis), opacity logit, colour -- and its 2-D covariance is R diag(long^2, short^2) R^T + 0.3 I (splat_attrs).

Two models of what the compositor owes, both over GIVEN projected records (debug_projected: px, py, A, B, C, log2 alpha, r, g, b,
alpha, ex, ey) and GIVEN bin lists (debug_tile_lists), so that the compositor is judged apart from projection and binning:
  blend_lists          float64, per pixel of every bin, nearest first: e = A dx^2 + B dx dy + C dy^2 + log2 alpha at the pixel centre,
                       a fragment with e <= -8 is discarded, else C += T w c, D += T w z, T *= 1 - w.  Entries whose float64 maximum
                       of e over the bin's pixel centres is below -8.5 are skipped before anything is evaluated (they are discarded
                       at every pixel anyway); bins that keep no entry are not evaluated at all -- the GPU test asserts them exactly
                       clear.  That keeps 4096 x 4096 viewports with needles whose bounding boxes span the screen cheap.
  fp32_reference_form  the same blend in float32 in the oracle's operation order (composite_impl: centre-relative dx, dy, the
                       quadratic form as two matrix-vector products, alpha exp2, back to front d = w c + (1 - w) d): the yardstick
                       E_ref = max |fp32_reference_form - blend_lists| outside budget pixels.
The flip budget of a pixel is the sum of w (|c| + |dst|) over its fragments with |e + 8| <= min(delta, 0.5), delta = N_ROUNDINGS 2^-24 S,
S = |A| a^2 + |B a b| + |C| b^2 + 126 (a, b: the splat's centre relative to the centre of the pixel's 16 x 16 tile); for T and the
depth plane w (1 + 1).  N_ROUNDINGS = 17 is COUNTED in msplat_composite.hip.h, not measured: a, b (lines 305: 2), Aa, Bb, Cb, Ba (307:
4), c1, c2 (308-309: 2), c0 = fma(Aa + Bb, a, fma(Cb, b, log2 alpha - 118)) (318: 4), base (402: 2), lin (403: 1), e (411: 2); u and
v are half-integers below 8 and exact.  (A batch with a record more than 128 px from the tile's centre takes the compensated c0 of lines
319-328, which rounds twice: the count is the plain form's, the larger.)  The cap of 0.5 (BAND_CAP) is not the count's: 4000 px from a needle's centre S is 2e7 and delta
23 -- every fragment of the needle would be exempt, and no offset keeps such a case under the 2 % below.  Beyond 0.5 the count
says nothing the fp32 reference form's own error, which the bound holds twice, does not say; the cull of blend_lists assumes the
same 0.5.

walk() restates the kernel's batch pipeline in float64 per (bin, quadrant) work item: batches of 64 entries, strips that die once
their 64 pixels are below t_epsilon, records dropped because they reach dead strips only -- what the probe's words 1 and 2 must show.

Case families (a Case: attrs of an SH0 cloud, the view, claims):
  batch_edges   96 x 64 px, six bins of 1, 63, 64, 65, 127, 128 entries (frame 1: 129, 191, 192, 193, 256, 257), alpha ~ 0.03 so that
                no strip saturates and every batch runs; colours unclamped: negative ones, and 1e4 in one bin
  saturation    opaque stacks (alpha ~ 0.99) on one 32 x 32 bin: "one" / "two": all four strips die after exactly one / two batches
                with 100 more entries behind; "bar": 64 bars over rows 0 ... 3 of every tile kill strip 0 only, farther splats then
                reach strip 0 only, strips 0 and 1, all four; "mid": saturation in the middle of a batch; "exact": logit 20 is alpha
                = 1.0 in float32 and the centre sits on a pixel centre: T = 0 exactly there; "edge" (64 x 32 px, 1100 splats): a batch
                boundary at which t_epsilon = 1/64 ends the walk and the default does not, and a two-pass cut at rank 1024 that hands
                pass 1 an incomplete batch
  tile_test     needles at 45, 20 and 80 degrees past the four corners of a tile: the float64 maximum of e over the tile's pixel
                centres is -8 + {1, 0.2, 0.12} and -8.05 - {0.2, 1}, at 0, 500 and 2000 px from the needle's centre; and splats of
                covariance 0.3 I centred between pixel centres with alpha 0.006: listed, they light nothing
  threshold     isotropic splats whose e at one chosen pixel centre is -8 +- {1e-2, 1e-3}; off-grid centres keep the other pixels
                out of the band (the 2 % cap below is the proof)
  conditioning  needles of short variance 0.5 px^2 and long sigma max(100, 0.5 d) at 45 and 10 degrees that cross tiles d = 100,
                500, 1000, 2000, 4000 px from their centres (2048^2, from 2000 on 4096^2), centres inside the viewport and in the
                guard band outside it; three needles per tile at most.  (Long sigmas end at 2000 px: beyond, the projection's float32
                determinant cancels by more than the whole -- tests/test_compositor_limits_fixtures.py tells it)
  ragged        333 x 211, 17 x 5 (strips 2 and 3 of the only tile lie outside the image) and 1 x 1
Per case at most 2 % of the evaluated pixels may need the flip budget (asserted by the fixture module on the model alone).
(Not reachable: a colour of -0.0.  An SH0 colour is 0.5 + s, which rounds to +0.0.)"""
import collections
import functools
import math

import numpy as np

from tests import binning_limit_cases as blc
from tests import scenes

BIN, TILE, BATCH = 32, 16, 64
LOG2E = 1.4426950408889634
KK = -0.5 * LOG2E
SH0 = 0.28209479177387814
N_ROUNDINGS = 17
BAND_CAP = 0.5                          # the flip band's half width is min(delta, this): see the module docstring
CULL = -8.5                             # blend_lists skips a list entry whose float64 max of e over the bin is below this
INSET = blc.INSET
RANK_MASK = 0xFFFFFF
T_EPS_DEFAULT = 1.0 / 16384.0
T_EPS = (0.0, T_EPS_DEFAULT, 1.0 / 64.0)
FAINT, OPAQUE, EXACT = -3.5, 4.6, 20.0  # logits: alpha 0.029, 0.990, 1.0

Case = collections.namedtuple("Case", "name attrs view claims")


# ---- clouds --------------------------------------------------------------------------------------------------------------------

class Splats:
    """splats in pixels, in upload order = far to near"""

    def __init__(self):
        self.rows = []

    def add(self, cx, cy, s_long, s_short, theta, logit, colour):
        cx, cy, s_long, s_short, theta, logit = np.broadcast_arrays(*(np.atleast_1d(np.asarray(a, np.float64)) for a in (cx, cy, s_long, s_short, theta, logit)))
        colour = np.broadcast_to(np.asarray(colour, np.float64), (cx.shape[0], 3))
        self.rows.append(np.column_stack([cx, cy, s_long, s_short, theta, logit, colour]))
        return self

    def table(self, order=None):
        t = np.concatenate(self.rows) if self.rows else np.zeros((0, 9))
        return t if order is None else t[order]


def splat_attrs(table, v):
    """attributes of the cloud whose splat i has the pixel-space design table[i] in view v, rank i"""
    n = table.shape[0]
    W, H = v[2][2], v[2][3]
    fx, fy = blc.focal(v)
    assert abs(fx - fy) <= 1e-4 * fx, (fx, fy)
    depth = blc.descending_depths(n)
    cx, cy, sl, ss, th, logit = (table[:, k] for k in range(6))
    xyz = np.stack([(cx - W / 2.0) * depth / fx, (cy - H / 2.0) * depth / fy, -depth], axis=1).astype(np.float32)
    log_scale = np.stack([np.log(sl * depth / fx), np.log(ss * depth / fx), np.full(n, blc.Z_LOG_SCALE)], axis=1).astype(np.float32)
    rot = np.zeros((n, 4), np.float32)
    rot[:, 0], rot[:, 3] = np.cos(th / 2.0), np.sin(th / 2.0)
    f_dc = ((table[:, 6:9] - 0.5) / SH0).astype(np.float32)
    return dict(xyz=xyz, f_dc=f_dc, f_rest=None, opacity=logit.astype(np.float32), log_scale=log_scale, rot=rot)


def cloud_of(case):
    return scenes.cloud_from_attrs(case.attrs, full_sh=False)


def make(name, splats, W, H, reaches, order=None, **claims):
    v = blc.view(W, H)
    table = splats.table(order)
    table.setflags(write=False)
    claims.update(reaches=reaches, n=table.shape[0], table=table)
    claims.setdefault("lengths", None)
    return Case(name, splat_attrs(table, v), v, claims)


def rho_of(logit):
    return np.sqrt(2.0 * np.log(256.0 * blc.alpha_of(logit)))


def tiles_of(W, H):
    return (W + BIN - 1) // BIN, (H + BIN - 1) // BIN


def rec12_of(sp, F=np.float32):
    """the library's projected records from the oracle's splats, in project_kernel's float32 arithmetic (F = np.float64: the same
    values without a rounding after the oracle's, for the comparison with orc.composite_f64)"""
    inv = sp["inv"].astype(F)
    rho2 = F(2.0) * np.log(F(256.0) * sp["alpha"].astype(F)).astype(F)
    with np.errstate(invalid="ignore"):
        ex = np.sqrt(rho2 * sp["cov"][:, 0]).astype(F) * F(1.0001) + F(0.01)
        ey = np.sqrt(rho2 * sp["cov"][:, 3]).astype(F) * F(1.0001) + F(0.01)
    k = F(KK)
    return np.column_stack([sp["px"], sp["py"], k * inv[:, 0], k * (inv[:, 1] + inv[:, 2]), k * inv[:, 3], np.log2(sp["alpha"].astype(F)).astype(F),
                            sp["rgb"][:, 0], sp["rgb"][:, 1], sp["rgb"][:, 2], sp["alpha"], ex, ey]).astype(F)


# ---- the models ----------------------------------------------------------------------------------------------------------------

def emax_box(rec, x0, x1, y0, y1):
    """float64 maximum of e over the box [x0, x1] x [y0, y1] per record (rows of rec, boxes broadcast): e is a concave quadratic, so
    unless the centre lies in the box the maximum is on an edge, at the clamped 1-D maximiser"""
    rec = np.asarray(rec, np.float64)
    px, py, A, B, C, la = (rec[..., k] for k in range(6))
    dxl, dxh, dyl, dyh = x0 - px, x1 - px, y0 - py, y1 - py
    inside = (dxl <= 0) & (dxh >= 0) & (dyl <= 0) & (dyh >= 0)
    best = np.full(np.broadcast(px, dxl).shape, -np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        for dx in (dxl, dxh):
            dy = np.clip(-B * dx / (2.0 * C), dyl, dyh)
            best = np.maximum(best, A * dx * dx + B * dx * dy + C * dy * dy + la)
        for dy in (dyl, dyh):
            dx = np.clip(-B * dy / (2.0 * A), dxl, dxh)
            best = np.maximum(best, A * dx * dx + B * dx * dy + C * dy * dy + la)
    return np.where(inside, la, best)


def kept_lists(rec12, tile_start, pairs, W, H):
    """(bins, idx): the bins that keep an entry after the float64 cull, and per such bin its kept ranks NEAREST FIRST, -1 padded"""
    tiles_x, tiles_y = tiles_of(W, H)
    ts = np.asarray(tile_start, np.int64)
    assert ts.shape[0] == tiles_x * tiles_y + 1, (ts.shape, tiles_x, tiles_y)
    lengths = np.diff(ts)
    rank = (np.asarray(pairs[ts[0]:ts[-1]], np.int64) & RANK_MASK)
    b = np.repeat(np.arange(lengths.shape[0]), lengths)
    bx, by = b % tiles_x, b // tiles_x
    em = emax_box(np.asarray(rec12, np.float64)[rank], bx * BIN + 0.5, np.minimum(bx * BIN + BIN, W) - 0.5,
                  by * BIN + 0.5, np.minimum(by * BIN + BIN, H) - 0.5)
    keep = em > CULL
    b, rank = b[keep][::-1], rank[keep][::-1]                    # nearest first within every bin (stable below)
    o = np.argsort(b, kind="stable")
    b, rank = b[o], rank[o]
    bins, first, cnt = np.unique(b, return_index=True, return_counts=True)
    idx = np.full((bins.shape[0], int(cnt.max()) if cnt.size else 0), -1, np.int64)
    pos = np.arange(b.shape[0]) - np.repeat(first, cnt)
    idx[np.repeat(np.arange(bins.shape[0]), cnt), pos] = rank
    return bins, idx


def pixel_grid(bins, W, H):
    """(X, Y, valid, xc, yc) per pixel of the bins, (len(bins), 1024): pixel centres, inside the image, centre of the pixel's tile"""
    tiles_x, _ = tiles_of(W, H)
    p = np.arange(BIN * BIN)
    xi = (bins % tiles_x)[:, None] * BIN + (p % BIN)[None, :]
    yi = (bins // tiles_x)[:, None] * BIN + (p // BIN)[None, :]
    return xi + 0.5, yi + 0.5, (xi < W) & (yi < H), (xi // TILE) * TILE + 0.5 * TILE, (yi // TILE) * TILE + 0.5 * TILE


def blend_lists(rec12, tile_start, pairs, W, H, zw=None, chunk=256, kept=None):
    """the float64 blend of given records over given bin lists (the module docstring has the definition).  Returns a dict over the
    evaluated bins, pixels as (bin, 1024 = 32 rows of 32): bins, valid, colour (.., 3), T, depth (D + T), budget (colour), budget1
    (T and the depth plane), cmax (max |c| of the bin's kept entries), flagged (pixels with a fragment in the band), smax (the
    largest S of a lit fragment).  kept: the (bins, idx) of kept_lists to walk instead of the records' own"""
    rec = np.asarray(rec12, np.float64)
    z = np.zeros(rec.shape[0]) if zw is None else np.asarray(zw, np.float64)
    bins, idx = kept_lists(rec12, tile_start, pairs, W, H) if kept is None else kept
    nb = bins.shape[0]
    out = dict(bins=bins, valid=np.zeros((nb, 1024), bool), colour=np.zeros((nb, 1024, 3)), T=np.ones((nb, 1024)), depth=np.ones((nb, 1024)),
               budget=np.zeros((nb, 1024)), budget1=np.zeros((nb, 1024)), cmax=np.zeros(nb), flagged=np.zeros((nb, 1024), bool))
    ulp = 2.0 ** -24
    smax = [126.0]
    for c0 in range(0, nb, chunk):
        sl = slice(c0, min(c0 + chunk, nb))
        X, Y, valid, xc, yc = pixel_grid(bins[sl], W, H)
        ix = idx[sl]
        L = (ix >= 0).sum(axis=1)
        Cc, T, D = np.zeros(X.shape + (3,)), np.ones(X.shape), np.zeros(X.shape)
        steps = []

        def fragment(j):
            act = np.flatnonzero(L > j)
            r = rec[ix[act, j]]
            dx, dy = X[act] - r[:, 0:1], Y[act] - r[:, 1:2]
            e = r[:, 2:3] * dx * dx + r[:, 3:4] * dx * dy + r[:, 4:5] * dy * dy + r[:, 5:6]
            a, b = r[:, 0:1] - xc[act], r[:, 1:2] - yc[act]
            S = np.abs(r[:, 2:3]) * a * a + np.abs(r[:, 3:4] * a * b) + np.abs(r[:, 4:5]) * b * b + 126.0
            w = np.where(e > -8.0, np.exp2(np.minimum(e, 0.0)), 0.0)
            band = np.abs(e + 8.0) <= np.minimum(N_ROUNDINGS * ulp * S, BAND_CAP)
            smax[0] = max(smax[0], float(np.where((w > 0.0) & valid[act], S, 0.0).max()))
            return act, r, w, band, np.exp2(np.minimum(e, 0.0))

        anyband = False
        for j in range(int(L.max())):
            act, r, w, band, _ = fragment(j)
            tw = T[act] * w
            Cc[act] += tw[..., None] * r[:, None, 6:9]
            D[act] += tw * z[ix[act, j]][:, None]
            T[act] *= 1.0 - w
            anyband = anyband or bool((band & valid[act]).any())
            out["cmax"][c0 + act] = np.maximum(out["cmax"][c0 + act], np.abs(r[:, 6:9]).max(axis=1))
        bud, bud1, flagged = np.zeros(X.shape), np.zeros(X.shape), np.zeros(X.shape, bool)
        if anyband:                                                # back to front, for |dst| of the fragments in the band
            dst = np.zeros(X.shape + (3,))
            for j in range(int(L.max()) - 1, -1, -1):
                act, r, w, band, wraw = fragment(j)
                cm, dm = np.abs(r[:, 6:9]).max(axis=1)[:, None], np.abs(dst[act]).max(axis=-1)
                bud[act] += np.where(band, wraw * (cm + dm), 0.0)
                bud1[act] += np.where(band, 2.0 * wraw, 0.0)
                flagged[act] |= band
                dst[act] = w[..., None] * r[:, None, 6:9] + (1.0 - w)[..., None] * dst[act]
        out["valid"][sl], out["colour"][sl], out["T"][sl], out["depth"][sl] = valid, Cc, T, D + T
        out["budget"][sl], out["budget1"][sl], out["flagged"][sl] = bud, bud1, flagged & valid
    out["smax"] = smax[0]
    return out


def fp32_reference_form(rec12, tile_start, pairs, W, H, zw=None, chunk=256):
    """blend_lists' colour, T and depth in float32 in composite_impl's operation order, over the same kept entries"""
    F = np.float32
    rec = np.asarray(rec12, F)
    z = np.zeros(rec.shape[0], F) if zw is None else np.asarray(zw, F)
    bins, idx = kept_lists(rec12, tile_start, pairs, W, H)
    nb = bins.shape[0]
    out = dict(bins=bins, colour=np.zeros((nb, 1024, 3), F), T=np.ones((nb, 1024), F), depth=np.ones((nb, 1024), F))
    for c0 in range(0, nb, chunk):
        sl = slice(c0, min(c0 + chunk, nb))
        X, Y, _, _, _ = pixel_grid(bins[sl], W, H)
        X, Y = X.astype(F), Y.astype(F)
        ix = idx[sl]
        L = (ix >= 0).sum(axis=1)
        d, T, dz = np.zeros(X.shape + (3,), F), np.ones(X.shape, F), np.ones(X.shape, F)
        for j in range(int(L.max()) - 1, -1, -1):                  # far to near: the oracle's draw order
            act = np.flatnonzero(L > j)
            r = rec[ix[act, j]]
            dx, dy = X[act] - r[:, 0:1], Y[act] - r[:, 1:2]
            A, Bh, C = r[:, 2:3], F(0.5) * r[:, 3:4], r[:, 4:5]
            mx = A * dx + Bh * dy
            my = Bh * dx + C * dy
            q = dx * mx + dy * my
            sa = r[:, 9:10] * np.exp2(np.minimum(q, F(0.0)))
            sa = np.where(sa <= F(1.0 / 256.0), F(0.0), sa)        # discard: a zero weight is an exact no-op below
            oma = F(1.0) - sa
            d[act] = sa[..., None] * r[:, None, 6:9] + oma[..., None] * d[act]
            dz[act] = sa * z[ix[act, j]][:, None] + oma * dz[act]
            T[act] = oma * T[act]
        assert d.dtype == F and T.dtype == F and dz.dtype == F
        out["colour"][sl], out["T"][sl], out["depth"][sl] = d, T, dz
    return out


def reference_error(model, form):
    """E_ref per quantity: max |fp32_reference_form - blend_lists| over valid pixels outside the flip budget"""
    ok = model["valid"] & ~model["flagged"]
    e = {}
    for k in ("colour", "T", "depth"):
        d = np.abs(form[k].astype(np.float64) - model[k])
        e[k] = float(d[ok].max()) if ok.any() else 0.0
    return e


def bound_of(model, E, t_eps):
    """the GPU test's bound per colour value and per T / depth value (ISSUE: 1e-4 max(1, max|c|) + 2 E_ref + t_eps max|c| + flips;
    max|c| is taken per BIN, which is never wider than per case)"""
    cm = model["cmax"][:, None]
    return (1e-4 * np.maximum(1.0, cm) + 2.0 * E["colour"] + t_eps * cm + model["budget"],
            1e-4 + 2.0 * E["T"] + t_eps + model["budget1"], 1e-4 + 2.0 * E["depth"] + t_eps + model["budget1"])


def blocks(img, bins, W, H):
    """the pixels of a (H, W[, ch]) image as (len(bins), 1024[, ch]) blocks, zeros outside the image; and the mask of the pixels of
    all OTHER bins, (H, W)"""
    tiles_x, tiles_y = tiles_of(W, H)
    ch = img.shape[2:]
    full = np.zeros((tiles_y * BIN, tiles_x * BIN) + ch, img.dtype)
    full[:H, :W] = img
    full = full.reshape((tiles_y, BIN, tiles_x, BIN) + ch)
    full = np.moveaxis(full, 2, 1).reshape((tiles_y * tiles_x, BIN * BIN) + ch)
    other = np.ones(tiles_y * tiles_x, bool)
    other[bins] = False
    mask = np.repeat(np.repeat(other.reshape(tiles_y, tiles_x), BIN, axis=0), BIN, axis=1)[:H, :W]
    return full[bins], mask


def walk(rec12, tile_start, pairs, W, H, t_eps, only_bins=None, any_test=True):
    """The kernel's walk per (bin, quadrant) work item whose tile lies in the image, in float64: dict (bin, quad) -> (list length,
    batches staged, lo, hi, safe, inband).  lo: records that light (e > -8) a pixel of a strip that is alive when their batch is
    staged; hi: records whose y reach (py +- ey) meets an alive strip and whose maximum of e over the tile's pixel-centre box is
    above -8.15.  safe: at every batch boundary every strip's largest T is below t_eps / 4 or above 4 t_eps (float32 cannot move
    the batch count).  inband: staged records whose emax lies in [-8.15, -7.9], where float32 may decide either way.
    any_test = False: the walk of a kernel WITHOUT the test that drops records which reach dead strips only (the fixture module
    shows that its count leaves [lo, hi])"""
    rec = np.asarray(rec12, np.float64)
    tiles_x, tiles_y = tiles_of(W, H)
    ts = np.asarray(tile_start, np.int64)
    res = {}
    lx, ly = np.arange(256) % TILE, np.arange(256) // TILE
    for b in (range(tiles_x * tiles_y) if only_bins is None else only_bins):
        ranks = (np.asarray(pairs[ts[b]:ts[b + 1]], np.int64) & RANK_MASK)[::-1]
        for quad in range(4):
            x0, y0 = (b % tiles_x) * BIN + (quad & 1) * TILE, (b // tiles_x) * BIN + (quad >> 1) * TILE
            if x0 >= W or y0 >= H:
                continue
            X, Y = x0 + lx + 0.5, y0 + ly + 0.5
            valid = (x0 + lx < W) & (y0 + ly < H)
            strip = ly // 4
            alive = np.array([bool(valid[strip == k].any()) for k in range(4)])
            present = alive.copy()
            T = np.ones(256)
            batches = lo = hi = inband = 0
            safe = True
            for s in range(0, ranks.shape[0], BATCH):
                if not alive.any():
                    break
                r = rec[ranks[s:s + BATCH]]
                batches += 1
                dx, dy = X[None, :] - r[:, 0:1], Y[None, :] - r[:, 1:2]
                e = r[:, 2:3] * dx * dx + r[:, 3:4] * dx * dy + r[:, 4:5] * dy * dy + r[:, 5:6]
                counted = alive if any_test else present
                live_px = valid & counted[strip]
                lo += int(((e > -8.0) & live_px[None, :]).any(axis=1).sum())
                em = emax_box(r, x0 + 0.5, x0 + TILE - 0.5, y0 + 0.5, y0 + TILE - 0.5)
                reach = np.zeros(r.shape[0], bool)
                for k in range(4):
                    if counted[k]:
                        reach |= (r[:, 1] + r[:, 11] >= y0 + 4 * k + 0.5) & (r[:, 1] - r[:, 11] <= y0 + 4 * k + 3.5)
                hi += int((reach & (em > -8.15)).sum())
                inband += int((reach & (em >= -8.15) & (em <= -7.9)).sum())
                w = np.where(e > -8.0, np.exp2(np.minimum(e, 0.0)), 0.0)
                T = T * np.prod(1.0 - w, axis=0)
                for k in range(4):
                    m = valid & (strip == k)
                    if m.any():
                        tmax = T[m].max()
                        alive[k] = tmax >= t_eps
                        safe = safe and (t_eps == 0.0 or tmax < t_eps / 4.0 or tmax > 4.0 * t_eps)
            res[(int(b), quad)] = (int(ranks.shape[0]), batches, lo, hi, bool(safe), inband)
    return res


# ---- batch_edges ---------------------------------------------------------------------------------------------------------------

BATCH_LENGTHS = ((1, 63, 64, 65, 127, 128), (129, 191, 192, 193, 256, 257))
HUGE_BIN = 3                            # the bin whose colours reach 1e4


@functools.lru_cache(maxsize=None)
def batch_edges(frame):
    W, H = 96, 64
    rng = np.random.default_rng(300 + frame)
    s, which = Splats(), []
    rho = float(rho_of(FAINT))
    for b, L in enumerate(BATCH_LENGTHS[frame]):
        x0, y0 = (b % 3) * BIN, (b // 3) * BIN
        off = rng.uniform(-6.0, 6.0, (L, 2))
        room = (0.5 * BIN - INSET - np.abs(off).max(axis=1)) / rho          # sqrt(long^2 + 0.3) may be this much
        s_long = np.sqrt(np.minimum(room, rng.uniform(2.0, 3.6, L)) ** 2 - 0.3)
        col = 0.8 * rng.standard_normal((L, 3))
        if b == HUGE_BIN:
            col[::7] = (1e4, -1e4, 3e3)
        s.add(x0 + 16.0 + off[:, 0], y0 + 16.0 + off[:, 1], s_long, s_long * rng.uniform(0.4, 1.0, L), rng.uniform(0.0, np.pi, L), FAINT, col)
        which += [b] * L
    order = rng.permutation(len(which))                           # the bins' entries interleave in rank
    return make("batch_edges_%d" % frame, s, W, H, "lists of exactly 1 ... 257 entries: full, short and empty batches in the pipeline",
                order=order, lengths=np.array(BATCH_LENGTHS[frame]), probe=True)


# ---- saturation ----------------------------------------------------------------------------------------------------------------

SATURATION = ("one", "two", "bar", "mid", "exact", "edge")
EDGE_V, EDGE_CUT = 1100, 1024           # saturation("edge"): occ_cut(1100, 1 / 64) = (1100 - 64) & ~1023


def blanket(s, n, logit, rng, W=BIN, H=BIN):
    """n splats of sigma 200 px centred near the viewport's middle: w ~ alpha at every pixel"""
    s.add(W / 2.0 + rng.uniform(-3, 3, n), H / 2.0 + rng.uniform(-3, 3, n), 200.0, 180.0, rng.uniform(0, np.pi, n), logit,
          0.8 * rng.standard_normal((n, 3)))


def specks(s, n, rng, x0):
    """n faint specks spread over the bin at x0"""
    s.add(x0 + rng.uniform(6, 26, n), rng.uniform(6, 26, n), 1.2, 0.8, rng.uniform(0, np.pi, n), FAINT, 0.8 * rng.standard_normal((n, 3)))


@functools.lru_cache(maxsize=None)
def saturation(variant):
    """one 32 x 32 bin (four tiles).  Upload order is far to near: what is added LAST is walked FIRST"""
    rng = np.random.default_rng(400 + SATURATION.index(variant))
    s = Splats()
    if variant == "one":          # nearest batch: 60 faint + 4 opaque -> T ~ 0.17 x 1e-8; then 100 more
        blanket(s, 100, FAINT, rng); blanket(s, 60, FAINT, rng); blanket(s, 4, OPAQUE, rng)
        batches = {0.0: 3, T_EPS_DEFAULT: 1, 1.0 / 64.0: 1}
    elif variant == "two":        # batch 1: 64 faint (T ~ 0.15 > 4 / 64); batch 2: 4 opaque among 60 faint; then 100 more
        blanket(s, 100, FAINT, rng); blanket(s, 60, FAINT, rng); blanket(s, 4, OPAQUE, rng); blanket(s, 64, FAINT, rng)
        batches = {0.0: 4, T_EPS_DEFAULT: 2, 1.0 / 64.0: 2}
    elif variant == "mid":        # 4 opaque blankets in the MIDDLE of the first batch (entries 30 ... 33), 100 more behind the batch
        blanket(s, 100, FAINT, rng); blanket(s, 30, FAINT, rng); blanket(s, 4, OPAQUE, rng); blanket(s, 30, FAINT, rng)
        batches = {0.0: 3, T_EPS_DEFAULT: 1, 1.0 / 64.0: 1}
    elif variant == "exact":      # alpha = 1.0f on pixel centres (8.5, 8.5) and (24.5, 20.5), small splats; 70 faint blankets behind
        blanket(s, 70, FAINT, rng)
        s.add([8.5, 24.5], [8.5, 20.5], 2.0, 1.5, [0.3, 1.1], EXACT, [[0.9, -0.4, 0.2], [0.1, 0.7, 1.5]])
        batches = {0.0: 2, T_EPS_DEFAULT: 2, 1.0 / 64.0: 2}
    elif variant == "edge":
        # 64 x 32 px, bins A (x < 32) and B.  104 blankets over both; B also holds 996 specks.  A's list, nearest first: 57 faint + 7
        # half-transparent blankets = ONE batch that leaves T ~ 1e-3 -- below (1/64) / 4, above 4 / 16384 --, then 40 opaque BRIGHT
        # ones: with t_epsilon = 1/64 A's walk ends after the batch and the bright ones are never blended, a difference of ~1e-3.
        # V = 1100, and the nearest 76 splats are 30 of A's batch and 46 specks of B: pass 1 of a two-pass frame at share 1/64
        # (cut = 1024) gets 30 entries of A, an incomplete batch it must not start on
        B = BIN
        specks(s, EDGE_V - 40 - 34 - 76, rng, B)
        s.add(32.0 + rng.uniform(-3, 3, 40), 16.0 + rng.uniform(-3, 3, 40), 200.0, 180.0, rng.uniform(0, np.pi, 40), OPAQUE, [3.0, 2.0, 4.0])
        far = Splats()                                             # the batch's farther 34: the half-transparent ones among them
        blanket(far, 27, FAINT, rng, 2 * BIN, BIN); blanket(far, 7, 0.0, rng, 2 * BIN, BIN)
        s.rows.append(far.table(rng.permutation(34)))
        mix = Splats()                                             # its nearest 30, faint (B's first batch leaves T ~ 0.6), among B's specks
        blanket(mix, 30, FAINT, rng, 2 * BIN, BIN); specks(mix, 46, rng, B)
        s.rows.append(mix.table(rng.permutation(76)))
        return make("saturation_edge", s, 2 * BIN, BIN, "a strip test that decides at a batch boundary; pass 1 in front of an incomplete batch",
                    lengths=np.array([104, EDGE_V]), batches={0.0: 2, T_EPS_DEFAULT: 2, 1.0 / 64.0: 1}, probe=True)
    else:                         # bar: farther splats per tile that reach strip 0 only, strips 0 and 1, all four; 64 bars nearest
        for tx in range(2):
            for ty in range(2):
                x0, y0 = tx * TILE, ty * TILE
                s.add(x0 + rng.uniform(4, 12, 20), y0 + rng.uniform(1.5, 2.2, 20), 1.2, 0.3, 0.0, 2.0, 0.8 * rng.standard_normal((20, 3)))     # strip 0 only
                s.add(x0 + rng.uniform(4, 12, 20), y0 + rng.uniform(3.6, 4.4, 20), 1.2, 0.9, 0.0, 2.0, 0.8 * rng.standard_normal((20, 3)))     # strips 0 and 1
                s.add(x0 + rng.uniform(6, 10, 20), y0 + rng.uniform(7.5, 8.5, 20), 3.0, 3.0, 0.0, 2.0, 0.8 * rng.standard_normal((20, 3)))     # all four
        order = rng.permutation(240)
        far = s.table(order)
        s = Splats()
        s.rows.append(far)
        for k in range(64):       # bars over rows 0 ... 3 of the tiles of bin row k % 2, as wide as the viewport
            s.add(16.0 + rng.uniform(-2, 2), (k % 2) * TILE + 2.0, 200.0, math.sqrt(3.7), 0.0, OPAQUE, 0.8 * rng.standard_normal(3))
        batches = None
    return make("saturation_" + variant, s, BIN, BIN, "strips that die between batches; records that reach dead strips only",
                lengths=np.array([s.table().shape[0]]), batches=batches, probe=True)


# ---- tile_test -----------------------------------------------------------------------------------------------------------------

TILE_ANGLES = (45.0, 20.0, 80.0)
TILE_TARGETS = (-7.0, -7.8, -7.88, -8.25, -9.05)     # -8 + {1, 0.2}, -8.05 - {0.2, 1}; and -8 + 0.12, clear of a slack of -0.2
TILE_DISTANCES = {0: (512, 60.0), 500: (1024, 180.0), 2000: (3072, 1000.0)}      # distance -> (viewport edge, long sigma)
NEEDLE_SHORT = math.sqrt(0.2)                        # short variance 0.2 + 0.3 = 0.5 px^2
NEEDLE_LOGIT = 2.5


def needle_past_corner(P, sx, sy, angle, target, d, s_long, logit=NEEDLE_LOGIT):
    """(cx, cy, theta) of the needle whose e at the pixel centre P -- the (sx, sy) corner of a tile's pixel-centre box -- is `target`,
    P lying d px along the needle from its centre and the needle passing OUTSIDE the box: its direction is mirrored for the corners
    it would otherwise cut through"""
    th = math.radians(angle) * (-sx * sy)
    u = np.array([math.cos(th), math.sin(th)])
    n = np.array([-u[1], u[0]])
    if n[0] * sx + n[1] * sy < 0:
        n = -n
    la = math.log2(float(blc.alpha_of(logit)))
    t2 = ((target - la) / KK - d * d / (s_long ** 2 + 0.3)) * (NEEDLE_SHORT ** 2 + 0.3)
    assert t2 > 0, (target, d, s_long)
    c = np.asarray(P, np.float64) + math.sqrt(t2) * n - d * u
    return c[0], c[1], th


@functools.lru_cache(maxsize=None)
def tile_test(d):
    """60 needles, one per (corner, angle, target), each aimed at a tile of its own (tiles 3 apart); 16 minimum-size splats between
    pixel centres.  claims["aims"]: rows (rank, tile x0, tile y0, target)"""
    W, s_long = TILE_DISTANCES[d]
    s, aims = Splats(), []
    k = 0
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        for angle in TILE_ANGLES:
            for target in TILE_TARGETS:
                x0 = W // 2 - 4 * 3 * TILE + (k % 8) * 3 * TILE
                y0 = W // 2 - 4 * 3 * TILE + (k // 8) * 3 * TILE
                P = (x0 + (TILE - 0.5 if sx > 0 else 0.5), y0 + (TILE - 0.5 if sy > 0 else 0.5))
                # the centre on the side along the needle that keeps it nearer the viewport's middle (the Sort culls beyond |ndc| = 1.5)
                cx, cy, th = min((needle_past_corner(P, sx, sy, angle, target, sign * d, s_long) for sign in (1.0, -1.0)),
                                 key=lambda c: max(abs(c[0] - W / 2.0), abs(c[1] - W / 2.0)))
                assert max(abs(cx - W / 2.0), abs(cy - W / 2.0)) < 0.74 * W, (d, k, cx, cy)
                s.add(cx, cy, s_long, NEEDLE_SHORT, th, NEEDLE_LOGIT, [0.9 - 0.01 * k, 0.2 + 0.02 * k, 0.5])
                aims.append((k, x0, y0, target))
                k += 1
    for j in range(16):           # covariance 0.3 I, centred on a pixel CORNER: w <= 1/256 at the four nearest pixel centres
        s.add(40.0 + 13 * j, 24.0 + 7 * j, 1e-3, 1e-3, 0.0, math.log(0.006 / 0.994), [5.0, 5.0, 5.0])
    return make("tile_test_%d" % d, s, W, W, "the exact footprint-against-tile test next to its slack", aims=np.array(aims, np.float64),
                dust=np.arange(60, 76), probe=True)


# ---- threshold -----------------------------------------------------------------------------------------------------------------

THRESHOLD_EPS = (1e-2, 1e-3, -1e-3, -1e-2)


@functools.lru_cache(maxsize=None)
def threshold():
    """96 x 64 px: 24 isotropic splats, each with ONE chosen pixel centre P at e = -8 + eps; claims["aims"]: (rank, Px, Py, eps)"""
    W, H = 96, 64
    s, aims = Splats(), []
    la = math.log2(float(blc.alpha_of(1.0)))
    for k in range(24):
        eps = THRESHOLD_EPS[k % 4]
        v = 2.0 + 0.37 * (k // 4)                                   # variance incl. the 0.3
        r = math.sqrt((-8.0 + eps - la) / KK * v)
        phi = 0.4 + 0.83 * k                                        # off-axis, off-diagonal directions
        P = (8.5 + 16 * (k % 6) + (k % 3), 8.5 + 16 * (k // 6) - (k % 2))
        s.add(P[0] - r * math.cos(phi), P[1] - r * math.sin(phi), math.sqrt(v - 0.3), math.sqrt(v - 0.3), 0.0, 1.0, [1.0 + 0.1 * k, -0.5, 0.25])
        aims.append((k, P[0], P[1], eps))
    return make("threshold", s, W, H, "fragments next to the discard threshold, outside the rounding band", aims=np.array(aims), probe=False)


# ---- conditioning --------------------------------------------------------------------------------------------------------------

CONDITIONING_D = (100, 500, 1000, 2000, 4000)
CONDITIONING_ANGLES = (45.0, 10.0)


@functools.lru_cache(maxsize=None)
def conditioning(d):
    """24 needles of long sigma max(100, 0.75 d): every one is aimed at a point Q of the viewport that lies d px along it from its
    centre; half of the centres lie inside the viewport, half in the guard band outside it (the Sort culls beyond |ndc| = 1.5)"""
    W = 2048 if d < 2000 else 4096
    s_long = max(100.0, 0.5 * d)
    rng = np.random.default_rng((600 if d != 4000 else 601) + d)      # (seed 600 puts four needles on one tile at 4000 px)
    s, aims = Splats(), []
    for k in range(24):
        angle = math.radians(CONDITIONING_ANGLES[k % 2])
        want_outside = k % 4 >= 2
        found = None
        for attempt in range(400):                                   # a point Q of the viewport and a centre d px from it, of the wanted kind
            Q = rng.uniform(8.0, W - 8.0, 2) if attempt >= 100 or not want_outside else np.array([rng.uniform(8.0, 60.0), rng.uniform(8.0, W - 8.0)])
            for th in (angle, -angle, angle + math.pi, math.pi - angle):
                c = Q - d * np.array([math.cos(th), math.sin(th)])
                outside = not (0 <= c[0] < W and 0 <= c[1] < W)
                if np.abs(c - W / 2.0).max() < 0.74 * W and outside == want_outside:
                    found = (c, th, Q)
                    break
            if found:
                break
        assert found, (d, k)
        c, th, Q = found
        s.add(c[0], c[1], s_long, NEEDLE_SHORT, th, NEEDLE_LOGIT, [0.3 + 0.05 * k, 1.2 - 0.04 * k, 0.6])
        aims.append((k, Q[0], Q[1], float(want_outside)))
    return make("conditioning_%d" % d, s, W, W, "c0's three quadratic terms cancel far from the splat's centre", aims=np.array(aims), probe=False)


# ---- ragged --------------------------------------------------------------------------------------------------------------------

RAGGED = ((333, 211), (17, 5), (1, 1))


@functools.lru_cache(maxsize=None)
def ragged(W, H):
    rng = np.random.default_rng(700 + W)
    n = 150 if W > 100 else 12
    s = Splats()
    mx, my = min(4.0, 0.2 * W), min(4.0, 0.2 * H)                  # centres up to 4 px outside, inside the Sort's guard band
    s.add(rng.uniform(-mx, W + mx, n), rng.uniform(-my, H + my, n), rng.uniform(1.0, 9.0, n), rng.uniform(0.4, 2.0, n), rng.uniform(0, np.pi, n),
          rng.uniform(-2.0, 3.0, n), 0.8 * rng.standard_normal((n, 3)))
    return make("ragged_%dx%d" % (W, H), s, W, H, "tiles and strips that end outside the image", probe=False)


CASES = collections.OrderedDict(
    [("batch_edges_%d" % f, functools.partial(batch_edges, f)) for f in (0, 1)]
    + [("saturation_" + v, functools.partial(saturation, v)) for v in SATURATION]
    + [("tile_test_%d" % d, functools.partial(tile_test, d)) for d in TILE_DISTANCES]
    + [("threshold", threshold)]
    + [("conditioning_%d" % d, functools.partial(conditioning, d)) for d in CONDITIONING_D]
    + [("ragged_%dx%d" % wh, functools.partial(ragged, *wh)) for wh in RAGGED])


def t_eps_of(name):
    """the t_epsilon values a case's frame runs with: all three for saturation, the default elsewhere"""
    return T_EPS if name.startswith("saturation") else (T_EPS_DEFAULT,)
