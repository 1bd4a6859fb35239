"""Named inputs for the bin-list build at its limits (inputs only, like sort_limit_cases.py; tests/test_binning_limits_fixtures.py
checks every claim made here on the CPU, tests/test_gpu_binning_limits.py builds the lists on the GPU), and the plain model of
what the two partitions must leave behind (model_lists).

Rectangles are DESIGNED, not drawn.  The camera is sort_limit_cases.view()'s -- camera.pose((0, 0, 0)), the identity, and
camera.perspective(fovy, W / H, zn, zf) with zf a power of two, so depth = -z exactly -- with the focal length max(W, H) / 2 px.
Splat i of a cloud is rank i of the frame: depths are distinct multiples of 2^-12 that descend with the upload index.  A
rectangle (tx0, ty0, tx1, ty1) becomes ONE axis-aligned splat (identity rotation, own x and y scale, a z scale of e^-16) whose
w > 1/256 footprint box -- half extents rho sqrt(cov), rho^2 = 2 ln(256 alpha), cov = (focal s / depth)^2 + 0.3 -- is centred on the
rectangle and ends INSET = 2.75 px inside its border: the kernel widens the box by x 1.0001 + 0.01 px (at most 0.42 px here) and
float32 holds the centre to 1e-3 px, so neither reaches a bin border.  EMPTY is a splat in the middle of the viewport that passes
the Sort's cull with alpha = 3e-4 <= 1/256: it gets a rank and kRectEmpty.  A splat beyond the far plane of a view, or nearer than
its ndc.z = 0.25 plane, keeps its rank too and is kRectEmpty in that view (view_rects).

A case is a Case: attrs of an SH0 cloud, the view (cam, proj, vp, nf), the designed rectangles per rank in that view (int64
(n, 4), EMPTY rows where nothing is drawn) and its claims -- see claims_of -- plus "reaches", the branch it is meant for.
Constants of the kernels are restated here; the fixture module pins the claims that rest on them."""
import collections
import functools
import math

import numpy as np

from splatapult_amd import camera
from tests import scenes

BIN = 32
EMPTY = (255, 0, 0, 0)                  # kRectEmpty = 0x000000FF: tx0 = 255 > tx1 = 0
RECT_EMPTY = 0x000000FF
INSET = 2.75                            # px between the footprint box and the designed rectangle's border (no multiple of 0.5:
                                        # the w = 1/256 contour of stacked equal splats then passes no pixel centre at its tips)
BIN_CHUNK = 1024                        # draw-order ranks per chunk of the column pass (kBinChunk)
PAIR_CHUNK = 4096                       # words per chunk of the row pass (kPairChunk)
WAVE_WORDS = 1024                       # words of a row-pass chunk one wave moves (64 lanes x 16 items)
OWNER_CAP = 8 * BIN_CHUNK               # bin1_downsweep: chunks with more items binary-search s_off
HEAVY_PAIRS, HEAVY_CAP, HEAVY_PARTS = 49152, 128, 8
PAIR_COLS = 4                           # radix_upsweep<MODE_PAIR>: columns of a chunk counted in LDS
GROUP, SUPER = 32, 128                  # chunk rows per group / supergroup of the two-level tables
K_FAR = 6                               # zf = 64 where a case does not choose its own
DEPTH0, STEP = 8.0, 2.0 ** -12
EMPTY_LOGIT, Z_LOG_SCALE = -8.0, -16.0

Case = collections.namedtuple("Case", "name attrs view rects claims")


def view(W, H, zn=0.1, zf=2.0 ** K_FAR):
    fovy = 2.0 * math.atan(H / float(max(W, H)))          # tan(fovy / 2) = (H / 2) / focal, focal = max(W, H) / 2
    return camera.pose((0.0, 0.0, 0.0)), camera.perspective(fovy, W / H, zn, zf), [0, 0, W, H], [zn, zf]


def focal(v):
    """(fx, fy) in px of a view, from the float32 matrix the library and the oracle get"""
    proj, vp = np.asarray(v[1], np.float64), v[2]
    return proj[0] * vp[2] / 2.0, proj[5] * vp[3] / 2.0


def near_for(thr, zf):
    """the near plane whose ndc.z = 0.25 rejection ends at depth thr: ndc.z = A - 2 zf zn / ((zf - zn) depth), A = (zf + zn) / (zf - zn)"""
    return 0.75 * zf * thr / (2.0 * zf - 1.25 * thr)


def descending_depths(n, start=DEPTH0):
    """n distinct depths, descending with the index: the nearest is `start`"""
    d = start + (n - 1 - np.arange(n, dtype=np.float64)) * STEP
    assert n == 0 or d[0] < 2.0 ** K_FAR - 1.0
    return d


def alpha_of(logit):
    """the oracle's float32 sigmoid (build_cloud)"""
    F = np.float32
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + np.exp(-np.asarray(logit, F), dtype=F))).astype(np.float64)


def cloud_attrs(rects, v, depth, logit, seed):
    """attributes of the cloud whose splat i covers rects[i] in view v from depth[i] with opacity logit[i]"""
    rects = np.asarray(rects, np.int64).reshape(-1, 4)
    n = rects.shape[0]
    W, H = v[2][2], v[2][3]
    fx, fy = focal(v)
    empty = rects[:, 0] > rects[:, 2]
    tx0, ty0, tx1, ty1 = (np.where(empty, 0, rects[:, k]) for k in range(4))
    logit = np.where(empty, EMPTY_LOGIT, np.broadcast_to(np.asarray(logit, np.float64), (n,))).astype(np.float32)
    rho2 = 2.0 * np.log(256.0 * np.where(empty, 1.0, alpha_of(logit)))
    assert (rho2 > 1.0).all(), "an opacity too low for a footprint of 13.25 px"
    cx = np.where(empty, W / 2.0, 0.5 * BIN * (tx0 + tx1 + 1))
    cy = np.where(empty, H / 2.0, 0.5 * BIN * (ty0 + ty1 + 1))
    hx = 0.5 * BIN * (tx1 - tx0 + 1) - INSET
    hy = 0.5 * BIN * (ty1 - ty0 + 1) - INSET
    sx, sy = np.sqrt(hx * hx / rho2 - 0.3), np.sqrt(hy * hy / rho2 - 0.3)          # px
    xyz = np.stack([(cx - W / 2.0) * depth / fx, (cy - H / 2.0) * depth / fy, -depth], axis=1).astype(np.float32)
    log_scale = np.stack([np.log(sx * depth / fx), np.log(sy * depth / fy), np.full(n, Z_LOG_SCALE)], axis=1).astype(np.float32)
    rot = np.zeros((n, 4), np.float32)
    rot[:, 0] = 1.0
    f_dc = (0.8 * np.random.default_rng(seed).standard_normal((n, 3))).astype(np.float32)
    return dict(xyz=xyz, f_dc=f_dc, f_rest=None, opacity=logit, log_scale=log_scale, rot=rot)


def cloud_of(case):
    return scenes.cloud_from_attrs(case.attrs, full_sh=False)


def pack(rects):
    """the library's rectangle words"""
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    return (r[:, 0] | (r[:, 1] << 8) | (r[:, 2] << 16) | (r[:, 3] << 24)).astype(np.uint32)


def tiles_of(v):
    return (v[2][2] + BIN - 1) // BIN, (v[2][3] + BIN - 1) // BIN


# ---- the model: what the two stable partitions leave behind -------------------------------------------------------------------

def pairs_of(rects):
    """the (splat, bin) pairs in the order the column pass enumerates them: (rank, tx, ty) arrays, rank-major, then column, then
    row (an item is one column of one rectangle and writes its rows as consecutive words)"""
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    drawn = r[:, 0] <= r[:, 2]
    w = np.where(drawn, r[:, 2] - r[:, 0] + 1, 0)
    h = np.where(drawn, r[:, 3] - r[:, 1] + 1, 0)
    cnt = w * h
    rank = np.repeat(np.arange(r.shape[0], dtype=np.int64), cnt)
    local = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    hh = h[rank]
    return rank, r[rank, 0] + local // hh, r[rank, 1] + local % hh


def lists_from_pairs(rank, tx, ty, tiles_x, tiles_y):
    """(tile_start, words): the pairs stably sorted by bin = ty * tiles_x + tx; a word is (tx << 24) | rank"""
    b = ty * tiles_x + tx
    order = np.argsort(b, kind="stable")
    start = np.zeros(tiles_x * tiles_y + 1, np.int64)
    np.cumsum(np.bincount(b, minlength=tiles_x * tiles_y), out=start[1:])
    return start.astype(np.uint32), ((tx[order] << 24) | rank[order]).astype(np.uint32)


def model_lists(rects, tiles_x, tiles_y):
    """the expected msplat_debug_get_tile_lists of a frame with these rectangles per rank: no chunks, no passes"""
    return lists_from_pairs(*pairs_of(rects), tiles_x, tiles_y)


def claims_of(rects, v, reaches, **more):
    """what the fixture module asserts of a case: M (items = rectangle columns) and pairs per column-pass chunk, D, the words per
    bin column and per bin row, the heavy chunks, and the branch it is meant to reach"""
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    tiles_x, tiles_y = tiles_of(v)
    drawn = r[:, 0] <= r[:, 2]
    w = np.where(drawn, r[:, 2] - r[:, 0] + 1, 0)
    h = np.where(drawn, r[:, 3] - r[:, 1] + 1, 0)
    chunk = np.arange(r.shape[0]) // BIN_CHUNK
    nch = -(-r.shape[0] // BIN_CHUNK)
    M = np.bincount(chunk, weights=w, minlength=nch).astype(np.int64)
    P = np.bincount(chunk, weights=w * h, minlength=nch).astype(np.int64)
    _, tx, ty = pairs_of(r)
    c = dict(n=r.shape[0], M=M, pairs=P, D=int(P.sum()), per_column=np.bincount(tx, minlength=tiles_x),
             per_row=np.bincount(ty, minlength=tiles_y), heavy=int((P > HEAVY_PAIRS).sum()), reaches=reaches)
    c.update(more)
    return c


def make(name, rects, W, H, seed, reaches, logit=2.0, depth=None, zn=0.1, zf=2.0 ** K_FAR, **more):
    rects = np.asarray(rects, np.int64).reshape(-1, 4)
    v = view(W, H, zn, zf)
    if depth is None:
        depth = descending_depths(rects.shape[0])
    assert (np.diff(depth) < 0).all() and (depth.astype(np.float32) == depth).all()
    rects.setflags(write=False)
    return Case(name, cloud_attrs(rects, v, depth, logit, seed), v, rects, claims_of(rects, v, reaches, **more))


def view_rects(case, depth, zn, zf):
    """the case's rectangles in another view of its camera (other near / far planes): EMPTY where the splat is beyond the far plane
    or nearer than the ndc.z = 0.25 plane; the planes keep 0.05 away from every depth (asserted)"""
    thr = 2.0 * zf * zn / (0.75 * zf + 1.25 * zn)
    assert np.abs(depth - zf).min() > 0.05 and np.abs(depth - thr).min() > 0.05
    r = case.rects.copy()
    r[(depth > zf) | (depth < thr)] = EMPTY
    r.setflags(write=False)
    return r


def rect_rows(tx0, ty0, tx1, ty1):
    return np.stack(np.broadcast_arrays(*(np.atleast_1d(a) for a in (tx0, ty0, tx1, ty1))), axis=1).astype(np.int64)


# ---- column pass -----------------------------------------------------------------------------------------------------------

OWNER_EDGE = ("M8191", "M8192", "M8193", "full")


@functools.lru_cache(maxsize=None)
def owner_edge(variant):
    """one chunk of 1024 ranks on 512 x 64 px (16 x 2 bins).  M8191 / M8192 / M8193: 1020 rectangles of 8 columns, 31 / 32 / 33 of
    them 9 wide, and EMPTY at ranks 5, 6, 7 and 500 -- the owner table up to 8192 items, the binary search of s_off from 8193.
    full: every rectangle 16 wide, EMPTY at ranks 0 and 1023, in a run of 17 from 300 and in pairs every 97 ranks: the search
    meets equal offsets at both ends of the table and in its middle (M = 16 x the drawn rectangles: 16384 less the empties' share)"""
    i = np.arange(BIN_CHUNK)
    ty0, ty1 = np.where(i % 3 == 1, 1, 0), np.where(i % 3 == 0, 0, 1)
    if variant == "full":
        r = rect_rows(0, ty0, 15, ty1)
        hole = (i == 0) | (i == 1023) | ((i >= 300) & (i < 317)) | (i % 97 == 50) | (i % 97 == 51)
        r[hole] = EMPTY
        return make("owner_edge_full", r, 512, 64, 11, "binary search of s_off over runs of equal offsets")
    tx0 = i % 8
    r = rect_rows(tx0, ty0, tx0 + 7, ty1)
    wide = np.flatnonzero(tx0 < 7)[::25][:{"M8191": 31, "M8192": 32, "M8193": 33}[variant]]
    r[wide, 2] += 1
    r[[5, 6, 7, 500]] = EMPTY
    return make("owner_edge_" + variant, r, 512, 64, 12,
                "owner table (M <= 8192)" if variant != "M8193" else "binary search of s_off (M = 8193)")


THIN_M = (0, 1, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def thin_chunks(m):
    """three chunks on 512 x 64 px whose middle one has m items: m single-column rectangles at ranks 1024 + 3 j, the rest EMPTY;
    per_wave = roundup64(ceil(m / 4)) leaves one to three waves (all four at m = 0) without an item"""
    i = np.arange(3 * BIN_CHUNK)
    r = rect_rows(i % 13, i % 2, i % 13 + 3, np.maximum(i % 2, (i // 2) % 2))
    mid = np.arange(BIN_CHUNK, 2 * BIN_CHUNK)
    r[mid] = EMPTY
    j = np.arange(m)
    r[BIN_CHUNK + 3 * j] = rect_rows(j % 16, j % 2, j % 16, np.maximum(j % 2, (j // 5) % 2))
    per_wave = (((m + 3) >> 2) + 63) & ~63
    idle = sum(1 for w in range(4) if w * per_wave >= m)
    return make("thin_chunks_%d" % m, r, 512, 64, 20 + m, "waves without an item", idle_waves=idle)


@functools.lru_cache(maxsize=None)
def store_shapes():
    """32 x 416 px (1 x 13 bins), one column: the position of an item's first word is the running sum of the earlier heights, and
    every (pos mod 4, rows) with rows = 1 ... 12 occurs (single rows fill up to the wanted alignment): one-word head, two-word
    head, 16-byte body, two-word and one-word tail in every combination"""
    rows, pos = [], 0
    for h in range(1, 13):
        for a in range(4):
            while pos % 4 != a:
                rows.append(1); pos += 1
            rows.append(h); pos += h
    rows = np.array(rows)
    k = np.arange(rows.size)
    ty0 = (5 * k) % (14 - rows)
    r = rect_rows(0, ty0, 0, ty0 + rows - 1)
    pos = np.cumsum(rows) - rows
    combos = set(zip((pos % 4).tolist(), rows.tolist()))
    return make("store_shapes", r, 32, 416, 30, "every head / body / tail of the emit", logit=-1.0, pos=pos, combos=combos)


@functools.lru_cache(maxsize=None)
def heavy_edge(extra):
    """1536 x 1024 px (48 x 32 bins), two chunks.  Chunk 0: 1024 rectangles of 48 x 1 bins = 49152 pairs, not heavy; extra: rank 512
    is 7 x 7 = 49 bins instead, 49153 pairs, heavy.  Chunk 1: 1024 SQUARE rectangles of one or four bins (the nearer half of the
    splats: pass 1 of a two-pass frame at a share of 1/2).  Square, because the frame is compared with the oracle's image: the
    reference's geometry stage turns its 3.5-sigma quad by theta = atan2(major - cov_xx, cov_xy), and an axis-aligned splat away
    from the viewport's centre has cov_xy ~ 1e-12, not 0 -- theta is then the quotient of two rounding residues, and for 54 of
    256 rectangles of 2 x 1 bins it came out as pi / 2: the quad stands upright and cuts the splat's ends off (measured: the
    library equals the float64 definition to 1.3e-6 there, the oracle misses up to 0.016).  A round splat's quad holds its
    footprint at any theta; the other image-checked cases sit on the viewport's centre line, where cov_xy is exactly 0.
    tests/test_binning_limits_fixtures.py asserts that the quad holds the footprint box wherever an image is compared"""
    i = np.arange(BIN_CHUNK)
    a = rect_rows(0, i % 32, 47, i % 32)
    if extra:
        a[512] = (20, 11, 26, 17)
    tx0, ty0 = (7 * i) % 47, (11 * i) % 31
    b = rect_rows(tx0, ty0, tx0 + i % 2, ty0 + i % 2)
    return make("heavy_edge_%d" % (49153 if extra else 49152), np.concatenate([a, b]), 1536, 1024, 40 + int(extra),
                "the heavy threshold is > 49152", logit=-1.5)


HEAVY_PARTS_SHAPES = {1: (32, 1600), 7: (224, 256), 8: (256, 256), 9: (288, 256), 256: (8192, 64)}


@functools.lru_cache(maxsize=None)
def heavy_parts(tiles_x):
    """a chunk above the threshold and a light one at tiles_x = 1 (cpp = 1: parts 1 ... 7 own no column), 7 (part 7 owns none), 8, 9
    (cpp = 2: parts 5 ... 7 own none, part 4 one column) and 256 (cpp = 32).  Most rectangles span the screen; every eighth starts
    at column rank mod tiles_x and every fifth lacks the last row, so that a part sees rectangles that end inside it, start inside
    it or miss it"""
    W, H = HEAVY_PARTS_SHAPES[tiles_x]
    ty = H // BIN
    i = np.arange(BIN_CHUNK)
    a = rect_rows(np.where(i % 8 == 3, i % tiles_x, 0), 0, tiles_x - 1, np.where(i % 5 == 2, ty - 2, ty - 1))
    b = rect_rows(i % tiles_x, i % ty, i % tiles_x, i % ty)[:300]
    cpp = -(-tiles_x // HEAVY_PARTS)
    return make("heavy_parts_%d" % tiles_x, np.concatenate([a, b]), W, H, 50 + tiles_x, "column blocks of a split chunk",
                logit=8.0, cpp=cpp, parts_with_columns=-(-tiles_x // cpp))


SLOTS_N = 130 * BIN_CHUNK                 # 133 120
SLOTS_NEAR = (924, 100)                   # the nearest splats: 924 from depth 8, then 100 from 8.5; the others from 17
SLOTS_VIEWS = {"many": (0.1, 64.0), "one": (0.1, 16.0), "light": (near_for(8.36, 16.0), 16.0)}


def heavy_slots_depth():
    n1, n2 = SLOTS_NEAR
    d = np.concatenate([descending_depths(SLOTS_N - n1 - n2, 17.0), descending_depths(n2, 8.5), descending_depths(n1, 8.0)])
    assert d[0] < 50.0
    return d


@functools.lru_cache(maxsize=1)
def heavy_slots():
    """224 x 224 px (7 x 7 bins): 133 120 nearly opaque full-screen splats = 130 chunks of 50 176 pairs, about 6.5 M pairs, in the
    view "many" (zf = 64).  "one" (zf = 16): the 132 096 splats beyond depth 17 are rejected (ranked, kRectEmpty), chunk 129 is
    the one heavy chunk.  "light" (zf = 16 and a near plane whose ndc.z = 0.25 rejection ends at depth 8.36): of chunk 129 only
    the 100 splats at depth 8.5 are drawn, 4900 pairs, nothing heavy"""
    r = rect_rows(0, 0, 6, 6)
    r = np.repeat(r, SLOTS_N, axis=0)
    return make("heavy_slots", r, 224, 224, 60, "more heavy chunks than helper slots; helpers without a heavy chunk",
                logit=8.0, depth=heavy_slots_depth())


@functools.lru_cache(maxsize=3)
def heavy_slots_view(which):
    """(view, the designed rectangles, claims) of heavy_slots() in the view `which`"""
    case = heavy_slots()
    zn, zf = SLOTS_VIEWS[which]
    v = view(224, 224, zn, zf)
    r = view_rects(case, heavy_slots_depth(), zn, zf)
    return v, r, claims_of(r, v, which)


GROUPS_V = (32 * 1024 - 1, 32 * 1024 + 1, 128 * 1024 - 1, 128 * 1024 + 1, 129 * 1024 + 5)


@functools.lru_cache(maxsize=2)
def one_column_groups(V, col):
    """V single-bin rectangles in column `col` (0 or 255) of the 8192 x 64 strip: every pair on ONE digit of the column pass, whose
    tables have 32 / 33, 128 / 129 and 130 chunk rows -- a group, a supergroup, and the 1 to 3 row tails of coop_row_sum"""
    i = np.arange(V)
    ty = (i // 3) % 2
    return make("one_column_%d_col%d" % (V, col), rect_rows(col, ty, col, ty), 8192, 64, 70 + col, "one table column carries every pair", logit=8.0)


# ---- row pass --------------------------------------------------------------------------------------------------------------

ONE_ROW_D = (4095, 4096, 4097, 32 * 4096 - 1, 32 * 4096 + 1, 128 * 4096 - 1, 128 * 4096 + 1)


@functools.lru_cache(maxsize=2)
def one_row(D):
    """8192 x 32 px (256 x 1 bins): every word carries row 0, the row pass is a pure stable copy of D words -- D // 256 rectangles
    over the whole strip behind one of D % 256 columns that ends at column 255"""
    rem = D % 256
    r = rect_rows(0, 0, 255, 0)
    r = np.repeat(r, D // 256, axis=0)
    if rem:
        r = np.concatenate([r, rect_rows(256 - rem, 0, 255, 0)])
    return make("one_row_%d" % D, r, 8192, 32, 80, "one digit in the row pass, chunk and group edges", logit=8.0)


ONE_BIN_V = (1, 4096, 4097, 70000)


@functools.lru_cache(maxsize=2)
def one_bin(V):
    """32 x 32 px, V splats on the one bin: one list of V entries (above the 4080-entry clamp of the heaviest-first order from
    4096, above 65 535 at 70 000)"""
    r = np.repeat(rect_rows(0, 0, 0, 0), V, axis=0)
    return make("one_bin_%d" % V, r, 32, 32, 90, "one list", logit=-3.0 if V == 4097 else 8.0)


SPARSE = ("one_each", "ends", "col_4095", "col_4096", "col_4097", "span4", "span5")


def columns_case(name, cols, counts, reaches, seed, logit=8.0):
    """single-bin rectangles on 8192 x 32 px: counts[k] of them in column cols[k], dealt round-robin over the ranks"""
    cols, counts = np.asarray(cols), np.asarray(counts)
    tx = np.repeat(cols, counts)
    tx = tx[np.argsort(np.concatenate([np.arange(c) for c in counts]), kind="stable")]
    return make(name, rect_rows(tx, 0, tx, 0), 8192, 32, seed, reaches, logit=logit)


@functools.lru_cache(maxsize=None)
def sparse_columns(variant):
    """8192 x 32 px (256 x 1 bins).  one_each: one pair in each of the 256 columns (in a scrambled order), every column shorter than a
    wave's share; ends: 3000 pairs each in columns 0 and 255, 254 empty columns between them (the walk of the downsweep iterates
    255 times, the upsweep counts column 255 with global atomics); col_L: columns 0, 7 and 255 of exactly L words, a column boundary
    one word before, on and one word after a chunk boundary; span4 / span5: chunks of 4096 words that span exactly four / five columns"""
    if variant == "one_each":
        tx = (np.arange(256) * 37) % 256
        return make("sparse_one_each", rect_rows(tx, 0, tx, 0), 8192, 32, 100, "columns shorter than a wave's words", logit=-0.5)
    if variant == "ends":
        return columns_case("sparse_ends", [0, 255], [3000, 3000], "empty columns between occupied ones", 101)
    if variant.startswith("col_"):
        L = int(variant[4:])
        return columns_case("sparse_" + variant, [0, 7, 255], [L, L, L], "a column boundary at a chunk boundary", 102)
    if variant == "span4":
        return columns_case("sparse_span4", [0, 1, 2, 3, 4, 5, 6, 7], [1000, 1000, 1000, 1096] * 2, "chunks that span exactly 4 columns", 103)
    assert variant == "span5"
    return columns_case("sparse_span5", [0, 1, 2, 3, 4, 10, 20, 21, 22, 200], [800, 800, 800, 800, 896] * 2,
                        "chunks that span exactly 5 columns: the kPairCols edge", 104)


@functools.lru_cache(maxsize=None)
def tall_weights():
    """32 x 8192 px (1 x 256 bins): 100 consecutive ranks of 1 x 256 rectangles (weight 256 = bit 8 on every lane of a ballot), then
    100 rectangles in row 255 only and 100 in row 0 only"""
    r = np.concatenate([np.repeat(rect_rows(0, 0, 0, 255), 100, axis=0), np.repeat(rect_rows(0, 255, 0, 255), 100, axis=0),
                        np.repeat(rect_rows(0, 0, 0, 0), 100, axis=0)])
    return make("tall_weights", r, 32, 8192, 110, "nine bit planes of the weight", logit=-3.0)


# ---- capacity edge ---------------------------------------------------------------------------------------------------------

CAP_FAR = 300                             # ranks 0 ... 299 lie at depth 9 and beyond, the others from depth 8


def cap_edge_depth(n):
    return np.concatenate([descending_depths(CAP_FAR, 9.0), descending_depths(n - CAP_FAR, 8.0)])


@functools.lru_cache(maxsize=None)
def cap_edge():
    """64 x 416 px (2 x 13 bins): 600 rectangles of 1 to 5 rows in either column and a LAST one of 2 x 13 bins, whose second column
    ends the pair array: with a capacity of D - 1 that item straddles the cap (pos + rows > cap: the guarded stores)"""
    i = np.arange(600)
    h, tx = 1 + (7 * i) % 5, (i // 3) % 2
    ty0 = (3 * i) % (14 - h)
    r = np.concatenate([rect_rows(tx, ty0, tx, ty0 + h - 1), rect_rows(0, 0, 1, 12)])
    return make("cap_edge", r, 64, 416, 120, "pos + rows > cap", depth=cap_edge_depth(601))


def cap_edge_small_view():
    """(view, rectangles) of cap_edge() with the near plane's rejection at depth 8.5: only ranks 0 ... 299 are drawn"""
    zn = near_for(8.5, 64.0)
    return view(64, 416, zn, 64.0), view_rects(cap_edge(), cap_edge_depth(601), zn, 64.0)
