"""CPU check of the inputs of tests/test_gpu_binning_limits.py: every case of tests/binning_limit_cases.py has exactly the
rectangles it was designed for -- taken from the oracle's projection as _check_projection bounds the library's (oracle_rects) --,
keeps its 2 px from every bin border, holds its centres to 1e-3 px, and has the M and pairs per column-pass chunk, the D and
the words per bin column and row it claims.  Oracle only: if a helper, a seed or a constant changes so that a case stops reaching
its branch, this fails without a GPU.

The expected lists are binning_limit_cases.model_lists (np.repeat over the rectangles, one stable sort by bin).  `staged` below
restates the SAME result the way the library gets it -- two stable partitions over 1024-rank and 4096-word chunks -- and must equal
the model on every case; on the small cases both equal gpu_harness._expected_tile_lists.  A case names the mistake it exists to
catch (MISTAKES); a mistake is a few lines of numpy inside `staged`, and the case's output must change under it.  That is the
proof that the cases discriminate: deliberately broken GPU builds are not run, because a broken partition turns a count into
an address.  The random cloud of test_gpu_parity.py::test_tile_lists_exact does not notice eleven of the mistakes.

Cases that bracket a threshold from the harmless side are asserted NOT to change (owner_edge M8191 / M8192, thin_chunks 0, 255 and 256,
heavy_edge 49153 under ">=", the -1 sizes of the group edges, sparse col_4096, span4): they exist so that the threshold is
met from both sides.  "a part's column range is one too wide" is not among the mistakes: both parts then write the same words to
the same places, which changes nothing; the range one too NARROW is.

Measured (-rP prints it), the tiled front-to-back renderer against the back-to-front oracle on the image-checked cases: 100 % of
values within 1e-4 on all six; max |diff| 3.3e-5 and mean 1.6e-5 on one_bin_4097, max 1.0e-6 on tall_weights, 4.8e-7 on both
heavy_edge frames, 3.0e-7 on store_shapes, 3.0e-8 on sparse_one_each -- inside check_image's caps without the flip budget.  That
comparison shares the reference's 3.5-sigma quad with the oracle, so tiled_meets_the_caps also asserts that the quad holds every
footprint box (binning_limit_cases.heavy_edge says why)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import binning_limit_cases as blc
from tests import scenes
from tests.checks import TIGHT, check_image
from tests.gpu_harness import _expected_tile_lists
from tests.render_cases import oracle_rects

E = np.array(blc.EMPTY, np.int64)


# ---- the library's way to the same lists, with room for mistakes ---------------------------------------------------------------

MISTAKES = {
    "owner_first": "the owner search picks the first, not the last, of equal offsets: an item lands in the EMPTY rectangle before it",
    "per_wave_down": "per_wave is rounded down to a multiple of 64: the items beyond 4 per_wave are never ranked",
    "eight_planes": "eight weight bit planes instead of nine: a 256-row item weighs 0 and the column's next item lands on its words",
    "head_wrong_row": "the one-word head of the emit (odd position) writes the next row",
    "tail_wrong_row": "the one-word tail of the emit (last word at an even position) writes the row before",
    "heavy_ge": "the heavy threshold is >= 49152",
    "part_narrow": "a part's column range is one too narrow: its last column is never written",
    "unslotted_dropped": "a heavy chunk that gets no helper slot is flagged as split all the same: only its first column block is written",
    "group_edge_32": "column pass: the chunk row that starts a group misses the row before it in its prefix",
    "group_edge_128": "column pass: the chunk row that starts a supergroup misses the row before it in its prefix",
    "row_group_edge_32": "row pass: the chunk row that starts a group misses the row before it in its prefix",
    "row_group_edge_128": "row pass: the chunk row that starts a supergroup misses the row before it in its prefix",
    "wave_first_col": "column recovery stops at the wave's first column",
    "cols_beyond_fourth": "counts beyond the fourth column of a chunk are dropped",
    "len16": "a list length is kept in 16 bits",
    "order_unclamped": "the heaviest-first bucket 255 - (len >> 4) is not clamped at 4080 entries",
}


def shifted(chunk, digit, ndig, every):
    """how far the words of (chunk, digit) land too early when the first chunk row of every `every`-th misses the row before it"""
    nch = int(chunk.max()) + 1 if chunk.size else 0
    cnt = np.bincount(chunk * ndig + digit, minlength=nch * ndig).reshape(nch, ndig)
    short = np.zeros_like(cnt)
    for c in range(every, nch, every):
        short[c:] += cnt[c - 1]                       # every later row sums the same group totals
    return short[chunk, digit]


def overwrite(pos, chunk, D):
    """the source index of the word every position holds after each word went to pos (later chunks win); -1: nobody wrote it"""
    o = np.argsort(chunk, kind="stable")
    src = np.full(D, -1, np.int64)
    src[pos[o]] = o
    return src


def staged(rects, tiles_x, tiles_y, mistake=None, slots=blc.HEAVY_CAP):
    """(tile_start, words, heavy chunks, heaviest-first bucket per bin) as bin1_* and radix_*<MODE_PAIR> arrive at them"""
    r = np.array(rects, np.int64).reshape(-1, 4)
    n = r.shape[0]
    i = np.arange(n)
    chunk = i // blc.BIN_CHUNK
    nch = -(-n // blc.BIN_CHUNK)
    drawn = r[:, 0] <= r[:, 2]
    w = np.where(drawn, r[:, 2] - r[:, 0] + 1, 0)
    h = np.where(drawn, r[:, 3] - r[:, 1] + 1, 0)
    M = np.bincount(chunk, weights=w, minlength=nch).astype(np.int64)
    P = np.bincount(chunk, weights=w * h, minlength=nch).astype(np.int64)
    is_heavy = P >= blc.HEAVY_PAIRS if mistake == "heavy_ge" else P > blc.HEAVY_PAIRS
    if mistake == "owner_first":
        r[(M[chunk] > blc.OWNER_CAP) & drawn & np.r_[False, ~drawn[:-1]] & (i % blc.BIN_CHUNK != 0)] = E
    if mistake == "per_wave_down":
        first_item = np.cumsum(w) - w - np.r_[0, np.cumsum(M)][chunk]
        r[drawn & (first_item + w > 4 * (((M + 3) >> 2) & ~63)[chunk])] = E
    if mistake == "eight_planes":
        same = np.r_[(r[1:, 0] == r[:-1, 0]) & (r[1:, 2] == r[:-1, 2]) & (chunk[1:] == chunk[:-1]), False]
        r[(h == 256) & same] = E
    rank, tx, ty = blc.pairs_of(r)
    ch = rank // blc.BIN_CHUNK
    cpp = -(-tiles_x // blc.HEAVY_PARTS)
    split = is_heavy & (np.cumsum(is_heavy) <= slots)
    if mistake == "part_narrow":
        keep = ~(split[ch] & (tx % cpp == cpp - 1))
        rank, tx, ty, ch = rank[keep], tx[keep], ty[keep], ch[keep]
    if mistake == "unslotted_dropped":
        keep = ~((is_heavy & ~split)[ch] & (tx >= cpp))
        rank, tx, ty, ch = rank[keep], tx[keep], ty[keep], ch[keep]
    # column pass: a stable partition by column; position p of its output is the index here
    o = np.argsort(tx, kind="stable")
    rank, tx, ty, ch = rank[o], tx[o], ty[o], ch[o]
    D = rank.size
    p = np.arange(D)
    if mistake in ("group_edge_32", "group_edge_128"):
        src = overwrite(p - shifted(ch, tx, tiles_x, int(mistake[11:])), ch, D)
        held = src >= 0                                 # (a position's column follows from the column totals; stale words are dropped)
        rank, ty, tx = rank[src[held]], ty[src[held]], tx[held]
        D = rank.size
        p = np.arange(D)
    first = np.r_[True, (rank[1:] != rank[:-1]) | (tx[1:] != tx[:-1])] if D else np.zeros(0, bool)
    last = np.r_[first[1:], True] if D else first
    if mistake == "head_wrong_row":
        sel = first & (p % 2 == 1) & (ty + 1 < tiles_y)
        ty = np.where(sel, ty + 1, ty)
    if mistake == "tail_wrong_row":
        sel = last & (p % 2 == 0) & (ty > 0)
        ty = np.where(sel, ty - 1, ty)
    # row pass: a stable partition by row over chunks of 4096 words; the column comes back from the position
    counted = np.ones(D, bool)
    if mistake == "cols_beyond_fourth":
        counted = tx - tx[(p // blc.PAIR_CHUNK) * blc.PAIR_CHUNK] < blc.PAIR_COLS
    txw = tx[(p // blc.WAVE_WORDS) * blc.WAVE_WORDS] if mistake == "wave_first_col" else tx
    word = (txw << 24) | rank
    b = ty * tiles_x + tx
    o = np.argsort(ty, kind="stable")
    if mistake in ("row_group_edge_32", "row_group_edge_128"):
        rowpos = np.empty(D, np.int64)
        rowpos[o] = p
        src = overwrite(rowpos - shifted(p // blc.PAIR_CHUNK, ty, tiles_y, int(mistake[15:])), p // blc.PAIR_CHUNK, D)
        words = word[src[src >= 0]]
    else:
        words = word[o]
    cnt = np.bincount(b[counted], minlength=tiles_x * tiles_y)
    if mistake == "len16":
        cnt = cnt & 0xFFFF
    start = np.zeros(tiles_x * tiles_y + 1, np.int64)
    np.cumsum(cnt, out=start[1:])
    bucket = 255 - (cnt >> 4) if mistake == "order_unclamped" else 255 - np.minimum(cnt >> 4, 255)
    return start.astype(np.uint32), words.astype(np.uint32), int(is_heavy.sum()), bucket


def differs(a, b):
    return any(np.shape(x) != np.shape(y) or not np.array_equal(x, y) for x, y in zip(a, b))


def assert_catches(rects, v, mistakes, brackets=(), **kw):
    tiles = blc.tiles_of(v)
    good = staged(rects, *tiles, **kw)
    want = blc.model_lists(rects, *tiles)
    np.testing.assert_array_equal(good[0], want[0])
    np.testing.assert_array_equal(good[1], want[1])
    for m in mistakes:
        assert m in MISTAKES and differs(staged(rects, *tiles, mistake=m, **kw), good), "%s goes unnoticed" % m
    for m in brackets:
        assert m in MISTAKES and not differs(staged(rects, *tiles, mistake=m, **kw), good), "%s is noticed from the harmless side" % m
    return good


# ---- the design, from the oracle's projection -------------------------------------------------------------------------------

def assert_design(case, v=None, rects=None, cloud=None):
    """the oracle ranks splat i as i, projects exactly the designed rectangles (EMPTY where nothing is drawn) with centres within
    1e-3 px of the design and footprint boxes 2 px inside the rectangles' borders; returns the oracle's rectangles as rows"""
    v = case.view if v is None else v
    rects = case.rects if rects is None else rects
    cam, proj, vp, nf = v
    W, H = vp[2], vp[3]
    aos = (blc.cloud_of(case) if cloud is None else cloud).as_array()
    ref = orc.render_frame(aos, False, cam, proj, vp, nf, nthreads=8, want_image=False, want_splats=True)
    n = rects.shape[0]
    assert ref["V"] == n                                                         # every splat passes the Sort's cull ...
    np.testing.assert_array_equal(ref["sorted_idx"], np.arange(n))               # ... and its rank is its upload index
    k = ref["sorted_keys"].astype(np.int64)
    assert (np.diff(k)[k[1:] != 0] > 0).all()                # distinct keys, but for the saturated ones beyond the far plane (key 0)
    sp = ref["splats"]
    drawn, tx0, ty0, tx1, ty1 = oracle_rects(sp, W, H)
    got = np.stack([tx0, ty0, tx1, ty1], axis=1)
    got[~drawn] = E
    np.testing.assert_array_equal(got, rects)
    d = rects[:, 0] <= rects[:, 2]
    np.testing.assert_array_equal(d, drawn)
    rho2 = 2.0 * np.log(256.0 * sp["alpha"][d].astype(np.float64))
    px, py = sp["px"][d].astype(np.float64), sp["py"][d].astype(np.float64)
    ex, ey = np.sqrt(rho2 * sp["cov"][d, 0]), np.sqrt(rho2 * sp["cov"][d, 3])
    r = rects[d]
    off = max(np.abs(px - 0.5 * blc.BIN * (r[:, 0] + r[:, 2] + 1)).max(), np.abs(py - 0.5 * blc.BIN * (r[:, 1] + r[:, 3] + 1)).max()) if d.any() else 0.0
    clear = min((px - ex - blc.BIN * r[:, 0]).min(), (blc.BIN * (r[:, 2] + 1) - px - ex).min(),
                (py - ey - blc.BIN * r[:, 1]).min(), (blc.BIN * (r[:, 3] + 1) - py - ey).min()) if d.any() else np.inf
    print("%s: %d splats, %d drawn, centres off by at most %.3g px, boxes at least %.3f px inside their rectangles" % (case.name, n, d.sum(), off, clear))
    assert off <= 1e-3 and clear >= 2.0
    assert ((sp["reject"][~d] != 0) | (sp["alpha"][~d] <= 1.0 / 256.0)).all()           # EMPTY: rejected by a plane, or too faint
    return got, ref


def assert_claims(case, got, v=None, claims=None):
    """the claims hold for the ORACLE's rectangles"""
    c = case.claims if claims is None else claims
    o = blc.claims_of(got, case.view if v is None else v, c["reaches"])
    for k in ("n", "D", "heavy"):
        assert o[k] == c[k], (k, o[k], c[k])
    for k in ("M", "pairs", "per_column", "per_row"):
        np.testing.assert_array_equal(o[k], c[k], err_msg=k)
    return c


def small_equal(rects, v):
    """the model against the Python loops of gpu_harness._expected_tile_lists"""
    tiles = blc.tiles_of(v)
    ts, words = blc.model_lists(rects, *tiles)
    exp = _expected_tile_lists(blc.pack(rects), *tiles)
    assert ts[-1] == sum(len(e) for e in exp) == words.size
    for t, e in enumerate(exp):
        assert (words[ts[t]:ts[t + 1]] & 0xFFFFFF).tolist() == e, "bin %d" % t
        assert (words[ts[t]:ts[t + 1]] >> 24 == t % tiles[0]).all()


def tiled_meets_the_caps(case, ref):
    cam, proj, vp, nf = case.view
    W, H = vp[2], vp[3]
    aos = blc.cloud_of(case).as_array()
    # the reference rasterises a splat inside its 3.5-sigma quad only, turned by theta = atan2(major - cov_xx, cov_xy): with
    # cov_xy ~ 1e-12 that angle is a quotient of rounding residues and the quad of a long splat can stand across it.  The tiled
    # renderer shares the quad with the oracle, so this comparison cannot see that; the library composites the footprint itself
    sp = ref["splats"][ref["splats"]["reject"] == 0]
    sp = sp[sp["alpha"] > 1.0 / 256.0]
    rho = np.sqrt(2.0 * np.log(256.0 * sp["alpha"].astype(np.float64)))
    assert (sp["hx"] >= rho * np.sqrt(sp["cov"][:, 0])).all() and (sp["hy"] >= rho * np.sqrt(sp["cov"][:, 3])).all(), \
        "%s: the oracle's quad cuts a footprint" % case.name
    image, budget = orc.composite_flip(ref["splats"], W, H, nthreads=8)
    tiled = orc.render_frame_tiled(aos, False, cam, proj, vp, nf, nthreads=8)
    d = np.abs(tiled["image"].astype(np.float64) - image)[..., :3]
    print("%s: tiled front-to-back vs back-to-front oracle: within 1e-4 %.5f, mean %.3g, max %.3g" % (case.name, (d <= 1e-4).mean(), d.mean(), d.max()))
    check_image(tiled["image"], image, budget=budget)
    assert d.max() <= TIGHT
    assert (image[..., :3] != 0).any()


# ---- column pass -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", blc.OWNER_EDGE)
def test_owner_edge(variant):
    case = blc.owner_edge(variant)
    got, _ = assert_design(case)
    c = assert_claims(case, got)
    assert c["n"] == 1024 and c["M"].size == 1
    if variant == "full":
        e = case.rects[:, 0] > case.rects[:, 2]
        assert e[0] and e[1023] and e[300:317].all() and c["M"][0] == 16 * (~e).sum() > blc.OWNER_CAP
        assert_catches(case.rects, case.view, ["owner_first"])
    else:
        assert c["M"][0] == int(variant[1:]) and (c["M"][0] > blc.OWNER_CAP) == (variant == "M8193")
        assert_catches(case.rects, case.view, ["owner_first"] if variant == "M8193" else [], [] if variant == "M8193" else ["owner_first"])
    small_equal(case.rects, case.view)


@pytest.mark.parametrize("m", blc.THIN_M)
def test_thin_chunks(m):
    case = blc.thin_chunks(m)
    got, _ = assert_design(case)
    c = assert_claims(case, got)
    assert c["M"].tolist() == [4096, m, 4096] and c["pairs"][1] >= m
    assert c["idle_waves"] == {0: 4, 1: 3, 63: 3, 64: 3, 65: 2, 255: 0, 256: 0, 257: 1}[m]
    bracket = m in (0, 255, 256)                      # ceil(m / 4) is a multiple of 64 there: rounding down changes nothing
    assert_catches(case.rects, case.view, [] if bracket else ["per_wave_down"], ["per_wave_down"] if bracket else [])
    small_equal(case.rects, case.view)


def test_store_shapes():
    case = blc.store_shapes()
    got, ref = assert_design(case)
    c = assert_claims(case, got)
    h = got[:, 3] - got[:, 1] + 1
    np.testing.assert_array_equal(c["pos"], np.cumsum(h) - h)                   # one column: pos is the running sum of the heights
    assert c["combos"] == {(a, rows) for a in range(4) for rows in range(1, 13)} and c["M"].size == 1
    assert_catches(case.rects, case.view, ["head_wrong_row", "tail_wrong_row"])
    small_equal(case.rects, case.view)
    tiled_meets_the_caps(case, ref)


@pytest.mark.parametrize("extra", [False, True])
def test_heavy_edge(extra):
    case = blc.heavy_edge(extra)
    got, ref = assert_design(case)
    c = assert_claims(case, got)
    assert c["pairs"][0] == blc.HEAVY_PAIRS + int(extra) and c["heavy"] == int(extra) and c["pairs"][1] < 4096
    good = assert_catches(case.rects, case.view, [] if extra else ["heavy_ge"], ["heavy_ge"] if extra else [])
    assert good[2] == int(extra)
    tiled_meets_the_caps(case, ref)


@pytest.mark.parametrize("tiles_x", sorted(blc.HEAVY_PARTS_SHAPES))
def test_heavy_parts(tiles_x):
    case = blc.heavy_parts(tiles_x)
    got, _ = assert_design(case)
    c = assert_claims(case, got)
    assert blc.tiles_of(case.view)[0] == tiles_x and c["pairs"][0] > blc.HEAVY_PAIRS > c["pairs"][1] and c["heavy"] == 1
    assert (c["cpp"], c["parts_with_columns"]) == {1: (1, 1), 7: (1, 7), 8: (1, 8), 9: (2, 5), 256: (32, 8)}[tiles_x]
    assert_catches(case.rects, case.view, ["part_narrow"])


def test_heavy_slots():
    case = blc.heavy_slots()
    cloud = blc.cloud_of(case)
    want = {"many": (130, blc.SLOTS_N * 49), "one": (1, 1024 * 49), "light": (0, 100 * 49)}
    for which in ("light", "one", "many"):
        v, rects, claims = blc.heavy_slots_view(which)
        got, _ = assert_design(case, v, rects, cloud)
        c = assert_claims(case, got, v, claims)
        assert (c["heavy"], c["D"]) == want[which] and c["M"].size == 130
    assert 130 > blc.HEAVY_CAP > 2 * 1 + 8
    assert_catches(rects, v, ["unslotted_dropped", "part_narrow"], slots=10)


@pytest.mark.parametrize("col", [0, 255])
@pytest.mark.parametrize("V", blc.GROUPS_V)
def test_one_column_groups(V, col):
    case = blc.one_column_groups(V, col)
    got, _ = assert_design(case)
    c = assert_claims(case, got)
    assert c["D"] == V and c["per_column"][col] == V and c["M"].size == -(-V // 1024)
    rows = c["M"].size
    edge = "group_edge_32" if rows <= 33 else "group_edge_128"
    after = rows % (32 if rows <= 33 else 128) in (1, 2)
    assert_catches(case.rects, case.view, [edge] if after else [], [] if after else [edge])


# ---- row pass --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", blc.ONE_ROW_D)
def test_one_row(D):
    case = blc.one_row(D)
    got, _ = assert_design(case)
    c = assert_claims(case, got)
    assert c["D"] == D and c["per_row"].tolist() == [D] and blc.tiles_of(case.view) == (256, 1)
    rows = -(-D // blc.PAIR_CHUNK)
    edge = {33: "row_group_edge_32", 129: "row_group_edge_128"}.get(rows)
    bracket = {32: "row_group_edge_32", 128: "row_group_edge_128"}.get(rows)
    # (at 524289 every column but the last holds 2048 words, two whole waves: there no wave crosses a column)
    wave = [] if D == 128 * 4096 + 1 else ["wave_first_col"]
    assert_catches(case.rects, case.view, wave + ([edge] if edge else []), [bracket] if bracket else [])


@pytest.mark.parametrize("V", blc.ONE_BIN_V)
def test_one_bin(V):
    case = blc.one_bin(V)
    got, ref = assert_design(case)
    c = assert_claims(case, got)
    assert c["D"] == V and c["per_column"].tolist() == [V]
    assert_catches(case.rects, case.view, (["order_unclamped"] if V >= 4096 else []) + (["len16"] if V > 65535 else []),
                   (["order_unclamped"] if V < 4096 else []) + (["len16"] if V <= 65535 else []))
    if V == 4097:
        tiled_meets_the_caps(case, ref)


@pytest.mark.parametrize("variant", blc.SPARSE)
def test_sparse_columns(variant):
    case = blc.sparse_columns(variant)
    got, ref = assert_design(case)
    c = assert_claims(case, got)
    pc = c["per_column"]
    _, tx, _ = blc.pairs_of(case.rects)
    tx = np.sort(tx)
    span = [np.unique(tx[k:k + blc.PAIR_CHUNK]).size for k in range(0, tx.size, blc.PAIR_CHUNK)]
    reach = [int(tx[k:k + blc.PAIR_CHUNK].max() - tx[k]) for k in range(0, tx.size, blc.PAIR_CHUNK)]
    if variant == "one_each":
        assert (pc == 1).all() and reach == [255]
        assert_catches(case.rects, case.view, ["wave_first_col", "cols_beyond_fourth"])
        small_equal(case.rects, case.view)
        tiled_meets_the_caps(case, ref)
    elif variant == "ends":
        assert pc[0] == pc[255] == 3000 and pc.sum() == 6000 and span == [2, 1] and reach == [255, 0]
        assert_catches(case.rects, case.view, ["wave_first_col", "cols_beyond_fourth"])
    elif variant.startswith("col_"):
        L = int(variant[4:])
        assert pc[0] == pc[7] == pc[255] == L and pc.sum() == 3 * L
        on_edge = L == blc.PAIR_CHUNK
        assert (max(span) == 1) == on_edge
        assert_catches(case.rects, case.view, [] if on_edge else ["wave_first_col"], ["wave_first_col"] if on_edge else [])
    else:
        k = int(variant[4:])
        assert span == [k, k] and pc.sum() == 2 * blc.PAIR_CHUNK and (min(reach) >= blc.PAIR_COLS) == (k == 5)
        assert_catches(case.rects, case.view, ["wave_first_col"] + (["cols_beyond_fourth"] if k == 5 else []), ["cols_beyond_fourth"] if k == 4 else [])


def test_tall_weights():
    case = blc.tall_weights()
    got, ref = assert_design(case)
    c = assert_claims(case, got)
    h = got[:, 3] - got[:, 1] + 1
    assert (h[:100] == 256).all() and (got[100:200, 1] == 255).all() and (got[200:, 3] == 0).all() and c["D"] == 25800
    assert c["per_row"][0] == c["per_row"][255] == 200 and (c["per_row"][1:255] == 100).all()
    assert_catches(case.rects, case.view, ["eight_planes"])
    small_equal(case.rects, case.view)
    tiled_meets_the_caps(case, ref)


# ---- capacity edge ---------------------------------------------------------------------------------------------------------

def test_cap_edge():
    case = blc.cap_edge()
    got, _ = assert_design(case)
    c = assert_claims(case, got)
    D = c["D"]
    assert 1000 < D < 10000 and tuple(got[-1]) == (0, 0, 1, 12)
    # the last item -- the last rectangle's column 1, the last column -- writes the words D - 13 ... D - 1: it straddles a cap of D - 1
    rank, tx, _ = blc.pairs_of(case.rects)
    o = np.argsort(tx, kind="stable")
    assert (rank[o][-13:] == 600).all() and (tx[o][-13:] == 1).all()
    for cap, over in ((D, False), (D - 1, True)):                      # the verdict is incl > cap; ">=" would refuse the exact fit
        assert (D > cap) == over and (D >= cap) is True
    small_equal(case.rects, case.view)
    v, rects = blc.cap_edge_small_view()
    got2, _ = assert_design(case, v, rects)
    assert 0 < blc.claims_of(got2, v, "")["D"] < D - 13 and (got2[blc.CAP_FAR:] == E).all()


# ---- what a random cloud does not notice -----------------------------------------------------------------------------------

def test_the_random_cloud_of_test_tile_lists_exact_misses_most_mistakes():
    """scenes.hard_attrs(2500, 5) at 640 x 360, the input of test_gpu_parity.py::test_tile_lists_exact: its rectangles (from the
    oracle) leave the lists unchanged under these mistakes, every one of which a designed case catches"""
    W, H = 640, 360
    cam, proj, vp, nf = scenes.default_view(W, H)
    aos = scenes.cloud_from_attrs(scenes.hard_attrs(2500, 5)).as_array()
    ref = orc.render_frame(aos, True, cam, proj, vp, nf, nthreads=8, want_image=False, want_splats=True)
    drawn, tx0, ty0, tx1, ty1 = oracle_rects(ref["splats"], W, H)
    rects = np.stack([tx0, ty0, tx1, ty1], axis=1)
    rects[~drawn] = E
    tiles = ((W + 31) // 32, (H + 31) // 32)
    good = staged(rects, *tiles)
    np.testing.assert_array_equal(good[1], blc.model_lists(rects, *tiles)[1])
    assert good[0][-1] > 10000
    blind = [m for m in MISTAKES if not differs(staged(rects, *tiles, mistake=m), good)]
    print("the random cloud (%d pairs) does not notice: %s" % (good[0][-1], ", ".join(blind)))
    for m in ("owner_first", "eight_planes", "heavy_ge", "part_narrow", "group_edge_32", "row_group_edge_32", "len16", "order_unclamped"):
        assert m in blind, m
    assert len(blind) >= 3
