"""CPU check of the inputs of tests/test_gpu_sort_limits.py: every case of tests/sort_limit_cases.py has exactly the keys, the
visible set, the bit length B, the visible count and the per-chunk digit occupancy it was designed for.  Oracle only -- if a
helper or a seed changes so that a case stops reaching its limit (a chunk on one digit, a digit width, a count at a chunk edge),
this fails without a GPU.  The oracle's own sort is checked on every case against numpy.argsort(kind="stable").

Measured, the rendered all-equal plane (-rP prints it): the tiled front-to-back renderer against the back-to-front oracle, 256 x 192:
100 % of values within 1e-4, mean |diff| 9.3e-6, max 6.2e-5 -- inside check_image's caps without the flip budget."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import sort_limit_cases as slc
from tests.checks import TIGHT, check_image


def digit_range(p, B):
    """(shift, bits) of pass p of the three-pass sort for keys whose largest quantised depth has B bits: ws_digit_range
    (msplat_sort.hip.h) restated -- 10 bits, then max(B - 10, 16) bits split in two, the larger half first"""
    if p == 0:
        return 0, 10
    rem = max(B - 10, 16)
    b1 = (rem + 1) >> 1
    return (10, b1) if p == 1 else (10 + b1, rem - b1)


WIDTHS = {B: (digit_range(1, B)[1], digit_range(2, B)[1]) for B in range(0, 33)}


def test_the_digit_widths():
    assert [WIDTHS[B] for B in range(26, 33)] == [(8, 8), (9, 8), (9, 9), (10, 9), (10, 10), (11, 10), (11, 11)]
    assert all(WIDTHS[B] == (8, 8) for B in range(0, 27))
    for B in range(0, 33):
        assert 10 + sum(WIDTHS[B]) >= B and digit_range(2, B)[0] + digit_range(2, B)[1] <= 32


def chunk_digits(q, C, B):
    """per pass: the number of non-empty digits of every chunk that holds a key.  Pass 0 walks the cloud (a chunk = C upload
    positions, culled ones included), passes 1 and 2 the visible keys in the order the pass before left them"""
    pos = np.flatnonzero(q > 0)
    seq = (0xFFFFFFFF - q[pos]).astype(np.uint32)
    out = []
    for p in range(3):
        shift, bits = digit_range(p, B)
        d = ((seq >> np.uint32(shift)) & np.uint32((1 << bits) - 1)).astype(np.int64)
        chunk = (pos if p == 0 else np.arange(seq.size)) // C
        occupied = np.unique(chunk * 2048 + d) // 2048
        out.append(np.bincount(occupied)[np.unique(occupied)])
        seq = seq[np.argsort(d, kind="stable")]
    return out


def presorted(case, cloud, view=None, q=None):
    """oracle.presort of the case (or of its second view) is exactly the design; returns (keys, idx)"""
    cam, proj, vp, nf = case.view if view is None else view
    q = case.q if q is None else q
    keys, idx = orc.presort(cloud.as_array(), orc.mat4_mul(proj, orc.mat4_inverse(cam)), nf[1])
    vis = np.flatnonzero(q > 0)
    np.testing.assert_array_equal(idx, vis)
    np.testing.assert_array_equal(keys, (0xFFFFFFFF - q[vis]).astype(np.uint32))
    return keys, idx


def check_case(case, cloud=None):
    cloud = slc.cloud_of(case) if cloud is None else cloud
    keys, idx = presorted(case, cloud)
    V, B = case.claims["V"], case.claims["B"]
    assert keys.size == V
    assert B == (int((~keys).max()).bit_length() if V else 0)
    skeys, sidx = orc.sort(keys, idx)
    perm = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(skeys, keys[perm])
    np.testing.assert_array_equal(sidx, idx[perm])
    order = case.claims["order"]
    if order is not None:
        want = {"identity": idx, "reversed": idx[::-1], "evens_then_odds": np.concatenate([idx[0::2], idx[1::2]])}[order]
        np.testing.assert_array_equal(sidx, want)
    occupancy = None
    if case.claims["digits"] is not None:
        occupancy = chunk_digits(case.q, case.C, B)
        for p, (lo, hi) in case.claims["digits"].items():
            assert occupancy[p].size > 0 and occupancy[p].min() >= lo and occupancy[p].max() <= hi, (p, occupancy[p])
    return keys, occupancy


@pytest.mark.parametrize("C", [4096, 2048])
@pytest.mark.parametrize("name", slc.SMALL_NAMES)
def test_small_cases_are_what_they_claim(name, C):
    case = slc.small_case(C, name)
    N, V, B = case.q.size, case.claims["V"], case.claims["B"]
    assert N < slc.SPATIAL_MIN
    keys, occupancy = check_case(case)
    print("%s, C = %d: N %d, V %d, B %d (digits 10 + %d + %d), distinct keys %d%s" % (
        name, C, N, V, B, WIDTHS[B][0], WIDTHS[B][1], np.unique(keys).size,
        "" if occupancy is None else ", digits per chunk %s" % [(int(o.min()), int(o.max())) for o in occupancy]))
    if name == "one_key" or name.startswith("groups_one_key"):
        assert np.unique(keys).size == 1 and V == N
    if name == "one_key":
        assert N == 3 * C + 1
    if name.startswith(("one_digit", "two_keys")):
        assert B == int(name[-2:])
        p = int(name[name.index("_p") + 2])
        shift, bits = digit_range(p, B)
        mask = np.uint32(((1 << bits) - 1) << shift)
        assert np.unique(keys & ~mask).size == 1 and np.unique(keys & mask).size >= 2      # the keys differ in that pass's digit only
        if name.startswith("two_keys"):
            assert np.unique(keys).size == 2 and (keys[0::2] == keys[0]).all() and (keys[1::2] == keys[1]).all() and keys[0] < keys[1]
    if name in ("ascending", "descending"):
        assert N == V == 5 * C
        d = np.diff(case.q.astype(np.int64))
        assert (d > 0).all() if name == "ascending" else (d < 0).all()
    if name.startswith("width_"):
        assert B == int(name[6:])
        q = case.q[case.q > 0]
        assert V == N and q.max() == ((1 << 24) - 1) << (B - 24) and q.min() == 3 << (B - 24)
    if name == "saturated":
        zf, z = case.view[3][1], -case.attrs["xyz"][:, 2].astype(np.float64)
        sat = case.q == slc.SAT
        assert B == 32 and V == N and (keys == 0).sum() == sat.sum() >= 1000 and (~sat).sum() >= 1000
        assert (z == zf).sum() == 50 and (z == 3 * zf).sum() == 50 and (z[sat] >= zf).all() and (z[~sat] < zf).all()
        assert case.q[~sat].max() == ((1 << 22) - 1) << 10                                  # the ordinary keys alone have B = 32 too
    if name.startswith("edge_"):
        v, place, delta = name[6:].split("_")[0], name.split("_")[2], int(name[name.index("_N") + 2:])
        assert V == {"1": 1, "C-1": C - 1, "C": C, "C+1": C + 1, "2C": 2 * C, "16C": 16 * C, "16C+1": 16 * C + 1, "17C": 17 * C}[v]
        assert N % C == delta % C
        vis = case.q > 0
        first, last = np.flatnonzero(vis)[[0, -1]]
        if place == "front":
            assert first == N - V and first >= 2 * C
        elif place == "alternate":
            assert not (vis[:-1] & vis[1:]).any() and first == 0
        elif place == "middle":
            per_chunk = np.add.reduceat(vis, np.arange(0, N, C))
            gap = np.flatnonzero(per_chunk == 0)
            assert gap.size >= 2 and gap[1] == gap[0] + 1 and gap[0] > 0 and per_chunk[:gap[0]].all()
            assert per_chunk[gap[0] + 2:].sum() == V - per_chunk[:gap[0]].sum() > 0
        else:
            assert first == last == (0 if place == "first" else N - 1)
    if name.startswith("groups_"):
        assert N == V == ((16 * C, 16 * C + 1, 32 * C + 1)[int(name[-1])])


def test_the_small_cases_cover_what_the_sort_can_choose():
    """every digit width, B controlled; every V and every placement of the edge cases at N = k C - 1, k C and k C + 1"""
    got = {slc.small_case(2048, "width_%d" % B).claims["B"] for B in range(24, 33)}
    assert {WIDTHS[B] for B in got} == {WIDTHS[B] for B in range(0, 33)} and len({WIDTHS[B] for B in got}) == 7
    combos = slc.edge_combos()
    for place in slc.EDGE_PLACES:
        assert {d for v, p, d in combos if p == place} == {-1, 0, 1}
        assert {v for v, p, d in combos if p == place} == set(slc.EDGE_V)
    assert {(p, d) for v, p, d in combos if v == "1"} == {(p, d) for p in ("first", "last") for d in (-1, 0, 1)}


@pytest.mark.parametrize("name", sorted(slc.LARGE))
def test_large_cases_are_what_they_claim(name):
    case = slc.large_case(name)
    n, C = slc.LARGE[name]
    cloud = slc.cloud_of(case)
    keys, _ = check_case(case, cloud)
    assert case.q.size == n == case.claims["V"] >= slc.SPATIAL_MIN and case.claims["B"] == 32
    if name.startswith("table_switch"):
        assert -(-n // 2048) == (512 if name.endswith("512_rows") else 513)
    else:
        assert (n > 2097152) == (C == 8192)
        nview, nq = slc.narrow(case)
        nkeys, _ = presorted(case, cloud, nview, nq)
        V2 = nkeys.size
        print("%s: the narrow view sees %d of %d" % (name, V2, n))
        assert 0 < V2 and V2 + V2 // 4 <= 2097152            # passes 1 and 2 of the frame after it take 4096-key chunks
        assert np.unique(keys).size == (1 if name.endswith("one_key") else n)


@pytest.mark.parametrize("kind", ["random", "one_key"])
def test_grid_cap_cases_are_what_they_claim(kind):
    case = slc.grid_cap_case(kind)
    cloud = slc.cloud_of(case)
    check_case(case, cloud)
    assert case.q.size == 40 * 4096 + 77 == case.claims["V"]
    nview, nq = slc.narrow(case)
    nkeys, _ = presorted(case, cloud, nview, nq)
    assert 0.5 * case.q.size < nkeys.size < 0.7 * case.q.size


def test_nothing_is_visible_from_the_view_that_looks_away():
    case = slc.small_case(2048, "width_32")
    cam, proj, vp, nf = slc.away_view()
    keys, idx = orc.presort(slc.cloud_of(case).as_array(), orc.mat4_mul(proj, orc.mat4_inverse(cam)), nf[1])
    assert keys.size == 0


def test_the_plane_is_one_key_and_the_tiled_renderer_meets_the_caps():
    """the all-equal plane: one key, drawn in upload order; an implementation that composites front to back with early
    termination, tile by tile, meets check_image's caps against the back-to-front oracle on this frame"""
    case = slc.plane_case()
    cloud = slc.cloud_of(case)
    keys, _ = check_case(case, cloud)
    assert np.unique(keys).size == 1 and keys.size == slc.PLANE_N
    cam, proj, vp, nf = case.view
    aos = cloud.as_array()
    ref = orc.render_frame(aos, False, cam, proj, vp, nf, nthreads=8, want_image=False, want_splats=True)
    np.testing.assert_array_equal(ref["sorted_idx"], np.arange(slc.PLANE_N))
    image, budget = orc.composite_flip(ref["splats"], slc.W, slc.H, nthreads=8)
    tiled = orc.render_frame_tiled(aos, False, cam, proj, vp, nf, nthreads=8)
    d = np.abs(tiled["image"].astype(np.float64) - image)[..., :3]
    covered = (image[..., :3] != 0).any(axis=-1).mean()
    print("plane: tiled front-to-back vs back-to-front oracle: within 1e-4 %.5f, mean %.3g, max %.3g; pixels drawn %.3f"
          % ((d <= 1e-4).mean(), d.mean(), d.max(), covered))
    assert covered > 0.25
    check_image(tiled["image"], image, budget=budget)
    assert d.max() <= TIGHT
