"""The depth sort at its limits: skewed keys, digit and chunk edges, and its grid-stride loops.

The rest of the suite feeds the sort random clouds, whose keys spread evenly over every digit.  The cases of
tests/sort_limit_cases.py (designed keys; every claim asserted on the CPU by tests/test_sort_limits_fixtures.py) put a whole chunk,
or the whole cloud, on ONE digit -- a per-wave 16-bit packed rank counter of ws_downsweep then reaches 512 or 1024, the packed
per-wave bases reach CHUNK, a group-table row carries the whole cloud in one word --, make a pass a pure stable copy, feed sorted
and reversed input, choose every digit width of ws_digit_range (8 + 8 ... 11 + 11 bits, changing from frame to frame on one
context, with a frame that sees nothing in between), and place the visible count V and the cloud size N on chunk and group edges
(4096-key chunks for one frame at a time, 2048 for frames in flight, 8192 beyond 2 097 152 splats; groups of 16 chunk rows, of 32
beyond 512 rows).  MSPLAT_GRID_CAP = 1, 5, 8 makes the chunk loops of ws_upsweep / ws_downsweep (and of the 8-bit passes, the two
binning passes and the Morton sort at upload) take up to 40 and 80 turns at 164 k splats: the loop re-zeroes the packed counters,
its row-sum scratch aliases s_keys behind the loop's trailing barrier, and a grid of 8 takes the xcd_contiguous remap.

Every comparison is exact (sort_count, sorted_keys, sorted_indices against the oracle, ties in ascending upload index, tile lists
and pixels against the uncapped context bit for bit) except the image of the all-equal plane, which meets check_image's caps as
they are.  Forms: the default (512-thread workgroups), frame_mode = FRAMES_IN_FLIGHT (256 threads), MSPLAT_SORT=lsd8, lsd8 with
the ballot ranking, lsd8 with MSPLAT_SCAN_KERNELS=1.

Measured on the MI355X (-rP prints the image figures): the plane against the oracle, max |diff| 6.0e-4 in upload order and
1.5e-4 in storage order, mean 5.1e-7 / 2.2e-7, 99.999 % of values within 1e-4; the whole module runs in 10 s, its slowest test
(2 097 153 splats, four frames) in 0.7 s.

Not asserted, because the library reports neither: which grid a launch had (that the cap reaches the launches was seen once in the
stage times of the 164 k-splat random cloud: sort 50 us uncapped, 152 / 225 / 941 us with a cap of 8 / 5 / 1, binning 37 -> 238 /
368 / 1727 us), and that passes 1 and 2 of the frames after the narrow view of the 2 097 153-splat cloud ran on
4096-key chunks (the condition, an earlier frame's V + V / 4 <= 2 M, is asserted by the fixture module).

Deliberate breaks of ws_downsweep, tried once on scratch builds: packed counters read back with 10 bits fail the two
2 097 153-splat cases here and nothing in tests/test_gpu_parity.py; with 9 bits they fail 23 tests here (every one-digit case) and
the saturated and tiny-q cases of test_sort_exact_for_every_key_range.  A build WITHOUT the trailing barrier of the chunk loop still
passes everything, capped grids included: the next turn writes its row-sum scratch only after its global loads have returned, and
no wave was ever that far behind.  The loop's second turn is covered here; that barrier is not."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import SplatRenderer, _capi
from tests import scenes
from tests import sort_limit_cases as slc
from tests.checks import check_image
from tests.gpu_harness import _check_projection, _expected_tile_lists, oracle_frame

pytestmark = pytest.mark.gpu

# form -> (chunk of pass 0, SplatRenderer arguments, environment at msplat_create)
FORMS = {
    "default": (4096, {}, {}),
    "in_flight": (2048, {"frame_mode": _capi.FRAMES_IN_FLIGHT}, {}),
    "lsd8": (2048, {}, {"MSPLAT_SORT": "lsd8"}),
    "lsd8_ballot": (2048, {"rank_mode": _capi.RANK_BALLOT}, {"MSPLAT_SORT": "lsd8"}),
    "lsd8_scan": (2048, {}, {"MSPLAT_SORT": "lsd8", "MSPLAT_SCAN_KERNELS": "1"}),
}
ENV = ("MSPLAT_SORT", "MSPLAT_SCAN_KERNELS", "MSPLAT_GRID_CAP")


def renderer(cloud, form, monkeypatch, n, cap=None, **kw):
    """a context of the given form (the switches are read once, by msplat_create) holding the cloud in upload order"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    env = dict(FORMS[form][2])
    if cap is not None:
        env["MSPLAT_GRID_CAP"] = str(cap)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    args = dict(FORMS[form][1])
    if n >= slc.SPATIAL_MIN:
        args["spatial_order"] = _capi.SPATIAL_OFF          # Morton storage would undo the designed chunk contents
    args.update(kw)
    r = SplatRenderer(device=0, **args)
    ok = r.Init(cloud, False, False)
    for k in env:
        monkeypatch.delenv(k)
    assert ok, r.last_error()
    if args.get("spatial_order") != _capi.SPATIAL_ON:
        assert r.storage_order() is None
    return r


def oracle_sort(aos, view):
    cam, proj, vp, nf = view
    keys, idx = orc.sort(*orc.presort(aos, orc.mat4_mul(proj, orc.mat4_inverse(cam)), nf[1]))
    keys.setflags(write=False); idx.setflags(write=False)
    return keys, idx


def check_sort(r, want, what):
    keys, idx = want
    assert r.sort_count() == keys.size, what
    k, i = r.sorted_keys(), r.sorted_indices()
    np.testing.assert_array_equal(k, keys, err_msg=what)
    np.testing.assert_array_equal(i, idx, err_msg=what)
    tie = k[1:] == k[:-1]
    assert (i[1:][tie] > i[:-1][tie]).all(), what                # ties in ascending upload index
    return k, i


@functools.lru_cache(maxsize=4)
def small(C, name):
    """(case, its cloud, the oracle's sorted keys and permutation), computed once per chunk size"""
    case = slc.small_case(C, name)
    cloud = slc.cloud_of(case)
    return case, cloud, oracle_sort(cloud.as_array(), case.view)


# ------------------------------------------------------------------------------------------------
# 1. the named cases in every form of the sort
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", slc.SMALL_NAMES)
def test_small_cases_sort_exactly_in_every_form(name, monkeypatch):
    for form, (C, _, _) in FORMS.items():
        case, cloud, want = small(C, name)
        what = "%s, %s (C = %d, N = %d, V = %d, B = %d)" % (name, form, C, case.q.size, case.claims["V"], case.claims["B"])
        r = renderer(cloud, form, monkeypatch, case.q.size)
        for frame in range(2):                  # the second frame runs on the tables the first one left behind
            r.Sort(*case.view)
            check_sort(r, want, "%s frame %d" % (what, frame))
        r.Render(*case.view)
        assert r.verify_order() == (0, 0), what
        r.close()


# ------------------------------------------------------------------------------------------------
# 2. the digit width changes from frame to frame on one context
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["default", "in_flight"])
def test_the_digit_width_changes_from_frame_to_frame(form, monkeypatch):
    """one upload; B = 32, 26, 29, saturated, nothing visible, 27, 32: the histogram row stride is the digit count, the group
    tables are zeroed by the successor pass, the minimum key lives in two parity words"""
    C = FORMS[form][0]
    case = slc.width_case(C, 32)
    cloud = slc.cloud_of(case)
    aos = cloud.as_array()
    r = renderer(cloud, form, monkeypatch, case.q.size)
    for frame, B in enumerate((32, 26, 29, "saturated", None, 27, 32)):
        view = slc.away_view() if B is None else slc.width_case(C, B).view
        want = oracle_sort(aos, view)
        r.Sort(*view)
        k, _ = check_sort(r, want, "%s frame %d (B = %s)" % (form, frame, B))
        if B is None:
            assert k.size == 0
        elif B == "saturated":
            assert (k == 0).sum() >= 1000 and (k != 0).sum() >= 1000
        else:
            assert k.size == case.q.size and int(~k[0]).bit_length() == B
        r.Render(*view)
        assert r.verify_order() == (0, 0)
    r.close()


# ------------------------------------------------------------------------------------------------
# 3. the three cases above a million splats (SH0, sort only)
# ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def large(name):
    case = slc.large_case(name)
    cloud = slc.cloud_of(case)
    return case, cloud, cloud.as_array()


@pytest.mark.parametrize("form", ["in_flight", "lsd8"])
@pytest.mark.parametrize("name", ["table_switch_512_rows", "table_switch_513_rows"])
def test_group_table_switch_at_512_rows(name, form, monkeypatch):
    """1 048 576 and 1 048 577 splats with frames in flight: 512 rows of 2048 keys in groups of 16, 513 rows in groups of 32"""
    case, cloud, aos = large(name)
    want = oracle_sort(aos, case.view)
    r = renderer(cloud, form, monkeypatch, case.q.size)
    for frame in range(2):
        r.Sort(*case.view)
        check_sort(r, want, "%s %s frame %d" % (name, form, frame))
    assert r.verify_order()[0] == 0
    r.close()


@pytest.mark.parametrize("form", ["default", "lsd8"])
@pytest.mark.parametrize("name", ["items_switch_4096_descending", "items_switch_4096_one_key", "items_switch_8192_descending",
                                  "items_switch_8192_one_key"])
def test_chunk_size_switch_at_2097152_splats(name, form, monkeypatch):
    """2 097 152 splats: 512 chunks of 4096 keys; 2 097 153: 257 chunks of 8192.  On the larger cloud a frame from the narrow view
    (60 % visible) is rendered, which tells the host its V: passes 1 and 2 of the next frames then take 4096-key chunks, for the
    narrow view and again for the whole cloud"""
    case, cloud, aos = large(name)
    r = renderer(cloud, form, monkeypatch, case.q.size)
    want = oracle_sort(aos, case.view)
    r.Sort(*case.view)
    _, i = check_sort(r, want, "%s %s" % (name, form))
    np.testing.assert_array_equal(i, np.arange(case.q.size, dtype=np.uint32))        # already sorted: upload order
    if case.C == 8192:
        nview, nq = slc.narrow(case)
        nwant = oracle_sort(aos, nview)
        assert nwant[0].size == (nq > 0).sum()
        for frame, (view, w) in enumerate(((nview, nwant), (nview, nwant), (case.view, want))):
            r.Sort(*view)
            check_sort(r, w, "%s %s, frame %d after the switch" % (name, form, frame))
            if frame == 0:
                r.Render(*view)
    assert r.verify_order()[0] == 0
    r.close()


# ------------------------------------------------------------------------------------------------
# 4. the all-equal plane, rendered: the draw order is the tie rule alone
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spatial", [False, True])
def test_the_all_equal_plane_is_drawn_in_storage_order(spatial, monkeypatch):
    """20 000 translucent splats with ONE key at 256 x 192: image against the oracle (check_image's caps), rectangles and tile lists
    exact.  spatial: stored in Morton order (SPATIAL_ON) -- equal keys are drawn in ascending storage slot, so the oracle is fed
    the cloud in storage order (oracle_frame(r=...)) and the draw order is the storage order itself"""
    case = slc.plane_case()
    cloud = slc.cloud_of(case)
    cam, proj, vp, nf = case.view
    r = renderer(cloud, "default", monkeypatch, case.q.size, **({"spatial_order": _capi.SPATIAL_ON} if spatial else {}))
    order = r.storage_order()
    assert (order is not None) == spatial
    ref = oracle_frame(cloud.as_array(), False, cam, proj, vp, nf, r=r)
    r.Sort(*case.view)
    assert r.sort_count() == ref["V"] == slc.PLANE_N
    assert np.unique(r.sorted_keys()).size == 1
    np.testing.assert_array_equal(r.sorted_indices(), ref["sorted_idx"])
    np.testing.assert_array_equal(r.sorted_indices(), order if spatial else np.arange(slc.PLANE_N))
    img = r.Render(*case.view)
    d = np.abs(img[..., :3].astype(np.float64) - ref["image"][..., :3])
    print("plane, %s order: max |diff| %.3g, mean %.3g, within 1e-4: %.5f" % ("storage" if spatial else "upload", d.max(), d.mean(), (d <= 1e-4).mean()))
    check_image(img, ref["image"], budget=ref["budget"])
    assert (img[..., :3] != 0).any(axis=-1).mean() > 0.25
    rect = _check_projection(r, ref, slc.W, slc.H)
    st = r.stats()
    ts, pairs = r.debug_tile_lists()
    exp = _expected_tile_lists(rect, st["tiles_x"], st["tiles_y"])
    assert st["pairs"] == sum(len(e) for e in exp) == ts[-1]
    for t, e in enumerate(exp):
        assert (pairs[ts[t]:ts[t + 1]] & 0xFFFFFF).tolist() == e, "tile %d" % t
    assert r.verify_order() == (0, 0)
    r.close()


# ------------------------------------------------------------------------------------------------
# 5. MSPLAT_GRID_CAP: the grid-stride loops take several turns
# ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid_cap_frames(kind):
    """(cloud, [(view, oracle keys, oracle permutation)] of the three frames of a context)"""
    case = slc.grid_cap_case(kind)
    cloud = slc.cloud_of(case)
    aos = cloud.as_array()
    if kind == "hard":
        views = [scenes.default_view(slc.W, slc.H, yaw=yaw) for yaw in (0.0, 0.7)]
    else:
        views = [case.view, slc.narrow(case)[0]]
    sorts = [oracle_sort(aos, v) for v in views]
    assert 0 < sorts[1][0].size != sorts[0][0].size > 0           # the second frame has another V
    return cloud, [(views[j], sorts[j]) for j in (0, 1, 0)]


def three_frames(r, frames, what):
    out = []
    for f, (view, want) in enumerate(frames):
        r.Sort(*view)
        check_sort(r, want, "%s frame %d" % (what, f))
        img = r.Render(*view)
        ts, pairs = r.debug_tile_lists()
        assert r.verify_order() == (0, 0), what
        out.append((ts, pairs, img))
    return out


@pytest.mark.parametrize("form", ["default", "in_flight", "lsd8"])
@pytest.mark.parametrize("kind", ["random", "one_key", "hard"])
def test_grid_cap_changes_nothing(kind, form, monkeypatch):
    """164 k splats = 41 chunks of 4096 keys (81 of 2048) on 1, 5 and 8 workgroups (8: the xcd_contiguous remap of the downsweeps;
    1 and 5: the plain mapping), three frames per context: keys and permutation against the oracle, tile lists and pixels bit for
    bit those of the uncapped context (one-pass frames: the lists of a two-pass frame are those of its second pass)"""
    cloud, frames = grid_cap_frames(kind)
    base = renderer(cloud, form, monkeypatch, slc.GRID_CAP_N, two_pass=_capi.TWO_PASS_OFF)
    want = three_frames(base, frames, "%s %s uncapped" % (kind, form))
    base.close()
    assert all((img[..., :3] != 0).any() for _, _, img in want)
    for cap in (1, 5, 8):
        r = renderer(cloud, form, monkeypatch, slc.GRID_CAP_N, cap=cap, two_pass=_capi.TWO_PASS_OFF)
        got = three_frames(r, frames, "%s %s cap %d" % (kind, form, cap))
        r.close()
        for f, (a, b) in enumerate(zip(got, want)):
            for x, y, part in zip(a, b, ("list offsets", "lists", "pixels")):
                np.testing.assert_array_equal(x, y, err_msg="%s %s cap %d frame %d: %s" % (kind, form, cap, f, part))


def test_grid_cap_gives_the_same_storage_order(monkeypatch):
    """the Morton sort at upload under MSPLAT_GRID_CAP=5"""
    cloud, frames = grid_cap_frames("random")
    orders = []
    for cap in (None, 5):
        r = renderer(cloud, "default", monkeypatch, slc.GRID_CAP_N, cap=cap, spatial_order=_capi.SPATIAL_ON)
        orders.append(r.storage_order())
        assert orders[-1] is not None and np.array_equal(np.sort(orders[-1]), np.arange(slc.GRID_CAP_N))
        r.Sort(*frames[0][0])
        np.testing.assert_array_equal(r.sorted_keys(), frames[0][1][0])
        r.close()
    np.testing.assert_array_equal(orders[0], orders[1])
