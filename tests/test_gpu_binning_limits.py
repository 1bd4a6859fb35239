"""The bin-list build at its limits: skewed rectangles, chunk edges, heavy chunks with and without helper slots.

The rest of the suite feeds the two partitions that build the bin lists (bin1_upsweep / bin1_downsweep, radix_upsweep /
radix_downsweep<MODE_PAIR> + tile_table_role) random, "hard" and scene-like clouds, whose pairs spread evenly over columns, rows and
chunks.  The cases of tests/binning_limit_cases.py are DESIGNED rectangles -- one axis-aligned splat per rectangle at a designed
depth, so the rank, the rectangle and every list are known before anything runs; tests/test_binning_limits_fixtures.py asserts
every claim on the CPU and, per case, the mistake it catches:
  owner_edge      M = 8191 / 8192 / 8193 items in a chunk and a chunk of 16-wide rectangles with runs of EMPTY ones: the owner
                  table against the binary search of s_off over equal offsets (the search picks the first of equal offsets)
  thin_chunks     a middle chunk of 0, 1, 63, 64, 65, 255, 256, 257 items: waves without work (per_wave rounded down)
  store_shapes    every (pos mod 4, rows = 1 ... 12): the heads, body and tails of the emit (a head or tail writes the wrong row)
  heavy_edge      49152 pairs in a chunk are not heavy, 49153 are (the threshold is >=)
  heavy_parts     a split chunk at tiles_x = 1, 7, 8, 9, 256 (a part's column range is one too narrow)
  heavy_slots     0, 1 and 130 heavy chunks on one context (a heavy chunk without a slot is flagged as split)
  one_column      every pair in column 0 / 255, 32, 33, 128, 129, 130 chunk rows (a group's first row misses the row before it)
  one_row         tiles_y = 1: a pure stable copy of 4095 ... 524289 words (the same in the row pass; column recovery)
  one_bin         one list of 1, 4096, 4097, 70 000 entries (the heaviest-first bucket is not clamped; a length in 16 bits)
  sparse_columns  one pair per column, columns {0, 255} only, columns of 4095 / 4096 / 4097 words, chunks over exactly 4 and 5
                  columns (column recovery stops at the wave's first column; counts beyond the fourth column are dropped)
  tall_weights    more than 64 consecutive 1 x 256 rectangles (eight weight bit planes instead of nine)
  cap_edge        the last item straddles a capacity of D - 1 (the guarded stores; the verdict is incl > cap)

Every case: projection through _check_projection, then EXACTLY -- the library's rectangles are the designed ones, stats()["pairs"]
= D, msplat_debug_get_tile_lists is the model word for word (column byte and rank), verify_order() = (0, 0).  Forms: the default,
rank_mode = RANK_BALLOT, MSPLAT_SCAN_KERNELS=1, frame_mode = FRAMES_IN_FLIGHT; three frames per context (the three-kernel row pass,
then the scan-free one; both parities of the heavy list; helpers absent, then present), every frame's lists and pixels bit for
bit those of the default's first frame.  Which heavy regime ran is read from msplat_debug_get_heavy_chunks after every frame.

Images against the oracle (check_image, caps unchanged; -rP prints them): see MEASURED below.  Every other case is list-exact and
bit-for-bit only: its splats are nearly opaque (the 133 120 full-screen ones end every pixel after two layers).

Not asserted, because the library has no tap for it: which form radix_upsweep took (LDS columns, global atomics, the one-column
straight line) and whether bin1_downsweep used the owner table.  The fixture module asserts the conditions instead: the columns
and words per 4096-word chunk of the column-ordered pairs (sparse_columns), and M against 8192 (owner_edge).

MEASURED on the MI355X (EXPERIMENTS.md, round 29): the module runs in 7.1 s, its slowest test (test_heavy_slots_walk, seven frames
of up to 6.5 M pairs) in 0.77 s, the 132 k-splat one-column cases in 0.37 s each.  No list, rectangle or pair count was wrong in any
form.  Images against the oracle, max |diff| (mean), every value within 1e-4: store_shapes 1.5e-6 (1.5e-7), heavy_edge_49152 2.2e-6
(2.0e-7), heavy_edge_49153 2.4e-6 (2.0e-7), one_bin_4097 6.5e-6 (7.2e-7), sparse_one_each 1.0e-6 (5.5e-8), tall_weights 1.7e-6
(2.1e-7).

A finding on the way, in the input and not in a kernel: heavy_edge first had near rectangles of 2 x 1 bins, and its image missed
check_image's share (98.99 % of values within 1e-4).  The library's frame equalled the float64 definition to 1.3e-6; the oracle
was off by up to 0.016, because the reference's 3.5-sigma quad is turned by an angle that is a quotient of rounding residues when
cov_xy ~ 1e-12, and stood across 54 of those splats.  binning_limit_cases.heavy_edge tells the story; its near rectangles are
square now, and the fixture module asserts that the oracle's quad holds every footprint where an image is compared."""
import functools
import time

import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import MsplatError, SplatRenderer, _capi, camera
from tests import binning_limit_cases as blc
from tests.checks import check_image, same_bits
from tests.gpu_harness import QUEUE_SENTINEL, _check_projection, bin_edge, device_frame, no_sentinel, oracle_frame, stereo_frame

pytestmark = pytest.mark.gpu

# form -> (SplatRenderer arguments, environment at msplat_create)
FORMS = {
    "default": ({}, {}),
    "ballot": ({"rank_mode": _capi.RANK_BALLOT}, {}),
    "scan": ({}, {"MSPLAT_SCAN_KERNELS": "1"}),
    "in_flight": ({"frame_mode": _capi.FRAMES_IN_FLIGHT}, {}),
}
ENV = ("MSPLAT_SCAN_KERNELS", "MSPLAT_GRID_CAP", "MSPLAT_SORT")


def renderer(cloud, form, monkeypatch, cap=None, **kw):
    """a context of the given form (the switches are read once, by msplat_create) holding the cloud in upload order"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    env = dict(FORMS[form][1])
    if cap is not None:
        env["MSPLAT_GRID_CAP"] = str(cap)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = SplatRenderer(device=0, **dict(FORMS[form][0], **kw))
    ok = r.Init(cloud, False, False)
    for k in env:
        monkeypatch.delenv(k)
    assert ok, r.last_error()
    assert r.storage_order() is None
    return r


CASES = dict([("owner_edge_" + v, lambda v=v: blc.owner_edge(v)) for v in blc.OWNER_EDGE]
             + [("thin_chunks_%d" % m, lambda m=m: blc.thin_chunks(m)) for m in blc.THIN_M]
             + [("store_shapes", blc.store_shapes)]
             + [("heavy_edge_%d" % (49152 + e), lambda e=e: blc.heavy_edge(bool(e))) for e in (0, 1)]
             + [("heavy_parts_%d" % t, lambda t=t: blc.heavy_parts(t)) for t in sorted(blc.HEAVY_PARTS_SHAPES)]
             + [("one_column_%d_col%d" % (V, c), lambda V=V, c=c: blc.one_column_groups(V, c)) for V in blc.GROUPS_V for c in (0, 255)]
             + [("one_row_%d" % D, lambda D=D: blc.one_row(D)) for D in blc.ONE_ROW_D]
             + [("one_bin_%d" % V, lambda V=V: blc.one_bin(V)) for V in blc.ONE_BIN_V]
             + [("sparse_" + v, lambda v=v: blc.sparse_columns(v)) for v in blc.SPARSE]
             + [("tall_weights", blc.tall_weights)])
IMAGES = ("one_bin_4097", "store_shapes", "heavy_edge_49152", "heavy_edge_49153", "sparse_one_each", "tall_weights")


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=2)
def prepared(name):
    """(case, cloud, oracle reference, model lists) of a named case, computed once; the reference has an image where the case gets one"""
    case = CASES[name]()
    assert case.name == name
    cloud = blc.cloud_of(case)
    return (case, cloud) + expected(cloud, case.view, case.rects, image=name in IMAGES)


def expected(cloud, v, rects, image=False):
    cam, proj, vp, nf = v
    if image:
        ref = oracle_frame(cloud.as_array(), False, cam, proj, vp, nf)
        frozen(ref["image"], ref["budget"])
    else:
        ref = orc.render_frame(cloud.as_array(), False, cam, proj, vp, nf, nthreads=16, want_image=False, want_splats=True)
    frozen(ref["splats"])
    return ref, frozen(*blc.model_lists(rects, *blc.tiles_of(v)))


def slots_after(last_heavy):
    """the helper slots issue_binning gives a frame whose predecessor met last_heavy heavy chunks"""
    return min(blc.HEAVY_CAP, 2 * last_heavy + 8) if last_heavy else 0


def frame(r, v, rects, ref, model, what, heavy=None):
    """Sort + Render of one frame and everything that is asserted of every frame; returns (list offsets, lists, pixels).
    heavy: (heavy chunks of this frame, of the frame before it on the context)"""
    r.Sort(*v)
    img = r.Render(*v)
    W, H = v[2][2], v[2][3]
    assert r.sort_count() == rects.shape[0], what
    rect = _check_projection(r, ref, W, H)
    np.testing.assert_array_equal(rect, blc.pack(rects), err_msg=what)
    st = r.stats()
    assert (st["tiles_x"], st["tiles_y"]) == blc.tiles_of(v), what
    assert st["pairs"] == model[0][-1] == model[1].size, (what, st["pairs"], model[1].size)
    ts, pairs = r.debug_tile_lists()
    np.testing.assert_array_equal(ts, model[0], err_msg=what + ": list offsets")
    np.testing.assert_array_equal(pairs, model[1], err_msg=what + ": lists")
    assert r.verify_order() == (0, 0), what
    if heavy is not None:
        assert r.heavy_chunks() == (heavy[0], slots_after(heavy[1])), (what, r.heavy_chunks(), heavy)
    return ts, pairs, img


def report(what, img, ref):
    d = np.abs(img[..., :3].astype(np.float64) - ref["image"][..., :3])
    print("%s: max |diff| %.3g, mean %.3g, within 1e-4: %.5f" % (what, d.max(), d.mean(), (d <= 1e-4).mean()))
    check_image(img, ref["image"], budget=ref["budget"])
    assert (img[..., :3] != 0).any()


# ------------------------------------------------------------------------------------------------
# 1. every named case in every form, three frames per context
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_lists_are_exact_in_every_form(name, monkeypatch):
    case, cloud, ref, model = prepared(name)
    h = case.claims["heavy"]
    first = None
    for form in FORMS:
        r = renderer(cloud, form, monkeypatch)
        for f in range(3):
            what = "%s, %s, frame %d" % (name, form, f)
            got = frame(r, case.view, case.rects, ref, model, what, heavy=(h, h if f else 0))
            if first is None:
                first = got
                if name in IMAGES:
                    report(name, got[2], ref)
            same_bits(got[2], first[2], what + ": pixels")
        r.close()
    print("%s: %d ranks, D %d, heavy chunks %d -- %s" % (name, case.claims["n"], case.claims["D"], h, case.claims["reaches"]))


# ------------------------------------------------------------------------------------------------
# 2. heavy chunks and helper slots
# ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def slots_prepared():
    case = blc.heavy_slots()
    cloud = blc.cloud_of(case)
    views = {}
    for which in blc.SLOTS_VIEWS:
        v, rects, claims = blc.heavy_slots_view(which)
        views[which] = (v, rects, claims) + expected(cloud, v, rects)
    return cloud, views


def test_heavy_slots_walk():
    """light -> one -> many -> many -> light -> light -> many on ONE context whose capacity holds the 6.5 M pairs (a retry after an
    overflow would launch the frame twice and move the slots): helper slots 0, 0, 10 (for 130 heavy chunks: split and unsplit
    chunks in one launch), 128 = kHeavyCap (still fewer than 130), 128 with NO heavy chunk (heavy_flag rewritten to 0), 0, 0 (130
    heavy chunks, all unsplit).  Every frame's lists are the model's; frames of one view are bit-identical"""
    cloud, views = slots_prepared()
    r = SplatRenderer(device=0, pair_capacity=7 * 1000 * 1000)
    assert r.Init(cloud, False, False), r.last_error()
    assert r.storage_order() is None
    last, seen, pixels = 0, [], {}
    for f, which in enumerate(("light", "one", "many", "many", "light", "light", "many")):
        v, rects, claims, ref, model = views[which]
        got = frame(r, v, rects, ref, model, "frame %d (%s)" % (f, which), heavy=(claims["heavy"], last))
        seen.append((claims["heavy"], slots_after(last)))
        last = claims["heavy"]
        same_bits(got[2], pixels.setdefault(which, got[2]), "frame %d (%s): pixels" % (f, which))
        assert (got[2][..., :3] != 0).any()
    print("heavy chunks, helper slots per frame: %s" % seen)
    assert seen == [(0, 0), (1, 0), (130, 10), (130, 128), (0, 128), (0, 0), (130, 0)]
    assert r.stats()["pair_capacity"] == 7 * 1000 * 1000
    r.close()


def test_a_growing_context_builds_the_6_5_m_pairs():
    """without a fixed capacity the first "many" frame overflows the initial buffer, grows it and is right"""
    cloud, views = slots_prepared()
    v, rects, claims, ref, model = views["many"]
    r = SplatRenderer(device=0)
    assert r.Init(cloud, False, False), r.last_error()
    cap0 = r.stats()["pair_capacity"]
    frame(r, v, rects, ref, model, "many, growing context")
    print("pair capacity %d -> %d for %d pairs" % (cap0, r.stats()["pair_capacity"], claims["D"]))
    assert cap0 < claims["D"] <= r.stats()["pair_capacity"]
    assert r.heavy_chunks()[0] == 130
    r.close()


@pytest.mark.parametrize("cap", [1, 5])
def test_one_heavy_chunk_under_grid_cap(cap, monkeypatch):
    """MSPLAT_GRID_CAP = 1 and 5: nmain is 1 / 5 main workgroups for 130 chunks (the XCD remap off), the helpers of the one heavy
    chunk in front of them from the second frame on; lists exact, pixels those of the uncapped context"""
    cloud, views = slots_prepared()
    v, rects, claims, ref, model = views["one"]
    want = None
    for c in (None, cap):
        r = renderer(cloud, "default", monkeypatch, cap=c)
        for f in range(3):
            got = frame(r, v, rects, ref, model, "one, cap %s, frame %d" % (c, f), heavy=(1, 1 if f else 0))
            want = got if want is None else want
            same_bits(got[2], want[2], "one, cap %s, frame %d: pixels" % (c, f))
        r.close()


def test_heavy_edge_as_a_pinned_two_pass_frame(monkeypatch):
    """share 1/2 pins the cut at rank 1024: pass 1 bins chunk 1 from d_first = 1024 on, pass 2 the whole frame (render_parity flips
    twice); pixels are the one-pass frame's, both passes binned pairs, and the tap reports the second chain's heavy chunk"""
    for extra in (False, True):
        case, cloud, ref, model = prepared("heavy_edge_%d" % (49152 + extra))
        a = renderer(cloud, "default", monkeypatch, two_pass=_capi.TWO_PASS_OFF)
        want = frame(a, case.view, case.rects, ref, model, "one pass")[2]
        assert a.two_pass_info() is None
        a.close()
        b = renderer(cloud, "default", monkeypatch, two_pass=_capi.TWO_PASS_ON)
        b.two_pass_state(0.5)
        for f in range(3):
            b.Sort(*case.view)
            img = b.Render(*case.view)
            same_bits(img, want, "two passes, frame %d" % f)
            info = b.two_pass_info()
            assert info is not None and info["visible"] == 2048 and info["pairs_pass1"] > 0 and info["pairs_pass2"] > 0, info
            assert b.heavy_chunks()[0] == int(extra), (b.heavy_chunks(), info)
            assert b.verify_order() == (0, 0)
        print("heavy_edge %d, two passes at share 1/2: %s, heavy tap %s" % (49152 + extra, info, b.heavy_chunks()))
        assert b.two_pass_state(0.5)[0] == 3
        b.close()


def test_a_split_chunk_in_a_stereo_chain(monkeypatch):
    """heavy_parts at tiles_x = 9 through RenderStereo (both views' ranks in one binning chain, 2 x 8 virtual bin rows): each eye
    is bit-identical to its own Render, with helpers absent (first frame) and present"""
    case, cloud, ref, model = prepared("heavy_parts_9")
    cam, proj, vp, nf = case.view
    eyes = [camera.translate_local(cam, dx=-0.004), camera.translate_local(cam, dx=+0.004)]
    r = renderer(cloud, "default", monkeypatch)
    r.Sort(*case.view)
    want = []
    for e in range(2):
        want.append(device_frame(r, case.view, None, None, call=r.Render, render_cam=eyes[e], **bin_edge()))
        no_sentinel(want[-1])
    assert not np.array_equal(want[0], want[1])
    r.close()
    rs = renderer(cloud, "default", monkeypatch)
    rs.Sort(*case.view)
    for f in range(3):
        imgs = stereo_frame(rs, eyes, [proj, proj], vp, nf, None, None, call=rs.RenderStereo, **bin_edge())
        assert rs.stats()["tiles_y"] == 16
        heavy, slots = rs.heavy_chunks()
        assert heavy >= 1 and slots == (slots_after(heavy) if f else 0), (f, heavy, slots)
        for e in range(2):
            same_bits(imgs[e], want[e], "frame %d eye %d" % (f, e))
        assert rs.verify_order() == (0, 0)
    print("stereo chain: heavy chunks %d, helper slots %d" % (heavy, slots))
    rs.close()


# ------------------------------------------------------------------------------------------------
# 3. the capacity edge
# ------------------------------------------------------------------------------------------------

def test_the_last_item_straddles_the_capacity(monkeypatch):
    """cap_edge: with pair_capacity = D the frame is right and nothing overflows; with D - 1 the last item (13 rows, the end of the
    pair array) takes the guarded stores and the Render fails with MSPLAT_ERR_PAIR_OVERFLOW naming D; the next frame of the
    smaller view on that context is right"""
    case = blc.cap_edge()
    cloud = blc.cloud_of(case)
    ref, model = expected(cloud, case.view, case.rects)
    D = case.claims["D"]
    sv, srects = blc.cap_edge_small_view()
    sref, smodel = expected(cloud, sv, srects)
    for form in ("default", "ballot"):
        a = renderer(cloud, form, monkeypatch, pair_capacity=D)
        assert a.stats()["pair_capacity"] == D, "msplat_create changed the capacity: size the case to %d" % a.stats()["pair_capacity"]
        want = [frame(a, case.view, case.rects, ref, model, "%s, capacity D, frame %d" % (form, f)) for f in range(2)]
        same_bits(want[1][2], want[0][2], "capacity D")
        a.close()
        b = renderer(cloud, form, monkeypatch, pair_capacity=D - 1)
        assert b.stats()["pair_capacity"] == D - 1
        b.Sort(*case.view)
        with pytest.raises(MsplatError) as e:
            b.Render(*case.view)
        assert e.value.code == _capi.ERR_PAIR_OVERFLOW and ("need %d" % D) in str(e.value), str(e.value)
        small = frame(b, sv, srects, sref, smodel, "%s, capacity D - 1, the smaller view" % form)
        c = renderer(cloud, form, monkeypatch)
        same_bits(small[2], frame(c, sv, srects, sref, smodel, "the smaller view on a context of its own")[2], "the smaller view")
        b.close(); c.close()
