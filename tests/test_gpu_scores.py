"""GPU tests of the score frame (msplat_render_scores, msplat_mark_scores).  The vectors are compared with the
float64 definition of tests/scores_rule.py under its derived bound (tests/test_scores.py holds the fp32 walk three orders of
magnitude inside it and keeps the bound from hiding a failure), and with the library's own other execution shapes bit for bit:
windows against their complements, regions against windows, contexts that differ in everything the sums must not depend on, masked
and cropped contexts against contexts that were uploaded the visible splats only, compact storages against an FP32 context of their
download.  msplat_mark_scores is compared with numpy, exactly.  Views are at most 517 x 293 with at most 20 k splats.  Refusals are
checked before any launch: a host address handed to the library is answered by its pointer query (check_device_source)."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import _capi
from splatapult_amd._capi import MsplatError
from tests import ids_rule, scenes
from tests import scores_rule as sr
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import make_renderer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL1 = sr.TOL + 2.0 ** -24          # one value: the colour frame's bound plus the rounding of q


def case_renderer(name, **kw):
    if name == "stack":
        aos, W, H, view = sr.stack()
    else:
        aos, _, W, H, view = sr.case(name)
    r = make_renderer(aos, **kw)
    r.Sort(*view)
    return r, W, H, view


def host(score, hits=None):
    """the tensors RenderScores returns as numpy uint64 / uint32"""
    s = score.cpu().numpy().view(np.uint64)
    return s if hits is None else (s, hits.cpu().numpy().view(np.uint32))


def scores_of(r, view, window=None, region=None):
    """(score, pixels) of one frame from fresh zeros, as numpy"""
    s, p = host(*r.RenderScores(*view, window=window, region=region, pixels=True))
    assert s.shape == p.shape == (r._n,)
    return s, p


def zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)


def assert_same(got, want, what):
    same_bits(got[0], want[0], "%s: score" % what)
    same_bits(got[1], want[1], "%s: pixels" % what)


@pytest.fixture(scope="module")
def sparse_scores():
    """the whole-viewport vectors of a default context on the sparse case, computed once, read-only"""
    r, W, H, view = case_renderer("sparse")
    s, p = scores_of(r, view)
    same_bits(host(r.RenderScores(*view)), s, "the score-only kernel")
    r.close()
    s.setflags(write=False)
    p.setflags(write=False)
    return s, p


def assert_inside_the_bound(ref, s, p, what):
    S, bound = sr.per_upload_index(ref, ref["S"]), sr.per_upload_index(ref, ref["bound"])
    A, sure = sr.per_upload_index(ref, ref["A"]), sr.per_upload_index(ref, ref["sure"])
    err = np.abs(s.astype(np.float64) / sr.ONE - S)
    drawn = A > 0
    print("%s: worst err / bound %.3g over %d drawn splats; sum of scores %.6g (definition %.6g)"
          % (what, (err[drawn] / bound[drawn]).max(), drawn.sum(), s.sum() / sr.ONE, S.sum()))
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, "%d splat(s) outside the bound, first %d: score %.9g, definition %.9g, bound %.3g" % (
        bad.size, bad[0], s[bad[0]] / sr.ONE, S[bad[0]], bound[bad[0]])
    # splats not in the Sort and splats the projection rejects: A = 0, so the bound is 0 and the score exactly 0
    assert not s[~drawn].any() and not p[~drawn].any()
    assert (p <= A).all(), "a splat hits more pixels than its footprint has: %s" % np.flatnonzero(p > A)[:5]
    assert (p >= sure).all(), "a splat misses pixels it surely reaches: %s" % np.flatnonzero(p < sure)[:5]
    assert ((p == 0) == (s == 0)).all()


# ---- 1. against the definition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sr.CASES)
def test_the_scores_match_the_definition(name):
    ref = sr.reference(name)
    r, W, H, view = case_renderer(name)
    assert r.sort_count() == ref["V"] and r._n == ref["n"]
    s, p = scores_of(r, view)
    same_bits(host(r.RenderScores(*view)), s, "the score-only kernel")
    r.close()
    assert_inside_the_bound(ref, s, p, name)
    assert (s > 0).sum() >= 0.9 * (ref["A"] > 0).sum()


# ---- 2. bit-exact invariants -----------------------------------------------------------------------------------------------------
def complement(window, W, H):
    """the rectangles that complete a window to the viewport: below, above, left, right"""
    x0, y0, w, h = window
    rects = [(0, 0, W, y0), (0, y0 + h, W, H - y0 - h), (0, y0, x0, h), (x0 + w, y0, W - x0 - w, h)]
    return [q for q in rects if q[2] > 0 and q[3] > 0]


def test_windows_regions_and_accumulation_are_exact(sparse_scores):
    import torch
    r, W, H, view = case_renderer("sparse")
    n = r._n
    assert_same(scores_of(r, view), sparse_scores, "a second context")
    for window in ids_rule.windows(W, H):
        x0, y0, w, h = window
        own = scores_of(r, view, window)
        # the window plus its complement, accumulated into one pair of arrays
        score, hits = zeros(n)
        for q in [window] + complement(window, W, H):
            got = r.RenderScores(*view, window=q, score=score, pixels=hits)
            assert got[0] is score and got[1] is hits
        assert_same(host(score, hits), sparse_scores, "window %s plus its complement" % (window,))
        # a region plane of the viewport that is nonzero exactly on the window
        plane = np.zeros((H, W), np.uint8)
        plane[y0:y0 + h, x0:x0 + w] = 1 + (np.arange(w) % 255)
        assert_same(scores_of(r, view, region=plane), own, "a region that is window %s" % (window,))
    # a region of bytes 0 / 2 / 255 inside a window, tight and with a pitch; bool planes too
    window = (13, 27, 40, 9)
    rng = np.random.default_rng(7)
    region = rng.choice(np.array([0, 2, 255], np.uint8), (9, 40))
    tight = scores_of(r, view, window, region)
    assert 0 < tight[0].sum() < scores_of(r, view, window)[0].sum()
    wide = np.full((9, 40 + 9), 255, np.uint8)                   # padding that would select everything
    wide[:, :40] = region
    d_wide = torch.from_numpy(wide).to(DEV)
    assert_same(scores_of(r, view, window, d_wide[:, :40]), tight, "a pitched region")
    assert_same(scores_of(r, view, window, torch.from_numpy(region != 0).to(DEV)), tight, "a bool region")
    # the sum of the selected pixels' 1 x 1 windows
    score, hits = zeros(n)
    for y, x in np.argwhere(region != 0)[::7]:
        r.RenderScores(*view, window=(13 + int(x), 27 + int(y), 1, 1), score=score, pixels=hits)
    sel = np.zeros_like(region)
    sel[tuple(np.argwhere(region != 0)[::7].T)] = 1
    assert_same(host(score, hits), scores_of(r, view, window, sel), "single pixels against their region")
    # two calls into one array are twice one call; an all-zero region adds nothing
    score, hits = zeros(n)
    r.RenderScores(*view, score=score, pixels=hits)
    r.RenderScores(*view, score=score, pixels=hits)
    assert_same(host(score, hits), (2 * sparse_scores[0], 2 * sparse_scores[1]), "two calls into one array")
    r.RenderScores(*view, region=np.zeros((H, W), np.uint8), score=score, pixels=hits)
    assert_same(host(score, hits), (2 * sparse_scores[0], 2 * sparse_scores[1]), "an all-zero region")
    r.close()


# ---- 3. what the sums do not depend on -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(t_epsilon=0.0), dict(compositor_waves=64), dict(frame_mode=_capi.FRAMES_SERIAL),
                                dict(two_pass=_capi.TWO_PASS_ON), dict(fb_format="fp16"), dict(target_mode="premultiplied")],
                         ids=["t_epsilon_0", "64_waves", "serial", "two_pass", "fp16", "premultiplied"])
def test_the_scores_do_not_depend_on_the_context(kw, sparse_scores):
    kw = dict(kw)
    mode = kw.pop("target_mode", None)
    r, W, H, view = case_renderer("sparse", **kw)                 # 627 tiles: 64 waves take several items each
    if mode:
        r.set_target_mode(mode)
    info = None
    if "two_pass" in kw:
        before = r.Render(*view)
        info = r.two_pass_info()
        assert info is not None, "two_pass = ON did not run the Render as two passes"
    assert_same(scores_of(r, view), sparse_scores, str(kw))
    assert_same(scores_of(r, view, (13, 27, 40, 9)), scores_of_default_window(), "%s, a window" % kw)
    if info is not None:
        assert r.two_pass_info() == info, "the score frame changed msplat_get_two_pass_info"
        same_bits(r.Render(*view), before, "the Render after the score frame")
    r.close()


_WINDOW = {}


def scores_of_default_window():
    """window (13, 27, 40, 9) of a default context on sparse, computed once"""
    if not _WINDOW:
        r, W, H, view = case_renderer("sparse")
        _WINDOW["v"] = scores_of(r, view, (13, 27, 40, 9))
        r.close()
    return _WINDOW["v"]


# ---- 4. against the id frame -----------------------------------------------------------------------------------------------------
def test_a_single_pixel_scores_highest_what_the_id_frame_names():
    ref = ids_rule.reference("sparse")
    r, W, H, view = case_renderer("sparse")
    decided = np.argwhere(ref["decided"] & (ref["best"] > 0.0))
    rng = np.random.default_rng(23)
    worst = 0.0
    for y, x in decided[rng.choice(decided.shape[0], 200, replace=False)]:
        x, y = int(x), int(y)
        score = r.RenderScores(*view, window=(x, y, 1, 1))
        top, val = int(score.argmax()), int(score.max())
        picked, _ = r.Pick(*view, x, y)
        assert top == picked == int(ref["id"][y, x]), "pixel (%d, %d): the highest score is %d's, Pick names %s, the rule %d" % (
            x, y, top, picked, ref["id"][y, x])
        err = abs(val / sr.ONE - float(ref["best"][y, x]))
        worst = max(worst, err)
        assert err <= TOL1, "pixel (%d, %d): score %.9g, the rule's best %.9g" % (x, y, val / sr.ONE, ref["best"][y, x])
    print("200 decided pixels: worst |score / 2^23 - best| = %.3g (bound %.3g)" % (worst, TOL1))
    empty = np.argwhere(ref["decided"] & (ref["best"] == 0.0))[::997]
    assert empty.shape[0] >= 5
    for y, x in empty:                                            # a pixel no splat reaches: nothing scores
        assert int(r.RenderScores(*view, window=(int(x), int(y), 1, 1)).max()) == 0 and r.Pick(*view, int(x), int(y))[0] is None
    r.close()


# ---- 5. the stop rule, on the designed case --------------------------------------------------------------------------------------
def test_the_stack_stops_where_nothing_can_score_and_does_not_wrap():
    """Twelve discs that cover the viewport, alpha 0.9 x 10, 1.0, 0.9.  Behind the eighth T = 1e-8 <= 2^-24 on every pixel, so the
    ninth to twelfth score exactly 0 -- the eleventh too, whose definition value of 2e-7 lies inside its bound.  A central tile of
    the front splat sums to 0.9 * 2^31."""
    ref = sr.reference("stack")
    r, W, H, view = case_renderer("stack")
    assert r.sort_count() == 12
    s, p = scores_of(r, view)
    print("stack: scores / 2^23 =", s / sr.ONE, "pixels =", p)
    assert not s[[8, 9, 11]].any() and not p[[8, 9, 11]].any(), "splats 9, 10 and 12 score"
    assert_inside_the_bound(ref, s, p, "stack")                   # splat 11 among them
    assert (p[:8] == W * H).all()
    # the front splat, tile by tile: 256 pixels of 0.9 * 2^23 each, above 2^30 and below 2^31
    tile = sr.per_upload_index(ref, ref["tile"])[0]
    for window in ((16, 16, 16, 16), (0, 0, 16, 16), (32, 32, 16, 16)):
        t, tp = scores_of(r, view, window)
        assert tp[0] == 256 and 2 ** 30 < t[0] <= 2 ** 31, (window, t[0])
    t, _ = scores_of(r, view, (16, 16, 16, 16))                    # the central tile is the definition's largest
    assert abs(t[0] / sr.ONE - tile) <= 256 * TOL1, (t[0] / sr.ONE, tile)
    assert s[0] > 8 * 2 ** 30
    r.close()
    r, W, H, view = case_renderer("stack", t_epsilon=0.5)         # the colour frame would stop behind the first splat
    assert_same(scores_of(r, view), (s, p), "t_epsilon = 0.5")
    r.close()


# ---- 6. numbering ----------------------------------------------------------------------------------------------------------------
def tie_free():
    return vr.cloud_aos(*vr.TIE_FREE), vr.view()


def sorted_scores(aos, view, **kw):
    r = make_renderer(np.ascontiguousarray(aos), **kw)
    r.Sort(*view)
    got = scores_of(r, view)
    r.close()
    return got


def test_morton_and_upload_order_give_the_same_scores():
    aos, view = tie_free()
    off = sorted_scores(aos, view, spatial_order=_capi.SPATIAL_OFF)
    r = make_renderer(aos, spatial_order=_capi.SPATIAL_ON)
    order = r.storage_order()
    assert order is not None and (order != np.arange(order.shape[0])).any(), "the cloud was not reordered"
    r.Sort(*view)
    on = scores_of(r, view)
    assert_same(on, off, "spatial_order ON against OFF")
    assert (on[0] > 0).sum() > 1000, "the view shows too few splats to tell the numberings apart"
    assert np.isin(np.flatnonzero(on[0]), r.sorted_indices()).all()
    r.close()


@pytest.mark.parametrize("spatial", [_capi.SPATIAL_OFF, _capi.SPATIAL_ON], ids=["upload_order", "morton_order"])
def test_masked_and_cropped_contexts_equal_the_subset_upload(spatial):
    aos, view = tie_free()
    n = aos.shape[0]
    r = make_renderer(aos, spatial_order=spatial)
    M = vr.matrices()["scaled"]                                  # q is exact for every float32 centre
    in_box = vr.crop(aos[:, 0:3], M, "box")
    for what, keep_mask, apply in (("mask", vr.random_mask(n), lambda m: r.SetVisibility(m)),
                                   ("crop", in_box, lambda m: (r.SetVisibility(None), r.SetCrop(M, "box")))):
        apply(keep_mask)
        r.Sort(*view)
        got = scores_of(r, view)
        keep = np.flatnonzero(keep_mask)
        sub = sorted_scores(aos[keep], view, spatial_order=spatial)
        want = (np.zeros(n, np.uint64), np.zeros(n, np.uint32))
        want[0][keep], want[1][keep] = sub
        assert_same(got, want, "%s against the subset upload" % what)
        assert got[0].any() and not got[0][~keep_mask.astype(bool)].any(), "%s: a hidden splat scores" % what
    r.close()


@pytest.mark.parametrize("storage", ["sh_fp16", "sh_q8"])
def test_compact_storages_give_the_scores_of_their_download(storage):
    aos, view = tie_free()
    r = make_renderer(aos, cloud_storage=storage)
    assert r.cloud_storage() == storage
    r.Sort(*view)
    got = scores_of(r, view)
    stored = r.download_cloud(True)
    r.close()
    assert_same(got, sorted_scores(stored, view), storage)


# ---- 7. mark_scores --------------------------------------------------------------------------------------------------------------
def test_mark_scores_against_numpy_and_the_prune_round_trip(sparse_scores):
    import torch
    r, W, H, view = case_renderer("sparse")
    n = r._n
    score = r.RenderScores(*view)
    s = sparse_scores[0]
    same_bits(host(score), s, "the device scores")
    median = int(np.median(s[s > 0]))
    GUARD = 16                                                   # bytes behind the mask
    rng = np.random.default_rng(5)
    start = rng.integers(0, 256, n, dtype=np.uint8)
    for op in (sr.BELOW, sr.AT_LEAST):
        for threshold in (0, 1, median, 2 ** 63):
            for begin, value in ((np.ones(n, np.uint8), 0), (np.zeros(n, np.uint8), 1), (start, 200)):
                m = torch.from_numpy(np.concatenate([begin, np.full(GUARD, 0x5A, np.uint8)])).to(DEV)
                torch.cuda.synchronize()
                rc = r._lib.msplat_mark_scores(r._ctx, C.c_void_p(score.data_ptr()), n, op, threshold, C.c_void_p(m.data_ptr()), value)
                assert rc == _capi.OK, r.last_error()
                r.synchronize()
                out = m.cpu().numpy()
                assert (out[n:] == 0x5A).all(), "bytes behind the mask were written"
                same_bits(out[:n], sr.mark_reference(s, op, threshold, begin, value), "op %d, threshold %d, value %d" % (op, threshold, value))
    # a score of exactly the threshold is kept by BELOW and taken by AT_LEAST; a threshold above 2^63 compares unsigned
    hand = torch.from_numpy(np.resize(np.array([0, 1, 5, 5, 6, 2 ** 63, 2 ** 64 - 1], np.uint64), n).view(np.int64)).to(DEV)
    for op, name, threshold in ((sr.BELOW, "below", 5), (sr.AT_LEAST, "at_least", 5), (sr.BELOW, "below", 2 ** 64 - 1), (sr.AT_LEAST, "at_least", 2 ** 63 + 1)):
        m = torch.from_numpy(start.copy()).to(DEV)
        r.MarkScores(hand, name, threshold, m, 77)
        same_bits(m.cpu().numpy(), sr.mark_reference(hand.cpu().numpy(), op, threshold, start, 77), "%s %d by hand" % (name, threshold))
    same_bits(host(score), s, "msplat_mark_scores wrote the scores")

    # prune: hide what scores below the median, on the device; the frame is that of a context that was uploaded the survivors only
    mask = torch.ones(n, dtype=torch.uint8, device=DEV)
    r.MarkScores(score, "below", median, mask, 0)
    r.SetVisibility(mask)
    r.Sort(*view)
    keep = np.flatnonzero(s >= median)
    assert 0.2 * (s > 0).sum() < keep.size < 0.8 * (s > 0).sum() and r.sort_count() <= keep.size
    same_bits(mask.cpu().numpy(), (s >= median).astype(np.uint8), "the pruning mask")
    aos = sr.case("sparse")[0]
    sub = make_renderer(np.ascontiguousarray(aos[keep]))
    sub.Sort(*view)
    assert sub.sort_count() == r.sort_count()
    same_bits(r.Render(*view), sub.Render(*view), "the pruned frame against the survivors' upload")
    pruned = scores_of(r, view)
    want = (np.zeros(n, np.uint64), np.zeros(n, np.uint32))
    want[0][keep], want[1][keep] = scores_of(sub, view)
    assert_same(pruned, want, "the scores after pruning")
    sub.close()
    r.close()


# ---- 8. the frames around it, queued frames, refusals -----------------------------------------------------------------------------
def test_renders_around_a_score_frame_are_what_they_were(sparse_scores):
    r, W, H, view = case_renderer("sparse", enable_timing=True)
    s, _, _, _ = case_renderer("sparse")
    want = s.Render(*view)                                       # a context that never runs a score frame
    s.close()
    same_bits(r.Render(*view), want, "the Render before")
    r.synchronize()
    assert r.timings()["frames_averaged"] == 1                   # that Render's set (msplat_get_timings restarts the average)
    assert_same(scores_of(r, view), sparse_scores, "between two Renders")
    scores_of(r, view, (13, 27, 40, 9))
    r.synchronize()
    assert r.timings()["frames_averaged"] == 0, "a score frame recorded a timing set"
    same_bits(r.Render(*view), want, "the Render after")
    r.close()


def test_an_async_submit_context_queues_the_frame(sparse_scores):
    r, W, H, view = case_renderer("sparse", async_submit=True)
    score, hits = zeros(r._n)
    r.RenderScores(*view, score=score, pixels=hits)
    r.RenderScores(*view, window=(13, 27, 40, 9), score=score, pixels=hits)
    r.synchronize()
    w = scores_of_default_window()
    assert_same(host(score, hits), (sparse_scores[0] + w[0], sparse_scores[1] + w[1]), "async_submit, two queued frames")
    assert_same(scores_of(r, view), sparse_scores, "async_submit, fresh arrays")
    r.close()


def raw_scores(r, f, window=None, region=None, pitch=0, score=None, pixels=None, n=None):
    win = (C.c_int32 * 4)(*window) if window is not None else None
    p = lambda v: C.c_void_p(v) if v else None
    return r._lib.msplat_render_scores(r._ctx, *f, win, p(region), pitch, p(score), p(pixels), r._n if n is None else n)


def test_refusals_say_why_and_leave_the_context_usable():
    import torch
    r, W, H, view = case_renderer("hand_placed")
    n = r._n
    want = scores_of(r, view)
    f = r._args.load(*view)
    score, hits = zeros(n)
    region = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    mask = torch.ones(n, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    host_bytes = np.ones(max(H * W, 8 * n) + 8, np.uint8)         # host memory: every pointer query must refuse it
    at = host_bytes.ctypes.data + (-host_bytes.ctypes.data) % 8

    def refused(code, words, **kw):
        kw.setdefault("score", score.data_ptr())
        kw.setdefault("pixels", hits.data_ptr())
        rc = raw_scores(r, f, **kw)
        msg = r.last_error()
        assert rc == code and "msplat_render_scores" in msg and all(w in msg for w in words), (rc, code, msg)
        r.synchronize()
        assert not score.any() and not hits.any(), "a refused frame wrote its arrays"

    rc = raw_scores(r, f, score=None, pixels=hits.data_ptr())
    assert rc == _capi.ERR_INVALID_ARG and "d_score is NULL" in r.last_error()
    for window in ((0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -3, 4), (-1, 0, 4, 4), (0, -1, 4, 4), (W - 3, 0, 4, 4), (0, H - 3, 4, 4),
                   (0, 0, W + 1, H), (W, H, 1, 1), (0, 0, 2 ** 31 - 1, 1), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)):
        refused(_capi.ERR_INVALID_ARG, ["window", "not inside"], window=window)
    refused(_capi.ERR_INVALID_ARG, ["region pitch"], region=region.data_ptr(), pitch=W - 1)
    refused(_capi.ERR_INVALID_ARG, ["region pitch"], window=(0, 0, 40, 9), region=region.data_ptr(), pitch=39)
    for wrong in (n - 1, n + 1, 0):
        refused(_capi.ERR_INVALID_ARG, ["scores for a cloud of"], n=wrong)
    refused(_capi.ERR_INVALID_ARG, ["d_score", "8-byte aligned"], score=score.data_ptr() + 4)
    refused(_capi.ERR_INVALID_ARG, ["d_pixels", "4-byte aligned"], pixels=hits.data_ptr() + 2)
    refused(_capi.ERR_INVALID_ARG, ["d_region", "not device memory"], region=at)
    refused(_capi.ERR_INVALID_ARG, ["d_score", "not device memory"], score=at)
    refused(_capi.ERR_INVALID_ARG, ["d_pixels", "not device memory"], pixels=at)
    L = r._lib
    for args, words in (((C.c_void_p(at), n, 0, 1, C.c_void_p(mask.data_ptr()), 0), ["d_score", "not device memory"]),
                        ((C.c_void_p(score.data_ptr()), n, 0, 1, C.c_void_p(at), 0), ["d_mask", "not device memory"]),
                        ((C.c_void_p(score.data_ptr() + 4), n, 0, 1, C.c_void_p(mask.data_ptr()), 0), ["8-byte aligned"]),
                        ((C.c_void_p(score.data_ptr()), n - 1, 0, 1, C.c_void_p(mask.data_ptr()), 0), ["mask bytes"]),
                        ((C.c_void_p(score.data_ptr()), n, 2, 1, C.c_void_p(mask.data_ptr()), 0), ["op 2"]),
                        ((None, n, 0, 1, C.c_void_p(mask.data_ptr()), 0), ["d_score is NULL"])):
        assert L.msplat_mark_scores(r._ctx, *args) == _capi.ERR_INVALID_ARG
        msg = r.last_error()
        assert "msplat_mark_scores" in msg and all(w in msg for w in words), msg
    r.synchronize()
    assert mask.all() and (host_bytes == 1).all()

    switches = [("msplat_set_depth_test", lambda on: r.set_depth_test(24 if on else 0)),
                ("msplat_set_target_emulation", lambda on: r.set_target_emulation("rgba8" if on else None)),
                ("probe", lambda on: r.set_tile_probe(on)),
                ("banded", lambda on: r.set_band(2 if on else 1, 0))]
    for word, switch in switches:
        switch(True)
        refused(_capi.ERR_UNSUPPORTED, [word])
        with pytest.raises(MsplatError) as e:
            r.RenderScores(*view)
        assert e.value.code == _capi.ERR_UNSUPPORTED
        r.Render(*view)                                          # the Render of that configuration still works
        switch(False)
        assert_same(scores_of(r, view), want, "after %s" % word)
    r.close()

    # before a Sort, before an upload, with a point cloud
    aos, _, W, H, view = sr.case("hand_placed")
    r = make_renderer(aos)
    with pytest.raises(MsplatError) as e:
        r.RenderScores(*view)
    assert e.value.code == _capi.ERR_NO_SORT and "msplat_render_scores" in r.last_error()
    r.Sort(*view)
    assert_same(scores_of(r, view), want, "after the refusal before the Sort")
    r.close()
    cfg = _capi.Config()
    cfg.struct_size = C.sizeof(_capi.Config)
    cfg.t_epsilon = -1.0
    h = C.c_void_p()
    assert L.msplat_create(C.byref(h), C.byref(cfg)) == _capi.OK
    p = [np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)) for x in scenes.default_view(W, H, z=4.0)]
    fp = [x.ctypes.data_as(C.POINTER(C.c_float)) for x in p]
    d_score = C.c_void_p(score.data_ptr())
    assert L.msplat_render_scores(h, *fp, None, None, 0, d_score, None, n) == _capi.ERR_NO_CLOUD and b"msplat_render_scores" in L.msplat_last_error(h)
    assert L.msplat_mark_scores(h, d_score, n, 0, 1, C.c_void_p(mask.data_ptr()), 0) == _capi.ERR_NO_CLOUD and b"msplat_mark_scores" in L.msplat_last_error(h)
    pts = np.random.default_rng(81).uniform(-1, 1, (500, 8)).astype(np.float32)
    pts[:, 3] = 1.0
    pts[:, 4:] = np.abs(pts[:, 4:])
    assert L.msplat_upload_points(h, pts.ctypes.data, pts.shape[0], 32, 0, 16) == _capi.OK
    assert L.msplat_sort(h, *fp) == _capi.OK
    assert L.msplat_render_scores(h, *fp, None, None, 0, d_score, None, 500) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    assert L.msplat_mark_scores(h, d_score, 500, 0, 1, C.c_void_p(mask.data_ptr()), 0) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    img = np.zeros((H, W, 4), np.float32)
    assert L.msplat_render(h, *fp, img.ctypes.data, 0, 0) == _capi.OK         # the point context still renders
    L.msplat_destroy(h)
    torch.cuda.synchronize()
    assert not score.any() and not hits.any() and mask.all()
