"""CPU check of tests/projection_limit_cases.py, judged by the oracle alone: the fixtures of tests/test_gpu_projection_limits.py are
what they claim to be, tests/projection_rule.py restates the oracle's vertex + geometry stage bit for bit, and the three
statements of the footprint rule (include/msplat.h) -- the literal oracle's orc_cov2_class, the numpy oracle's cov2_class and
projection_rule's -- put every fixture splat into the same class.  No device."""
import numpy as np
import pytest

from oracle import np_oracle
from oracle import oracle as orc
from tests import projection_limit_cases as pc
from tests import projection_rule as rule
from tests.checks import TIGHT, check_image
from tests.render_cases import oracle_rects

F = np.float32
SMALL = (129, 97)                 # the viewport of the frame comparisons: 5 x 4 bins, ragged on both axes


def both(aos, vw, srgb=False, render=None):
    """(the oracle's frame data, projection_rule's records of the same draw order) after asserting that the records agree bit for
    bit -- centre, covariance, conic, colour, alpha, ndc, depth, reject -- and that the three classifiers agree"""
    cam, proj, vp, nf = vw
    rcam, rproj, rvp, rnf = render or vw
    ref = orc.render_frame(aos, True, cam, proj, vp, nf, render_cam=rcam, render_proj=rproj, srgb=srgb, nthreads=8,
                           want_image=False, want_splats=True)
    if render is not None:
        # orc.render_frame projects with the Sort call's viewport and near / far; the render view's are its own
        ref["splats"] = orc.project(ref["sorted_idx"], aos, True, srgb, orc.mat4_inverse(rcam), rproj, rvp, rnf, rcam[12:15])
    mine = rule.project(aos, ref["sorted_idx"], True, srgb, orc.mat4_inverse(rcam), rproj, rvp, rnf, rcam[12:15])
    bad = rule.compare_with_oracle(mine, ref["splats"])
    assert not bad, "projection_rule differs from the oracle in %s" % ", ".join(bad)
    cov = ref["splats"]["cov"]
    cls = orc.cov2_class(cov)
    np.testing.assert_array_equal(cls, mine["cls"])
    np.testing.assert_array_equal(cls, np_oracle.cov2_class(cov[:, 0], cov[:, 1], cov[:, 2], cov[:, 3]))
    return ref, mine


# ---- the conditioning ladder --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.LADDER_CAMERAS)
def test_ladder_has_every_class_under_every_camera(name):
    ref, mine = both(pc.ladder_cloud(name).as_array(), pc.view(name))
    ok = ~mine["guard"]                                    # visible and accepted by the guard-band, near and far tests
    cls, L = mine["cls"], rule.major_variance(mine["cov"])
    counts = np.bincount(cls[ok], minlength=3)
    ill = int((ok & (cls == rule.G) & (L > 1e5)).sum())
    # the splats whose class depends on WHICH off-diagonal element is taken for b: an implementation that takes cov2D[1][0]
    # classifies them differently, and the GPU tests' exact drawn set shows it
    other = rule.minor_variance(mine["cov"], b_from=2)
    with np.errstate(invalid="ignore"):
        tell = ok & ((rule.minor_variance(mine["cov"]) >= 0) != (other >= 0))
    decades = np.histogram(np.log10(L[ok & np.isfinite(L)]), bins=[-np.inf, 3, 4, 5, 6, 7, 8, np.inf])[0]
    print("ladder %-15s V %d, accepted %d: G %d (%d with L > 1e5), Q %d, X %d; %d splat(s) tell m01 from m10; L per decade "
          "(<1e3, 1e3.., ..., >=1e8) %s" % (name, ref["V"], ok.sum(), counts[0], ill, counts[1], counts[2], tell.sum(), decades.tolist()))
    assert (counts >= 16).all(), counts
    assert ill >= 16, ill
    assert tell.sum() >= 1
    assert (decades[1:6] >= 16).all(), decades             # every decade from 1e3 to 1e8 is there
    # the Q and X splats would be drawn if only alpha and the guard tests decided
    assert ((mine["alpha"] > F(1.0 / 256.0)) & ok & (cls != rule.G)).sum() >= 32


@pytest.mark.parametrize("name", pc.LADDER_CAMERAS)
def test_ladder_frames_of_the_two_cpu_renderers_agree(name):
    """the literal oracle and the tiled CPU renderer draw the same frame, within the bound the CPU suite uses for the pair
    (check_image with the flip budget, and TIGHT without it).  Before the rule the literal oracle drew the X splats and the tiled
    renderer did not: that frame is made here by clearing `reject` for them, and the difference is printed."""
    W, H = SMALL
    aos, vw = pc.ladder_cloud(name, W, H).as_array(), pc.view(name, W, H)
    ref, mine = both(aos, vw)
    sp = ref["splats"]
    ok = ~mine["guard"]
    counts = np.bincount(mine["cls"][ok], minlength=3)
    assert counts[1] >= 4 and counts[2] >= 4, counts
    image, budget = orc.composite_flip(sp, W, H, nthreads=8)
    cam, proj, vp, nf = vw
    tiled = orc.render_frame_tiled(aos, True, cam, proj, vp, nf, nthreads=8)
    assert tiled["V"] == ref["V"]
    np.testing.assert_array_equal(tiled["sorted_idx"], ref["sorted_idx"])
    d = np.abs(tiled["image"].astype(np.float64) - image)[..., :3]
    before = sp.copy()
    before["reject"][ok & (mine["cls"] == rule.X)] = 0
    old = orc.composite(before, W, H, nthreads=8)
    with np.errstate(invalid="ignore"):
        do = np.abs(tiled["image"].astype(np.float64) - old)[..., :3]
    print("ladder %-15s %d x %d, G %d Q %d X %d: tiled vs literal within 1e-4 %.5f, max %.3g; with the X splats drawn as before the "
          "rule: %d pixel(s) not finite, %d differ by more than 1e-4, max %.3g" % (
              name, W, H, counts[0], counts[1], counts[2], (d <= 1e-4).mean(), d.max(), (~np.isfinite(old)).any(axis=-1).sum(),
              (np.nan_to_num(do, nan=np.inf) > 1e-4).any(axis=-1).sum(), np.nanmax(do) if np.isfinite(do).any() else np.nan))
    check_image(tiled["image"], image, budget=budget)
    assert d.max() <= TIGHT
    assert (image[..., :3] != 0).any()


# ---- threshold neighbours -------------------------------------------------------------------------------------------------------

def test_thresholds_are_hit_and_decided_as_the_oracle_says():
    seen = set()
    for near in pc.THRESHOLD_NEARS:
        aos, labels = pc.threshold_case(near)
        sort, render = pc.threshold_views(near)
        ref, mine = both(aos, sort, render=render)
        assert ref["V"] == aos.shape[0], "Sort's camera culls %d fixture splat(s)" % (aos.shape[0] - ref["V"])
        rej = np.zeros(aos.shape[0], bool)
        rej[ref["sorted_idx"]] = ref["splats"]["reject"] != 0
        ndc = np.zeros((aos.shape[0], 3), F)
        ndc[ref["sorted_idx"]] = ref["splats"]["ndc"]
        for i, (name, which) in enumerate(labels):
            if name == "plain":
                assert not rej[i], i
                continue
            seen.add((name, which))
            if name == "p.w=0":
                assert rej[i], (name, which)
                continue
            axis = "xyz".index(name[4])
            target = F(name.split("=")[1])
            want = {"pred": pc.pred(target), "exact": target, "succ": pc.succ(target)}[which]
            assert ndc[i, axis] == want, (name, which, ndc[i, axis])
            # near plane: < 0.25 rejects; far plane: > 1 rejects; guard band: beyond +-2 rejects -- the value itself is kept
            outside = {"ndc.z=0.25": which == "pred", "ndc.z=1": which == "succ"}.get(name, which == ("succ" if target > 0 else "pred"))
            assert rej[i] == outside, (name, which, ndc[i], rej[i])
    names = ("ndc.z=0.25", "ndc.z=1", "ndc.x=+2", "ndc.x=-2", "ndc.y=+2", "ndc.y=-2", "p.w=0")
    missing = [(n, w) for n in names for w in ("pred", "exact", "succ") if (n, w) not in seen]
    assert not missing, missing
    assert ("p.w=0", "tz*tz underflows") in seen


def test_alpha_thresholds():
    aos, vw = pc.alpha_case()
    ref, mine = both(aos, vw)
    sp = ref["splats"]
    assert ref["V"] == aos.shape[0] and (sp["reject"] == 0).all()
    drawn = oracle_rects(sp, pc.W, pc.H)[0]
    for j, (name, alpha) in enumerate(pc.ALPHAS):
        r = int(np.flatnonzero(ref["sorted_idx"] == j)[0])
        assert sp["alpha"][r] == alpha and (sp["px"][r], sp["py"][r]) == (pc.W / 2, pc.H / 2), (name, sp[r])
        assert sp["cov"][r].tolist() == [F(0.3), 0.0, 0.0, F(0.3)], sp["cov"][r]
        img = orc.composite(sp[r:r + 1], pc.W, pc.H)
        lit = np.argwhere((img != np.array([0, 0, 0, 1], F)).any(axis=-1))
        print("alpha %-5s = %.9g: the oracle lights %d pixel(s)" % (name, alpha, lit.shape[0]))
        assert bool(drawn[r]) == (name in ("succ", "one"))
        if name in ("pred", "exact"):
            assert lit.shape[0] == 0
        if name == "succ":
            assert lit.tolist() == [[pc.H // 2, pc.W // 2]]
        if name == "one":
            assert lit.shape[0] > 1


# ---- rectangle edges -------------------------------------------------------------------------------------------------------------

def test_rectangle_edges():
    aos, vw, wanted = pc.rect_edges_case()
    ref, mine = both(aos, vw)
    sp = ref["splats"]
    assert ref["V"] == aos.shape[0] == 128
    rank = np.empty(128, np.int64)
    rank[ref["sorted_idx"]] = np.arange(128)
    edges = pc.footprint_edges(sp)
    for j, (axis, side, t) in enumerate(wanted):
        got = edges[2 * axis + (0 if side < 0 else 1)][rank[j]]
        assert sp["reject"][rank[j]] == 0
        assert abs(got - round(t)) < 1e-3 and (got > round(t)) == (t > round(t)), (axis, side, t, got)
    n = len(wanted)
    drawn, tx0, ty0, tx1, ty1 = oracle_rects(sp, pc.W, pc.H)
    off, whole, zero = (rank[n + a:n + b] for a, b in ((0, 16), (16, 20), (20, 24)))
    assert (sp["reject"][off] == 0).all() and not drawn[off].any()
    ndc = np.abs(sp["ndc"][off, :2]).max(axis=1)
    assert ((ndc >= 1.19) & (ndc < 1.5)).all(), ndc
    bx, by = (pc.W - 1) // 32, (pc.H - 1) // 32
    assert drawn[whole].all() and (tx0[whole] == 0).all() and (ty0[whole] == 0).all() and (tx1[whole] == bx).all() and (ty1[whole] == by).all()
    assert drawn[zero].all() and (sp["cov"][zero] == np.array([0.3, 0, 0, 0.3], F)).all()
    # a footprint that ends within EDGE_DELTA of the first or last pixel from outside lights nothing; from inside, it does
    assert drawn[rank[:n]].sum() < n


# ---- colour ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("look", range(len(pc.COLOUR_LOOKS)))
def test_colour_case(look):
    aos, vw, dirs = pc.colour_case(look)
    for srgb in (False, True):
        ref, mine = both(aos, vw, srgb=srgb)
        assert ref["V"] == aos.shape[0] and (ref["splats"]["reject"] == 0).all()
    ref, mine = both(aos, vw)
    assert sorted(sorted(np.abs(d).tolist()) for d in dirs).count([0.0, 0.0, 1.0]) == 1
    assert sum(1 for d in dirs if np.count_nonzero(d) == 2) == 4 and sum(1 for d in dirs if np.count_nonzero(d) == 3) == 4
    sh = np.abs(aos[:2 * len(dirs)][:, np.r_[4:16, 25:61]])
    assert sh.min() >= 1e-3 and sh.max() <= 1e2 and (np.log10(sh.max()) - np.log10(sh.min())) > 4.5
    rgb = np.empty((aos.shape[0], 3), F)
    rgb[ref["sorted_idx"]] = ref["splats"]["rgb"]
    flat = rgb[2 * len(dirs):]
    assert flat.min() <= -1.99 and flat.max() >= 3.99
    below, above = flat[flat <= pc.SRGB_EDGE], flat[flat > pc.SRGB_EDGE]
    gap = [(int(pc._ord(v)) - int(pc._ord(pc.SRGB_EDGE))) for v in (below.max(), above.min())]
    print("colour look %d: nearest colours to the sRGB knee 0.04045: %+d and %+d ulps (0.5 + s lies on a grid of 8 ulps there)" % (look, *gap))
    assert -8 <= gap[0] <= 0 < gap[1] <= 8, gap


def test_every_axis_and_diagonal_is_a_view_direction():
    seen = set()
    for look in range(len(pc.COLOUR_LOOKS)):
        seen |= {tuple(int(v) for v in d) for d in pc.colour_case(look)[2]}
    want = {(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)} - {(0, 0, 0)}
    assert seen == want, want - seen


# ---- non-finite attributes and counts ----------------------------------------------------------------------------------------------

def test_nonfinite_geometry_is_rejected_and_neighbours_are_ordinary():
    aos, vw, where = pc.nonfinite_geometry_case()
    ref, mine = both(aos, vw)
    sp = ref["splats"]
    poisoned = np.array([i for i, _, _ in where])
    vis = np.isin(poisoned, ref["sorted_idx"])
    rank = {int(i): r for r, i in enumerate(ref["sorted_idx"])}
    drawn = oracle_rects(sp, pc.W, pc.H)[0]
    for (i, field, v), seen in zip(where, vis):
        state = "culled by Sort"
        if seen:
            r = rank[i]
            state = "rejected, class %s" % rule.CLASS_NAMES[mine["cls"][r]] if sp["reject"][r] else "accepted"
            assert not drawn[r], (i, field, v)
            if field.startswith("cov"):
                assert mine["cls"][r] == rule.Q, (field, v)
        print("non-finite %-6s = %-4s at upload index %3d: %s" % (field, v, i, state))
    assert vis.sum() >= 9, "only %d of the poisoned splats reach the projection" % vis.sum()
    others = ~np.isin(ref["sorted_idx"], poisoned)
    assert others.sum() >= 128 and (sp["reject"][others] == 0).all() and np.isfinite(sp["inv"][others]).all()
    assert len({i // 64 for i in poisoned}) == 4                     # every wave of the upload order has some


def test_nonfinite_colour_is_drawn():
    aos, vw, where = pc.nonfinite_colour_case()
    ref, mine = both(aos, vw)
    rank = {int(i): r for r, i in enumerate(ref["sorted_idx"])}
    for i, field, v in where:
        s = ref["splats"][rank[i]]
        assert s["reject"] == 0, (i, field, v)
        assert not np.isfinite(s["alpha"] if field == "alpha" else s["rgb"]).all(), (i, field, v, s["rgb"])


@pytest.mark.parametrize("V", pc.COUNTS)
def test_counts(V):
    for stride, rem in ((1, 0), (8, 3)):
        aos, vw = pc.count_case(V, stride, rem)
        ref, mine = both(aos, vw)
        assert ref["V"] == V, (ref["V"], V)
        assert (ref["sorted_idx"] % stride == rem).all()
        assert (ref["splats"]["reject"] == 0).all()
