"""CPU check of the inputs and models of tests/test_gpu_compositor_limits.py: every claim of tests/compositor_limit_cases.py, from the
oracle's projection (orc.render_frame(..., want_splats=True)) and binning_limit_cases.model_lists over the oracle's rectangles.
Nothing here touches a GPU.

Per case: every splat passes the Sort and rank = upload index; the lists have the designed lengths; at most 2 % of the evaluated
pixels need the flip budget; blend_lists over the model's lists equals orc.composite_f64 over ALL splats to (1e-12 + 8 x 2^-53 S) max(1, |c|) on every
evaluated pixel (S: the largest magnitude in a lit fragment's exponent, 126 near the centre: float64's own cancellation), and every pixel it did not evaluate is exactly clear there (viewports up to 2048 px: the float64 frame of a larger
one is 300 MB and more; the model's code path does not depend on the size); E_ref = max |fp32_reference_form - blend_lists| outside
budget pixels is printed and finite.  Per family: the batch after which each strip dies, with margins (walk: T below t_eps / 4 or
above 4 t_eps at every batch boundary); the designed maxima of e of tile_test; the chosen fragments of threshold; the tiles the
conditioning needles cross, at most three per tile; the strips of 17 x 5 that lie outside the image.

What a mistake in the kernel would change is shown on the model, as tests/test_binning_limits_fixtures.py does (the four were also
tried once on the device, as scratch builds with one line changed each: EXPERIMENTS.md round 30):
  the sign of c4         blend_lists with B negated leaves the GPU test's bound on batch_edges, tile_test and conditioning
  the `any` strip test   walk(any_test=False) counts more records than walk's upper bound on saturation_bar: probe word 1 sees it
  the 0.05 slack at -0.2 the needles aimed at -8 + 0.12 light their tile's corner pixel by more than the bound at 0 and 500 px
  pass 1's cnt < 64 stop saturation_edge: 30 of bin A's entries lie above occ_cut(1100, 1/64) = 1024, 74 below; a pass 1 that starts
                         on them moves the batch boundary from entry 64 to entry 30, behind which t_epsilon = 1/64 ends the walk in
                         the single pass: entries 64 ... 93, opaque and bright, would be blended at T ~ 1e-3

A finding on the way, in the projection and not in the compositor: the float32 determinant m00 m11 - m01 m10 of a 45-degree needle
cancels -- relative error ~ 2^-23 sigma_long^2 / (short variance) -- so the conic of a needle of sigma 1000 px and short variance
0.5 px^2 is off by up to 12 %, of sigma 3000 px by more than the whole (the determinant can come out negative and the library rejects
the splat).  The oracle and the library round alike there (the records agree), so nothing fails; but the long sigmas stop at 2000 px
here, not at 3000, and the designed maxima of tile_test_2000 are met to +-1 only, which is asserted as such."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import binning_limit_cases as blc
from tests import compositor_limit_cases as clc
from tests.render_cases import oracle_rects, window_depth


@functools.lru_cache(maxsize=2)
def prepared(name):
    """(case, oracle splats, model lists, records, window depths) of a case, computed once and left unchanged"""
    case = clc.CASES[name]()
    assert case.name == name
    cam, proj, vp, nf = case.view
    W, H = vp[2], vp[3]
    ref = orc.render_frame(clc.cloud_of(case).as_array(), False, cam, proj, vp, nf, nthreads=8, want_image=False, want_splats=True)
    n = case.claims["n"]
    assert ref["V"] == n, "%d of %d splats pass the Sort" % (ref["V"], n)
    np.testing.assert_array_equal(ref["sorted_idx"], np.arange(n))             # rank = upload index
    sp = ref["splats"]
    assert (sp["reject"] == 0).all()
    drawn, tx0, ty0, tx1, ty1 = oracle_rects(sp, W, H)
    rects = np.stack([tx0, ty0, tx1, ty1], axis=1)
    rects[~drawn] = blc.EMPTY
    ts, pairs = blc.model_lists(rects, *clc.tiles_of(W, H))
    rec, zw = clc.rec12_of(sp), window_depth(sp)
    assert np.isfinite(rec).all()
    for a in (sp, ts, pairs, rec, zw):
        a.setflags(write=False)
    return case, sp, ts, pairs, rec, zw


@functools.lru_cache(maxsize=2)
def modelled(name):
    case, sp, ts, pairs, rec, zw = prepared(name)
    W, H = case.view[2][2], case.view[2][3]
    m = clc.blend_lists(rec, ts, pairs, W, H, zw)
    E = clc.reference_error(m, clc.fp32_reference_form(rec, ts, pairs, W, H, zw))
    return m, E


@pytest.mark.parametrize("name", list(clc.CASES))
def test_model_and_budget(name):
    case, sp, ts, pairs, rec, zw = prepared(name)
    W, H = case.view[2][2], case.view[2][3]
    m, E = modelled(name)
    lengths = np.diff(ts.astype(np.int64))
    if case.claims["lengths"] is not None:
        np.testing.assert_array_equal(lengths, case.claims["lengths"])
    evaluated, flagged = int(m["valid"].sum()), int(m["flagged"].sum())
    print("%s: %d splats, %d pairs, %d of %d bins evaluated, %d of %d pixels in the flip band (%.3f %%), E_ref colour %.3g, T %.3g, depth %.3g -- %s"
          % (name, case.claims["n"], pairs.size, m["bins"].size, lengths.size, flagged, evaluated, 100.0 * flagged / evaluated,
             E["colour"], E["T"], E["depth"], case.claims["reaches"]))
    assert evaluated > 0 and flagged <= 0.02 * evaluated
    assert all(np.isfinite(v) for v in E.values())
    for k in ("colour", "T", "depth", "budget", "budget1"):
        assert np.isfinite(m[k]).all(), k
    assert (m["T"] >= 0).all() and (m["T"] <= 1).all() and (m["depth"] >= 0).all() and (m["depth"] <= 1.0 + 1e-12).all()
    if max(W, H) <= 2048:
        # the model, independently: float64 records without project_kernel's roundings against the oracle's float64 compositor
        m64 = clc.blend_lists(clc.rec12_of(sp, np.float64), ts, pairs, W, H)
        f64 = orc.composite_f64(sp, W, H, nthreads=8)
        got, other = clc.blocks(f64, m64["bins"], W, H)
        d = np.abs(got[..., :3] - m64["colour"]) / np.maximum(1.0, m64["cmax"])[:, None, None]
        # (1e-12, plus what float64 itself owes an exponent whose terms reach S: two forms of e differ by a few 2^-53 S)
        tol = 1e-12 + 8.0 * 2.0 ** -53 * m64["smax"]
        print("%s: blend_lists against composite_f64: %.3g (largest S %.3g: tolerance %.3g)" % (name, d[m64["valid"]].max(), m64["smax"], tol))
        assert d[m64["valid"]].max() <= tol
        assert (f64[other][:, :3] == 0).all() and (f64[other][:, 3] == 1).all()


def corrupted(name, what):
    """does the model of a kernel with the mistake leave the bound of the GPU test somewhere?  (colour, default t_epsilon)"""
    case, sp, ts, pairs, rec, zw = prepared(name)
    W, H = case.view[2][2], case.view[2][3]
    m, E = modelled(name)
    bad = np.array(rec)
    if what == "c4":
        bad[:, 3] = -bad[:, 3]
    wrong = clc.blend_lists(bad, ts, pairs, W, H, zw, kept=clc.kept_lists(rec, ts, pairs, W, H))
    over = np.abs(wrong["colour"] - m["colour"]) > clc.bound_of(m, E, clc.T_EPS_DEFAULT)[0][..., None]
    return int((over & m["valid"][..., None]).sum())


@pytest.mark.parametrize("name", ["batch_edges_0", "tile_test_0", "conditioning_100", "conditioning_1000", "ragged_333x211"])
def test_the_sign_of_c4_is_noticed(name):
    n = corrupted(name, "c4")
    print("%s: %d colour values leave the bound when B changes its sign" % (name, n))
    assert n > 100


# ---- batch_edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", [0, 1])
def test_batch_edges(frame):
    case, sp, ts, pairs, rec, zw = prepared("batch_edges_%d" % frame)
    wk = clc.walk(rec, ts, pairs, 96, 64, clc.T_EPS_DEFAULT)
    assert len(wk) == 24
    for (b, q), (length, batches, lo, hi, safe, _) in wk.items():
        assert length == clc.BATCH_LENGTHS[frame][b] and batches == -(-length // 64) and safe and lo <= hi, (b, q, length, batches, safe)
    col = sp["rgb"]
    assert (col < 0).any() and np.abs(col).max() > 5e3                          # unclamped: negative, and 1e4
    huge = np.unique((pairs[ts[clc.HUGE_BIN]:ts[clc.HUGE_BIN + 1]] & clc.RANK_MASK))
    assert np.abs(col[np.setdiff1d(np.arange(col.shape[0]), huge)]).max() < 10.0      # ... in one bin only
    assert (sp["alpha"] < 0.04).all()


# ---- saturation ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", clc.SATURATION)
def test_saturation(variant):
    case, sp, ts, pairs, rec, zw = prepared("saturation_" + variant)
    W, H = case.view[2][2], case.view[2][3]
    for te in clc.T_EPS:
        wk = clc.walk(rec, ts, pairs, W, H, te)
        print("%s, t_eps %g: %s" % (case.name, te, {k: v[:4] for k, v in wk.items()}))
        assert all(v[4] for v in wk.values()), "a strip's T sits within a factor 4 of t_eps at a batch boundary"
        if case.claims["batches"] is not None:
            assert all(v[1] == case.claims["batches"][te] for k, v in wk.items() if k[0] == 0), (te, case.claims["batches"])
    if variant == "exact":
        m, _ = modelled(case.name)
        assert (sp["alpha"][-2:] == 1.0).all()
        for x, y in ((8, 8), (24, 20)):
            assert m["T"][0, y * 32 + x] == 0.0                                   # T is exactly 0 on the two pixel centres
    if variant == "bar":
        # strip 0 of every tile is dead after the bars, strips 1 ... 3 are not; the records behind that reach strip 0 only are
        # dropped: 20 per tile.  A walk without the `any` test stages more than the upper bound of the walk with it
        te = clc.T_EPS_DEFAULT
        with_any, without = clc.walk(rec, ts, pairs, W, H, te), clc.walk(rec, ts, pairs, W, H, te, any_test=False)
        for k in with_any:
            assert with_any[k][1] == without[k][1] == 5
            assert without[k][2] >= with_any[k][3] + 15, (k, with_any[k], without[k])
        m, _ = modelled(case.name)
        T = m["T"][0].reshape(32, 32)
        for ty in range(2):
            assert T[16 * ty:16 * ty + 4].max() < te / 4 and all(T[16 * ty + 4 * k:16 * ty + 4 * k + 4].max() > 4 * (1.0 / 64.0) for k in (1, 2, 3))
    if variant == "edge":
        # the two-pass cut: 76 splats above it, 30 of them in bin A's list (its nearest), 46 in bin B's only
        assert case.claims["n"] == clc.EDGE_V and (clc.EDGE_V - 64) & ~1023 == clc.EDGE_CUT
        a = pairs[ts[0]:ts[1]] & clc.RANK_MASK
        assert (a >= clc.EDGE_CUT).sum() == 30 and (a[-30:] >= clc.EDGE_CUT).all()
        # what the single pass skips with t_eps = 1/64 is visible: the model's T after A's first batch times the bright colour
        m, _ = modelled(case.name)
        first = a[::-1][:64]
        T1 = np.prod(1.0 - blc.alpha_of(case.claims["table"][first, 5]))
        print("saturation_edge: T after bin A's first batch ~ %.3g" % T1)
        assert 4 * clc.T_EPS_DEFAULT < T1 < (1.0 / 64.0) / 4           # times alpha 0.99 and colours of 2 ... 4: ~4e-3, no rounding error


# ---- tile_test -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", list(clc.TILE_DISTANCES))
def test_tile_test(d):
    case, sp, ts, pairs, rec, zw = prepared("tile_test_%d" % d)
    W = case.view[2][2]
    aims = case.claims["aims"]
    k, x0, y0, target = aims[:, 0].astype(int), aims[:, 1], aims[:, 2], aims[:, 3]
    r = np.asarray(rec, np.float64)[k]
    em = clc.emax_box(r, x0 + 0.5, x0 + 15.5, y0 + 0.5, y0 + 15.5)
    off = em - target
    print("tile_test_%d: the designed maxima are met to %.3g (mean |.| %.3g)" % (d, np.abs(off).max(), np.abs(off).mean()))
    # the maximum is taken at a corner of the box: the needle passes outside
    corners = np.stack([clc.emax_box(r, cx, cx, cy, cy) for cx in (x0 + 0.5, x0 + 15.5) for cy in (y0 + 0.5, y0 + 15.5)])
    assert np.abs(corners.max(axis=0) - em).max() <= 1e-9
    centre_dist = np.hypot(r[:, 0] - (x0 + 8), r[:, 1] - (y0 + 8))
    assert np.abs(centre_dist - d).max() <= 16.0
    if d < 2000:
        assert np.abs(off).max() <= 0.05
        assert ((em > -8.15) & (em < -7.9)).sum() == 0 and (np.abs(em + 7.88) <= 0.05).sum() == 12
    else:
        # the projection's float32 determinant moves the conic (module docstring): both sides of the slack stay populated
        assert np.abs(off).max() <= 1.0 and (em > -7.9).sum() >= 12 and (em < -8.15).sum() >= 12
    # dust: listed (drawn), and e <= -8.3 at every pixel centre: it lights nothing
    dust = case.claims["dust"]
    rd = np.asarray(rec, np.float64)[dust]
    qx, qy = np.round(rd[:, 0]), np.round(rd[:, 1])
    near = np.stack([clc.emax_box(rd, qx + ox, qx + ox, qy + oy, qy + oy) for ox in (-0.5, 0.5) for oy in (-0.5, 0.5)])
    assert np.abs(rd[:, 0] - qx).max() < 1e-3 and near.max() < -8.3
    listed = np.unique(pairs & clc.RANK_MASK)
    assert np.isin(dust, listed).all()
    if d < 2000:
        # a slack of -0.2 (emax > -7.8) would drop the needles aimed at -7.88: their corner pixel is lit by more than the bound
        m, E = modelled(case.name)
        sel = np.abs(target + 7.88) < 1e-9
        w = np.exp2(em[sel]) * np.abs(r[sel, 6:9]).max(axis=1)
        bound = 1e-4 + 2 * E["colour"] + clc.T_EPS_DEFAULT
        print("tile_test_%d: the -7.88 needles light their corner by %.3g ... %.3g, bound %.3g" % (d, w.min(), w.max(), bound))
        assert (w > bound).all() if d == 0 else (w > bound).any()


# ---- threshold -----------------------------------------------------------------------------------------------------------------

def test_threshold():
    case, sp, ts, pairs, rec, zw = prepared("threshold")
    aims = case.claims["aims"]
    r = np.asarray(rec, np.float64)[aims[:, 0].astype(int)]
    e = clc.emax_box(r, aims[:, 1], aims[:, 1], aims[:, 2], aims[:, 2])
    print("threshold: e + 8 at the chosen pixels: %s" % np.round(e + 8.0, 5))
    assert np.abs(e + 8.0 - aims[:, 3]).max() <= 2e-4 and (np.sign(e + 8.0) == np.sign(aims[:, 3])).all()
    m, _ = modelled("threshold")
    tiles_x = 3
    for px, py in aims[:, 1:3]:
        b = int(py // 32) * tiles_x + int(px // 32)
        i = int(np.flatnonzero(m["bins"] == b)[0])
        assert not m["flagged"][i, (int(py) % 32) * 32 + int(px) % 32]            # outside the rounding band: the verdict is owed


# ---- conditioning --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", clc.CONDITIONING_D)
def test_conditioning(d):
    case, sp, ts, pairs, rec, zw = prepared("conditioning_%d" % d)
    W = case.view[2][2]
    aims = case.claims["aims"]
    r = np.asarray(rec, np.float64)
    inside = (r[:, 0] >= 0) & (r[:, 0] < W) & (r[:, 1] >= 0) & (r[:, 1] < W)
    assert inside.sum() == 12 and np.array_equal(~inside, aims[:, 3] != 0)
    assert np.abs(np.hypot(r[:, 0] - aims[:, 1], r[:, 1] - aims[:, 2]) - d).max() < 0.01
    # the tile around Q, d px from the centre, is lit by its needle
    x0, y0 = np.floor(aims[:, 1] / 16) * 16, np.floor(aims[:, 2] / 16) * 16
    lit = clc.emax_box(r, x0 + 0.5, x0 + 15.5, y0 + 0.5, y0 + 15.5)
    print("conditioning_%d: max e over the tile at %d px: %s" % (d, d, np.round(lit, 2)))
    assert (lit > -7.0).sum() >= 20
    # three needles per tile at most
    t = np.arange(W // 16) * 16.0
    X0, Y0 = np.meshgrid(t, t)
    count = np.zeros(X0.shape, int)
    for k in range(r.shape[0]):
        count += clc.emax_box(r[k], X0 + 0.5, X0 + 15.5, Y0 + 0.5, Y0 + 15.5) > -8.0
    print("conditioning_%d: tiles lit by 1, 2, 3 needles: %s" % (d, [int((count == c).sum()) for c in (1, 2, 3)]))
    assert count.max() <= 3 and (count >= 1).sum() > 500
    assert (sp["cov"][:, 0] + sp["cov"][:, 3] > 0.9 * max(100.0, 0.5 * d) ** 2).all()


# ---- ragged --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", clc.RAGGED)
def test_ragged(W, H):
    case, sp, ts, pairs, rec, zw = prepared("ragged_%dx%d" % (W, H))
    m, _ = modelled(case.name)
    assert int(m["valid"].sum()) <= W * H and ts[-1] > 0
    wk = clc.walk(rec, ts, pairs, W, H, clc.T_EPS_DEFAULT)
    assert len(wk) == -(-W // 16) * -(-H // 16)
    if (W, H) == (17, 5):
        assert sorted(wk) == [(0, 0), (0, 1)] and m["valid"].sum() == 85         # rows 0 ... 4: strip 0 and one row of strip 1
    assert (m["colour"][m["valid"]] != 0).any()
