"""composite_kernel's blend at its limits: designed lists against a float64 blend of the GPU's own records and lists.

The rest of the suite sees the compositor's arithmetic through whole frames of random clouds under check_image, which lets 0.1 % of
the values be anywhere up to 5e-3.  Here every case of tests/compositor_limit_cases.py (tests/test_compositor_limits_fixtures.py
asserts its claims on the CPU) is rendered into an fp32 device target in CLEAR and PREMULTIPLIED (alpha = 1 - T) and once more with
the depth plane; records, rectangles and lists are taken back from the same context, and EVERY value is held to

    |img - blend_lists| <= 1e-4 max(1, max|c|) + 2 E_ref + t_eps max|c| + flip budget        (T and the depth plane: c = 1)

with blend_lists the float64 blend of those records over those lists, E_ref the distance of the oracle's float32 operation order
from it on the same records (per quantity, measured against the reference and never against the kernel), max|c| per bin.  Pixels of
bins the model does not evaluate are exactly clear.  The lists have the designed lengths, or list every needle in the bin it is aimed
at: the test proves which regime it ran in.  -rP prints worst error, E_ref and their ratio.

Probe (batch_edges, saturation, tile_test): a probed context's pixels are the plain context's; per work item -- rows mapped to (bin,
quadrant) through bin_order() and the kernel's 8 x 4 mapping -- word 6 is the list length, word 2 the batches compositor_limit_cases.
walk designs, word 1 lies between walk's lower and upper count of staged records.
Execution shapes: every case as a two-pass frame with the share pinned to 1/64, 0.3 and 0.9 (two_pass_info proves the two passes),
one batch_edges and one saturation frame through RenderStereo with the same camera twice and on compositor_waves = 64: all
bit-identical to the plain frame.

MEASURED on the MI355X (EXPERIMENTS.md, round 30, has every case): the module runs in 21 s, its slowest test in 2.8 s.  Worst
colour error outside the flip band, E_ref and their ratio on `conditioning` -- nobody had measured these ratios before.  "before": the
kernel as this module found it, c0 = (A a + B b) a + C b b + log2 alpha - 118 in plain float32:

    needle crosses tiles at   before    E_ref     ratio    now       ratio
    100 px                    2.8e-4    3.6e-4    0.77     2.6e-4    0.72
    500 px                    2.3e-3    1.8e-3    1.24     5.3e-4    0.29
    1000 px                   1.1e-2    9.9e-3    1.13     2.0e-4    0.020
    2000 px                   3.9e-2    3.7e-2    1.04     5.0e-4    0.013
    4000 px                   0.154     0.153     1.00     1.1e-3    0.0073

Not 0.3 to 0.7 of the reference form, as a CPU emulation had suggested: c0 cancels like the centre-relative form does.  Every value
was inside its bound all the same (the bound holds E_ref twice), but test_probe_counts_what_the_walk_designs[tile_test_2000] was not:
of 3832 walked work items one (bin 3698, quadrant 2) staged a needle whose float64 maximum of e over the tile is -8.161 -- float32
had moved the exact footprint-against-tile test by 0.111 where the bound allows 0.1 (and the same error the other way drops a needle
of w up to 2^-7.9).  THE FIX is in composite_kernel: a batch that holds a record more than 128 px from the tile's centre evaluates
c0 as a compensated float32 sum: the column "now".  With it all 91 tests pass; EXPERIMENTS.md has the benchmark
beside the parent's.  Near the centre the biased exponent costs more than the reference form loses (ratios of 10 ... 100
on saturation, threshold and ragged), at absolute errors of 1.4e-5 and less: the 1e-4 floor."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import _capi
from tests import compositor_limit_cases as clc
from tests.checks import same_bits
from tests.gpu_harness import bin_edge, device_frame, make_renderer, no_sentinel, stereo_frame
from tests.render_cases import window_depth

pytestmark = pytest.mark.gpu

RUNS = [(name, te) for name in clc.CASES for te in clc.t_eps_of(name)]
SHARES = (1.0 / 64.0, 0.3, 0.9)


def run_id(run):
    return "%s-t_eps_%g" % run


def probed_runs():
    return [(name, te) for name, te in RUNS if name.startswith(("batch_edges", "saturation", "tile_test"))]


@functools.lru_cache(maxsize=2)
def prepared(name):
    """(case, cloud, window depth per rank from the oracle's projection), computed once"""
    case = clc.CASES[name]()
    cam, proj, vp, nf = case.view
    cloud = clc.cloud_of(case)
    ref = orc.render_frame(cloud.as_array(), False, cam, proj, vp, nf, nthreads=16, want_image=False, want_splats=True)
    assert ref["V"] == case.claims["n"]
    zw = window_depth(ref["splats"])
    zw.setflags(write=False)
    return case, cloud, ref["splats"], zw


def plain_frame(r, case):
    r.Sort(*case.view)
    img = device_frame(r, case.view, "clear", None, call=r.Render, **bin_edge())
    no_sentinel(img)
    return img


def held(what, err, bound, ok, E):
    """every value within its bound; prints the worst error outside the flip band, E_ref and their ratio"""
    worst = float(err[ok].max()) if ok.any() else 0.0
    print("%s: worst error %.3g, E_ref %.3g, ratio %s" % (what, worst, E, "%.3g" % (worst / E) if E > 0 else "-"))
    over = err > bound
    assert not over.any(), "%s: %d value(s) above their bound, worst excess %.3g (error %.3g)" % (what, over.sum(), (err - bound)[over].max(), err[over].max())


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_every_value_against_the_float64_blend_of_the_own_lists(run):
    name, te = run
    case, cloud, sp, zw = prepared(name)
    W, H = case.view[2][2], case.view[2][3]
    n = case.claims["n"]
    r = make_renderer(cloud, t_epsilon=te)
    assert r.storage_order() is None
    clear = plain_frame(r, case)
    pm = device_frame(r, case.view, "premultiplied", None, call=r.Render, **bin_edge())
    again, z = device_frame(r, case.view, "clear", None, call=r.Render, depth=True, **bin_edge())
    same_bits(again, clear, "%s: the frame with a depth plane" % name)
    assert r.sort_count() == n
    np.testing.assert_array_equal(r.sorted_indices(), np.arange(n))                # rank = upload index
    rec, rect = r.debug_projected()
    ts, pairs = r.debug_tile_lists()
    assert r.verify_order() == (0, 0)
    r.close()
    np.testing.assert_array_equal(rec[:, 9], sp["alpha"])

    # which regime ran: the designed lengths; or every aimed point's bin lists its splat, and the (bin, splat) pairs that the record's
    # own conic lights (float64 maximum of e over the bin above -8) but the library's rectangle leaves out are counted and printed:
    # that is the projection's finding (module docstring), not the compositor's
    lengths = np.diff(ts.astype(np.int64))
    if case.claims["lengths"] is not None:
        np.testing.assert_array_equal(lengths, case.claims["lengths"])
    else:
        tiles_x, tiles_y = clc.tiles_of(W, H)
        bx, by = np.meshgrid(np.arange(tiles_x), np.arange(tiles_y))
        have = np.zeros((n, tiles_y * tiles_x), bool)
        have[pairs & clc.RANK_MASK, np.repeat(np.arange(lengths.size), lengths)] = True
        missing = 0
        for k in range(n):
            need = clc.emax_box(rec[k], bx * 32 + 0.5, np.minimum(bx * 32 + 32, W) - 0.5, by * 32 + 0.5, np.minimum(by * 32 + 32, H) - 0.5) > -8.0
            missing += int((need.reshape(-1) & ~have[k]).sum())
        print("%s: %d (bin, splat) pair(s) that the record's conic lights lie outside the library's rectangle" % (name, missing))
        aims = case.claims.get("aims")
        if aims is not None:
            ax, ay = (aims[:, 1] + (8 if name.startswith("tile_test") else 0)), (aims[:, 2] + (8 if name.startswith("tile_test") else 0))
            inside = (ax >= 0) & (ax < W) & (ay >= 0) & (ay < H)
            b = (ay[inside] // 32).astype(np.int64) * tiles_x + (ax[inside] // 32).astype(np.int64)
            assert have[aims[inside, 0].astype(np.int64), b].all(), "%s: an aimed bin does not list its splat" % name

    model = clc.blend_lists(rec, ts, pairs, W, H, zw)
    E = clc.reference_error(model, clc.fp32_reference_form(rec, ts, pairs, W, H, zw))
    bc, bT, bz = clc.bound_of(model, E, te)
    v, ok = model["valid"], model["valid"] & ~model["flagged"]
    what = "%s, t_eps %g" % (name, te)

    got, other = clc.blocks(clear, model["bins"], W, H)
    assert (clear[..., 3] == 1.0).all() and not clear[other][:, :3].any(), "%s: a bin the model leaves clear is not" % what
    err = np.where(v[..., None], np.abs(got[..., :3].astype(np.float64) - model["colour"]), 0.0)
    held(what + ", colour", err, bc[..., None], np.broadcast_to(ok[..., None], err.shape), E["colour"])

    same_bits(pm[..., :3], clear[..., :3], "%s: the premultiplied layer's colour" % what)
    gotp, _ = clc.blocks(pm[..., 3], model["bins"], W, H)
    assert not pm[other].any(), "%s: a bin the model leaves clear is not (premultiplied)" % what
    held(what + ", T", np.where(v, np.abs(1.0 - gotp.astype(np.float64) - model["T"]), 0.0), bT, ok, E["T"])

    gotz, _ = clc.blocks(z, model["bins"], W, H)
    assert (z[other] == 1.0).all() and (z >= 0.0).all() and (z <= 1.0).all()
    held(what + ", depth plane", np.where(v, np.abs(gotz.astype(np.float64) - model["depth"]), 0.0), bz, ok, E["depth"])

    if name == "saturation_exact":
        assert pm[8, 8, 3] == 1.0 and pm[20, 24, 3] == 1.0                         # alpha 1.0f on a pixel centre: T is exactly 0
    print("%s: %d pairs, %d bins evaluated, %d pixels in the flip band -- %s" % (what, pairs.size, model["bins"].size, model["flagged"].sum(), case.claims["reaches"]))


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_two_pass_frames_are_the_plain_frame(run):
    """the share pinned to 1/64, 0.3 and 0.9 (below 1024 + 64 splats the cut is 0: pass 1 walks the whole list and must stop in front
    of its last, incomplete batch; saturation_edge has its cut at 1024 with share 1/64)"""
    name, te = run
    case, cloud, sp, zw = prepared(name)
    r = make_renderer(cloud, t_epsilon=te, two_pass=_capi.TWO_PASS_OFF)
    want = plain_frame(r, case)
    assert r.two_pass_info() is None
    r.close()
    b = make_renderer(cloud, t_epsilon=te, two_pass=_capi.TWO_PASS_ON)
    for k, share in enumerate(SHARES):
        b.two_pass_state(share)
        img = plain_frame(b, case)
        info = b.two_pass_info()
        assert info is not None and info["visible"] == case.claims["n"], (share, info)
        same_bits(img, want, "%s, t_eps %g, two passes at share %g" % (name, te, share))
    assert b.two_pass_state(SHARES[-1])[0] == len(SHARES)
    print("%s, t_eps %g: %s" % (name, te, info))
    b.close()


@pytest.mark.parametrize("run", [("batch_edges_1", clc.T_EPS_DEFAULT)] + [("saturation_edge", te) for te in clc.T_EPS], ids=run_id)
def test_stereo_and_short_pool_are_the_plain_frame(run):
    name, te = run
    case, cloud, sp, zw = prepared(name)
    cam, proj, vp, nf = case.view
    r = make_renderer(cloud, t_epsilon=te)
    want = plain_frame(r, case)
    r.close()
    s = make_renderer(cloud, t_epsilon=te)
    s.Sort(*case.view)
    for e, img in enumerate(stereo_frame(s, [cam, cam], [proj, proj], vp, nf, None, None, call=s.RenderStereo, **bin_edge())):
        same_bits(img, want, "%s, t_eps %g, eye %d" % (name, te, e))
    s.close()
    p = make_renderer(cloud, t_epsilon=te, compositor_waves=64)
    same_bits(plain_frame(p, case), want, "%s, t_eps %g, compositor_waves = 64" % (name, te))
    p.close()


def probe_rows(r, tiles_x, tiles_y):
    """(table, bin, quadrant) per work item of the latest probed render: composite_kernel's item -> (slot, quadrant) mapping -- the
    first items & ~31 items 8 bins x 4 quadrants, the tail plain -- and bin = order[slot]"""
    table, order = r.debug_tile_probe_table(), r.bin_order()
    items = table.shape[0]
    assert items == 4 * tiles_x * tiles_y and order.shape[0] == items // 4
    assert np.array_equal(np.sort(order), np.arange(items // 4))
    q = np.arange(items)
    mapped = q < (items & ~31)
    slot = np.where(mapped, (q >> 5) * 8 + (q & 7), q >> 2)
    quad = np.where(mapped, (q >> 3) & 3, q & 3)
    return table, order[slot].astype(np.int64), quad


@pytest.mark.parametrize("run", probed_runs(), ids=run_id)
def test_probe_counts_what_the_walk_designs(run):
    """(tile_test_2000 is the case that found c0's cancellation: with c0 in plain float32 one of its 3832 walked work items staged a
    record whose float64 emax is -8.161, 0.111 beyond the slack where the bound allows 0.1)"""
    name, te = run
    case, cloud, sp, zw = prepared(name)
    W, H = case.view[2][2], case.view[2][3]
    tiles_x, tiles_y = clc.tiles_of(W, H)
    r = make_renderer(cloud, t_epsilon=te)
    want = plain_frame(r, case)
    rec, _ = r.debug_projected()
    ts, pairs = r.debug_tile_lists()
    r.close()
    p = make_renderer(cloud, t_epsilon=te)
    p.set_tile_probe(True)
    same_bits(plain_frame(p, case), want, "%s, t_eps %g: the probe changed pixels" % (name, te))
    table, bins, quad = probe_rows(p, tiles_x, tiles_y)
    p.close()
    row_of = {(int(b), int(q)): i for i, (b, q) in enumerate(zip(bins, quad))}
    assert len(row_of) == table.shape[0]

    # every item: ran exactly when its tile lies in the image, and word 6 is its bin's list length
    x0, y0 = (bins % tiles_x) * 32 + (quad & 1) * 16, (bins // tiles_x) * 32 + (quad >> 1) * 16
    inside = (x0 < W) & (y0 < H)
    assert ((table[:, 7] != 0) == inside).all()
    lengths = np.diff(ts.astype(np.int64))
    np.testing.assert_array_equal(table[inside, 6], lengths[bins[inside]])

    # the walked items: all of a small frame; of a large one the bins of the aimed tiles and every fifth bin that keeps an entry
    kept, _ = clc.kept_lists(rec, ts, pairs, W, H)
    if kept.size > 1000:
        aims = case.claims["aims"]
        aimed = (aims[:, 2] // 32).astype(np.int64) * tiles_x + (aims[:, 1] // 32).astype(np.int64)
        kept = np.union1d(aimed, kept[::5])
        idle = np.setdiff1d(np.arange(tiles_x * tiles_y), clc.kept_lists(rec, ts, pairs, W, H)[0])
        sel = inside & np.isin(bins, idle)
        # a bin whose every entry stays below -8.5: nothing is staged, nothing saturates, every batch runs
        assert not table[sel, 1].any() and (table[sel, 2] == -(-lengths[bins[sel]] // 64)).all()
    wk = clc.walk(rec, ts, pairs, W, H, te, only_bins=kept if kept.size < tiles_x * tiles_y else None)
    widest, wrong = 0, []
    for (b, q), (length, batches, lo, hi, safe, inband) in wk.items():
        row = table[row_of[(b, q)]]
        assert safe, "bin %d quadrant %d: the design leaves float32 room to move a batch" % (b, q)
        assert row[6] == length and row[2] == batches, "bin %d quadrant %d: length %d, batches %d, designed %d and %d" % (b, q, row[6], row[2], length, batches)
        widest = max(widest, hi - lo)
        if not lo <= row[1] <= hi:
            # how far float32 moved the staging test: the float64 emax of the records next to the slack, against -8.05
            x0, y0 = (b % tiles_x) * 32 + (q & 1) * 16, (b // tiles_x) * 32 + (q >> 1) * 16
            em = np.sort(clc.emax_box(rec[pairs[ts[b]:ts[b + 1]] & clc.RANK_MASK], x0 + 0.5, x0 + 15.5, y0 + 0.5, y0 + 15.5))[::-1]
            moved = -8.05 - em[int(row[1]) - 1] if row[1] > hi else em[int(row[1])] + 8.05
            wrong.append((b, q, int(row[1]), lo, hi, float(moved)))
    print("%s, t_eps %g: %d work items walked, batches %s, widest [lo, hi] %d" % (name, te, len(wk), sorted({v[1] for v in wk.values()}), widest))
    if wrong:
        print("%s: %d of %d work items staged a count outside [lo, hi]; float32 moved the exact test by up to %.3g (the bounds allow 0.1): %s"
              % (name, len(wrong), len(wk), max(w[5] for w in wrong), wrong[:8]))
    assert not wrong, "%d work item(s): records staged outside the designed [lo, hi], first (bin, quadrant, staged, lo, hi, moved by) %s" % (len(wrong), wrong[0])
