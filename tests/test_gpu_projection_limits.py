"""project_kernel at its limits, on the device: the fixtures of tests/projection_limit_cases.py (tests/test_projection_limits_fixtures.py
checks on the CPU that they are what they claim) against the oracle's records, and the footprint rule of include/msplat.h --
class Q (the reference's quad is NaN) and class X (no Gaussian) draw nothing: empty rectangle, no pairs, no ids, no scores, no
depth -- as an exact statement about which ranks have a rectangle.  Every instantiation of the kernel (PROJ_PASS1, PROJ_LISTED,
PROJ_TWO_VIEWS, the fp16 and 8-bit stores, both SH widths) writes PROJ_PLAIN's records, bit for bit.

Shapes: at most 4097 splats, 353 x 301 pixels (12 x 10 bins), fp32 targets."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import _capi
from tests import projection_limit_cases as pc
from tests import projection_rule as rule
from tests.checks import bits, check_image, same_bits
from tests.gpu_harness import _check_projection, bin_px, make_renderer
from tests.render_cases import oracle_rects
from tests.sh_q8_rule import REST, deq

pytestmark = pytest.mark.gpu

W, H = pc.W, pc.H
ONE_PASS = dict(spatial_order=_capi.SPATIAL_OFF, two_pass=_capi.TWO_PASS_OFF)


def round16(aos):
    """the cloud the SH_FP16 store renders: f_rest rounded to IEEE fp16, everything else unchanged"""
    out = np.array(aos, np.float32, copy=True)
    out[:, REST] = out[:, REST].astype(np.float16).astype(np.float32)
    return out


def oracle_of(aos, vw, render=None, srgb=False, full_sh=True):
    """the oracle's Sort with view `vw` and projection with `render` (default: the same view)"""
    cam, proj, vp, nf = vw
    rcam, rproj, rvp, rnf = render or vw
    ref = orc.render_frame(aos, full_sh, cam, proj, vp, nf, render_cam=rcam, render_proj=rproj, srgb=srgb, nthreads=8,
                           want_image=False, want_splats=True)
    if render is not None:
        ref["splats"] = orc.project(ref["sorted_idx"], aos, full_sh, srgb, orc.mat4_inverse(rcam), rproj, rvp, rnf, np.asarray(rcam, np.float32)[12:15])
    return ref


def drawn_of(rect):
    return (rect & 255) <= ((rect >> 16) & 255)


def check_records(r, aos, vw, render=None, srgb=False, full_sh=True, what=""):
    """Sort + Render, then: visible set and order are the oracle's; _check_projection (centre, conic, colour, alpha, rectangle
    covers the oracle's footprint and is tight); and the drawn set, exactly: a rank with a rectangle is one the oracle does not
    reject and whose alpha is above 1/256, and every rank whose oracle footprint reaches a pixel (oracle_rects' mask) has one"""
    r.Sort(*vw)
    img = r.Render(*(render or vw))
    ref = oracle_of(aos, vw, render, srgb, full_sh)
    assert r.sort_count() == ref["V"], (what, r.sort_count(), ref["V"])
    np.testing.assert_array_equal(r.sorted_indices(), ref["sorted_idx"], err_msg=what)
    sp = ref["splats"]
    _, rect = r.debug_projected()
    drawn = drawn_of(rect)
    with np.errstate(invalid="ignore"):
        may = (sp["reject"] == 0) & (sp["alpha"] > np.float32(1.0 / 256.0))
    must = oracle_rects(sp, int(vw[2][2]), int(vw[2][3]), bin_px())[0]
    cls = orc.cov2_class(sp["cov"])
    wrong = drawn & ~may
    print("%s: V %d, drawn %d, must be drawn %d, may be drawn %d; drawn but rejected or faint: %d (class Q %d, X %d)" % (
        what, ref["V"], drawn.sum(), must.sum(), may.sum(), wrong.sum(), (wrong & (cls == rule.Q)).sum(), (wrong & (cls == rule.X)).sum()))
    assert not wrong.any(), "%s: %d rank(s) have a rectangle that the oracle rejects or whose alpha is <= 1/256 (class Q: %d, X: %d), e.g. rank %s" % (
        what, wrong.sum(), (wrong & (cls == rule.Q)).sum(), (wrong & (cls == rule.X)).sum(), np.flatnonzero(wrong)[:8])
    assert drawn[must].all(), "%s: %d rank(s) the oracle can light up have no rectangle" % (what, (~drawn[must]).sum())
    assert np.array_equal(drawn[must | ~may], must[must | ~may])          # the two as one exact statement, where it is decided
    _check_projection(r, ref, int(vw[2][2]), int(vw[2][3]))
    return ref, img, rect


# ---- records against the oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.LADDER_CAMERAS)
def test_ladder_records_and_the_exact_drawn_set(name):
    """(on the parent commit's kernel, which tested det > 0 only, this fails for every Q splat that is not faint: EXPERIMENTS.md)"""
    aos, vw = pc.ladder_cloud(name).as_array(), pc.view(name)
    r = make_renderer(aos, **ONE_PASS)
    ref, _, rect = check_records(r, aos, vw, what="ladder %s" % name)
    cls = orc.cov2_class(ref["splats"]["cov"])
    assert (cls != rule.G).sum() >= 32 and not drawn_of(rect)[cls != rule.G].any()
    r.close()


@pytest.mark.parametrize("near", pc.THRESHOLD_NEARS)
def test_threshold_neighbours(near):
    aos, labels = pc.threshold_case(near)
    sort, render = pc.threshold_views(near)
    r = make_renderer(aos, **ONE_PASS)
    ref, img, rect = check_records(r, aos, sort, render=render, what="thresholds, near %g" % near)
    assert np.isfinite(img).all()
    # every ordinary neighbour is drawn or off screen; nothing on the rejecting side of a threshold has a rectangle
    rej = np.zeros(aos.shape[0], bool)
    rej[ref["sorted_idx"]] = ref["splats"]["reject"] != 0
    has = np.zeros(aos.shape[0], bool)
    has[ref["sorted_idx"]] = drawn_of(rect)
    assert not (has & rej).any()
    assert has[[i for i, (n, _) in enumerate(labels) if n == "plain"]].sum() >= 32
    r.close()


def test_alpha_thresholds():
    aos, vw = pc.alpha_case()
    r = make_renderer(aos, **ONE_PASS)
    ref, img, rect = check_records(r, aos, vw, what="alpha thresholds")
    has = np.zeros(aos.shape[0], bool)
    has[ref["sorted_idx"]] = drawn_of(rect)
    assert has[:4].tolist() == [False, False, True, True], has[:4]        # pred(1/256), 1/256, succ(1/256), 1
    r.close()
    # succ(1/256) alone: the oracle lights exactly one pixel, so the rectangle is not empty.  Whether the compositor lights it is
    # a threshold flip -- it evaluates w = exp2(q + log2 alpha), and log2f(succ(1/256)) is -8 exactly, so w = 1/256 is discarded
    # (measured on the MI355X: no pixel lit) -- which the comparator's flip budget covers; no other pixel may be touched
    one = np.ascontiguousarray(aos[2:3])
    r = make_renderer(one, **ONE_PASS)
    r.Sort(*vw)
    img = r.Render(*vw)
    sp = oracle_of(one, vw)["splats"]
    want, budget = orc.composite_flip(sp, W, H)
    lit = np.argwhere((img != np.array([0, 0, 0, 1], np.float32)).any(axis=-1))
    print("alpha = succ(1/256) alone: the oracle lights %s, the frame %s" % (
        np.argwhere((want != np.array([0, 0, 0, 1], np.float32)).any(axis=-1)).tolist(), lit.tolist()))
    assert drawn_of(r.debug_projected()[1]).all()
    assert lit.tolist() in ([], [[H // 2, W // 2]]), lit
    check_image(img, want, budget=budget)
    r.close()


def test_rectangle_edges():
    aos, vw, wanted = pc.rect_edges_case()
    r = make_renderer(aos, **ONE_PASS)
    ref, img, rect = check_records(r, aos, vw, what="rectangle edges")
    image, budget = orc.composite_flip(ref["splats"], W, H)
    check_image(img, image, budget=budget)
    r.close()


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("look", range(len(pc.COLOUR_LOOKS)))
def test_colour(look, srgb):
    aos, vw, _ = pc.colour_case(look)
    r = make_renderer(aos, srgb=srgb, **ONE_PASS)
    ref, img, rect = check_records(r, aos, vw, srgb=srgb, what="colour look %d srgb %d" % (look, srgb))
    rec, _ = r.debug_projected()
    # (printed only: project_kernel evaluates the oracle's operations in the oracle's order, the sRGB curve with the device's powf)
    same = bits(rec[:, 6:9]) == bits(ref["splats"]["rgb"])
    print("colour look %d srgb %d: %d of %d colour values bit-equal to the oracle's" % (look, srgb, same.sum(), same.size))
    r.close()


def test_nonfinite_geometry():
    aos, vw, where = pc.nonfinite_geometry_case()
    r = make_renderer(aos, **ONE_PASS)
    ref, img, rect = check_records(r, aos, vw, what="non-finite geometry")
    assert np.isfinite(img).all()
    # the frame is that of the cloud without the poisoned splats, bit for bit
    keep = np.setdiff1d(np.arange(aos.shape[0]), [i for i, _, _ in where])
    clean = make_renderer(np.ascontiguousarray(aos[keep]), **ONE_PASS)
    clean.Sort(*vw)
    same_bits(img, clean.Render(*vw), "non-finite geometry: the frame without the poisoned splats")
    clean.close()
    r.close()


def test_nonfinite_colour():
    """NaN / inf in SH coefficients and alpha = +inf: drawn, as the reference draws them.  The records carry the oracle's non-finite
    values in the oracle's channels, and every other splat's record is bit for bit what it is without them"""
    aos, vw, where = pc.nonfinite_colour_case()
    r = make_renderer(aos, **ONE_PASS)
    r.Sort(*vw)
    r.Render(*vw)
    ref = oracle_of(aos, vw)
    np.testing.assert_array_equal(r.sorted_indices(), ref["sorted_idx"])
    rec, rect = r.debug_projected()
    sp = ref["splats"]
    poisoned = np.isin(ref["sorted_idx"], [i for i, _, _ in where])
    assert poisoned.sum() == len(where)
    np.testing.assert_array_equal(np.isnan(rec[:, 6:9]), np.isnan(sp["rgb"]))
    np.testing.assert_array_equal(np.isposinf(rec[:, 6:9]), np.isposinf(sp["rgb"]))
    np.testing.assert_array_equal(np.isneginf(rec[:, 6:9]), np.isneginf(sp["rgb"]))
    np.testing.assert_array_equal(rec[:, 9], sp["alpha"])
    assert (~np.isfinite(rec[poisoned][:, 6:10])).any(axis=1).all()
    fixed = aos.copy()
    for i, _, _ in where:
        fixed[i] = aos[i - 1]
        fixed[i, 0:3] = aos[i, 0:3]
    clean = make_renderer(fixed, **ONE_PASS)
    clean.Sort(*vw)
    clean.Render(*vw)
    rec2, rect2 = clean.debug_projected()
    same_bits(rec[~poisoned], rec2[~poisoned], "records of the ordinary splats")
    same_bits(rect[~poisoned], rect2[~poisoned], "rectangles of the ordinary splats")
    assert drawn_of(rect)[poisoned].sum() >= len(where) - 2               # (a poisoned splat may lie off screen; most do not)
    clean.close()
    r.close()


# ---- nothing is drawn for Q and X ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.LADDER_CAMERAS)
def test_ladder_frame_is_the_frame_without_q_and_x(name):
    """both frames are HIP: the full ladder against the same cloud with its Q and X splats removed (upload order kept, so the draw
    order of the others is unchanged), bit for bit -- colour and depth plane; ids and scores name no Q or X splat"""
    aos, vw = pc.ladder_cloud(name).as_array(), pc.view(name)
    ref = oracle_of(aos, vw)
    cls = orc.cov2_class(ref["splats"]["cov"])
    gone = np.sort(ref["sorted_idx"][cls != rule.G])
    assert gone.size >= 32
    keep = np.setdiff1d(np.arange(aos.shape[0]), gone)
    full = make_renderer(aos, **ONE_PASS)
    part = make_renderer(np.ascontiguousarray(aos[keep]), **ONE_PASS)
    full.Sort(*vw); part.Sort(*vw)
    assert full.sort_count() == part.sort_count() + gone.size
    fi, fz = full.Render(*vw, depth=True)
    pi, pz = part.Render(*vw, depth=True)
    d = bits(fi) != bits(pi)
    print("ladder %s: %d Q / X splat(s); %d of %d pixel(s) differ from the frame without them" % (name, gone.size, d.any(axis=-1).sum(), d.shape[0] * d.shape[1]))
    same_bits(fi, pi, "ladder %s: colour" % name)
    same_bits(fz, pz, "ladder %s: depth plane" % name)
    ids = full.RenderIds(*vw)
    assert not np.isin(ids[ids != _capi.ID_NONE], gone).any()
    np.testing.assert_array_equal(ids == _capi.ID_NONE, part.RenderIds(*vw) == _capi.ID_NONE)
    score = full.RenderScores(*vw).cpu().numpy()
    assert (score[gone] == 0).all() and (score[keep] != 0).any()
    np.testing.assert_array_equal(score[keep], part.RenderScores(*vw).cpu().numpy())
    st = full.stats(), part.stats()
    assert (st[0]["drawn"], st[0]["pairs"]) == (st[1]["drawn"], st[1]["pairs"]), st
    full.close(); part.close()


# ---- every instantiation writes the same records -------------------------------------------------------------------------------

def plain_records(aos, vw, **kw):
    r = make_renderer(aos, **dict(ONE_PASS, **kw))
    r.Sort(*vw)
    img = r.Render(*vw)
    rec, rect = r.debug_projected()
    r.close()
    return img, rec, rect


def assert_same_records(rec, rect, rec0, rect0, what, projected=None, min_rects=16):
    """against the plain frame's: the record of every rank the plain frame draws (`projected`: among the ranks this mode's
    projections wrote), bit for bit; the rectangle of every rank that still has one (a two-pass frame's gate empties rectangles, and
    what is left describes its second pass), and no rank has one that the plain frame has not"""
    drawn0 = drawn_of(rect0)
    sel = drawn0 if projected is None else drawn0 & projected
    assert sel.sum() >= 16, (what, sel.sum())
    same_bits(rec[sel], rec0[sel], "%s: records" % what)
    has = drawn_of(rect)
    assert not has[~drawn0].any(), "%s: %d rank(s) gained a rectangle" % (what, has[~drawn0].sum())
    same_bits(rect[has], rect0[has], "%s: rectangles" % what)
    print("%s: %d record(s) and %d rectangle(s) compared" % (what, sel.sum(), has.sum()))
    assert has.sum() >= min_rects, (what, has.sum())


MODE_CLOUDS = {
    "ladder": lambda: (pc.ladder_cloud("squashed").as_array(), pc.view("squashed")),
    "nonfinite": lambda: (pc.nonfinite_geometry_case()[0], pc.nonfinite_geometry_case()[1]),
}


@pytest.mark.parametrize("fixture", sorted(MODE_CLOUDS))
def test_two_pass_projections_write_the_plain_records(fixture):
    """PROJ_PASS1 at share 1.0 projects every rank; at share 1/64 it projects the ranks in front of the cut and PROJ_LISTED those
    behind it that the gate lets pass.  The buffers are filled before each frame, so a rank that no projection wrote shows the fill"""
    aos, vw = MODE_CLOUDS[fixture]()
    img0, rec0, rect0 = plain_records(aos, vw)
    V = rec0.shape[0]
    r = make_renderer(aos, spatial_order=_capi.SPATIAL_OFF, two_pass=_capi.TWO_PASS_ON)
    for share in (1.0, 1.0 / 64.0):
        r.two_pass_state(share)
        r.Sort(*vw)
        r.debug_fill_projected(FILL)
        img = r.Render(*vw)
        info = r.two_pass_info()
        print("%s, share %g: %s" % (fixture, share, info))
        assert info is not None, "the frame ran in one pass"
        same_bits(img, img0, "%s, share %g: frame" % (fixture, share))
        rec, rect = r.debug_projected()
        written = (bits(rec) != np.uint32(0x01010101 * FILL)).any(axis=1)
        front = np.arange(V) >= V - info["splats_pass1"]
        assert written[front].all() and written[~front].sum() == info["splats_pass2"], (written[front].sum(), written[~front].sum(), info)
        if share == 1.0:
            assert info["splats_pass1"] == V
        assert_same_records(rec, rect, rec0, rect0, "%s, share %g (PROJ_PASS1%s)" % (fixture, share, " + PROJ_LISTED" if info["splats_pass2"] else ""),
                            projected=written, min_rects=0)
    r.close()


@functools.lru_cache(maxsize=None)
def sparse_ladder():
    """every other splat of the default ladder with alpha 0.005: the cut of a two-pass frame falls on rank 1024 (occ_cut: a multiple
    of 1024), pass 1 holds the thousand nearest splats, and a pixel under all of them keeps T = 0.995^1000 = 7e-3, far above the
    1/16384 at which a bin is finished"""
    aos = pc.ladder_cloud("default").as_array()[::2].copy()
    aos[:, 3] = np.float32(0.005)
    aos.setflags(write=False)
    return aos


def test_listed_projection_with_no_bin_finished():
    aos, vw = sparse_ladder(), pc.view("default")
    img0, rec0, rect0 = plain_records(aos, vw)
    r = make_renderer(aos, spatial_order=_capi.SPATIAL_OFF, two_pass=_capi.TWO_PASS_ON)
    r.two_pass_state(1.0 / 64.0)
    r.Sort(*vw)
    img = r.Render(*vw)
    info = r.two_pass_info()
    print("sparse ladder, share 1/64: %s" % info)
    assert info is not None and info["bins_unfinished"] == info["bins"], info
    assert info["splats_pass2"] >= 1024 and info["splats_pass1"] + info["splats_pass2"] == rec0.shape[0], info
    same_bits(img, img0, "frame")
    rec, rect = r.debug_projected()
    assert_same_records(rec, rect, rec0, rect0, "PROJ_PASS1 + PROJ_LISTED, every rank projected")
    r.close()


@pytest.mark.parametrize("storage", ["sh_fp16", "sh_q8"])
@pytest.mark.parametrize("fixture", sorted(MODE_CLOUDS))
def test_compact_stores_write_the_records_of_their_decoded_cloud(fixture, storage):
    aos, vw = MODE_CLOUDS[fixture]()
    decoded = round16(aos) if storage == "sh_fp16" else deq(aos)
    img0, rec0, rect0 = plain_records(decoded, vw)
    r = make_renderer(aos, cloud_storage=storage, **ONE_PASS)
    assert r.cloud_storage() == storage
    ref, img, rect = check_records(r, decoded, vw, what="%s in %s" % (fixture, storage))
    rec, _ = r.debug_projected()
    assert_same_records(rec, rect, rec0, rect0, "%s in %s" % (fixture, storage))
    same_bits(img, img0, "%s in %s: frame" % (fixture, storage))
    r.close()


@pytest.mark.parametrize("fixture", sorted(MODE_CLOUDS))
def test_base_sh_width(fixture):
    """the degree-0/1 instantiation (25-float records) against the oracle with the same records, and its geometry against the full-SH
    kernel's: centre, conic, alpha, extents and rectangle do not depend on the SH width"""
    aos, vw = MODE_CLOUDS[fixture]()
    base = np.ascontiguousarray(aos[:, :25])
    _, rec0, rect0 = plain_records(aos, vw)
    r = make_renderer(base, **ONE_PASS)
    ref, img, rect = check_records(r, base, vw, full_sh=False, what="%s, base SH" % fixture)
    rec, _ = r.debug_projected()
    geometry = [0, 1, 2, 3, 4, 5, 9, 10, 11]
    assert_same_records(rec[:, geometry], rect, rec0[:, geometry], rect0, "%s, base SH: geometry" % fixture)
    r.close()


@pytest.mark.parametrize("fixture", sorted(MODE_CLOUDS))
def test_two_views_write_both_eyes_records(fixture):
    """PROJ_TWO_VIEWS: the second view's records lie at V rounded up to 64; both eyes against two plain Renders.  The second view's
    rectangles carry its bin rows behind the first view's: the row fields are compared after taking the offset off"""
    import torch
    from splatapult_amd import camera
    aos, vw = MODE_CLOUDS[fixture]()
    cam, proj, vp, nf = vw
    eyes = [cam, camera.translate_local(cam, dx=0.064)]
    plain = []
    r = make_renderer(aos, **ONE_PASS)
    r.Sort(*vw)
    for e in range(2):
        img = r.Render(eyes[e], proj, vp, nf)
        plain.append((img,) + r.debug_projected())
    fbs = [torch.full((H, W, 4), -5.0, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    r.RenderStereo(eyes, [proj, proj], vp, nf, out_ptrs=[t.data_ptr() for t in fbs], pitch_bytes=W * 16)
    r.synchronize()
    rows = (H + bin_px() - 1) // bin_px()
    for e in range(2):
        rec, rect = r.debug_projected_view(e)
        img0, rec0, rect0 = plain[e]
        same_bits(fbs[e].cpu().numpy(), img0, "%s, eye %d: frame" % (fixture, e))
        if e == 1:
            has = drawn_of(rect)
            assert ((rect[has] >> 8) & 255).min() >= rows, "the second view's rectangles do not lie behind the first's rows"
            rect = np.where(has, rect - np.uint32((rows << 8) | (rows << 24)), rect)
        assert_same_records(rec, rect, rec0, rect0, "%s, PROJ_TWO_VIEWS eye %d" % (fixture, e))
    r.close()


# ---- V at the wave edges -------------------------------------------------------------------------------------------------------

FILL = 0xA5


@pytest.mark.parametrize("storage", ["fp32", "sh_q8"])
@pytest.mark.parametrize("V", pc.COUNTS)
def test_counts_at_the_wave_edges(V, storage):
    """V = 1, 63, 64, 65, 128, 129 visible splats: alone in the cloud, and as every eighth splat of a cloud of 8 V (all sorted indices
    equal modulo 8: in the 8-bit store the eight lanes that fetch one record read neighbouring 128-byte lines).  The ranks beyond V
    keep the bytes the buffers were filled with"""
    for stride, rem in ((1, 0), (8, 3)):
        aos, vw = pc.count_case(V, stride, rem)
        decoded = deq(aos) if storage == "sh_q8" else aos
        r = make_renderer(aos, cloud_storage=storage, **ONE_PASS)
        r.debug_fill_projected(FILL)
        ref, img, rect = check_records(r, decoded, vw, what="V %d, stride %d, %s" % (V, stride, storage))
        assert ref["V"] == V and (r.sorted_indices() % stride == rem).all()
        if stride > 1:
            extra = min(64, V * (stride - 1))
            rec, rect = r.debug_projected_view(0, extra=extra)
            assert (bits(rec[V:]) == np.uint32(0x01010101 * FILL)).all(), "records beyond rank V = %d were written" % V
            assert (rect[V:] == np.uint32(0xFF | FILL << 8)).all(), "rectangles beyond rank V = %d were written" % V
            assert drawn_of(rect[:V]).any()
        r.close()
