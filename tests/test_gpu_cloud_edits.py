"""GPU tests of what the cloud edits share (msplat_edit.hip.inc; DESIGN.md 4, "Cloud edits"): the mask and the overlay's classes through a
chain of msplat_transform_cloud / msplat_append_cloud / msplat_transform_cloud calls on ONE context, a compaction at the chain's end,
and the pinned staging slots of the host routes written twice with no synchronise in between and grown by a larger cloud.  Only
existing API.  The reference of every comparison is a FRESH context that was uploaded the rule's rows (tests/transform_harness.py,
tests/append_rule.py) and was set the mask extended by ones and the classes extended by zeros -- or, for the staging slots, a context
that was handed the same bytes through the _device routes, which stage nothing -- and every comparison is same_bits or ==: the
downloaded records, the storage order, the frame's lists and pixels, the projected records and rectangles, and what
msplat_get_visibility / msplat_get_overlay report.  Views are 256 x 160; clouds have at most 5000 splats."""
import numpy as np
import pytest

from splatapult_amd import _capi
from splatapult_amd.renderer import _aos_upload
from tests import append_rule as ar
from tests import compact_harness as ch
from tests import overlay_rule as ov
from tests import transform_harness as th
from tests import transform_rule as tr
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import make_renderer, sorted_frame

pytestmark = pytest.mark.gpu

VIEW = vr.view()
W, H = vr.W, vr.H
OFF, ON = _capi.SPATIAL_OFF, _capi.SPATIAL_ON
MATS = tr.matrices()
N, NS, K = 257, 300, 130                     # one splat past a kBoxSplats box; 130 of a 300-splat source are appended
PALETTE = ov.palette(3)                      # a = 0, 2^-8, 0.5: entry 0 has no effect, and class 3 is beyond the palette


def chain_inputs():
    rng = np.random.default_rng(77)
    mask = np.arange(N) % 3 != 0                                # every third splat hidden
    classes = rng.integers(0, 4, N).astype(np.uint8)
    pick = np.zeros(NS, bool)
    pick[rng.choice(NS, K, replace=False)] = True
    assert (PALETTE[:, 3] == 0).sum() == 1 and 0 < (~mask).sum() < N and set(classes.tolist()) == {0, 1, 2, 3} and pick.sum() == K
    return mask, classes, pick


def drawn_ranks(rect):
    return (rect & 255) <= ((rect >> 16) & 255)


def observed(r):
    """everything the tests compare of a context: ch.context_state, the projected records of its frame and the two getters"""
    st = ch.context_state(r, VIEW, True)
    st["rec"], st["rect"] = r.debug_projected()
    st["visibility"], st["overlay"] = r.visibility(), r.overlay()
    return st


def fresh(rows, spatial, mask, classes, crop=None):
    """what a context reports that was uploaded `rows` and set the planes"""
    f = make_renderer(np.ascontiguousarray(rows), spatial_order=spatial)
    f.SetOverlay(palette=PALETTE)
    if mask is not None:
        f.SetVisibility(mask)
    if classes is not None:
        f.SetOverlay(classes)
    if crop is not None:
        f.SetCrop(*crop)
    st = observed(f)
    f.close()
    return st


def assert_same(got, ref, what):
    th.assert_same_context_again(got, ref, what)
    same_bits(got["rect"], ref["rect"], "%s: the rectangles" % what)
    drawn = drawn_ranks(ref["rect"])                            # (a rank without a rectangle holds what an earlier frame left)
    same_bits(got["rec"][drawn], ref["rec"][drawn], "%s: the projected records of the ranks with a rectangle" % what)
    assert got["visibility"] == ref["visibility"], "%s: msplat_get_visibility %s, the fresh context's %s" % (what, got["visibility"], ref["visibility"])
    assert got["overlay"] == ref["overlay"], "%s: msplat_get_overlay %s, the fresh context's %s" % (what, got["overlay"], ref["overlay"])


def run_chain(spatial, with_mask, with_classes):
    """transform a selection, append 130 of 300 splats of an sh_fp16 source to the fp32 cloud, transform again -- after each step
    the context against a fresh one.  Returns (the renderer, its rows, mask and classes after the chain)"""
    mask, classes, pick = chain_inputs()
    mask, classes = (mask if with_mask else None), (classes if with_classes else None)
    r = make_renderer(vr.cloud_aos(N), spatial_order=spatial)
    assert (r.storage_order() is not None) == (spatial == ON)
    r.SetOverlay(palette=PALETTE)
    if with_mask:
        r.SetVisibility(mask.copy())
    if with_classes:
        r.SetOverlay(classes.copy())
    assert_same(observed(r), fresh(vr.cloud_aos(N), spatial, mask, classes), "before the chain")

    select = vr.random_mask(N, seed=6, share=0.4)
    rows = th.rule_rows(r.download_cloud(True), MATS["rigid"], select)
    r.TransformCloud(MATS["rigid"], select)
    assert_same(observed(r), fresh(rows, spatial, mask, classes), "after the first transform")

    src = make_renderer(ar.source_aos(NS), cloud_storage="sh_fp16", spatial_order=spatial)
    assert src.cloud_storage() != r.cloud_storage()
    rows = ar.merged_rows(r.download_cloud(True), src.download_cloud(True), pick)
    k, _ = r.AppendCloud(src, pick)
    src.close()
    assert k == K and r.stats()["num_splats"] == N + K
    if with_mask:
        mask = ar.merged_mask(mask, K)
    if with_classes:
        classes = np.concatenate([classes, np.zeros(K, np.uint8)])
    assert_same(observed(r), fresh(rows, spatial, mask, classes), "after the append")

    select = vr.random_mask(N + K, seed=9, share=0.5)
    assert select[:N].any() and select[N:].any()
    rows = th.rule_rows(r.download_cloud(True), MATS["similarity"], select)
    r.TransformCloud(MATS["similarity"], select)
    got = observed(r)
    assert_same(got, fresh(rows, spatial, mask, classes), "after the second transform")
    if with_mask:                                               # the planes did something: splats hidden, colours tinted
        assert got["visibility"]["hidden"] == int((~mask).sum()) > 0 and mask[got["frame"]["idx"]].all()
    if with_classes:
        assert got["overlay"] == dict(has_classes=True, palette_count=3, active=True)
        plain = fresh(rows, spatial, mask, None)
        drawn = drawn_ranks(got["rect"])
        tinted = np.isin(classes[got["frame"]["idx"]], (1, 2)) & drawn
        same_bits(got["rec"][drawn & ~tinted], plain["rec"][drawn & ~tinted], "the records of class 0 (a == 0) and class 3 (beyond the palette)")
        assert tinted.any() and (got["rec"][tinted, 6:9] != plain["rec"][tinted, 6:9]).any(), "no colour changed"
    return r, rows, mask, classes


@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton"])
def test_the_mask_and_the_classes_survive_a_chain_of_edits(spatial):
    r, _, _, _ = run_chain(spatial, True, True)
    r.close()


@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton"])
@pytest.mark.parametrize("plane", ["mask_only", "classes_only"])
def test_one_plane_survives_the_chain_without_the_other(plane, spatial):
    r, _, _, _ = run_chain(spatial, plane == "mask_only", plane == "classes_only")
    want = dict(has_mask=plane == "mask_only", has_classes=plane == "classes_only")
    assert dict(has_mask=r.visibility()["has_mask"], has_classes=r.overlay()["has_classes"]) == want
    r.close()


@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton"])
def test_a_compaction_after_the_chain_drops_both_planes_and_keeps_the_palette_and_the_crop(spatial):
    r, rows, mask, classes = run_chain(spatial, True, True)
    crop = (vr.matrices()["scaled"], "box", False)
    r.SetCrop(*crop)
    keep = mask & vr.crop(rows[:, 0:3], crop[0], "box")
    assert 0 < keep.sum() < mask.sum()                          # the mask and the crop both drop splats
    assert r.CompactCloud() == int(keep.sum())
    got = observed(r)
    assert got["visibility"] == dict(has_mask=False, crop=("box", False), hidden=0), got["visibility"]
    assert got["overlay"] == dict(has_classes=False, palette_count=3, active=False), got["overlay"]
    assert_same(got, fresh(rows[keep], spatial, None, None, crop), "the compacted cloud against the subset's upload")
    r.SetOverlay(classes[keep])                                 # the palette is still there: the classes alone bring the tint back
    assert r.overlay() == dict(has_classes=True, palette_count=3, active=True)
    ref = make_renderer(np.ascontiguousarray(rows[keep]), spatial_order=spatial)
    ref.SetOverlay(classes[keep], PALETTE)
    ref.SetCrop(*crop)
    ch.assert_same_frame(sorted_frame(r, VIEW), sorted_frame(ref, VIEW), "the compacted cloud, tinted again")
    r.close()
    ref.close()


# ---- the staging slots ----------------------------------------------------------------------------------------------------------

def upload_again(r, aos):
    """msplat_upload_cloud on the renderer's own context: its staging slots stay"""
    held, args = _aos_upload(aos)                                # (held: the memory args points into)
    assert _capi.lib().msplat_upload_cloud(r._ctx, *args) == _capi.OK, r.last_error()
    r._n = aos.shape[0]


def test_a_staging_slot_is_reused_without_a_synchronise_and_grows_with_the_cloud():
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to("cuda:0")
    r = make_renderer(vr.cloud_aos(300), spatial_order=ON)
    ref = make_renderer(vr.cloud_aos(300), spatial_order=ON)
    fbs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()

    def twice(set_host, set_ref, first, second, what):
        """two values set through the host route back to back, each followed by a Sort and a device-output Render and none by a
        synchronise, the caller's array overwritten as soon as the set call returns; then the frames against the reference's"""
        for value, fb in zip((first, second), fbs):
            mine = value.copy()
            set_host(mine)
            mine[...] = 255 if mine.dtype == np.uint8 else (~mine if mine.dtype == np.bool_ else 0.75)
            r.Sort(*VIEW)
            r.Render(*VIEW, out_ptr=fb.data_ptr(), pitch_bytes=W * 16)
        r.synchronize()
        frames = []
        for k, (value, fb) in enumerate(zip((first, second), fbs)):
            set_ref(value)
            ref.Sort(*VIEW)
            frames.append(ref.Render(*VIEW))
            same_bits(fb.cpu().numpy(), frames[k], "%s: frame %d" % (what, k))
        assert not np.array_equal(frames[0], frames[1]), "%s: the two values show the same frame" % what

    for n in (300, 5000):                                        # the larger cloud's planes do not fit the slots of the smaller one's
        if n != 300:
            for x in (r, ref):
                upload_again(x, vr.cloud_aos(n))
                assert x.visibility()["has_mask"] is False and x.overlay() == dict(has_classes=False, palette_count=3, active=False)
        masks = (np.arange(n) % 3 != 0, vr.random_mask(n, seed=4, share=0.6))
        twice(r.SetVisibility, lambda m: ref.SetVisibility(dev(m)), *masks, "%d splats, masks" % n)
        rng = np.random.default_rng(n)
        classes = tuple(rng.integers(0, 4, n).astype(np.uint8) for _ in range(2))
        for x in (r, ref):
            x.SetOverlay(palette=PALETTE)
        twice(r.SetOverlay, lambda c: ref.SetOverlay(dev(c)), *classes, "%d splats, classes" % n)
        # (the palette has no device route: the reference sets each palette once, a synchronising Render between them)
        palettes = (ov.palette(256), ov.palette(3, seed=1))
        twice(lambda p: r.SetOverlay(palette=p), lambda p: ref.SetOverlay(palette=p.copy()), *palettes, "%d splats, palettes" % n)
        for x in (r, ref):
            x.SetOverlay(palette=PALETTE)
    r.close()
    ref.close()
