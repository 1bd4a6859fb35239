"""What the GPU tests of msplat_compact_cloud share that talks to a device: what a context is after an upload -- its size, storage
kind, downloaded records, storage order, cull boxes and a frame's lists and pixels --, the comparison of two such states bit for
bit, a compaction that returns the map as numpy, and a renderer created under MSPLAT_GRID_CAP.  torch is imported inside the
functions that need it.  pytest rewrites `assert` in test modules only, so every assertion here carries its values in its message."""
import numpy as np

from splatapult_amd import SplatRenderer
from tests import compact_rule as cr
from tests.checks import same_bits
from tests.gpu_harness import make_renderer, sorted_frame

FRAME_KEYS = ("keys", "idx", "img")


def context_state(r, view, full_sh):
    """everything the tests compare of a context that holds a cloud; Sorts and Renders `view`"""
    order = r.storage_order()
    frame = sorted_frame(r, view)
    return dict(n=r.stats()["num_splats"], storage=r.cloud_storage(), cloud=r.download_cloud(full_sh), order=order, boxes=r.cull_boxes(),
                frame=frame)


def assert_same_context(got, ref, what):
    """got: a compacted context's state; ref: that of a context uploaded the kept rows"""
    assert got["n"] == ref["n"], "%s: num_splats %d, the subset's %d" % (what, got["n"], ref["n"])
    assert got["storage"] == ref["storage"], "%s: stored as %s, the subset as %s" % (what, got["storage"], ref["storage"])
    same_bits(got["cloud"], ref["cloud"], "%s: the downloaded records" % what)
    assert (got["order"] is None) == (ref["order"] is None), "%s: storage order %s, the subset's %s" % (
        what, "upload" if got["order"] is None else "Morton", "upload" if ref["order"] is None else "Morton")
    if ref["order"] is not None:
        same_bits(got["order"], ref["order"], "%s: the storage order" % what)
    assert got["boxes"] == ref["boxes"], "%s: cull boxes %s, the subset's %s" % (what, got["boxes"], ref["boxes"])
    assert_same_frame(got["frame"], ref["frame"], what)


def assert_same_frame(a, b, what):
    assert a["V"] == b["V"], "%s: sort_count %d against %d" % (what, a["V"], b["V"])
    for k in FRAME_KEYS:
        same_bits(a[k], b[k], "%s: %s" % (what, k))
    assert (a["drawn"], a["pairs"]) == (b["drawn"], b["pairs"]), "%s: drawn / pairs %s against %s" % (
        what, (a["drawn"], a["pairs"]), (b["drawn"], b["pairs"]))


def compact(r):
    """CompactCloud(index_map=True) with the map as numpy uint32 (MSPLAT_ID_NONE where a splat was dropped)"""
    k, m = r.CompactCloud(index_map=True)
    m = m.cpu().numpy().view(np.uint32)
    return k, m


def assert_map(m, k, keep, what):
    want, want_k = cr.index_map(keep)
    assert k == want_k, "%s: K %d, the rule's %d" % (what, k, want_k)
    same_bits(m, want, "%s: the index map" % what)


def subset_state(aos, keep, view, **kw):
    """the reference: the state of a context that was uploaded aos[keep] only"""
    s = make_renderer(np.ascontiguousarray(aos[keep]), **kw)
    st = context_state(s, view, aos.shape[1] == 61)
    s.close()
    return st


def mask_then_compact(aos, mask, view, what, **kw):
    """a context uploaded `aos`, masked, compacted and compared with the subset upload; returns (the renderer, map)"""
    full_sh = aos.shape[1] == 61
    keep = cr.keep_of(mask)
    r = make_renderer(aos, **kw)
    before = r.download_cloud(full_sh)
    r.SetVisibility(mask)
    k, m = compact(r)
    assert_map(m, k, keep, what)
    got = context_state(r, view, full_sh)
    same_bits(got["cloud"], before[keep], "%s: the download against the kept rows of the download before" % what)
    assert_same_context(got, subset_state(aos, keep, view, **kw), what)
    assert r.visibility() == dict(has_mask=False, crop=None, hidden=0), "%s: %s" % (what, r.visibility())
    return r, m


GRID_CAP_ENV = ("MSPLAT_SORT", "MSPLAT_SCAN_KERNELS", "MSPLAT_GRID_CAP")


def capped_renderer(cloud, monkeypatch, cap=None, **kw):
    """a context created under MSPLAT_GRID_CAP = cap (None: uncapped); the switch is read once, by msplat_create"""
    for k in GRID_CAP_ENV:
        monkeypatch.delenv(k, raising=False)
    if cap is not None:
        monkeypatch.setenv("MSPLAT_GRID_CAP", str(cap))
    r = SplatRenderer(device=0, **kw)
    ok = r.Init(cloud, False, False)
    if cap is not None:
        monkeypatch.delenv("MSPLAT_GRID_CAP")
    assert ok, r.last_error()
    return r
