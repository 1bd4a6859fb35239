"""GPU tests of selection by neighbourhood (msplat_neighbour_values).  Every value is compared BIT FOR BIT with
the header's rule restated in numpy float32 as brute force over all pairs (tests/neighbour_rule.py); the hash grid may only decide
which pairs are tested.  Clouds hold at most 4097 splats, every call passes an explicit max_tests, d_values sits between sentinel
words; tests/test_neighbours.py checks the fixtures and the cell function on the CPU."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import MsplatError, _capi
from tests import neighbour_rule as nr
from tests import visibility_rule as vr
from tests.checks import same_bits
from tests.gpu_harness import make_renderer, sorted_frame

pytestmark = pytest.mark.gpu

OFF, ON = _capi.SPATIAL_OFF, _capi.SPATIAL_ON
ORDERS = pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
DEV = "cuda:0"
F = np.float32
SENTINEL = nr.SENTINEL
PAD = 19            # floats of sentinel on both sides of d_values: the array starts 4-byte aligned and no better
BIG = 1 << 40       # a budget no cloud of 4097 splats reaches (4097^2 < 2^25)
FIXTURE_RADIUS = dict(boundary=nr.BOUNDARY_RADIUS, hostile=nr.HOSTILE_RADIUS, geo=nr.GEO_RADIUS)


def cloud_with_centres(xyz, **kw):
    """a renderer holding valid splats whose centres are xyz, bit for bit"""
    aos = np.array(vr.cloud_aos(xyz.shape[0]))
    aos[:, 0:3] = xyz
    r = make_renderer(aos, **kw)
    same_bits(r.debug_positions()[:, 0:3], np.ascontiguousarray(xyz), "the position plane holds the fixture's centres")
    return r


def to_device(a):
    import torch
    t = torch.from_numpy(np.array(a)).to(DEV)                          # (a copy: the fixtures are read-only)
    torch.cuda.synchronize()
    return t


def padded_values(n):
    import torch
    buf = torch.full((n + 2 * PAD,), float(SENTINEL), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    return buf, buf[PAD:PAD + n]


def near(r, kind, radius, source=None, query=None, cap=0, max_tests=BIG):
    """the call into sentinel-padded memory: (values of the n words, info); the padding must keep its bytes"""
    n = r._n
    buf, out = padded_values(n)
    src = None if source is None else to_device(source)
    qry = src if query is source else (None if query is None else to_device(query))
    got, info = r.NeighbourValues(radius, kind, source=src, query=qry, cap=cap, max_tests=max_tests, out=out, info=True)
    assert got.data_ptr() == out.data_ptr()
    whole = buf.cpu().numpy()
    assert (whole[:PAD] == SENTINEL).all() and (whole[PAD + n:] == SENTINEL).all(), "the padding around d_values was written"
    return whole[PAD:PAD + n].copy(), info


def check_info(info, xyz, d2, radius, source=None, query=None, what=""):
    want = nr.info(xyz, d2, radius, source, query)
    assert (info["sources"], info["queries"]) == (want["sources"], want["queries"]), (what, info, want)
    assert want["pairs"] <= info["tests"] <= want["queries"] * want["sources"], (what, info, want)
    assert info["max_bucket"] <= info["sources"] and (info["buckets"] & (info["buckets"] - 1)) == 0 and info["buckets"] >= 1, (what, info)
    return want


# ---- 1. sizes and stores ---------------------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("storage", ["fp32", "sh_q8"])
@pytest.mark.parametrize("n", nr.SIZES)
def test_values_equal_the_rule_at_every_size_in_every_store(n, storage, spatial):
    xyz, d2 = nr.random_cloud(n), nr.d2_of("random", n)
    r = cloud_with_centres(xyz, cloud_storage=storage, spatial_order=spatial)
    assert r.cloud_storage() == storage and (n < 63 or (r.storage_order() is not None) == (spatial == ON))
    for which, radius in nr.random_radii(n).items():
        for kind in nr.KINDS:
            what = "n %d, %s, order %d, radius %s, %s" % (n, storage, spatial, which, kind)
            got, info = near(r, kind, radius)
            same_bits(got, nr.values(d2, kind, radius), what)
            check_info(info, xyz, d2, radius, what=what)
            assert info["buckets"] >= n
            if which == "all" and kind == "count":
                assert (got == n - 1).all(), "one neighbourhood holds the whole cloud: everyone counts everyone else"
            if which == "none":
                assert not got.any() if kind == "count" else np.isposinf(got).all()
    r.close()


# ---- 2. the boundary -------------------------------------------------------------------------------------------------------------
@ORDERS
def test_the_radius_is_closed_cell_boundaries_and_coincident_copies_are_handled(spatial):
    b = nr.boundary_cloud()
    xyz, d2, radius = b["xyz"], nr.d2_of("boundary"), nr.BOUNDARY_RADIUS
    r = cloud_with_centres(xyz, spatial_order=spatial)
    count, info = near(r, "count", radius)
    dist2, _ = near(r, "dist2", radius)
    same_bits(count, nr.values(d2, "count", radius), "count")
    same_bits(dist2, nr.values(d2, "dist2", radius), "dist2")
    check_info(info, xyz, d2, radius)
    for i, j in b["exact"]:
        assert count[i] == 1 and count[j] == 1 and dist2[i] == nr.r2_of(radius) == dist2[j], "a pair at exactly the radius is counted"
    for i, j in b["ulp"]:
        assert count[i] == 0 and count[j] == 0 and np.isposinf(dist2[i]) and np.isposinf(dist2[j]), "one ulp farther is not"
    c0, c1 = b["coincident"]
    assert (count[c0:c1] == nr.COINCIDENT - 1).all() and (dist2[c0:c1] == 0).all() and info["max_bucket"] >= nr.COINCIDENT
    l0, l1 = b["lattice"]
    assert count[l0:l1].max() == 26 and count[l0:l1].min() == 7 and (xyz[l0:l1] < 0).any()
    r.close()


# ---- 3. hostile centres ----------------------------------------------------------------------------------------------------------
@ORDERS
def test_nan_infinite_and_huge_centres_have_no_neighbours_and_outliers_do_not_coarsen_the_grid(spatial):
    hc = nr.hostile_cloud()
    xyz, d2, radius = hc["xyz"], nr.d2_of("hostile"), nr.HOSTILE_RADIUS
    r = cloud_with_centres(xyz, spatial_order=spatial)
    count, info = near(r, "count", radius)
    dist2, _ = near(r, "dist2", radius)
    same_bits(count, nr.values(d2, "count", radius), "count")
    same_bits(dist2, nr.values(d2, "dist2", radius), "dist2")
    want = check_info(info, xyz, d2, radius)
    assert info["sources"] == info["queries"] == xyz.shape[0] - len(hc["bad"]), "NaN and infinite centres are left out of the grid and the search"
    for i in hc["bad"] + hc["huge"]:
        assert count[i] == 0 and np.isposinf(dist2[i])
    for i in hc["outliers"][:2] + hc["clamped"]:
        assert count[i] == 1 and dist2[i] == 0
    # outliers at 1e6 and clamped cells at 1e30 beside a unit cube: the candidates stay far from all pairs
    assert info["tests"] < want["queries"] * want["sources"] // 4, (info, want)
    r.close()


@ORDERS
def test_a_geo_referenced_cloud_keeps_its_cells(spatial):
    xyz, d2, radius = nr.geo_cloud(), nr.d2_of("geo"), nr.GEO_RADIUS
    r = cloud_with_centres(xyz, spatial_order=spatial)
    for kind in nr.KINDS:
        got, info = near(r, kind, radius)
        same_bits(got, nr.values(d2, kind, radius), kind)
    want = check_info(info, xyz, d2, radius)
    assert info["tests"] < want["queries"] * want["sources"] // 4, (info, want)
    r.close()


# ---- 4. collisions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "boundary", "hostile"])
def test_forced_bucket_counts_give_identical_bytes_and_one_bucket_tests_every_pair(name):
    n = 4097 if name == "random" else 0
    xyz, d2 = nr.xyz_of(name, n), nr.d2_of(name, n)
    radius = nr.random_radii(n)["some"] if name == "random" else FIXTURE_RADIUS[name]
    r = cloud_with_centres(xyz, spatial_order=ON)
    L = _capi.lib()
    m = nr.set_masks(xyz.shape[0])
    for kind, source, query in (("count", None, None), ("dist2", m["random_source"], m["random_query"])):
        want_info = nr.info(xyz, d2, radius, source, query)
        ref = None
        for buckets in (0, 1, 2, 64):
            assert L.msplat_debug_set_neighbour_buckets(r._ctx, buckets) == _capi.OK, r.last_error()
            got, info = near(r, kind, radius, source, query)
            what = "%s, %s, %d buckets" % (name, kind, buckets)
            check_info(info, xyz, d2, radius, source, query, what)
            if ref is None:
                ref = got
                same_bits(got, nr.values(d2, kind, radius, source, query), what)
                assert info["buckets"] >= xyz.shape[0]
            else:
                same_bits(got, ref, what)
                assert info["buckets"] == buckets
            if buckets == 1:
                assert info["tests"] == want_info["queries"] * want_info["sources"], "one bucket, visited once by every query: %r" % (info,)
                assert info["max_bucket"] == want_info["sources"]
    for bad in (3, (1 << 24) + 1, 1 << 25, 0xFFFFFFFF):
        assert L.msplat_debug_set_neighbour_buckets(r._ctx, bad) == _capi.ERR_INVALID_ARG and "power of two" in r.last_error()
    assert L.msplat_debug_set_neighbour_buckets(r._ctx, 0) == _capi.OK
    r.close()


# ---- 5. sets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 4097])
def test_source_and_query_sets_and_caps(n):
    xyz, d2, m = nr.random_cloud(n), nr.d2_of("random", n), nr.set_masks(n)
    radius = nr.random_radii(n)["some"]
    r = cloud_with_centres(xyz, spatial_order=ON if n > 65 else OFF)
    sets = {"NULL": None, "random_source": m["random_source"], "random_query": m["random_query"], "empty": m["empty"], "full": m["full"]}
    checked = 0
    for sname, qname in (("NULL", "NULL"), ("random_source", "random_query"), ("random_source", "random_source"), ("empty", "full"),
                         ("full", "empty"), ("NULL", "random_query"), ("random_source", "NULL"), ("empty", "empty"), ("full", "full")):
        source, query = sets[sname], sets[qname]
        for kind, cap in (("count", 0), ("count", 1), ("count", 2), ("count", 255), ("dist2", 0)):
            what = "n %d, source %s, query %s, %s cap %d" % (n, sname, qname, kind, cap)
            got, info = near(r, kind, radius, source, query, cap)
            same_bits(got, nr.values(d2, kind, radius, source, query, cap), what)
            check_info(info, xyz, d2, radius, source, query, what)
            if query is not None:
                assert (got[query == 0] == SENTINEL).all(), "%s: the words of unselected queries keep their sentinel" % what
            checked += 1
    assert checked == 45 and nr.result(d2, "count", radius).max() > 2
    r.close()


def test_grow_selection_is_the_rules_dilation():
    n = 4097
    xyz, d2 = nr.random_cloud(n), nr.d2_of("random", n)
    radius = nr.random_radii(n)["some"] * F(0.6)
    r = cloud_with_centres(xyz, spatial_order=ON)
    seed = np.zeros(n, np.uint8)
    seed[[5, 1900, 4096]] = (200, 1, 255)
    mask = to_device(seed)
    for steps in (0, 1, 3):
        grown = r.GrowSelection(mask, radius, steps, max_tests=BIG)
        r.synchronize()
        want = nr.grow(d2, seed, radius, steps)
        same_bits(grown.cpu().numpy(), want, "%d step(s)" % steps)
        assert grown.data_ptr() != mask.data_ptr()
    same_bits(mask.cpu().numpy(), seed, "the caller's mask is left alone")
    assert (want != 0).sum() > (nr.grow(d2, seed, radius, 1) != 0).sum() > 3, "the selection does grow, and further in three steps"
    r.close()


# ---- 6. the budget ---------------------------------------------------------------------------------------------------------------
def raw(r, kind, radius, d_values, source=None, query=None, n=None, cap=0, max_tests=BIG, info=None):
    p = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else C.c_void_p(t.data_ptr()))
    return r._lib.msplat_neighbour_values(r._ctx, kind, radius, p(source), p(query), r._n if n is None else n, cap, max_tests, p(d_values),
                                          None if info is None else C.byref(info))


def test_a_search_beyond_the_budget_is_refused_before_it_is_launched():
    n = 4097
    xyz, d2 = nr.random_cloud(n), nr.d2_of("random", n)
    radius = nr.random_radii(n)["some"]
    r = cloud_with_centres(xyz, spatial_order=ON)
    _, first = near(r, "count", radius)
    tests = first["tests"]
    assert tests > n
    buf, out = padded_values(n)
    ni = _capi.NeighbourInfo(struct_size=C.sizeof(_capi.NeighbourInfo))
    assert raw(r, 0, radius, out, max_tests=tests - 1, info=ni) == _capi.ERR_UNSUPPORTED
    msg = r.last_error()
    assert "msplat_neighbour_values" in msg and str(tests) in msg and str(tests - 1) in msg, msg
    assert (ni.tests, ni.sources, ni.queries, ni.buckets) == (tests, n, n, first["buckets"]), "info is filled by the refused call too"
    r.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all(), "the refused call wrote d_values"
    with pytest.raises(MsplatError) as e:
        r.NeighbourValues(radius, max_tests=1)
    assert e.value.code == _capi.ERR_UNSUPPORTED
    assert raw(r, 0, radius, out, max_tests=tests, info=ni) == _capi.OK, r.last_error()
    same_bits(buf.cpu().numpy()[PAD:PAD + n], nr.values(d2, "count", radius), "the same context, the budget met exactly")
    r.close()


# ---- 7. nothing else moves -------------------------------------------------------------------------------------------------------
def test_the_context_its_sort_and_its_frames_are_untouched_and_the_call_repeats_its_bytes(monkeypatch):
    n, view = 4097, vr.view()
    aos = vr.cloud_aos(n)
    xyz = np.ascontiguousarray(aos[:, 0:3])
    d2 = nr.d2_matrix(xyz)
    radius = F(0.35)
    want = {kind: nr.values(d2, kind, radius) for kind in nr.KINDS}
    assert 2 < want["count"].mean() < 200
    r = make_renderer(aos, spatial_order=ON)
    before = sorted_frame(r, view)
    bytes_before = r.stats()["device_bytes"]
    first = {kind: near(r, kind, radius)[0] for kind in nr.KINDS}
    bytes_first = r.stats()["device_bytes"]
    assert bytes_first >= bytes_before + 16 * n, "msplat_stats.device_bytes counts the grid's scratch"
    for kind in nr.KINDS:
        same_bits(first[kind], want[kind], kind)
        same_bits(near(r, kind, radius)[0], first[kind], "%s: a second identical call" % kind)
    assert r.stats()["device_bytes"] == bytes_first, "the scratch is reused"
    assert r.sort_count() == before["V"]
    img = r.Render(*view)
    same_bits(img, before["img"], "a Render after the calls, without a new Sort")
    after = sorted_frame(r, view)
    for key in ("keys", "idx", "img"):
        same_bits(after[key], before[key], "after the calls: %s" % key)
    # a masked and cropped context: the store is read, whatever they hide
    hide = np.ones(n, np.uint8)
    hide[::3] = 0
    r.SetVisibility(hide)
    r.SetCrop(vr.matrices()[vr.CROPS[0][0]], vr.CROPS[0][1], vr.CROPS[0][2])
    r.Sort(*view)
    assert r.sort_count() < before["V"]
    for kind in nr.KINDS:
        same_bits(near(r, kind, radius)[0], first[kind], "%s under a mask and a crop" % kind)
    r.close()
    # every grid-stride loop takes several turns
    monkeypatch.setenv("MSPLAT_GRID_CAP", "1")                           # read when the context is created
    one = make_renderer(aos, spatial_order=ON)
    m = nr.set_masks(n)
    for kind in nr.KINDS:
        same_bits(near(one, kind, radius)[0], first[kind], "%s with one workgroup per launch" % kind)
    got, info = near(one, "count", radius, m["random_source"], m["random_query"], cap=2)
    same_bits(got, nr.values(d2, "count", radius, m["random_source"], m["random_query"], 2), "sets with one workgroup per launch")
    check_info(info, xyz, d2, radius, m["random_source"], m["random_query"])
    one.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_say_why_and_leave_d_values_and_the_context_as_they_were():
    import torch
    L = _capi.lib()
    n, view = 257, vr.view()
    aos = vr.cloud_aos(n)
    r = make_renderer(aos)
    before = sorted_frame(r, view)
    vals = torch.full((n + 2,), float(SENTINEL), dtype=torch.float32, device=DEV)
    joint = torch.full((8 * n,), 1, dtype=torch.uint8, device=DEV)       # bytes that d_values can be laid over
    mask = torch.full((n,), 1, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    host_bytes = np.ones(4 * n + 16, np.uint8)
    at = host_bytes.ctypes.data
    ni = _capi.NeighbourInfo(struct_size=C.sizeof(_capi.NeighbourInfo))
    p = lambda v: C.c_void_p(v)

    def call(kind=0, radius=0.5, values=vals, source=None, query=None, k=n, cap=0, max_tests=BIG, info=ni):
        return raw(r, kind, radius, values, source, query, k, cap, max_tests, info)

    def refused(rc, code, words):
        msg = r.last_error()
        assert rc == code and "msplat_neighbour_values" in msg and all(w in msg for w in words), (rc, code, msg)

    over_source = p(joint.data_ptr() + 4 * n - 4)                       # d_source begins inside the last word of d_values
    for kw, words in ((dict(kind=2), ["kind 2"]), (dict(kind=-1), ["kind -1"]), (dict(radius=0.0), ["radius", "> 0"]), (dict(radius=-1.0), ["radius", "> 0"]),
                      (dict(radius=float("nan")), ["radius"]), (dict(radius=float("inf")), ["radius"]), (dict(radius=1e-30), ["not a normal fp32 number"]),
                      (dict(radius=1e20), ["not a normal fp32 number"]), (dict(kind=1, cap=1), ["cap 1", "MSPLAT_NEAR_DIST2"]),
                      (dict(k=n - 1), ["for a cloud of"]), (dict(k=n + 1), ["for a cloud of"]), (dict(k=0), ["for a cloud of"]),
                      (dict(values=None), ["d_values is NULL"]), (dict(values=p(vals.data_ptr() + 2)), ["d_values", "4-byte aligned"]),
                      (dict(values=p(at)), ["d_values", "not device memory"]), (dict(source=p(at)), ["d_source", "not device memory"]),
                      (dict(query=p(at)), ["d_query", "not device memory"]),
                      (dict(values=p(joint.data_ptr()), source=p(joint.data_ptr())), ["d_values overlaps d_source"]),
                      (dict(values=p(joint.data_ptr()), source=over_source), ["d_values overlaps d_source"]),
                      (dict(values=p(joint.data_ptr() + 4), query=p(joint.data_ptr())), ["d_values overlaps d_query"]),
                      (dict(values=p(joint.data_ptr() + 4), source=mask, query=p(joint.data_ptr() + 4 * n)), ["d_values overlaps d_query"])):
        refused(call(**kw), _capi.ERR_INVALID_ARG, words)
    ni.struct_size = _capi.NeighbourInfo.tests.offset
    refused(call(), _capi.ERR_INVALID_ARG, ["struct_size"])
    ni.struct_size = C.sizeof(_capi.NeighbourInfo)
    # adjacent is not overlapping: d_values right behind d_source, and without info
    assert call(values=p(joint.data_ptr() + n + (-n) % 4), source=p(joint.data_ptr()), info=None) == _capi.OK, r.last_error()
    r.synchronize()
    assert (vals.cpu().numpy() == SENTINEL).all() and (host_bytes == 1).all() and (mask.cpu().numpy() == 1).all(), "a refused call wrote"
    assert (joint.cpu().numpy()[:n] == 1).all()
    after = sorted_frame(r, view)
    for key in ("keys", "idx", "img"):
        same_bits(after[key], before[key], "after the refusals: %s" % key)
    with pytest.raises(ValueError):
        r.NeighbourValues(0.5, out=vals)                               # n + 2 floats
    with pytest.raises(ValueError):
        r.NeighbourValues(0.5, source=np.ones(n + 1, np.uint8))
    r.close()

    # before an upload; with a point cloud (which still renders)
    cfg = _capi.Config()
    cfg.struct_size = C.sizeof(_capi.Config)
    cfg.t_epsilon = -1.0
    h = C.c_void_p()
    assert L.msplat_create(C.byref(h), C.byref(cfg)) == _capi.OK
    d_vals = p(vals.data_ptr())
    assert L.msplat_neighbour_values(h, 0, 0.5, None, None, n, 0, BIG, d_vals, None) == _capi.ERR_NO_CLOUD
    assert b"msplat_neighbour_values" in L.msplat_last_error(h)
    cam, proj, vp, nf = view
    fptr = lambda a: np.ascontiguousarray(np.asarray(a, F).reshape(-1)).ctypes.data_as(C.POINTER(C.c_float))
    fp = [fptr(x) for x in (cam, proj, vp, nf)]
    pts = np.random.default_rng(81).uniform(-1, 1, (n, 8)).astype(F)
    pts[:, 3] = 1.0
    pts[:, 4:] = np.abs(pts[:, 4:])
    W, H = int(vp[2]), int(vp[3])
    assert L.msplat_upload_points(h, pts.ctypes.data, pts.shape[0], 32, 0, 16) == _capi.OK
    assert L.msplat_sort(h, *fp) == _capi.OK
    img0, img1 = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    assert L.msplat_render(h, *fp, img0.ctypes.data, 0, 0) == _capi.OK
    assert L.msplat_neighbour_values(h, 0, 0.5, None, None, n, 0, BIG, d_vals, None) == _capi.ERR_UNSUPPORTED and b"point cloud" in L.msplat_last_error(h)
    assert L.msplat_render(h, *fp, img1.ctypes.data, 0, 0) == _capi.OK
    same_bits(img1, img0, "the point context renders what it rendered")
    L.msplat_destroy(h)
    torch.cuda.synchronize()
    assert (vals.cpu().numpy() == SENTINEL).all()


def test_an_empty_cloud_succeeds_and_writes_nothing():
    import torch
    r = make_renderer(np.zeros((0, 61), F))
    ni = _capi.NeighbourInfo(struct_size=C.sizeof(_capi.NeighbourInfo))
    ni.tests = 7
    assert _capi.lib().msplat_neighbour_values(r._ctx, 0, 0.5, None, None, 0, 0, BIG, None, C.byref(ni)) == _capi.OK
    assert (ni.sources, ni.queries, ni.buckets, ni.max_bucket, ni.tests) == (0, 0, 0, 0, 0)
    got = r.NeighbourValues(0.5, "dist2", max_tests=BIG, out=torch.zeros(0, dtype=torch.float32, device=DEV))
    assert got.shape == (0,)
    r.close()
