"""GPU tests of the uploads from device memory: msplat_upload_cloud_device, msplat_upload_ply_vertices_device and
msplat_upload_attributes_device against the host routes they mirror -- records, keys, sorted indices and frames compared as
uint32, exactly --, the attribute route against GaussianCloud.FromAttributes within the bounds of
tests/test_gpu_parity.py::test_gpu_ingest_matches_host_import, the refusals, the source's lifetime and the viewer loop.
Sources are torch tensors on cuda:0; views are 256 x 160.  No test hands a host address to these calls: the pointer guard
(hipPointerGetAttributes, the first HIP call of each route) is checked by reading."""
import ctypes as C
import functools

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi, synthetic
from tests import scenes
from tests.checks import same_bits
from tests.render_cases import ply_layout

pytestmark = pytest.mark.gpu

STORAGES = ("fp32", "sh_fp16", "sh_q8")
NS = (0, 1, 63, 64, 65, 1000, 4097)          # wave edges; at stride 100 the spans of 1, 63, 65, 1000 and 4097 records end off a 16-byte boundary
VIEW = scenes.default_view(256, 160)
# the sixteen attributes of msplat_attr_offsets: floats each, first float in the reference's 61-float (25-float) record
ATTR_FLOATS = (4, 4, 4, 4, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4)
ATTR_SRC = (0, 4, 8, 12, 16, 19, 22, 25, 29, 33, 37, 41, 45, 49, 53, 57)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")       # (a copy: the shared inputs are read-only)


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def cloud_array(full_sh, n=4097, seed=31):
    """the records every route is fed (computed once, never changed): a synthetic cloud with a negative zero and a denormal in
    the f_rest of record 5"""
    aos = scenes.synth_cloud(n, seed, full_sh=full_sh, log_scale_mean=-3.0).as_array().copy()
    aos[5, 5], aos[5, 6] = -0.0, 1e-40
    if full_sh:
        aos[5, 30], aos[5, 31], aos[5, 60] = 1e-40, -0.0, -1e-41
    aos.setflags(write=False)
    return aos


@functools.lru_cache(maxsize=None)
def layout(kind, full_sh):
    """(stride, the 16 offsets): the reference's own 100 / 244-byte record; a 272-byte record with the attributes at shuffled
    offsets; a 276-byte one whose offsets are arbitrary BYTES (the host's memcpy takes them)"""
    if kind == "ref":
        return (244 if full_sh else 100), tuple(4 * s for s in ATTR_SRC)
    stride, unit = (272, 4) if kind == "shuffled272" else (276, 1)
    rng = np.random.default_rng(272 if unit == 4 else 276)
    order = rng.permutation(16)
    gaps = rng.multinomial((stride - 244) // unit, [1 / 17] * 17) * unit
    off, at = [0] * 16, 0
    for slot, k in enumerate(order):
        at += int(gaps[slot])
        off[k] = at
        at += 4 * ATTR_FLOATS[k]
    assert at <= stride and sorted(off) != list(off)
    assert unit == 4 or any(o % 4 for o in off[:7])
    return stride, tuple(off)


def pack_records(aos, stride, off):
    """the (n, 25 | 61) cloud as n records of `stride` bytes, junk between the attributes"""
    n, full = aos.shape[0], aos.shape[1] == 61
    buf = np.full((n, stride), 0xA5, np.uint8)
    raw = np.ascontiguousarray(aos).view(np.uint8).reshape(n, 4 * aos.shape[1])
    for k in range(16 if full else 7):
        buf[:, off[k]:off[k] + 4 * ATTR_FLOATS[k]] = raw[:, 4 * ATTR_SRC[k]:4 * (ATTR_SRC[k] + ATTR_FLOATS[k])]
    return buf


def context(storage="fp32", **kw):
    r = SplatRenderer(device=0, cloud_storage=storage, **kw)
    assert r._create(False), r.last_error()
    return r


def upload_records(r, buf, off, full_sh, device):
    """msplat_upload_cloud[_device] of the packed records into r's context 0; returns the code"""
    n, stride = buf.shape
    o = _capi.AttrOffsets(*off)
    if device:
        t = dev(buf)
        rc = r._lib.msplat_upload_cloud_device(r._ctx, ptr(t), n, stride, C.byref(o), int(full_sh))
    else:
        rc = r._lib.msplat_upload_cloud(r._ctx, buf.ctypes.data, n, stride, C.byref(o), int(full_sh))
    r._n = n
    return rc


def observe(r, full_sh, view=VIEW):
    """everything the issue compares between two routes, as uint32: the downloaded records, then after one Sort the keys and the
    sorted indices, then the frame"""
    got = {"storage": r.cloud_storage(), "cloud": u32(r.download_cloud(full_sh))}
    r.Sort(*view)
    got["keys"], got["indices"] = r.sorted_keys(), r.sorted_indices()
    got["frame"] = u32(r.Render(*view))
    return got


def same_observations(a, b, msg):
    assert a["storage"] == b["storage"], msg
    for k in ("cloud", "keys", "indices", "frame"):
        same_bits(a[k], b[k], "%s: %s differs" % (msg, k))


# ---- 1. records, device against host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ref", "shuffled272", "bytes276"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("full_sh", [0, 1])
def test_device_records_equal_host_records(full_sh, storage, kind):
    stride, off = layout(kind, bool(full_sh))
    host, devr = context(storage), context(storage)
    for n in NS:
        buf = pack_records(cloud_array(bool(full_sh))[:n], stride, off)
        assert upload_records(host, buf, off, full_sh, False) == _capi.OK, host.last_error()
        assert upload_records(devr, buf, off, full_sh, True) == _capi.OK, devr.last_error()
        a, b = observe(host, bool(full_sh)), observe(devr, bool(full_sh))
        assert a["storage"] == (storage if full_sh or storage != "sh_q8" else "fp32")      # a degree-0 cloud asked to be SH_Q8 is FP32
        assert n < 1000 or len(a["keys"]) > n // 2
        same_observations(a, b, "n = %d" % n)
        if storage == "fp32" and n:
            same_bits(a["cloud"], u32(cloud_array(bool(full_sh))[:n]), "the FP32 download is the upload, bit for bit")
    host.close(), devr.close()


# ---- 2. spatial order, band cull, frames in flight --------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_spatial_order_and_band_cull_are_equal_between_the_routes(storage):
    stride, off = layout("ref", True)
    buf = pack_records(cloud_array(True), stride, off)
    seen = []
    for device in (False, True):
        r = context(storage, spatial_order=_capi.SPATIAL_ON)
        assert upload_records(r, buf, off, 1, device) == _capi.OK, r.last_error()
        order = r.storage_order()
        assert order is not None and sorted(order.tolist()) == list(range(4097))
        got = observe(r, True)
        r.set_band(3, 1, band_cull=True)            # the band-restricted cull: the only observer of pos4.w
        r.Sort(*VIEW)
        seen.append((order, got, r.sort_count(), r.sorted_indices()))
        r.close()
    same_bits(seen[0][0], seen[1][0], "msplat_get_storage_order differs")
    same_observations(seen[0][1], seen[1][1], "spatial order on")
    assert 0 < seen[0][2] < len(seen[0][1]["keys"]), "the band cull dropped nothing: it observes no footprint bound here"
    assert seen[0][2] == seen[1][2], "sort_count under the band cull differs: %d host, %d device" % (seen[0][2], seen[1][2])
    same_bits(seen[0][3], seen[1][3], "the band's sorted indices differ")


def test_frames_in_flight_render_the_host_route_frame():
    import torch
    stride, off = layout("shuffled272", True)
    buf = pack_records(cloud_array(True)[:1000], stride, off)
    one = context()
    assert upload_records(one, buf, off, 1, False) == _capi.OK, one.last_error()
    want = observe(one, True)["frame"]
    t = dev(buf)
    fly = SplatRenderer(device=0, frames_in_flight=2)
    assert fly.InitFromDevice(t.data_ptr(), 1000, stride, off, True), fly.last_error()
    fbs = [torch.zeros((160, 256, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        fly.Sort(*VIEW)
        assert fly.frame_slot == k
        fly.Render(*VIEW, out_ptr=fbs[k].data_ptr(), pitch_bytes=256 * 16)
    fly.synchronize()
    for k in range(2):
        same_bits(u32(fbs[k].cpu().numpy()), want, "context %d" % k)
    fly.close(), one.close()


# ---- 3. vertices ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attrs(n=4097, seed=0xD0):
    a = synthetic.generate(n, seed=seed, full_sh=True, log_scale_mean=-3.0)
    a["rot"] = (a["rot"] * np.linspace(0.25, 4.0, n, dtype=np.float32)[:, None]).astype(np.float32)     # not normalised
    a["rot"][7] = 0.0                                                                                   # identity by the host's rule
    a["rot"][8] = (0.0, 0.0, 3.0, 0.0)
    for v in a.values():
        v.setflags(write=False)
    return a


def vertex_block(a, n, rest=True):
    """synthetic.write_ply's 62-float vertex (17 without f_rest) of the first n splats, as the file holds it"""
    cols = [a["xyz"][:n], np.zeros((n, 3), np.float32), a["f_dc"][:n]] + ([a["f_rest"][:n]] if rest else [])
    cols += [a["opacity"][:n, None], a["log_scale"][:n], a["rot"][:n]]
    return np.ascontiguousarray(np.concatenate(cols, axis=1), "<f4")


def layout_without_rest():
    L = _capi.PlyLayout()
    L.vertex_size = 17 * 4
    L.x, L.y, L.z = 0, 4, 8
    for i in range(3):
        L.f_dc[i] = 24 + 4 * i
    for i in range(45):
        L.f_rest[i] = -1
    L.opacity = 36
    for i in range(3):
        L.scale[i] = 40 + 4 * i
    for i in range(4):
        L.rot[i] = 52 + 4 * i
    return L


def upload_vertices(r, block, L, full_sh, device):
    n = block.shape[0]
    if device:
        t = dev(block)
        rc = r._lib.msplat_upload_ply_vertices_device(r._ctx, ptr(t), n, C.byref(L), int(full_sh))
    else:
        rc = r._lib.msplat_upload_ply_vertices(r._ctx, block.ctypes.data, n, C.byref(L), int(full_sh))
    r._n = n
    return rc


@pytest.mark.parametrize("storage", STORAGES)
def test_device_vertices_equal_host_vertices(storage):
    a = attrs()
    absent = ply_layout()
    absent.opacity = -1                     # reads as 0: alpha 1/2
    cases = [("write_ply", vertex_block(a, 1000), ply_layout(), 1, True), ("degree 0 asked for", vertex_block(a, 65), ply_layout(), 0, False),
             ("no f_rest", vertex_block(a, 1000, rest=False), layout_without_rest(), 1, False),
             ("no opacity", vertex_block(a, 63), absent, 1, True)]
    host, devr = context(storage), context(storage)
    for name, block, L, full_sh, full in cases:
        assert upload_vertices(host, block, L, full_sh, False) == _capi.OK, host.last_error()
        assert upload_vertices(devr, block, L, full_sh, True) == _capi.OK, devr.last_error()
        x, y = observe(host, full), observe(devr, full)
        same_observations(x, y, name)
        if name == "no opacity":
            assert (x["cloud"].view(np.float32)[:, 3] == 0.5).all()
    host.close(), devr.close()


# ---- 4. attributes ----------------------------------------------------------------------------------------------------------
def upload_attributes(r, a, n, full_sh=1, offset=None, rest=True):
    """msplat_upload_attributes_device of the first n splats; offset = name: that array is a view that starts one float into a
    larger tensor (4-byte aligned only)"""
    import torch
    t = {}
    for k in ("xyz", "f_dc", "f_rest", "opacity", "log_scale", "rot"):
        flat = np.ascontiguousarray(a[k][:n]).reshape(-1)
        if k == offset:
            big = torch.full((flat.size + 3,), float("nan"), dtype=torch.float32, device="cuda:0")
            big[1:1 + flat.size] = dev(flat)
            t[k] = big[1:1 + flat.size]
            assert t[k].numel() == 0 or t[k].data_ptr() % 16 == 4
        else:
            t[k] = dev(flat if n else np.zeros(4, np.float32))      # (n = 0: a pointer all the same -- a NULL f_rest means degree 0)
    torch.cuda.synchronize()
    rc = r._lib.msplat_upload_attributes_device(r._ctx, n, ptr(t["xyz"]), ptr(t["f_dc"]), ptr(t["f_rest"]) if rest else None,
                                                ptr(t["opacity"]), ptr(t["log_scale"]), ptr(t["rot"]), int(full_sh))
    r._n = n
    return rc


@pytest.mark.parametrize("storage", STORAGES)
def test_device_attributes_equal_the_packed_vertex_block(storage):
    a = attrs()
    host, devr = context(storage), context(storage)
    for n in NS:
        assert upload_vertices(host, vertex_block(a, n), ply_layout(), 1, False) == _capi.OK, host.last_error()
        assert upload_attributes(devr, a, n) == _capi.OK, devr.last_error()
        same_observations(observe(host, True), observe(devr, True), "n = %d" % n)
    # SH degree 0: asked for, or no f_rest given
    assert upload_vertices(host, vertex_block(a, 65), ply_layout(), 0, False) == _capi.OK, host.last_error()
    want = observe(host, False)
    for kw in ({"full_sh": 0}, {"rest": False}):
        assert upload_attributes(devr, a, 65, **kw) == _capi.OK, devr.last_error()
        same_observations(want, observe(devr, False), "degree 0 (%s)" % kw)
    host.close(), devr.close()


@pytest.mark.parametrize("name", ["xyz", "f_dc", "f_rest", "opacity", "log_scale", "rot"])
def test_an_attribute_array_needs_only_4_byte_alignment(name):
    a = attrs()
    host, devr = context(), context()
    assert upload_vertices(host, vertex_block(a, 1000), ply_layout(), 1, False) == _capi.OK, host.last_error()
    assert upload_attributes(devr, a, 1000, offset=name) == _capi.OK, devr.last_error()
    same_observations(observe(host, True), observe(devr, True), name + " one float into a larger tensor")
    host.close(), devr.close()


def test_device_attributes_against_the_host_import():
    """the bounds of tests/test_gpu_parity.py::test_gpu_ingest_matches_host_import: alpha rtol 1e-6, covariance within 3e-6 of the
    splat's largest entry (device expf / sqrt against glibc), positions and SH exact; zero quaternions become the identity and
    the others are normalised, as on the host"""
    a = attrs()
    n = 4097
    ref = scenes.cloud_from_attrs({k: np.array(v) for k, v in a.items()}, True).as_array()
    r = context()
    assert upload_attributes(r, a, n) == _capi.OK, r.last_error()
    got = r.download_cloud(True)
    np.testing.assert_array_equal(got[:, :3], ref[:, :3])
    np.testing.assert_array_equal(got[:, 4:16], ref[:, 4:16])
    np.testing.assert_array_equal(got[:, 25:], ref[:, 25:])
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-6)
    scale = np.abs(ref[:, 16:25]).max(axis=1, keepdims=True)
    assert (np.abs(got[:, 16:25] - ref[:, 16:25]) <= 3e-6 * scale).all()
    s = np.exp(a["log_scale"][7].astype(np.float64)) ** 2               # rot = 0: R = identity, Sigma = diag(s^2)
    np.testing.assert_allclose(got[7, 16:25].reshape(3, 3), np.diag(s), rtol=1e-5, atol=0)
    s = np.exp(a["log_scale"][8].astype(np.float64)) ** 2               # rot = (0, 0, 3, 0): a half turn about y, Sigma = diag(s^2) again
    np.testing.assert_allclose(got[8, 16:25].reshape(3, 3), np.diag(s), rtol=1e-5, atol=1e-12)
    r.close()


# ---- 5. failures ------------------------------------------------------------------------------------------------------------
def good_frame():
    r = context()
    stride, off = layout("ref", True)
    assert upload_records(r, pack_records(cloud_array(True)[:1000], stride, off), off, 1, False) == _capi.OK
    want = observe(r, True)["frame"]
    r.close()
    return want


@pytest.mark.parametrize("storage,bad,text", [("sh_fp16", 70000.0, "beyond the fp16 range (|c| >= 65520) of MSPLAT_STORAGE_SH_FP16"),
                                              ("sh_q8", float("nan"), "not finite: MSPLAT_STORAGE_SH_Q8 cannot quantise them")])
@pytest.mark.parametrize("route", ["records", "attributes"])
def test_f_rest_failures_are_the_host_routes(route, storage, bad, text):
    stride, off = layout("ref", True)
    r = context(storage)
    if route == "records":
        aos = cloud_array(True)[:1000].copy()
        aos[321, 40] = bad
        host = context(storage)
        assert upload_records(host, pack_records(aos, stride, off), off, 1, False) == _capi.ERR_UNSUPPORTED
        assert "1 f_rest values are " + text in host.last_error()
        host.close()
        rc = upload_records(r, pack_records(aos, stride, off), off, 1, True)
    else:
        a = {k: np.array(v) for k, v in attrs().items()}
        a["f_rest"][321, 17] = bad
        rc = upload_attributes(r, a, 1000)
    assert rc == _capi.ERR_UNSUPPORTED
    assert "1 f_rest values are " + text in r.last_error()
    f = r._args.load(*VIEW)
    assert r._lib.msplat_sort(r._ctx, *f) == _capi.ERR_NO_CLOUD
    # ... and the context takes a good upload afterwards (FP32 frames differ from compact ones: compare within the storage)
    ok = context(storage)
    buf = pack_records(cloud_array(True)[:1000], stride, off)
    assert upload_records(ok, buf, off, 1, False) == _capi.OK and upload_records(r, buf, off, 1, True) == _capi.OK, r.last_error()
    same_observations(observe(ok, True), observe(r, True), "the upload after the failure")
    ok.close(), r.close()


def test_refusals_come_before_any_read():
    import torch
    stride, off = layout("ref", True)
    o = _capi.AttrOffsets(*off)
    L = ply_layout()
    r = context()
    lib, h = r._lib, r._ctx
    t = torch.zeros(64, dtype=torch.float32, device="cuda:0")            # 256 bytes, 16-byte aligned
    torch.cuda.synchronize()
    base = t.data_ptr()
    assert base % 16 == 0
    INV, UNS = _capi.ERR_INVALID_ARG, _capi.ERR_UNSUPPORTED
    # a base 4 bytes off a 16-byte boundary
    assert lib.msplat_upload_cloud_device(h, C.c_void_p(base + 4), 1, 100, C.byref(o), 0) == INV and "16-byte" in r.last_error()
    assert lib.msplat_upload_ply_vertices_device(h, C.c_void_p(base + 4), 1, C.byref(L), 1) == INV
    # an attribute array 2 bytes off a 4-byte boundary
    p = C.c_void_p(base)
    assert lib.msplat_upload_attributes_device(h, 1, p, p, p, C.c_void_p(base + 2), p, p, 1) == INV and "4-byte" in r.last_error()
    # NULL with n = 5
    assert lib.msplat_upload_cloud_device(h, None, 5, stride, C.byref(o), 1) == INV
    assert lib.msplat_upload_cloud_device(h, p, 5, stride, None, 1) == INV
    assert lib.msplat_upload_ply_vertices_device(h, None, 5, C.byref(L), 1) == INV
    assert lib.msplat_upload_attributes_device(h, 5, p, p, p, p, None, p, 1) == INV
    # strides and offsets, as the host call; stride 1028
    assert lib.msplat_upload_cloud_device(h, p, 1, 102, C.byref(o), 0) == INV
    assert lib.msplat_upload_cloud_device(h, p, 1, 240, C.byref(o), 1) == INV and "beyond stride" in r.last_error()
    assert lib.msplat_upload_cloud_device(h, p, 1, 1028, C.byref(o), 1) == UNS
    # n = 2^24 + 1 with a pointer to 16 bytes
    small = torch.zeros(4, dtype=torch.float32, device="cuda:0")
    q = C.c_void_p(small.data_ptr())
    big = (1 << 24) + 1
    assert lib.msplat_upload_cloud_device(h, q, big, 100, C.byref(o), 0) == UNS and "2^24" in r.last_error()
    assert lib.msplat_upload_ply_vertices_device(h, q, big, C.byref(L), 1) == UNS
    assert lib.msplat_upload_attributes_device(h, big, q, q, q, q, q, q, 1) == UNS
    # none of them left a cloud, and the context is usable
    assert lib.msplat_sort(h, *r._args.load(*VIEW)) == _capi.ERR_NO_CLOUD
    assert upload_records(r, pack_records(cloud_array(True)[:1000], stride, off), off, 1, True) == _capi.OK, r.last_error()
    same_bits(observe(r, True)["frame"], good_frame(), "the upload after the refusals")
    r.close()


# ---- 6. lifetime ------------------------------------------------------------------------------------------------------------
def test_the_source_may_be_overwritten_and_freed_on_return():
    stride, off = layout("ref", True)
    r = context()
    t = dev(pack_records(cloud_array(True)[:1000], stride, off))
    o = _capi.AttrOffsets(*off)
    assert r._lib.msplat_upload_cloud_device(r._ctx, ptr(t), 1000, stride, C.byref(o), 1) == _capi.OK, r.last_error()
    r._n = 1000
    t.view(-1)[:] = 0xFF            # every float a NaN
    del t
    same_bits(observe(r, True)["frame"], good_frame(), "the frame after the source was overwritten and dropped")
    r.close()


# ---- 7. the viewer loop -----------------------------------------------------------------------------------------------------
def host_frame_of(a, n):
    ref = context()
    assert upload_vertices(ref, vertex_block(a, n), ply_layout(), 1, False) == _capi.OK, ref.last_error()
    frame = observe(ref, True)["frame"]
    ref.close()
    return frame


def test_the_viewer_loop_updates_one_renderer_in_place():
    clouds = [synthetic.generate(2000, seed=900 + k, full_sh=True, log_scale_mean=-3.0) for k in range(3)]
    r = SplatRenderer(device=0)
    bytes_after = []
    steps = [(clouds[0], 1000), (clouds[1], 1000), (clouds[2], 1000), (clouds[0], 500), (clouds[1], 2000)]
    for step, (a, n) in enumerate(steps):
        t = [dev(a[k][:n]) for k in ("xyz", "f_dc", "f_rest", "opacity", "log_scale", "rot")]
        if step == 1:
            t[2] = t[2].reshape(n, 3, 15)
        ok = r.InitFromTensors(*t) if step == 0 else r.UpdateFromTensors(*t)
        assert ok, r.last_error()
        del t
        r.Sort(*VIEW)
        same_bits(u32(r.Render(*VIEW)), host_frame_of(a, n), "update %d (n = %d)" % (step, n))
        bytes_after.append(r.stats()["device_bytes"])
    assert bytes_after[0] == bytes_after[2], "a re-upload of the same n allocated: %s" % bytes_after[:3]
    assert bytes_after[3] == bytes_after[2], "a smaller cloud re-uses the store"
    r.close()
