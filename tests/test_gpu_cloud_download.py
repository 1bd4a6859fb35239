"""GPU tests of the downloads into device memory and msplat_export_ply: msplat_download_cloud_device against
msplat_download_cloud, bit for bit, and back through msplat_upload_cloud_device; msplat_download_attributes_device,
msplat_download_ply_vertices_device and the exported file against the rule of tests/egress_rule.py applied to the downloaded records
and against the covariance bound, which shares no formula with the kernel; upload numbering on a store in Morton order; the
context's state; the editing loop closed through a file; the refusals.  Clouds have at most 4097 splats, views are 256 x 160, sources
and destinations are torch tensors on cuda:0.  No test hands a host address to a device-pointer argument: that guard
(hipPointerGetAttributes, the first HIP call of each route) is checked by reading.  The five hand-written rows of the hostile
families are records no attribute tensor can produce (a covariance that is not symmetric), so that family is uploaded as records."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from splatapult_amd import PointRenderer, SplatRenderer, _capi
from tests import egress_rule as er
from tests import scenes
from tests.checks import check_image, same_bits
from tests.render_cases import ply_layout, random_points

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 1000, 4097)          # wave edges; 1, 63, 65, 1000 and 4097 records of 100 / 244 B end off a 16-byte boundary
VIEW = scenes.default_view(256, 160)
REF_OFF = (0, 16, 32, 48, 64, 76, 88, 100, 116, 132, 148, 164, 180, 196, 212, 228)
ON, OFF = _capi.SPATIAL_ON, _capi.SPATIAL_OFF
INGEST = 3e-6                                 # the ingest tests' covariance bound (device expf / sqrt against glibc)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def u8_tensor(nbytes, fill=0xA5):
    import torch
    t = torch.full((max(nbytes, 1),), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


def ptr(t, n=1):
    return C.c_void_p(t.data_ptr() if n else None)


@functools.lru_cache(maxsize=None)
def cloud_array(full_sh, n=4097, seed=41):
    """the records the tests upload (computed once, never changed), a negative zero and a denormal among the SH of record 5"""
    aos = scenes.synth_cloud(n, seed, full_sh=full_sh, log_scale_mean=-3.0).as_array().copy()
    aos[5, 5], aos[5, 6] = -0.0, 1e-40
    if full_sh:
        aos[5, 30], aos[5, 60] = 1e-40, -1e-41
    aos.setflags(write=False)
    return aos


def context(storage="fp32", **kw):
    r = SplatRenderer(device=0, cloud_storage=storage, **kw)
    assert r._create(False), r.last_error()
    return r


def upload(r, aos, device_ptr=None):
    """msplat_upload_cloud of the records (or msplat_upload_cloud_device of the same layout at device_ptr) into r's context 0"""
    n, full = aos.shape[0], aos.shape[1] == 61
    o = _capi.AttrOffsets(*REF_OFF)
    if device_ptr is None:
        a = np.ascontiguousarray(aos)
        rc = r._lib.msplat_upload_cloud(r._ctx, a.ctypes.data, n, a.shape[1] * 4, C.byref(o), int(full))
    else:
        rc = r._lib.msplat_upload_cloud_device(r._ctx, device_ptr, n, aos.shape[1] * 4, C.byref(o), int(full))
    assert rc == _capi.OK, r.last_error()
    r._n = n
    return r


def observe(r, full_sh, view=VIEW):
    """as uint32: the downloaded records, then after one Sort the keys and the sorted indices, then the frame"""
    got = {"storage": r.cloud_storage(), "cloud": u32(r.download_cloud(full_sh))}
    r.Sort(*view)
    got["keys"], got["indices"] = r.sorted_keys(), r.sorted_indices()
    got["frame"] = u32(r.Render(*view))
    return got


def same_observations(a, b, msg, keys=("cloud", "keys", "indices", "frame")):
    for k in keys:
        same_bits(a[k], b[k], "%s: %s differs" % (msg, k))


def records_device(r, full_sh, extra=64):
    """msplat_download_cloud_device into a tensor of 0xA5 that is `extra` bytes longer than the records -> (N, 25 | 61) uint32"""
    n, rec = r._n, 244 if full_sh else 100
    t = u8_tensor(n * rec + extra)
    rc = r._lib.msplat_download_cloud_device(r._ctx, ptr(t), n * rec)
    assert rc == _capi.OK, r.last_error()
    raw = t.cpu().numpy()
    assert (raw[n * rec:] == 0xA5).all(), "bytes behind the %d records were written" % n
    return raw[:n * rec].view(np.uint32).reshape(n, rec // 4), t


def tensors_np(t):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in t.items()}


def vertices_device(r, L, extra=64):
    """msplat_download_ply_vertices_device into 0xA5 -> (N, vertex_size) uint8"""
    n, vs = r._n, L.vertex_size
    t = u8_tensor(n * vs + extra)
    rc = r._lib.msplat_download_ply_vertices_device(r._ctx, ptr(t), n * vs, C.byref(L))
    assert rc == _capi.OK, r.last_error()
    raw = t.cpu().numpy()
    assert (raw[n * vs:] == 0xA5).all(), "bytes behind the %d vertices were written" % n
    return raw[:n * vs].reshape(n, vs)


def layout_without_rest():
    L = ply_layout()
    for i in range(45):
        L.f_rest[i] = -1
    L.vertex_size, L.opacity = 17 * 4, 36
    for i in range(3):
        L.scale[i] = 40 + 4 * i
    for i in range(4):
        L.rot[i] = 52 + 4 * i
    return L


def layout_offsets(L):
    """[(name, column, byte offset)] of the properties a layout has"""
    out = [("xyz", 0, L.x), ("xyz", 1, L.y), ("xyz", 2, L.z)] + [("f_dc", i, L.f_dc[i]) for i in range(3)]
    out += [("f_rest", i, L.f_rest[i]) for i in range(45)] + [("opacity", 0, L.opacity)]
    out += [("log_scale", i, L.scale[i]) for i in range(3)] + [("rot", i, L.rot[i]) for i in range(4)]
    return [p for p in out if p[2] >= 0]


def shuffled272():
    """a 272-byte vertex with the 59 properties at shuffled offsets and 36 bytes of gaps, made as the device-upload tests make their
    shuffled record"""
    rng = np.random.default_rng(272)
    order = rng.permutation(59)
    gaps = rng.multinomial((272 - 59 * 4) // 4, [1 / 60] * 60) * 4
    off, at = [0] * 59, 0
    for slot, k in enumerate(order):
        at += int(gaps[slot])
        off[k] = at
        at += 4
    assert at <= 272 and sorted(off) != off
    L = _capi.PlyLayout()
    L.vertex_size = 272
    L.x, L.y, L.z = off[0:3]
    for i in range(3):
        L.f_dc[i] = off[3 + i]
    for i in range(45):
        L.f_rest[i] = off[6 + i]
    L.opacity = off[51]
    for i in range(3):
        L.scale[i] = off[52 + i]
    for i in range(4):
        L.rot[i] = off[55 + i]
    return L


def check_block(block, L, attrs, what):
    """every property the layout has holds the attribute's bits, every other byte of the vertex is 0"""
    n = block.shape[0]
    covered = np.zeros(L.vertex_size, bool)
    for name, col, off in layout_offsets(L):
        want = np.asarray(attrs[name], np.float32).reshape(n, -1)[:, col]
        got = np.ascontiguousarray(block[:, off:off + 4]).view(np.uint32)[:, 0]
        assert (got == u32(want)).all(), "%s: %s[%d] at offset %d differs" % (what, name, col, off)
        covered[off:off + 4] = True
    assert not block[:, ~covered].any(), "%s: a byte no property covers is not 0" % what


def records_close(got, want, what):
    """check 4's bounds between the records of a context that loaded an exported file and the records that were exported: copies exact,
    alpha rtol 2e-6 (a logit, then a sigmoid), covariance within the export's bound plus the ingest's 3e-6 of the largest entry"""
    full = want.shape[1] == 61
    cols = [0, 1, 2] + (list(range(4, 16)) + list(range(25, 61)) if full else [4, 8, 12])       # (SH degree 0: the file holds f_dc only)
    same_bits(u32(got[:, cols]), u32(want[:, cols]), what + ": positions and SH")
    np.testing.assert_allclose(got[:, 3], want[:, 3], rtol=2e-6, atol=0, err_msg=what + ": alpha")
    sym = lambda c: 0.5 * (c.reshape(-1, 3, 3).astype(np.float64) + c.reshape(-1, 3, 3).astype(np.float64).transpose(0, 2, 1))
    a, b = sym(got[:, 16:25]), sym(want[:, 16:25])
    top = np.abs(b).max(axis=(1, 2))
    ls = er.export_rule(want)["log_scale"]
    L = np.where(np.isfinite(ls), np.abs(ls), np.float32(0)).max(axis=1).astype(np.float32)
    bound = (3.0 * np.spacing(L).astype(np.float64) + 2.0 ** -21 + INGEST) * top
    err = np.abs(a - b).max(axis=(1, 2))
    assert (err <= bound).all(), "%s: covariance off by %.3g of the largest entry" % (what, (err / np.maximum(top, 1e-300)).max())


# ---- 1. records -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON])
@pytest.mark.parametrize("storage,full_sh", [("fp32", 1), ("fp32", 0), ("sh_fp16", 1), ("sh_fp16", 0), ("sh_q8", 1)])
def test_device_records_equal_the_host_download_and_upload_again(storage, full_sh, spatial):
    r, back, host = context(storage, spatial_order=spatial), context(spatial_order=spatial), context(spatial_order=spatial)
    for n in NS:
        aos = cloud_array(bool(full_sh))[:n]
        upload(r, aos)
        assert r.cloud_storage() == storage and (r.storage_order() is not None) == (spatial == ON and n > 1)
        want = r.download_cloud(bool(full_sh))
        got, t = records_device(r, bool(full_sh))
        same_bits(got, u32(want), "%s, n = %d: msplat_download_cloud_device against msplat_download_cloud" % (storage, n))
        if storage == "fp32" and n:
            same_bits(got, u32(aos), "the FP32 device download is the upload, bit for bit")
        # ... and the records feed msplat_upload_cloud_device with the reference offsets
        upload(back, want, device_ptr=ptr(t, n))
        upload(host, want)
        same_observations(observe(host, bool(full_sh)), observe(back, bool(full_sh)), "%s, n = %d: uploaded again" % (storage, n))
    r.close(), back.close(), host.close()


# ---- 2. attributes against the host -----------------------------------------------------------------------------------------
def family_renderer(family, **kw):
    import torch
    r = SplatRenderer(device=0, **kw)
    if family == "hand":
        assert r.Init(np.array(er.family_records("hand"))), r.last_error()
    else:
        a = er.family_attrs(family)
        t = [torch.from_numpy(np.array(a[k])).to("cuda:0") for k in er.NAMES]
        assert r.InitFromTensors(*t), r.last_error()
    return r


@pytest.mark.parametrize("family", er.FAMILIES)
def test_device_attributes_are_the_host_export_of_the_downloaded_records(family, tmp_path):
    r = family_renderer(family)
    rec = r.download_cloud(True)
    t = r.DownloadTensors()
    assert t is not None, r.last_error()
    assert all(str(v.device) == "cuda:0" and v.dtype.is_floating_point for v in t.values()) and tuple(t["opacity"].shape) == (r._n,)
    got = tensors_np(t)
    rule = er.export_rule(rec)
    er.close_to_rule(got, rule, family + ": the device against the rule")
    # GaussianCloud.ExportPly of the downloaded records themselves
    path = str(tmp_path / "host.ply")
    assert er.host_cloud(rec).ExportPly(path)
    er.close_to_rule(got, er.block_attrs(er.read_ply(path)[1]), family + ": the device against GaussianCloud.ExportPly")
    worst = er.check_covariance(got, rec, family)
    same = int((u32(got["rot"]) == u32(rule["rot"])).all(axis=1).sum())
    print("%s: %d of %d rot rows bit-identical to the rule; worst covariance error %.3g of the largest entry" % (family, same, r._n, worst))
    if family != "hand":
        assert (u32(got["xyz"]) == u32(er.family_attrs(family)["xyz"])).all(), "row i is not the splat uploaded as i"
    # without f_rest: the other five are the same
    t5 = r.DownloadTensors(f_rest=False)
    assert t5 is not None and t5["f_rest"] is None
    for k in er.NAMES:
        if k != "f_rest":
            same_bits(t5[k].cpu().numpy(), got[k], family + ": " + k + " without f_rest")
    r.close()


def test_a_degree_0_cloud_exports_zeros_for_f_rest():
    r = upload(context(), cloud_array(False)[:1000])
    got = tensors_np(r.DownloadTensors())
    assert got["f_rest"].shape == (1000, 45) and not u32(got["f_rest"]).any()
    er.close_to_rule(got, er.export_rule(r.download_cloud(False)), "degree 0")
    r.close()


# ---- 3. vertex block --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON])
def test_the_vertex_block_holds_the_six_tensors_and_zeros(spatial):
    r = upload(context(spatial_order=spatial), cloud_array(True)[:1001])           # a last wave of 41 vertices: 10168 bytes, no multiple of 16
    attrs = tensors_np(r.DownloadTensors())
    L = ply_layout()
    block = vertices_device(r, L)
    check_block(block, L, attrs, "write_ply's layout")
    same_bits(np.ascontiguousarray(block).view(np.uint32), u32(er.vertex_block(attrs, True)), "the block is ExportPly's vertex block")
    assert not block[:, 12:24].any(), "nx ny nz are zeros"
    S = shuffled272()
    shuffled = vertices_device(r, S)
    check_block(shuffled, S, attrs, "shuffled272")
    at = S.opacity
    S.opacity = -1
    skipped = vertices_device(r, S)
    check_block(skipped, S, attrs, "shuffled272 without opacity")
    assert not skipped[:, at:at + 4].any()
    keep = np.ones(272, bool)
    keep[at:at + 4] = False
    same_bits(skipped[:, keep], shuffled[:, keep], "the other properties are unchanged")
    r.close()


# ---- 4. the file ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,full_sh", [(4097, True), (1000, False)])
def test_the_exported_file_is_the_host_header_and_the_device_block_and_loads_again(n, full_sh, tmp_path):
    aos = cloud_array(full_sh)[:n]
    r = upload(context(), aos)
    path, host_path = str(tmp_path / "device.ply"), str(tmp_path / "host.ply")
    assert r.ExportPly(path), r.last_error()
    header, block = er.read_ply(path)
    gc = scenes.cloud_from_attrs({k: v[:n] for k, v in er.family_attrs("generate", 4097).items()}, full_sh)
    assert gc.GetNumGaussians() == n and gc.ExportPly(host_path)
    assert header == er.read_ply(host_path)[0], "the header is not msplat_cloud_export_ply's"
    assert block.shape == (n, 62 if full_sh else 17)
    L = ply_layout() if full_sh else layout_without_rest()
    same_bits(u32(block), np.ascontiguousarray(vertices_device(r, L)).view(np.uint32).reshape(n, -1), "the file's vertices are the device block")
    f = SplatRenderer(device=0)
    assert f.InitFromPly(path, True), f.last_error()
    assert f._n == n
    records_close(f.download_cloud(full_sh), r.download_cloud(full_sh), "the file loaded again")
    r.Sort(*VIEW), f.Sort(*VIEW)
    check_image(f.Render(*VIEW), r.Render(*VIEW))
    r.close(), f.close()


def test_an_empty_cloud_exports_a_header(tmp_path):
    r = upload(context(), cloud_array(True)[:0])
    path = str(tmp_path / "empty.ply")
    assert r.ExportPly(path), r.last_error()
    header, block = er.read_ply(path)
    assert b"element vertex 0\n" in header and block.shape == (0, 62) and os.path.getsize(path) == len(header)
    t = r.DownloadTensors()
    assert t is not None and all(v.shape[0] == 0 for v in t.values())
    assert r._lib.msplat_download_cloud_device(r._ctx, None, 0) == _capi.OK
    assert r._lib.msplat_download_ply_vertices_device(r._ctx, None, 0, C.byref(ply_layout())) == _capi.OK
    r.close()


# ---- 5. numbering and state -------------------------------------------------------------------------------------------------
def all_routes(r, h, tmp_path, name):
    """what every route writes through context h of renderer r, as uint32 / bytes"""
    keep, r._ctx = r._ctx, h
    try:
        out = {"records": records_device(r, True)[0], "block": vertices_device(r, ply_layout())}
        t = r.DownloadTensors()
        assert t is not None, r.last_error()
        out.update({k: u32(v) for k, v in tensors_np(t).items()})
        path = str(tmp_path / (name + ".ply"))
        assert r.ExportPly(path), r.last_error()
        out["file"] = np.frombuffer(open(path, "rb").read(), np.uint8)
    finally:
        r._ctx = keep
    return out


def test_every_route_writes_upload_numbering_and_leaves_the_context_alone(tmp_path):
    aos = cloud_array(True)
    plain = upload(context(spatial_order=OFF), aos)
    want = all_routes(plain, plain._ctx, tmp_path, "plain")
    same_bits(want["records"], u32(aos), "the plain context's records")
    r = upload(context(spatial_order=ON), aos)
    assert r.storage_order() is not None
    mask = np.arange(4097) % 3 != 0
    r.SetVisibility(mask)
    r.SetCrop(np.diag([0.5, 0.5, 0.5, 1.0]).astype(np.float32).T.reshape(16), "sphere")
    before = observe(r, True)
    assert 0 < len(before["keys"]) < 2800 and r.visibility()["hidden"] > 1300
    got = all_routes(r, r._ctx, tmp_path, "ordered")
    for k in want:
        same_bits(got[k], want[k], "spatial order, mask and crop: " + k)
    assert r.visibility()["has_mask"] and r.visibility()["crop"] == ("sphere", False)
    same_bits(u32(r.Render(*VIEW)), before["frame"], "a Render after the downloads draws the latest Sort")
    same_observations(observe(r, True), before, "the next Sort and Render")
    plain.close(), r.close()


def test_an_attached_context_and_frames_in_flight(tmp_path):
    import torch
    aos = cloud_array(True)
    plain = upload(context(spatial_order=OFF), aos)
    want = all_routes(plain, plain._ctx, tmp_path, "plain")
    fly = SplatRenderer(device=0, frames_in_flight=2, spatial_order=ON)           # (async_submit is on with frames in flight)
    assert fly.Init(np.array(aos)), fly.last_error()
    fbs = [torch.zeros((160, 256, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        fly.Sort(*VIEW)
        fly.Render(*VIEW, out_ptr=fbs[k].data_ptr(), pitch_bytes=256 * 16)
    # frames are in flight on both contexts: the attached one (context 1) exports its owner's finished cloud
    got = all_routes(fly, fly._ctxs[1], tmp_path, "attached")
    for k in want:
        same_bits(got[k], want[k], "the attached context with frames in flight: " + k)
    fly.synchronize()
    one = upload(context(spatial_order=ON), aos)
    one.Sort(*VIEW)
    frame = u32(one.Render(*VIEW))
    for k in range(2):
        same_bits(u32(fbs[k].cpu().numpy()), frame, "frame %d in flight" % k)
    plain.close(), fly.close(), one.close()


# ---- 6. the loop closes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "sh_q8"])
def test_the_editing_loop_ends_in_a_file_a_fresh_context_loads(storage, tmp_path):
    r = SplatRenderer(device=0, cloud_storage=storage)
    assert r.Init(np.array(cloud_array(True)[:1000])), r.last_error()
    other = SplatRenderer(device=0, cloud_storage=storage)
    assert other.Init(np.array(cloud_array(True, 600, 43))), other.last_error()
    c, s = np.cos(0.6), np.sin(0.6)
    M = np.array([[c, 0, s, 0.4], [0, 1, 0, -0.2], [-s, 0, c, 0.1], [0, 0, 0, 1]], np.float32)       # a turn about y, moved
    r.TransformCloud(M.T.reshape(16), np.arange(1000) % 2 == 0)
    k, _ = r.AppendCloud(other, np.arange(600) % 3 != 1)
    assert k == 400
    r.SetCrop(np.diag([0.4, 0.4, 0.4, 1.0]).astype(np.float32).T.reshape(16), "sphere")
    kept = r.CompactCloud()
    assert 200 < kept < 1300
    path = str(tmp_path / "edited.ply")
    assert r.ExportPly(path), r.last_error()
    edited = r.download_cloud(True)
    header, block = er.read_ply(path)
    assert block.shape == (kept, 62)
    same_bits(u32(block[:, 9:54]), u32(er.export_rule(edited)["f_rest"]), "the exported f_rest are the stored (dequantised) values")
    f = SplatRenderer(device=0)
    assert f.InitFromPly(path, True), f.last_error()
    records_close(f.download_cloud(True), edited, storage + ": the edited cloud loaded again")
    r.Sort(*VIEW), f.Sort(*VIEW)
    assert r.sort_count() > 100
    check_image(f.Render(*VIEW), r.Render(*VIEW))
    r.close(), other.close(), f.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_and_leave_the_context_rendering(tmp_path):
    import torch
    lib = _capi.lib()
    INV, UNS, NOC, IO = _capi.ERR_INVALID_ARG, _capi.ERR_UNSUPPORTED, _capi.ERR_NO_CLOUD, _capi.ERR_IO
    n = 1000
    t = u8_tensor(n * 272 + 64)
    p, L = ptr(t), ply_layout()
    path = str(tmp_path / "refused.ply").encode()

    def calls(h, n_, p_):
        """the four calls with good arguments for a cloud of n_ splats"""
        return [("msplat_download_cloud_device", lambda: lib.msplat_download_cloud_device(h, p_, n_ * 244)),
                ("msplat_download_attributes_device", lambda: lib.msplat_download_attributes_device(h, n_, p_, p_, p_, p_, p_, p_)),
                ("msplat_download_ply_vertices_device", lambda: lib.msplat_download_ply_vertices_device(h, p_, n_ * 248, C.byref(L))),
                ("msplat_export_ply", lambda: lib.msplat_export_ply(h, path))]

    def refused(r, name, rc, code, *words):
        assert rc == code, (name, rc, r.last_error())
        assert name in r.last_error() and all(w in r.last_error() for w in words), (name, r.last_error())

    # before an upload
    c = context()
    for name, call in calls(c._ctx, n, p):
        refused(c, name, call(), NOC)
    c.close()
    # a point cloud: refused, and it still renders
    pr = PointRenderer(device=0)
    assert pr.Init(random_points(500, 3)), pr.last_error()
    want = pr.Render(*VIEW)
    for name, call in calls(pr._ctx, 500, p):
        refused(pr, name, call(), UNS, "point cloud")
    same_bits(pr.Render(*VIEW), want, "the points after the refusals")
    pr.close()
    assert not os.path.exists(path.decode())

    r = upload(context(), cloud_array(True)[:n])
    before = observe(r, True)
    h = r._ctx
    # one byte short
    refused(r, "msplat_download_cloud_device", lib.msplat_download_cloud_device(h, p, n * 244 - 1), INV)
    refused(r, "msplat_download_ply_vertices_device", lib.msplat_download_ply_vertices_device(h, p, n * 248 - 1, C.byref(L)), INV)
    # n = N + 1
    refused(r, "msplat_download_attributes_device", lib.msplat_download_attributes_device(h, n + 1, p, p, p, p, p, p), INV)
    # NULL destinations
    refused(r, "msplat_download_cloud_device", lib.msplat_download_cloud_device(h, None, n * 244), INV, "NULL")
    refused(r, "msplat_download_attributes_device", lib.msplat_download_attributes_device(h, n, p, p, p, None, p, p), INV, "d_opacity")
    refused(r, "msplat_download_ply_vertices_device", lib.msplat_download_ply_vertices_device(h, p, n * 248, None), INV)
    refused(r, "msplat_export_ply", lib.msplat_export_ply(h, None), INV)
    # a device pointer 4 bytes off for d_aos and d_vertices, 2 bytes off for d_xyz
    p4, p2 = C.c_void_p(t.data_ptr() + 4), C.c_void_p(t.data_ptr() + 2)
    refused(r, "msplat_download_cloud_device", lib.msplat_download_cloud_device(h, p4, n * 244), INV, "16-byte")
    refused(r, "msplat_download_ply_vertices_device", lib.msplat_download_ply_vertices_device(h, p4, n * 248, C.byref(L)), INV, "16-byte")
    refused(r, "msplat_download_attributes_device", lib.msplat_download_attributes_device(h, n, p2, p, p, p, p, p), INV, "d_xyz", "4-byte")
    # layout errors as msplat_upload_ply_vertices reports them
    bad = ply_layout()
    bad.rot[3] = 248
    refused(r, "msplat_download_ply_vertices_device", lib.msplat_download_ply_vertices_device(h, p, n * 272, C.byref(bad)), INV, "property offset 248")
    bad = ply_layout()
    bad.vertex_size = 1028
    refused(r, "msplat_download_ply_vertices_device", lib.msplat_download_ply_vertices_device(h, p, n * 1028, C.byref(bad)), UNS, "vertex size")
    # an unwritable path
    refused(r, "msplat_export_ply", lib.msplat_export_ply(h, str(tmp_path / "no_such_dir" / "x.ply").encode()), IO)
    assert (t.cpu().numpy() == 0xA5).all(), "a refused call wrote to its destination"
    same_bits(u32(r.Render(*VIEW)), before["frame"], "a Render after the refusals draws the latest Sort")
    same_observations(observe(r, True), before, "after the refusals")
    # ... and the good calls still work
    for name, call in calls(h, n, p):
        assert call() == _capi.OK, (name, r.last_error())
    r.close()
