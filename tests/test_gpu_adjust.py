"""GPU tests of msplat_adjust_cloud: the selected splats of a context's cloud recoloured and faded on the
device.  The reference of every comparison is merged behaviour, never the code under test -- a context that was uploaded the rule's
rows (tests/adjust_rule.py) of the download taken before the call, in the same storage and with the same spatial_order, or the
context before the call -- and every comparison is same_bits unless said otherwise: num_splats, the storage kind, the downloaded
records, the storage order, the cull boxes after a Sort and the frame's sort_count, keys, indices, pixels, drawn and pair counts.
Views are 256 x 160; the clouds have at most 4097 splats.  tests/test_adjust.py checks the rule and these fixtures on the CPU.  No
test hands a host address to msplat_adjust_cloud: its pointer guard (check_device_source, before anything is launched) is checked
by reading."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from splatapult_amd.points import PointRenderer
from tests import adjust_rule as ar
from tests import compact_harness as ch
from tests import overlay_rule as ov
from tests import transform_harness as th
from tests import visibility_rule as vr
from tests.checks import check_image, same_bits
from tests.gpu_harness import make_renderer, oracle_frame, sorted_frame
from tests.render_cases import random_points

pytestmark = pytest.mark.gpu

VIEW = vr.view()
OFF, ON = _capi.SPATIAL_OFF, _capi.SPATIAL_ON
MAPS = ar.maps()
# (cloud_storage, full SH): the three storages of a full-SH cloud, and an SH-degree-0 cloud (25-float rows)
STORES = {"fp32": ("fp32", True), "sh_fp16": ("sh_fp16", True), "sh_q8": ("sh_q8", True), "degree0": ("fp32", False)}
_P = C.POINTER(C.c_float)


def call_args(mode, m, scale):
    """(the rule's colour, AdjustCloud's colour, its opacity) of one call in `mode`"""
    flags = ar.MODES[mode]
    return (ar.abi(MAPS[m]) if flags & ar.COLOUR else None, MAPS[m] if flags & ar.COLOUR else None,
            ar.SCALES[scale] if flags & ar.OPACITY else None)


def rule_rows(before, mode, m, scale, select=None):
    c12, _, s = call_args(mode, m, scale)
    return ar.adjust_rows(before, c12, s, ar.MODES[mode], select)


def raw_adjust(r, colour=None, scale=1.0, d_select=None, n=None, flags=ar.COLOUR | ar.OPACITY):
    """msplat_adjust_cloud on the renderer's context, the return code; colour: the ABI's 12 floats or None"""
    c = None if colour is None else np.ascontiguousarray(colour, np.float32).ctypes.data_as(_P)
    return _capi.lib().msplat_adjust_cloud(r._ctx, c, C.c_float(scale), d_select, r._n if n is None else n, flags)


def adjusted_equals_the_upload(aos, mode, m, scale, select, what, make=make_renderer, **kw):
    """a context uploaded `aos` and adjusted, against a context uploaded the rule's rows of its download"""
    full_sh = aos.shape[1] == 61
    r = make(aos, **kw)
    before = r.download_cloud(full_sh)
    storage = r.cloud_storage()
    _, colour, opacity = call_args(mode, m, scale)
    r.AdjustCloud(colour, opacity, select)
    with pytest.raises(_capi.MsplatError) as e:                  # has_sort is cleared: Sort first
        r.Render(*VIEW)
    assert e.value.code == _capi.ERR_NO_SORT, what
    got = ch.context_state(r, VIEW, full_sh)
    assert r.cloud_storage() == storage, what
    rows = rule_rows(before, mode, m, scale, select)
    ch.assert_same_context(got, th.uploaded_state(rows, VIEW, cloud_storage=storage, spatial_order=kw["spatial_order"]), what)
    if select is not None:
        same_bits(got["cloud"][np.asarray(select) == 0], before[np.asarray(select) == 0], "%s: the unselected rows" % what)
    r.close()


# ---- 1. the adjusted context equals the upload of the rule's rows -------------------------------------------------------------
# every select case in one of the three modes, the maps and the scales taking turns; then the three modes on one selection
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("n", ar.SIZES)
def test_an_adjusted_context_equals_the_upload_of_the_rules_rows(n, store, spatial):
    storage, full_sh = STORES[store]
    aos = ar.cloud(n, full_sh)
    if store == "sh_q8":
        # the reference uploads downloaded rows, which quantises them again, and an opacity-only call copies the codes: on rows at a
        # fixed point of the quantiser (tests/test_adjust.py) the two are the same bits
        aos = ar.q8_stable(aos)
    cases = ar.select_cases(n)
    modes, maps, scales = list(ar.MODES), list(MAPS), list(ar.SCALES)
    for i, (name, select) in enumerate(cases.items()):
        mode, m, scale = modes[i % 3], maps[i % len(maps)], scales[(i + 1) % len(scales)]
        if store == "sh_q8" and mode != "opacity":
            # (with colour every splat is selected, as in the transform's test)
            select, name = None, "none"
        adjusted_equals_the_upload(aos, mode, m, scale, select, "n %d, %s, %s, %s, %s, %s" % (n, store, name, mode, m, scale),
                                   cloud_storage=storage, spatial_order=spatial)
    select = None if store == "sh_q8" else cases["random_30"]
    for mode, m, scale in (("colour", "negative", "one"), ("both", "gain4", "straddle")):
        adjusted_equals_the_upload(aos, mode, m, scale, select, "n %d, %s, random_30, %s, %s, %s" % (n, store, mode, m, scale),
                                   cloud_storage=storage, spatial_order=spatial)
    adjusted_equals_the_upload(aos, "opacity", "identity", "straddle", cases["random_30"], "n %d, %s, random_30, opacity, straddle" % (n, store),
                               cloud_storage=storage, spatial_order=spatial)


def test_the_swap_applied_twice_returns_the_cloud():
    n = 257
    aos = ar.cloud(n)
    r = make_renderer(aos, spatial_order=ON)
    r.AdjustCloud(MAPS["swap"])
    once = r.download_cloud(True)
    assert not np.array_equal(once, aos)
    r.AdjustCloud(MAPS["swap"])
    # an exact permutation with a bias of 0: only the sign of a zero can differ (-0 + 0 = +0)
    np.testing.assert_array_equal(r.download_cloud(True), aos)
    r.close()


# ---- 2. per row, in every storage ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
@pytest.mark.parametrize("store", list(STORES))
def test_unselected_rows_keep_their_bits_and_selected_rows_are_the_stores_encoding_of_the_rule(store, spatial):
    storage, full_sh = STORES[store]
    n = 1000
    aos, select = ar.cloud(n, full_sh), ar.wave_select(n)
    r = make_renderer(aos, cloud_storage=storage, spatial_order=spatial)
    before = r.download_cloud(full_sh)
    sh = [c for c in range(4, 16)] + [c for c in range(25, before.shape[1])]
    for mode, m, scale in (("colour", "tint", "one"), ("both", "negative", "half"), ("opacity", "identity", "straddle"),
                           ("opacity", "identity", "two"), ("both", "grey", "zero")):
        _, colour, opacity = call_args(mode, m, scale)
        r.AdjustCloud(colour, opacity, select)
        got = r.download_cloud(full_sh)
        what = "%s, %s %s %s" % (store, mode, m, scale)
        assert r.cloud_storage() == storage and r.stats()["num_splats"] == n
        same_bits(got[~select], before[~select], "%s: the unselected rows" % what)
        rule = rule_rows(before, mode, m, scale, select)
        if mode == "opacity":
            # nothing is decoded: every column but alpha keeps its bits in every row, selected or not, in every storage
            same_bits(np.delete(got, 3, axis=1), np.delete(before, 3, axis=1), "%s: every column except alpha" % what)
            same_bits(got[:, 3], rule[:, 3], "%s: alpha" % what)
        else:
            same_bits(got[select], ar.stored(rule, storage)[select], "%s: the selected rows" % what)
            assert (got[select][:, sh] != before[select][:, sh]).any(axis=1).all(), what
        if mode == "colour":
            same_bits(got[:, 3], before[:, 3], "%s: alpha" % what)
        before = got
    r.close()


# ---- 3. a fade ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
def test_a_fade_of_a_selection_gives_the_frame_of_the_rules_rows_and_the_oracles_image(spatial):
    n = vr.TIE_FREE[0]
    aos, select = ar.cloud(n), vr.random_mask(n, seed=6, share=0.4)
    cam, proj, vp, nf = VIEW
    r = make_renderer(aos, spatial_order=spatial)
    whole = sorted_frame(r, VIEW)
    r.AdjustCloud(opacity=ar.SCALES["2^-9"], select=select)
    rows = rule_rows(aos, "opacity", "identity", "2^-9", select)
    got = sorted_frame(r, VIEW)
    s = make_renderer(rows, spatial_order=spatial)
    ch.assert_same_frame(got, sorted_frame(s, VIEW), "the frame after the fade")
    s.close()
    assert not np.array_equal(got["img"], whole["img"])          # the faded splats no longer change a pixel
    ref = oracle_frame(rows, True, cam, proj, vp, nf, r=r)
    assert ref["V"] == got["V"]
    print("max |diff| against the oracle %.3g" % np.abs(got["img"] - ref["image"]).max())
    check_image(got["img"], ref["image"], budget=ref["budget"])
    r.close()


# ---- 4. mask, crop and overlay classes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
def test_the_mask_is_kept_and_hides_the_same_upload_indices(spatial):
    n = vr.TIE_FREE[0]
    aos, mask, select = ar.cloud(n), vr.random_mask(n, seed=8, share=0.5), vr.random_mask(n, seed=6, share=0.4)
    r = make_renderer(aos, spatial_order=spatial)
    before = r.download_cloud(True)
    r.SetVisibility(mask)
    r.AdjustCloud(MAPS["tint"], 0.5, select)
    assert r.visibility()["has_mask"]
    got = ch.context_state(r, VIEW, True)
    assert r.visibility() == dict(has_mask=True, crop=None, hidden=int((~mask).sum())), r.visibility()
    rows = rule_rows(before, "both", "tint", "half", select)
    ref = th.uploaded_state(rows, VIEW, mask=mask, spatial_order=spatial)
    ch.assert_same_context(got, ref, "a mask set before the call")
    assert 0 < got["frame"]["V"] < n and mask[got["frame"]["idx"]].all()
    r.close()


def test_a_crop_set_before_the_call_is_kept():
    aos = vr.crop_cloud()
    n, crop = aos.shape[0], (vr.matrices()["scaled"], "box", False)
    r = make_renderer(aos, spatial_order=OFF)
    r.SetCrop(*crop)
    hidden = int((~vr.crop(aos[:, 0:3], crop[0], "box")).sum())
    assert 0 < hidden < n
    r.Sort(*VIEW)
    assert r.visibility()["hidden"] == hidden
    r.AdjustCloud(MAPS["grey"], 0.5)
    rows = rule_rows(aos, "both", "grey", "half")
    got = ch.context_state(r, VIEW, True)
    assert r.visibility() == dict(has_mask=False, crop=("box", False), hidden=hidden), r.visibility()      # the centres did not move
    ch.assert_same_context(got, th.uploaded_state(rows, VIEW, crop=crop, spatial_order=OFF), "a crop set before the call")
    r.close()


@pytest.mark.parametrize("flight", [1, 2])
@pytest.mark.parametrize("spatial", [OFF, ON], ids=["upload_order", "morton_order"])
def test_the_overlay_classes_are_kept_and_tint_the_same_upload_indices(spatial, flight):
    n = 257
    aos, select = ar.cloud(n), vr.random_mask(n, seed=6, share=0.4)
    classes, palette = np.random.default_rng(77).integers(0, 4, n).astype(np.uint8), ov.palette(3)
    a = make_renderer(aos, spatial_order=spatial, frames_in_flight=flight)
    a.SetOverlay(classes, palette)
    a.AdjustCloud(MAPS["negative"], 0.5, select)
    assert a.overlay() == dict(has_classes=True, palette_count=3, active=True), a.overlay()
    b = make_renderer(rule_rows(aos, "both", "negative", "half", select), spatial_order=spatial)
    b.SetOverlay(classes, palette)
    plain = make_renderer(rule_rows(aos, "both", "negative", "half", select), spatial_order=spatial)
    want, untinted = sorted_frame(b, VIEW), sorted_frame(plain, VIEW)
    assert not np.array_equal(want["img"], untinted["img"])      # the classes do something
    for k in range(flight):                                      # every context of the rotation
        ch.assert_same_frame(sorted_frame(a, VIEW), want, "after AdjustCloud, frame %d" % k)
    for r in (a, b, plain):
        r.close()


def test_four_frames_in_flight_all_render_the_adjusted_cloud_under_the_mask():
    n = 4097
    aos, mask = ar.cloud(n), vr.random_mask(n, seed=8, share=0.5)
    rows = rule_rows(aos, "both", "tint", "half")
    s = make_renderer(rows, spatial_order=OFF)
    s.SetVisibility(mask)
    want = sorted_frame(s, VIEW)
    s.close()
    fly = make_renderer(aos, spatial_order=OFF, frames_in_flight=4)
    fly.SetVisibility(mask)
    for _ in range(2):                                           # two frames are in flight when the call comes
        fly.Sort(*VIEW)
    fly.AdjustCloud(MAPS["tint"], 0.5)
    seen = set()
    for f in range(4):
        ch.assert_same_frame(sorted_frame(fly, VIEW), want, "frame %d after the call" % f)
        assert fly.visibility()["has_mask"], f
        seen.add(fly._ctx.value)
    assert len(seen) == 4                                        # one frame per context
    fly.close()


# ---- 5. refusals and failures -------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    n = 257
    aos = ar.cloud(n)
    tint = ar.abi(MAPS["tint"])
    r = make_renderer(aos, spatial_order=ON)
    r.SetVisibility(vr.mask_cases(n)["every_other"])
    before = ch.context_state(r, VIEW, True)
    L = _capi.lib()
    assert raw_adjust(r, tint, 0.5, flags=0) == _capi.ERR_INVALID_ARG
    assert raw_adjust(r, tint, 0.5, flags=4) == _capi.ERR_INVALID_ARG
    assert raw_adjust(r, tint, 0.5, flags=ar.COLOUR | 0x100) == _capi.ERR_INVALID_ARG
    same_bits(r.Render(*VIEW), before["frame"]["img"], "a Render after the refusal draws the latest Sort")
    assert raw_adjust(r, None, 0.5, flags=ar.COLOUR) == _capi.ERR_INVALID_ARG
    assert raw_adjust(r, None, 0.5, flags=ar.COLOUR | ar.OPACITY) == _capi.ERR_INVALID_ARG
    for k in (0, 7, 11):                                         # G and the offset are checked
        for v in (np.nan, np.inf):
            bad = tint.copy()
            bad[k] = v
            assert raw_adjust(r, bad, 0.5, flags=ar.COLOUR) == _capi.ERR_INVALID_ARG, (k, v)
    for s in (np.nan, np.inf, -0.5):
        assert raw_adjust(r, tint, s, flags=ar.OPACITY) == _capi.ERR_INVALID_ARG, s
        assert raw_adjust(r, tint, s, flags=ar.COLOUR | ar.OPACITY) == _capi.ERR_INVALID_ARG, s
    assert raw_adjust(r, tint, 0.5, n=n - 1) == _capi.ERR_INVALID_ARG
    assert raw_adjust(r, tint, 0.5, n=n + 1) == _capi.ERR_INVALID_ARG
    assert L.msplat_adjust_cloud(None, tint.ctypes.data_as(_P), C.c_float(0.5), None, n, ar.COLOUR) == _capi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        r.AdjustCloud(MAPS["tint"], select=np.ones(n - 1, bool))
    with pytest.raises(ValueError):
        r.AdjustCloud(MAPS["tint"], select=np.ones(n, np.float32))
    with pytest.raises(ValueError):
        r.AdjustCloud()
    assert r.visibility()["has_mask"]
    same_bits(r.Render(*VIEW), before["frame"]["img"], "a Render after the refusals")
    th.assert_same_context_again(ch.context_state(r, VIEW, True), before, "after the refusals")
    r.close()
    # a point cloud: refused, and it still renders
    p = PointRenderer(device=0)
    assert p.Init(random_points(500, 3)), p.last_error()
    want = p.Render(*VIEW)
    assert L.msplat_adjust_cloud(p._ctx, tint.ctypes.data_as(_P), C.c_float(0.5), None, 500, ar.COLOUR | ar.OPACITY) == _capi.ERR_UNSUPPORTED
    same_bits(p.Render(*VIEW), want, "the points after the refusal")
    p.close()
    # no cloud
    c = SplatRenderer(device=0)
    assert c._create(False), c.last_error()
    assert L.msplat_adjust_cloud(c._ctx, tint.ctypes.data_as(_P), C.c_float(0.5), None, 0, ar.COLOUR | ar.OPACITY) == _capi.ERR_NO_CLOUD
    c.close()


def test_an_fp16_overflow_after_the_gain_fails_and_changes_nothing():
    aos, row = ar.overflow_cloud()
    n = aos.shape[0]
    r = make_renderer(aos, cloud_storage="sh_fp16", spatial_order=ON)
    before = ch.context_state(r, VIEW, True)
    assert raw_adjust(r, ar.abi(MAPS["gain4"]), 1.0, flags=ar.COLOUR) == _capi.ERR_UNSUPPORTED
    assert "fp16" in r.last_error() and "adjusted" in r.last_error()
    same_bits(r.Render(*VIEW), before["frame"]["img"], "a Render after the failure draws the latest Sort")
    same_bits(r.download_cloud(True), before["cloud"], "the download after the failure")
    th.assert_same_context_again(ch.context_state(r, VIEW, True), before, "after the failure")
    sel = np.ones(n, bool)
    sel[row] = False
    r.AdjustCloud(MAPS["gain4"], select=sel)                     # without that splat the call goes through
    got = r.download_cloud(True)
    same_bits(got[row], before["cloud"][row], "the unselected splat")
    same_bits(got[sel], ar.stored(rule_rows(before["cloud"], "colour", "gain4", "one", sel), "sh_fp16")[sel], "the selected splats")
    r.close()


# ---- 6. an attached context ---------------------------------------------------------------------------------------------------
def test_an_attached_context_renders_the_old_cloud_until_it_is_attached_again():
    L = _capi.lib()
    n = 4097
    aos = ar.cloud(n)
    a = make_renderer(aos, spatial_order=ON)                     # the owner
    b = SplatRenderer(device=0, spatial_order=ON)
    assert b._create(False), b.last_error()
    assert L.msplat_attach_cloud(b._ctx, a._ctx) == _capi.OK, b.last_error()
    b._n = n
    whole = ch.context_state(a, VIEW, True)
    a.AdjustCloud(MAPS["tint"], 0.5)
    new = th.uploaded_state(rule_rows(aos, "both", "tint", "half"), VIEW, spatial_order=ON)
    th.assert_same_context_again(ch.context_state(a, VIEW, True), new, "the owner")
    th.assert_same_context_again(ch.context_state(b, VIEW, True), whole, "the attached context of a store its owner adjusted")
    assert L.msplat_attach_cloud(b._ctx, a._ctx) == _capi.OK, b.last_error()
    th.assert_same_context_again(ch.context_state(b, VIEW, True), new, "attached again")
    a.close(), b.close()


# ---- 7. a small grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 5])
def test_a_small_grid_changes_nothing(cap, monkeypatch):
    n = 4097                                                     # 65 waves of 64 records: 65 and 13 turns of the grid-stride loop
    make = lambda aos, **kw: ch.capped_renderer(aos, monkeypatch, cap, **kw)
    for store in ("fp32", "sh_fp16"):
        adjusted_equals_the_upload(ar.cloud(n), "both", "negative", "straddle", ar.wave_select(n), "MSPLAT_GRID_CAP=%d, %s" % (cap, store),
                                   make=make, cloud_storage=store, spatial_order=ON)


# ---- 8. the C++ shim and example_render --fade / --tint -----------------------------------------------------------------------
def test_example_render_fades_and_tints_the_cloud_it_draws(tmp_path, golden_dir):
    """SplatRenderer::AdjustCloud (msplat_host.hpp) through example_render: the frame after --fade and --tint is the oracle's image
    of the rule's rows (check_image's bounds: the tool's camera is the oracle's to rounding), and --save writes those rows"""
    import os
    import subprocess
    from splatapult_amd import GaussianCloud, camera
    from tests import scenes
    from tests.conftest import ROOT
    exe, libdir = str(tmp_path / "example_render"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-I", ROOT, os.path.join(ROOT, "splatapult_amd", "host", "example_render.cpp"),
                    "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    W, H = 320, 200
    ply, out, saved = os.path.join(golden_dir, "test.ply"), str(tmp_path / "o.f32"), str(tmp_path / "adjusted.ply")
    subprocess.run([exe, ply, out + "0", str(W), str(H)], check=True, timeout=120)
    subprocess.run([exe, ply, out, str(W), str(H), "--fade", "0.5", "--tint", "1,0.5,0.25,0.3", "--save", saved], check=True, timeout=120)
    plain, img = (np.fromfile(p, np.float32).reshape(H, W, 4) for p in (out + "0", out))
    assert np.abs(img - plain).max() > 0.05                      # the frame changed
    gc = GaussianCloud()
    assert gc.ImportPly(ply)
    rows = ar.adjust_rows(gc.as_array(), ar.abi(ar.tint((1.0, 0.5, 0.25), 0.3)), 0.5, ar.COLOUR | ar.OPACITY)
    cam = camera.pose((0.0, 0.0, 5.0))
    proj = camera.perspective(np.float32(45.0 * 3.14159265358979 / 180.0), W / H)
    ref = oracle_frame(rows, True, cam, proj, [0, 0, W, H], scenes.NF)
    check_image(img, ref["image"], budget=ref["budget"])
    back = GaussianCloud()
    assert back.ImportPly(saved)
    got = back.as_array()
    # the tool builds G = (1 - A) I and o = A (R, G, B) in fp32, the rule's map here is rounded once from float64: every entry and
    # the bias within an ulp, so a coefficient of magnitude <= m differs by at most 2^-23 (m + 1) plus its own rounding; asserted 2^-21
    sh = [c for c in range(4, 16)] + [c for c in range(25, 61)]
    err = np.abs(got[:, sh].astype(np.float64) - rows[:, sh])
    assert err.max() <= 2.0 ** -21 * (1.0 + np.abs(rows[:, sh]).max()), err.max()
    # alpha goes through the PLY's logit x = -log(1 / alpha - 1) and back: d alpha / alpha = (1 - alpha) dx, and the seven fp32
    # operations of the round trip leave |dx| <= 2^-23 (|x| + 3) / (1 - alpha); asserted 2^-23 (|x| + 4) alpha
    a = rows[:, 3].astype(np.float64)
    assert (a > 0).all() and (a <= 0.5).all()
    x = np.abs(np.log(1.0 / a - 1.0))
    assert (np.abs(got[:, 3] - a) <= 2.0 ** -23 * (x + 4.0) * a).all(), float((np.abs(got[:, 3] - a) / (2.0 ** -23 * (x + 4.0) * a)).max())
    same_bits(got[:, 0:3], rows[:, 0:3], "the centres")
