"""The HIP path against the REFERENCE'S OWN SHADERS (round 4).

tests/golden/glref_*.npz hold what /root/reference/shader/presort_compute.glsl and splat_{vert,geom,frag}.glsl computed for the
scenes of tests/glref_cases.py when executed by Mesa llvmpipe in the build container (tests/golden/make_glref_golden.py,
oracle/glref/glref.c).  Here libmsplat.so renders the same scenes through the C ABI on the MI355X and is compared with those
outputs directly -- not with this repo's restatement of the shaders:
  visible set, 32-bit depth keys, draw order ... exact
  framebuffer ................................. SURVEY 8c: max |diff| <= 5e-3 (+ the oracle's threshold-flip budget), mean <= 1e-4,
                                                >= 99.9 % of values within 1e-4; alpha == 1
The CPU suite checks the oracle against the same fixtures (tests/test_oracle.py) and, in the build container, against the shaders
themselves (tests/test_reference_shaders.py)."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from splatapult_amd import SplatRenderer
from tests import glref_cases

pytestmark = pytest.mark.gpu
CASES = glref_cases.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_path_matches_the_reference_shaders(name):
    c = CASES[name]
    g = np.load(os.path.join(glref_cases.GOLDEN, "glref_%s.npz" % name))
    assert str(g["digest"]) == glref_cases.digest(c["aos"]), "the scene generator no longer reproduces the fixture's cloud"
    assert "llvmpipe" in str(g["gl_version"])
    vp = [0, 0, c["W"], c["H"]]
    r = SplatRenderer(device=0)
    assert r.Init(c["aos"], c["srgb"], False), r.last_error()
    r.Sort(c["cam"], c["proj"], vp, c["nf"])
    # presort_compute.glsl's output, bit for bit: which splats survive, and their keys
    assert r.sort_count() == g["keys"].shape[0]
    order = np.argsort(r.sorted_indices(), kind="stable")
    np.testing.assert_array_equal(r.sorted_indices()[order], g["idx"])
    np.testing.assert_array_equal(r.sorted_keys()[order], g["keys"])
    np.testing.assert_array_equal(r.sorted_indices(), g["draw_order"])          # ascending key, ties by index
    rcam = c["cam"] if c["render_cam"] is None else c["render_cam"]
    rproj = c["proj"] if c["render_proj"] is None else c["render_proj"]
    img = r.Render(rcam, rproj, vp, c["nf"])
    assert (img[..., 3] == 1.0).all()
    d = np.abs(img[..., :3].astype(np.float64) - g["rgb"])
    # fragments within 1e-4 of the w = 1/256 discard threshold may fall on either side: the oracle says how much that can move a pixel
    ref = orc.render_frame(c["aos"], c["full_sh"], c["cam"], c["proj"], vp, c["nf"], render_cam=c["render_cam"],
                           render_proj=c["render_proj"], srgb=c["srgb"], want_image=False, want_splats=True)
    _, budget = orc.composite_flip(ref["splats"], c["W"], c["H"])
    print("HIP vs reference shaders (%s): V %d, max |diff| %.3g, mean %.3g, within 1e-4: %.5f" % (
        name, g["keys"].shape[0], d.max(), d.mean(), (d <= 1e-4).mean()))
    assert d.mean() <= 1e-4 and (d <= 1e-4).mean() >= 0.999
    assert (d.max(axis=-1) <= 5e-3 + budget).all(), "max |diff| %.3g beyond the threshold-flip budget" % d.max()


@pytest.mark.parametrize("name", glref_cases.LADDER_NAMES)
def test_projection_ladder_matches_the_reference_shaders(name):
    """the projection's conditioning ladder (glref_projection_limits.npz): visible set, keys and draw order of the shaders, the
    footprint rule's class of every rank as the fixture recorded it -- no rank of class Q or X, or rejected by the guard tests, has a
    rectangle --, and the frame of the drawable splats below glref_cases.LADDER_IMAGE_L drawn alone within SURVEY 8c"""
    from splatapult_amd import _capi
    c = glref_cases.ladder_case(name)
    g = np.load(os.path.join(glref_cases.GOLDEN, "glref_projection_limits.npz"))
    assert str(g[name + "_digest"]) == glref_cases.digest(c["aos"]), "the scene generator no longer reproduces the fixture's cloud"
    np.testing.assert_array_equal(g[name + "_cls"], c["cls"])
    vp = [0, 0, c["W"], c["H"]]
    one_pass = dict(spatial_order=_capi.SPATIAL_OFF, two_pass=_capi.TWO_PASS_OFF)
    r = SplatRenderer(device=0, **one_pass)
    assert r.Init(c["aos"], False, False), r.last_error()
    r.Sort(c["cam"], c["proj"], vp, c["nf"])
    order = np.argsort(r.sorted_indices(), kind="stable")
    np.testing.assert_array_equal(r.sorted_indices()[order], g[name + "_idx"])
    np.testing.assert_array_equal(r.sorted_keys()[order], g[name + "_keys"])
    np.testing.assert_array_equal(r.sorted_indices(), g[name + "_draw_order"])
    r.Render(c["cam"], c["proj"], vp, c["nf"])
    _, rect = r.debug_projected()
    drawn = (rect & 255) <= ((rect >> 16) & 255)
    assert not drawn[c["cls"] != 0].any(), "%d rank(s) of class Q, X or rejected by the guard tests have a rectangle" % drawn[c["cls"] != 0].sum()
    r.close()
    sel = glref_cases.ladder_g_image(c)
    part = np.ascontiguousarray(c["aos"][np.sort(c["order"][sel])])        # upload order kept: the same draw order
    r = SplatRenderer(device=0, **one_pass)
    assert r.Init(part, False, False), r.last_error()
    r.Sort(c["cam"], c["proj"], vp, c["nf"])
    assert r.sort_count() == sel.sum()
    img = r.Render(c["cam"], c["proj"], vp, c["nf"])
    r.close()
    assert (img[..., 3] == 1.0).all()
    ref = orc.render_frame(part, True, c["cam"], c["proj"], vp, c["nf"], want_image=False, want_splats=True)
    _, budget = orc.composite_flip(ref["splats"], c["W"], c["H"])
    d = np.abs(img[..., :3].astype(np.float64) - g[name + "_rgb_g"])
    print("HIP vs reference shaders (ladder %s, %d G splats below %g px^2): max |diff| %.3g, mean %.3g, within 1e-4: %.5f" % (
        name, sel.sum(), float(g["image_l"]), d.max(), d.mean(), (d <= 1e-4).mean()))
    assert d.mean() <= 1e-4 and (d <= 1e-4).mean() >= 0.999
    assert (d.max(axis=-1) <= 5e-3 + budget).all(), "max |diff| %.3g beyond the threshold-flip budget" % d.max()


def test_baseline_config2_matches_the_reference_shaders():
    """BASELINE configs[1] (1 M splats, SH3, 1920x1080) on the MI355X against what the reference's shaders computed for the same
    frame on llvmpipe (glref_cfg2_1m_1080p.npz): visible count, keys, indices and draw order by digest; a 512 x 256 window of the
    image within SURVEY 8c; 8x8 box means of the WHOLE frame"""
    c = glref_cases.config2()
    g = np.load(os.path.join(glref_cases.GOLDEN, "glref_cfg2_1m_1080p.npz"))
    assert str(g["digest"]) == glref_cases.digest(c["aos"])
    vp = [0, 0, c["W"], c["H"]]
    from splatapult_amd import _capi
    # (upload order kept: the fixture's frame was drawn with equal keys in ascending upload index, and a cloud of this size would
    #  otherwise be stored in the library's spatial order, whose tie rule is the storage slot -- include/msplat.h; that path is
    #  checked against the oracle fed the same order in test_gpu_parity.py)
    r = SplatRenderer(device=0, spatial_order=_capi.SPATIAL_OFF)
    assert r.Init(c["aos"], False, False), r.last_error()
    r.Sort(c["cam"], c["proj"], vp, c["nf"])
    assert r.sort_count() == int(g["V"])
    si, sk = r.sorted_indices(), r.sorted_keys()
    order = np.argsort(si, kind="stable")
    assert glref_cases.u32_digest(si[order]) == str(g["idx_digest"])          # the visible set of presort_compute.glsl
    assert glref_cases.u32_digest(sk[order]) == str(g["keys_digest"])         # ... and its keys
    assert glref_cases.u32_digest(si) == str(g["order_digest"])               # the draw order: ascending key, ties by index
    img = r.Render(c["cam"], c["proj"], vp, c["nf"])
    assert (img[..., 3] == 1.0).all()
    y0, y1, x0, x1 = glref_cases.CFG2_WINDOW
    d = np.abs(img[y0:y1, x0:x1, :3].astype(np.float64) - g["window"])
    dm = np.abs(glref_cases.box_mean8(img[..., :3]).astype(np.float64) - g["mean8"])
    print("HIP vs reference shaders (config 2, 1 M splats, 1080p): window max |diff| %.3g, mean %.3g, within 1e-4: %.5f; 8x8 means max %.3g" % (
        d.max(), d.mean(), (d <= 1e-4).mean(), dm.max()))
    assert d.mean() <= 1e-4 and (d <= 1e-4).mean() >= 0.999 and d.max() <= 5e-3
    assert dm.max() <= 1e-3 and dm.mean() <= 1e-5


@pytest.mark.parametrize("name", sorted(glref_cases.point_cases()))
def test_point_renderer_matches_the_reference_point_shaders(name):
    """PointRenderer on the MI355X against shader/point_{vert,geom,frag}.glsl as llvmpipe executed them with the GL
    texture of core/texture.cpp (glref_points.npz).  Draw order exact; magnified sprites (GL_LINEAR, no level of detail) to float
    rounding; minified ones within glref_cases.POINT_MINIFIED_TOL (llvmpipe's level of detail is 0.045 below the specification's and
    its mip levels round differently: tests/test_reference_shaders.py measures both); pixels whose centre is within 1/400 pixel of a
    quad edge are decided by GL's sub-pixel vertex snapping and are only counted"""
    from splatapult_amd import PointRenderer
    c = glref_cases.point_cases()[name]
    g = np.load(os.path.join(glref_cases.GOLDEN, "glref_points.npz"))
    assert str(g[name + "_digest"]) == glref_cases.digest(c["points"]) + glref_cases.digest(c["sprite"].astype(np.float32))
    vp = [0, 0, c["W"], c["H"]]
    r = PointRenderer(device=0)
    assert r.Init(c["points"], c["srgb"], sprite=c["sprite"]), r.last_error()
    if c["depth_bits"]:
        r.set_depth_test(c["depth_bits"])
    img = r.Render(c["cam"], c["proj"], vp, c["nf"])
    np.testing.assert_array_equal(r.sorted_indices(), g[name + "_order"])
    fr = orc.points_frame(c["points"], c["sprite"], c["cam"], c["proj"], vp, c["nf"], srgb=c["srgb"], depth_bits=c["depth_bits"])
    edge = glref_cases.point_edge_mask(fr["pts"], c["W"], c["H"])
    d = np.abs(img[..., :3] - g[name + "_rgb"]).max(axis=-1)
    lit = g[name + "_rgb"].sum(-1) > 0
    print("HIP point renderer vs reference point shaders (%s): max |diff| %.3g off the quad edges, mean over lit %.3g, %d edge pixels "
          "of which %d differ" % (name, d[~edge].max(), d[lit].mean(), int(edge.sum()), int((d[edge] > 0.03).sum())))
    assert (img[..., 3] == 1.0).all()
    if c["kind"] == "magnified":
        assert d[~edge].max() <= 2e-5
    else:
        assert d[~edge].max() <= glref_cases.POINT_MINIFIED_TOL and d[lit].mean() <= 5e-3
    assert ((img[..., :3].sum(-1) > 0) == lit)[~edge].all()
    assert (d[edge] > 0.03).sum() <= 8
