"""CPU check of the inputs of tests/test_gpu_bin_grid_limits.py: the strips of scenes.strip_view / scenes.strip_attrs really
reach the 8-bit limit of the bin grid.  Oracle only -- if a seed or a helper changes so that the GPU tests stop reaching bin
index 255, this fails without a GPU.

A splat's bin rectangle is taken from the oracle's projection exactly as _check_projection (tests/test_gpu_parity.py) bounds the
library's from below: the pixels with w > 1/256 lie within rho sqrt(cov) of the centre, clipped to the viewport, divided by
the 32-px bin."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import scenes
from tests.test_gpu_parity import TIGHT, check_image

BIN = 32      # msplat_tile_size(): the bin edge in pixels (asserted against the library by the GPU module)

# name -> (W, H, yaw, n, seed, hard): the five inputs of the GPU module's strip tests
STRIPS = {
    "wide_synth": (8192, 64, 0.0, 40000, 5, False),
    "tall_synth": (64, 8192, 0.0, 40000, 6, False),
    "wide_hard": (8192, 64, 0.1, 20000, 7, True),
    "tall_hard": (64, 8192, 0.0, 20000, 8, True),
    "ragged_hard": (8191, 33, 0.0, 20000, 9, True),
}


@functools.lru_cache(maxsize=None)
def strip_cloud(name):
    W, H, yaw, n, seed, hard = STRIPS[name]
    return scenes.cloud_from_attrs(scenes.strip_attrs(n, seed, W, H, hard))


def strip_case(name):
    """(cloud, W, H, view) of a named strip"""
    W, H, yaw = STRIPS[name][:3]
    return strip_cloud(name), W, H, scenes.strip_view(W, H, yaw)


def oracle_rects(sp, W, H):
    """(drawn, tx0, ty0, tx1, ty1) per sorted splat from the oracle's projection: drawn = some pixel centre of the viewport lies
    inside the w > 1/256 footprint's bounding box"""
    alpha = sp["alpha"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho2 = 2.0 * np.log(256.0 * alpha)
    vis = (sp["reject"] == 0) & (rho2 > 0)
    ex = np.sqrt(np.maximum(rho2, 0) * sp["cov"][:, 0])
    ey = np.sqrt(np.maximum(rho2, 0) * sp["cov"][:, 3])
    x0 = np.ceil(sp["px"] - ex - 0.5); x1 = np.floor(sp["px"] + ex - 0.5)
    y0 = np.ceil(sp["py"] - ey - 0.5); y1 = np.floor(sp["py"] + ey - 0.5)
    drawn = vis & (x1 >= 0) & (y1 >= 0) & (x0 <= W - 1) & (y0 <= H - 1) & (x0 <= x1) & (y0 <= y1)
    c = lambda v, hi: (np.clip(np.nan_to_num(v), 0, hi - 1) // BIN).astype(np.int64)
    return drawn, c(x0, W), c(y0, H), c(x1, W), c(y1, H)


@pytest.mark.parametrize("name", sorted(STRIPS))
def test_the_strips_reach_bin_255_and_the_tiled_renderer_meets_the_caps(name):
    cloud, W, H, (cam, proj, vp, nf) = strip_case(name)
    aos = cloud.as_array()
    ref = orc.render_frame(aos, True, cam, proj, vp, nf, nthreads=8, want_image=False, want_splats=True)
    drawn, tx0, ty0, tx1, ty1 = oracle_rects(ref["splats"], W, H)
    lo, hi = (tx0, tx1) if W > H else (ty0, ty1)
    assert (max(W, H) + BIN - 1) // BIN == 256
    reached = np.zeros(257, np.int64)                   # difference array over the long axis
    np.add.at(reached, lo[drawn], 1)
    np.add.at(reached, hi[drawn] + 1, -1)
    reached = np.cumsum(reached)[:256]
    span = int((hi - lo + 1)[drawn].max())
    pairs = int(((tx1 - tx0 + 1) * (ty1 - ty0 + 1))[drawn].sum())
    ties = ref["V"] - np.unique(ref["sorted_keys"]).size
    print("%s: V %d, pairs >= %d, bins reached %d, widest span %d, splats on bin 255: %d, starting there: %d, equal keys %d"
          % (name, ref["V"], pairs, (reached > 0).sum(), span, reached[255], (drawn & (lo == 255)).sum(), ties))
    assert (reached > 0).all(), "bins without a splat: %s" % np.flatnonzero(reached == 0)[:16]
    assert reached[255] > 0
    assert (drawn & (lo == 255)).any()                  # a rectangle that STARTS in bin 255 (tx0 = 255 is also kRectEmpty's)
    assert ties > 0
    if STRIPS[name][5]:
        assert span == 256
    # an implementation with early termination, front to back and tiled, meets check_image's caps on this input
    image, budget = orc.composite_flip(ref["splats"], W, H, nthreads=8)
    tiled = orc.render_frame_tiled(aos, True, cam, proj, vp, nf, nthreads=8)
    assert tiled["V"] == ref["V"]
    d = np.abs(tiled["image"].astype(np.float64) - image)[..., :3]
    print("%s: tiled front-to-back vs back-to-front oracle: within 1e-4 %.5f, mean %.3g, max %.3g" % (name, (d <= 1e-4).mean(), d.mean(), d.max()))
    check_image(tiled["image"], image, budget=budget)
    assert d.max() <= TIGHT                            # ... without needing the flip budget
