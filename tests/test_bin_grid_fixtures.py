"""CPU check of the inputs of tests/test_gpu_bin_grid_limits.py: the strips of scenes.strip_view / scenes.strip_attrs really
reach the 8-bit limit of the bin grid.  Oracle only -- if a seed or a helper changes so that the GPU tests stop reaching bin
index 255, this fails without a GPU.

A splat's bin rectangle is taken from the oracle's projection exactly as _check_projection (tests/gpu_harness.py) bounds the
library's from below: the pixels with w > 1/256 lie within rho sqrt(cov) of the centre, clipped to the viewport, divided by
the 32-px bin."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.checks import TIGHT, check_image
from tests.render_cases import BIN, STRIPS, oracle_rects, strip_case

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
