"""CPU tests of selection by neighbourhood (msplat_neighbour_values), no device: the fixtures of the GPU tests
hold what they claim -- pairs at exactly the radius, partners one ulp farther, lattice points on cell boundaries --; the grid's cell
function (tests/neighbour_rule.py restates near_cell of msplat_neighbours.hip.h) is conservative on all of them: two centres the rule
calls neighbours are at most one cell apart per axis; the names exist in the headers, the library and the bindings, and the refusals
that need no device are made."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from splatapult_amd import SplatRenderer, _capi
from tests import neighbour_rule as nr
from tests.conftest import ROOT

F = np.float32


# ---- 1. the fixtures are what they claim -------------------------------------------------------------------------------------------
def test_designed_pairs_lie_exactly_at_the_radius_and_their_partners_one_ulp_beyond():
    b = nr.boundary_cloud()
    xyz, r2 = b["xyz"], nr.r2_of(nr.BOUNDARY_RADIUS)
    assert r2 == F(25.0 / 256.0) and nr.edge(nr.BOUNDARY_RADIUS) == 5125.0 / 16384.0
    d2 = nr.d2_of("boundary")
    assert len(b["exact"]) == len(b["ulp"]) == 12
    for i, j in b["exact"]:
        assert d2[i, j] == r2 and d2[j, i] == r2, (i, j, d2[i, j])
    for i, j in b["ulp"]:
        assert r2 < d2[i, j] <= r2 * F(1.00001) and d2[j, i] == d2[i, j], (i, j, d2[i, j])      # (one ulp of a coordinate near 4)
    count = nr.result(d2, "count", nr.BOUNDARY_RADIUS)
    near = nr.result(d2, "dist2", nr.BOUNDARY_RADIUS)
    for i, j in b["exact"]:
        assert count[i] == 1 and count[j] == 1 and near[i] == r2, "a pair at exactly the radius is counted, and alone"
    for i, j in b["ulp"]:
        assert count[i] == 0 and count[j] == 0 and np.isposinf(near[i]), "one ulp farther is outside"
    c0, c1 = b["coincident"]
    assert c1 - c0 == nr.COINCIDENT == 257 and (xyz[c0:c1] == xyz[c0]).all()
    assert (count[c0:c1] == 256).all() and (near[c0:c1] == 0).all(), "coincident duplicates are each other's neighbours"
    assert (xyz < 0).any(axis=0).all() and (xyz > 0).any(axis=0).all(), "negative and positive coordinates on every axis"


def test_lattice_points_sit_exactly_on_cell_boundaries():
    b = nr.boundary_cloud()
    xyz = b["xyz"]
    l0, l1 = b["lattice"]
    h = nr.edge(nr.BOUNDARY_RADIUS)
    rel = xyz[l0:l1].astype(np.float64) / h * 2                                   # exact: every quotient is an integer
    assert (rel == np.round(rel)).all() and rel.min() == -(nr.LATTICE // 2) and rel.max() == nr.LATTICE // 2
    assert (rel % 2 == 0).all(axis=1).sum() == 5 ** 3, "the points with every coordinate on a cell boundary"
    # half a cell apart: 26 neighbours inside the radius for an inner point, the points one whole cell away are outside
    count = nr.result(nr.d2_of("boundary"), "count", nr.BOUNDARY_RADIUS)[l0:l1]
    inner = (np.abs(rel) < nr.LATTICE // 2).all(axis=1)
    assert (count[inner] == 26).all() and count.min() == 7
    # the cell function puts a boundary point into the cell it opens or the one below (the product is rounded), never elsewhere,
    # and a point between two boundaries into its cell
    cell = nr.cells(xyz[l0:l1], nr.BOUNDARY_RADIUS)
    k = np.floor(rel / 2).astype(np.int64)
    assert (np.abs(cell - k) <= 1).all() and (cell[rel % 2 != 0] == k[rel % 2 != 0]).all() and cell.min() < 0 < cell.max()


def test_hostile_and_geo_fixtures_hold_their_families():
    hc = nr.hostile_cloud()
    xyz = hc["xyz"]
    fin = nr.finite_rows(xyz)
    assert not fin[list(hc["bad"])].any() and fin.sum() == xyz.shape[0] - 5
    assert fin[list(hc["huge"])].all() and (np.abs(xyz[list(hc["huge"])]).max(axis=1) == F(1e30)).all()
    d2 = nr.d2_of("hostile")
    count, near = nr.result(d2, "count", nr.HOSTILE_RADIUS), nr.result(d2, "dist2", nr.HOSTILE_RADIUS)
    for i in hc["bad"] + hc["huge"]:
        assert count[i] == 0 and np.isposinf(near[i]), i
    everyone = nr.neighbour_matrix(d2, nr.HOSTILE_RADIUS)
    assert not everyone[:, list(hc["bad"] + hc["huge"])].any(), "never counted either"
    o, c = hc["outliers"], hc["clamped"]
    assert count[o[0]] == 1 and count[o[1]] == 1 and near[o[0]] == 0 and count[o[2]] == 0 and count[o[3]] == 0, "the coincident outliers find each other"
    assert count[c[0]] == 1 and count[c[1]] == 1 and near[c[1]] == 0
    cell = nr.cells(xyz[fin], nr.HOSTILE_RADIUS)
    lim = (np.abs(cell) == nr.CELL_MAX).any(axis=1)
    assert lim.sum() == len(hc["huge"]) + len(c), "the clamp path is taken by the centres at 1e30 and 3e20 and by no other"
    assert len(np.unique(cell[~lim], axis=0)) > 250, "the outliers at 1e6 do not make the cells coarse: the unit cube still fills its 7^3 cells"
    assert 1 < count[fin].mean() < 30
    g = nr.geo_cloud()
    assert (np.abs(g) >= 1e5 - 1).all()
    cell = nr.cells(g, nr.GEO_RADIUS)
    assert len(np.unique(cell, axis=0)) > 100 and np.abs(cell).min() > 2 ** 22, "cells stay apart where an fp32 coordinate has no fraction left"
    assert 4 < nr.result(nr.d2_of("geo"), "count", nr.GEO_RADIUS).mean() < 40


# ---- 2. the cell function is conservative ----------------------------------------------------------------------------------------
def assert_conservative(xyz, radius, d2=None, what=""):
    xyz = np.asarray(xyz, F)
    d2 = nr.d2_matrix(xyz) if d2 is None else d2
    W = nr.neighbour_matrix(d2, radius)
    fin = nr.finite_rows(xyz)
    assert not W[~fin].any() and not W[:, ~fin].any()
    cell = nr.cells(np.where(fin[:, None], xyz, 0), radius)
    i, j = np.nonzero(W)
    apart = np.abs(cell[i] - cell[j]).max(axis=1) if i.size else np.zeros(0, np.int64)
    assert (apart <= 1).all(), "%s: %d neighbour pair(s) more than one cell apart, first %d, %d" % (what, (apart > 1).sum(), i[apart > 1][0], j[apart > 1][0])
    return int(i.size), int((apart == 1).sum())


@pytest.mark.parametrize("name", ["boundary", "hostile", "geo"])
def test_neighbours_are_at_most_one_cell_apart_in_the_fixtures(name):
    radius = dict(boundary=nr.BOUNDARY_RADIUS, hostile=nr.HOSTILE_RADIUS, geo=nr.GEO_RADIUS)[name]
    pairs, crossing = assert_conservative(nr.xyz_of(name), radius, nr.d2_of(name), what=name)
    print("%s: %d neighbour pairs, %d of them in adjacent cells" % (name, pairs, crossing))
    assert pairs > 500 and crossing > 100


@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("which", ["none", "some", "all"])
def test_neighbours_are_at_most_one_cell_apart_in_the_random_clouds(n, which):
    assert_conservative(nr.random_cloud(n), nr.random_radii(n)[which], nr.d2_of("random", n), what="random %d %s" % (n, which))
    if which == "all":
        cell = nr.cells(nr.random_cloud(n), nr.random_radii(n)[which])
        assert set(np.unique(cell)) == {-1, 0}, "the largest radius puts every centre into the eight cells around zero: one neighbourhood"


@pytest.mark.parametrize("radius,k_max", [(0.3125, 40), (0.01, 2 ** 24), (1e-3, 2 ** 31), (7.0, 2 ** 20), (3e-5, 2 ** 39), (1e-12, 2 ** 41), (2e18, 4)])
def test_pairs_straddling_a_cell_boundary_by_one_ulp_stay_one_cell_apart(radius, k_max):
    """the adversarial case of the argument in DESIGN.md: a just below a boundary up to k_max cells from zero -- for the last but
    one radius beyond the clamp --, b the rule's farthest neighbour across it"""
    p = nr.straddling_pairs(radius, k_max)
    cell = nr.cells(p, radius)
    a, b = cell[0::2], cell[1::2]
    d2 = np.array([nr.d2_matrix(p[k:k + 2])[0, 1] for k in range(0, p.shape[0], 2)])
    assert (d2 <= nr.r2_of(radius)).all()
    assert (np.abs(a - b) <= 1).all(), np.abs(a - b).max()
    if k_max <= 2 ** 20:        # (farther out the float32 coordinates are coarser than the radius: a and b coincide)
        assert (np.abs(a - b).max(axis=1) == 1).sum() > p.shape[0] // 4, "the pairs do straddle"
    if k_max > nr.CELL_MAX:
        assert (np.abs(cell) == nr.CELL_MAX).any(), "some lie beyond the clamp"


# ---- 3. symbols and refusals -----------------------------------------------------------------------------------------------------
def test_the_headers_declare_the_call_the_library_exports_it_and_the_bindings_have_it():
    header = open(os.path.join(ROOT, "include", "msplat.h")).read()
    debug = open(os.path.join(ROOT, "include", "msplat_debug.h")).read()
    for decl in ("int msplat_neighbour_values(msplat_ctx* ctx, int32_t kind, float radius, const uint8_t* d_source, const uint8_t* d_query, uint64_t n, "
                 "uint32_t cap, uint64_t max_tests, float* d_values, msplat_neighbour_info* info /* may be NULL */);",
                 "enum { MSPLAT_NEAR_COUNT = 0, MSPLAT_NEAR_DIST2 = 1 };", "typedef struct msplat_neighbour_info { uint32_t struct_size;",
                 "} msplat_neighbour_info;"):
        assert decl in header, decl
    for said in ("r2 = radius * radius, rounded once", "j != i in upload numbering", "d2(i, j) <= r2", "((dx dx) + (dy dy)) + (dz dz)",
                 "is never a neighbour and has none", "(float)min(count_i, cap)", "+inf if there is none", "no floating-point atomic",
                 "tests > max_tests fails with MSPLAT_ERR_UNSUPPORTED", "16 408 bytes of rows"):
        assert said in header, said
    assert len(header.splitlines()) <= 300
    assert "int msplat_debug_set_neighbour_buckets(msplat_ctx* ctx, uint32_t buckets);" in debug
    L = C.CDLL(_capi.LIB_PATH)
    protos = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    for name in ("msplat_neighbour_values", "msplat_debug_set_neighbour_buckets"):
        assert hasattr(L, name), "libmsplat.so does not export %s" % name
        assert name in protos, "no ctypes prototype for %s" % name
    assert protos["msplat_neighbour_values"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64,
                                                           C.c_void_p, C.POINTER(_capi.NeighbourInfo)])
    assert protos["msplat_debug_set_neighbour_buckets"] == (C.c_int, [C.c_void_p, C.c_uint32])
    assert _capi.NEAR_KINDS == {"count": 0, "dist2": 1} and tuple(sorted(_capi.NEAR_KINDS, key=_capi.NEAR_KINDS.get)) == nr.KINDS
    # the struct as the compiler lays it out (the shim test asserts the same numbers in C++)
    assert C.sizeof(_capi.NeighbourInfo) == 32 and _capi.NeighbourInfo.sources.offset == 4 and _capi.NeighbourInfo.tests.offset == 24
    sig = inspect.signature(SplatRenderer.NeighbourValues)
    assert list(sig.parameters) == ["self", "radius", "kind", "source", "query", "cap", "max_tests", "out", "info"]
    assert [sig.parameters[k].default for k in ("kind", "source", "query", "cap", "max_tests", "out", "info")] == ["count", None, None, 0, None, None, False]
    grow = inspect.signature(SplatRenderer.GrowSelection)
    assert list(grow.parameters)[:4] == ["self", "mask", "radius", "steps"] and grow.parameters["steps"].default == 1


def test_refusals_that_need_no_device():
    L = _capi.lib()
    err = lambda: L.msplat_last_error(None).decode()
    ni = _capi.NeighbourInfo(struct_size=C.sizeof(_capi.NeighbourInfo))
    assert L.msplat_neighbour_values(None, 0, 0.1, None, None, 0, 0, 1, None, C.byref(ni)) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    assert L.msplat_debug_set_neighbour_buckets(None, 64) == _capi.ERR_INVALID_ARG and "ctx is NULL" in err()
    # the Python layer refuses what cannot be right before it asks for a device: the renderer below has no context
    r = SplatRenderer()
    for call in (lambda: SplatRenderer.NeighbourValues(r, 0.1, "nearest"), lambda: SplatRenderer.NeighbourValues(r, 0.1, 2),
                 lambda: SplatRenderer.NeighbourValues(r, 0.1, "dist2", cap=1), lambda: SplatRenderer.NeighbourValues(r, 0.1, 1, cap=3),
                 lambda: SplatRenderer.NeighbourValues(r, 0.0), lambda: SplatRenderer.NeighbourValues(r, -1.0),
                 lambda: SplatRenderer.NeighbourValues(r, np.nan), lambda: SplatRenderer.NeighbourValues(r, np.inf),
                 lambda: SplatRenderer.NeighbourValues(r, 0.1, cap=-1), lambda: SplatRenderer.NeighbourValues(r, 0.1, max_tests=-1),
                 lambda: SplatRenderer.GrowSelection(r, None, 0.1), lambda: SplatRenderer.GrowSelection(r, np.zeros(4, np.uint8), 0.1, steps=-1)):
        with pytest.raises(ValueError):
            call()


def test_the_rule_handles_sets_caps_and_unselected_words():
    n = 65
    d2, m = nr.d2_of("random", n), nr.set_masks(n)
    radius = nr.random_radii(n)["some"]
    full = nr.result(d2, "count", radius)
    assert (nr.result(d2, "count", radius, m["full"]) == full).all() and not nr.result(d2, "count", radius, m["empty"]).any()
    part = nr.result(d2, "count", radius, m["random_source"])
    assert (part <= full).all() and (part < full).any() and (nr.result(d2, "count", radius, cap=2) == np.minimum(full, 2)).all()
    v = nr.values(d2, "dist2", radius, query=m["random_query"])
    assert (v[m["random_query"] == 0] == nr.SENTINEL).all() and (v[m["random_query"] != 0] != nr.SENTINEL).all()
    assert np.isposinf(nr.result(d2, "dist2", radius, m["empty"])).all()
    # the dilation grows, and three steps reach at least as far as one
    seed = np.zeros(n, np.uint8)
    seed[3] = 200
    one, three = nr.grow(d2, seed, radius), nr.grow(d2, seed, radius, 3)
    assert one[3] == 200 and set(np.unique(one)) <= {0, 1, 200} and ((one != 0) <= (three != 0)).all() and (three != 0).sum() > (one != 0).sum() > 1
    assert nr.info(nr.random_cloud(n), d2, radius)["pairs"] == int(full.sum())


def test_the_shim_with_the_neighbour_method_compiles_with_gxx(tmp_path):
    src = tmp_path / "neighbours_shim.cpp"
    src.write_text("""
#include <cstddef>
#include "splatapult_amd/host/msplat_host.hpp"
#include "include/msplat_debug.h"
static_assert(sizeof(msplat_neighbour_info) == 32 && offsetof(msplat_neighbour_info, sources) == 4 && offsetof(msplat_neighbour_info, tests) == 24,
              "the layout the ctypes binding assumes");
static_assert(MSPLAT_NEAR_COUNT == 0 && MSPLAT_NEAR_DIST2 == 1, "the kinds");
int main()
{
    SplatRenderer r;
    msplat_neighbour_info info;
    // no context yet: the call on the renderer is refused, none crashes
    bool ok = !r.NeighbourValues(MSPLAT_NEAR_COUNT, 0.1f, nullptr, nullptr, 0, 0, 1, nullptr, &info) && info.struct_size == sizeof(msplat_neighbour_info);
    ok = ok && msplat_neighbour_values(nullptr, MSPLAT_NEAR_DIST2, 0.1f, nullptr, nullptr, 0, 0, 1, nullptr, nullptr) == MSPLAT_ERR_INVALID_ARG;
    ok = ok && msplat_debug_set_neighbour_buckets(nullptr, 1) == MSPLAT_ERR_INVALID_ARG;
    return ok ? 0 : 1;
}
""")
    exe, libdir = str(tmp_path / "neighbours_shim"), os.path.dirname(_capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-L", libdir, "-lmsplat", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, cwd=ROOT)
    assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 0
