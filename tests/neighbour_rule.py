"""The rule of msplat_neighbour_values (include/msplat.h) restated in numpy float32 as brute force over all
pairs, the grid's cell function restated likewise (msplat_neighbours.hip.h: near_cell), and the fixtures the CPU and GPU tests share.
No device, no library.  Every array a builder returns is read-only and computed once."""
import functools

import numpy as np

F = np.float32
KINDS = ("count", "dist2")
SIZES = (1, 2, 63, 64, 65, 4096, 4097)
EDGE = np.float64(1.0009765625)     # kNearEdge = 1 + 2^-10: cell edge h = radius * EDGE, in double
CELL_MAX = 2 ** 40                  # kNearCellMax: cell coordinates are clamped to [-CELL_MAX, CELL_MAX]
SENTINEL = F(-12345.5)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------

def r2_of(radius):
    return F(radius) * F(radius)


def d2_matrix(xyz):
    """d2[i, j] = ((dx dx) + (dy dy)) + (dz dz), dx = x_i - x_j, every operation rounded to float32; NaN / +inf where the
    arithmetic gives them"""
    p = np.asarray(xyz, F)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [p[:, None, k] - p[None, :, k] for k in range(3)]
        out = d[0] * d[0]
        out += d[1] * d[1]          # (a + b, rounded, then + c, rounded: in-place float32 additions are exactly that)
        out += d[2] * d[2]
    assert out.dtype == F
    return out


def neighbour_matrix(d2, radius, source=None):
    """W[i, j]: splat j is a neighbour of splat i"""
    with np.errstate(invalid="ignore"):
        W = d2 <= r2_of(radius)                     # (false for a NaN)
    W[np.arange(W.shape[0]), np.arange(W.shape[0])] = False
    if source is not None:
        W &= (np.asarray(source) != 0)[None, :]
    return W


def result(d2, kind, radius, source=None, cap=0):
    """float32[n]: what the call computes for EVERY splat (values() keeps the words of unselected queries)"""
    W = neighbour_matrix(d2, radius, source)
    if kind == "count":
        c = W.sum(axis=1).astype(np.int64)
        if cap:
            c = np.minimum(c, cap)
        return c.astype(F)
    assert kind == "dist2" and cap == 0
    return np.where(W, d2, F(np.inf)).min(axis=1, initial=F(np.inf)).astype(F)


def values(d2, kind, radius, source=None, query=None, cap=0, base=None):
    n = d2.shape[0]
    out = np.full(n, SENTINEL, F) if base is None else np.array(base, F)
    sel = np.ones(n, bool) if query is None else np.asarray(query) != 0
    out[sel] = result(d2, kind, radius, source, cap)[sel]
    return out


def finite_rows(xyz):
    return np.isfinite(np.asarray(xyz, F)).all(axis=1)


def info(xyz, d2, radius, source=None, query=None):
    """sources, queries as msplat_neighbour_info counts them, and the pairs within the radius: the floor of its `tests`"""
    fin = finite_rows(xyz)
    src = fin if source is None else fin & (np.asarray(source) != 0)
    qry = fin if query is None else fin & (np.asarray(query) != 0)
    pairs = int(neighbour_matrix(d2, radius, source)[qry].sum())
    return dict(sources=int(src.sum()), queries=int(qry.sum()), pairs=pairs)


def grow(d2, mask, radius, steps=1):
    """the dilation GrowSelection computes: per step every splat with a selected neighbour joins with byte 1, other bytes stay"""
    out = np.array(mask, np.uint8)
    for _ in range(steps):
        out[result(d2, "count", radius, out, cap=1) >= 1] = 1
    return out


# ---- the cell function ------------------------------------------------------------------------------------------------------------

def edge(radius):
    """h, exactly as the host forms it: the float32 radius times EDGE, in double"""
    return np.float64(F(radius)) * EDGE


def inv_edge(radius):
    return np.float64(1.0) / edge(radius)


def cells(xyz, radius):
    """int64 (n, 3): floor((double)x * (1 / h)), one rounding, clamped; for finite rows"""
    t = np.floor(np.asarray(xyz, F).astype(np.float64) * inv_edge(radius))
    return np.clip(t, -float(CELL_MAX), float(CELL_MAX)).astype(np.int64)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_cloud(n, seed=5):
    """n centres, uniform in [-1, 1]^3 (negative coordinates included)"""
    return _frozen(np.random.default_rng(seed + n).uniform(-1.0, 1.0, (n, 3)).astype(F))


def random_radii(n):
    """radii giving about 0, about 8 and all n - 1 neighbours in random_cloud(n); the last one puts every centre in ONE cell"""
    some = (8.0 * 8.0 / (max(n, 2) * 4.18879)) ** (1.0 / 3.0)
    return dict(none=F(1e-4), some=F(min(some, 1.5)), all=F(4.0))


BOUNDARY_RADIUS = F(0.3125)                 # 5 / 16: r2 = 25 / 256 and h = 5125 / 16384 are exact
# offsets of length EXACTLY the radius whose squares add exactly: the axes, and 3-4-5 triangles in every plane
_EXACT_OFFSETS = ([(s * 0.3125, 0, 0) for s in (1, -1)] + [(0, s * 0.3125, 0) for s in (1, -1)] + [(0, 0, s * 0.3125) for s in (1, -1)] +
                  [(0.1875, 0.25, 0), (-0.25, 0.1875, 0), (0, 0.1875, -0.25), (0.25, 0, 0.1875), (-0.1875, 0, -0.25), (0, -0.25, -0.1875)])
COINCIDENT = 257                            # more than a wave in one bucket
LATTICE = 9                                 # points per axis around zero, half a cell apart: every second one sits exactly on a cell boundary


@functools.lru_cache(maxsize=None)
def boundary_cloud():
    """dict(xyz, exact, ulp, lattice, coincident): index pairs (i, j) at exactly the radius, their partners one ulp farther, the
    rows of the lattice and of the coincident copies.  Groups are more than two radii apart from each other"""
    pts, exact, ulp = [], [], []
    bases = [(2.0 * i - 3.0, 2.0 * j - 3.0, 2.0 * k + 1.5) for i in range(4) for j in range(3) for k in range(2)]      # 24 bases, clear of the lattice
    for t, off in enumerate(_EXACT_OFFSETS):
        a = np.array(bases[2 * t], np.float64)
        pts += [a, a + np.array(off)]
        exact.append((len(pts) - 2, len(pts) - 1))
        a = np.array(bases[2 * t + 1], np.float64)
        b = (a + np.array(off)).astype(F)
        k = int(np.argmax(np.abs(off)))                     # the longest component, one ulp outwards
        b[k] = np.nextafter(b[k], F(np.inf) if off[k] > 0 else F(-np.inf))
        pts += [a, b.astype(np.float64)]
        ulp.append((len(pts) - 2, len(pts) - 1))
    first_lattice = len(pts)
    g = (np.arange(LATTICE) - LATTICE // 2) * (edge(BOUNDARY_RADIUS) / 2)          # multiples of h / 2 from -2 h to 2 h: exact
    pts += [np.array((x, y, z)) for x in g for y in g for z in g]
    first_copy = len(pts)
    pts += [np.array((3.5, -3.25, 5.0))] * COINCIDENT
    xyz = np.array(pts, np.float64)
    assert (xyz.astype(F).astype(np.float64) == xyz).all(), "every fixture coordinate is a float32 number"
    return dict(xyz=_frozen(xyz.astype(F)), exact=tuple(exact), ulp=tuple(ulp), lattice=(first_lattice, first_copy),
                coincident=(first_copy, first_copy + COINCIDENT))


HOSTILE_RADIUS = F(0.15)
HOSTILE_ORDINARY = 600


@functools.lru_cache(maxsize=None)
def hostile_cloud():
    """dict(xyz, bad, huge, outliers, clamped): ordinary centres in [-0.5, 0.5]^3 with, among them, NaN and infinite centres
    (bad), centres at 1e30 (finite: d2 overflows to +inf; their cell coordinates are clamped), outliers at 1e6 -- two of them
    coincident, one 0.25 beside them, outside the radius -- and two coincident centres at 3e20, a true pair in a clamp cell"""
    xyz = np.array(random_cloud(HOSTILE_ORDINARY, seed=11))
    xyz *= F(0.5)
    extra = np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (np.nan, np.nan, np.nan), (np.inf, -np.inf, 0.25),
                      (1e30, 0, 0), (0, -1e30, 0.5),
                      (1e6, 1e6, -1e6), (1e6, 1e6, -1e6), (-1e6, 0.25, 0), (1e6, 1e6, -999999.75), (0, 2e6, 0),
                      (-3e20, 3e20, 1.0), (-3e20, 3e20, 1.0)], F)
    rows = np.linspace(7, HOSTILE_ORDINARY - 7, extra.shape[0]).astype(int) + np.arange(extra.shape[0])
    for r, e in zip(rows, extra):
        xyz = np.insert(xyz, r, e, axis=0)
    assert all((xyz[r] == e)[~np.isnan(e)].all() for r, e in zip(rows, extra))
    return dict(xyz=_frozen(xyz), bad=tuple(rows[:5]), huge=tuple(rows[5:7]), outliers=tuple(rows[7:12]), clamped=tuple(rows[12:]))


GEO_RADIUS = F(0.0175)
GEO_OFFSET = (1e5, -2e5, 1e5)


@functools.lru_cache(maxsize=None)
def geo_cloud():
    """a geo-referenced cloud: 12^3 centres 0.01 apart (as float32 allows: the ulp at 1e5 is 2^-7) around GEO_OFFSET, jittered:
    5e6 to 1e7 cells from zero, where an fp32 cell coordinate has no fraction left"""
    g = np.arange(12) * 0.01
    p = np.array([(x, y, z) for x in g for y in g for z in g]) + np.random.default_rng(3).uniform(-0.004, 0.004, (1728, 3))
    return _frozen((p + np.array(GEO_OFFSET)).astype(F))


def straddling_pairs(radius, k_max, count=64, seed=9):
    """adversarial pairs for the cell function: a lies just below cell boundary k h of one axis (k up to k_max, both signs), b as
    far beyond it as the rule allows -- the largest float32 step along the axis with d2(a, b) <= r2.  (2 count, 3) float32, pairs in
    consecutive rows"""
    rng = np.random.default_rng(seed)
    h = edge(radius)
    out = []
    for t in range(count):
        k = t % 3
        a = (rng.uniform(-40, 40, 3) * h).astype(F)
        a[k] = np.nextafter(F(np.float64(rng.integers(1, k_max) * (1 if t % 2 else -1)) * h), F(-np.inf))
        b = a.copy()
        b[k] = F(np.float64(a[k]) + np.float64(F(radius)))
        while not (d2_matrix(np.stack([a, b]))[0, 1] <= r2_of(radius)):
            b[k] = np.nextafter(b[k], F(-np.inf))
        out += [a, b]
    return np.array(out, F)


FIXTURES = {"boundary": lambda: boundary_cloud()["xyz"], "hostile": lambda: hostile_cloud()["xyz"], "geo": geo_cloud}


@functools.lru_cache(maxsize=4)
def d2_of(name, n=0):
    """the fixture's d2 matrix, computed once (name "random": random_cloud(n))"""
    d2 = d2_matrix(random_cloud(n) if name == "random" else FIXTURES[name]())
    d2.setflags(write=False)
    return d2


def xyz_of(name, n=0):
    return random_cloud(n) if name == "random" else FIXTURES[name]()


@functools.lru_cache(maxsize=None)
def set_masks(n, seed=17):
    """source and query byte masks: random (nonzero bytes of several values), empty, full"""
    rng = np.random.default_rng(seed + n)
    rand_s = (rng.uniform(size=n) < 0.4) * rng.integers(1, 256, n)
    rand_q = (rng.uniform(size=n) < 0.6) * rng.integers(1, 256, n)
    out = dict(random_source=rand_s.astype(np.uint8), random_query=rand_q.astype(np.uint8), empty=np.zeros(n, np.uint8),
               full=np.full(n, 255, np.uint8))
    return {k: _frozen(v) for k, v in out.items()}
