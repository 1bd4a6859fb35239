"""Named inputs for the depth sort at its limits (inputs only, like scenes.py; tests/test_sort_limits_fixtures.py checks every
claim made here on the CPU, tests/test_gpu_sort_limits.py sorts the cases on the GPU).

Keys are DESIGNED, not drawn.  The camera is camera.pose((0, 0, 0)), the identity, and the projection
camera.perspective(fovy, aspect, 0.1, zf) with zf = 2^k: row 3 of the MVP is then exactly (0, 0, -1, 0), so depth = -z for any x
and y, q = trunc(depth / zf * 2^32) = depth * 2^(32 - k) and key = 0xFFFFFFFF - q.  A splat at z = -(q / 2^(32 - k)) gets exactly
the quantised depth q for every q with at most 24 significant bits; depth >= zf saturates (q = 0xFFFFFFFF, key 0); q = 0 (z = -0.0)
is culled, because the cull needs depth > 0.  x and y stay inside the 1.5 clip band: |x|, |y| <= 0.3 depth.

A case is a Case: the attributes of an SH0 cloud (scenes.cloud_from_attrs(a, full_sh=False)), the view (cam, proj, vp, nf), the
designed q per splat (0 = culled) and what it claims:
  V       visible splats
  B       bit length of the largest visible q (what ws_digit_range cuts the digits from)
  digits  {pass: (lo, hi)}: every chunk of C keys has lo .. hi non-empty digits in that pass of the three-pass sort
  order   "identity" / "reversed" / "evens_then_odds": the sorted permutation of the visible splats, or None
C is the chunk of the form under test: 4096 keys (one frame at a time), 2048 (frames in flight, the 8-bit passes)."""
import collections
import functools
import math

import numpy as np

from splatapult_amd import camera
from tests import scenes

W, H = 256, 192
K = 10                                  # zf = 2^10 where the case does not choose its own
SAT = 0xFFFFFFFF                        # q of a splat at depth >= zf
SPATIAL_MIN = 262144                    # from this size on a cloud is stored in Morton order unless spatial_order = SPATIAL_OFF
NARROW_FOVY = math.radians(10.0)        # a second view of the same keys: the splats with |x| = 0.3 depth leave its clip band
FOCAL = 0.5 * H / math.tan(0.5 * camera.FOVY)      # pixels per unit of x / depth

Case = collections.namedtuple("Case", "name attrs view q claims C")


def view(k=K, fovy=camera.FOVY, yaw=0.0):
    zf = float(2 ** k)
    return camera.pose((0.0, 0.0, 0.0), yaw), camera.perspective(fovy, W / H, 0.1, zf), [0, 0, W, H], [0.1, zf]


def cloud_of(case):
    return scenes.cloud_from_attrs(case.attrs, full_sh=case.attrs["f_rest"] is not None)


def q_of(depth, k):
    """the designed quantised depth of splats at z = -depth under zf = 2^k (uint64; 0 = culled, SAT = saturated)"""
    qf = np.asarray(depth, np.float64) * 2.0 ** (32 - k)
    assert (qf == np.floor(qf)).all() and (qf >= 0).all(), "the design leaves nothing to the truncation"
    return np.where(qf >= 2.0 ** 32, float(SAT), qf).astype(np.uint64)


def attrs_at(depth, seed, wide=None, px_sigma=1.0, opacity=(0.5, 2.0)):
    """attributes of a cloud with splat i at z = -depth[i] (float64, exact in float32; 0 = culled) and |x|, |y| <= 0.3 depth.
    wide (bool per splat): those splats sit at |x| = 0.3 depth and the others inside |x|, |y| <= 0.04 depth, so that the view
    with NARROW_FOVY culls exactly the wide ones.  Sizes follow the depth: about px_sigma pixels on screen"""
    depth = np.asarray(depth, np.float64)
    n = depth.shape[0]
    assert (depth.astype(np.float32).astype(np.float64) == depth).all()
    rng = np.random.default_rng(seed)
    u = rng.uniform(-0.3, 0.3, (n, 2))
    if wide is not None:
        u = rng.uniform(-0.04, 0.04, (n, 2))
        u[wide, 0] = np.where(rng.random(int(wide.sum())) < 0.5, -0.3, 0.3)
    xyz = np.empty((n, 3), np.float32)
    xyz[:, 0] = u[:, 0] * depth
    xyz[:, 1] = u[:, 1] * depth
    xyz[:, 2] = -depth
    size = np.log(np.maximum(depth, 2.0 ** -20) * (px_sigma / FOCAL))
    log_scale = (size[:, None] + rng.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)
    rot = rng.standard_normal((n, 4)).astype(np.float32)
    rot /= np.maximum(np.linalg.norm(rot, axis=1, keepdims=True), 1e-6)
    return dict(xyz=xyz, f_dc=(0.8 * rng.standard_normal((n, 3))).astype(np.float32), f_rest=None,
                opacity=(opacity[0] + opacity[1] * rng.standard_normal(n)).astype(np.float32), log_scale=log_scale, rot=rot)


def make(name, q, C, seed, k=K, digits=None, order=None, wide=None, depth=None, **kw):
    """a case from its designed q under zf = 2^k (or from the depths, for splats beyond the far plane)"""
    if depth is None:
        q = np.asarray(q, np.uint64)
        depth = q.astype(np.float64) / 2.0 ** (32 - k)
    q = q_of(depth, k)
    vis = q[q > 0]
    claims = dict(V=int(vis.size), B=int(vis.max()).bit_length() if vis.size else 0, digits=digits, order=order)
    return Case(name, attrs_at(depth, seed, wide=wide, **kw), view(k), q, claims, C)


def mantissas(rng, n, shift):
    """n random 24-bit mantissas, the exact maximum and a small minimum among them, shifted left"""
    m = rng.integers(1, 1 << 24, n, dtype=np.uint64)
    m[rng.integers(0, n)] = (1 << 24) - 1
    if n > 1:
        m[(int(np.argmax(m)) + 1) % n] = 3
    return m << np.uint64(shift)


# digit cuts of the three passes: bits [0, 10) | [10, 18) | [18, 26) while B <= 26 (here B <= 24), [0, 10) | [10, 21) | [21, 32) at B = 32
CUTS = {24: ((0, 10), (10, 18), (18, 24)), 32: ((8, 10), (10, 21), (21, 32))}      # (the bits a 24-bit mantissa << 0 / << 8 has there)
CONST = {24: 0x9A6A55, 32: 0x9A6A5500}                                                # bit 23 / bit 31 set: B holds in every case


def one_digit(C, p, B, two, seed):
    """q random inside pass p's digit and constant elsewhere (two: two values alternating by upload index, the larger q first)"""
    lo, hi = CUTS[B][p]
    mask = ((1 << hi) - 1) ^ ((1 << lo) - 1)
    rng = np.random.default_rng(seed)
    n = 4 * C if two else 4 * C + 33
    if two:
        d = np.where(np.arange(n) % 2 == 0, mask, mask & (mask >> 1) & ~(1 << lo))       # even: every bit of the digit; odd: fewer
    else:
        d = (rng.integers(0, 1 << (hi - lo), n, dtype=np.uint64) << np.uint64(lo)).astype(np.uint64)
        d[:2] = (mask, 0)
    q = (np.uint64(CONST[B] & ~mask) | np.asarray(d, np.uint64)).astype(np.uint64)
    q[q == 0] = np.uint64(1 << lo)
    nb = 1 << (hi - lo)
    digits = {r: ((2, 2) if two else (2, nb)) if r == p else (1, 1) for r in range(3)}
    name = "%s_p%d_B%d" % ("two_keys" if two else "one_digit", p, B)
    return make(name, q, C, seed, digits=digits, order="evens_then_odds" if two else None)


EDGE_V = ("C-1", "C", "C+1", "2C", "16C", "16C+1", "17C")
EDGE_PLACES = ("front", "alternate", "middle")


def edge_mask(C, V, place, delta):
    """which splats of the cloud are visible: V of them, the culled ones placed as `place` says, N = k C + delta"""
    need = {"front": V + 2 * C + 3, "alternate": 2 * V, "middle": V + 3 * C, "first": 3 * C, "last": 3 * C}[place]
    N = -(-need // C) * C + delta
    if N < need:
        N += C
    vis = np.zeros(N, bool)
    if place == "front":                   # every culled splat in front of the first visible one: pass 0's first chunks are empty
        vis[N - V:] = True
    elif place == "alternate":             # every other splat
        vis[0:2 * V:2] = True
    elif place == "middle":                # two whole chunks of culled splats in the middle of the visible ones
        a = V // 2
        a0 = -(-a // C) * C
        vis[:a] = True
        vis[a0 + 2 * C:a0 + 2 * C + V - a] = True
    elif place == "first":
        vis[0] = True
    else:
        vis[N - 1] = True
    assert vis.sum() == V
    return vis


def edge_combos():
    """(V, place, delta) of the edge cases: every V meets every placement, every placement every N = k C + delta"""
    combos = [(v, p, (-1, 0, 1)[(vi + pi) % 3]) for vi, v in enumerate(EDGE_V) for pi, p in enumerate(EDGE_PLACES)]
    return combos + [("1", p, d) for p in ("first", "last") for d in (-1, 0, 1)]


def edge_case(C, i):
    v, place, delta = edge_combos()[i]
    V = {"1": 1, "C-1": C - 1, "C": C, "C+1": C + 1, "2C": 2 * C, "16C": 16 * C, "16C+1": 16 * C + 1, "17C": 17 * C}[v]
    vis = edge_mask(C, V, place, delta)
    q = mantissas(np.random.default_rng(7000 + i), vis.size, 8 * (i % 2))          # B = 24 and B = 32 in turn
    q[~vis] = 0
    return make("edge_V%s_%s_N%+d" % (v, place, delta), q, C, 7100 + i)


WIDTH_E = 14                              # the width cloud: depth = m / 2^14 with 24-bit m, so q = m 2^(18 - k) under zf = 2^k
SATURATED_K = 8                           # zf = 256: m >= 2^22 saturates


@functools.lru_cache(maxsize=None)
def width_depths(C):
    """one cloud for every digit width: random 24-bit mantissas m with the exact maximum 2^24 - 1, a small minimum, 2^22 - 1 (the
    largest that stays below zf = 256), and a hundred splats at exactly 256 and 768 = zf and 3 zf of the saturated view"""
    rng = np.random.default_rng(4242)
    m = mantissas(rng, 3 * C + 77, 0)
    at = rng.permutation(m.size)[:103]
    m[at[:50]] = 1 << 22
    m[at[50:100]] = 3 << 22
    m[at[100:]] = ((1 << 22) - 1, (1 << 24) - 1, 3)
    d = m.astype(np.float64) / 2.0 ** WIDTH_E
    d.setflags(write=False)
    return d


def width_k(B):
    """the zf = 2^k under which the width cloud's largest q has B bits: halving zf raises B by one"""
    return 32 + 24 - WIDTH_E - B


def width_case(C, B):
    """B = 24 .. 32, or "saturated" """
    k = SATURATED_K if B == "saturated" else width_k(B)
    return make("saturated" if B == "saturated" else "width_%d" % B, None, C, 4243, k=k, depth=width_depths(C))


def away_view():
    """the camera turned round: nothing of any of these clouds is visible"""
    return view(K, yaw=math.pi)


ONE_DIGIT = {1: (1, 1), 0: (1, 1), 2: (1, 1)}


def small_builders():
    """name -> builder(C) of every case below a million splats"""
    b = collections.OrderedDict()
    b["one_key"] = lambda C: make("one_key", np.full(3 * C + 1, 0x00ABCD00, np.uint64), C, 1, digits=ONE_DIGIT, order="identity")
    for B in (24, 32):
        for p in range(3):
            b["one_digit_p%d_B%d" % (p, B)] = lambda C, p=p, B=B: one_digit(C, p, B, False, 100 + 10 * p + B)
            b["two_keys_p%d_B%d" % (p, B)] = lambda C, p=p, B=B: one_digit(C, p, B, True, 200 + 10 * p + B)
    b["ascending"] = lambda C: make("ascending", ((np.arange(5 * C, dtype=np.uint64) + 1) * 401) << 8, C, 2, order="reversed")
    b["descending"] = lambda C: make("descending", (5 * C - np.arange(5 * C, dtype=np.uint64)) * 401, C, 3, order="identity")
    for B in list(range(24, 33)) + ["saturated"]:
        b["saturated" if B == "saturated" else "width_%d" % B] = lambda C, B=B: width_case(C, B)
    for i, (v, place, delta) in enumerate(edge_combos()):
        b["edge_V%s_%s_N%+d" % (v, place, delta)] = lambda C, i=i: edge_case(C, i)
    for j, mult in enumerate(((16, 0), (16, 1), (32, 1))):
        b["groups_random_%d" % j] = lambda C, j=j, mult=mult: make("groups_random_%d" % j, mantissas(np.random.default_rng(300 + j),
                                                                     mult[0] * C + mult[1], 8), C, 310 + j)
        b["groups_one_key_%d" % j] = lambda C, j=j, mult=mult: make("groups_one_key_%d" % j, np.full(mult[0] * C + mult[1], 0xC0000000, np.uint64),
                                                                      C, 320 + j, digits=ONE_DIGIT, order="identity")
    return b


SMALL_NAMES = tuple(small_builders())


@functools.lru_cache(maxsize=8)
def small_case(C, name):
    case = small_builders()[name](C)
    assert case.name == name
    return case


# the three cases above a million splats: name -> (N, chunk of pass 0 in the form they are meant for)
LARGE = {"table_switch_512_rows": (1048576, 2048), "table_switch_513_rows": (1048577, 2048),
         "items_switch_4096_descending": (2097152, 4096), "items_switch_4096_one_key": (2097152, 4096),
         "items_switch_8192_descending": (2097153, 8192), "items_switch_8192_one_key": (2097153, 8192)}


@functools.lru_cache(maxsize=1)
def large_case(name):
    """table_switch: 512 and 513 rows of 2048 keys with frames in flight (groups of 16 rows, then of 32); items_switch: the last
    cloud with 4096-key chunks and the first with 8192.  40 % of an items_switch cloud sit at |x| = 0.3 depth: the NARROW_FOVY
    view sees the other 60 %, fewer than 2 M / 1.25 splats, with the same keys"""
    n, C = LARGE[name]
    rng = np.random.default_rng(n)
    if name.startswith("table_switch"):
        return make(name, mantissas(rng, n, 8), C, n)
    wide = rng.random(n) < 0.4
    if name.endswith("one_key"):
        return make(name, np.full(n, 0xFFFFFF00, np.uint64), C, n, order="identity", wide=wide, px_sigma=0.25)
    return make(name, (np.uint64(n) - np.arange(n, dtype=np.uint64)) << np.uint64(10), C, n, order="identity", wide=wide, px_sigma=0.25)


def narrow(case):
    """(view, q) of the case's second view: the same keys, the wide splats culled"""
    q = case.q.copy()
    q[np.abs(case.attrs["xyz"][:, 0].astype(np.float64)) > 0.1 * -case.attrs["xyz"][:, 2].astype(np.float64)] = 0
    k = int(round(math.log2(case.view[3][1])))
    return view(k, fovy=NARROW_FOVY), q


PLANE_N = 20000


@functools.lru_cache(maxsize=1)
def plane_case():
    """the all-equal plane that is rendered: 20 000 translucent splats of about 2 px at depth 4, every key equal, so the draw
    order is the tie rule alone"""
    return make("plane", np.full(PLANE_N, 1 << 24, np.uint64), 4096, 55, digits=ONE_DIGIT, order="identity",
                px_sigma=2.0, opacity=(0.0, 1.5))


GRID_CAP_N = 40 * 4096 + 77


@functools.lru_cache(maxsize=None)
def grid_cap_case(kind):
    """the clouds of the MSPLAT_GRID_CAP tests: 40 chunks of 4096 keys and a ragged one (80 of 2048) -- "random", "one_key" (both
    with a NARROW_FOVY view that culls 40 %) and "hard" (scenes.hard_attrs, which has no designed keys: q is None)"""
    n = GRID_CAP_N
    if kind == "hard":
        return Case("grid_cap_hard", scenes.hard_attrs(n, 77), scenes.default_view(W, H), None, None, 4096)
    rng = np.random.default_rng(900)
    wide = rng.random(n) < 0.4
    if kind == "one_key":
        return make("grid_cap_one_key", np.full(n, 1 << 24, np.uint64), 4096, 901, order="identity", wide=wide, px_sigma=0.7)
    return make("grid_cap_random", mantissas(rng, n, 8), 4096, 902, wide=wide, px_sigma=0.7)
