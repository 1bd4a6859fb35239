"""What the tests of msplat_append_cloud share (numpy only; no device, no library, no torch): the call's numbering restated -- which
source splats a select array picks, the source-to-merged index map as N plus the exclusive prefix sum of the select flags, K, the
merged rows and the extended mask --, the source sizes on the edges of a wave, and the plan by which the GPU test spreads source
sizes, select cases and storage orders over its destination sizes.  Nothing here is measured: the tests compare an appended context
with a context that was uploaded the merged rows."""
import numpy as np

from tests import transform_rule as tr
from tests import visibility_rule as vr

ID_NONE = 0xFFFFFFFF                     # MSPLAT_ID_NONE: the map's entry of a source splat that was not selected
WAVE = 64                                # source slots per turn of append_convert_kernel
# one splat, one short of a wave, a wave, a wave and a splat, 65 waves of which the last holds one splat (and two scan chunks)
SRC_SIZES = (1, WAVE - 1, WAVE, WAVE + 1, 4097)
SRC_SEED = 33                            # the source clouds are not the destination's (visibility_rule's seed 21 / TIE_FREE)


def picked(select, ns):
    """bool per source splat: what a select array (None: every splat; bool, or bytes with nonzero = selected) picks"""
    return np.ones(ns, bool) if select is None else np.asarray(select) != 0


def index_map(select, ns, n):
    """(map, K): map[i] = the merged cloud's upload index of source splat i -- n plus the exclusive prefix sum of the select flags
    -- or ID_NONE; uint32"""
    sel = picked(select, ns)
    assert sel.shape == (ns,), (sel.shape, ns)
    excl = np.cumsum(sel, dtype=np.int64) - sel
    return np.where(sel, n + excl, ID_NONE).astype(np.uint32), int(sel.sum())


def merged_rows(own, src, select):
    """the merged cloud in upload numbering: the destination's rows, then the selected source rows in ascending source index"""
    assert own.shape[1] == src.shape[1], (own.shape, src.shape)
    return np.ascontiguousarray(np.concatenate([own, src[picked(select, src.shape[0])]]))


def merged_mask(mask, k):
    """the mask after the call: the old values, then K visible ones; None stays None"""
    return None if mask is None else np.concatenate([np.asarray(mask) != 0, np.ones(k, bool)])


def select_cases(ns):
    """name -> the selection over a source of ns splats: transform_rule's cases (every splat, visibility_rule's masks -- all-zero
    among them as all_hidden) and the two ends of the numbering"""
    cases = dict(tr.select_cases(ns))
    first, last = np.zeros(ns, bool), np.zeros(ns, bool)
    first[0], last[ns - 1] = True, True
    cases["first_only"], cases["last_only"] = first, last
    return cases


def source_aos(ns, full_sh=True):
    aos = vr.cloud_aos(ns, SRC_SEED)
    return aos if full_sh else np.ascontiguousarray(aos[:, :25])


def plan(d):
    """the appends of destination size number d (0..3, vr.SIZES[d]) for one pair of storage kinds: a list of (ns, select case name,
    destination spatial_order on?, source spatial_order on?).  Every source size takes its select cases in turn, a quarter of them
    per destination size, so that over the four destination sizes every (source size, select case) pair occurs; the 4097-splat
    source meets every combination of the two storage orders, the 4097-splat destination among them"""
    assert 0 <= d < len(vr.SIZES)
    out = []
    for i, ns in enumerate(SRC_SIZES):
        names = sorted(select_cases(ns))
        per = -(-len(names) // len(vr.SIZES))
        for k in range(per):
            slot = (d * per + k + i) % (per * len(vr.SIZES))
            name = names[slot % len(names)]
            if ns == SRC_SIZES[-1]:
                own_on, src_on = bool((k + d) & 1), bool(((k + d) >> 1) & 1)
            else:
                own_on, src_on = bool((i + k) & 1), bool((i + d) & 1)
            out.append((ns, name, own_on, src_on))
    return out
