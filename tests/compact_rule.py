"""What the compaction tests share (numpy only; no device, no torch): msplat_compact_cloud's numbering restated -- the keep flags
of a mask, the old-to-new index map as their exclusive prefix sum, K --, the cloud sizes on the edges of the scan's chunks, and the
mask cases.  Nothing here is measured: the tests compare a compacted context with a context that was uploaded the kept rows."""
import numpy as np

from tests import visibility_rule as vr

CHUNK = 4096                             # kCompactChunk: flags per workgroup of compact_count_kernel / compact_index_kernel
ID_NONE = 0xFFFFFFFF                     # MSPLAT_ID_NONE: a dropped splat's entry of the map
# visibility_rule's sizes (the edges of a cull box) and the edges of the scan's chunks: one flag short of a chunk, one chunk, one
# chunk and a flag, two chunks and a flag (the third chunk holds one splat)
CHUNK_SIZES = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SIZES = tuple(sorted(set(vr.SIZES) | set(CHUNK_SIZES)))


def keep_of(mask):
    """bool per splat: what a mask (bool, or bytes with nonzero = visible) keeps"""
    return np.asarray(mask) != 0


def index_map(keep):
    """(map, K): map[i] = the new upload index of splat i -- the exclusive prefix sum of the keep flags -- or ID_NONE; uint32"""
    keep = keep_of(keep)
    excl = np.cumsum(keep, dtype=np.int64) - keep
    return np.where(keep, excl, ID_NONE).astype(np.uint32), int(keep.sum())


def mask_cases(n):
    """visibility_rule.mask_cases plus the ends of the numbering and, from two chunks on, exactly the flags of one whole chunk
    (C .. 2C - 1) hidden: that chunk's count is 0 and the offsets of the chunks behind it do not move"""
    cases = dict(vr.mask_cases(n))
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[0], last[n - 1] = True, True
    cases["first_only"], cases["last_only"] = first, last
    if n >= 2 * CHUNK:
        hidden = np.ones(n, bool)
        hidden[CHUNK:2 * CHUNK] = False
        cases["one_chunk_hidden"] = hidden
    return cases


# what each case keeps, by its name: n -> K
KEPT_BY_NAME = {
    "all_visible": lambda n: n, "all_hidden": lambda n: 0, "one_visible": lambda n: 1, "every_other": lambda n: (n + 1) // 2,
    "first_only": lambda n: 1, "last_only": lambda n: 1, "one_box_hidden": lambda n: n - vr.BOX, "one_box_visible": lambda n: vr.BOX,
    "one_chunk_hidden": lambda n: n - CHUNK,
}
