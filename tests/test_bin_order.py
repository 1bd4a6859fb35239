"""The XCD-local bin order of the persistent compositor waves (splatapult_amd/csrc/msplat_bin_order.h), on the host.

msplat_debug_bin_order(tiles_x, rows) is the table order[slot] -> bin that msplat_device.hip uploads: composite_kernel gives the
slots of one residue class mod 8 to one XCD, and the table is built so that each class is made of compact blocks of bins.  The
construction is restated here in Python (blocks of BLOCK bins numbered row-major, block k in class k % 8, slot s takes the next
bin of class s % 8 while it has one, else of the fullest class) and every bound below is derived from it, none from a run."""
import ctypes as C

import numpy as np
import pytest

from splatapult_amd import _capi

BLOCK = (4, 4)        # the compiled-in block shape (bins): kBinBlockW x kBinBlockH
GRIDS = [(1, 1), (1, 255), (255, 1), (3, 2), (7, 5), (8, 8), (9, 17), (60, 34), (63, 70), (256, 256)]


def host_order(tiles_x, rows):
    out = np.full(tiles_x * rows, 0xFFFFFFFF, np.uint32)
    assert _capi.lib().msplat_debug_bin_order(tiles_x, rows, out.ctypes.data_as(C.POINTER(C.c_uint32))) == _capi.OK
    return out


def block_class(tiles_x, rows):
    """class of every bin: its block's row-major number mod 8"""
    bw, bh = BLOCK
    nbx = (tiles_x + bw - 1) // bw
    y, x = np.divmod(np.arange(tiles_x * rows), tiles_x)
    return ((y // bh) * nbx + x // bw) % 8


def restated(tiles_x, rows):
    bw, bh = BLOCK
    nbx, nby = (tiles_x + bw - 1) // bw, (rows + bh - 1) // bh
    cls = [[] for _ in range(8)]
    for by in range(nby):
        for bx in range(nbx):
            c = cls[(by * nbx + bx) % 8]
            for y in range(by * bh, min(rows, (by + 1) * bh)):
                c.extend(range(y * tiles_x + bx * bw, y * tiles_x + min(tiles_x, (bx + 1) * bw)))
    nxt, out = [0] * 8, []
    for s in range(tiles_x * rows):
        c = s % 8
        if nxt[c] == len(cls[c]):
            c = max(range(8), key=lambda k: (len(cls[k]) - nxt[k], -k))
        out.append(cls[c][nxt[c]])
        nxt[c] += 1
    return np.array(out, np.uint32)


@pytest.mark.parametrize("tiles_x,rows", GRIDS)
def test_the_table_is_a_permutation_built_as_documented(tiles_x, rows):
    got = host_order(tiles_x, rows)
    np.testing.assert_array_equal(np.sort(got), np.arange(tiles_x * rows, dtype=np.uint32))
    np.testing.assert_array_equal(got, restated(tiles_x, rows))
    np.testing.assert_array_equal(got, host_order(tiles_x, rows))          # a pure function


@pytest.mark.parametrize("tiles_x,rows", GRIDS)
def test_slot_s_holds_a_bin_of_class_s_mod_8_but_for_the_remainder(tiles_x, rows):
    """The fill rule, walked slot by slot: slot s holds a bin of class s % 8 unless that class had none left by then, and then one of
    the class that had the most left.  The remainder: nothing is taken from another class before the first class runs out, and with
    m = the smallest class no class runs out before slot 8 m (each has filled m of its own slots by then) -- so every slot below 8 m
    follows its class, and at most n - 8 m slots, the bins by which the classes differ in size, do not."""
    got = host_order(tiles_x, rows)
    n = tiles_x * rows
    cls = block_class(tiles_x, rows)
    left = np.bincount(cls, minlength=8)
    m = int(left.min())
    foreign = 0
    for s in range(n):
        c, have = s % 8, int(cls[got[s]])
        if left[c] > 0:
            assert have == c, (s, c, have)
        else:
            assert left[have] == left.max(), (s, have, left)
            assert s >= 8 * m
            foreign += 1
        left[have] -= 1
    assert foreign <= n - 8 * m


def test_neighbouring_bins_share_their_class_at_1080p():
    """60 x 34 bins (1920 x 1080).  A bin shares its block -- hence its class -- with its right-hand neighbour unless it is the last
    of its block's row, and with the neighbour below unless it is in the block's last row: in a full bw x bh block all but one bin
    has such a neighbour, (bw * bh - 1) / (bw * bh) >= 3 / 4 for every shape from 2 x 2 up.  The slots follow the classes except for
    the remainder (the test above), so the share is taken over slot % 8 and the bins in foreign slots count against it."""
    tiles_x, rows = 60, 34
    bw, bh = BLOCK
    got = host_order(tiles_x, rows)
    slot_class = np.empty(tiles_x * rows, np.int64)
    slot_class[got] = np.arange(tiles_x * rows) % 8
    g = slot_class.reshape(rows, tiles_x)
    y, x = np.divmod(np.arange(tiles_x * rows).reshape(rows, tiles_x), tiles_x)
    right_in_block = (x % bw != bw - 1) & (x + 1 < tiles_x)
    below_in_block = (y % bh != bh - 1) & (y + 1 < rows)
    shares = np.zeros((rows, tiles_x), bool)
    shares[:, :-1] |= right_in_block[:, :-1] & (g[:, :-1] == g[:, 1:])
    shares[:-1, :] |= below_in_block[:-1, :] & (g[:-1, :] == g[1:, :])
    has_neighbour = right_in_block | below_in_block
    assert (bw * bh - 1) / (bw * bh) >= 0.75
    assert shares.sum() >= 0.75 * tiles_x * rows, (shares.sum(), tiles_x * rows)
    # whenever the neighbour lies in the same block, the classes agree -- but for the bins in foreign slots, each of which can spoil
    # itself, its left-hand neighbour and the one above
    cls = block_class(tiles_x, rows)
    foreign = (cls != slot_class).sum()
    assert (has_neighbour & ~shares).sum() <= 3 * foreign


def test_arguments_are_checked():
    L = _capi.lib()
    out = np.zeros(4, np.uint32)
    p = out.ctypes.data_as(C.POINTER(C.c_uint32))
    for tx, rows in [(0, 1), (1, 0), (257, 1), (1, 257), (-1, 4)]:
        assert L.msplat_debug_bin_order(tx, rows, p) == _capi.ERR_INVALID_ARG
    assert L.msplat_debug_bin_order(2, 2, None) == _capi.ERR_INVALID_ARG
