// msplat_bin_order.h -- the order in which persistent compositor waves walk the bins (host code; DESIGN.md section 4, "Bin order").
//
// composite_kernel maps work item i to slot (i >> 5) * 8 + (i & 7), workgroup b runs on XCD b % 8 and pulls from queue shard b % 32
// first: XCD x composites the slots with slot % 8 == x, in ascending order.  With the identity table neighbouring bins therefore
// always sit on different XCDs, and the 48-byte record of a splat that covers several bins is fetched through the fabric once per
// XCD that meets it.  bin_order_xcd gives every residue class compact 2-D blocks of bins instead, so that a splat's bins share an L2.
#pragma once

#include <stdint.h>

#include <vector>

namespace msplat {

constexpr int kXcds = 8;
// the block shape the library uses.  Measured at config 2 (EXPERIMENTS.md round 20): 2 x 2, 4 x 2 and 4 x 4 gain 1.8-2.0 % over storage
// order and lie within each other's spread, 8 x 4 and 8 x 8 gain 0.4-0.5 % (an XCD's share of the image gets lumpy: 2040 bins are 72 or
// 40 such blocks for 8 classes)
constexpr int kBinBlockW = 4, kBinBlockH = 4;

// out[slot] = bin (row-major in a tiles_x x rows grid), a permutation of 0 .. tiles_x * rows - 1; a pure function of its arguments.
// The grid is cut into blocks of bw x bh bins (partial at the right and top edges), numbered row-major; block k belongs to class
// k % 8 and every class lists its bins in block order, row-major inside a block.  Slot s takes the next bin of class s % 8 while that
// class has one left, otherwise the next bin of the class with the most left (the lowest such class): affinity is given up only for
// the bins by which the classes differ in size.
inline void bin_order_xcd(int tiles_x, int rows, int bw, int bh, uint32_t* out)
{
    std::vector<uint32_t> cls[kXcds];
    const int nbx = (tiles_x + bw - 1) / bw, nby = (rows + bh - 1) / bh;
    for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
            std::vector<uint32_t>& c = cls[(by * nbx + bx) % kXcds];
            for (int y = by * bh; y < rows && y < (by + 1) * bh; ++y)
                for (int x = bx * bw; x < tiles_x && x < (bx + 1) * bw; ++x) c.push_back((uint32_t)(y * tiles_x + x));
        }
    size_t next[kXcds] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int nbins = tiles_x * rows;
    for (int s = 0; s < nbins; ++s) {
        int c = s % kXcds;
        if (next[c] == cls[c].size()) {
            size_t most = 0;
            for (int k = 0; k < kXcds; ++k)
                if (cls[k].size() - next[k] > most) { most = cls[k].size() - next[k]; c = k; }
        }
        out[s] = cls[c][next[c]++];
    }
}

}  // namespace msplat
