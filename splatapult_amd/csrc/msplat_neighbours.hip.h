// msplat_neighbours.hip.h -- selection by neighbourhood: what is AROUND a splat as one float per splat (msplat_neighbour_values): the
// number of source splats within a radius of its centre, or the squared distance to the nearest one
// (one of the parts of msplat_kernels.hip.h; host side: msplat_neighbours.hip.inc; the rule: include/msplat.h)
//
// The rule is brute force over all pairs; the hash grid below only decides which pairs are tested, never what a pair contributes:
//   neighbour_count_kernel     sources per hash bucket (integer atomics)
//   neighbour_sums_kernel      bucket counts per chunk of kNearChunk buckets, the fullest bucket
//   compact_offsets_kernel     (msplat_compact.hip.h) exclusive scan of the chunk sums, the total
//   neighbour_starts_kernel    start[b] = the entries in front of bucket b
//   neighbour_scatter_kernel   entry = (x, y, z, bits of the upload index) into its bucket's range, through an atomic cursor
//   neighbour_tests_kernel     the candidate pairs the search may test: the budget's number (row reduction)
//   neighbour_fill_kernel      the value of a selected query without a finite centre: it has no neighbour
//   neighbour_search_kernel    one lane per query entry, in bucket order: the buckets of its 27 cells, every bucket once
// No workgroup waits for another one.  The order inside a bucket varies from run to run; a count and a minimum do not depend on it.
// A set (sources, queries) is listed by the same four kernels: the query list is a grid of its own, walked entry by entry, so that
// neighbouring lanes hold queries of one bucket -- mostly of one cell -- and walk the same candidate ranges.
#pragma once

#include "msplat_compact.hip.h"
#include "msplat_rows.hip.h"
#include "msplat_values.hip.h"

#pragma clang fp contract(off)

namespace msplat {

constexpr int kNearCount = 0, kNearDist2 = 1;              // mirrors MSPLAT_NEAR_* (static_assert in msplat_neighbours.hip.inc)
// The cell function, in DOUBLE and without an origin: cell = floor(x * (1 / h)), edge h = radius * kNearEdge, clamped to
// [-kNearCellMax, kNearCellMax].  DESIGN.md derives the pair: at |t| <= 2^40 + 2 the rounding of the product moves the two t of a
// pair by 2^-12 of a cell together, radius / h = 0.99902 leaves 2^-10 for that and for the rounding of d2, r2 and 1 / h.  (An
// fp32 cell function needs an origin inside the cloud to keep |t| small; the minimum of the centres is not one -- a single outlier
// 1000 m below the scan moves it there and clamps the whole scan into one cell -- and a robust origin costs more than fp64 does.)
constexpr double kNearEdge = 1.0009765625;                 // 1 + 2^-10
constexpr double kNearCellMax = 1099511627776.0;           // 2^40: beyond it two different fp32 coordinates are many cells apart
constexpr int kNearItems = 16;                             // bucket counts per thread in the scan: four 16-byte loads
constexpr int kNearChunk = kThreads * kNearItems;          // 4096 buckets per workgroup and turn
constexpr uint32_t kNearBucketsMax = 1u << 24;

struct NearCells {
    double inv_h;               // 1 / h, in double, rounded once on the host
    uint32_t mask;              // buckets - 1, buckets a power of two
};

struct TestsRow {                       // what neighbour_tests_kernel reduces
    unsigned long long tests;

    __host__ __device__ __forceinline__ void clear() { tests = 0ull; }
    __device__ __forceinline__ void merge(const TestsRow& o) { tests += o.tests; }
};

__device__ __forceinline__ bool near_finite(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// floor((double)x * inv_h), clamped: one rounding, the product's.  A finite x gives a finite product (inv_h < 2^65), never a NaN
__device__ __forceinline__ long long near_cell(float x, double inv_h)
{
    const double t = floor(__dmul_rn((double)x, inv_h));
    return (long long)fmin(fmax(t, -kNearCellMax), kNearCellMax);
}

// odd multipliers for the low words, others for the 9 bits above them, then the 32-bit finaliser of MurmurHash3 (public domain):
// the low bits the mask keeps depend on every input bit
__device__ __forceinline__ uint32_t near_bucket(long long cx, long long cy, long long cz, uint32_t mask)
{
    uint32_t h = ((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u);
    h ^= (uint32_t)(cx >> 32) * 0x9E3779B1u + (uint32_t)(cy >> 32) * 0x7FEB352Du + (uint32_t)(cz >> 32) * 0x846CA68Bu;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h & mask;
}

__device__ __forceinline__ uint32_t near_bucket_of(const float4 p, const NearCells& g)
{
    return near_bucket(near_cell(p.x, g.inv_h), near_cell(p.y, g.inv_h), near_cell(p.z, g.inv_h), g.mask);
}

// ---- a set's list.  The members of a set: set[upload index] != 0 (nullptr: every splat) and a finite centre
struct NearSetArgs {
    const float4* pos;          // the store's plane (storage order)
    const uint32_t* order;      // slot -> upload index of a reordered store; nullptr: the store is in upload order
    const uint8_t* set;
    uint32_t n;
    NearCells g;
    uint32_t* cnt;              // [cells]: members per bucket after the count, 0 again after the scatter
    const uint32_t* start;      // [cells]: the scatter reads it
    float4* ent;                // [n]: the scatter writes it
};

// the slot's member, if it holds one: its centre, upload index and bucket
__device__ __forceinline__ bool near_member(const NearSetArgs& a, uint32_t slot, float4& p, uint32_t& u, uint32_t& b)
{
    if (slot >= a.n) return false;
    u = a.order ? a.order[slot] : slot;
    if (a.set && a.set[u] == 0) return false;
    p = a.pos[slot];
    if (!near_finite(p)) return false;
    b = near_bucket_of(p, a.g);
    return true;
}

// As if every active lane had run atomicAdd(&cnt[b], delta) and received the old value, for delta = +1 or -1 (called by whole waves).
// Where all active lanes of the wave name ONE bucket -- coincident centres, a dense cell of a store in Morton order -- its first
// lane adds their number once and the lanes take consecutive values: one atomic on the line instead of 64 (Guideline 12's
// per-wave aggregate, which the compiler forms by itself only for a wave-uniform address)
template <int DELTA>
__device__ __forceinline__ uint32_t near_bucket_add(uint32_t* __restrict__ cnt, uint32_t b, bool active)
{
    const unsigned long long act = __ballot(active);
    if (!act) return 0u;
    const int lane = threadIdx.x & 63, first = __ffsll((long long)act) - 1;
    const uint32_t b0 = __shfl(b, first, 64);
    if (__ballot(active && b == b0) == act) {
        const uint32_t all = (uint32_t)__popcll(act);
        uint32_t old = 0u;
        if (lane == first) old = DELTA > 0 ? atomicAdd(&cnt[b0], all) : atomicSub(&cnt[b0], all);
        old = __shfl(old, first, 64);
        const uint32_t rank = (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
        return DELTA > 0 ? old + rank : old - rank;
    }
    if (!active) return 0u;
    return DELTA > 0 ? atomicAdd(&cnt[b], 1u) : atomicSub(&cnt[b], 1u);
}

__global__ __launch_bounds__(kThreads) void neighbour_count_kernel(const NearSetArgs a)
{
    for (uint32_t base = blockIdx.x * kThreads; base < a.n; base += gridDim.x * kThreads) {
        float4 p;
        uint32_t u, b = 0u;
        const bool member = near_member(a, base + threadIdx.x, p, u, b);
        (void)near_bucket_add<1>(a.cnt, b, member);
    }
}

// the thread's 16 counts of chunk `chunk` (the arrays are padded to whole chunks)
__device__ __forceinline__ void near_load_counts(const uint32_t* __restrict__ cnt, uint32_t chunk, uint32_t c[kNearItems])
{
    const uint4* p = reinterpret_cast<const uint4*>(cnt + (size_t)chunk * kNearChunk + threadIdx.x * kNearItems);
#pragma unroll
    for (int k = 0; k < kNearItems / 4; ++k) {
        const uint4 v = p[k];
        c[4 * k] = v.x; c[4 * k + 1] = v.y; c[4 * k + 2] = v.z; c[4 * k + 3] = v.w;
    }
}

// sums[chunk] = the members of the chunk's buckets; *max_bucket (zeroed by the host; nullptr: not wanted) = the fullest bucket
__global__ __launch_bounds__(kThreads) void neighbour_sums_kernel(const uint32_t* __restrict__ cnt, uint32_t nchunks, uint32_t* __restrict__ sums,
                                                                  uint32_t* __restrict__ max_bucket)
{
    __shared__ uint32_t s_sum[kThreads / 64], s_max[kThreads / 64];
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        uint32_t c[kNearItems], sum = 0u, top = 0u;
        near_load_counts(cnt, chunk, c);
#pragma unroll
        for (int k = 0; k < kNearItems; ++k) {
            sum += c[k];
            top = max(top, c[k]);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            sum += __shfl_xor(sum, d, 64);
            top = max(top, (uint32_t)__shfl_xor(top, d, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            s_sum[threadIdx.x >> 6] = sum;
            s_max[threadIdx.x >> 6] = top;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0u, m = 0u;
#pragma unroll
            for (int w = 0; w < kThreads / 64; ++w) {
                t += s_sum[w];
                m = max(m, s_max[w]);
            }
            sums[chunk] = t;
            if (max_bucket && m) atomicMax(max_bucket, m);
        }
        __syncthreads();
    }
}

// start[b] = offsets[chunk of b] + the members of the chunk's buckets in front of b
__global__ __launch_bounds__(kThreads) void neighbour_starts_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ offsets,
                                                                    uint32_t nchunks, uint32_t* __restrict__ start)
{
    __shared__ uint32_t s_tmp[kThreads / 64];
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        uint32_t c[kNearItems], sum = 0u, total;
        near_load_counts(cnt, chunk, c);
#pragma unroll
        for (int k = 0; k < kNearItems; ++k) sum += c[k];
        uint32_t run = offsets[chunk] + block_incl_scan(sum, s_tmp, total) - sum;
        uint4* out = reinterpret_cast<uint4*>(start + (size_t)chunk * kNearChunk + threadIdx.x * kNearItems);
#pragma unroll
        for (int k = 0; k < kNearItems / 4; ++k) {
            uint4 v;
            v.x = run; run += c[4 * k];
            v.y = run; run += c[4 * k + 1];
            v.z = run; run += c[4 * k + 2];
            v.w = run; run += c[4 * k + 3];
            out[k] = v;
        }
    }
}

// a member takes the last free entry of its bucket's range: cnt counts down to 0 and start[b + 1] stays the range's end
__global__ __launch_bounds__(kThreads) void neighbour_scatter_kernel(const NearSetArgs a)
{
    for (uint32_t base = blockIdx.x * kThreads; base < a.n; base += gridDim.x * kThreads) {
        float4 p;
        uint32_t u = 0u, b = 0u;
        const bool member = near_member(a, base + threadIdx.x, p, u, b);
        const uint32_t left = near_bucket_add<-1>(a.cnt, b, member);
        if (member) a.ent[a.start[b] + left - 1u] = make_float4(p.x, p.y, p.z, __uint_as_float(u));
    }
}

// ---- the walk of a query's neighbourhood.  Bit k of the result: cell k (k = dx + 1 + 3 (dy + 1) + 9 (dz + 1)) of the 27 around
// (cx, cy, cz) lies inside the clamp range -- no source lives outside it -- and no cell before it has its bucket.  The 27 buckets
// live in registers for the 351 comparisons and are dead afterwards: the walk recomputes the bucket of each fresh cell (one hash)
// instead of indexing an array, so nothing is spilled
__device__ __forceinline__ void near_cell_at(long long cx, long long cy, long long cz, int k, long long& x, long long& y, long long& z)
{
    x = cx + k % 3 - 1;
    y = cy + (k / 3) % 3 - 1;
    z = cz + k / 9 - 1;
}

__device__ __forceinline__ bool near_in_range(long long x, long long y, long long z)
{
    constexpr long long T = (long long)kNearCellMax;
    return x >= -T && x <= T && y >= -T && y <= T && z >= -T && z <= T;
}

__device__ __forceinline__ uint32_t near_fresh_cells(long long cx, long long cy, long long cz, uint32_t mask)
{
    uint32_t b[27], fresh = 0u;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        long long x, y, z;
        near_cell_at(cx, cy, cz, k, x, y, z);
        const bool in = near_in_range(x, y, z);
        b[k] = in ? near_bucket(x, y, z, mask) : 0xFFFFFFFFu;       // (no bucket: mask <= 2^24 - 1)
        bool first = in;
#pragma unroll
        for (int j = 0; j < k; ++j) first = first && b[j] != b[k];
        fresh |= first ? 1u << k : 0u;
    }
    return fresh;
}

struct NearQueryArgs {
    const float4* qent;         // the query list: (x, y, z, bits of the upload index), in bucket order
    const uint32_t* nq;         // device: its length
    const float4* ent;          // the source grid's entries ...
    const uint32_t* start;      // ... and bucket b's range [start[b], start[b + 1])
    NearCells g;
    float r2;
    uint32_t cap;               // COUNT: stop at cap; 0: no cap
    float* values;              // one float per splat, upload numbering
};

// the sizes of the distinct buckets every query would visit: what msplat_neighbour_values compares with max_tests
__global__ __launch_bounds__(kThreads) void neighbour_tests_kernel(const NearQueryArgs a, TestsRow* __restrict__ part /* [gridDim.x] */)
{
    TestsRow r;
    r.clear();
    const uint32_t nq = *a.nq;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < nq; i += gridDim.x * kThreads) {
        const float4 q = a.qent[i];
        const long long cx = near_cell(q.x, a.g.inv_h), cy = near_cell(q.y, a.g.inv_h), cz = near_cell(q.z, a.g.inv_h);
        const uint32_t fresh = near_fresh_cells(cx, cy, cz, a.g.mask);
        for (int k = 0; k < 27; ++k) {
            if (!((fresh >> k) & 1u)) continue;
            long long x, y, z;
            near_cell_at(cx, cy, cz, k, x, y, z);
            const uint32_t b = near_bucket(x, y, z, a.g.mask);
            r.tests += a.start[b + 1] - a.start[b];
        }
    }
    row_reduce_store(r, part + blockIdx.x);
}

// a selected query without a finite centre has no neighbour: `empty` is 0 (COUNT) or +inf (DIST2).  One lane per stored slot
__global__ __launch_bounds__(kThreads) void neighbour_fill_kernel(const float4* __restrict__ pos, const uint32_t* __restrict__ order,
                                                                  const uint8_t* __restrict__ query, uint32_t n, float empty,
                                                                  float* __restrict__ values)
{
    for (uint32_t slot = blockIdx.x * kThreads + threadIdx.x; slot < n; slot += gridDim.x * kThreads) {
        const uint32_t u = order ? order[slot] : slot;
        if (query && query[u] == 0) continue;
        if (!near_finite(pos[slot])) values[u] = empty;
    }
}

// one lane per query entry.  Every source lies in exactly one bucket and the lane walks each bucket of its neighbourhood once, so a
// source is tested once whatever the collisions; a candidate is judged by its distance alone (dist2_rn, the query's centre first)
template <int KIND>
__global__ __launch_bounds__(kThreads) void neighbour_search_kernel(const NearQueryArgs a)
{
    const uint32_t nq = *a.nq;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < nq; i += gridDim.x * kThreads) {
        const float4 q = a.qent[i];
        const uint32_t qi = __float_as_uint(q.w);
        const long long cx = near_cell(q.x, a.g.inv_h), cy = near_cell(q.y, a.g.inv_h), cz = near_cell(q.z, a.g.inv_h);
        const uint32_t fresh = near_fresh_cells(cx, cy, cz, a.g.mask);
        uint32_t count = 0u;
        float best = INFINITY;
        bool full = false;
        for (int k = 0; k < 27 && !full; ++k) {
            if (!((fresh >> k) & 1u)) continue;
            long long x, y, z;
            near_cell_at(cx, cy, cz, k, x, y, z);
            const uint32_t b = near_bucket(x, y, z, a.g.mask);
            const uint32_t end = a.start[b + 1];
            for (uint32_t e = a.start[b]; e < end && !full; ++e) {
                const float4 c = a.ent[e];
                const float p[3] = {c.x, c.y, c.z};
                const float d2 = dist2_rn(q.x, q.y, q.z, p);
                if (__float_as_uint(c.w) == qi || !(d2 <= a.r2)) continue;
                if constexpr (KIND == kNearCount) {
                    count += 1u;
                    full = a.cap != 0u && count >= a.cap;
                } else {
                    best = fminf(best, d2);
                }
            }
        }
        a.values[qi] = KIND == kNearCount ? (float)count : best;
    }
}

}  // namespace msplat
