// msplat_compact.hip.h -- msplat_compact_cloud: the splats a context's mask and crop let through, gathered into a store of their own
// (one of the parts of msplat_kernels.hip.h; host side: msplat_compact.hip.inc)
//
// Five plain launches on the context's stream, each reading what the one before it wrote:
//   compact_flags_kernel    one byte per splat in UPLOAD numbering: 1 = kept (the rule of visibility_kernel, msplat_cloud.hip.h)
//   compact_count_kernel    kept splats per chunk of kCompactChunk flags
//   compact_offsets_kernel  exclusive scan of the chunk counts (one workgroup), the total K
//   compact_index_kernel    index_map[u] = new upload index of splat u (the exclusive prefix sum of the flags) or MSPLAT_ID_NONE
//   compact_gather_kernel   the kept records and positions, bit for bit, to slot index_map[u] of the new store
// No workgroup waits for another one: the scan is three launches, not a decoupled look-back.
#pragma once

#include "msplat_cloud.hip.h"

#pragma clang fp contract(off)

namespace msplat {

constexpr int kCompactItems = 16;                           // flag bytes per thread: one 16-byte load
constexpr int kCompactChunk = kThreads * kCompactItems;     // 4096 flags per workgroup and turn
constexpr uint32_t kCompactNone = 0xFFFFFFFFu;              // MSPLAT_ID_NONE

struct CompactFlagsArgs {
    const float4* pos;          // the store's plane (storage order)
    const uint8_t* mask;        // one byte per splat in UPLOAD numbering, nonzero = kept; nullptr: no mask
    const uint32_t* order;      // slot -> upload index of a reordered store; nullptr: the store is in upload order
    uint32_t n;
    int shape;                  // MSPLAT_CROP_BOX / _SPHERE, | MSPLAT_CROP_INVERT; 0: no crop
    float m[16];                // world -> crop space, column-major; row 3 is not read
    uint8_t* flags;             // out: 0 / 1 per splat, upload numbering
};

// one lane per stored slot.  The crop is evaluated here, on the store's own centres, not read off the context's plane: there a NaN x
// means "hidden", and a genuine NaN centre under a mask alone is a kept splat
__global__ __launch_bounds__(kThreads) void compact_flags_kernel(const CompactFlagsArgs a)
{
    for (uint32_t slot = blockIdx.x * kThreads + threadIdx.x; slot < a.n; slot += gridDim.x * kThreads) {
        const uint32_t u = a.order ? a.order[slot] : slot;
        bool keep = a.mask ? a.mask[u] != 0 : true;
        if (a.shape != 0) keep = keep && (crop_inside(a.pos[slot], a.m, a.shape) != ((a.shape & kCropInvert) != 0));
        a.flags[u] = keep ? 1 : 0;
    }
}

// the thread's 16 flags of chunk `chunk` (the plane is padded with zeros to whole chunks and 16-byte aligned)
__device__ __forceinline__ uint4 compact_load_flags(const uint8_t* __restrict__ flags, uint32_t chunk)
{
    return *reinterpret_cast<const uint4*>(flags + (size_t)chunk * kCompactChunk + threadIdx.x * kCompactItems);
}

// (every byte is 0 or 1: the kept count is the population count)
__device__ __forceinline__ uint32_t compact_popc(const uint4 f) { return __popc(f.x) + __popc(f.y) + __popc(f.z) + __popc(f.w); }

__global__ __launch_bounds__(kThreads) void compact_count_kernel(const uint8_t* __restrict__ flags, uint32_t nchunks,
                                                                 uint32_t* __restrict__ counts)
{
    __shared__ uint32_t s_w[kThreads / 64];
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        uint32_t c = compact_popc(compact_load_flags(flags, chunk));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
        if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
#pragma unroll
            for (int w = 0; w < kThreads / 64; ++w) t += s_w[w];
            counts[chunk] = t;
        }
        __syncthreads();
    }
}

// counts[chunk] -> the kept splats in front of the chunk, in place; *total = K.  One workgroup, kThreads chunks per turn: 2^24
// splats are 4096 chunks, 16 turns
__global__ __launch_bounds__(kThreads) void compact_offsets_kernel(uint32_t* __restrict__ counts, uint32_t nchunks,
                                                                   uint32_t* __restrict__ total)
{
    __shared__ uint32_t s_tmp[kThreads / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nchunks; base += kThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < nchunks ? counts[i] : 0u;
        uint32_t sum;
        const uint32_t incl = block_incl_scan(c, s_tmp, sum);
        if (i < nchunks) counts[i] = carry + incl - c;
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}

// per chunk: the thread's prefix over its 16 bytes, the workgroup's scan of the thread counts, the chunk's base.  The 4096 map
// words go through LDS so that a wave stores 256 contiguous bytes (index_map is only 4-byte aligned: dword stores); a row of 16
// words is padded by one, so the 64 lanes of the transposing writes hit 64 different banks
__global__ __launch_bounds__(kThreads) void compact_index_kernel(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ offsets,
                                                                 uint32_t n, uint32_t nchunks, uint32_t* __restrict__ index_map)
{
    __shared__ uint32_t s_tmp[kThreads / 64];
    __shared__ uint32_t s_map[kCompactChunk + kCompactChunk / kCompactItems];
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint4 f = compact_load_flags(flags, chunk);
        const uint32_t c = compact_popc(f);
        uint32_t sum;
        uint32_t rank = offsets[chunk] + block_incl_scan(c, s_tmp, sum) - c;
        const uint32_t w[4] = {f.x, f.y, f.z, f.w};
        uint32_t* row = s_map + threadIdx.x * (kCompactItems + 1);
#pragma unroll
        for (int k = 0; k < kCompactItems; ++k) {
            const uint32_t keep = (w[k >> 2] >> (8 * (k & 3))) & 1u;
            row[k] = keep ? rank : kCompactNone;
            rank += keep;
        }
        __syncthreads();
        const uint32_t u0 = chunk * (uint32_t)kCompactChunk;
#pragma unroll
        for (int k = 0; k < kCompactItems; ++k) {
            const uint32_t s = k * kThreads + threadIdx.x;
            if (u0 + s < n) index_map[u0 + s] = s_map[s + s / kCompactItems];
        }
        __syncthreads();
    }
}

// old stored slot j, upload index u = order[j] -> slot index_map[u] of the new store, which is in (new) upload order.  The loop of
// gather_cloud_kernel: one wave moves 64 / F4 records per step with coalesced 16-byte accesses; a dropped record is not read
__global__ __launch_bounds__(kThreads) void compact_gather_kernel(const uint32_t* __restrict__ index_map, const uint32_t* __restrict__ order,
                                                                  uint32_t n, int F4, const float4* __restrict__ pos_in,
                                                                  const float4* __restrict__ recs_in, float4* __restrict__ pos_out,
                                                                  float4* __restrict__ recs_out)
{
    const uint64_t total = (uint64_t)n * (uint32_t)F4;
    for (uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kThreads) {
        const uint32_t j = (uint32_t)(e / (uint32_t)F4), sub = (uint32_t)(e - (uint64_t)j * (uint32_t)F4);
        const uint32_t dst = index_map[order ? order[j] : j];
        if (dst == kCompactNone) continue;
        recs_out[(size_t)dst * F4 + sub] = recs_in[e];
        if (sub == 0u) pos_out[dst] = pos_in[j];
    }
}

}  // namespace msplat
