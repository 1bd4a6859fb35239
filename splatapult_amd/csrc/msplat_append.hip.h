// msplat_append.hip.h -- msplat_append_cloud: the selected splats of a source cloud put behind a context's own, in a store of their
// own -- copied where the two stores are of one kind, decoded and encoded again where they are not
// (one of the parts of msplat_kernels.hip.h; host side: msplat_append.hip.inc; the rule: include/msplat.h)
//
// The numbering is the compaction's scan (compact_count / _offsets / _index_kernel of msplat_compact.hip.h, launched as they are)
// over a flag plane that append_flags_kernel makes of the caller's select bytes; its value is the splat's rank among the selected,
// and slot N + rank of the new store is where it goes.  Then
//   append_map_kernel      the caller's index map: N + rank, or MSPLAT_ID_NONE
//   append_gather_kernel   records and positions bit for bit: the context's own rows from storage order to upload order (no map),
//                          and the selected rows of a source of the same kind to slot N + rank
//   append_convert_kernel  the selected rows of a source of ANOTHER kind: transform_kernel's shape, see there
// Every kept byte is read once and written once with 16-byte accesses; a record that is not selected is not read.
#pragma once

#include "msplat_compact.hip.h"

#pragma clang fp contract(off)

namespace msplat {

// select bytes -> the 0 / 1 plane the scan reads: whole chunks of kCompactChunk, zeros behind n.  One 16-byte store per thread and
// turn; the select bytes are a caller's array of any alignment and go byte by byte.  select == nullptr: every splat
__global__ __launch_bounds__(kThreads) void append_flags_kernel(const uint8_t* __restrict__ select, uint32_t n, uint32_t nchunks,
                                                                uint8_t* __restrict__ flags)
{
    const uint32_t groups = nchunks * (uint32_t)kThreads;       // of kCompactItems flags
    for (uint32_t g = blockIdx.x * kThreads + threadIdx.x; g < groups; g += gridDim.x * kThreads) {
        const uint32_t i0 = g * (uint32_t)kCompactItems;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < kCompactItems; ++k) {
            const uint32_t i = i0 + (uint32_t)k;
            const bool on = i < n && (select ? select[i] != 0 : true);
            w[k >> 2] |= (on ? 1u : 0u) << (8 * (k & 3));
        }
        *reinterpret_cast<uint4*>(flags + (size_t)i0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// the caller's map (4-byte aligned): the scan's rank + base, MSPLAT_ID_NONE kept
__global__ __launch_bounds__(kThreads) void append_map_kernel(const uint32_t* __restrict__ rank, uint32_t n, uint32_t base,
                                                              uint32_t* __restrict__ index_map)
{
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const uint32_t r = rank[i];
        index_map[i] = r == kCompactNone ? kCompactNone : r + base;
    }
}

// stored slot j of a cloud, upload index u = order[j] -> slot base + rank[u] of the new store (rank == nullptr: base + u, every
// record).  compact_gather_kernel's loop: one wave moves 64 / F4 records per step with coalesced 16-byte accesses; a record that
// is not selected is not read
__global__ __launch_bounds__(kThreads) void append_gather_kernel(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ order,
                                                                 uint32_t n, uint32_t base, int F4, const float4* __restrict__ pos_in,
                                                                 const float4* __restrict__ recs_in, float4* __restrict__ pos_out,
                                                                 float4* __restrict__ recs_out)
{
    const uint64_t total = (uint64_t)n * (uint32_t)F4;
    for (uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kThreads) {
        const uint32_t j = (uint32_t)(e / (uint32_t)F4), sub = (uint32_t)(e - (uint64_t)j * (uint32_t)F4);
        const uint32_t u = order ? order[j] : j;
        uint32_t dst = u;
        if (rank) {
            dst = rank[u];
            if (dst == kCompactNone) continue;
        }
        dst += base;
        recs_out[(size_t)dst * F4 + sub] = recs_in[e];
        if (sub == 0u) pos_out[dst] = pos_in[j];
    }
}

struct AppendConvertArgs {
    const float4* pos_in;       // the source store (storage order)
    const float4* recs_in;
    const uint32_t* order;      // slot -> upload index of a reordered source store; nullptr: it is in upload order
    const uint32_t* rank;       // per source upload index: rank among the selected, or MSPLAT_ID_NONE
    float4* pos_out;            // the new store, in upload order
    float4* recs_out;
    uint32_t* n_over;           // the pack routines' count (store_record's)
    uint32_t n;                 // source splats
    uint32_t base;              // the destination's own splats: rank r goes to slot base + r
};

// A workgroup is one wave; a wave takes 64 stored source slots per turn.  Nothing selected among them (a ballot): the turn ends
// before a record is loaded.  Otherwise the selected rows of the span -- and only those -- go to LDS with coalesced 16-byte loads, each
// selected lane decodes its row to the FP32 record floats (the values msplat_download_cloud returns; padding 0) and encodes them in the
// destination kind as store_record does, and the wave writes the rows to slot base + rank with 16-byte stores.  pos4 is copied:
// the 16-float head -- centre, alpha, covariance -- is fp32 in every kind, so the footprint bound an upload would compute is the same.
// A row is padded to an odd number of words (transform_kernel: 64 lanes, 64 banks).  An FP32 row is not held in registers: the pack
// routines read it from LDS, the unpack routines write it there.
template <bool FULL_SH, int SRC_STORAGE, int DST_STORAGE>
__global__ __launch_bounds__(64) void append_convert_kernel(const AppendConvertArgs a)
{
    static_assert(SRC_STORAGE != DST_STORAGE, "a source of the same kind is copied (append_gather_kernel)");
    constexpr int SF4 = cloud_f4(SRC_STORAGE, FULL_SH), DF4 = cloud_f4(DST_STORAGE, FULL_SH);
    constexpr int SRW = SF4 * 4, DRW = DF4 * 4;
    constexpr int STRIDE = (SRW > DRW ? SRW : DRW) + 1;
    constexpr int NF = (FULL_SH ? 16 : 8) * 4;          // FP32 record floats
    __shared__ uint32_t s_rec[64 * STRIDE];
    const uint32_t lane = threadIdx.x;
    const uint32_t nwaves = (a.n + 63u) / 64u;
    for (uint32_t wv = blockIdx.x; wv < nwaves; wv += gridDim.x) {
        const uint32_t j0 = wv * 64u, rows = min(64u, a.n - j0);
        const bool mine = lane < rows;
        const uint32_t j = j0 + lane;
        const uint32_t rk = mine ? a.rank[a.order ? a.order[j] : j] : kCompactNone;
        const bool sel = rk != kCompactNone;
        const unsigned long long picked = __ballot(sel);
        if (picked == 0ull) continue;                   // (wave-uniform) no record of the span is read
        const float4* src = a.recs_in + (size_t)j0 * SF4;
#pragma unroll
        for (int k = 0; k < SF4; ++k) {
            const uint32_t e = (uint32_t)k * 64u + lane, r = e / (uint32_t)SF4;
            if (e < rows * (uint32_t)SF4 && ((picked >> r) & 1ull)) {
                const float4 v = src[e];
                uint32_t* w = s_rec + r * STRIDE + (e % (uint32_t)SF4) * 4u;
                w[0] = __float_as_uint(v.x); w[1] = __float_as_uint(v.y); w[2] = __float_as_uint(v.z); w[3] = __float_as_uint(v.w);
            }
        }
        __syncthreads();
        if (sel) {
            uint32_t* row = s_rec + lane * STRIDE;
            if constexpr (SRC_STORAGE == kStorageFp32) {
                uint32_t w[DRW];
                uint32_t over;
                const float* f = reinterpret_cast<const float*>(row);
                if constexpr (DST_STORAGE == kStorageShQ8) over = sh8_pack<FULL_SH>(f, w); else over = sh16_pack<FULL_SH>(f, w);
                if (over) atomicAdd(a.n_over, over);
#pragma unroll
                for (int k = 0; k < DRW; ++k) row[k] = w[k];
            } else if constexpr (DST_STORAGE == kStorageFp32) {
                uint32_t w[SRW];
#pragma unroll
                for (int k = 0; k < SRW; ++k) w[k] = row[k];
#pragma unroll
                for (int k = 0; k < NF; ++k) row[k] = 0u;
                float* f = reinterpret_cast<float*>(row);
                if constexpr (SRC_STORAGE == kStorageShQ8) sh8_unpack<FULL_SH>(w, f); else sh16_unpack<FULL_SH>(w, f);
            } else {
                uint32_t w[SRW > DRW ? SRW : DRW];
                float f[NF];
#pragma unroll
                for (int k = 0; k < SRW; ++k) w[k] = row[k];
#pragma unroll
                for (int k = 0; k < NF; ++k) f[k] = 0.0f;
                if constexpr (SRC_STORAGE == kStorageShQ8) sh8_unpack<FULL_SH>(w, f); else sh16_unpack<FULL_SH>(w, f);
                uint32_t over;
                if constexpr (DST_STORAGE == kStorageShQ8) over = sh8_pack<FULL_SH>(f, w); else over = sh16_pack<FULL_SH>(f, w);
                if (over) atomicAdd(a.n_over, over);
#pragma unroll
                for (int k = 0; k < DRW; ++k) row[k] = w[k];
            }
            a.pos_out[a.base + rk] = a.pos_in[j];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < DF4; ++k) {
            const uint32_t e = (uint32_t)k * 64u + lane;
            const uint32_t r = e / (uint32_t)DF4, sub = e % (uint32_t)DF4;
            const uint32_t d = __shfl(rk, r & 63u, 64);      // (every lane takes part in the shuffle)
            if (r < rows && ((picked >> (r & 63u)) & 1ull)) {
                const uint32_t* w = s_rec + r * STRIDE + sub * 4u;
                a.recs_out[(size_t)(a.base + d) * DF4 + sub] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
            }
        }
        __syncthreads();                                // the rows are read before the next turn overwrites them
    }
}

}  // namespace msplat
