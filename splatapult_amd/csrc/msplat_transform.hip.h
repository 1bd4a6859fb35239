// msplat_transform.hip.h -- msplat_transform_cloud: the selected splats of a context's cloud moved by a matrix -- centre, world
// covariance, SH bands 1..3 and the footprint bound -- on their way into a store of their own
// (one of the parts of msplat_kernels.hip.h; host side: msplat_transform.hip.inc; the rule: include/msplat.h)
//
// One launch, one pass: every stored record is read once and written once, 2 x (16 + 16 F4) bytes per splat.  The ingest kernels'
// shape: a workgroup is one wave, a wave takes 64 stored records per turn -- one contiguous span of the store -- with coalesced
// 16-byte loads, and each lane owns a splat.  A wave none of whose splats is selected (a ballot) stores what it loaded and touches
// neither LDS nor the record's contents: compact_gather_kernel's copy.  Otherwise the span goes through LDS, a selected lane decodes
// its row to the FP32 record floats, applies the rule, encodes the row again in the store's kind, and the wave writes the rows out
// with 16-byte stores; an unselected lane leaves its row alone, so its record and its pos4 arrive bit for bit.
// A row is padded by one word: a record is a multiple of 4 words, so the 64 lanes of the per-lane reads and writes would otherwise
// share the banks of 64 / gcd(64, words) addresses; with an odd stride they hit 64 different banks (32 per half wave).
#pragma once

#include "msplat_cloud.hip.h"

#pragma clang fp contract(off)

namespace msplat {

struct TransformArgs {
    const float4* pos_in;       // the old store (storage order)
    const float4* recs_in;
    const uint32_t* order;      // slot -> upload index of a reordered store; nullptr: the store is in upload order
    const uint8_t* select;      // one byte per splat in UPLOAD numbering, nonzero = transformed; nullptr: every splat
    float4* pos_out;            // the new store, in upload order
    float4* recs_out;
    uint32_t* n_over;           // the pack routines' count (store_record's)
    uint32_t n;
    int keep_sh;                // MSPLAT_TRANSFORM_KEEP_SH: d1 .. d3 are not read
    float m[12];                // rows 0..2 of M: m[3 k + r] = M[4 k + r] = A[k][r], k = 3: the translation
    float d1[9], d2[25], d3[49];      // msplat_sh_rotation's matrices, row-major
};

// record float of SH coefficient k (1..15) of channel c
__host__ __device__ constexpr int sh_slot(int c, int k) { return k < 4 ? 4 + 4 * c + k : 25 + 12 * c + (k - 4); }

// The FP32 record floats of one splat, where they are: an FP32 store's row in LDS, read and written a few words at a time (the
// compiler then keeps no more of the record in registers than one band), or the array a compact record was unpacked into
struct RowFloats {
    uint32_t* w;
    __device__ __forceinline__ float get(int k) const { return __uint_as_float(w[k]); }
    __device__ __forceinline__ void set(int k, float v) const { w[k] = __float_as_uint(v); }
};
struct ArrayFloats {
    float* f;
    __device__ __forceinline__ float get(int k) const { return f[k]; }
    __device__ __forceinline__ void set(int k, float v) const { f[k] = v; }
};

// sh'[k0 + i] = (..(D[i][0] sh[k0] + D[i][1] sh[k0 + 1]) + ..) + D[i][NB - 1] sh[k0 + NB - 1], per channel; fp32, left to right
template <int NB, int K0, class Rec>
__device__ __forceinline__ void rotate_band(const Rec& f, const float* D)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float in[NB], out[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) in[j] = f.get(sh_slot(c, K0 + j));
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            float s = __fmul_rn(D[i * NB], in[0]);
#pragma unroll
            for (int j = 1; j < NB; ++j) s = __fadd_rn(s, __fmul_rn(D[i * NB + j], in[j]));
            out[i] = s;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) f.set(sh_slot(c, K0 + i), out[i]);
    }
}

// the rule of msplat.h on the FP32 record floats; returns the new pos4
template <bool FULL_SH, class Rec>
__device__ __forceinline__ float4 transform_record(const Rec& f, const TransformArgs& a)
{
    const float* m = a.m;
    const float x = f.get(0), y = f.get(1), z = f.get(2);
    float p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[r], x), __fmul_rn(m[3 + r], y)), __fmul_rn(m[6 + r], z)), m[9 + r]);
        f.set(r, p[r]);
    }
    float S[9], T[9];     // T = A S, then S' = T A^T; column-major like S
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = f.get(16 + k);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r)
            T[3 * c + r] = __fadd_rn(__fadd_rn(__fmul_rn(m[r], S[3 * c]), __fmul_rn(m[3 + r], S[3 * c + 1])), __fmul_rn(m[6 + r], S[3 * c + 2]));
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            S[3 * c + r] = __fadd_rn(__fadd_rn(__fmul_rn(T[r], m[c]), __fmul_rn(T[3 + r], m[3 + c])), __fmul_rn(T[6 + r], m[6 + c]));
            f.set(16 + 3 * c + r, S[3 * c + r]);
        }
    const float bound = footprint_bound(S, f.get(3));
    if (!a.keep_sh) {
        rotate_band<3, 1>(f, a.d1);
        if constexpr (FULL_SH) {
            rotate_band<5, 4>(f, a.d2);
            rotate_band<7, 9>(f, a.d3);
        }
    }
    return make_float4(p[0], p[1], p[2], bound);
}

template <bool FULL_SH, int STORAGE>
__global__ __launch_bounds__(64) void transform_kernel(const TransformArgs a)
{
    constexpr int F4 = cloud_f4(STORAGE, FULL_SH);      // float4 per stored record
    constexpr int RW = F4 * 4, STRIDE = RW + 1;         // words per record; per LDS row
    constexpr int NF = (FULL_SH ? 16 : 8) * 4;          // FP32 record floats
    __shared__ uint32_t s_rec[64 * STRIDE];
    const uint32_t lane = threadIdx.x;
    const uint32_t nwaves = (a.n + 63u) / 64u;
    for (uint32_t wv = blockIdx.x; wv < nwaves; wv += gridDim.x) {
        const uint32_t j0 = wv * 64u, rows = min(64u, a.n - j0), elems = rows * (uint32_t)F4;
        const float4* src = a.recs_in + (size_t)j0 * F4;
        float4 v[F4];
#pragma unroll
        for (int k = 0; k < F4; ++k) {
            const uint32_t e = (uint32_t)k * 64u + lane;
            if (e < elems) v[k] = src[e];
        }
        const bool mine = lane < rows;
        const uint32_t j = j0 + lane;
        const uint32_t dst = mine ? (a.order ? a.order[j] : j) : 0u;      // the row's slot in the new store: its upload index
        const bool sel = mine && (a.select ? a.select[dst] != 0 : true);
        float4 p = mine ? a.pos_in[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (__ballot(sel) == 0ull) {                    // (wave-uniform) nothing to transform: the gather's copy
#pragma unroll
            for (int k = 0; k < F4; ++k) {
                const uint32_t e = (uint32_t)k * 64u + lane;
                const uint32_t d = __shfl(dst, (e / (uint32_t)F4) & 63u, 64);      // (every lane takes part in the shuffle)
                if (e < elems) a.recs_out[(size_t)d * F4 + e % (uint32_t)F4] = v[k];
            }
            if (mine) a.pos_out[dst] = p;
            continue;
        }
#pragma unroll
        for (int k = 0; k < F4; ++k) {
            const uint32_t e = (uint32_t)k * 64u + lane;
            if (e < elems) {
                uint32_t* w = s_rec + (e / (uint32_t)F4) * STRIDE + (e % (uint32_t)F4) * 4u;
                w[0] = __float_as_uint(v[k].x); w[1] = __float_as_uint(v[k].y); w[2] = __float_as_uint(v[k].z); w[3] = __float_as_uint(v[k].w);
            }
        }
        __syncthreads();
        if (sel) {
            uint32_t* row = s_rec + lane * STRIDE;
            if constexpr (STORAGE == kStorageFp32) {
                p = transform_record<FULL_SH>(RowFloats{row}, a);
            } else {
                uint32_t w[RW];
                float f[NF];
#pragma unroll
                for (int k = 0; k < RW; ++k) w[k] = row[k];
#pragma unroll
                for (int k = 0; k < NF; ++k) f[k] = 0.0f;
                if constexpr (STORAGE == kStorageShQ8) sh8_unpack<FULL_SH>(w, f); else sh16_unpack<FULL_SH>(w, f);
                p = transform_record<FULL_SH>(ArrayFloats{f}, a);
                uint32_t over;
                if constexpr (STORAGE == kStorageShQ8) over = sh8_pack<FULL_SH>(f, w); else over = sh16_pack<FULL_SH>(f, w);
                if (over) atomicAdd(a.n_over, over);
#pragma unroll
                for (int k = 0; k < RW; ++k) row[k] = w[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < F4; ++k) {
            const uint32_t e = (uint32_t)k * 64u + lane;
            const uint32_t r = e / (uint32_t)F4, sub = e % (uint32_t)F4;
            const uint32_t d = __shfl(dst, r & 63u, 64);
            if (e < elems) {
                const uint32_t* w = s_rec + r * STRIDE + sub * 4u;
                a.recs_out[(size_t)d * F4 + sub] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
            }
        }
        if (mine) a.pos_out[dst] = p;
        __syncthreads();                                // the rows are read before the next turn overwrites them
    }
}

}  // namespace msplat
