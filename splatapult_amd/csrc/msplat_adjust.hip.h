// msplat_adjust.hip.h -- msplat_adjust_cloud: the selected splats of a context's cloud recoloured by an affine map of their colour --
// applied to the SH coefficients, so it holds in every view direction -- and / or faded by a factor on alpha, on their way into a
// store of their own
// (one of the parts of msplat_kernels.hip.h; host side: msplat_adjust.hip.inc; the rule: include/msplat.h)
//
// transform_kernel's shape (msplat_transform.hip.h), written again and not shared -- that kernel's registers stay as they were:
// one launch, one pass, every stored record read once and written once; a workgroup is one wave, a wave takes 64 stored records per
// turn with coalesced 16-byte loads, a wave none of whose splats is selected (a ballot) stores what it loaded and touches no LDS;
// otherwise the span is staged in LDS at an odd row stride, a selected lane applies the rule to its row and the wave writes the
// rows out with 16-byte stores.  The two parts of the rule are wave-uniform switches:
//   colour:  an FP32 row is adjusted where it lies, one coefficient (r g b) at a time; a compact row is unpacked, adjusted and
//            packed again in the store's kind (the DC terms are fp32 words of the head in every kind);
//   opacity: alpha and the covariance are fp32 words of the row in every kind (the head of a compact record): alpha is written,
//            the covariance read for the footprint bound, and nothing behind the head is decoded -- a fade alone never packs.
#pragma once

#include "msplat_transform.hip.h"

#pragma clang fp contract(off)

namespace msplat {

struct AdjustArgs {
    const float4* pos_in;       // the old store (storage order)
    const float4* recs_in;
    const uint32_t* order;      // slot -> upload index of a reordered store; nullptr: the store is in upload order
    const uint8_t* select;      // one byte per splat in UPLOAD numbering, nonzero = adjusted; nullptr: every splat
    float4* pos_out;            // the new store, in upload order
    float4* recs_out;
    uint32_t* n_over;           // the pack routines' count (store_record's)
    uint32_t n;
    int colour, opacity;        // MSPLAT_ADJUST_COLOUR / _OPACITY: which parts of the rule run
    float g[9];                 // g[3 j + c] = G[c][j]: the ABI's first nine floats
    float bias[3];              // what the DC term of channel c gains: the offset and G's action on the 0.5 every colour carries
    float opacity_scale;
};

// record float of SH coefficient k (0..15) of channel c
__host__ __device__ constexpr int sh_slot0(int c, int k) { return k == 0 ? 4 + 4 * c : sh_slot(c, k); }

// the colour part of the rule on the FP32 record floats: the three channels of a coefficient are read before any is written
template <bool FULL_SH, class Rec>
__device__ __forceinline__ void adjust_colour(const Rec& f, const AdjustArgs& a)
{
#pragma unroll
    for (int k = 0; k < (FULL_SH ? 16 : 4); ++k) {
        const float r = f.get(sh_slot0(0, k)), g = f.get(sh_slot0(1, k)), b = f.get(sh_slot0(2, k));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float s = __fadd_rn(__fadd_rn(__fmul_rn(a.g[c], r), __fmul_rn(a.g[3 + c], g)), __fmul_rn(a.g[6 + c], b));
            if (k == 0) s = __fadd_rn(s, a.bias[c]);
            f.set(sh_slot0(c, k), s);
        }
    }
}

template <bool FULL_SH, int STORAGE>
__global__ __launch_bounds__(64) void adjust_kernel(const AdjustArgs a)
{
    constexpr int F4 = cloud_f4(STORAGE, FULL_SH);      // float4 per stored record
    constexpr int RW = F4 * 4, STRIDE = RW + 1;         // words per record; per LDS row
    constexpr int NF = (FULL_SH ? 16 : 8) * 4;          // FP32 record floats
    constexpr int S0 = STORAGE == kStorageFp32 ? 16 : 7;      // the row's word of S[0]: sh16_head_slot(7) = 16; alpha is word 3 in every kind
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
        if (__ballot(sel) == 0ull) {                    // (wave-uniform) nothing to adjust: the gather's copy
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
            if (a.colour) {
                if constexpr (STORAGE == kStorageFp32) {
                    adjust_colour<FULL_SH>(RowFloats{row}, a);
                } else {
                    uint32_t w[RW];
                    float f[NF];
#pragma unroll
                    for (int k = 0; k < RW; ++k) w[k] = row[k];
#pragma unroll
                    for (int k = 0; k < NF; ++k) f[k] = 0.0f;
                    if constexpr (STORAGE == kStorageShQ8) sh8_unpack<FULL_SH>(w, f); else sh16_unpack<FULL_SH>(w, f);
                    adjust_colour<FULL_SH>(ArrayFloats{f}, a);
                    uint32_t over;
                    if constexpr (STORAGE == kStorageShQ8) over = sh8_pack<FULL_SH>(f, w); else over = sh16_pack<FULL_SH>(f, w);
                    if (over) atomicAdd(a.n_over, over);
#pragma unroll
                    for (int k = 0; k < RW; ++k) row[k] = w[k];
                }
            }
            if (a.opacity) {
                const float t = __fmul_rn(a.opacity_scale, __uint_as_float(row[3]));
                const float alpha = t > 0.0f ? (t > 1.0f ? 1.0f : t) : 0.0f;      // (a NaN: 0) the clamp of the 8-bit targets
                row[3] = __float_as_uint(alpha);
                float S[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) S[k] = __uint_as_float(row[S0 + k]);
                p.w = footprint_bound(S, alpha);
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
