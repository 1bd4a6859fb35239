// msplat_scores.hip.h -- the score frame (msplat_render_scores, msplat_mark_scores): how much of the frame, or of a region of it, each
// splat contributes, and the compare that turns such a vector into a visibility mask
// (one of the parts of msplat_kernels.hip.h; see DESIGN.md section 4 and INTEGRATION.md 21)
#pragma once

#include "msplat_common.hip.h"
#include "msplat_composite.hip.h"
#include "msplat_ids.hip.h"

#pragma clang fp contract(off)

namespace msplat {

constexpr float kScoreOne = 8388608.0f;        // MSPLAT_SCORE_ONE (include/msplat.h): 2^23, one fully covered pixel
constexpr float kScoreStop = 5.9604644775390625e-8f;      // 2^-24: below it every later q rounds to 0

// The sum of v over the 64 lanes of the wave, the same value in every lane (readlane: wave-uniform).  Four steps inside each row of 16
// lanes (two quad permutes, two row rotations: afterwards every lane holds its row's sum), then the rows: lane 15 of rows 0 / 2 into
// rows 1 / 3, lane 31 into rows 2 and 3.  No carry can be lost: the callers' totals fit 32 bits.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);      // quad_perm [1, 0, 3, 2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);      // quad_perm [2, 3, 0, 1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);     // row_ror:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);     // row_ror:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);     // row_bcast:15 into rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);     // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ------------------------------------------------------------------------------------------
// composite_scores_kernel: per splat the sum over the window's pixels (those the region selects) of q = rint(c 2^23), c = T w as
// composite_ids_kernel defines it, and with PIXELS the number of pixels with q >= 1.  A kernel of its own beside composite_ids_kernel:
// the same items, walk, footprint test, prefetch and exponent; per pixel it carries only T (0 outside the window or the region: such a
// pixel contributes nothing and keeps no strip alive).
// Where the walk may stop: c <= T in fp32 (w <= 1), so once T <= 2^-24 every later c 2^23 <= 0.5 and rounds to 0 (ties to even):
// walking on changes nothing, and the sums do not depend on how the pixels are grouped, on the grid or on t_epsilon.
// The reduction: per surviving record each lane adds its four q (<= 2^25), the wave sums them through DPP (<= 2^31: a tile of 256
// pixels of 2^23) and lane j keeps record j's total; the hit count needs no lanes at all, it is the population of four ballots.  After
// the batch lane j looks up rank -> storage slot -> upload index like the id frame's final store and issues one 64-bit atomic add per
// (splat, tile) that scored.  Integer sums: the order of the atomics does not matter.
// ------------------------------------------------------------------------------------------
template <bool PIXELS>
__global__ __launch_bounds__(kCompThreads) void composite_scores_kernel(const uint32_t* __restrict__ tile_start, const uint32_t* __restrict__ pairs,
                                                                        const float4* __restrict__ rec, const uint32_t* __restrict__ sorted,
                                                                        const uint32_t* __restrict__ order, IdsParams p, uint32_t cap,
                                                                        uint32_t* __restrict__ queue, uint32_t nitems,
                                                                        const uint8_t* __restrict__ region, size_t region_pitch,
                                                                        unsigned long long* __restrict__ score, uint32_t* __restrict__ pixels)
{
    __shared__ float4 s_rec[(kCompThreads + 1) * 2];
    constexpr int NS = 4;                            // 16x4 strips per tile
    constexpr int ROWS = 4 * NS;
    typedef float v2f __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x;
    const int lx = lane & 15, ly = lane >> 4;
    for (uint32_t qpos = blockIdx.x; qpos < nitems;) {
    const int trow = (int)(qpos / (uint32_t)p.tiles_w);
    const int tx = p.tile_x0 + (int)(qpos - (uint32_t)trow * (uint32_t)p.tiles_w), ty = p.tile_y0 + trow;
    const int bin = (ty >> 1) * p.tiles_x + (tx >> 1);
    const int x = tx * kTile + lx, ybase = ty * kTile + ly;
    const float fx = (float)x + 0.5f;
    const float fy0 = (float)ybase + 0.5f;

    uint32_t start = tile_start[bin], end = tile_start[bin + 1];
    if (start > cap) start = cap;
    if (end > cap) end = cap;

    float T[NS];
    bool inside[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int y = ybase + 4 * k;
        inside[k] = x >= p.x0 && x < p.x1 && y >= p.y0 && y < p.y1;
        if (inside[k] && region != nullptr) inside[k] = region[(size_t)(y - p.y0) * region_pitch + (size_t)(x - p.x0)] != 0;
        T[k] = inside[k] ? 1.0f : 0.0f;
    }
    // e(u, v) = c0 + c1 u + c2 v + c3 u^2 + c4 u v + c5 v^2 in tile-centred pixel coordinates (composite_kernel)
    const float xc = (float)(tx * kTile) + 0.5f * (float)kTile, yc = (float)(ty * kTile) + 0.5f * (float)ROWS;
    const float u = fx - xc;
    v2f vp[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) vp[h] = (v2f){fy0 + 8.0f * h - yc, fy0 + 8.0f * h + 4.0f - yc};
    uint32_t alive = 0;
#pragma unroll
    for (int k = 0; k < NS; ++k) alive |= (__ballot(inside[k]) != 0ull) ? (1u << k) : 0u;

    // ranks of batch b + 2 and records of batch b + 1 are in flight while batch b is walked (composite_kernel's pipeline)
    uint32_t hiA = end;
    uint32_t cntA = min((uint32_t)kCompThreads, hiA - start);
    uint32_t rankA = 0;                                        // the RAW pair word: masked where it is used
    if (lane < (int)cntA) rankA = pairs[hiA - 1u - lane];     // j = 0 is the nearest splat
    hiA -= cntA;
    uint32_t cnt = cntA;
    float4 p0 = make_float4(0, 0, 0, 0), p1 = p0, p2 = p0;
    uint32_t prk = 0;                                          // the rank that travels with the record
    if (lane < (int)cnt) {
        uint32_t rk = rankA & kRankMask;
        asm volatile("" : "+v"(rk));              // keep the mask out of the address arithmetic (see composite_depth_kernel)
        const float4* src = rec + (size_t)rk * 3;
        p0 = src[0]; p1 = src[1]; p2 = src[2];
        prk = rk;
    }
    cntA = min((uint32_t)kCompThreads, hiA - start);
    if (lane < (int)cntA) rankA = pairs[hiA - 1u - lane];
    hiA -= cntA;
    while (cnt != 0u && alive != 0u) {
        uint32_t n;
        {
            constexpr float U = 0.5f * (float)(kTile - 1);          // box of pixel centres: |u| <= U, |v| <= Vh
            constexpr float Vh = 0.5f * (float)(ROWS - 1);
            const float a = p0.x - xc, b = p0.y - yc;               // splat centre, tile-centred
            const float qa = p0.z, qb = p0.w, qc = p1.x;            // c3, c4, c5
            const float Aa = qa * a, Bb = qb * b, Cb = qc * b, Ba = qb * a;
            const float c1 = __builtin_fmaf(-2.0f, Aa, -Bb);
            const float c2 = __builtin_fmaf(-2.0f, Cb, -Ba);
            const float c0 = __builtin_fmaf(Aa + Bb, a, __builtin_fmaf(Cb, b, p1.y));
            // y reach of the footprint against the strips that are still live (strip k: v in [4k - Vh, 4k + 3 - Vh])
            const float vlo = b - p2.w, vhi = b + p2.w;
            bool rel = lane < (int)cnt && vhi >= -Vh && vlo <= Vh;
            if (alive != (1u << NS) - 1u) {                          // wave-uniform
                bool any = false;
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    any = any || ((alive & (1u << k)) && vhi >= 4.0f * k - Vh && vlo <= 4.0f * k + 3.0f - Vh);
                rel = rel && any;
            }
            // exact footprint-vs-tile test, as in composite_kernel: the maximum of the concave quadratic over the box of pixel centres
            const bool inside_box = fabsf(a) <= U && fabsf(b) <= Vh;
            const float i2c = -0.5f * __builtin_amdgcn_rcpf(qc), i2a = -0.5f * __builtin_amdgcn_rcpf(qa);
            const float ku = __builtin_fmaf(qa, U * U, c0), kv = __builtin_fmaf(qc, Vh * Vh, c0);
            float emax;
            {
                const float lp = __builtin_fmaf(qb, U, c2), lm = __builtin_fmaf(qb, -U, c2);       // edges u = +-U
                const float kp = __builtin_fmaf(c1, U, ku), km = __builtin_fmaf(c1, -U, ku);
                const float vq = fminf(fmaxf(lp * i2c, -Vh), Vh), vm = fminf(fmaxf(lm * i2c, -Vh), Vh);
                const float ep = __builtin_fmaf(__builtin_fmaf(qc, vq, lp), vq, kp);
                const float em = __builtin_fmaf(__builtin_fmaf(qc, vm, lm), vm, km);
                const float mp = __builtin_fmaf(qb, Vh, c1), mm = __builtin_fmaf(qb, -Vh, c1);    // edges v = +-Vh
                const float hp = __builtin_fmaf(c2, Vh, kv), hm = __builtin_fmaf(c2, -Vh, kv);
                const float up = fminf(fmaxf(mp * i2a, -U), U), um = fminf(fmaxf(mm * i2a, -U), U);
                const float fp_ = __builtin_fmaf(__builtin_fmaf(qa, up, mp), up, hp);
                const float fm_ = __builtin_fmaf(__builtin_fmaf(qa, um, mm), um, hm);
                emax = fmaxf(fmaxf(ep, em), fmaxf(fp_, fm_));
            }
            rel = rel && (inside_box || emax > -8.05f);
            const uint64_t relmask = __ballot(rel);
            n = (uint32_t)__popcll(relmask);
            if (rel) {
                const int slot = __popcll(relmask & ((1ull << lane) - 1ull));      // keeps list order
                s_rec[slot * 2 + 0] = make_float4(qc, c0, c1, c2);
                s_rec[slot * 2 + 1] = make_float4(qa, qb, __builtin_bit_cast(float, prk), 0.0f);
            }
        }
        __syncthreads();
        cnt = cntA;
        if (lane < (int)cnt) {
            uint32_t rk = rankA & kRankMask;
            asm volatile("" : "+v"(rk));
            const float4* src = rec + (size_t)rk * 3;
            p0 = src[0]; p1 = src[1]; p2 = src[2];
            prk = rk;
        }
        cntA = min((uint32_t)kCompThreads, hiA - start);
        if (lane < (int)cntA) rankA = pairs[hiA - 1u - lane];
        hiA -= cntA;
        if (n != 0u) {
            uint32_t total = 0, hits = 0;     // of record `lane` of this batch
            float4 a = s_rec[0];          // c5, c0, c1, c2
            float4 b = s_rec[1];          // c3, c4, rank
            for (uint32_t j = 0; j < n; ++j) {      // (not unrolled: the wave sum is a convergent operation)
                // next record (slot n is a harmless over-read inside the 65-slot array)
                const float4 na = s_rec[(j + 1) * 2 + 0];
                const float4 nb = s_rec[(j + 1) * 2 + 1];
                const float base = __builtin_fmaf(__builtin_fmaf(b.x, u, a.z), u, a.y);      // c0 + c1 u + c3 u^2
                const float lin = __builtin_fmaf(b.y, u, a.w);                               // c2 + c4 u
                const v2f vbase = (v2f){base, base}, vlin = (v2f){lin, lin}, vC = (v2f){a.x, a.x};
                uint32_t qsum = 0, nz = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const v2f e = __builtin_elementwise_fma(vp[h], __builtin_elementwise_fma(vC, vp[h], vlin), vbase);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int k = 2 * h + i;
                        // the id frame's w: the discard is a compare, and w <= 1 -- the stop rule rests on T w <= T
                        const float w = e[i] > -8.0f ? __builtin_amdgcn_exp2f(fminf(e[i], 0.0f)) : 0.0f;
                        const float c = T[k] * w;
                        const uint32_t q = (uint32_t)__builtin_rintf(c * kScoreOne);      // exact product, nearest even
                        qsum += q;
                        if (PIXELS) nz += (uint32_t)__popcll(__ballot(q != 0u));
                        T[k] = T[k] - c;
                    }
                }
                const uint32_t s = wave_sum_u32(qsum);
                total = lane == (int)j ? s : total;
                if (PIXELS) hits = lane == (int)j ? nz : hits;
                a = na; b = nb;
            }
            if (lane < (int)n && total != 0u) {
                uint32_t rk = __builtin_bit_cast(uint32_t, s_rec[lane * 2 + 1].z) & kRankMask;
                asm volatile("" : "+v"(rk));
                uint32_t id = sorted[rk];
                if (order != nullptr) id = order[id];
                atomicAdd(&score[id], (unsigned long long)total);
                if (PIXELS) atomicAdd(&pixels[id], hits);
            }
        }
        // strips whose 64 pixels are all finished (or outside the window and the region) are finished
        uint32_t na = 0;
#pragma unroll
        for (int k = 0; k < NS; ++k) na |= (__ballot(T[k] > kScoreStop) != 0ull) ? (1u << k) : 0u;
        alive = na;
        __syncthreads();
    }

    __syncthreads();      // s_rec is reused by the next tile
    if (gridDim.x >= nitems) break;       // every work item has its own wave: nothing to pull
    uint32_t nq = 0;
    if (threadIdx.x == 0) nq = queue_next(queue, nitems);
    qpos = __builtin_amdgcn_readfirstlane(nq);
    }   // persistent tile loop
}

// mark_scores_kernel (msplat_mark_scores): one thread per splat; mask[i] = value where score[i] < threshold (at_least: >=)
__global__ __launch_bounds__(kThreads) void mark_scores_kernel(const unsigned long long* __restrict__ score, uint32_t n, bool at_least,
                                                               unsigned long long threshold, uint8_t* __restrict__ mask, uint8_t value)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if ((score[i] >= threshold) == at_least) mask[i] = value;
}

}  // namespace msplat
