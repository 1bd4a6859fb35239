// msplat_ids.hip.h -- the id frame (msplat_render_ids, msplat_mark_ids): which splat each pixel shows, and the scatter that turns a
// region of that plane into a visibility mask
// (one of the parts of msplat_kernels.hip.h; see DESIGN.md section 4 and INTEGRATION.md 20)
#pragma once

#include "msplat_common.hip.h"
#include "msplat_composite.hip.h"

#pragma clang fp contract(off)

namespace msplat {

constexpr uint32_t kIdNone = 0xFFFFFFFFu;      // MSPLAT_ID_NONE (include/msplat.h)

// The window of the viewport an id frame writes, and the 16x16 tiles that intersect it (work item i = tile (tile_x0 + i % tiles_w,
// tile_y0 + i / tiles_w)).  Pixel (x, y) of the viewport goes to row y - y0, column x - x0 of the planes.
struct IdsParams {
    int tiles_x;                      // bins per row of the frame (FrameParams::tiles_x)
    int x0, y0, x1, y1;               // the window, [x0, x1) x [y0, y1), inside the viewport
    int tile_x0, tile_y0, tiles_w;
};

// ------------------------------------------------------------------------------------------
// composite_ids_kernel: per pixel the splat with the largest contribution c_i = T_i w_i, T_i = prod_{j nearer}(1 - w_j), w as
// splat_frag.glsl:18-42 defines it (0 where the shader discards).  A kernel of its own beside composite_kernel, which is tuned to its
// register budget: the same wave layout (one wave per 16x16 tile, lane (lx, ly) owns pixels (x0 + lx, y0 + 4k + ly), k = 0..3, one per
// 16x4 strip), the same walk (the bin's list near to far in batches of 64, the exact footprint-versus-tile test, survivors compacted
// into LDS in list order, the same three-stage prefetch of pair words and records), the same polynomial form of the exponent in
// tile-centred coordinates -- without the exponent bias: the discard is a compare here, and the wave keeps the default float mode.
// Per pixel it carries T, the best contribution so far and that splat's rank: 12 registers, no colour.
// Where the walk may stop: every later contribution is at most the current T (w <= 1: the exponent is clamped to 0, and T w <= T in
// fp32), and T never grows, so a pixel with T <= best and best > 0 is finished -- under the strict `>` below no later splat can
// replace its answer.  A strip is finished when its 64 pixels are (or lie outside the window), a tile when its strips are.  The rule
// is exact in the kernel's own arithmetic: walking on changes nothing, so the plane does not depend on how the pixels are grouped,
// on the grid or on t_epsilon, which the kernel never sees.
// The final store looks up rank -> storage slot (`sorted`, the Sort's index list), storage slot -> upload index (`order`, NULL for
// a cloud stored in upload order) and zw[rank], the window depth project_kernel leaves per rank.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void composite_ids_kernel(const uint32_t* __restrict__ tile_start, const uint32_t* __restrict__ pairs,
                                                                     const float4* __restrict__ rec, const float* __restrict__ zw,
                                                                     const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ order,
                                                                     IdsParams p, uint32_t cap, uint32_t* __restrict__ queue, uint32_t nitems,
                                                                     uint32_t* __restrict__ ids, size_t ids_pitch,
                                                                     float* __restrict__ id_depth, size_t depth_pitch)
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

    float T[NS], best[NS];
    uint32_t brank[NS];
    bool inside[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        T[k] = 1.0f; best[k] = 0.0f; brank[k] = 0u;
        inside[k] = x >= p.x0 && x < p.x1 && ybase + 4 * k >= p.y0 && ybase + 4 * k < p.y1;
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
            float4 a = s_rec[0];          // c5, c0, c1, c2
            float4 b = s_rec[1];          // c3, c4, rank
#pragma unroll 2
            for (uint32_t j = 0; j < n; ++j) {
                // next record (slot n is a harmless over-read inside the 65-slot array)
                const float4 na = s_rec[(j + 1) * 2 + 0];
                const float4 nb = s_rec[(j + 1) * 2 + 1];
                const float base = __builtin_fmaf(__builtin_fmaf(b.x, u, a.z), u, a.y);      // c0 + c1 u + c3 u^2
                const float lin = __builtin_fmaf(b.y, u, a.w);                               // c2 + c4 u
                const v2f vbase = (v2f){base, base}, vlin = (v2f){lin, lin}, vC = (v2f){a.x, a.x};
                const uint32_t rk = __builtin_bit_cast(uint32_t, b.z);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const v2f e = __builtin_elementwise_fma(vp[h], __builtin_elementwise_fma(vC, vp[h], vlin), vbase);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int k = 2 * h + i;
                        // splat_frag.glsl:37-40 discard: w = exp2(e) > 1/256  <=>  e > -8; w <= 1 (alpha <= 1): the rounding of e must not
                        // lift it above, the stop rule rests on T w <= T
                        const float w = e[i] > -8.0f ? __builtin_amdgcn_exp2f(fminf(e[i], 0.0f)) : 0.0f;
                        const float c = T[k] * w;
                        const bool better = c > best[k];      // strict: of equal contributions the nearest splat keeps the pixel
                        best[k] = better ? c : best[k];
                        brank[k] = better ? rk : brank[k];
                        T[k] = T[k] - c;
                    }
                }
                a = na; b = nb;
            }
        }
        // strips whose 64 pixels are all finished (or outside the window) are finished
        uint32_t na = 0;
#pragma unroll
        for (int k = 0; k < NS; ++k)
            na |= (__ballot(inside[k] && !(best[k] > 0.0f && T[k] <= best[k])) != 0ull) ? (1u << k) : 0u;
        alive = na;
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < NS; ++k) {
        if (inside[k]) {
            uint32_t id = kIdNone;
            float z = 1.0f;
            if (best[k] > 0.0f) {
                uint32_t rk = brank[k] & kRankMask;
                asm volatile("" : "+v"(rk));
                id = sorted[rk];
                if (order != nullptr) id = order[id];
                if (id_depth != nullptr) z = zw[rk];
            }
            const size_t row = (size_t)(ybase + 4 * k - p.y0);
            ((uint32_t*)((char*)ids + row * ids_pitch))[x - p.x0] = id;
            if (id_depth != nullptr) ((float*)((char*)id_depth + row * depth_pitch))[x - p.x0] = z;
        }
    }
    __syncthreads();      // s_rec is reused by the next tile
    if (gridDim.x >= nitems) break;       // every work item has its own wave: nothing to pull
    uint32_t nq = 0;
    if (threadIdx.x == 0) nq = queue_next(queue, nitems);
    qpos = __builtin_amdgcn_readfirstlane(nq);
    }   // persistent tile loop
}

// mark_ids_kernel (msplat_mark_ids): one thread per pixel of a w x h id plane; mask[id] = value for every pixel the region selects
// (NULL: all) whose id is a splat of the cloud.  Plain byte stores: colliding writers store the same value.
__global__ __launch_bounds__(kThreads) void mark_ids_kernel(const uint32_t* __restrict__ ids, size_t ids_pitch, uint32_t w, uint32_t h,
                                                            const uint8_t* __restrict__ region, size_t region_pitch,
                                                            uint8_t* __restrict__ mask, uint32_t n, uint8_t value)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (uint64_t)w * h) return;
    const uint32_t y = (uint32_t)(i / w), x = (uint32_t)(i - (uint64_t)y * w);
    if (region != nullptr && region[(size_t)y * region_pitch + x] == 0) return;
    const uint32_t id = ((const uint32_t*)((const char*)ids + (size_t)y * ids_pitch))[x];
    if (id < n) mask[id] = value;      // MSPLAT_ID_NONE and any id beyond the cloud: skipped
}

}  // namespace msplat
