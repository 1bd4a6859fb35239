// msplat_overlay.hip.h -- the render-time overlay (msplat_set_overlay*, msplat_set_overlay_palette): a class byte per splat and a palette
// of up to 256 RGBA entries tint the colour project_kernel left in each splat's record, before the compositor reads it
// (one of the parts of msplat_kernels.hip.h; see DESIGN.md section 4 and INTEGRATION.md 26)
#pragma once

#include "msplat_common.hip.h"

#pragma clang fp contract(off)

namespace msplat {

constexpr int kOverlayEntries = 256;       // palette entries on the device: those beyond the caller's count hold a = 0 (no effect)
static_assert(kOverlayEntries == kThreads, "overlay_kernel: one palette entry per thread of a workgroup");

// overlay_classes_kernel: the classes in STORAGE order, once per change of the classes or of the store's order.  A cloud stored in Morton
// order is sorted by storage slot (sorted_idx holds slots) while the caller's classes speak upload numbering: cls_slot[s] = cls[order[s]],
// so that the per-frame kernel gathers one byte per rank, not an index and then a byte.
__global__ __launch_bounds__(kThreads) void overlay_classes_kernel(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ order,
                                                                   uint32_t n, uint8_t* __restrict__ cls_slot)
{
    for (uint32_t s = blockIdx.x * kThreads + threadIdx.x; s < n; s += gridDim.x * kThreads) cls_slot[s] = cls[order[s]];
}

// overlay_kernel: one lane per draw-order rank, right behind the frame's projection.  Rank r's splat (storage slot sorted_idx[r]) has
// class k = cls_slot[slot]; with (h_r, h_g, h_b, a) = palette[k] and a != 0 each colour lane c of its 48-byte record -- r1.z, r1.w,
// r2.x, dwords 6..8 -- becomes
//     t = 1.0f - a;   c' = (t * c) + (a * h)
// every operation rounded to fp32, nothing fused.  A rank with a == 0 is neither read nor written (its bits stay, a NaN included), and a
// wave without a tinted rank touches no record at all: a selection of a few per cent costs the index and class reads.  Position, conic,
// alpha, extents, the rectangle and z_w are not touched, so the lists, `drawn`, `pairs` and the depth plane are the plain frame's.
// EVERY rank of the frame is tinted, also one whose rectangle is empty (it reaches no pixel; leaving it out would cost a fourth read).
// Ranks: [0, V), V read from the word the projection read; two views in one chain (two_views != 0): [0, V) and [V1, V1 + V) with
// V1 = V rounded up to 64 (project_kernel's PROJ_TWO_VIEWS), both views' rank r - V1 being splat sorted_idx[r - V1]; the gap is untouched.
// The palette (4 KB, kOverlayEntries float4) goes into LDS once per workgroup, one entry per thread; the loop is grid-stride.
__global__ __launch_bounds__(kThreads) void overlay_kernel(const uint32_t* __restrict__ sorted_idx, const uint32_t* __restrict__ d_V,
                                                           const uint8_t* __restrict__ cls_slot, const float4* __restrict__ palette,
                                                           float* __restrict__ rec, uint32_t two_views)
{
    __shared__ float4 s_pal[kOverlayEntries];
    s_pal[threadIdx.x] = palette[threadIdx.x];
    __syncthreads();
    const uint32_t V = *d_V;
    const uint32_t V1 = two_views ? (V + 63u) & ~63u : 0u;
    const uint32_t total = V1 + V;
    for (uint32_t r0 = blockIdx.x * kThreads; r0 < total; r0 += gridDim.x * kThreads) {
        const uint32_t r = r0 + threadIdx.x;
        const uint32_t rl = r >= V1 ? r - V1 : r;          // rank inside its view
        if (r >= total || rl >= V) continue;               // past the end, or the gap between the views
        const float4 h = s_pal[cls_slot[sorted_idx[rl]]];
        if (h.w != 0.0f) {
            const float t = __fsub_rn(1.0f, h.w);
            float* c = rec + (size_t)r * 12 + 6;
            const float c0 = c[0], c1 = c[1], c2 = c[2];
            c[0] = __fadd_rn(__fmul_rn(t, c0), __fmul_rn(h.w, h.x));
            c[1] = __fadd_rn(__fmul_rn(t, c1), __fmul_rn(h.w, h.y));
            c[2] = __fadd_rn(__fmul_rn(t, c2), __fmul_rn(h.w, h.z));
        }
    }
}

}  // namespace msplat
