// msplat_values.hip.h -- selection by attribute: what a splat IS as one float per splat (msplat_cloud_values), such an array compared
// with a closed range into a mask (msplat_mark_values) and counted into a histogram with a summary (msplat_histogram_values)
// (one of the parts of msplat_kernels.hip.h; host side: msplat_values.hip.inc; the rule: include/msplat.h)
//
// The arrays are in UPLOAD numbering (a store in Morton order: through its slot -> upload table, as mark_volume_kernel's bytes are).
// cloud_values_kernel reads the bytes its kind needs and no more: the 16-byte position entry, or single words and float4s of the
// 64-byte fp32 head every storage kind's record begins with -- FP32 records in the reference's float order, compact records in
// sh16_head_slot order.  Each lane loads the pieces of its own record: the heads of neighbouring slots are 96 to 256 bytes apart, so
// there is no run for a wave to load together; a staged load of the heads alone would address the same bytes (with the 96- and
// 160-byte strides one head in four straddles two 128-byte lines either way) and add an LDS round trip.  DESIGN.md.
#pragma once

#include "msplat_download.hip.h"
#include "msplat_rows.hip.h"

#pragma clang fp contract(off)

namespace msplat {

// mirrors MSPLAT_VALUE_* (static_asserts in msplat_values.hip.inc)
constexpr int kValueX = 0, kValueY = 1, kValueZ = 2, kValueReach2 = 3, kValueDistance2 = 4, kValueAlpha = 5, kValueRed = 6, kValueGreen = 7,
              kValueBlue = 8, kValueColourDist2 = 9, kValueScaleMin = 10, kValueScaleMid = 11, kValueScaleMax = 12, kValueKinds = 13;
// what a kind reads: the position plane; word 3 of the record; its three DC words; its nine covariance words
constexpr int kValuesOfPos = 0, kValuesOfAlpha = 1, kValuesOfColour = 2, kValuesOfScale = 3;
__host__ __device__ constexpr int values_group(int kind)
{
    return kind <= kValueDistance2 ? kValuesOfPos : (kind == kValueAlpha ? kValuesOfAlpha : (kind <= kValueColourDist2 ? kValuesOfColour : kValuesOfScale));
}

struct CloudValuesArgs {
    const float4* pos;          // the store's plane (storage order)
    const float4* recs;         // the store's records
    const uint32_t* order;      // slot -> upload index of a reordered store; nullptr: the store is in upload order
    uint32_t n;
    int kind;                   // kValue*
    float p[3];                 // param[0..2] of DISTANCE2 / COLOUR_DIST2
    float* out;                 // one float per splat, upload numbering
};

// (dx dx + dy dy) + dz dz, every operation rounded to fp32
__device__ __forceinline__ float dist2_rn(float x, float y, float z, const float* p)
{
    const float dx = __fsub_rn(x, p[0]), dy = __fsub_rn(y, p[1]), dz = __fsub_rn(z, p[2]);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// one lane per stored slot.  GROUP = values_group(kind); the position group reads no record, so the host launches it as
// <false, kStorageFp32, kValuesOfPos> for every store
template <bool FULL_SH, int STORAGE, int GROUP>
__global__ __launch_bounds__(kThreads) void cloud_values_kernel(const CloudValuesArgs a)
{
    constexpr int F4 = cloud_f4(STORAGE, FULL_SH);
    constexpr bool COMPACT = STORAGE != kStorageFp32;      // the head is words 0..15 in sh16_head_slot order
    const uint32_t slot = blockIdx.x * kThreads + threadIdx.x;
    if (slot >= a.n) return;
    const float4* rec4 = a.recs + (size_t)slot * F4;
    const float* rec = reinterpret_cast<const float*>(rec4);
    float v;
    if constexpr (GROUP == kValuesOfPos) {
        const float4 p = a.pos[slot];
        v = a.kind == kValueX ? p.x : (a.kind == kValueY ? p.y : (a.kind == kValueZ ? p.z : p.w));
        if (a.kind == kValueDistance2) v = dist2_rn(p.x, p.y, p.z, a.p);
    } else if constexpr (GROUP == kValuesOfAlpha) {
        v = rec[3];
    } else if constexpr (GROUP == kValuesOfColour) {
        float dc[3];
        if constexpr (COMPACT) {
            const float4 q = rec4[1];                       // words 4..7: DC r g b, S[0]
            dc[0] = q.x; dc[1] = q.y; dc[2] = q.z;
        } else {
            dc[0] = rec[4]; dc[1] = rec[8]; dc[2] = rec[12];
        }
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = __fadd_rn(0.5f, __fmul_rn(0.28209479177387814f, dc[k]));
        v = a.kind == kValueRed ? c[0] : (a.kind == kValueGreen ? c[1] : c[2]);
        if (a.kind == kValueColourDist2) v = dist2_rn(c[0], c[1], c[2], a.p);
    } else {
        float S[9], evec[9], eval[3];
        if constexpr (COMPACT) {
            const float4 q0 = rec4[2], q1 = rec4[3];        // words 8..15: S[1..8]
            S[0] = rec[7];
            S[1] = q0.x; S[2] = q0.y; S[3] = q0.z; S[4] = q0.w; S[5] = q1.x; S[6] = q1.y; S[7] = q1.z; S[8] = q1.w;
        } else {
            const float4 q0 = rec4[4], q1 = rec4[5];        // floats 16..23
            S[0] = q0.x; S[1] = q0.y; S[2] = q0.z; S[3] = q0.w; S[4] = q1.x; S[5] = q1.y; S[6] = q1.z; S[7] = q1.w;
            S[8] = rec[24];
        }
        jacobi_eigen3(S, evec, eval);
        const float e = a.kind == kValueScaleMin ? eval[0] : (a.kind == kValueScaleMid ? eval[1] : eval[2]);
        // sqrtf(max(e, 0.0f)), IEEE: the double root of a float, rounded to fp32, is the correctly rounded fp32 root (53 >= 2 * 24 + 2)
        v = (float)sqrt((double)(e < 0.0f ? 0.0f : e));     // (a NaN stays, as in egress_vertex)
    }
    a.out[a.order ? a.order[slot] : slot] = v;
}

// one lane per value: 4 bytes read, at most one written.  inside = lo <= v <= hi (a NaN is never inside); outside != 0 marks the others
__global__ __launch_bounds__(kThreads) void mark_values_kernel(const float* __restrict__ values, uint32_t n, float lo, float hi, int outside,
                                                               uint8_t* __restrict__ mask, uint8_t value)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float v = values[i];
    if ((v >= lo && v <= hi) != (outside != 0)) mask[i] = value;
}

// ---- msplat_histogram_values.  The counts are integers added with integer atomics, the minimum and maximum go through the row
// reduction of msplat_rows.hip.h like the measure's (no floating-point atomic): nothing depends on the grid or on any order.
struct ValueRow {                       // what a lane, a wave, a workgroup and the whole array accumulate
    uint32_t selected, finite, nan, below, above;
    float vmin, vmax;
    uint32_t pad;

    __host__ __device__ __forceinline__ void clear()
    {
        selected = finite = nan = below = above = pad = 0u;
        vmin = INFINITY;
        vmax = -INFINITY;
    }
    __device__ __forceinline__ void merge(const ValueRow& o)
    {
        selected += o.selected; finite += o.finite; nan += o.nan; below += o.below; above += o.above;
        vmin = fminf(vmin, o.vmin);
        vmax = fmaxf(vmax, o.vmax);
    }
};

// grid-stride over the values in turns of the whole workgroup (every wave stays whole: the ballots below count its 64 lanes).
// bins > 0: s_bins is the workgroup's histogram (dynamic LDS, bins words), flushed into `counts` (zeroed by the host) where nonzero.
// A wave whose binned lanes all hit one bin adds their number once: an array of equal values costs one LDS atomic per wave and turn
__global__ __launch_bounds__(kThreads) void histogram_values_kernel(const float* __restrict__ values, const uint8_t* __restrict__ select,
                                                                    uint32_t n, float lo, float hi, float scale, uint32_t bins,
                                                                    uint32_t* __restrict__ counts, ValueRow* __restrict__ part /* [gridDim.x] */)
{
    extern __shared__ uint32_t s_bins[];
    for (uint32_t b = threadIdx.x; b < bins; b += kThreads) s_bins[b] = 0u;
    __syncthreads();
    ValueRow r;
    r.clear();
    const float fbins = (float)bins;
    for (uint32_t base = blockIdx.x * kThreads; base < n; base += gridDim.x * kThreads) {
        const uint32_t i = base + threadIdx.x;
        bool binned = false;
        uint32_t b = 0u;
        if (i < n && (!select || select[i] != 0)) {
            const float v = values[i];
            r.selected += 1u;
            if (v != v) {
                r.nan += 1u;
            } else {
                if (isfinite(v)) {
                    r.finite += 1u;
                    r.vmin = fminf(r.vmin, v);
                    r.vmax = fmaxf(r.vmax, v);
                }
                if (bins) {
                    if (v < lo) r.below += 1u;
                    else if (v > hi) r.above += 1u;
                    else {
                        const float t = __fmul_rn(__fsub_rn(v, lo), scale);
                        b = t >= fbins ? bins - 1u : (uint32_t)t;
                        binned = true;
                    }
                }
            }
        }
        if (bins) {
            const unsigned long long act = __ballot(binned);
            if (act) {
                const int first = __ffsll((long long)act) - 1;
                const uint32_t b0 = __shfl(b, first, 64);
                if (__ballot(binned && b == b0) == act) {
                    if ((int)(threadIdx.x & 63) == first) atomicAdd(&s_bins[b0], (uint32_t)__popcll(act));
                } else if (binned) {
                    atomicAdd(&s_bins[b], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < bins; b += kThreads) {
        const uint32_t c = s_bins[b];
        if (c) atomicAdd(&counts[b], c);
    }
    row_reduce_store(r, part + blockIdx.x);
}

}  // namespace msplat
