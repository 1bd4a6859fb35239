// msplat_select.hip.h -- selection by position (msplat_mark_volume, msplat_mark_view) and where a selection is (msplat_measure_cloud):
// three functions of the store's 16-byte position plane.  The marks write one byte per selected splat into the caller's mask in
// UPLOAD numbering (a store in Morton order: through its slot -> upload table); the measure reads such a mask.  None of them is part
// of a frame: no Sort is needed and nothing of the context changes.  (Included by msplat_kernels.hip.h after msplat_cloud.hip.h,
// whose crop_inside is the rule of the volume mark, and msplat_rows.hip.h, whose row reduction the measure is.)
#pragma once

#include "msplat_cloud.hip.h"
#include "msplat_rows.hip.h"

namespace msplat {

struct MarkVolumeArgs {
    const float4* pos;          // the store's plane (storage order)
    const uint32_t* order;      // slot -> upload index of a reordered store; nullptr: the store is in upload order
    uint32_t n;
    int shape;                  // MSPLAT_CROP_BOX / _SPHERE, | MSPLAT_CROP_INVERT
    float m[16];                // world -> volume, column-major; row 3 is not read
    uint8_t* mask;              // one byte per splat, upload numbering
    uint8_t value;
};

// one lane per stored slot: 16 (+ 4) bytes read, one byte written where the crop rule holds.  The byte stores of a reordered store
// are scattered over upload numbers, as visibility_kernel's mask reads are
__global__ __launch_bounds__(kThreads) void mark_volume_kernel(const MarkVolumeArgs a)
{
    const uint32_t slot = blockIdx.x * kThreads + threadIdx.x;
    if (slot >= a.n) return;
    const float4 p = a.pos[slot];
    if (crop_inside(p, a.m, a.shape) != ((a.shape & kCropInvert) != 0)) a.mask[a.order ? a.order[slot] : slot] = a.value;
}

struct MarkViewArgs {
    const float4* pos;
    const uint32_t* order;
    uint32_t n;
    float mvp[16];              // projMat * inverse(cameraMat): FrameParams::mvp of a Sort with the same arguments
    float W, H;                 // viewport[2], viewport[3]
    float x0, y0, x1, y1;       // the window: x0 <= cx < x1, y0 <= cy < y1 (integers up to 8192: exact)
    const uint8_t* region;      // one byte per pixel of the window, nonzero = selects; nullptr: every pixel
    size_t region_pitch;
    uint8_t* mask;
    uint8_t value;
};

// select through: the centre's pixel, cull_key's operations up to xx and yy (bit for bit the Sort's), then the viewport transform of
// msplat.h.  A NaN fails every comparison; cx and cy are converted to int only once they are known to lie inside the window
__global__ __launch_bounds__(kThreads) void mark_view_kernel(const MarkViewArgs a)
{
    const uint32_t slot = blockIdx.x * kThreads + threadIdx.x;
    if (slot >= a.n) return;
    const float4 p = a.pos[slot];
    const float* m = a.mvp;
    const float px = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], p.x), __fmul_rn(m[4], p.y)), __fmul_rn(m[8], p.z)), m[12]);
    const float py = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[1], p.x), __fmul_rn(m[5], p.y)), __fmul_rn(m[9], p.z)), m[13]);
    const float pw = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[3], p.x), __fmul_rn(m[7], p.y)), __fmul_rn(m[11], p.z)), m[15]);
    const float depth = pw;
    const float xx = __fdiv_rn(px, depth);
    const float yy = __fdiv_rn(py, depth);
    const float cx = __fmul_rn(0.5f, __fadd_rn(a.W, __fmul_rn(xx, a.W)));
    const float cy = __fmul_rn(0.5f, __fadd_rn(a.H, __fmul_rn(yy, a.H)));
    if (!(depth > 0.0f && cx >= a.x0 && cx < a.x1 && cy >= a.y0 && cy < a.y1)) return;
    if (a.region) {
        const uint32_t col = (uint32_t)((int)cx - (int)a.x0), row = (uint32_t)((int)cy - (int)a.y0);
        if (a.region[(size_t)row * a.region_pitch + col] == 0) return;
    }
    a.mask[a.order ? a.order[slot] : slot] = a.value;
}

// ---- msplat_measure_cloud: count, AABB, largest footprint bound and the first and second moments of the selected centres.  A row
// reduction (msplat_rows.hip.h): no atomics and a summation order fixed by the grid, so a call repeated on a context returns the
// same bytes.  The counts, the box and the bound do not depend on any order.
constexpr int kMeasureSums = 9;         // x y z, xx yy zz xy xz yz
struct MeasureRow {                     // what a lane, a wave, a workgroup and the whole cloud accumulate
    double s[kMeasureSums];
    float lo[3], hi[3];
    float reach;
    uint32_t selected, finite;          // (a cloud holds at most 2^24 splats)

    __host__ __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int k = 0; k < kMeasureSums; ++k) s[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
        reach = 0.0f;
        selected = finite = 0u;
    }
    __device__ __forceinline__ void merge(const MeasureRow& o)
    {
#pragma unroll
        for (int k = 0; k < kMeasureSums; ++k) s[k] += o.s[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], o.lo[k]); hi[k] = fmaxf(hi[k], o.hi[k]); }
        reach = fmaxf(reach, o.reach);
        selected += o.selected;
        finite += o.finite;
    }
};

// grid-stride over the stored slots; part: one row per workgroup
__global__ __launch_bounds__(kThreads) void measure_cloud_kernel(const float4* __restrict__ pos, const uint32_t* __restrict__ order,
                                                                 const uint8_t* __restrict__ select, uint32_t n,
                                                                 MeasureRow* __restrict__ part /* [gridDim.x] */)
{
    MeasureRow r;
    r.clear();
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        if (select && select[order ? order[i] : i] == 0) continue;
        const float4 p = pos[i];
        r.selected += 1u;
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
            r.finite += 1u;
            r.lo[0] = fminf(r.lo[0], p.x); r.lo[1] = fminf(r.lo[1], p.y); r.lo[2] = fminf(r.lo[2], p.z);
            r.hi[0] = fmaxf(r.hi[0], p.x); r.hi[1] = fmaxf(r.hi[1], p.y); r.hi[2] = fmaxf(r.hi[2], p.z);
            if (p.w > r.reach && isfinite(p.w)) r.reach = p.w;               // (NaN never wins)
            const double x = p.x, y = p.y, z = p.z;                          // (a product of two floats is exact in double)
            r.s[0] += x; r.s[1] += y; r.s[2] += z;
            r.s[3] += x * x; r.s[4] += y * y; r.s[5] += z * z;
            r.s[6] += x * y; r.s[7] += x * z; r.s[8] += y * z;
        }
    }
    row_reduce_store(r, part + blockIdx.x);
}

}  // namespace msplat
