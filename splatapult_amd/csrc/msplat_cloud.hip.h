// msplat_cloud.hip.h -- upload-time kernels: GPU PLY ingest (GaussianCloud::ImportPly's per-vertex math) from a vertex block or from
// attribute arrays, the repack of interleaved records that are on the device, and the spatial storage order (moments, Morton codes,
// gather, cull boxes)
// (one of the parts of msplat_kernels.hip.h)
#pragma once

#include "msplat_common.hip.h"

#pragma clang fp contract(off)

namespace msplat {

// ------------------------------------------------------------------------------------------
// GPU ingest: GaussianCloud::ImportPly's per-vertex lambda (gaussiancloud.cpp:254-361)
//   alpha = 1/(1+exp(-opacity)), scale = exp(log scale), Sigma = R S S^T R^T from the normalised quaternion,
//   SH repack -- written straight into the renderer's device layout (pos4 + padded records).
// One wave per 64 vertices: their bytes are contiguous in the PLY vertex block, so the wave copies the span
// with coalesced 16-byte loads into LDS and every lane then picks its properties out of its own vertex.
// Same operation order as the host code (splatapult_amd/host/gaussian_scene.cpp), contraction off.
// ------------------------------------------------------------------------------------------
struct PlyLayout {             // mirrors msplat_ply_layout (include/msplat.h)
    uint32_t vertex_size;
    int32_t x, y, z;
    int32_t f_dc[3];
    int32_t f_rest[45];
    int32_t opacity;
    int32_t scale[3];
    int32_t rot[4];
};

// One record out of the wave's hands: the FP32 record floats f[] (padded, reference float order) -> pos4[i] and recs[i].
// STORAGE = kStorageShFp16 / kStorageShQ8: the records are written compact (msplat_common.hip.h: sh16_pack / sh8_pack); *n_over
// counts the f_rest values beyond the fp16 range / the non-finite ones (the upload then fails)
template <bool FULL_SH, int STORAGE>
__device__ __forceinline__ void store_record(const float* f, uint64_t i, float4* __restrict__ pos4, float4* __restrict__ recs,
                                             uint32_t* __restrict__ n_over)
{
    constexpr int F4 = FULL_SH ? 16 : 8;
    pos4[i] = make_float4(f[0], f[1], f[2], footprint_bound(&f[16], f[3]));      // .w: world-space footprint bound for the band cull
    if constexpr (STORAGE != kStorageFp32) {
        constexpr int CF4 = cloud_f4(STORAGE, FULL_SH);
        uint32_t w[CF4 * 4];
        uint32_t over;
        if constexpr (STORAGE == kStorageShQ8) over = sh8_pack<FULL_SH>(f, w); else over = sh16_pack<FULL_SH>(f, w);
        if (over) atomicAdd(n_over, over);
#pragma unroll
        for (int k = 0; k < CF4; ++k)
            recs[i * CF4 + k] = make_float4(__uint_as_float(w[4 * k]), __uint_as_float(w[4 * k + 1]), __uint_as_float(w[4 * k + 2]),
                                            __uint_as_float(w[4 * k + 3]));
    } else {
#pragma unroll
        for (int k = 0; k < F4; ++k) recs[i * F4 + k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
    }
}

// ImportPly's per-vertex math on vertex i, behind both ingest kernels.  `rd` hands out the vertex's properties by name:
// rd.pos(c), rd.f_dc(c), rd.f_rest(k) (PLY order f_rest_0..44; asked for with FULL_SH only), rd.opacity(), rd.scale(c), rd.rot(c) (w x y z)
template <bool FULL_SH, int STORAGE, class Reader>
__device__ __forceinline__ void ingest_vertex(const Reader& rd, uint64_t i, float4* __restrict__ pos4, float4* __restrict__ recs,
                                              uint32_t* __restrict__ n_over)
{
    constexpr int F4 = FULL_SH ? 16 : 8;
    float f[F4 * 4];
#pragma unroll
    for (int k = 0; k < F4 * 4; ++k) f[k] = 0.0f;
    f[0] = rd.pos(0); f[1] = rd.pos(1); f[2] = rd.pos(2);
    f[3] = 1.0f / (1.0f + expf(-rd.opacity()));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f[4 + 4 * c] = rd.f_dc(c);
        if constexpr (FULL_SH) {
#pragma unroll
            for (int k = 1; k < 4; ++k) f[4 + 4 * c + k] = rd.f_rest(c * 15 + k - 1);
#pragma unroll
            for (int k = 4; k < 16; ++k) f[25 + 12 * c + (k - 4)] = rd.f_rest(c * 15 + k - 1);
        }
    }
    const float s0 = expf(rd.scale(0)), s1 = expf(rd.scale(1)), s2 = expf(rd.scale(2));
    float w = rd.rot(0), x = rd.rot(1), y = rd.rot(2), z = rd.rot(3);
    const float len = sqrtf((w * w + x * x) + (y * y + z * z));
    if (len <= 0.0f) { w = 1.0f; x = 0.0f; y = 0.0f; z = 0.0f; }
    else { const float inv = 1.0f / len; w *= inv; x *= inv; y *= inv; z *= inv; }
    const float xx = x * x, yy = y * y, zz = z * z, xz = x * z, xy = x * y, yz = y * z;
    const float wx = w * x, wy = w * y, wz = w * z;
    // R[c][r], column-major like the host code
    const float R[9] = {1.0f - 2.0f * (yy + zz), 2.0f * (xy + wz),        2.0f * (xz - wy),
                        2.0f * (xy - wz),        1.0f - 2.0f * (xx + zz), 2.0f * (yz + wx),
                        2.0f * (xz + wy),        2.0f * (yz - wx),        1.0f - 2.0f * (xx + yy)};
    const float sc[3] = {s0, s1, s2};
    float B[9];      // (R S) S^T : column c scaled by s_c twice (the zero terms of the 3x3 products add exactly)
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) B[c * 3 + r] = (R[c * 3 + r] * sc[c]) * sc[c];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            // V[c][r] = B[0][r]*Rt[c][0] + B[1][r]*Rt[c][1] + B[2][r]*Rt[c][2],  Rt[c][k] = R[k][c]
            float s = B[0 * 3 + r] * R[0 * 3 + c];
            s = s + B[1 * 3 + r] * R[1 * 3 + c];
            s = s + B[2 * 3 + r] * R[2 * 3 + c];
            f[16 + c * 3 + r] = s;
        }
    store_record<FULL_SH, STORAGE>(f, i, pos4, recs, n_over);
}

// the wave's span of `span` bytes (a multiple of 4; src 16-byte aligned) into LDS with coalesced 16-byte loads; the sub-16-byte
// tail of the last block goes word by word
__device__ __forceinline__ void stage_span(char* __restrict__ dst, const char* __restrict__ src, uint32_t span, int lane)
{
    for (uint32_t off = lane * 16u; off < span; off += 64u * 16u) {
        if (off + 16u <= span) {
            *reinterpret_cast<float4*>(dst + off) = *reinterpret_cast<const float4*>(src + off);
        } else {
            for (uint32_t o = off; o < span; o += 4u)
                *reinterpret_cast<float*>(dst + o) = *reinterpret_cast<const float*>(src + o);
        }
    }
}

struct PlyVertexReader {       // one vertex of the block in LDS; an absent property (offset -1) reads as 0, like BinaryAttribute::Read
    const char* v;
    const PlyLayout& L;
    __device__ __forceinline__ float rd(int32_t off) const { return off >= 0 ? *reinterpret_cast<const float*>(v + off) : 0.0f; }
    __device__ __forceinline__ float pos(int c) const { return rd(c == 0 ? L.x : (c == 1 ? L.y : L.z)); }
    __device__ __forceinline__ float f_dc(int c) const { return rd(L.f_dc[c]); }
    __device__ __forceinline__ float f_rest(int k) const { return rd(L.f_rest[k]); }
    __device__ __forceinline__ float opacity() const { return rd(L.opacity); }
    __device__ __forceinline__ float scale(int c) const { return rd(L.scale[c]); }
    __device__ __forceinline__ float rot(int c) const { return rd(L.rot[c]); }
};

template <bool FULL_SH, int STORAGE = kStorageFp32>
__global__ __launch_bounds__(64) void ingest_kernel(const char* __restrict__ raw, uint64_t n, PlyLayout L,
                                                    float4* __restrict__ pos4, float4* __restrict__ recs,
                                                    uint32_t* __restrict__ n_over)
{
    extern __shared__ __attribute__((aligned(16))) char s_raw[];
    const int lane = threadIdx.x;
    const uint32_t vs = L.vertex_size;
    const uint64_t v0 = (uint64_t)blockIdx.x * 64u;
    const uint64_t byte0 = v0 * vs;
    const uint64_t total = n * (uint64_t)vs;
    const uint32_t span = (uint32_t)min((uint64_t)64u * vs, total - byte0);      // multiple of 4
    stage_span(s_raw, raw + byte0, span, lane);
    __syncthreads();
    const uint64_t i = v0 + lane;
    if (i >= n) return;
    ingest_vertex<FULL_SH, STORAGE>(PlyVertexReader{s_raw + (size_t)lane * vs, L}, i, pos4, recs, n_over);
}

// The same record from six attribute arrays in device memory (msplat_upload_attributes_device; the arrays of
// msplat_cloud_from_attributes).  Only 4-byte alignment is assumed.  One wave per 64 splats: xyz, f_dc, opacity, scale and rot are
// 14 floats a splat, read by the lane that owns it (a wave's loads cover one contiguous run per array); the 64 x 45 floats of f_rest
// are one contiguous 11.25-KB run, staged through LDS with one dword per lane and step (256 B per load instruction), and read back
// at a stride of 45 words -- odd, so the 64 lanes hit 64 different banks.
struct AttrArrays {
    const float* xyz; const float* f_dc; const float* f_rest; const float* opacity; const float* log_scale; const float* rot;
};

struct AttrReader {
    const AttrArrays& A;
    uint64_t i;
    const float* rest;         // the splat's 45 floats in LDS (FULL_SH only)
    __device__ __forceinline__ float pos(int c) const { return A.xyz[i * 3 + c]; }
    __device__ __forceinline__ float f_dc(int c) const { return A.f_dc[i * 3 + c]; }
    __device__ __forceinline__ float f_rest(int k) const { return rest[k]; }
    __device__ __forceinline__ float opacity() const { return A.opacity[i]; }
    __device__ __forceinline__ float scale(int c) const { return A.log_scale[i * 3 + c]; }
    __device__ __forceinline__ float rot(int c) const { return A.rot[i * 4 + c]; }
};

template <bool FULL_SH, int STORAGE = kStorageFp32>
__global__ __launch_bounds__(64) void ingest_attributes_kernel(AttrArrays A, uint64_t n, float4* __restrict__ pos4,
                                                               float4* __restrict__ recs, uint32_t* __restrict__ n_over)
{
    __shared__ float s_rest[FULL_SH ? 64 * 45 : 1];
    const int lane = threadIdx.x;
    const uint64_t v0 = (uint64_t)blockIdx.x * 64u;
    if constexpr (FULL_SH) {
        const uint32_t words = (uint32_t)min((uint64_t)64u, n - v0) * 45u;
        const float* src = A.f_rest + v0 * 45u;
        for (uint32_t o = lane; o < words; o += 64u) s_rest[o] = src[o];
        __syncthreads();
    }
    const uint64_t i = v0 + lane;
    if (i >= n) return;
    ingest_vertex<FULL_SH, STORAGE>(AttrReader{A, i, s_rest + (FULL_SH ? lane * 45 : 0)}, i, pos4, recs, n_over);
}

// Interleaved records in device memory (msplat_upload_cloud_device): n records of `stride` bytes (a multiple of 4, base 16-byte
// aligned) with the attributes at the byte offsets of msplat_attr_offsets -> pos4 + the padded (or compact) records, the host
// loop of msplat_upload_cloud field by field.  The ingest kernel's shape: one wave per 64 records, their span copied into dynamic
// LDS (64 * stride bytes), each lane then picks its attributes out of its own record.
struct AttrOffsets {           // mirrors msplat_attr_offsets (include/msplat.h)
    uint32_t pos_with_alpha, r_sh0, g_sh0, b_sh0;
    uint32_t cov3_col0, cov3_col1, cov3_col2;
    uint32_t sh_full[9];       // r_sh1 r_sh2 r_sh3 g_sh1 .. b_sh3
};

template <bool FULL_SH, int STORAGE = kStorageFp32>
__global__ __launch_bounds__(64) void repack_kernel(const char* __restrict__ aos, uint64_t n, uint32_t stride, AttrOffsets O,
                                                    float4* __restrict__ pos4, float4* __restrict__ recs,
                                                    uint32_t* __restrict__ n_over)
{
    extern __shared__ __attribute__((aligned(16))) char s_raw[];
    constexpr int F4 = FULL_SH ? 16 : 8;
    const int lane = threadIdx.x;
    const uint64_t v0 = (uint64_t)blockIdx.x * 64u;
    const uint64_t byte0 = v0 * stride;
    const uint32_t span = (uint32_t)min((uint64_t)64u * stride, n * (uint64_t)stride - byte0);      // multiple of 4
    stage_span(s_raw, aos + byte0, span, lane);
    __syncthreads();
    const uint64_t i = v0 + lane;
    if (i >= n) return;
    const uint32_t* r = reinterpret_cast<const uint32_t*>(s_raw + (size_t)lane * stride);
    // cnt floats from byte offset off of the record, bits untouched.  The host's memcpy takes any offset: one that is no multiple
    // of 4 (uniform over the wave) is put together from neighbouring words -- off + 4 cnt < stride then, so word cnt is the record's
    auto put = [&](float* d, uint32_t off, int cnt) {
        const uint32_t* w = r + (off >> 2);
        const uint32_t sh = off & 3u;
        if (sh == 0u) {
#pragma unroll
            for (int k = 0; k < cnt; ++k) d[k] = __uint_as_float(w[k]);
        } else {
            uint32_t lo = w[0];
#pragma unroll
            for (int k = 0; k < cnt; ++k) {
                const uint32_t hi = w[k + 1];
                d[k] = __uint_as_float(__builtin_amdgcn_alignbyte(hi, lo, sh));
                lo = hi;
            }
        }
    };
    float f[F4 * 4];
    put(f + 0, O.pos_with_alpha, 4);
    put(f + 4, O.r_sh0, 4);
    put(f + 8, O.g_sh0, 4);
    put(f + 12, O.b_sh0, 4);
    put(f + 16, O.cov3_col0, 3);
    put(f + 19, O.cov3_col1, 3);
    put(f + 22, O.cov3_col2, 3);
    if constexpr (FULL_SH) {
#pragma unroll
        for (int k = 0; k < 9; ++k) put(f + 25 + 4 * k, O.sh_full[k], 4);
        f[61] = f[62] = f[63] = 0.0f;
    } else {
#pragma unroll
        for (int k = 25; k < 32; ++k) f[k] = 0.0f;
    }
    store_record<FULL_SH, STORAGE>(f, i, pos4, recs, n_over);
}

// ------------------------------------------------------------------------------------------
// Spatial storage order (round 4; see box_live above).  Upload-time only: the moments of the positions and of the footprint
// bounds, a 32-bit code per splat (2 bits of size class above a 30-bit Morton code: 10 bits per axis over mean +- 3 sigma,
// outliers clamped to the border cells), a stable sort of the codes with the 8-bit radix passes above (ties keep upload
// order), a gather of the cloud into that order and one bounding box per kBoxSplats stored splats.  Draw order is by depth key,
// ties by STORAGE order.
// ------------------------------------------------------------------------------------------
// (two stages with a fixed summation order and no atomics: every device of a group, and every run, must arrive at the same
//  storage order bit for bit -- tie order is part of the frame)
constexpr int kMoments = 10;
__global__ __launch_bounds__(kThreads) void cloud_moments_kernel(const float4* __restrict__ pos, uint32_t n,
                                                                 double* __restrict__ part /* [gridDim.x][kMoments] */)
{
    __shared__ double s_w[kThreads / 64][kMoments];
    // sum xyz, sum of squares xyz, count of finite positions; sum, sum of squares, count of log2(footprint bound) where it is > 0
    double s[kMoments] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const float4 p = pos[i];
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
            s[0] += p.x; s[1] += p.y; s[2] += p.z;
            s[3] += (double)p.x * p.x; s[4] += (double)p.y * p.y; s[5] += (double)p.z * p.z;
            s[6] += 1.0;
            if (p.w > 0.0f && isfinite(p.w)) {
                const double l = (double)log2f(p.w);
                s[7] += l; s[8] += l * l; s[9] += 1.0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kMoments; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d, 64);
        if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < kMoments) {
        double t = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) t += s_w[w][threadIdx.x];
        part[(size_t)blockIdx.x * kMoments + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(kThreads) void cloud_moments_finish(const double* __restrict__ part, uint32_t rows,
                                                                 double* __restrict__ acc /* kMoments */)
{
    __shared__ double s_t[kThreads][kMoments];
    double s[kMoments] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t r = threadIdx.x; r < rows; r += kThreads)
#pragma unroll
        for (int k = 0; k < kMoments; ++k) s[k] += part[(size_t)r * kMoments + k];
#pragma unroll
    for (int k = 0; k < kMoments; ++k) s_t[threadIdx.x][k] = s[k];
    __syncthreads();
    for (int half = kThreads / 2; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half)
#pragma unroll
            for (int k = 0; k < kMoments; ++k) s_t[threadIdx.x][k] += s_t[threadIdx.x + half][k];
        __syncthreads();
    }
    if (threadIdx.x < kMoments) acc[threadIdx.x] = s_t[0][threadIdx.x];
}

__device__ __forceinline__ uint32_t morton_spread10(uint32_t v)      // 10 bits -> every third bit
{
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

__global__ __launch_bounds__(kThreads) void morton_kernel(const float4* __restrict__ pos, uint32_t n,
                                                          const double* __restrict__ acc, uint32_t* __restrict__ code,
                                                          uint32_t* __restrict__ index)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const double cnt = acc[6] > 0.0 ? acc[6] : 1.0;
    float q[3];
    const float4 p = pos[i];
    const float c[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double mean = acc[k] / cnt;
        const double var = acc[3 + k] / cnt - mean * mean;
        const float sd = (float)sqrt(var > 1e-30 ? var : 1e-30);
        const float t = (c[k] - (float)mean) / (6.0f * sd) + 0.5f;                // mean +- 3 sigma -> [0, 1]
        q[k] = isfinite(t) ? fminf(fmaxf(t, 0.0f), 1.0f) * 1023.0f : 0.0f;
    }
    // Size class in the two top bits: a box's reach on screen is its extent plus its LARGEST footprint, and the largest of
    // 256 log-normal sizes is several times the typical one -- splats are therefore grouped by footprint bound first (z = deviation
    // of log2(bound) from its mean in sigmas: <= 0.5 | <= 1.25 | <= 2 | the rest, ~69 / 20 / 9 / 2 %), by position inside a class.
    uint32_t cls = 3u;
    if (p.w > 0.0f && isfinite(p.w) && acc[9] > 0.0) {
        const double lm = acc[7] / acc[9], lv = acc[8] / acc[9] - lm * lm;
        const float z = (log2f(p.w) - (float)lm) / (float)sqrt(lv > 1e-12 ? lv : 1e-12);
        cls = z <= 0.5f ? 0u : (z <= 1.25f ? 1u : (z <= 2.0f ? 2u : 3u));
    }
    code[i] = (cls << 30) | morton_spread10((uint32_t)q[0]) | (morton_spread10((uint32_t)q[1]) << 1) | (morton_spread10((uint32_t)q[2]) << 2);
    index[i] = i;
}

// stored slot j <- uploaded splat order[j]: one wave moves 64 / F4 records per step with coalesced 16-byte accesses
__global__ __launch_bounds__(kThreads) void gather_cloud_kernel(const uint32_t* __restrict__ order, uint32_t n, int F4,
                                                                const float4* __restrict__ pos_in,
                                                                const float4* __restrict__ recs_in,
                                                                float4* __restrict__ pos_out, float4* __restrict__ recs_out)
{
    const uint64_t total = (uint64_t)n * (uint32_t)F4;
    for (uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kThreads) {
        const uint32_t j = (uint32_t)(e / (uint32_t)F4), sub = (uint32_t)(e - (uint64_t)j * (uint32_t)F4);
        const uint32_t src = order[j];
        recs_out[e] = recs_in[(size_t)src * F4 + sub];
        if (sub == 0u) pos_out[j] = pos_in[src];
    }
}

// one workgroup per box of kBoxSplats stored splats
__global__ __launch_bounds__(kThreads) void cull_boxes_kernel(const float4* __restrict__ pos, uint32_t n,
                                                              CullBox* __restrict__ boxes)
{
    __shared__ float s_red[7][kThreads / 64];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, wmax = 0.0f;
    const uint32_t base = blockIdx.x * kBoxSplats;
    for (uint32_t k = threadIdx.x; k < (uint32_t)kBoxSplats && base + k < n; k += kThreads) {
        const float4 p = pos[base + k];
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
            lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
            hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
            if (p.w > wmax) wmax = p.w;                                     // (NaN never wins; inf does, and then nothing is band-culled)
        }
    }
    float r[7] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], wmax};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float o = __shfl_xor(r[k], d, 64);
            r[k] = k < 3 ? fminf(r[k], o) : fmaxf(r[k], o);
        }
        if ((threadIdx.x & 63) == 0) s_red[k][threadIdx.x >> 6] = r[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
            for (int w = 1; w < kThreads / 64; ++w) r[k] = k < 3 ? fminf(r[k], s_red[k][w]) : fmaxf(r[k], s_red[k][w]);
        CullBox b;
        b.lo = make_float4(r[0], r[1], r[2], r[6]);
        b.hi = make_float4(r[3], r[4], r[5], 0.0f);
        boxes[blockIdx.x] = b;
    }
}

// ---- per-splat visibility (msplat_set_visibility / msplat_set_crop, include/msplat.h).  A hidden splat is a splat pass 0 of the
// sort rejects: the context's Sort reads a COPY of the position plane in which a hidden splat's x is a quiet NaN -- every comparison
// of cull_key is then false -- and cull boxes built over the visible splats only.  Nothing else in the frame knows.
constexpr int kCropBox = 1, kCropSphere = 2, kCropShapeMask = 0xFF, kCropInvert = 0x100;      // MSPLAT_CROP_*
struct VisibilityArgs {
    const float4* pos;          // the store's plane (storage order)
    const uint8_t* mask;        // one byte per splat in UPLOAD numbering, nonzero = visible; nullptr: no mask
    const uint32_t* order;      // slot -> upload index of a reordered store; nullptr: the store is in upload order
    uint32_t n;
    int shape;                  // MSPLAT_CROP_BOX / _SPHERE, | MSPLAT_CROP_INVERT; 0: no crop
    float m[16];                // world -> crop space, column-major; row 3 is not read
    float4* vis_pos;            // out: pos with x = NaN where hidden
    CullBox* boxes;             // out: one box per kBoxSplats slots over the visible finite centres; hi.w (read by no kernel) = the
                                // box's hidden splats, as a float: msplat_get_visibility sums them
};

// the crop rule of msplat.h, in cull_key's operation order (fp32, no contraction); false for a NaN centre with either shape
__device__ __forceinline__ bool crop_inside(const float4 p, const float* m, int shape)
{
    const float qx = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], p.x), __fmul_rn(m[4], p.y)), __fmul_rn(m[8], p.z)), m[12]);
    const float qy = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[1], p.x), __fmul_rn(m[5], p.y)), __fmul_rn(m[9], p.z)), m[13]);
    const float qz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[2], p.x), __fmul_rn(m[6], p.y)), __fmul_rn(m[10], p.z)), m[14]);
    if ((shape & kCropShapeMask) == kCropSphere)
        return __fadd_rn(__fadd_rn(__fmul_rn(qx, qx), __fmul_rn(qy, qy)), __fmul_rn(qz, qz)) <= 1.0f;
    return fabsf(qx) <= 1.0f && fabsf(qy) <= 1.0f && fabsf(qz) <= 1.0f;
}

// one workgroup per box, one lane per stored slot: 16 + 16 + 1 (+ 4) bytes per splat, coalesced but for the mask bytes of a
// reordered store (Morton neighbours: scattered over upload numbers).  The hidden count stays per box: one atomicAdd per workgroup
// on ONE counter was measured first and was the kernel -- 23 k same-address atomics at 6 M splats, 255-280 us against 50-80 us
// without them (EXPERIMENTS.md, round 21)
__global__ __launch_bounds__(kThreads) void visibility_kernel(const VisibilityArgs a)
{
    static_assert(kBoxSplats == kThreads, "one lane per slot of a box");
    __shared__ float s_red[7][kThreads / 64];
    __shared__ uint32_t s_hid[kThreads / 64];
    float r[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0f};
    const uint32_t slot = blockIdx.x * kBoxSplats + threadIdx.x;
    bool hide = false;
    if (slot < a.n) {
        float4 p = a.pos[slot];
        bool vis = true;
        if (a.mask) vis = a.mask[a.order ? a.order[slot] : slot] != 0;
        if (a.shape != 0) vis = vis && (crop_inside(p, a.m, a.shape) != ((a.shape & kCropInvert) != 0));
        hide = !vis;
        if (vis && isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
            r[0] = p.x; r[1] = p.y; r[2] = p.z; r[3] = p.x; r[4] = p.y; r[5] = p.z;
            if (p.w > 0.0f) r[6] = p.w;                                     // (as cull_boxes_kernel: NaN never wins)
        }
        if (hide) p.x = __uint_as_float(0x7FC00000u);
        a.vis_pos[slot] = p;
    }
    const uint32_t hid = (uint32_t)__popcll(__ballot(hide));
    if ((threadIdx.x & 63) == 0) s_hid[threadIdx.x >> 6] = hid;
    // the box: cull_boxes_kernel's reduction (written again, not shared: that kernel's registers stay as they were)
#pragma unroll
    for (int k = 0; k < 7; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float o = __shfl_xor(r[k], d, 64);
            r[k] = k < 3 ? fminf(r[k], o) : fmaxf(r[k], o);
        }
        if ((threadIdx.x & 63) == 0) s_red[k][threadIdx.x >> 6] = r[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t h = s_hid[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) {
            h += s_hid[w];
#pragma unroll
            for (int k = 0; k < 7; ++k) r[k] = k < 3 ? fminf(r[k], s_red[k][w]) : fmaxf(r[k], s_red[k][w]);
        }
        CullBox b;
        b.lo = make_float4(r[0], r[1], r[2], r[6]);
        b.hi = make_float4(r[3], r[4], r[5], (float)h);        // (h <= 256: exact)
        a.boxes[blockIdx.x] = b;
    }
}

}  // namespace msplat
