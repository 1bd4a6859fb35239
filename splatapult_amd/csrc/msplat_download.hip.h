// msplat_download.hip.h -- the way out of the device: the stored cloud as the reference's interleaved records (unpack_kernel) or as
// the PLY attributes GaussianCloud::ExportPly writes (egress_kernel), into device memory, in upload numbering
// (one of the parts of msplat_kernels.hip.h; host side: msplat_download.hip.inc; the rule: include/msplat.h)
//
// The inverse of the ingest kernels of msplat_cloud.hip.h and their shape: a workgroup is one wave, a wave takes 64 rows.  The rows
// are OUTPUT rows -- upload indices row0 + 64 b .. -- and row i is read from stored slot inv[i] (inv == nullptr: the store is in
// upload order, slot i).  A stored record is 128, 160 or 256 bytes on a boundary of its own size, so the gather of a reordered store
// moves whole cache lines; the 100 / 244 / 248-byte rows that go out are no multiple of 16 bytes and would be partial lines if they
// were scattered, so the wave's 64 rows, one contiguous run in the destination whatever the storage order, are put together in
// LDS and stored with whole-wave 16-byte stores (stage_span run backwards).  EXPERIMENTS.md, round 28.
//   invert_order_kernel   inv[order[slot]] = slot, once per call on a reordered store
//   unpack_kernel         records: the stored record decoded by sh16_unpack / sh8_unpack, the padding dropped
//   egress_kernel         ExportPly's per-splat rule, a Writer per destination in the way ingest_vertex has a Reader per source
#pragma once

#include "msplat_cloud.hip.h"

#pragma clang fp contract(off)

namespace msplat {

// dynamic LDS of the kernels below, in bytes: the 64 stored rows (padded to an odd number of words: 64 lanes, 64 banks), later
// overwritten by the 64 rows that go out
__host__ __device__ constexpr uint32_t download_lds_bytes(int storage, bool full_sh, uint32_t out_row_bytes)
{
    const uint32_t in = 64u * (uint32_t)(cloud_f4(storage, full_sh) * 4 + 1) * 4u, out = 64u * out_row_bytes;
    return in > out ? in : out;
}

__global__ __launch_bounds__(kThreads) void invert_order_kernel(const uint32_t* __restrict__ order, uint32_t n, uint32_t* __restrict__ inv)
{
    for (uint32_t j = blockIdx.x * kThreads + threadIdx.x; j < n; j += gridDim.x * kThreads) inv[order[j]] = j;
}

// the wave's span of `span` bytes (a multiple of 4) from LDS to dst (16-byte aligned) with coalesced 16-byte stores; the sub-16-byte
// tail of the last block goes word by word: not a byte behind the span is written
__device__ __forceinline__ void flush_span(char* __restrict__ dst, const char* __restrict__ src, uint32_t span, int lane)
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

// the same to a destination that is only 4-byte aligned (a caller's f_rest array): one dword per lane and step, 256 B an instruction
__device__ __forceinline__ void flush_words(float* __restrict__ dst, const float* __restrict__ src, uint32_t words, int lane)
{
    for (uint32_t o = lane; o < words; o += 64u) dst[o] = src[o];
}

// The wave's `rows` stored records (lane r: slot `slot`) -> LDS with coalesced 16-byte loads, then each lane's own row decoded to the
// FP32 record floats f[] (the values msplat_download_cloud returns; padding 0).  On return every lane has read its row: s_rec is free.
template <bool FULL_SH, int STORAGE>
__device__ __forceinline__ void load_record_floats(uint32_t* s_rec, const float4* __restrict__ recs, uint32_t slot, uint32_t rows,
                                                   uint32_t lane, float* f)
{
    constexpr int F4 = cloud_f4(STORAGE, FULL_SH), RW = F4 * 4, STRIDE = RW + 1, NF = (FULL_SH ? 16 : 8) * 4;
#pragma unroll
    for (int k = 0; k < F4; ++k) {
        const uint32_t e = (uint32_t)k * 64u + lane, r = e / (uint32_t)F4, sub = e % (uint32_t)F4;
        const uint32_t s = __shfl(slot, r & 63u, 64);      // (every lane takes part in the shuffle)
        if (r < rows) {
            const float4 v = recs[(size_t)s * F4 + sub];
            uint32_t* w = s_rec + r * STRIDE + sub * 4u;
            w[0] = __float_as_uint(v.x); w[1] = __float_as_uint(v.y); w[2] = __float_as_uint(v.z); w[3] = __float_as_uint(v.w);
        }
    }
    __syncthreads();
    const uint32_t* row = s_rec + lane * STRIDE;
    if (lane < rows) {
        if constexpr (STORAGE == kStorageFp32) {
#pragma unroll
            for (int k = 0; k < NF; ++k) f[k] = __uint_as_float(row[k]);
        } else {
            uint32_t w[RW];
#pragma unroll
            for (int k = 0; k < RW; ++k) w[k] = row[k];
#pragma unroll
            for (int k = 0; k < NF; ++k) f[k] = 0.0f;
            if constexpr (STORAGE == kStorageShQ8) sh8_unpack<FULL_SH>(w, f); else sh16_unpack<FULL_SH>(w, f);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NF; ++k) f[k] = 0.0f;
    }
    __syncthreads();
}

// rows row0 .. row0 + cnt - 1 (upload numbering) as tight reference records, 244 B with full SH, 100 B without, at out (the address
// of row row0, 16-byte aligned): bit for bit what msplat_download_cloud's host loop writes
template <bool FULL_SH, int STORAGE>
__global__ __launch_bounds__(64) void unpack_kernel(const float4* __restrict__ recs, const uint32_t* __restrict__ inv, uint32_t row0,
                                                    uint32_t cnt, char* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_buf[];
    constexpr int NF = (FULL_SH ? 16 : 8) * 4, OW = FULL_SH ? 61 : 25;
    const uint32_t lane = threadIdx.x, r0 = blockIdx.x * 64u, rows = min(64u, cnt - r0);
    const uint32_t i = row0 + r0 + lane;
    const uint32_t slot = lane < rows ? (inv ? inv[i] : i) : 0u;
    float f[NF];
    load_record_floats<FULL_SH, STORAGE>(s_buf, recs, slot, rows, lane, f);
    if (lane < rows) {
#pragma unroll
        for (int k = 0; k < OW; ++k) s_buf[lane * OW + k] = __float_as_uint(f[k]);      // (61 and 25 are odd: 64 banks)
    }
    __syncthreads();
    flush_span(out + (size_t)r0 * (OW * 4), reinterpret_cast<const char*>(s_buf), rows * (uint32_t)(OW * 4), (int)lane);
}

// ------------------------------------------------------------------------------------------
// The PLY attributes: GaussianCloud::ExportPly's per-splat rule (splatapult_amd/host/gaussian_scene.cpp) on the decoded record,
// operation for operation -- JacobiEigen3 in double, everything else in fp32, contraction off.
// ------------------------------------------------------------------------------------------
// one Jacobi rotation in the (P, Q) plane: JacobiEigen3's loop body.  P and Q are template arguments and every loop below is
// unrolled, so that a and v are eighteen named registers: a run-time index into either would send them to scratch
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3])
{
    if (fabs(a[P][Q]) < 1e-300) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * a[P][Q]);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double akp = a[k][P], akq = a[k][Q];
        a[k][P] = c * akp - s * akq;
        a[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double apk = a[P][k], aqk = a[Q][k];
        a[P][k] = c * apk - s * aqk;
        a[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
}

// JacobiEigen3: V (column-major, as stored) symmetrised, cyclic sweeps over (0,1), (0,2), (1,2), eigenvalues ascending with ties in
// index order (std::sort's insertion sort of three), rounded once to fp32; evec[3 k + r] = component r of eigenvector k.  The early
// exit is the lane's own; the bound of 32 sweeps is what ends a NaN record
__device__ __forceinline__ void jacobi_eigen3(const float* V, float* evec, float* eval)
{
    double a[3][3], v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) a[r][c] = 0.5 * ((double)V[c * 3 + r] + (double)V[r * 3 + c]);
#pragma unroll 1
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        if (off < 1e-30) break;
        jacobi_rotate<0, 1>(a, v);
        jacobi_rotate<0, 2>(a, v);
        jacobi_rotate<1, 2>(a, v);
    }
    // the position of each diagonal entry in the stable ascending order, then the three outputs by selects
    const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
    const int p0 = (d1 < d0 ? 1 : 0) + (d2 < d0 ? 1 : 0);
    const int p1 = (d1 < d0 ? 0 : 1) + (d2 < d1 ? 1 : 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool is0 = p0 == k, is1 = !is0 && p1 == k;
        eval[k] = (float)(is0 ? d0 : (is1 ? d1 : d2));
#pragma unroll
        for (int r = 0; r < 3; ++r) evec[k * 3 + r] = (float)(is0 ? v[r][0] : (is1 ? v[r][1] : v[r][2]));
    }
}

// QuatFromMat3: rotation matrix (column-major, det +1) -> quaternion (w, x, y, z), fp32
__device__ __forceinline__ void quat_from_mat3(const float* R, float* q)
{
    const float m00 = R[0], m11 = R[4], m22 = R[8];
    const float tr = m00 + m11 + m22;
    float w, x, y, z;
    if (tr > 0.0f) {
        const float s = sqrtf(tr + 1.0f) * 2.0f;
        w = 0.25f * s;
        x = __fdiv_rn(R[1 * 3 + 2] - R[2 * 3 + 1], s);
        y = __fdiv_rn(R[2 * 3 + 0] - R[0 * 3 + 2], s);
        z = __fdiv_rn(R[0 * 3 + 1] - R[1 * 3 + 0], s);
    } else if (m00 > m11 && m00 > m22) {
        const float s = sqrtf(1.0f + m00 - m11 - m22) * 2.0f;
        w = __fdiv_rn(R[1 * 3 + 2] - R[2 * 3 + 1], s);
        x = 0.25f * s;
        y = __fdiv_rn(R[1 * 3 + 0] + R[0 * 3 + 1], s);
        z = __fdiv_rn(R[2 * 3 + 0] + R[0 * 3 + 2], s);
    } else if (m11 > m22) {
        const float s = sqrtf(1.0f + m11 - m00 - m22) * 2.0f;
        w = __fdiv_rn(R[2 * 3 + 0] - R[0 * 3 + 2], s);
        x = __fdiv_rn(R[1 * 3 + 0] + R[0 * 3 + 1], s);
        y = 0.25f * s;
        z = __fdiv_rn(R[2 * 3 + 1] + R[1 * 3 + 2], s);
    } else {
        const float s = sqrtf(1.0f + m22 - m00 - m11) * 2.0f;
        w = __fdiv_rn(R[0 * 3 + 1] - R[1 * 3 + 0], s);
        x = __fdiv_rn(R[2 * 3 + 0] + R[0 * 3 + 2], s);
        y = __fdiv_rn(R[2 * 3 + 1] + R[1 * 3 + 2], s);
        z = 0.25f * s;
    }
    const float n = sqrtf(w * w + x * x + y * y + z * z);
    q[0] = __fdiv_rn(w, n); q[1] = __fdiv_rn(x, n); q[2] = __fdiv_rn(y, n); q[3] = __fdiv_rn(z, n);
}

// ExportPly's rule on one decoded record f[], behind every egress kernel.  `o` takes the splat's properties by name:
// o.pos(c, v), o.f_dc(c, v), o.f_rest(k, v) (PLY order f_rest_0..44: the inverse of ingest_vertex's repack; zeros for a cloud
// without full SH), o.opacity(v), o.scale(c, v), o.rot(c, v) (w x y z)
template <bool FULL_SH, class Out>
__device__ __forceinline__ void egress_vertex(const float* f, Out& o)
{
    o.pos(0, f[0]); o.pos(1, f[1]); o.pos(2, f[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.f_dc(c, f[4 + 4 * c]);
#pragma unroll
        for (int k = 1; k < 16; ++k) {
            float v = 0.0f;
            if constexpr (FULL_SH) v = k < 4 ? f[4 + 4 * c + k] : f[25 + 12 * c + (k - 4)];
            o.f_rest(c * 15 + k - 1, v);
        }
    }
    o.opacity(-logf(__fdiv_rn(1.0f, f[3]) - 1.0f));      // ComputeOpacityFromAlpha
    float evec[9], eval[3], q[4];
    jacobi_eigen3(f + 16, evec, eval);
    // a proper rotation (det +1) before the quaternion
    const float det = evec[0] * (evec[4] * evec[8] - evec[5] * evec[7]) - evec[3] * (evec[1] * evec[8] - evec[2] * evec[7]) +
                      evec[6] * (evec[1] * evec[5] - evec[2] * evec[4]);
    if (det < 0.0f) {
#pragma unroll
        for (int k = 0; k < 9; ++k) evec[k] = -evec[k];
    }
    quat_from_mat3(evec, q);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.scale(k, logf(sqrtf(eval[k] < 0.0f ? 0.0f : eval[k])));      // (std::max(eval, 0.0f): a NaN stays)
#pragma unroll
    for (int k = 0; k < 4; ++k) o.rot(k, q[k]);
}

// ---- the destinations.  A Writer is the kernel argument; begin() prepares the wave's LDS, lane() is one splat's Out, flush() stores
// what the lanes left in LDS.  Every pointer is the address of row row0.
// Six attribute arrays (msplat_download_attributes_device), 4-byte aligned: xyz, f_dc, opacity, scale and rot are 14 floats a
// splat, stored by the lane that owns it (a wave's stores cover one contiguous run per array); the 64 x 45 floats of f_rest are one
// contiguous 11.25-KB run, put together in LDS at a stride of 45 words -- odd: 64 banks -- and stored one dword per lane and step.
// f_rest == nullptr: skipped
struct AttrWriter {
    float* xyz; float* f_dc; float* f_rest; float* opacity; float* log_scale; float* rot;
    struct Out {
        const AttrWriter& A;
        size_t i;              // row, from row0
        float* rest;           // the splat's 45 floats in LDS
        __device__ __forceinline__ void pos(int c, float v) { A.xyz[i * 3 + c] = v; }
        __device__ __forceinline__ void f_dc(int c, float v) { A.f_dc[i * 3 + c] = v; }
        __device__ __forceinline__ void f_rest(int k, float v) { if (A.f_rest) rest[k] = v; }
        __device__ __forceinline__ void opacity(float v) { A.opacity[i] = v; }
        __device__ __forceinline__ void scale(int c, float v) { A.log_scale[i * 3 + c] = v; }
        __device__ __forceinline__ void rot(int c, float v) { A.rot[i * 4 + c] = v; }
    };
    __device__ __forceinline__ void begin(uint32_t*, uint32_t, uint32_t) const {}
    __device__ __forceinline__ Out lane(uint32_t* s_buf, uint32_t r0, uint32_t lane_) const
    {
        return Out{*this, (size_t)r0 + lane_, reinterpret_cast<float*>(s_buf) + lane_ * 45u};
    }
    __device__ __forceinline__ void flush(const uint32_t* s_buf, uint32_t r0, uint32_t rows, uint32_t lane_) const
    {
        if (f_rest) flush_words(f_rest + (size_t)r0 * 45u, reinterpret_cast<const float*>(s_buf), rows * 45u, (int)lane_);
    }
};

// A PLY vertex block (msplat_download_ply_vertices_device, msplat_export_ply), 16-byte aligned: the wave's 64 vertices are zeroed in
// LDS, every lane writes the properties the layout has (offset >= 0) into its own vertex, and the span goes out with 16-byte
// stores -- so every byte of a vertex that no property covers is written, as 0
struct VertexWriter {
    char* out;
    PlyLayout L;
    struct Out {
        char* v;
        const PlyLayout& L;
        __device__ __forceinline__ void wr(int32_t off, float x) { if (off >= 0) *reinterpret_cast<float*>(v + off) = x; }
        __device__ __forceinline__ void pos(int c, float x) { wr(c == 0 ? L.x : (c == 1 ? L.y : L.z), x); }
        __device__ __forceinline__ void f_dc(int c, float x) { wr(L.f_dc[c], x); }
        __device__ __forceinline__ void f_rest(int k, float x) { wr(L.f_rest[k], x); }
        __device__ __forceinline__ void opacity(float x) { wr(L.opacity, x); }
        __device__ __forceinline__ void scale(int c, float x) { wr(L.scale[c], x); }
        __device__ __forceinline__ void rot(int c, float x) { wr(L.rot[c], x); }
    };
    __device__ __forceinline__ void begin(uint32_t* s_buf, uint32_t rows, uint32_t lane_) const
    {
        const uint32_t span = rows * L.vertex_size;      // (64 vertices are a multiple of 16 bytes: the last 16-byte block fits)
        for (uint32_t off = lane_ * 16u; off < span; off += 64u * 16u)
            *reinterpret_cast<float4*>(reinterpret_cast<char*>(s_buf) + off) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        __syncthreads();
    }
    __device__ __forceinline__ Out lane(uint32_t* s_buf, uint32_t, uint32_t lane_) const
    {
        return Out{reinterpret_cast<char*>(s_buf) + (size_t)lane_ * L.vertex_size, L};
    }
    __device__ __forceinline__ void flush(const uint32_t* s_buf, uint32_t r0, uint32_t rows, uint32_t lane_) const
    {
        flush_span(out + (size_t)r0 * L.vertex_size, reinterpret_cast<const char*>(s_buf), rows * L.vertex_size, (int)lane_);
    }
};

template <bool FULL_SH, int STORAGE, class Writer>
__global__ __launch_bounds__(64) void egress_kernel(const float4* __restrict__ recs, const uint32_t* __restrict__ inv, uint32_t row0,
                                                    uint32_t cnt, const Writer W)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_buf[];
    constexpr int NF = (FULL_SH ? 16 : 8) * 4;
    const uint32_t lane = threadIdx.x, r0 = blockIdx.x * 64u, rows = min(64u, cnt - r0);
    const uint32_t i = row0 + r0 + lane;
    const uint32_t slot = lane < rows ? (inv ? inv[i] : i) : 0u;
    float f[NF];
    load_record_floats<FULL_SH, STORAGE>(s_buf, recs, slot, rows, lane, f);
    W.begin(s_buf, rows, lane);
    if (lane < rows) {
        auto o = W.lane(s_buf, r0, lane);
        egress_vertex<FULL_SH>(f, o);
    }
    __syncthreads();
    W.flush(s_buf, r0, rows, lane);
}

}  // namespace msplat
