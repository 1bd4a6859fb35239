// msplat_common.hip.h -- constants, per-frame parameters, block scans, XCD-aware index maps, the presort cull and the
// box-level cull shared by the kernels of the splat hot path (hand-written CDNA4: gfx950, wave64).  Part of msplat_kernels.hip.h.
//
// Design notes: everything is HBM/LDS/VALU work -- no MFMA anywhere.
// Compiled with -ffp-contract=off: an FMA happens only where __builtin_fmaf is written.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// The key / reject arithmetic must execute exactly as written (bit-parity with the oracle):
// no implicit FMA contraction anywhere in this file (the build also passes -ffp-contract=off).
#pragma clang fp contract(off)

namespace msplat {

constexpr int kThreads = 256;            // 4 wave64 per workgroup
// Wave issue priorities (s_setprio; SIMD arbitration is priority first, then age).  With frames in flight the waves of different
// frames' kernels share SIMDs: the short, latency-bound sort / binning kernels run at 3, the HBM-bound projection at 2 and the
// VALU-bound compositor at 1 (its heaviest items) or 0, so a chain kernel's few instructions between two memory waits are issued
// ahead of the compositor's arithmetic instead of queueing behind it.  Measured r5 (tools/gpu_r5_d.sh, eight combinations,
// driver protocol, same box): config 2 5741 -> 6028 frames/s (6208 -> 6352 in 500-frame blocks), config 5 2890 -> 3036,
// 6 M / 1080p 2313 -> 2349, 6 M / 4096^2 1312 -> 1338, scene-like 5217 -> 5328; one frame at a time: unchanged.
constexpr int kChainPrio = 3, kProjPrio = 2, kCompPrioMax = 1;
#define MSPLAT_CHAIN_ENTER() __builtin_amdgcn_s_setprio(msplat::kChainPrio)
// keys per thread per chunk of the sort passes: 8 (2048-key chunks) up to 2 M splats -- 4 measured no faster (r1), 16 slower
// at 1 M (245 workgroups for 256 CUs: sort 76 -> 91 us) -- and 16 (4096-key chunks) beyond: digit runs twice as long make
// the scattered write-out cheaper (6 M splats: sort 234 -> 212 us, r2)
constexpr int kSortItems = 8;
constexpr int kSortItemsLarge = 16;
constexpr int kSortChunk = kThreads * kSortItems;   // 2048 keys per chunk
constexpr int kPairItems = 16;           // binning pass 2 moves 7x more words: bigger chunks, longer runs
constexpr int kPairChunk = kThreads * kPairItems;   // 4096 words per chunk
template <int MODE, int SORT_ITEMS> struct RadixCfg { static constexpr int ITEMS = (MODE == 2) ? kPairItems : SORT_ITEMS; static constexpr int CHUNK = kThreads * ITEMS; };
constexpr int kBinChunk = 1024;          // draw-order ranks per chunk in the tile-column partition (512 / 2048 measured at 1 M: binning 64 -> 70 us)
constexpr uint32_t kHeavyPairs = 49152;  // a column-pass chunk with more pairs than this is split over kHeavyParts workgroups
constexpr uint32_t kHeavyCap = 128;      // at most this many split chunks per frame (the rest run unsplit: correct, slower)
constexpr uint32_t kHeavyParts = 8;      // column blocks per split chunk
constexpr int kTile = 16;                // one compositor wave owns a 16x16 pixel tile ...
constexpr int kBin = 32;                 // ... binning works on 32x32 bins (4 tiles share one list, each
                                         // wave filters it for its own quadrant): 2.2-2.9x fewer pairs
// the compositors' sharded work queue (queue_next): 32 heads, one 64-byte line each
constexpr uint32_t kQueueShards = 32;
constexpr uint32_t kQueueStride = 16;          // words between heads
constexpr uint32_t kRectEmpty = 0x000000FFu;   // tx0=255 > tx1=0
constexpr uint32_t kRankMask = 0x00FFFFFFu;

enum { MODE_KEYS = 0, MODE_CULL = 1, MODE_PAIR = 2 };

// ------------------------------------------------------------------------------------------
// The three word tables kernels and host share.  These are the ONLY definitions of their layouts: no literal indexes them.
// ------------------------------------------------------------------------------------------
// Host-mapped status words (msplat_ctx::h_flags = the host's view, d_flags = the device's).  Kernels leave them with relaxed
// system-scope stores; the host reads them without ever waiting for the GPU (host_word, msplat_device.hip), so every one describes
// some EARLIER frame.  V, D and the heavy chunks only steer launch choices (any value gives the same pixels); the two-pass words
// are the controller's feedback (host/two_pass_controller.hpp) and what msplat_get_two_pass_info reports.
enum HostWord : int {
    kHostOverflowPairs = 0,    // pairs needed by an overflowed device-output render (poll_async_overflow)        bin1_downsweep
    kHostV = 1,                // ranks binned by the latest frame: the Sort's own V                               bin1_downsweep
    kHostD = 2,                // ... and its pairs                                                               bin1_downsweep
    kHostHeavyChunks = 3,      // heavy chunks its column pass wanted                                             bin1_downsweep
    kHostPass1Pairs = 4,       // two-pass frame: pairs of pass 1                                                 occ_gate_kernel
    kHostUnfinishedBins = 5,   // ... bins pass 1 left unfinished                                                 occ_gate_kernel
    kHostPass1Splats = 6,      // ... splats in pass 1                                                            occ_gate_kernel
    kHostListedRanks = 7,      // ... listed ranks of pass 2                                                      project_kernel<PROJ_LISTED>
    kHostPass2Pairs = 8,       // ... pairs of pass 2                                         bin1_downsweep through host_D2
    kHostPass1Seq = 9,         // number of the frame words 4 to 6 describe                                       occ_gate_kernel
    kHostPass2Seq = 10,        // number of the frame word 8 describes                        bin1_downsweep through host_D2
    kHostWordCount = 16
};
// bin1_downsweep gets the pass-2 words through one pointer, host_D2 = d_flags + kHostPass2Pairs: the frame number lies this far behind
constexpr int kHostD2SeqOffset = kHostPass2Seq - kHostPass2Pairs;

// Device counters (msplat_ctx::counters)
enum Counter : int {
    kCntV = 0,                 // visible splats of the latest Sort
    kCntD = 1,                 // pairs of the latest binning chain
    kCntOverflow = 2,          // pairs a frame needed beyond the capacity (0: none)
    kCntDrawn = 4,             // msplat_get_stats: splats drawn (count_drawn_kernel) ...
    kCntPairs16 = 6,           // ... and its 64-bit count of (splat, 16 x 16 tile) pairs: words 6..7, 8-byte aligned
    kCntLdsProbe = 8,          // msplat_create: violations seen by lds_atomic_order_probe
    kCntVframe2 = 9,           // two views in one chain: ranks the binning walks
    kCntMinKey = 10,           // minimum key of the visible set, one word per sort parity: words 10..11
    kCntOrderBad = 12,         // msplat_debug_verify_order: key / list violations, words 12..13
    kCounterCount = 16
};

// Words of a two-pass frame (msplat_ctx::occ; msplat_occlusion.hip.h).  The cut is a multiple of 1024 = kBinChunk.
enum OccWord : int {
    kOccCut = 0,               // first rank of pass 1                                                            project_kernel<PROJ_PASS1>
    kOccListed = 1,            // ranks behind the cut that pass the gate                                         occ_gate_kernel
    kOccUnfinished = 2,        // bins pass 1 left unfinished                                                     occ_mask_kernel
    kOccRanks2 = 4,            // ranks the second binning chain walks: V, or 0 when no bin is left               occ_mask_kernel
    kOccWordCount = 16
};

// Workgroup residency stamps (r6; DIAGNOSTIC builds only: -DMSPLAT_STAMPS, tools/stamp_timeline.py).  rocprofv3 serialises dispatches
// while it collects counters and this box has no PC sampling, so what frames IN FLIGHT do to each other was unknown.  With stamps
// every workgroup of the frame's kernels leaves {kernel id, block, HW_ID, XCC_ID, start, end} (s_memrealtime: 100 MHz) in a hashed
// table -- plain stores, no atomics, nothing returns to the wave -- while a device flag is on.  The product build compiles the
// macro to nothing.
#ifdef MSPLAT_STAMPS
struct StampRec { uint32_t kid, blk, hwid, xcc; unsigned long long t0, t1; };
__device__ StampRec* g_stamp_buf = nullptr;
__device__ uint32_t g_stamp_mask = 0u;           // table size - 1 while stamping is on, else 0
struct StampScope {
    unsigned long long t0;
    uint32_t kid, mask;
    __device__ __forceinline__ explicit StampScope(uint32_t k) : t0(0ull), kid(k), mask(0u)
    {
        if (threadIdx.x == 0) {
            mask = __builtin_nontemporal_load(&g_stamp_mask);
            if (mask) t0 = wall_clock64();
        }
    }
    __device__ __forceinline__ ~StampScope()
    {
        if (threadIdx.x == 0 && mask) {
            StampRec r;
            r.kid = kid; r.blk = blockIdx.x;
            r.hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4);        // HW_REG_HW_ID
            r.xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);        // HW_REG_XCC_ID
            r.t0 = t0; r.t1 = wall_clock64();
            uint32_t h = (uint32_t)t0 * 2654435761u ^ (blockIdx.x * 40503u) ^ (kid << 26) ^ (r.hwid * 97u) ^ (r.xcc << 13);
            h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
            g_stamp_buf[h & mask] = r;
        }
    }
};
#define MSPLAT_STAMP(KID) msplat::StampScope stamp_scope_((uint32_t)(KID))
#else
#define MSPLAT_STAMP(KID)
#endif
// kernel ids of the stamps (tools/stamp_timeline.py names them)
enum { KID_WS_UP_CULL = 1, KID_WS_DOWN_CULL = 2, KID_WS_UP = 3, KID_WS_DOWN = 4, KID_PROJECT = 5, KID_BIN1_UP = 6, KID_BIN1_DOWN = 7,
       KID_ROW_UP = 8, KID_ROW_DOWN = 9, KID_COMPOSITE = 11, KID_BOX_CULL = 12, KID_RADIX_UP = 13, KID_RADIX_DOWN = 14 };

// Per-frame constants, passed by value (lives in SGPRs / kernarg segment).
struct FrameParams {
    float mvp[16];     // projMat * inverse(cameraMat)            (splatrenderer.cpp:161,175)
    float view[16];    // inverse(cameraMat)                      (splatrenderer.cpp:327)
    float proj[16];
    float eye[3];      // cameraMat[3].xyz                        (splatrenderer.cpp:328)
    float W, H, X0, Y0, zn, zf;
    float t_eps;
    int width, height;
    int tiles_x, tiles_y;       // tiles_y = number of OWNED bin rows (band mode) else ceil(H / 32)
    // Band (multi-GPU): the owned bin rows are blocks of band_block consecutive rows that start at
    // band_first, band_first + band_stride, ...; they are numbered vy = 0 .. tiles_y - 1 in ascending order ("virtual rows":
    // what the pair words, the bin lists and the compositor's work items carry).  banded == 0: every row, vy == row.
    int banded, band_first, band_block, band_stride;
    float band_inv_stride;      // 1 / band_stride: row numbers are below 256, so their quotients are taken in float (exact)
    int full_sh, srgb;
    int band_cull;              // multi-GPU only: Sort also drops splats that cannot reach an owned bin row
    float view_scale2;          // upper bound of sigma_max(mat3(view))^2, at most 1e-5 above it (view_scale2_of; 1 + 1e-6 for a rigid camera)
    int depth_bits;             // 0 = colour-only target (no depth test); 24 / 32 = emulated depth buffer
    int rop;                    // 0 = float accumulation; 1 = RGBA8, 2 = RGBA16F render-target rounding after every blend
    // Two views in ONE render chain (msplat_render_stereo, r4): the second view's matrices; its splats are the draw-order ranks
    // [V1, V1 + V) with V1 = V rounded up to 64 (a projection wave never straddles the views), its bin rows follow the first
    // view's: rows_view .. 2 rows_view - 1.  views == 1: everything above describes the only view.
    int views, rows_view;
    float view1[16], proj1[16], eye1[3];
};

// What the compositor needs of a frame (r5): eleven words instead of FrameParams' five matrices in its kernarg segment / SGPRs.
struct CompParams {
    int width, height, tiles_x;
    int banded, band_first, band_block, band_stride;     // as in FrameParams
    int rows_view;                                       // two views in one chain: bin rows of the first view
    float t_eps;
};
__host__ inline CompParams comp_params(const FrameParams& fp)
{
    return CompParams{fp.width, fp.height, fp.tiles_x, fp.banded, fp.band_first, fp.band_block, fp.band_stride, fp.rows_view, fp.t_eps};
}

// What project_kernel needs of a frame (r5): one view's matrices and the raster geometry -- no mvp (the sort's), no second view.
struct ProjParams {
    float view[16], proj[16], eye[3];
    float W, H, X0, Y0;
    int width, height, tiles_y;
    int banded, band_first, band_block, band_stride;
    float band_inv_stride;
    int srgb, depth_bits, rows_view;
};
struct ProjView1 { float view[16], proj[16], eye[3]; };   // the second view of a two-view chain (project_kernel<*, PROJ_TWO_VIEWS> only)
struct ProjNoView1 { int unused; };
__host__ inline ProjParams proj_params(const FrameParams& fp)
{
    ProjParams p;
    for (int i = 0; i < 16; ++i) { p.view[i] = fp.view[i]; p.proj[i] = fp.proj[i]; }
    for (int i = 0; i < 3; ++i) p.eye[i] = fp.eye[i];
    p.W = fp.W; p.H = fp.H; p.X0 = fp.X0; p.Y0 = fp.Y0;
    p.width = fp.width; p.height = fp.height; p.tiles_y = fp.tiles_y;
    p.banded = fp.banded; p.band_first = fp.band_first; p.band_block = fp.band_block; p.band_stride = fp.band_stride;
    p.band_inv_stride = fp.band_inv_stride;
    p.srgb = fp.srgb; p.depth_bits = fp.depth_bits; p.rows_view = fp.rows_view;
    return p;
}
__host__ inline ProjView1 proj_view1(const FrameParams& fp)
{
    ProjView1 v;
    for (int i = 0; i < 16; ++i) { v.view[i] = fp.view1[i]; v.proj[i] = fp.proj1[i]; }
    for (int i = 0; i < 3; ++i) v.eye[i] = fp.eye1[i];
    return v;
}

// ------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------

// band geometry (see FrameParams): real bin row of virtual row vy
template <class P>
__host__ __device__ __forceinline__ int band_real_row(const P& fp, int vy)
{
    if (!fp.banded) return vy;
    const int k = vy / fp.band_block;
    return fp.band_first + k * fp.band_stride + (vy - k * fp.band_block);
}
// d / band_stride for 0 <= d < 65536 without an integer division (~30 instructions on this hardware, twice per splat in the
// band-culled sort and in project_kernel): (d + 0.5) / s lies at least 0.5 / s away from every integer, far more than the
// float error of the product
template <class P>
__host__ __device__ __forceinline__ int band_quot(const P& fp, int d)
{
    return (int)(((float)d + 0.5f) * fp.band_inv_stride);
}
// virtual index of the first owned row >= t (>= tiles_y: there is none)
template <class P>
__host__ __device__ __forceinline__ int band_first_owned_from(const P& fp, int t)
{
    if (!fp.banded) return t < 0 ? 0 : t;
    if (t <= fp.band_first) return 0;
    const int d = t - fp.band_first, k = band_quot(fp, d), j = d - k * fp.band_stride;
    return j < fp.band_block ? k * fp.band_block + j : (k + 1) * fp.band_block;
}
// virtual index of the last owned row <= t (-1: there is none; may be >= tiles_y: clamp)
template <class P>
__host__ __device__ __forceinline__ int band_last_owned_upto(const P& fp, int t)
{
    if (!fp.banded) return t;
    if (t < fp.band_first) return -1;
    const int d = t - fp.band_first, k = band_quot(fp, d), j = d - k * fp.band_stride;
    return k * fp.band_block + (j < fp.band_block ? j : fp.band_block - 1);
}

// inclusive scan of one uint32 per thread across a workgroup of WAVES waves (s_tmp: WAVES words); ends with a barrier
template <int WAVES = 4>
__device__ __forceinline__ uint32_t block_incl_scan(uint32_t v, uint32_t* s_tmp, uint32_t& total)
{
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    if (lane == 63) s_tmp[w] = v;
    __syncthreads();
    uint32_t off = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        uint32_t s = s_tmp[k];
        if (k < w) off += s;
        total += s;
    }
    __syncthreads();
    return v + off;
}

// last index i <= hi with tab[i] <= x (tab ascending, tab[0] <= x): binary search of a fixed number of steps, 2^STEPS > hi
template <int STEPS>
__device__ __forceinline__ uint32_t last_le(const uint32_t* tab, uint32_t x, uint32_t hi)
{
    uint32_t lo = 0;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (tab[mid] <= x) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// elements a pass walks: the count an earlier kernel left on the device (d_n) or a static one, at most n_cap
__device__ __forceinline__ uint32_t active_count(const uint32_t* d_n, uint32_t n_static, uint32_t n_cap) { return min(d_n ? *d_n : n_static, n_cap); }

// ------------------------------------------------------------------------------------------
// Target pixel formats: the values of MSPLAT_FB_* (include/msplat.h).  The compositors take the format as a template constant that
// only load_px / store_px look at: the accumulators are fp32 in every instantiation and the inner loops never see it.
constexpr int kFbF32 = 0, kFbF16 = 1, kFbUnorm8 = 2, kFbSrgb8 = 3;

// sRGB8 -> linear (GL 4.6 8.24): entry k = (float)decode((double)((float)k / 255.0f)), decode(c) = c <= 0.04045 ? c / 12.92 :
// ((c + 0.055) / 1.055)^2.4 in double.  tests/fb8_rule.py restates it; tests/test_fb8.py compares the two tables.
static __device__ const float kSrgb8Decode[256] = {
    0.0f, 0.000303526991f, 0.000607053982f, 0.000910580973f, 0.00121410796f, 0.00151763496f, 0.00182116195f, 0.00212468882f,
    0.00242821593f, 0.00273174304f, 0.00303526991f, 0.00334653584f, 0.00367650739f, 0.00402471703f, 0.00439144205f, 0.00477695372f,
    0.00518151699f, 0.00560539216f, 0.00604883349f, 0.00651209103f, 0.00699541066f, 0.00749903219f, 0.00802319311f, 0.00856812578f,
    0.00913405884f, 0.00972121768f, 0.010329823f, 0.0109600946f, 0.0116122449f, 0.0122864889f, 0.0129830325f, 0.0137020834f,
    0.0144438446f, 0.0152085163f, 0.0159962941f, 0.0168073773f, 0.017641956f, 0.0185002219f, 0.0193823632f, 0.0202885643f,
    0.0212190114f, 0.0221738853f, 0.0231533684f, 0.024157634f, 0.0251868609f, 0.0262412224f, 0.0273208935f, 0.02842604f,
    0.0295568351f, 0.0307134446f, 0.0318960324f, 0.0331047662f, 0.0343398079f, 0.0356013142f, 0.0368894525f, 0.0382043719f,
    0.0395462364f, 0.0409151986f, 0.0423114114f, 0.043735031f, 0.045186203f, 0.0466650873f, 0.0481718257f, 0.0497065671f,
    0.0512694642f, 0.0528606512f, 0.0544802807f, 0.0561284944f, 0.0578054376f, 0.0595112443f, 0.0612460598f, 0.063010022f,
    0.0648032725f, 0.0666259453f, 0.0684781745f, 0.0703601018f, 0.0722718537f, 0.0742135718f, 0.0761853904f, 0.0781874284f,
    0.0802198276f, 0.0822827145f, 0.0843762159f, 0.0865004659f, 0.088655591f, 0.090841718f, 0.0930589661f, 0.0953074694f,
    0.0975873545f, 0.0998987332f, 0.10224174f, 0.104616493f, 0.107023105f, 0.109461717f, 0.111932434f, 0.114435382f,
    0.116970673f, 0.119538434f, 0.122138776f, 0.124771819f, 0.127437681f, 0.130136475f, 0.13286832f, 0.135633335f,
    0.138431624f, 0.141263291f, 0.144128472f, 0.147027269f, 0.149959788f, 0.152926162f, 0.155926466f, 0.158960834f,
    0.162029386f, 0.165132195f, 0.168269396f, 0.171441108f, 0.174647406f, 0.177888423f, 0.18116425f, 0.18447499f,
    0.187820777f, 0.191201687f, 0.194617838f, 0.198069319f, 0.20155625f, 0.205078736f, 0.208636865f, 0.212230757f,
    0.215860531f, 0.219526231f, 0.223227978f, 0.226965904f, 0.23074007f, 0.23455061f, 0.238397598f, 0.242281154f,
    0.246201351f, 0.25015831f, 0.254152119f, 0.258182883f, 0.262250692f, 0.266355634f, 0.270497829f, 0.274677336f,
    0.278894305f, 0.283148766f, 0.287440866f, 0.291770667f, 0.296138287f, 0.300543815f, 0.304987341f, 0.309468955f,
    0.313988745f, 0.318546802f, 0.323143244f, 0.327778131f, 0.332451552f, 0.337163657f, 0.341914445f, 0.346704096f,
    0.351532638f, 0.356400162f, 0.361306816f, 0.366252631f, 0.371237695f, 0.376262158f, 0.38132605f, 0.386429459f,
    0.391572505f, 0.396755248f, 0.401977807f, 0.407240242f, 0.412542641f, 0.417885095f, 0.423267692f, 0.428690523f,
    0.434153676f, 0.439657211f, 0.445201218f, 0.450785816f, 0.456411034f, 0.462077022f, 0.467783809f, 0.473531514f,
    0.479320198f, 0.48514995f, 0.491020888f, 0.496933013f, 0.502886474f, 0.50888133f, 0.514917672f, 0.520995617f,
    0.527115166f, 0.533276439f, 0.539479494f, 0.545724511f, 0.55201143f, 0.55834043f, 0.564711511f, 0.571124852f,
    0.577580452f, 0.584078431f, 0.590618849f, 0.597201824f, 0.603827357f, 0.610495567f, 0.617206573f, 0.623960435f,
    0.630757153f, 0.637596905f, 0.644479692f, 0.651405632f, 0.658374846f, 0.665387332f, 0.672443151f, 0.679542482f,
    0.686685324f, 0.693871796f, 0.701101899f, 0.708375812f, 0.715693533f, 0.723055124f, 0.730460763f, 0.73791045f,
    0.745404243f, 0.752942204f, 0.760524511f, 0.768151164f, 0.775822222f, 0.783537805f, 0.791297972f, 0.799102724f,
    0.806952298f, 0.814846575f, 0.822785735f, 0.830769897f, 0.838799f, 0.846873224f, 0.854992628f, 0.863157213f,
    0.871367097f, 0.8796224f, 0.887923121f, 0.896269381f, 0.904661179f, 0.913098633f, 0.921581864f, 0.930110872f,
    0.938685715f, 0.947306514f, 0.955973327f, 0.964686275f, 0.973445296f, 0.982250571f, 0.991102099f, 1.0f,
};

// the code an 8-bit unorm target stores for x (msplat.h: PresentRGBA8's rule, rop_store's rule): clamp -- NaN and -inf to 0, +inf to 1 --
// then an fp32 multiply, an fp32 add (-ffp-contract=off keeps them apart) and truncation
__device__ __forceinline__ uint32_t unorm8_code(float x)
{
    const float v = x > 0.0f ? (x > 1.0f ? 1.0f : x) : 0.0f;
    return (uint32_t)(v * 255.0f + 0.5f);
}

// ... and for an sRGB-encoded channel (LinearToSRGB, util.cpp:357-367): e = 12.92 v below 0.0031308, else 1.055 v^(1/2.4) - 0.055 with
// the power as exp2(log2(v) / 2.4) on the transcendental unit (v is a normal number there).  The contract is a margin, not bits:
// |255 e - code| <= 0.5 + 2^-10 against e in double (~1 ulp each for v_log_f32 and v_exp_f32, |log2 v| < 8.4: about 1e-4 of a code)
__device__ __forceinline__ uint32_t srgb8_code(float x)
{
    const float v = x > 0.0f ? (x > 1.0f ? 1.0f : x) : 0.0f;
    const float e = v <= 0.0031308f ? 12.92f * v : 1.055f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(v) * (1.0f / 2.4f)) - 0.055f;
    return (uint32_t)(e * 255.0f + 0.5f);
}

// stores one pixel of a target row in the format FMT (kFb*).  8-bit targets: one dword per pixel, bytes R G B A in memory order
template <int FMT>
__device__ __forceinline__ void store_px(void* row, int x, const float4 px)
{
    if (FMT == kFbF16) {
        union { _Float16 h[4]; uint2 u; } pk;
        pk.h[0] = (_Float16)px.x; pk.h[1] = (_Float16)px.y; pk.h[2] = (_Float16)px.z; pk.h[3] = (_Float16)px.w;
        ((uint2*)row)[x] = pk.u;
    } else if (FMT == kFbUnorm8) {
        ((uint32_t*)row)[x] = unorm8_code(px.x) | (unorm8_code(px.y) << 8) | (unorm8_code(px.z) << 16) | (unorm8_code(px.w) << 24);
    } else if (FMT == kFbSrgb8) {
        ((uint32_t*)row)[x] = srgb8_code(px.x) | (srgb8_code(px.y) << 8) | (srgb8_code(px.z) << 16) | (unorm8_code(px.w) << 24);
    } else {
        ((float4*)row)[x] = px;
    }
}

// reads one pixel of a target row (MSPLAT_TARGET_LOAD's destination) as fp32.  8-bit targets: (float)code / 255.0f, an fp32 division;
// the sRGB target's colour channels through the decode table, its alpha is linear
template <int FMT>
__device__ __forceinline__ float4 load_px(const void* row, int x)
{
    if (FMT == kFbF16) {
        union { _Float16 h[4]; uint2 u; } in;
        in.u = ((const uint2*)row)[x];
        return make_float4((float)in.h[0], (float)in.h[1], (float)in.h[2], (float)in.h[3]);
    } else if (FMT == kFbUnorm8) {
        const uint32_t w = ((const uint32_t*)row)[x];
        return make_float4((float)(w & 255u) / 255.0f, (float)((w >> 8) & 255u) / 255.0f, (float)((w >> 16) & 255u) / 255.0f,
                           (float)(w >> 24) / 255.0f);
    } else if (FMT == kFbSrgb8) {
        const uint32_t w = ((const uint32_t*)row)[x];
        return make_float4(kSrgb8Decode[w & 255u], kSrgb8Decode[(w >> 8) & 255u], kSrgb8Decode[(w >> 16) & 255u], (float)(w >> 24) / 255.0f);
    } else {
        return ((const float4*)row)[x];
    }
}

// Workgroup b is observed to run on XCD b % 8 (MI355X_MICROARCH.md; speed only, never correctness).
// Remap so that each XCD processes a CONTIGUOUS range of chunks.  Measured r1: using it for the
// scatter kernels (radix/bin1 downsweep) was 5-15 % SLOWER than the plain round-robin mapping.  Today ws_downsweep uses it
// whenever its grid allows, radix_downsweep<MODE_PAIR> and bin1_downsweep on request (do_order bit 1, xcd_map == 1): see ws_downsweep.
__device__ __forceinline__ uint32_t xcd_contiguous(uint32_t b, uint32_t n)
{
    const uint32_t q = n >> 3, r = n & 7u, xcd = b & 7u, idx = b >> 3;
    const uint32_t base = xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
    return base + idx;
}

// Largest eigenvalue of the symmetric 3x3 with diagonal a00 a11 a22 and off-diagonal a01 a02 a12: the trigonometric closed form,
// in double.  Junk in, junk out (NaN, or a value above the trace of a matrix that is not PSD): each caller orders the result
// against its own fallback.
__host__ __device__ inline double sym3_lambda_max(double a00, double a11, double a22, double a01, double a02, double a12)
{
    const double tr = a00 + a11 + a22, q = tr / 3.0;
    const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
    const double p2 = (a00 - q) * (a00 - q) + (a11 - q) * (a11 - q) + (a22 - q) * (a22 - q) + 2.0 * p1;
    double lmax = q;
    if (p2 > 0.0) {
        const double p = sqrt(p2 / 6.0);
        const double b00 = (a00 - q) / p, b11 = (a11 - q) / p, b22 = (a22 - q) / p, b01 = a01 / p, b02 = a02 / p, b12 = a12 / p;
        double r = 0.5 * (b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02));
        r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
        lmax = q + 2.0 * p * cos(acos(r) / 3.0);
    }
    return lmax;
}

// FrameParams::view_scale2: an upper bound of sigma_max(W)^2 for W = mat3(view), the factor by which the camera matrix can
// stretch a world-space length -- |J_row W|^2 <= |J_row|^2 sigma_max(W)^2 holds for ANY W, so the culls built on it are sound for
// every invertible camera matrix (scaled, squashed, sheared), not only rigid ones.  (The largest squared column norm of W, used
// at first, is a LOWER bound of sigma_max^2 and equals it only for a rotation times a uniform scale: a camera squashed along one
// axis lost visible splats to the band cull.)  Largest eigenvalue of W^T W in double; when the closed form's result is not
// finite or not between the largest column norm^2 and the Frobenius norm^2 (it lies between them), the Frobenius norm^2: never
// below sigma_max^2, NaN / inf for a matrix that holds one.  + 1e-6, which covers the rounding to float.  0 for W = 0.
__host__ inline float view_scale2_of(const float view[16])
{
    double g[3][3], frob = 0.0, colmax = 0.0;                 // g = W^T W (view[4 c + r]: column c, row r)
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            g[a][b] = (double)view[4 * a] * view[4 * b] + (double)view[4 * a + 1] * view[4 * b + 1] + (double)view[4 * a + 2] * view[4 * b + 2];
    for (int a = 0; a < 3; ++a) {
        frob += g[a][a];
        colmax = g[a][a] > colmax ? g[a][a] : colmax;
    }
    double lmax = sym3_lambda_max(g[0][0], g[1][1], g[2][2], g[0][1], g[0][2], g[1][2]);
    if (!(lmax >= colmax * (1.0 - 1e-9) && lmax <= frob * (1.0 + 1e-9))) lmax = frob;
    return (float)(lmax * (1.0 + 1e-6));
}

// World-space footprint bound of a splat, kept in pos4.w for the band-restricted cull: rho^2 * lambda_max(Sigma) with
// rho^2 = 2 ln(256 alpha) (the fragment shader's discard radius) -- every projected variance M Sigma M^T is at most |M|^2 times
// the largest eigenvalue.  (r1-r3 used trace(Sigma), 1.7x the radius of an isotropic splat: a rank of an 8-way row-sharded
// frame then kept 17 % of the visible splats for 12.5 % of the rows.)  Closed form for a symmetric 3x3, in double, + 1e-5.
// S = Sigma as stored: column-major 3x3 (S[3c + r]).  0 when alpha <= 1/256 (the splat can never pass the discard test).
__host__ __device__ inline float footprint_bound(const float* S, float alpha)
{
    const float rho2 = 2.0f * logf(256.0f * alpha);
    if (!(rho2 > 0.0f)) return 0.0f;
    const double a00 = S[0], a11 = S[4], a22 = S[8];
    const double a01 = 0.5 * ((double)S[1] + S[3]), a02 = 0.5 * ((double)S[2] + S[6]), a12 = 0.5 * ((double)S[5] + S[7]);
    const double tr = a00 + a11 + a22;
    double lmax = sym3_lambda_max(a00, a11, a22, a01, a02, a12);
    if (!(lmax <= tr)) lmax = tr;                       // NaN / negative-eigenvalue junk: fall back to the trace (also a bound for PSD)
    if (!(lmax >= 0.0)) lmax = 0.0;
    // never 0 for a splat that can be drawn: a zero (or underflowing) covariance still has the 0.3-pixel low-pass footprint, and
    // "bound == 0" means exactly "alpha <= 1/256" to the band cull and the two-pass gate
    const float bnd = (float)((double)rho2 * lmax * (1.0 + 1e-5));
    return bnd > 1.17549435e-38f ? bnd : 1.17549435e-38f;
}

// ------------------------------------------------------------------------------------------
// Cloud storage (msplat_set_cloud_storage; mirrors MSPLAT_STORAGE_*).  FP32: the padded records of 16 (full SH) or 8 float4 with
// the reference's float order.  SH_FP16: a 16-float fp32 head -- x y z alpha, DC r g b, Sigma[9] -- bit for bit the FP32 values,
// then the f_rest slots of the FP32 record as IEEE fp16 (band 1 of r g b first, so a degree-1 record is a prefix of a full one),
// two per dword, low half first; zero padding to 10 (full SH: 160 B) or 6 float4 (degree 1: 96 B).
// The conversions are integer bit operations: they do not depend on a wave's denorm mode and keep fp16 subnormals both ways.
// SH_Q8 (full SH only; a degree-1 cloud is stored FP32): the same 16-float head, then three fp32 steps -- one per SH band, shared by
// r g b -- then the 45 f_rest values as one-byte codes (two's complement, in sh16_half_slot order, four per dword, low byte first)
// and zero padding to 8 float4: 128 B, one cache line per splat.  Value = (float)code * step of the value's band (sh8_pack).
// ------------------------------------------------------------------------------------------
constexpr int kStorageFp32 = 0, kStorageShFp16 = 1, kStorageShQ8 = 3;
__host__ __device__ constexpr int cloud_f4(int storage, bool full_sh)
{
    if (storage == kStorageShQ8 && full_sh) return 8;
    return storage == kStorageShFp16 ? (full_sh ? 10 : 6) : (full_sh ? 16 : 8);
}
__host__ __device__ constexpr int sh16_count(bool full_sh) { return full_sh ? 45 : 9; }
// fp32 record float of head slot h (0..15) and of half h (0..44)
__host__ __device__ constexpr int sh16_head_slot(int h) { return h < 4 ? h : (h < 7 ? 4 + 4 * (h - 4) : 16 + (h - 7)); }
__host__ __device__ constexpr int sh16_half_slot(int h) { return h < 9 ? 5 + 4 * (h / 3) + h % 3 : 25 + (h - 9); }

// round to nearest even, like numpy.float16 (subnormals included); NaN keeps its sign and top payload bits
__host__ __device__ inline uint32_t f32_to_f16_bits(uint32_t x)
{
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a > 0x7F800000u) {
        const uint32_t m = (a >> 13) & 0x3FFu;
        return sign | 0x7C00u | (m ? m : 1u);
    }
    if (a >= 0x477FF000u) return sign | 0x7C00u;                  // >= 65520 (and inf): inf
    if (a >= 0x38800000u) return sign | ((a - 0x38000000u + 0xFFFu + ((a >> 13) & 1u)) >> 13);   // normal fp16
    if (a <= 0x33000000u) return sign;                            // <= 2^-25: zero (2^-25 itself is the tie with 0)
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u, s = 126u - (a >> 23);      // subnormal fp16: m * 2^-s units of 2^-24
    uint32_t q = m >> s;
    const uint32_t rem = m & ((1u << s) - 1u), half = 1u << (s - 1u);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    return sign | q;
}

__host__ __device__ inline uint32_t f16_bits_to_f32_bits(uint32_t h)
{
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    if (e == 31u) return sign | 0x7F800000u | (m << 13);
    if (e != 0u) return sign | (((h & 0x7FFFu) << 13) + 0x38000000u);
    // subnormal or zero: m * 2^-24 exactly, built from m's leading bit (2^-24 .. 2^-15 are normal fp32 numbers)
    if (m == 0u) return sign;
    const uint32_t k = 31u - (uint32_t)__builtin_clz(m);          // m = 1.f * 2^k
    return sign | ((103u + k) << 23) | ((m << (23u - k)) & 0x7FFFFFu);
}

__host__ __device__ inline uint32_t f32_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
__host__ __device__ inline float f32_from_bits(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }

// FP32 record floats f[] -> the SH_FP16 record w[cloud_f4(kStorageShFp16, FULL_SH) * 4]; returns the number of finite f_rest values
// that fp16 cannot hold (|c| >= 65520 rounds to inf)
template <bool FULL_SH>
__host__ __device__ inline uint32_t sh16_pack(const float* f, uint32_t* w)
{
    constexpr int NW = cloud_f4(kStorageShFp16, FULL_SH) * 4, NH = sh16_count(FULL_SH);
    uint32_t over = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = f32_bits(f[sh16_head_slot(k)]);
#pragma unroll
    for (int j = 0; j < NW - 16; ++j) {
        uint32_t v = 0u;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int h = 2 * j + p;
            if (h < NH) {
                const uint32_t x = f32_bits(f[sh16_half_slot(h)]), a = x & 0x7FFFFFFFu;
                over += (a >= 0x477FF000u && a < 0x7F800000u) ? 1u : 0u;
                v |= f32_to_f16_bits(x) << (16 * p);
            }
        }
        w[16 + j] = v;
    }
    return over;
}

// the inverse: fills the 16 head slots and the f_rest slots of an FP32 record f[] (padding slots are left alone)
template <bool FULL_SH>
__host__ __device__ inline void sh16_unpack(const uint32_t* w, float* f)
{
    constexpr int NH = sh16_count(FULL_SH);
#pragma unroll
    for (int k = 0; k < 16; ++k) f[sh16_head_slot(k)] = f32_from_bits(w[k]);
#pragma unroll
    for (int h = 0; h < NH; ++h) f[sh16_half_slot(h)] = f32_from_bits(f16_bits_to_f32_bits((w[16 + h / 2] >> (16 * (h & 1))) & 0xFFFFu));
}

// SH band (0..2 = degree 1..3) of half h: sh16_half_slot order is band 1 of r g b, then per channel 5 values of band 2 and 7 of band 3
__host__ __device__ constexpr int sh8_band(int h) { return h < 9 ? 0 : ((h - 9) % 12 < 5 ? 1 : 2); }

// the correctly rounded fp32 quotient, written out on the device like every division of the projection
__host__ __device__ inline float sh8_div(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// FP32 record floats f[] -> the SH_Q8 record w[32]; returns the number of non-finite f_rest values (their codes are 0: the upload
// fails).  Per band: m = max |c|; m < 2^-64: step 0, codes 0 (so that no quotient depends on a wave's denorm mode); else
// step = m / 127 and code = clamp(rint(c / step), -127, 127), halves to even.
template <bool FULL_SH>
__host__ __device__ inline uint32_t sh8_pack(const float* f, uint32_t* w)
{
    static_assert(FULL_SH, "SH_Q8 records exist for full-SH clouds only");
    constexpr int NH = sh16_count(true);
    uint32_t bad = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = f32_bits(f[sh16_head_slot(k)]);
    float m[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const uint32_t a = f32_bits(f[sh16_half_slot(h)]) & 0x7FFFFFFFu;
        bad += a >= 0x7F800000u ? 1u : 0u;
        const float av = f32_from_bits(a);
        m[sh8_band(h)] = av > m[sh8_band(h)] ? av : m[sh8_band(h)];      // (a NaN never becomes the maximum)
    }
    float step[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        step[b] = m[b] < 0x1p-64f ? 0.0f : sh8_div(m[b], 127.0f);
        w[16 + b] = f32_bits(step[b]);
    }
#pragma unroll
    for (int j = 0; j < 13; ++j) w[19 + j] = 0u;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const float c = f[sh16_half_slot(h)], st = step[sh8_band(h)];
        float q = st > 0.0f && st < 3.0e38f ? rintf(sh8_div(c, st)) : 0.0f;      // (an infinite step: a band with +-inf in it)
        q = q < -127.0f ? -127.0f : (q > 127.0f ? 127.0f : q);
        const int code = q == q ? (int)q : 0;
        w[19 + h / 4] |= ((uint32_t)code & 0xFFu) << (8 * (h & 3));
    }
    return bad;
}

// the inverse: fills the 16 head slots and the f_rest slots of an FP32 record f[] (padding slots are left alone)
template <bool FULL_SH>
__host__ __device__ inline void sh8_unpack(const uint32_t* w, float* f)
{
    static_assert(FULL_SH, "SH_Q8 records exist for full-SH clouds only");
#pragma unroll
    for (int k = 0; k < 16; ++k) f[sh16_head_slot(k)] = f32_from_bits(w[k]);
#pragma unroll
    for (int h = 0; h < sh16_count(true); ++h) {
        const int code = (int)(w[19 + h / 4] << (24 - 8 * (h & 3))) >> 24;      // sign-extended byte h
        f[sh16_half_slot(h)] = (float)code * f32_from_bits(w[16 + sh8_band(h)]);
    }
}

// Milder form: only GROUPS of g consecutive chunks share an XCD (workgroups p and p + 8 of every block of 8 g, which are
// dispatched right after one another): the partial cache lines at the seams between the runs that g neighbouring chunks write
// next to each other are then merged in that XCD's L2 before they go to HBM, without giving each XCD one long region of the
// output.  Identity on the last, incomplete block.
__device__ __forceinline__ uint32_t xcd_grouped(uint32_t b, uint32_t n, uint32_t g)
{
    const uint32_t blk = 8u * g, p = b % blk, base = b - p;
    if (base + blk > n) return b;
    return base + (p & 7u) * g + (p >> 3);
}

// presort_compute.glsl:38-55.  Operation order identical to oracle/msplat_oracle.c (orc_cull_key)
// so that keys and the visible set are bit-exact.
// BAND = false (r6): an instantiation for frames WITHOUT the band-restricted cull (every single-GPU frame) -- the branch below
// keeps ~25 uniform values live (view rows, proj[5], the layout), which is what pushed pass 0's upsweep over the SGPR file.
template <bool BAND = true>
__device__ __forceinline__ bool cull_key(const float4 p, const FrameParams& fp, uint32_t& key)
{
    const float* m = fp.mvp;
    float px = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], p.x), __fmul_rn(m[4], p.y)), __fmul_rn(m[8], p.z)), m[12]);
    float py = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[1], p.x), __fmul_rn(m[5], p.y)), __fmul_rn(m[9], p.z)), m[13]);
    float pw = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[3], p.x), __fmul_rn(m[7], p.y)), __fmul_rn(m[11], p.z)), m[15]);
    float depth = pw;
    float xx = __fdiv_rn(px, depth);
    float yy = __fdiv_rn(py, depth);
    const float CLIP = 1.5f;
    if (depth > 0.0f && xx < CLIP && xx > -CLIP && yy < CLIP && yy > -CLIP) {
        if (BAND && fp.band_cull) {
            // Band-restricted cull (never active on a single GPU, where the reference's cull
            // must be reproduced exactly).  Conservative bound on the footprint's y half-extent:
            //   ey^2 = rho^2 (M1 Sigma M1^T + 0.3) <= |J1|^2 |W|^2 * (rho^2 lambda_max(Sigma)) + 0.3 rho^2_max,
            // p.w = rho^2 lambda_max(Sigma) precomputed at upload (footprint_bound; 0 when alpha <= 1/256: never visible).
            if (!(p.w > 0.0f)) return false;
            // (a bound, not parity arithmetic: v_rcp_f32 instead of IEEE divisions, the 1 ulp is inside the 0.2 % + 1.5 px margin)
            const float* v = fp.view;
            const float ty = v[1] * p.x + v[5] * p.y + v[9] * p.z + v[13];
            const float tz = v[2] * p.x + v[6] * p.y + v[10] * p.z + v[14];
            const float rtz = __builtin_amdgcn_rcpf(tz);
            const float jsy = 0.5f * fp.proj[5] * fp.H * rtz;
            const float tr = ty * rtz;
            const float j2 = jsy * jsy * (1.0f + tr * tr);
            const float ey = __builtin_amdgcn_sqrtf(j2 * fp.view_scale2 * p.w + 3.4f) * 1.002f + 1.5f;
            const float cy = 0.5f * (fp.H + yy * fp.H) + fp.Y0;
            const float y0 = fmaxf(cy - ey, 0.0f), y1 = fminf(cy + ey, fp.H - 1.0f);
            if (!(y0 <= y1)) return false;
            const int r0 = (int)y0 / kBin, r1 = (int)y1 / kBin;
            const int v0 = band_first_owned_from(fp, r0), v1 = min(band_last_owned_upto(fp, r1), fp.tiles_y - 1);
            if (v0 > v1) return false;                 // no owned row in [r0, r1]
        }
        float f = __fmul_rn(__fdiv_rn(depth, fp.zf), 4294967296.0f);
        uint32_t q = (f >= 4294967296.0f) ? 0xFFFFFFFFu : (uint32_t)f;
        key = 0xFFFFFFFFu - q;
        return true;
    }
    return false;
}

// ------------------------------------------------------------------------------------------
// Chunk-level cull over a spatially ordered cloud (round 4).
// The reference culls per splat over the whole cloud (presort_compute.glsl:31-57, dispatched over N at splatrenderer.cpp:188-189)
// and so does pass 0 of the sort -- which is all of its work when most of the cloud cannot be seen: a rank of a row-sharded
// frame keeps 17 % of the splats, a camera inside a scene 40 %.  Large clouds are therefore STORED in Morton order of their
// positions (msplat_device.hip, spatial_reorder; the storage order is the library's business: sorted indices are reported in
// upload numbering and msplat_get_storage_order exposes the permutation) and every kBoxSplats consecutive stored splats carry a
// bounding box.  When an earlier frame saw less than 70 % of the cloud, Sort starts with box_cull_kernel: one thread per box,
// the live boxes listed in storage order; pass 0 then runs over the LISTED boxes only -- its chunks are made of live boxes, so
// its work is proportional to what can be seen, not to N.  (First attempt, r4: a per-chunk mask of live 1024-splat boxes tested
// inside pass 0 -- exact, but no faster: 40-64 % of such boxes are live for a rank that sees 17 % of the splats, every chunk
// still ran all its phases, and the box test sat on each chunk's critical path.)
// box_live is CONSERVATIVE: it returns false only if cull_key returns false for every splat the box can contain, so the
// visible set and the keys are exactly those of the per-splat test, and the listed boxes keep storage order, so ties do too.
// ------------------------------------------------------------------------------------------
constexpr int kBoxSplats = 256;          // stored splats per bounding box (four wave rows): 8 / 16 / 32 boxes per pass-0 chunk
constexpr int kBoxGroup = 256;           // boxes per workgroup of box_cull_kernel = entries per segment of the live list
struct CullBox {                         // 32 bytes
    float4 lo;                           // min x, y, z of the finite positions; .w = max footprint bound (pos4.w) of the box
    float4 hi;                           // max x, y, z; .w read by no kernel (visibility_kernel: the box's hidden splats).  lo.x > hi.x: no finite position in the box
};

__device__ __forceinline__ bool box_live(const CullBox& b, const FrameParams& fp)
{
    if (!(b.lo.x <= b.hi.x)) return false;            // nothing finite inside: cull_key rejects NaN / inf positions (comparisons false)
    const float* m = fp.mvp;
    const float* v = fp.view;
    // clip coordinates are affine in the position: over the box every plane function takes its extremes at the corners
    float w_max = -INFINITY, w_min = INFINITY, w_mag = 0.0f;
    float xr_min = INFINITY, xl_max = -INFINITY, yt_min = INFINITY, yb_max = -INFINITY, xy_mag = 0.0f;
    float yy_min = INFINITY, yy_max = -INFINITY, tz_max = -INFINITY, ty_abs = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x = (c & 1) ? b.hi.x : b.lo.x, y = (c & 2) ? b.hi.y : b.lo.y, z = (c & 4) ? b.hi.z : b.lo.z;
        const float px = m[0] * x + m[4] * y + m[8] * z + m[12];
        const float py = m[1] * x + m[5] * y + m[9] * z + m[13];
        const float pw = m[3] * x + m[7] * y + m[11] * z + m[15];
        const float aw = fabsf(m[3] * x) + fabsf(m[7] * y) + fabsf(m[11] * z) + fabsf(m[15]);
        const float ax = fabsf(m[0] * x) + fabsf(m[4] * y) + fabsf(m[8] * z) + fabsf(m[12]);
        const float ay = fabsf(m[1] * x) + fabsf(m[5] * y) + fabsf(m[9] * z) + fabsf(m[13]);
        w_max = fmaxf(w_max, pw); w_min = fminf(w_min, pw); w_mag = fmaxf(w_mag, aw);
        xy_mag = fmaxf(xy_mag, fmaxf(ax, ay) + 1.5f * aw);
        xr_min = fminf(xr_min, px - 1.5f * pw);       // visible needs px / pw <  1.5  <=>  px - 1.5 pw < 0  (pw > 0)
        xl_max = fmaxf(xl_max, px + 1.5f * pw);       //                px / pw > -1.5  <=>  px + 1.5 pw > 0
        yt_min = fminf(yt_min, py - 1.5f * pw);
        yb_max = fmaxf(yb_max, py + 1.5f * pw);
        if (fp.band_cull) {
            yy_min = fminf(yy_min, py / pw); yy_max = fmaxf(yy_max, py / pw);       // meaningful only when w_min > 0 (below)
            tz_max = fmaxf(tz_max, v[2] * x + v[6] * y + v[10] * z + v[14]);
            ty_abs = fmaxf(ty_abs, fabsf(v[1] * x + v[5] * y + v[9] * z + v[13]));
        }
    }
    // margins: the per-splat test evaluates the same sums in fp32 in another order (a few ulp of the sum of magnitudes)
    const float ew = 1e-5f * w_mag, exy = 1e-5f * xy_mag;
    if (!(w_max > -ew)) return false;                 // every splat has depth <= 0 (or the box is NaN: then nothing passes either)
    if (xr_min > exy || xl_max < -exy || yt_min > exy || yb_max < -exy) return false;
    if (fp.band_cull) {
        if (!(b.lo.w > 0.0f)) return false;           // every splat has alpha <= 1/256: cull_key drops them under the band cull
        // the band test needs the whole box in front of the camera (y / w is monotone along every edge only there)
        if (w_min > ew && tz_max < 0.0f) {
            const float rtz = 1.0f / -tz_max;         // largest 1 / |tz| in the box
            const float jsy = 0.5f * fabsf(fp.proj[5]) * fp.H * rtz;
            const float tr = ty_abs * rtz;
            const float j2 = jsy * jsy * (1.0f + tr * tr);
            // cull_key: ey = sqrt(j2 view_scale2 p.w + 3.4) * 1.002 + 1.5 with 1-ulp rcp / sqrt: 0.2 % + 1 px on top
            const float ey = sqrtf(j2 * fp.view_scale2 * b.lo.w + 3.4f) * 1.004f + 2.5f;
            const float cy0 = 0.5f * (fp.H + yy_min * fp.H) + fp.Y0, cy1 = 0.5f * (fp.H + yy_max * fp.H) + fp.Y0;
            const float slack = 1e-4f * (fabsf(cy0) + fabsf(cy1) + fp.H);
            const float y0 = fmaxf(cy0 - ey - slack, 0.0f), y1 = fminf(cy1 + ey + slack, fp.H - 1.0f);
            if (!(y0 <= y1)) return false;
            const int r0 = (int)y0 / kBin, r1 = (int)y1 / kBin;
            const int v0 = band_first_owned_from(fp, r0), v1 = min(band_last_owned_upto(fp, r1), fp.tiles_y - 1);
            if (v0 > v1) return false;                // no owned bin row between the box's lowest and highest reach
        }
    }
    return true;
}

// The live boxes of the current Sort: workgroup g of box_cull_kernel leaves the live ones of its kBoxGroup boxes, ascending, in
// list[g * kBoxGroup ...] and their number in cnt[g] (g < wgs <= 256: up to 2^24 splats).  list == nullptr: no list, pass 0
// walks the whole cloud.
struct LiveBoxes {
    const uint32_t* list;
    const uint32_t* cnt;
    uint32_t wgs;
    uint32_t n_storage;                  // splats in the cloud (the last box may be partial)
};

__global__ __launch_bounds__(kBoxGroup) void box_cull_kernel(const CullBox* __restrict__ boxes, uint32_t nboxes, FrameParams fp,
                                                             uint32_t* __restrict__ list, uint32_t* __restrict__ cnt)
{
    __shared__ uint32_t s_w[kBoxGroup / 64];
    const uint32_t b = blockIdx.x * kBoxGroup + threadIdx.x;
    const bool l = b < nboxes && box_live(boxes[b], fp);
    const unsigned long long m = __ballot(l);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_w[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kBoxGroup / 64; ++k) {
        if (k < w) off += s_w[k];
        total += s_w[k];
    }
    if (l) list[blockIdx.x * kBoxGroup + off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = b;
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// exclusive prefix of the segment counts: s_lpre[g] = live boxes before segment g, s_lpre[256] = all of them.  Every thread of a
// workgroup of >= 256 threads must call it (WAVES = its waves; s_tmp: WAVES words).  Ends with a barrier.  Returns the number of
// virtual positions pass 0 walks: the listed boxes are dense there (the cloud's last box may be partial: LiveChunk's `in`).
template <int WAVES>
__device__ __forceinline__ uint32_t live_prefix(const LiveBoxes& lb, uint32_t* s_lpre, uint32_t* s_tmp)
{
    const uint32_t t = threadIdx.x;
    uint32_t v = (t < 256u && t < lb.wgs) ? lb.cnt[t] : 0u;
    const uint32_t c = v;
    const int lane = t & 63, w = t >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(v, d, 64);
        if (lane >= d) v += x;
    }
    if (lane == 63) s_tmp[w] = v;
    __syncthreads();
    uint32_t off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        const uint32_t x = s_tmp[k];
        if (k < w) off += x;
        total += x;
    }
    if (t < 256u) s_lpre[t] = v + off - c;
    if (t == 0u) s_lpre[256] = total;
    __syncthreads();
    return s_lpre[256] * (uint32_t)kBoxSplats;
}

// storage box number of the vb-th live box (0xFFFFFFFF beyond the last)
__device__ __forceinline__ uint32_t live_box_at(const LiveBoxes& lb, const uint32_t* s_lpre, uint32_t vb)
{
    if (vb >= s_lpre[256]) return 0xFFFFFFFFu;
    const uint32_t g = last_le<8>(s_lpre, vb, 255u);         // its segment
    return lb.list[g * kBoxGroup + (vb - s_lpre[g])];
}

// One chunk of pass 0: virtual positions first, first + 1, ... of n; with a list (compact) s_box holds the chunk's live boxes
// (live_box_at of chunk * boxes per chunk + 0, 1, ...).
struct LiveChunk {      // {lb, s_box, compact, first, n}: mind the order of the last two
    const LiveBoxes& lb;
    const uint32_t* s_box;
    bool compact;
    uint32_t first, n;
    // storage index of virtual position i (== i without a list); `in`: the position holds a splat
    __device__ __forceinline__ uint32_t storage_of(uint32_t i, bool& in) const
    {
        if (!compact) { in = i < n; return i; }
        const uint32_t e = i - first, bx = s_box[e / kBoxSplats], st = bx * kBoxSplats + (e % kBoxSplats);
        in = bx != 0xFFFFFFFFu && st < lb.n_storage;
        return st;
    }
};

// two-pass frames (msplat_occlusion.hip.h): first rank of pass 1 for V visible splats and a share of them in pass 1
__device__ __forceinline__ uint32_t occ_cut(uint32_t V, float share)
{
    uint32_t r1 = (uint32_t)((float)V * share);
    r1 = (r1 + 63u) & ~63u;
    if (r1 < 64u) r1 = 64u;
    const uint32_t cut = r1 >= V ? 0u : V - r1;
    return cut & ~1023u;                      // whole chunks of the column pass (and waves of the projection) lie on one side of it
}

}  // namespace msplat
