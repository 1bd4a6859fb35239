// msplat_composite.hip.h -- the compositors: work queue, front-to-back composite_kernel (GL rasteriser + shader/splat_frag.glsl + ROP blend) and the
// draw-order variant with an emulated depth buffer / render-target rounding
// (one of the parts of msplat_kernels.hip.h)
#pragma once

#include "msplat_common.hip.h"
#include "msplat_binning.hip.h"

#pragma clang fp contract(off)

namespace msplat {

// The compositors' work queue.  One queue head serves only ~90 returning atomics per microsecond (measured r2: a
// half-tile launch pulling 8 k items from one head spent ~90 us queueing), so the head is sharded: item i lives
// in shard i % 32, a workgroup pulls from the shard of its index and, when that one is drained, from up to two
// neighbours (checked with a plain load first, so drained shards are not hammered by the exiting waves).
// Where the items are numbered heaviest-first (every item on its own wave) every shard hands out its
// share heaviest-first too; persistent waves otherwise walk the bins in the XCD-local order of msplat_bin_order.h (`tile_order` +
// 2 * 65536; a probed frame: storage order, `tile_order` + 65536).  The first item
// of every workgroup is static (its own index): queue[s] counts only the items of shard s taken dynamically.
__device__ __forceinline__ uint32_t queue_next(uint32_t* __restrict__ queue, uint32_t nitems)
{
    const uint32_t home = blockIdx.x % kQueueShards;
    for (uint32_t t = 0; t < 3u; ++t) {
        const uint32_t s = (home + t) % kQueueShards;
        const uint32_t stat = (gridDim.x + kQueueShards - 1u - s) / kQueueShards;      // items of shard s taken statically
        uint32_t* head = queue + s * kQueueStride;
        if (t != 0u) {
            const uint32_t cur = __hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((uint64_t)(cur + stat) * kQueueShards + s >= nitems) continue;
        }
        const uint32_t k = atomicAdd(head, 1u) + stat;
        const uint64_t item = (uint64_t)k * kQueueShards + s;
        if (item < nitems) return (uint32_t)item;
    }
    return 0xFFFFFFFFu;
}

// 0, 1, 2, ...: storage order, the bin order of a probed frame's persistent compositor waves (filled once, at msplat_create)
__global__ __launch_bounds__(kThreads) void iota_kernel(uint32_t* __restrict__ dst)
{
    dst[blockIdx.x * kThreads + threadIdx.x] = blockIdx.x * kThreads + threadIdx.x;
}

// ------------------------------------------------------------------------------------------
// composite: one 16x16 workgroup per tile, front-to-back over the tile's depth-ordered list
// (reverse of the reference's back-to-front ROP blend; algebraically identical -- SURVEY 8a-12):
//   C = sum_i T_i w_i c_i,  T_i = prod_{j nearer}(1 - w_j),  A = 1
// splat_frag.glsl:18-42 defines w and the discard (w <= 1/256); app.cpp:153-160 the blend/clear.
// ------------------------------------------------------------------------------------------

constexpr int kCompThreads = 64;   // one wave per 16x16 tile, 4 pixels (one per 16x4 strip) per lane
constexpr int kCompOcc = 5;        // occupancy bound handed to the compiler (<= 102 VGPRs); the kernel needs 76, so 6 waves fit a SIMD (tools/kres.sh).
                                   // A bound of 6+ was measured slower (r3: the allocator then squeezes the inner loop), DESIGN.md 4

// Work item = (bin, quadrant): one wave composites one 16x16 tile of a 32x32 bin.  The kernel is VALU bound: 21.5 VALU
// instructions per record in the inner loop (12 packed, 4 v_exp_f32, 3 scalar FMAs: ~147 pipe cycles) and ~70 per staged
// batch.  Formulations that were built, measured and removed (numbers in DESIGN.md 4): four waves per tile with 8x8 sub-block
// queues (LDS-pipe bound), one wave per 16x8 half tile, per-strip-pair masks, 6-8 waves per SIMD.
// Discard by underflow: the fragment shader's discard (w <= 1/256, splat_frag.glsl:37-40) would cost a compare and a select
// per pixel.  Here it is free: the exponent is biased by -118, so that w' = exp2(e - 118) is a NORMAL float exactly when
// e >= -8 and underflows otherwise, and the wave runs with fp32 denormals flushed (MODE.FP_DENORM, set below): the
// underflowing weights come out of v_exp_f32 as exact zeros.  The transmittance is carried scaled by 2^118 (Ts = 2^118 T), so
// tw = Ts w' = T w exactly as before (powers of two), colours accumulate unchanged and Ts -= 2^118 tw.  The bias costs 4 bits
// of the exponent's absolute precision (|e - 118| ~ 2^7 instead of <= 2^3): a relative error of 3e-6 in w.  Only e == -8
// exactly (w == 1/256, which the reference discards) is kept: a measure-zero threshold flip.
// Template parameters instead of run-time arguments (r5): FMT = the target's pixel format (kFb*: load_px / store_px); OCC = 0 one
// pass, 1 / 2 the passes of a two-pass frame; TWO_VIEWS = both eyes in one chain; PROBE = per-item counters.  The plain frame's
// instantiation <FMT, 0, false, false>
// carries none of the others' registers (r4 passed them at run time on top of the ~500-byte FrameParams: 81 VGPRs / 14 SGPR spills
// against r3's 79 / 5) and takes the eleven words of CompParams instead of five 4x4 matrices.
// TM = MSPLAT_TARGET_* (msplat_set_target_mode): what the final store -- the one place that writes pixels -- does with the target's
// contents.  kTargetClear: (C, 1), the code of every instantiation that existed before the parameter.  The inner loop never sees it.
// DEPTH (msplat_render_depth): the frame also hands out a W x H float32 depth plane -- window depth as one more colour channel, blended
// over GL's clear depth 1.0 (app.cpp:160):  depth = sum_i T_i w_i z_i + T,  z_i = 0.5 ndc.z + 0.5 of splat i (project_kernel's out_zq with
// depth_bits = 32: the float's bits).  z rides in the free word of the staged record, the inner loop gains one packed FMA per strip pair
// and the final store writes the plane next to the colour, same lane, once.  DEPTH = false: the code of every instantiation that existed
// before the parameter.
// ZTEST (msplat_render_occluded): GL_LESS against a caller's W x H float32 plane of window depths (app.cpp:160-163: the reference draws its
// geometry first and blends the splats over it under GL_DEPTH_TEST).  Splat i -- one z_i per splat, as for DEPTH, in the same free word of the
// staged record -- is absent from pixel p unless z_i < plane[p].  Each lane keeps the plane's value of its four pixels (closed = -inf: outside
// the image, or NaN), the wave their maximum: a record with !(z < max) is dropped at staging (which moves no batch boundary: the two-pass cut
// stays where it is), and in the inner loop the weight of a pixel with !(z < plane) becomes an exact 0 -- a compare and a select per pixel after
// the v_exp_f32; a zero weight is an exact no-op on every accumulator, as for the discard by underflow.  A tile without an open pixel goes
// straight to its final store.  Pass 2 of a two-pass frame re-reads the plane: no new per-pixel state.  (Built and removed before any measurement: a second,
// untested copy of the loop chosen per batch by a scalar branch when every staged record lies in front of the tile's MINIMUM -- two pass-1
// instantiations then spilled VGPRs into scratch, EXPERIMENTS.md round 14.)  ZTEST = false: the code of every instantiation that existed before the parameter.
// DEPTH && ZTEST (msplat_render_layers): both at once -- the loop gains exactly what each adds, the depth plane is blended over the occluder's
// value d0 (clamped to [0, 1]) instead of the clear depth, from the zp registers the lane already holds: no new per-pixel state.  TWO_VIEWS takes
// the second view's planes from ex.occluder1 / ex.depth1, rows counted in the view's own ty.
constexpr int kTargetClear = 0, kTargetLoad = 1, kTargetPremultiplied = 2;      // MSPLAT_TARGET_* (include/msplat.h)
// The occupancy bound of an instantiation: kCompOcc, except for the one-view DEPTH && ZTEST forms of the single pass and of pass 2, which spilled
// 2-14 VGPRs into scratch under it (96 allocatable registers; pass 1 and the two-view form fit): those alone get 4 waves (EXPERIMENTS.md round 15)
constexpr int comp_occ(int occ, bool two_views, bool depth, bool ztest) { return depth && ztest && !two_views && occ != 1 ? 4 : kCompOcc; }
struct CompExtra {
    void* out1;                  // TWO_VIEWS: the second view's target (bin rows >= rows_view belong to it)
    uint32_t* fin;               // OCC != 0: per (bin, quadrant) 0xFFFFFFFF = final, else entries composited by pass 1
    float4* state;               // OCC != 0: (r, g, b, 2^118 T) per pixel of the tiles pass 1 leaves unfinished
    const uint32_t* d_nbins;     // OCC == 2: `order` lists *d_nbins bins -- the unfinished ones -- and the items are theirs alone
    uint32_t* probe;             // PROBE: 8 words per work item
    const float* zw;             // DEPTH: window depth per rank
    float* depth;                // DEPTH: the depth plane, rows of depth_pitch bytes (row 0 = GL bottom, like the colour)
    size_t depth_pitch;
    float* zstate;               // DEPTH, OCC != 0: the depth accumulator per pixel, beside `state`
    const float* occluder;       // ZTEST: the plane of window depths the splats are tested against (zw as for DEPTH), rows of occluder_pitch bytes
    size_t occluder_pitch;
    const float* occluder1;      // TWO_VIEWS: the second view's planes, as out1 is its target; each kind's pitch is shared by the views
    float* depth1;
};

template <int FMT, int OCC, bool TWO_VIEWS, bool PROBE, int TM = kTargetClear, bool DEPTH = false, bool ZTEST = false>
__global__ __launch_bounds__(kCompThreads, comp_occ(OCC, TWO_VIEWS, DEPTH, ZTEST)) void composite_kernel(const uint32_t* __restrict__ tile_start,
                                                                 const uint32_t* __restrict__ pairs,
                                                                 const float4* __restrict__ rec,
                                                                 void* __restrict__ out, size_t pitch_bytes,
                                                                 CompParams fp, uint32_t cap,
                                                                 const uint32_t* __restrict__ order,
                                                                 uint32_t* __restrict__ queue, uint32_t ntiles,
                                                                 int prio_levels, CompExtra ex)
{
    constexpr int occ_pass = OCC;
    MSPLAT_STAMP(KID_COMPOSITE);
    uint32_t* __restrict__ const fin = ex.fin;
    float4* __restrict__ const state = ex.state;
    uint32_t* __restrict__ const probe = PROBE ? ex.probe : nullptr;
    if (OCC == 2) ntiles = *ex.d_nbins * 4u;
    // Two-pass frame (msplat_occlusion.hip.h), occ_pass 1 / 2; fin[bin * 4 + quadrant] and state[y * width + x] = (r, g, b, 2^118 T)
    // carry a tile from one to the other.  Pass 1 walks WHOLE batches only: a tile whose strips are all saturated after one of
    // them is final (fin = 0xFFFFFFFF, pixels written); otherwise it stops in front of the first incomplete batch, leaves its
    // accumulators in `state` and the number of entries it composited in fin.  Pass 2 skips the final tiles and RESUMES the others
    // at that entry of their complete list.  Batches count from the list's end and pass 1's list is a suffix of the complete one,
    // so the walk is cut at a batch boundary of the single pass: same batches, same strip tests between them, same pixels.
    // Lane (lx, ly) owns pixels (x0+lx, y0 + 4k + ly), k = 0..3: strip k is the 16x4 pixel block of
    // rows 4k..4k+3.  Per splat the exponent is split into a part shared by the four strips and a
    // 2-FMA part per strip; strips the splat's y-range cannot reach, or whose 64 pixels are all
    // saturated, are skipped with scalar branches.
    __shared__ float4 s_rec[(kCompThreads + 1) * 3];
    // (r4, measured and removed: the exponents of four staged records at a time from the matrix pipe -- e is a K = 5 contraction
    //  of per-record coefficients with per-pixel monomials on top of c0; v_mfma_f32_4x4x1_16b_f32, 3.5 per record instead of 3
    //  scalar + 4 packed FMAs; bit-compatible images.  20 % fewer non-MFMA VALU instructions, and the launch 14 % LONGER (81 -> 92 us):
    //  the MFMAs take the same issue port, SQ_ACTIVE_INST_VALU fell by 4 % only.  DESIGN.md 4, profiles/r04_pmc_sq_compositor_mfma.txt)

    // Persistent waves + dynamic queue: per-tile work varies by >10x (list length, early saturation),
    // so tiles are pulled heaviest-first from `order` instead of being bound to a workgroup index.
    // The first tile of every wave is static (its workgroup index): same-address atomics are served
    // at only ~8 ns each, so thousands of waves pulling at launch would queue up for tens of us.
    // Work item = (bin, quadrant): the four 16x16 tiles of a 32x32 bin share the bin's list.
    constexpr float kBias = 118.0f;
    constexpr float kScale = 0x1p118f;
    __builtin_amdgcn_s_setreg(1 | (4 << 6) | ((2 - 1) << 11), 0);      // MODE[5:4] = 0: flush fp32 denormals
    constexpr int NP = 2;                            // strip pairs per work item (the whole 16x16 tile)
    constexpr int NS = 2 * NP;                       // 16x4 strips per work item
    constexpr int ROWS = 4 * NS;                     // pixel rows per work item
    for (uint32_t qpos = blockIdx.x; qpos < ntiles;) {
    const int tile = (int)qpos;                       // probe slot
    const uint32_t tpos = qpos;                       // (bin, quadrant) index
    // The four tiles of a bin walk the SAME list, and workgroup b runs on XCD b % 8 (each XCD has its own L2): inside every
    // group of 32 items the quadrants of one bin are the items r, r + 8, r + 16, r + 24, i.e. on one XCD, as the first
    // (static) item of a wave and -- shard = item % 32, home shard = workgroup % 32 -- as a pulled one.  Three of the four
    // waves then find the list words and records in their XCD's L2 instead of fetching them from HBM again.  XCD x therefore composites
    // the slots with slot % 8 == x, in ascending order, and `order` (msplat_bin_order.h) gives each such class compact blocks of bins:
    // the bins a splat covers meet its record in one L2.
    uint32_t slot = tpos >> 2, quadrant = tpos & 3u;
    if (tpos < (ntiles & ~31u)) {
        slot = (tpos >> 5) * 8u + (tpos & 7u);
        quadrant = (tpos >> 3) & 3u;
    }
    const int bin = (int)order[slot];
    const int quad = (int)quadrant;
    const int bvy = bin / fp.tiles_x;
    const int tx = (bin - bvy * fp.tiles_x) * 2 + (quad & 1);
    const bool second = TWO_VIEWS && bvy >= fp.rows_view;
    const int ty = (second ? bvy - fp.rows_view : band_real_row(fp, bvy)) * 2 + (quad >> 1);
    if (tx * kTile >= fp.width || ty * kTile >= fp.height || (occ_pass == 2 && fin[bin * 4 + quad] == 0xFFFFFFFFu)) {
        // work item entirely outside the image, or (pass 2 of a two-pass frame) the tile was finished by pass 1
        if (occ_pass == 1 && threadIdx.x == 0) fin[bin * 4 + quad] = 0xFFFFFFFFu;
        if (gridDim.x >= ntiles) break;
        uint32_t nq = 0;
        if (threadIdx.x == 0) nq = queue_next(queue, ntiles);
        qpos = __builtin_amdgcn_readfirstlane(nq);
        continue;
    }
    // The launch lasts as long as its heaviest work item (the probe: max / mean item clocks = 2.0, and the heaviest item
    // spans the whole launch although it starts first), because a wave that shares its SIMD with four others gets a
    // fifth of the issue slots.  Items are numbered heaviest-first, so the wave's issue priority follows the item
    // number: the heaviest thousand items run at the single-wave issue rate from the start and the light ones fill
    // the slots they leave (SIMD arbitration is priority first, then age -- MI355X_MICROARCH.md).
    if (prio_levels == 1) {
        const uint32_t band = max(ntiles >> 3, 1u);                    // an eighth of the items per priority step
        const uint32_t lvl = qpos / band;
        // (r5: one step only, kCompPrioMax = 1 -- the levels above it belong to the other frames' short kernels, msplat_common.hip.h)
        if (lvl <= 3u) __builtin_amdgcn_s_setprio(kCompPrioMax);
        else __builtin_amdgcn_s_setprio(0);
    }
    const int lane = threadIdx.x;
    const int lx = lane & 15, ly = lane >> 4;
    const int x = tx * kTile + lx, ybase = ty * kTile + ly;
    const float fx = (float)x + 0.5f;
    const float fy0 = (float)ybase + 0.5f;
    const float tile_y0 = (float)(ty * kTile);

    uint32_t start = tile_start[bin], end = tile_start[bin + 1];
    if (start > cap) start = cap;
    if (end > cap) end = cap;
    if (occ_pass == 2) end -= min(fin[bin * 4 + quad], end - start);       // resume: the entries pass 1 composited are the list's last

    // Accumulators are kept as strip PAIRS (0,1) and (2,3): gfx950 executes a plain wave64 fp32 VALU
    // op in ~4 cycles but a packed v_pk_{fma,mul,add}_f32 does two per lane in the same slot (measured:
    // SQ_ACTIVE_INST_VALU / SQ_INSTS_VALU = 4.4 cycles), and this kernel is VALU bound.
    typedef float v2f __attribute__((ext_vector_type(2)));
    v2f T[NP], cr[NP], cg[NP], cb[NP], cz[NP];      // cz: DEPTH only
    bool inside[NS];
#pragma unroll
    for (int h = 0; h < NP; ++h) {
        T[h] = (v2f){kScale, kScale};                // the transmittance scaled by 2^118
        cr[h] = (v2f){0.0f, 0.0f}; cg[h] = (v2f){0.0f, 0.0f}; cb[h] = (v2f){0.0f, 0.0f};
        cz[h] = (v2f){0.0f, 0.0f};
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) inside[k] = (x < fp.width) && (ybase + 4 * k < fp.height);
    v2f zp[NP];                                      // ZTEST only: the plane at the lane's pixels, -inf where nothing passes
    if (ZTEST) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            float v = -__builtin_inff();
            if (inside[k]) v = ((const float*)((const char*)(second ? ex.occluder1 : ex.occluder) + (size_t)(ybase + 4 * k) * ex.occluder_pitch))[x];
            zp[k >> 1][k & 1] = v == v ? v : -__builtin_inff();      // NaN: closed
        }
    }
    if (occ_pass == 2) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            if (inside[k]) {
                const float4 st = state[(size_t)(ybase + 4 * k) * fp.width + x];
                cr[k >> 1][k & 1] = st.x; cg[k >> 1][k & 1] = st.y; cb[k >> 1][k & 1] = st.z; T[k >> 1][k & 1] = st.w;
                if (DEPTH) cz[k >> 1][k & 1] = ex.zstate[(size_t)(ybase + 4 * k) * fp.width + x];
            }
        }
    }
    // The exponent is evaluated as a polynomial in TILE-CENTRED pixel coordinates (|u|, |v| <= 7.5: no cancellation in u
    // and v; c0 itself cancels far from the splat's centre and is compensated there, below): e(u, v) = c0 + c1 u + c2 v + c3 u^2 + c4 u v + c5 v^2, coefficients per staged record.  Per record and lane
    // that is 3 scalar FMAs for the u part plus 2 packed FMAs per strip pair -- the centre-relative form (dx, dy, base,
    // lin) needed 4 + 3: 162 instead of 186 VALU pipe cycles per record.
    const float xc = (float)(tx * kTile) + 0.5f * (float)kTile, yc = tile_y0 + 0.5f * (float)ROWS;
    const float u = fx - xc;
    v2f vp[NP];
#pragma unroll
    for (int h = 0; h < NP; ++h) vp[h] = (v2f){fy0 + 8.0f * h - yc, fy0 + 8.0f * h + 4.0f - yc};
    uint32_t alive = 0;
#pragma unroll
    for (int k = 0; k < NS; ++k)
        alive |= (__ballot(inside[k] && (occ_pass != 2 || T[k >> 1][k & 1] >= fp.t_eps * kScale)) != 0ull) ? (1u << k) : 0u;

    // Three-stage software pipeline over batches of 64 list entries (nearest first):
    //   ranks of batch b+2 and records of batch b+1 are in flight while batch b is composited,
    // so a tile whose entries are mostly culled pays one memory latency per batch instead of two
    // dependent ones (that latency chain, not ALU work, is the critical path of the long tiles).
    uint32_t hiA = end;                                        // entries [start, hiA) not yet rank-loaded
    uint32_t cntA = min((uint32_t)kCompThreads, hiA - start);  // batch whose ranks are in rankA
    // rankA holds the RAW pair word; the rank mask is applied where the word is used.  Masking right after the
    // load made the compiler wait (s_waitcnt vmcnt(0)) for it -- and with it for the record loads issued just
    // before -- in front of the inner loop: the whole prefetch pipeline was serialised (27 % of the kernel).
    uint32_t rankA = 0;
    if (lane < (int)cntA) rankA = pairs[hiA - 1u - lane];     // j = 0 is the nearest splat
    hiA -= cntA;
    uint32_t cnt = cntA;                                       // batch whose records are in p0..p2
    float4 p0 = make_float4(0, 0, 0, 0), p1 = p0, p2 = p0;
    float pz = 0.0f;                                           // DEPTH: the window depth that travels with the record
    if (lane < (int)cnt) {
        uint32_t rk = rankA & kRankMask;
        asm volatile("" : "+v"(rk));              // keep the mask out of the address arithmetic (see composite_depth_kernel)
        const float4* src = rec + (size_t)rk * 3;
        p0 = src[0]; p1 = src[1]; p2 = src[2];
        if (DEPTH || ZTEST) pz = ex.zw[rk];
    }
    cntA = min((uint32_t)kCompThreads, hiA - start);
    if (lane < (int)cntA) rankA = pairs[hiA - 1u - lane];
    hiA -= cntA;
    float tile_zmax = 0.0f;                                    // ZTEST: the most distant plane value of the tile
    if (ZTEST) {
        // (here, behind the first record loads: the plane's loads were issued before them and the reduction waits for those alone)
        tile_zmax = fmaxf(fmaxf(zp[0].x, zp[0].y), fmaxf(zp[1].x, zp[1].y));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) tile_zmax = fmaxf(tile_zmax, __shfl_xor(tile_zmax, d, 64));
        tile_zmax = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, tile_zmax)));
        if (!(tile_zmax > 0.0f)) alive = 0;                    // z_w >= 0: no splat passes anywhere in the tile
    }
    const uint64_t probe_t0 = PROBE ? clock64() : 0ull;
    uint32_t probe_n = 0, probe_batches = 0, probe_useful = 0;      // probe_useful: (pixel, record) evaluations with w > 0
    uint64_t probe_inner = 0;
    // pair words / records whose loads have been issued so far (the prefetch pipeline runs two / one batches ahead)
    uint32_t probe_words = min(end - start, 2u * (uint32_t)kCompThreads), probe_recs = cnt;
    uint32_t consumed = 0;                            // (pass 1) entries composited: whole batches
    while (cnt != 0u && alive != 0u && !(occ_pass == 1 && cnt < (uint32_t)kCompThreads)) {
        consumed += cnt;
        // stage: every lane turns its list entry into the coefficients of e(u, v) in tile-centred coordinates and tests
        // it against the tile; the survivors are compacted into LDS in list order (near to far).  Straight-line code on
        // purpose: the CU has ONE scalar unit for its four SIMDs and this is the dependent chain between two batches --
        // the branchy form (per-strip y tests, the exact test under an EXEC mask) was ~115 VALU + ~80 scalar instructions
        // per batch, this one is ~60 + ~15.
        uint32_t n;
        {
            constexpr float U = 0.5f * (float)(kTile - 1);          // box of pixel centres: |u| <= U, |v| <= Vh
            constexpr float Vh = 0.5f * (float)(ROWS - 1);
            const float a = p0.x - xc, b = p0.y - yc;               // splat centre, tile-centred
            const float qa = p0.z, qb = p0.w, qc = p1.x;            // c3, c4, c5
            const float Aa = qa * a, Bb = qb * b, Cb = qc * b, Ba = qb * a;
            const float c1 = __builtin_fmaf(-2.0f, Aa, -Bb);
            const float c2 = __builtin_fmaf(-2.0f, Cb, -Ba);
            // c0 = (A a + B b) a + C b b + log2 alpha - 118 (the exponent bias rides on log2 alpha).  Its quadratic terms are as large as
            // |A| a^2 and cancel for a long thin splat that crosses the tile far from its centre (a 45-degree needle of short variance
            // 0.5 px^2 at 2000 px: terms of 1.4e6, an ulp of 0.125; plain float32 left 0.06 ... 0.2 of error in e, more than the 0.05
            // slack of the test below and 6 % in w: DESIGN.md 4).  A batch that holds a record more than kFarCentre px from the tile's
            // centre (wave-uniform: one ballot) therefore COMPENSATES the sum: every product and the two sums that cancel carry their
            // exact float32 residue (fma(x, y, -xy); Knuth's two-sum), the residues are added at the end.  Nearer than that the terms
            // stay below 1.2e5 (|A| <= 2.41: the 0.3 px^2 floor of the covariance) and the plain form is good to 8e-3.
            constexpr float kFarCentre = 128.0f;
            float c0 = __builtin_fmaf(Aa + Bb, a, __builtin_fmaf(Cb, b, p1.y - kBias));
            if (__ballot(lane < (int)cnt && (fabsf(a) > kFarCentre || fabsf(b) > kFarCentre)) != 0ull) {
                const float rAa = __builtin_fmaf(qa, a, -Aa), rBb = __builtin_fmaf(qb, b, -Bb), rCb = __builtin_fmaf(qc, b, -Cb);
                const float s = Aa + Bb, sv = s - Aa;
                const float rs = (Aa - (s - sv)) + (Bb - sv);                    // Aa + Bb = s + rs
                const float p = s * a, q = Cb * b;
                const float rp = __builtin_fmaf(s, a, -p), rq = __builtin_fmaf(Cb, b, -q);
                const float t = p + q, tv = t - p;
                const float rt = (p - (t - tv)) + (q - tv);                      // p + q = t + rt
                const float tail = __builtin_fmaf((rs + rAa) + rBb, a, __builtin_fmaf(rCb, b, (rp + rq) + rt));
                c0 = (t + (p1.y - kBias)) + tail;
            }
            // y reach of the footprint against the strips that are still live (strip k: v in [4k - Vh, 4k + 3 - Vh])
            const float vlo = b - p2.w, vhi = b + p2.w;
            bool rel = lane < (int)cnt && vhi >= -Vh && vlo <= Vh;
            if (alive != (1u << NS) - 1u) {                          // wave-uniform; only once strips have saturated
                bool any = false;
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    any = any || ((alive & (1u << k)) && vhi >= 4.0f * k - Vh && vlo <= 4.0f * k + 3.0f - Vh);
                rel = rel && any;
            }
            // exact footprint-vs-tile test (the list was built from bounding rectangles): e is a concave quadratic, so
            // unless the centre lies inside the box its maximum over the box is on one of the four edges (1-D maximiser,
            // clamped).  v_rcp_f32 instead of IEEE divisions: the maximiser only has to be good to the 0.05 slack below.
            const bool inside_box = fabsf(a) <= U && fabsf(b) <= Vh;
            const float i2c = -0.5f * __builtin_amdgcn_rcpf(qc), i2a = -0.5f * __builtin_amdgcn_rcpf(qa);
            const float ku = __builtin_fmaf(qa, U * U, c0), kv = __builtin_fmaf(qc, Vh * Vh, c0);
            float emax;
            {
                const float lp = __builtin_fmaf(qb, U, c2), lm = __builtin_fmaf(qb, -U, c2);       // edges u = +-U
                const float kp = __builtin_fmaf(c1, U, ku), km = __builtin_fmaf(c1, -U, ku);
                const float vp = fminf(fmaxf(lp * i2c, -Vh), Vh), vm = fminf(fmaxf(lm * i2c, -Vh), Vh);
                const float ep = __builtin_fmaf(__builtin_fmaf(qc, vp, lp), vp, kp);
                const float em = __builtin_fmaf(__builtin_fmaf(qc, vm, lm), vm, km);
                const float mp = __builtin_fmaf(qb, Vh, c1), mm = __builtin_fmaf(qb, -Vh, c1);    // edges v = +-Vh
                const float hp = __builtin_fmaf(c2, Vh, kv), hm = __builtin_fmaf(c2, -Vh, kv);
                const float up = fminf(fmaxf(mp * i2a, -U), U), um = fminf(fmaxf(mm * i2a, -U), U);
                const float fp_ = __builtin_fmaf(__builtin_fmaf(qa, up, mp), up, hp);
                const float fm_ = __builtin_fmaf(__builtin_fmaf(qa, um, mm), um, hm);
                emax = fmaxf(fmaxf(ep, em), fmaxf(fp_, fm_));
            }
            rel = rel && (inside_box || emax > -8.05f - kBias);
            if (ZTEST) rel = rel && pz < tile_zmax;                  // behind the whole tile's plane
            const uint64_t relmask = __ballot(rel);
            n = (uint32_t)__popcll(relmask);
            if (rel) {
                const int slot = __popcll(relmask & ((1ull << lane) - 1ull));
                // the four values the packed instructions broadcast (c5, r, g, b) sit at even dwords of the 16-byte reads: they
                // land in even VGPRs, which a packed operand can name directly (an odd one costs a v_mov)
                s_rec[slot * 3 + 0] = make_float4(qc, c0, p1.z, c1);
                s_rec[slot * 3 + 1] = make_float4(p1.w, c2, p2.x, qa);
                s_rec[slot * 3 + 2] = make_float4(qb, DEPTH || ZTEST ? pz : 0.0f, 0.0f, 0.0f);
            }
        }
        __syncthreads();
        cnt = cntA;
        if (lane < (int)cnt) {
            uint32_t rk = rankA & kRankMask;
            asm volatile("" : "+v"(rk));
            const float4* src = rec + (size_t)rk * 3;
            p0 = src[0]; p1 = src[1]; p2 = src[2];
            if (DEPTH || ZTEST) pz = ex.zw[rk];
        }
        cntA = min((uint32_t)kCompThreads, hiA - start);
        if (lane < (int)cntA) rankA = pairs[hiA - 1u - lane];
        hiA -= cntA;
        probe_n += n;
        ++probe_batches;
        probe_words += cntA;
        probe_recs += cnt;
        const uint64_t probe_t1 = PROBE ? clock64() : 0ull;
        if (n != 0u) {
            float4 a = s_rec[0];          // c5, c0, r, c1
            float4 b = s_rec[1];          // g, c2, b, c3
            float c4 = s_rec[2].x;
            float z = DEPTH || ZTEST ? s_rec[2].y : 0.0f;
#pragma unroll 2
            for (uint32_t j = 0; j < n; ++j) {
                // next record (slot n is a harmless over-read inside the 65-slot array)
                const float4 na = s_rec[(j + 1) * 3 + 0];
                const float4 nb = s_rec[(j + 1) * 3 + 1];
                const float nc4 = s_rec[(j + 1) * 3 + 2].x;
                const float nz = DEPTH || ZTEST ? s_rec[(j + 1) * 3 + 2].y : 0.0f;
                const float base = __builtin_fmaf(__builtin_fmaf(b.w, u, a.w), u, a.y);      // c0 + c1 u + c3 u^2
                const float lin = __builtin_fmaf(c4, u, b.y);                                // c2 + c4 u
                const v2f vbase = (v2f){base, base}, vlin = (v2f){lin, lin}, vC = (v2f){a.x, a.x};
                const v2f vr = (v2f){a.z, a.z}, vg = (v2f){b.x, b.x}, vb = (v2f){b.z, b.z};
                const v2f vz = (v2f){z, z};
                // Branch-free on purpose: the strips are independent dependency chains inside one basic
                // block, so the in-order wave can overlap them.  w = 0 where the fragment shader discards.
#pragma unroll
                for (int h = 0; h < NP; ++h) {
                    const v2f e = __builtin_elementwise_fma(vp[h], __builtin_elementwise_fma(vC, vp[h], vlin), vbase);
                    // splat_frag.glsl:37-40 discard: w = exp2(e) > 1/256  <=>  e > -8
                    v2f w;           // discard by underflow (see the kernel's header)
                    w.x = __builtin_amdgcn_exp2f(e.x);
                    w.y = __builtin_amdgcn_exp2f(e.y);
                    if (ZTEST) {     // GL_LESS against the plane: the fragment is not blended
                        w.x = z < zp[h].x ? w.x : 0.0f;
                        w.y = z < zp[h].y ? w.y : 0.0f;
                    }
                    if (PROBE) probe_useful += (w.x > 0.0f ? 1u : 0u) + (w.y > 0.0f ? 1u : 0u);      // per lane; summed over the wave at the end
                    const v2f tw = T[h] * w;
                    cr[h] = __builtin_elementwise_fma(tw, vr, cr[h]);
                    cg[h] = __builtin_elementwise_fma(tw, vg, cg[h]);
                    cb[h] = __builtin_elementwise_fma(tw, vb, cb[h]);
                    if (DEPTH) cz[h] = __builtin_elementwise_fma(tw, vz, cz[h]);
                    T[h] = __builtin_elementwise_fma(tw, (v2f){-kScale, -kScale}, T[h]);
                }
                a = na; b = nb; c4 = nc4; z = nz;
            }
        }
        if (PROBE) probe_inner += clock64() - probe_t1;
        // strips whose 64 pixels are all saturated (or outside the image) are finished
        uint32_t na = 0;
#pragma unroll
        for (int k = 0; k < NS; ++k)
            na |= (__ballot(inside[k] && T[k >> 1][k & 1] >= fp.t_eps * kScale) != 0ull) ? (1u << k) : 0u;
        alive = na;
        __syncthreads();
    }

    // (pass 1 of a two-pass frame) final, or to be resumed by pass 2?
    const bool carry = occ_pass == 1 && alive != 0u;
    if (occ_pass == 1 && lane == 0) fin[bin * 4 + quad] = carry ? consumed : 0xFFFFFFFFu;
    if (PROBE) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) probe_useful += (uint32_t)__shfl_xor((int)probe_useful, d, 64);
    }
    if (PROBE && lane == 0) {
        probe[tile * 8 + 0] = (uint32_t)(clock64() - probe_t0);        // shader clocks, whole tile
        probe[tile * 8 + 1] = probe_n;          // splats composited (after culling / saturation)
        probe[tile * 8 + 2] = probe_batches;    // batches of 64 list entries staged
        probe[tile * 8 + 3] = (uint32_t)probe_inner;   // shader clocks spent in the inner loops
        probe[tile * 8 + 4] = probe_words;      // 4-byte pair words loaded
        probe[tile * 8 + 5] = probe_recs;       // 48-byte projected records loaded
        probe[tile * 8 + 6] = end - start;      // length of the bin list
        probe[tile * 8 + 7] = 1u + probe_useful;      // != 0: the work item ran; - 1 = evaluations whose weight survived the discard (w > 0)
    }
    if (carry) {
#pragma unroll
        for (int k = 0; k < NS; ++k)
            if (inside[k])
                state[(size_t)(ybase + 4 * k) * fp.width + x] = make_float4(cr[k >> 1][k & 1], cg[k >> 1][k & 1], cb[k >> 1][k & 1], T[k >> 1][k & 1]);
        if (DEPTH) {
#pragma unroll
            for (int k = 0; k < NS; ++k)
                if (inside[k]) ex.zstate[(size_t)(ybase + 4 * k) * fp.width + x] = cz[k >> 1][k & 1];
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        if (inside[k] && !carry) {
            char* row = (char*)(second ? ex.out1 : out) + (size_t)(ybase + 4 * k) * pitch_bytes;
            float4 px = make_float4(cr[k >> 1][k & 1], cg[k >> 1][k & 1], cb[k >> 1][k & 1], 1.0f);
            bool keep = false;
            if (TM != kTargetClear) {
                // the GL blend (GL_ONE, GL_ONE_MINUS_SRC_ALPHA, app.cpp:154-156) is linear in the destination: over dst the frame is
                // C + T dst, alpha 1 - T (1 - dst.a).  T = 2^-118 Ts is exact; the forms keep an opaque dst opaque.  The pixel is read
                // and written once, by this lane.
                const float t = T[k >> 1][k & 1] * 0x1p-118f;
                if (TM == kTargetPremultiplied) {
                    px.w = 1.0f - t;
                } else {
                    const float4 d = load_px<FMT>(row, x);
                    px.x = __builtin_fmaf(t, d.x, px.x);
                    px.y = __builtin_fmaf(t, d.y, px.y);
                    px.z = __builtin_fmaf(t, d.z, px.z);
                    px.w = __builtin_fmaf(t, d.w - 1.0f, 1.0f);
                    // A pixel no splat reached (t == 1: every weight was 0, so C is 0 too) is handed through as it is: the formulas
                    // would round d.w - 1 for |d.w| < 0.5, turn -0 into +0 and -- this wave flushes fp32 denormals -- a denormal into 0
                    // (an 8-bit target's pixel is not stored at all: its four bytes stay, whatever decode and encode would make of them)
                    if (t == 1.0f) { px = d; keep = FMT == kFbUnorm8 || FMT == kFbSrgb8; }
                }
                // RGBA16F: the value is rounded to fp32 and THEN to half in every mode -- left alone, the compiler may fold an fma or
                // subtraction and the conversion into one v_fma_mixlo_f16 (a single rounding to half: LOAD over zeros then differed
                // from PREMULTIPLIED by an fp16 ulp in a few pixels per frame)
                if (FMT == kFbF16) asm volatile("" : "+v"(px.x), "+v"(px.y), "+v"(px.z), "+v"(px.w));
            }
            if (!keep) store_px<FMT>(row, x, px);
            if (DEPTH) {
                // expected window depth over the clear depth 1.0: the blend of kTargetLoad with colour z and dst = 1 (T = 2^-118 Ts is
                // exact; a pixel no splat reached reads exactly 1).  Every z is <= 1 and the weights sum to 1 - T, but the partial sums
                // are rounded: the minimum keeps the plane inside [0, 1] when z_w sits at 1
                // DEPTH && ZTEST (msplat_render_layers): over what the depth attachment holds instead, d0 = the plane's value clamped to
                // [0, 1] by the 8-bit targets' rule -- from the registers the test ran on (-inf: closed or NaN, gives 0), read before this
                // store: the plane may be the occluder's own memory.  One fma, so that d0 = 1 rounds like the sum above
                float* zrow = (float*)((char*)(second ? ex.depth1 : ex.depth) + (size_t)(ybase + 4 * k) * ex.depth_pitch);
                if (ZTEST) {
                    const float o = zp[k >> 1][k & 1];
                    const float d0 = o > 0.0f ? (o > 1.0f ? 1.0f : o) : 0.0f;
                    zrow[x] = fminf(__builtin_fmaf(T[k >> 1][k & 1] * 0x1p-118f, d0, cz[k >> 1][k & 1]), 1.0f);
                } else {
                    zrow[x] = fminf(cz[k >> 1][k & 1] + T[k >> 1][k & 1] * 0x1p-118f, 1.0f);
                }
            }
        }
    }
    __syncthreads();      // s_rec is reused by the next tile
    if (gridDim.x >= ntiles) break;       // every work item has its own wave: nothing to pull, no exit atomic
    uint32_t nq = 0;
    if (threadIdx.x == 0) nq = queue_next(queue, ntiles);
    qpos = __builtin_amdgcn_readfirstlane(nq);
    }   // persistent tile loop
}

// ------------------------------------------------------------------------------------------
// composite with an emulated depth buffer.  The reference enables GL_DEPTH_TEST
// (app.cpp:163, GL_LESS, depth writes on); it is live whenever the target has a depth attachment
// (default back buffer, XR swapchains) and inert for the colour-only --fp16/--fp32 FBO that the
// main compositor models.  With a depth buffer a fragment that survives the discard also has to
// pass z < zbuf and then writes its z: splats whose quantised depths tie, or that are drawn out
// of depth order (second XR eye re-using the first eye's sort), lose their later fragments.
// Whether a fragment passes depends on everything drawn BEFORE it, so this variant walks the list
// in draw order (far to near) with the literal "over" blend and cannot terminate early.
//
// The same draw-order walk also emulates what the render target does to the running colour (fp.rop, SURVEY 8a-12,
// src/app.cpp:1012-1020): the default RGBA8 back buffer clamps source, destination and result to [0,1] and stores 8-bit
// unorm after EVERY blend (GL 4.6 17.3.6), the --fp16 target rounds to fp16 after every blend; the main compositor
// accumulates in fp32 and rounds once.  fp.depth_bits = 0 then means "no depth test".
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float rop_store(float x, int rop)
{
    if (rop == 1) return floorf(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f + 0.5f) / 255.0f;
    if (rop == 2) return (float)(_Float16)x;            // round to nearest even, like the fp16 target
    return x;
}

// a lane's four pixels (x, ybase + 4k), one per 16x4 strip, in the draw-order compositors: running colour and alpha, emulated depth buffer
struct DrawPixels { float cr[4], cg[4], cb[4], ca[4]; uint32_t zbuf[4]; };

// The draw-order tile walk of composite_depth_kernel and composite_points_kernel (one wave per 16x16 tile, lists walked far to near
// in batches of 64, single-head queue).  The kernel declares the LDS (s_rec: kCompThreads * 3, s_z: kCompThreads) and supplies
// initial(px, x, ybase): what the cleared pixels start from; relevant(p0, p1, p2, X0, X1, Y0, Y1): can the record touch a pixel
// centre of the tile; shade(px, r, zj, fx, ybase): blends the staged record r[0..2] of depth zj into the lane's pixels;
// final_alpha(px, k): the alpha stored with pixel k.  depth_test: the records' quantised depths zq[rank] are staged too.
// FMT: the target's pixel format (kFb*).  KEEP_UNTOUCHED (MSPLAT_TARGET_LOAD into an 8-bit target): a pixel no fragment wrote -- its
// emulated depth is still the clear value: a fragment that writes leaves its own, smaller one -- is not stored, its bytes stay.
template <int FMT, bool KEEP_UNTOUCHED, class Initial, class Relevant, class Shade, class FinalAlpha>
__device__ __forceinline__ void draw_order_walk(const uint32_t* __restrict__ tile_start, const uint32_t* __restrict__ pairs,
                                                const float4* __restrict__ rec, const uint32_t* __restrict__ zq, bool depth_test,
                                                void* __restrict__ out, size_t pitch_bytes, const FrameParams& fp, uint32_t cap,
                                                const uint32_t* __restrict__ order, uint32_t* __restrict__ queue, uint32_t ntiles,
                                                float4* s_rec, uint32_t* s_z,
                                                Initial initial, Relevant relevant, Shade shade, FinalAlpha final_alpha)
{
    const int lane = threadIdx.x, lx = lane & 15, ly = lane >> 4;
    for (uint32_t qpos = blockIdx.x; qpos < ntiles;) {
        const int bin = (int)order[qpos >> 2], quad = (int)(qpos & 3u);
        const int bvy = bin / fp.tiles_x;
        const int tx = (bin - bvy * fp.tiles_x) * 2 + (quad & 1);
        const int ty = band_real_row(fp, bvy) * 2 + (quad >> 1);
        if (tx * kTile < fp.width && ty * kTile < fp.height) {
            const int x = tx * kTile + lx, ybase = ty * kTile + ly;
            const float fx = (float)x + 0.5f;
            const uint32_t start = min(tile_start[bin], cap), end = min(tile_start[bin + 1], cap);
            DrawPixels px;
#pragma unroll
            for (int k = 0; k < 4; ++k) { px.cr[k] = 0.0f; px.cg[k] = 0.0f; px.cb[k] = 0.0f; px.ca[k] = 0.0f; px.zbuf[k] = 0xFFFFFFFFu; }   // cleared to 1.0
            initial(px, x, ybase);
            const float X0 = (float)(tx * kTile) + 0.5f, X1 = X0 + (float)(kTile - 1);
            const float Y0 = (float)(ty * kTile) + 0.5f, Y1 = Y0 + (float)(kTile - 1);
            for (uint32_t base = start; base < end; base += kCompThreads) {      // ascending = draw order
                const uint32_t cnt = min((uint32_t)kCompThreads, end - base);
                float4 p0 = make_float4(0, 0, 0, 0), p1 = p0, p2 = p0;
                uint32_t z = 0;
                bool rel = false;
                if (lane < (int)cnt) {
                    uint32_t rank = pairs[base + lane] & kRankMask;
                    // hipcc 7.2 (gfx950) folds "(x & 0xFFFFFF) * 48 + base" in ONE basic block into v_mad_u64_u32
                    // on the UNMASKED word (mul24 known-bits combine; seen in the ISA, faulted on the GPU): keep
                    // the masked value opaque.  composite_kernel masks in a different block and is not affected.
                    asm volatile("" : "+v"(rank));
                    const float4* src = rec + (size_t)rank * 3;
                    p0 = src[0]; p1 = src[1]; p2 = src[2];
                    if (depth_test) z = zq[rank];
                    rel = relevant(p0, p1, p2, X0, X1, Y0, Y1);
                }
                const uint64_t relmask = __ballot(rel);
                const uint32_t n = (uint32_t)__popcll(relmask);
                if (rel) {
                    const int slot = __popcll(relmask & ((1ull << lane) - 1ull));     // keeps draw order
                    s_rec[slot * 3 + 0] = p0; s_rec[slot * 3 + 1] = p1; s_rec[slot * 3 + 2] = p2;
                    s_z[slot] = z;
                }
                __syncthreads();
                for (uint32_t j = 0; j < n; ++j) shade(px, s_rec + j * 3, s_z[j], fx, ybase);
                __syncthreads();
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (x < fp.width && ybase + 4 * k < fp.height && !(KEEP_UNTOUCHED && px.zbuf[k] == 0xFFFFFFFFu)) {
                    char* row = (char*)out + (size_t)(ybase + 4 * k) * pitch_bytes;
                    store_px<FMT>(row, x, make_float4(px.cr[k], px.cg[k], px.cb[k], final_alpha(px, k)));
                }
            }
        }
        uint32_t nq = 0;
        if (threadIdx.x == 0) nq = atomicAdd(queue, 1u);
        qpos = gridDim.x + __builtin_amdgcn_readfirstlane(nq);
    }
}

// TM (msplat_set_target_mode, MSPLAT_ROP_NONE only): kTargetLoad starts the running colour AND alpha from the target's pixel, the
// draw-order blend then runs over it (a = w + (1 - w) a); kTargetPremultiplied starts from (0, 0, 0, 0).  The emulated depth buffer
// is cleared to 1.0 either way: the target's contents lie behind every splat.
template <int FMT, int TM = kTargetClear>
__global__ __launch_bounds__(kCompThreads) void composite_depth_kernel(const uint32_t* __restrict__ tile_start, const uint32_t* __restrict__ pairs,
                                                                       const float4* __restrict__ rec, const uint32_t* __restrict__ zq,
                                                                       void* __restrict__ out, size_t pitch_bytes, FrameParams fp, uint32_t cap,
                                                                       const uint32_t* __restrict__ order, uint32_t* __restrict__ queue, uint32_t ntiles)
{
    __shared__ float4 s_rec[kCompThreads * 3];
    __shared__ uint32_t s_z[kCompThreads];
    auto initial = [&](DrawPixels& px, int x, int ybase) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (TM == kTargetLoad && x < fp.width && ybase + 4 * k < fp.height) {
                const char* row = (const char*)out + (size_t)(ybase + 4 * k) * pitch_bytes;
                const float4 d = load_px<FMT>(row, x);
                px.cr[k] = d.x; px.cg[k] = d.y; px.cb[k] = d.z; px.ca[k] = d.w;
            }
        }
    };
    // same exact footprint-vs-tile test as composite_kernel
    auto relevant = [](const float4& p0, const float4& p1, const float4&, float X0, float X1, float Y0, float Y1) -> bool {
        const float qa = p0.z, qb = p0.w, qc = p1.x, la = p1.y;
        const float dxl = X0 - p0.x, dxh = X1 - p0.x, dyl = Y0 - p0.y, dyh = Y1 - p0.y;
        if (dxl <= 0.0f && dxh >= 0.0f && dyl <= 0.0f && dyh >= 0.0f) return true;
        float emax = -1e30f;
        const float i2c = __builtin_amdgcn_rcpf(2.0f * qc), i2a = __builtin_amdgcn_rcpf(2.0f * qa);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float dx = s ? dxh : dxl;
            const float dy = fminf(fmaxf(-qb * dx * i2c, dyl), dyh);
            emax = fmaxf(emax, (qc * dy + qb * dx) * dy + qa * dx * dx + la);
            const float ey = s ? dyh : dyl;
            const float ex = fminf(fmaxf(-qb * ey * i2a, dxl), dxh);
            emax = fmaxf(emax, (qa * ex + qb * ey) * ex + qc * ey * ey + la);
        }
        return emax > -8.05f;
    };
    auto shade = [&](DrawPixels& px, const float4* r, uint32_t zj, float fx, int ybase) {
        const float4 a = r[0];      // px, py, A, B
        const float4 b = r[1];      // C, log2(alpha), r, g
        const float blue = r[2].x;
        const float dx = fx - a.x;
        const float base_e = __builtin_fmaf(a.z * dx, dx, b.y);
        const float lin = a.w * dx;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dy = ((float)(ybase + 4 * k) + 0.5f) - a.y;
            const float e = __builtin_fmaf(dy, __builtin_fmaf(b.x, dy, lin), base_e);
            // splat_frag.glsl:37-40 discard, then GL_LESS against the emulated depth buffer
            if (e > -8.0f && (fp.depth_bits == 0 || zj < px.zbuf[k])) {
                const float w = __builtin_amdgcn_exp2f(e);
                // splat_frag.glsl:27-28: out = (w rgb, w); GL_ONE, GL_ONE_MINUS_SRC_ALPHA
                float sr = w * b.z, sg = w * b.w, sb = w * blue;
                if (fp.rop == 1) {      // fixed-point target: the source colour is clamped before the blend
                    sr = fminf(fmaxf(sr, 0.0f), 1.0f); sg = fminf(fmaxf(sg, 0.0f), 1.0f); sb = fminf(fmaxf(sb, 0.0f), 1.0f);
                }
                const float oma = 1.0f - w;
                px.cr[k] = rop_store(sr + oma * px.cr[k], fp.rop);
                px.cg[k] = rop_store(sg + oma * px.cg[k], fp.rop);
                px.cb[k] = rop_store(sb + oma * px.cb[k], fp.rop);
                if (TM != kTargetClear) px.ca[k] = w + oma * px.ca[k];
                px.zbuf[k] = zj;
            }
        }
    };
    auto final_alpha = [](const DrawPixels& px, int k) -> float { return TM != kTargetClear ? px.ca[k] : 1.0f; };
    constexpr bool keep_untouched = TM == kTargetLoad && (FMT == kFbUnorm8 || FMT == kFbSrgb8);
    draw_order_walk<FMT, keep_untouched>(tile_start, pairs, rec, zq, fp.depth_bits != 0, out, pitch_bytes, fp, cap, order, queue, ntiles,
                                         s_rec, s_z, initial, relevant, shade, final_alpha);
}

}  // namespace msplat
