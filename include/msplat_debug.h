/*
 * msplat_debug.h -- parity-test taps, probes and experiment handles of libmsplat.so.  Nothing here is needed to bind
 * SplatRenderer::Sort / Render (that is msplat.h); these entry points let tests/ compare intermediate results with the oracle,
 * let bench.py count what the compositor fetched, and let a test pin what the library otherwise steers by itself.
 * All of them synchronise the context.
 */
#ifndef MSPLAT_DEBUG_H
#define MSPLAT_DEBUG_H

#include "msplat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- intermediate results of the latest Render ---- */
/* per draw-order rank r < V: 12 floats {px, py, A, B, C, log2(alpha), r, g, b, alpha, 0, 0} with
 * w(dx, dy) = exp2(A dx^2 + B dx dy + C dy^2 + log2 alpha); rect = bin rectangle tx0 | ty0<<8 | tx1<<16 | ty1<<24 (tx0 > tx1: empty) */
int msplat_debug_get_projected(msplat_ctx* ctx, float* rec12, uint32_t* rect, uint32_t cap);
/* the same for one view of the latest Render -- view 1: the second eye of msplat_render_stereo, whose ranks follow the first eye's at
 * V rounded up to 64 -- and for `count` ranks from the view's first one, which may be more than V: what lies beyond V is what the
 * buffers held before (fails when the buffers are smaller).  rect as the binning reads it: the second view's bin rows follow the
 * first's */
int msplat_debug_get_projected_view(msplat_ctx* ctx, int32_t view, float* rec12, uint32_t* rect, uint32_t count);
/* fills both buffers, whole: every byte of the records with `byte`, every rectangle with the empty rectangle 0xFF | byte << 8.
 * With the getter above tests/test_gpu_projection_limits.py shows that a projection writes its V ranks and nothing behind them */
int msplat_debug_fill_projected(msplat_ctx* ctx, int32_t byte);
/* tile_start has tiles_x * tiles_y + 1 entries; pairs[k] & 0xFFFFFF = draw-order rank.  After a two-pass Render both (and
 * msplat_get_stats().pairs / drawn) describe the SECOND pass */
int msplat_debug_get_tile_lists(msplat_ctx* ctx, uint32_t* tile_start, uint32_t tile_cap, uint32_t* pairs, uint64_t pair_cap);
/* on-device self-check of the ordering contracts (sorted keys ascending, ties by ascending storage slot; every bin list
 * ascending in draw-order rank): violation counts, both 0 on a healthy context.  Guards the lane-ordered LDS-atomic ranking,
 * which msplat_create probes but the hardware does not document (msplat_config.rank_mode = MSPLAT_RANK_BALLOT selects the ballot path) */
int msplat_debug_verify_order(msplat_ctx* ctx, uint32_t* key_violations, uint32_t* list_violations);
/* chunk-level cull for the latest Sort's camera: live / all bounding boxes (of 256 stored splats; 0 / 0 for a cloud in upload
 * order); *listed (may be NULL) = 1 when that Sort's first pass walked only the listed live boxes.  The boxes are the ones that Sort
 * used: under msplat_set_visibility / msplat_set_crop the context's own, built over the visible splats */
int msplat_debug_get_cull_boxes(msplat_ctx* ctx, uint32_t* live, uint32_t* total, int* listed);

/* ---- the conservative culls (band cull per splat and per box, the two-pass gate) bound a splat's reach by
 * |J_row|^2 * view_scale2 * rho^2 lambda_max(Sigma): view_scale2 as every frame computes it from viewMat = inverse(cameraMat)
 * (msplat_mat4_inverse), an upper bound of the squared spectral norm of its upper-left 3x3, at most 1e-5 above it (relative).
 * Host arithmetic: no context, no device ---- */
int msplat_debug_view_scale2(const float viewMat[16], float* out);

/* ---- two-pass frames (msplat_config.two_pass) ---- */
/* share > 0 pins the share of the visible splats in the first pass (any value gives the same pixels), 0 hands it back to the
 * feedback loop.  two_pass_frames: Renders of the context that ran in two passes; share_now: what the next one would use */
int msplat_debug_two_pass(msplat_ctx* ctx, float share, uint64_t* two_pass_frames, float* share_now);
/* the context's latest two-pass Render: out[0] = two-pass Renders so far (0: the rest is meaningless), [1] = splats projected by
 * pass 1, [2] = splats behind the cut that passed the gate (pass 2), [3] / [4] = (splat, bin) pairs binned by pass 1 / 2,
 * [5] = bins pass 1 left unfinished, [6] = bins, [7] = visible splats */
int msplat_get_two_pass_info(msplat_ctx* ctx, uint64_t out[8]);

/* ---- compositor probe (bench statistics): per (bin, quadrant) work item 8 words {shader clocks, records composited, batches
 * staged, inner-loop clocks, pair words fetched, records fetched, bin-list length, 1 + evaluations with w > 0}.  Off by default (a few clock reads per
 * batch; a probed context renders in one pass) ---- */
typedef struct msplat_composite_work {     /* sums over the work items of the latest render */
    uint64_t work_items;          /* 16x16 tiles composited */
    uint64_t list_entries;        /* sum of the bin-list lengths: what it would fetch without early termination */
    uint64_t pair_words_fetched;  /* 4-byte list entries whose loads were issued */
    uint64_t records_fetched;     /* 48-byte projected records whose loads were issued */
    uint64_t records_composited;  /* records that passed the exact footprint test of their 16x16 tile */
    uint64_t pixel_evals;         /* (pixel, splat) evaluations = 256 per composited record */
    uint64_t batches;             /* 64-entry batches staged */
    uint64_t clocks_sum, clocks_max, inner_clocks_sum;   /* shader clocks per work item (probe overhead included) */
    uint64_t useful_evals;        /* r6: evaluations whose weight survived the discard (w > 1/256): the rest of pixel_evals is the price
                                     of evaluating a whole 16x16 tile per record (splat_frag.glsl:37-40 runs per covered fragment) */
} msplat_composite_work;
int msplat_set_tile_probe(msplat_ctx* ctx, int enable);
/* (the record size is in the name: a caller built for the 4-word records of the first release fails to link) */
int msplat_debug_get_tile_probe8(msplat_ctx* ctx, uint32_t* dst8, uint32_t tile_cap);
int msplat_get_composite_work(msplat_ctx* ctx, msplat_composite_work* out);

/* ---- the compositor's schedule: the context's latest compositor launch, as the host chose it (no device work).  out[0] = work items
 * ((bin, quadrant) tiles), [1] = grid: workgroups launched -- grid < items means persistent waves pulling from the work queue, grid ==
 * items every item on its own wave --, [2] = 1 if the bins were walked heaviest-first, [3] = kernel kind: 0 the splat compositor, 1 the
 * draw-order depth / target-rounding compositor, 2 points.  After a two-pass Render the numbers are those of its FIRST pass (the second
 * pass's item count, the unfinished bins, exists on the device only; its grid is chosen the same way) ---- */
int msplat_debug_get_compositor_launch(msplat_ctx* ctx, uint32_t out[4]);

/* ---- the column pass's heavy chunks: what the context's latest binning chain (the second one of a two-pass Render) met and had.
 * out[0] = chunks of 1024 draw-order ranks with MORE than 49152 (splat, bin) pairs, as bin1_upsweep counted them -- every such chunk,
 * with or without a slot --, [1] = the helper slots its bin1_downsweep was launched with (min(128, 2 * an earlier frame's count + 8),
 * 0 after a frame without heavy chunks): min(out[0], out[1]) chunks were split over 8 workgroups, the others ran unsplit.  Reads a
 * host-mapped word and host bookkeeping after the usual synchronise: no device work.  tests/test_gpu_binning_limits.py proves with
 * it which regime its frames ran in ---- */
int msplat_debug_get_heavy_chunks(msplat_ctx* ctx, uint32_t out[2]);

/* ---- the order in which persistent compositor waves walk the bins (grid < items above, unordered): slot s of the table holds a bin,
 * and the slots of one residue class mod 8 -- the bins one XCD composites -- form compact blocks of bins, so that the bins a
 * splat covers share an L2.  msplat_debug_bin_order: the table for a grid of tiles_x x rows bins (1 .. 256 each) as the host computes
 * it with the compiled-in block shape, a permutation of 0 .. tiles_x * rows - 1 (no context, no device).
 * msplat_debug_get_bin_order: the tiles_x * tiles_y words the context's latest compositor launch walked, read back from the device --
 * that table for persistent waves, the heaviest-first order when every item had its own wave, 0, 1, 2, ... (storage order) for the persistent
 * waves of a probed context, whose probe slot i stays storage-order item i.  After a two-pass Render: the first pass's ---- */
int msplat_debug_bin_order(int32_t tiles_x, int32_t rows, uint32_t* out);
int msplat_debug_get_bin_order(msplat_ctx* ctx, uint32_t* out, uint32_t cap);

/* ---- msplat_band_exchange on ONE rank (tests on a one-GPU box): the runs of bin rows that rank `rank` of `world` owns travel
 * from src to dst through ncclSend / ncclRecv to the calling rank itself (`comm` = a 1-rank communicator) ---- */
int msplat_debug_band_exchange_loopback(msplat_ctx* ctx, void* comm, int32_t kind, int32_t block_rows, int32_t world, int32_t rank,
                                        const void* src, void* dst, uint64_t pitch_bytes, int32_t width, int32_t height, int32_t flags);

/* ---- msplat_config.cu_partition: the MSPLAT_CU_* the context's own stream really got (MSPLAT_CU_ALL on a caller's stream or when
 * the runtime refused the mask); mask8 != NULL: the stream's CU mask as hipExtStreamGetCUMask reports it (8 words) ---- */
int msplat_debug_cu_partition(msplat_ctx* ctx, uint32_t* mask8);

/* ---- MSPLAT_STORAGE_SH_Q8 on one record, on the host (no context, no device): the pack / unpack pair every upload route and the
 * download use.  rec_in / rec_out: the reference's 61-float record (rec_out: f_rest = code * step, the rest rec_in's bits);
 * steps_out: the steps of SH bands 1-3; codes_out: the 45 codes in f_rest order (floats 5-7, 9-11, 13-15, 25-60 of the record).
 * Returns the number of non-finite f_rest values (an upload fails when it is not 0), or MSPLAT_ERR_INVALID_ARG for a NULL ---- */
int msplat_debug_sh_q8_round(const float rec_in[61], float rec_out[61], float steps_out[3], int8_t codes_out[45]);

/* ---- the upload kernel alone: milliseconds between two stream events around the context's latest ingest_kernel / repack_kernel /
 * ingest_attributes_kernel launch (msplat_upload_ply_vertices[_device], msplat_upload_cloud_device, msplat_upload_attributes_device)
 * on a context created with enable_timing > 0; *ms = -1 when there is none.  tools/device_upload_timing.py.  After
 * msplat_compact_cloud: its span from the flags kernel to the end of the gather (the readback of K and the new store's allocation
 * included; -1 when nothing was kept).  tools/compact_timing.py.  After msplat_transform_cloud: transform_kernel alone (-1 for an
 * empty cloud).  tools/transform_timing.py.  After msplat_append_cloud: its gathers and append_convert_kernel, without the scan
 * (-1 for an empty result).  tools/append_timing.py.  After msplat_adjust_cloud: adjust_kernel alone (-1 for an empty cloud).
 * tools/adjust_timing.py.  After msplat_measure_cloud: its two kernels (-1 for an empty cloud).  tools/select_timing.py.  After
 * msplat_histogram_values: its two kernels, without the clearing of the counts (-1 for an empty cloud).  tools/values_timing.py ---- */
int msplat_debug_upload_kernel_ms(msplat_ctx* ctx, float* ms);

/* ---- the store's position plane as the kernels read it: N x (x, y, z, footprint bound) in STORAGE order (msplat_get_storage_order
 * maps a slot to its upload index), whatever the mask and the crop hide; cap_floats >= 4 N.  What msplat_mark_volume, msplat_mark_view
 * and msplat_measure_cloud are functions of.  Synchronises ---- */
int msplat_debug_get_positions(msplat_ctx* ctx, float* pos4_out, uint64_t cap_floats);

/* ---- msplat_neighbour_values' hash grid: forces its bucket count for the following calls on the context -- a power of two
 * 1 .. 2^24; 0 hands it back to the call (the smallest power of two >= N).  No result depends on it; tests/test_gpu_neighbours.py
 * makes hash collisions certain with it (1 bucket: every source is a candidate of every query) ---- */
int msplat_debug_set_neighbour_buckets(msplat_ctx* ctx, uint32_t buckets);

#ifdef __cplusplus
}
#endif
#endif /* MSPLAT_DEBUG_H */
