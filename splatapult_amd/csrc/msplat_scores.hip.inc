// msplat_scores.hip.inc -- the score frame: msplat_render_scores (how much of the frame each splat contributes) and
// msplat_mark_scores (such a vector compared with a threshold into a visibility mask); kernels in msplat_scores.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_ids.hip.inc, whose chain and window it shares)
//
// A score frame is the id frame's chain -- a plain one-pass frame's projection and binning, without z_w -- with
// composite_scores_kernel in place of the compositor, over the 16x16 tiles that intersect the caller's window.  Device memory only:
// the arrays are accumulated into with atomics, so there is no staging and no host-output retry.  Like the id frame it is never a
// two-pass frame and does not count as a Render.

struct ScoresTarget {            // what one score frame reads and adds to; device memory
    const uint8_t* region;       // NULL: every pixel of the window
    size_t region_pitch;
    uint64_t* score;
    uint32_t* pixels;            // NULL: none
};

static int launch_scores(msplat_ctx* ctx, const FrameParams& fp, const int32_t window[4], const ScoresTarget& t)
{
    WalkChain wc;
    int arc = issue_walk_chain(ctx, fp, window, false, true, wc);
    if (arc) return arc;
    if (fp.tiles_x * fp.tiles_y > 0) {
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(wc.grid), dim3(kCompThreads), 0, ctx->stream, (const uint32_t*)ctx->tile_start.p,
                               (const uint32_t*)ctx->pairsB.p, (const float4*)ctx->rec2d.p, (const uint32_t*)ctx->valA.p, wc.order, wc.p,
                               (uint32_t)ctx->pair_cap, (uint32_t*)ctx->queue.p, wc.items, t.region, t.region_pitch,
                               (unsigned long long*)t.score, t.pixels);
        };
        if (t.pixels) launch(composite_scores_kernel<true>);
        else launch(composite_scores_kernel<false>);
    }
    if (hipGetLastError() != hipSuccess) {
        ctx->tables_dirty = true;
        return fail(ctx, MSPLAT_ERR_HIP, "msplat_render_scores: a kernel launch failed");
    }
    return MSPLAT_OK;
}

static int scores_impl(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2],
                       IdsWindow win, const uint8_t* d_region, uint64_t region_pitch_bytes, uint64_t* d_score, uint32_t* d_pixels, uint64_t n)
{
    static const char* who = "msplat_render_scores";
    FrameParams fp;
    int rc = begin_frame(ctx, who, true, d_score ? nullptr : "d_score is NULL", cameraMat, projMat, viewport, nearFar, fp);
    if (rc) return rc;
    if ((rc = walk_frame_window(ctx, who, "score", fp, win))) return rc;
    const int32_t* w = win.v;
    if (n != ctx->N)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %llu scores for a cloud of %llu splats", who, (unsigned long long)n,
                    (unsigned long long)ctx->N);
    if ((rc = region_pitch(ctx, who, d_region, region_pitch_bytes, w[2]))) return rc;
    // (both alignments before any pointer query, and before an empty cloud succeeds: not check_device_array's order)
    if ((rc = check_aligned(ctx, who, "d_score", d_score, 8)) || (rc = check_aligned(ctx, who, "d_pixels", d_pixels, 4))) return rc;
    if (n == 0) return MSPLAT_OK;
    if ((rc = check_region(ctx, who, d_region, region_pitch_bytes, w[2], w[3]))) return rc;
    if ((rc = check_device_source(ctx, who, "d_score", d_score, 8 * n))) return rc;
    if (d_pixels && (rc = check_device_source(ctx, who, "d_pixels", d_pixels, 4 * n))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->tables_dirty && (rc = clear_frame_tables(ctx))) return rc;
    if (ctx->store && ctx->store->reordered && (rc = ensure_order_dev(ctx))) return rc;
    const ScoresTarget t{d_region, (size_t)region_pitch_bytes, d_score, d_pixels};
    return with_pending_overflow(ctx, [&] { return launch_scores(ctx, fp, w, t); });      // an EARLIER frame's; this one is still run
}

int msplat_render_scores(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2],
                         const int32_t window[4], const uint8_t* d_region, uint64_t region_pitch_bytes, uint64_t* d_score,
                         uint32_t* d_pixels, uint64_t n)
{
    IdsWindow win{window != nullptr, {0, 0, 0, 0}};
    if (window) std::memcpy(win.v, window, sizeof(win.v));      // copied: a queued call outlives the caller's array
    return submit_frame<false>(ctx, d_score != nullptr, cameraMat, projMat, cameraMat, projMat, viewport, nearFar,
                        [=](const float* cam, const float* proj, const float*, const float*, const float* vp, const float* nf) {
                            return scores_impl(ctx, cam, proj, vp, nf, win, d_region, region_pitch_bytes, d_score, d_pixels, n);
                        });
}

int msplat_mark_scores(msplat_ctx* ctx, const uint64_t* d_score, uint64_t n, int32_t op, uint64_t threshold, uint8_t* d_mask, uint8_t value)
{
    static const char* who = "msplat_mark_scores";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    int rc;
    if ((rc = check_splat_count(ctx, who, "visibility is for splat clouds", n))) return rc;
    if (op != MSPLAT_SCORE_BELOW && op != MSPLAT_SCORE_AT_LEAST)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: op %d is neither MSPLAT_SCORE_BELOW nor MSPLAT_SCORE_AT_LEAST", who, op);
    if (n == 0) return MSPLAT_OK;
    if (!d_score || !d_mask) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s is NULL", who, d_score ? "d_mask" : "d_score");
    if ((rc = check_device_array(ctx, who, "d_score", d_score, 8, n))) return rc;
    if ((rc = check_device_source(ctx, who, "d_mask", d_mask, n))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_per_item(ctx, who, n, mark_scores_kernel, (const unsigned long long*)d_score, (uint32_t)n, op == MSPLAT_SCORE_AT_LEAST,
                           (unsigned long long)threshold, d_mask, value);
}
