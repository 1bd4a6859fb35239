// msplat_ids.hip.inc -- the id frame: msplat_render_ids (which splat each pixel shows) and msplat_mark_ids (a region of that plane
// scattered into a visibility mask); kernels in msplat_ids.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after the render entry points)
//
// An id frame is the chain of a plain one-pass frame -- issue_projection(PROJ_PLAIN), issue_binning -- with composite_ids_kernel in
// place of the compositor, over the 16x16 tiles that intersect the caller's window.  It has no colour target, is never a two-pass
// frame and does not count as a Render: the two-pass controller, its statistics and the timing sets stay as the latest Render left
// them (the pair counters are the id frame's afterwards: the same projection and binning as a Render with its matrices).

struct IdsTarget {               // the planes of one id frame, both in one memory space; rows of the WINDOW
    uint32_t* ids;
    size_t ids_pitch;
    float* depth;                // NULL: none
    size_t depth_pitch;
};

// What the id frame and the score frame launch before their own kernel, and what that kernel walks
struct WalkChain {
    IdsParams p;
    uint32_t items;              // the 16x16 tiles the window touches
    uint32_t grid;               // waves: one per item, or the context's pool of persistent waves
    const uint32_t* order;       // storage slot -> upload index; NULL for a cloud stored in upload order
};

// a plain one-pass frame's projection and binning (want_zw: plus z_w per rank); window: x0, y0, w, h in viewport pixels (checked)
static int issue_walk_chain(msplat_ctx* ctx, const FrameParams& fp, const int32_t window[4], bool want_zw, bool async_overflow_flag,
                            WalkChain& wc)
{
    uint32_t* counters = (uint32_t*)ctx->counters.p;
    const uint32_t N = (uint32_t)ctx->N;
    RenderChain rc{ctx, fp, ctx->stream, false, N, counters + kCntV, counters + kCntD, counters + kCntOverflow, (uint32_t*)ctx->queue.p,
                   counters + kCntV, (uint32_t*)ctx->occ.p, fp.tiles_x * fp.tiles_y, (uint32_t)ctx->pair_cap,
                   false, 0, (int)std::max(1u, div_up(N, kProjThreads)), nullptr, nullptr, 0, async_overflow_flag, FramePlanes{}};
    rc.want_zw = want_zw;        // z_w per rank, as for a frame with planes
    if (want_zw) {
        int arc = buf_alloc(ctx, ctx->zq, std::max<uint64_t>(std::max(ctx->rank_cap, ctx->N), 1) * 4);
        if (arc) return arc;
    }
    issue_projection(rc, PROJ_PLAIN, 0.0f);
    issue_binning(rc, 0, 0);
    IdsParams& p = wc.p;
    p.tiles_x = fp.tiles_x;
    p.x0 = window[0]; p.y0 = window[1]; p.x1 = window[0] + window[2]; p.y1 = window[1] + window[3];
    p.tile_x0 = p.x0 / kTile; p.tile_y0 = p.y0 / kTile;
    p.tiles_w = (p.x1 - 1) / kTile - p.tile_x0 + 1;
    wc.items = (uint32_t)p.tiles_w * (uint32_t)((p.y1 - 1) / kTile - p.tile_y0 + 1);
    // every item on its own wave where the compositor would do the same, else the context's pool of persistent waves and the queue
    const uint32_t pool = (ctx->comp_waves_auto && wc.items <= 20480u) ? wc.items : (uint32_t)ctx->comp_waves;
    wc.grid = std::min(wc.items, pool);
    wc.order = (ctx->store && ctx->store->reordered) ? (const uint32_t*)ctx->store->order_dev.p : nullptr;
    return MSPLAT_OK;
}

static int launch_ids(msplat_ctx* ctx, const FrameParams& fp, const int32_t window[4], const IdsTarget& out, bool async_overflow_flag)
{
    WalkChain wc;
    int arc = issue_walk_chain(ctx, fp, window, true, async_overflow_flag, wc);
    if (arc) return arc;
    if (fp.tiles_x * fp.tiles_y > 0)
        hipLaunchKernelGGL(composite_ids_kernel, dim3(wc.grid), dim3(kCompThreads), 0, ctx->stream, (const uint32_t*)ctx->tile_start.p,
                           (const uint32_t*)ctx->pairsB.p, (const float4*)ctx->rec2d.p, (const float*)ctx->zq.p, (const uint32_t*)ctx->valA.p,
                           wc.order, wc.p, (uint32_t)ctx->pair_cap, (uint32_t*)ctx->queue.p, wc.items, out.ids, out.ids_pitch, out.depth,
                           out.depth_pitch);
    if (hipGetLastError() != hipSuccess) {
        ctx->tables_dirty = true;
        return fail(ctx, MSPLAT_ERR_HIP, "msplat_render_ids: a kernel launch failed");
    }
    return MSPLAT_OK;
}

// host output: the frame into staging planes of the context's, copied back; the pair buffer grows on overflow (render_to_host)
static int ids_to_host(msplat_ctx* ctx, const FrameParams& fp, const int32_t window[4], const IdsTarget& out)
{
    int rc;
    const size_t tight = (size_t)window[2] * 4, rows = (size_t)window[3];
    if ((rc = buf_alloc(ctx, ctx->fb_ids, tight * rows))) return rc;
    if (out.depth && (rc = buf_alloc(ctx, ctx->fb_idz, tight * rows))) return rc;
    const IdsTarget staged{(uint32_t*)ctx->fb_ids.p, tight, out.depth ? (float*)ctx->fb_idz.p : nullptr, tight};
    for (int attempt = 0; attempt < 6; ++attempt) {
        if ((rc = launch_ids(ctx, fp, window, staged, false))) return rc;
        uint32_t cnt[4];
        HIP_TRY(ctx, hipMemcpyAsync(cnt, ctx->counters.p, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (cnt[kCntOverflow] == 0) {
            HIP_TRY(ctx, hipMemcpy2D(out.ids, out.ids_pitch, staged.ids, tight, tight, rows, hipMemcpyDeviceToHost));
            if (out.depth) HIP_TRY(ctx, hipMemcpy2D(out.depth, out.depth_pitch, staged.depth, tight, tight, rows, hipMemcpyDeviceToHost));
            return MSPLAT_OK;
        }
        const uint64_t need = (uint64_t)cnt[kCntOverflow] + (cnt[kCntOverflow] >> 2) + 1024;
        if (ctx->cfg.pair_capacity != 0 || need > 0x7FFFFFFFull)
            return fail(ctx, MSPLAT_ERR_PAIR_OVERFLOW, "pair buffer too small: need %u, capacity %llu", cnt[kCntOverflow],
                        (unsigned long long)ctx->pair_cap);
        if ((rc = ensure_pair_capacity(ctx, need))) return rc;
    }
    return fail(ctx, MSPLAT_ERR_PAIR_OVERFLOW, "pair buffer could not be grown");
}

// a plane's pitch: 0 = tight rows of the window
static int ids_pitch(msplat_ctx* ctx, const char* who, const char* what, uint64_t& pitch_bytes, uint64_t w)
{
    if (pitch_bytes == 0) pitch_bytes = 4 * w;
    if (pitch_bytes < 4 * w || pitch_bytes % 4 != 0)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s pitch %llu too small / misaligned for %llu pixels of 4 bytes", who, what,
                    (unsigned long long)pitch_bytes, (unsigned long long)w);
    return MSPLAT_OK;
}

// an optional region plane, one byte per pixel of a w x h window: its pitch (0 = tight rows; read only with a region) ...
static int region_pitch(msplat_ctx* ctx, const char* who, const uint8_t* d_region, uint64_t& pitch_bytes, uint64_t w)
{
    if (pitch_bytes == 0) pitch_bytes = w;
    if (!d_region || pitch_bytes >= w) return MSPLAT_OK;
    return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: region pitch %llu too small for %llu pixels of 1 byte", who, (unsigned long long)pitch_bytes,
                (unsigned long long)w);
}

// ... and its rows: device memory of the context's device.  (Two functions: every caller has checks of its own between them)
static int check_region(msplat_ctx* ctx, const char* who, const uint8_t* d_region, uint64_t pitch_bytes, uint64_t w, uint64_t h)
{
    return d_region ? check_device_source(ctx, who, "d_region", d_region, (h - 1) * pitch_bytes + w) : MSPLAT_OK;
}

struct IdsWindow { bool given; int32_t v[4]; };

// a caller's window of a width x height viewport: not given = the whole viewport; else x0, y0, w, h, not empty and inside it
static int frame_window(msplat_ctx* ctx, const char* who, int width, int height, IdsWindow& win)
{
    if (!win.given) { win.v[0] = 0; win.v[1] = 0; win.v[2] = width; win.v[3] = height; }
    const int32_t* w = win.v;
    if (w[2] <= 0 || w[3] <= 0 || w[0] < 0 || w[1] < 0 || (int64_t)w[0] + w[2] > width || (int64_t)w[1] + w[3] > height)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: window (%d, %d, %d, %d) is empty or not inside the %d x %d viewport", who, w[0], w[1],
                    w[2], w[3], width, height);
    return MSPLAT_OK;
}

// What the frames that walk the lists themselves (the id frame, the score frame: `walk` names it) refuse after begin_frame, and
// their window (frame_window)
static int walk_frame_window(msplat_ctx* ctx, const char* who, const char* walk, const FrameParams& fp, IdsWindow& win)
{
    char why[160] = "";
    if (ctx->point_mode) std::snprintf(why, sizeof(why), "the context holds a point cloud (the sprite pipeline has no %s walk)", walk);
    else if (ctx->depth_bits != 0) std::snprintf(why, sizeof(why), "msplat_set_depth_test is on (the %s walk is front to back, without a depth buffer)", walk);
    else if (ctx->rop != MSPLAT_ROP_NONE) std::snprintf(why, sizeof(why), "msplat_set_target_emulation is not MSPLAT_ROP_NONE (the %s walk blends in fp32)", walk);
    else if (ctx->probe_on) std::snprintf(why, sizeof(why), "the tile probe (msplat_set_tile_probe) has no %s walk", walk);
    else if (ctx->banded) std::snprintf(why, sizeof(why), "the context is banded (msplat_set_band / msplat_set_band_layout): the %s frame covers whole windows", walk);
    if (why[0]) return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %s", who, why);
    return frame_window(ctx, who, fp.width, fp.height, win);
}

static int ids_impl(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2],
                    IdsWindow win, uint32_t* ids, uint64_t ids_pitch_bytes, float* id_depth, uint64_t depth_pitch_bytes, int out_is_device)
{
    static const char* who = "msplat_render_ids";
    FrameParams fp;
    int rc = begin_frame(ctx, who, true, ids ? nullptr : "ids is NULL", cameraMat, projMat, viewport, nearFar, fp);
    if (rc) return rc;
    if ((rc = walk_frame_window(ctx, who, "id", fp, win))) return rc;
    const int32_t* w = win.v;
    if ((rc = ids_pitch(ctx, who, "ids", ids_pitch_bytes, (uint64_t)w[2]))) return rc;
    if (id_depth && (rc = ids_pitch(ctx, who, "id_depth", depth_pitch_bytes, (uint64_t)w[2]))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->tables_dirty && (rc = clear_frame_tables(ctx))) return rc;
    if (ctx->store && ctx->store->reordered && (rc = ensure_order_dev(ctx))) return rc;
    const IdsTarget out{ids, (size_t)ids_pitch_bytes, id_depth, (size_t)depth_pitch_bytes};
    return with_pending_overflow(ctx, [&] {      // an EARLIER frame's; this one is still run
        return out_is_device ? launch_ids(ctx, fp, w, out, true) : ids_to_host(ctx, fp, w, out);
    });
}

int msplat_render_ids(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2],
                      const int32_t window[4], uint32_t* ids, uint64_t ids_pitch_bytes, float* id_depth, uint64_t id_depth_pitch_bytes,
                      int out_is_device)
{
    IdsWindow win{window != nullptr, {0, 0, 0, 0}};
    if (window) std::memcpy(win.v, window, sizeof(win.v));      // copied: a queued call outlives the caller's array
    return submit_frame<false>(ctx, out_is_device && ids, cameraMat, projMat, cameraMat, projMat, viewport, nearFar,
                        [=](const float* cam, const float* proj, const float*, const float*, const float* vp, const float* nf) {
                            return ids_impl(ctx, cam, proj, vp, nf, win, ids, ids_pitch_bytes, id_depth, id_depth_pitch_bytes, out_is_device);
                        });
}

int msplat_mark_ids(msplat_ctx* ctx, const uint32_t* d_ids, uint64_t ids_pitch_bytes, uint32_t w, uint32_t h, const uint8_t* d_region,
                    uint64_t region_pitch_bytes, uint8_t* d_mask, uint64_t n, uint8_t value)
{
    static const char* who = "msplat_mark_ids";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    int rc;
    if ((rc = check_splat_count(ctx, who, "visibility is for splat clouds", n))) return rc;
    if (w == 0 || h == 0 || n == 0) return MSPLAT_OK;
    if (!d_ids || !d_mask) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s is NULL", who, d_ids ? "d_mask" : "d_ids");
    if ((rc = ids_pitch(ctx, who, "ids", ids_pitch_bytes, w)) || (rc = region_pitch(ctx, who, d_region, region_pitch_bytes, w))) return rc;
    if ((rc = check_aligned(ctx, who, "d_ids", d_ids, 4))) return rc;      // (a pitched extent: not check_device_array's)
    if ((rc = check_device_source(ctx, who, "d_ids", d_ids, (uint64_t)(h - 1) * ids_pitch_bytes + 4ull * w))) return rc;
    if ((rc = check_region(ctx, who, d_region, region_pitch_bytes, w, h))) return rc;
    if ((rc = check_device_source(ctx, who, "d_mask", d_mask, n))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_per_item(ctx, who, (uint64_t)w * h, mark_ids_kernel, d_ids, (size_t)ids_pitch_bytes, w, h, d_region, (size_t)region_pitch_bytes,
                           d_mask, (uint32_t)n, value);
}
