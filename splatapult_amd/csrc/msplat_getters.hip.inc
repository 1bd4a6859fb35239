// msplat_getters.hip.inc -- what a context reports: sorted lists, statistics, timings, the parity-test taps and probes of msplat_debug.h, the diagnostic stamps
// (textually part of msplat_device.hip: included inside its extern "C" block, after struct msplat_ctx and the helpers; r6 split, VERDICT r5 item 7)

#ifdef MSPLAT_STAMPS
// diagnostic build only (msplat_common.hip.h, MSPLAT_STAMP): switch the workgroup stamps of the current device on / off, read the
// table (and clear it).  enable != 0 allocates 2^log2_slots records of 32 bytes at the first call.
static msplat::StampRec* g_stamps_dev = nullptr;
static uint32_t g_stamps_slots = 0;
int msplat_debug_stamps(int enable, uint32_t log2_slots)
{
    if (enable && !g_stamps_dev) {
        g_stamps_slots = 1u << std::min(26u, std::max(10u, log2_slots));
        if (hipMalloc((void**)&g_stamps_dev, (size_t)g_stamps_slots * sizeof(msplat::StampRec)) != hipSuccess) return MSPLAT_ERR_HIP;
        if (hipMemset(g_stamps_dev, 0, (size_t)g_stamps_slots * sizeof(msplat::StampRec)) != hipSuccess) return MSPLAT_ERR_HIP;
        if (hipMemcpyToSymbol(HIP_SYMBOL(msplat::g_stamp_buf), &g_stamps_dev, sizeof(g_stamps_dev)) != hipSuccess) return MSPLAT_ERR_HIP;
    }
    if (hipDeviceSynchronize() != hipSuccess) return MSPLAT_ERR_HIP;
    const uint32_t mask = (enable && g_stamps_dev) ? g_stamps_slots - 1u : 0u;
    if (hipMemcpyToSymbol(HIP_SYMBOL(msplat::g_stamp_mask), &mask, sizeof(mask)) != hipSuccess) return MSPLAT_ERR_HIP;
    return hipDeviceSynchronize() == hipSuccess ? (int)g_stamps_slots : MSPLAT_ERR_HIP;
}
int msplat_debug_stamps_read(void* dst, uint64_t bytes)
{
    if (!g_stamps_dev || !dst) return MSPLAT_ERR_INVALID_ARG;
    const size_t n = std::min<size_t>(bytes, (size_t)g_stamps_slots * sizeof(msplat::StampRec));
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dst, g_stamps_dev, n, hipMemcpyDeviceToHost) != hipSuccess) return MSPLAT_ERR_HIP;
    if (hipMemset(g_stamps_dev, 0, (size_t)g_stamps_slots * sizeof(msplat::StampRec)) != hipSuccess) return MSPLAT_ERR_HIP;
    return MSPLAT_OK;
}
#endif

int msplat_sort_count(msplat_ctx* ctx, uint32_t* v)
{
    drain_async(ctx);
    if (!ctx || !v) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->has_sort) return fail(ctx, MSPLAT_ERR_NO_SORT, "no sort yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(v, (const uint32_t*)ctx->counters.p + kCntV, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MSPLAT_OK;
}

static int copy_sorted(msplat_ctx* ctx, const Buf& src, uint32_t* dst, uint32_t cap)
{
    uint32_t v = 0;
    int rc = msplat_sort_count(ctx, &v);
    if (rc) return rc;
    if (!dst && v) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "dst is NULL");
    if (cap < v) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "capacity %u < sort count %u", cap, v);
    if (v) HIP_TRY(ctx, hipMemcpy(dst, src.p, (size_t)v * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MSPLAT_OK;
}

int msplat_get_sorted_indices(msplat_ctx* ctx, uint32_t* dst, uint32_t cap)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    int rc = copy_sorted(ctx, ctx->valA, dst, cap);
    if (rc == MSPLAT_OK && ctx->store && ctx->store->reordered) {      // storage slots -> upload indices
        uint32_t v = 0;
        if ((rc = msplat_sort_count(ctx, &v))) return rc;
        const std::vector<uint32_t>& ord = ctx->store->order_host;
        for (uint32_t i = 0; i < v; ++i) dst[i] = ord[dst[i]];
    }
    return rc;
}

// The storage order of the uploaded cloud: dst[j] = upload index of the splat in storage slot j (identity when the cloud
// was not reordered; *reordered says which).  Equal depth keys are drawn in ascending storage slot.
int msplat_get_storage_order(msplat_ctx* ctx, uint32_t* dst, uint64_t cap, int* reordered)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!ctx->has_cloud) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "no cloud uploaded");
    const bool ro = ctx->store && ctx->store->reordered;
    if (reordered) *reordered = ro ? 1 : 0;
    if (dst) {
        if (cap < ctx->N) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "capacity %llu < %llu splats", (unsigned long long)cap, (unsigned long long)ctx->N);
        for (uint64_t j = 0; j < ctx->N; ++j) dst[j] = ro ? ctx->store->order_host[j] : (uint32_t)j;
    }
    return MSPLAT_OK;
}

// chunk-level cull, for the latest Sort's camera: bounding boxes box_live keeps / boxes in the cloud (0 / 0 for a cloud in upload
// order); *listed = 1 when that Sort's pass 0 walked the listed boxes only.  Runs box_cull_kernel on demand, over the boxes that Sort
// used: the context's own under a mask or a crop (msplat_set_visibility), else the store's; synchronises.
int msplat_debug_get_cull_boxes(msplat_ctx* ctx, uint32_t* live, uint32_t* total, int* listed)
{
    drain_async(ctx);
    if (!ctx || !live || !total) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->has_sort) return fail(ctx, MSPLAT_ERR_NO_SORT, "no sort yet");
    *live = *total = 0;
    if (listed) *listed = ctx->last_sort_listed ? 1 : 0;
    const CloudStore* st = ctx->store.get();
    if (!(st && st->reordered && st->boxes.p)) return MSPLAT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t wgs = div_up(st->nboxes, kBoxGroup);
    Buf list, cnt;
    int rc = buf_alloc(ctx, list, (size_t)wgs * kBoxGroup * 4);
    if (!rc) rc = buf_alloc(ctx, cnt, 256 * 4);
    if (!rc) {
        launch_box_cull(ctx, st, ctx->vis_sorted, ctx->last_sort_fp, (uint32_t*)list.p, (uint32_t*)cnt.p);
        uint32_t h[256];
        hipError_t e = hipMemcpyAsync(h, cnt.p, (size_t)wgs * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = fail(ctx, MSPLAT_ERR_HIP, "msplat_debug_get_cull_boxes: %s", hipGetErrorString(e));
        else for (uint32_t g = 0; g < wgs; ++g) *live += h[g];
    }
    buf_free(ctx, list);
    buf_free(ctx, cnt);
    *total = st->nboxes;
    return rc;
}

int msplat_get_sorted_keys(msplat_ctx* ctx, uint32_t* dst, uint32_t cap)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    return copy_sorted(ctx, ctx->keyA, dst, cap);
}

int msplat_get_stats(msplat_ctx* ctx, msplat_stats* out)
{
    drain_async(ctx);
    if (!ctx || !out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ctx->has_render) {   // "drawn" is a statistic only: counted on demand, not in the frame
        uint32_t* counters = (uint32_t*)ctx->counters.p;
        HIP_TRY(ctx, hipMemsetAsync(counters + kCntDrawn, 0, (kCntLdsProbe - kCntDrawn) * sizeof(uint32_t), ctx->stream));     // drawn .. pairs16
        hipLaunchKernelGGL(count_drawn_kernel, dim3(256), dim3(kThreads), 0, ctx->stream, (const uint32_t*)ctx->rect.p,
                           (const float4*)ctx->rec2d.p, counters + kCntV, ctx->last_fp, counters + kCntDrawn,
                           (unsigned long long*)(counters + kCntPairs16));
    }
    HIP_TRY(ctx, hipMemcpyAsync(cnt, ctx->counters.p, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memset(out, 0, sizeof(*out));
    out->num_splats = ctx->N;
    out->sort_count = ctx->has_sort ? cnt[kCntV] : 0;
    out->pairs = ctx->has_render ? cnt[kCntD] : 0;
    out->drawn = ctx->has_render ? cnt[kCntDrawn] : 0;
    out->pairs_tile16 = ctx->has_render ? ((uint64_t)cnt[kCntPairs16 + 1] << 32 | cnt[kCntPairs16]) : 0;
    out->tiles_x = ctx->last_fp.tiles_x;
    out->tiles_y = ctx->last_fp.tiles_y;
    out->width = ctx->last_fp.width;
    out->height = ctx->last_fp.height;
    out->pair_capacity = ctx->pair_cap;
    out->device_bytes = ctx->device_bytes;
    if (ctx->has_render && cnt[kCntOverflow] != 0)
        return fail(ctx, MSPLAT_ERR_PAIR_OVERFLOW, "last render overflowed the pair buffer: need %u, capacity %llu",
                    cnt[kCntOverflow], (unsigned long long)ctx->pair_cap);
    return MSPLAT_OK;
}

int msplat_get_timings(msplat_ctx* ctx, msplat_timings* out)
{
    drain_async(ctx);
    if (!ctx || !out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    std::memset(out, 0, sizeof(*out));
    if (!ctx->ev_ok) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "context created without enable_timing");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // average over the sets recorded since the previous call (at most the kEvSets most recent)
    const uint32_t ns = std::min<uint32_t>(ctx->sort_sets, msplat_ctx::kEvSets);
    for (uint32_t k = 0; k < ns; ++k) {
        float t = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->ev[k][kEvSortBegin], ctx->ev[k][kEvSortEnd]));
        out->sort_total += t / ns;
    }
    const uint32_t nr = std::min<uint32_t>(ctx->render_sets, msplat_ctx::kEvSets);
    for (uint32_t k = 0; k < nr; ++k) {
        float a = 0, b = 0, c = 0, d = 0;
        const bool two = (ctx->two_pass_sets_mask & (1u << k)) != 0u;     // a two-pass frame: every stage ran twice
        HIP_TRY(ctx, hipEventElapsedTime(&a, ctx->ev[k][kEvRenderBegin], ctx->ev[k][kEvRenderEnd]));
        HIP_TRY(ctx, hipEventElapsedTime(&b, ctx->ev[k][kEvRenderBegin], ctx->ev[k][kEvProjected]));
        HIP_TRY(ctx, hipEventElapsedTime(&c, ctx->ev[k][kEvProjected], ctx->ev[k][kEvBinned]));
        HIP_TRY(ctx, hipEventElapsedTime(&d, ctx->ev[k][kEvBinned], ctx->ev[k][two ? kEvPass2Begin : kEvRenderEnd]));
        if (two) {
            float b2 = 0, c2 = 0, d2 = 0;
            HIP_TRY(ctx, hipEventElapsedTime(&b2, ctx->ev[k][kEvPass2Begin], ctx->ev[k][kEvPass2Projected]));      // mask + gate + second projection
            HIP_TRY(ctx, hipEventElapsedTime(&c2, ctx->ev[k][kEvPass2Projected], ctx->ev[k][kEvPass2Binned]));
            HIP_TRY(ctx, hipEventElapsedTime(&d2, ctx->ev[k][kEvPass2Binned], ctx->ev[k][kEvRenderEnd]));
            b += b2; c += c2; d += d2;
        }
        out->render_total += a / nr; out->project += b / nr; out->binning += c / nr; out->composite += d / nr;
        if (ctx->comp_kernel_sets_mask & (1u << k)) {
            float e = 0, e2 = 0;
            HIP_TRY(ctx, hipEventElapsedTime(&e, ctx->ev[k][kEvCompBegin], ctx->ev[k][kEvCompEnd]));
            if (two) HIP_TRY(ctx, hipEventElapsedTime(&e2, ctx->ev[k][kEvComp2Begin], ctx->ev[k][kEvComp2End]));
            out->reserved[1] += e + e2;  // summed here, averaged below
            out->reserved[2] += 1.0f;
        }
    }
    if (out->reserved[2] > 0.0f) out->reserved[1] /= out->reserved[2];
    out->reserved[0] = (float)nr;       // number of frames averaged
    ctx->sort_sets = 0;
    ctx->render_sets = 0;
    return MSPLAT_OK;
}

int msplat_debug_get_projected(msplat_ctx* ctx, float* rec12, uint32_t* rect, uint32_t cap)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!ctx->has_render) return fail(ctx, MSPLAT_ERR_NO_SORT, "no render yet");
    uint32_t v = 0;
    int rc = msplat_sort_count(ctx, &v);
    if (rc) return rc;
    if (cap < v) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "capacity %u < sort count %u", cap, v);
    if (v && rec12) HIP_TRY(ctx, hipMemcpy(rec12, ctx->rec2d.p, (size_t)v * 48, hipMemcpyDeviceToHost));
    if (v && rect) HIP_TRY(ctx, hipMemcpy(rect, ctx->rect.p, (size_t)v * 4, hipMemcpyDeviceToHost));
    return MSPLAT_OK;
}

int msplat_debug_get_projected_view(msplat_ctx* ctx, int32_t view, float* rec12, uint32_t* rect, uint32_t count)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!ctx->has_render) return fail(ctx, MSPLAT_ERR_NO_SORT, "no render yet");
    if (view < 0 || view >= std::max(ctx->last_fp.views, 1))
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "view %d: the latest Render had %d view(s)", view, std::max(ctx->last_fp.views, 1));
    uint32_t v = 0;
    int rc = msplat_sort_count(ctx, &v);
    if (rc) return rc;
    const uint64_t first = view ? ((uint64_t)v + 63u) & ~(uint64_t)63u : 0u;      // project_kernel<PROJ_TWO_VIEWS>: V1
    const uint64_t have = std::min<uint64_t>(ctx->rec2d.bytes / 48, ctx->rect.bytes / 4);
    if (first + count > have)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "ranks %llu .. %llu: the buffers hold %llu", (unsigned long long)first,
                    (unsigned long long)(first + count), (unsigned long long)have);
    if (count && rec12) HIP_TRY(ctx, hipMemcpy(rec12, (const char*)ctx->rec2d.p + first * 48, (size_t)count * 48, hipMemcpyDeviceToHost));
    if (count && rect) HIP_TRY(ctx, hipMemcpy(rect, (const char*)ctx->rect.p + first * 4, (size_t)count * 4, hipMemcpyDeviceToHost));
    return MSPLAT_OK;
}

int msplat_debug_fill_projected(msplat_ctx* ctx, int32_t byte)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!ctx->rec2d.p || !ctx->rect.p) return fail(ctx, MSPLAT_ERR_NO_SORT, "no cloud yet");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemset(ctx->rec2d.p, byte & 255, ctx->rec2d.bytes));
    // (an EMPTY rectangle that is not kRectEmpty: tx0 = 255 > tx1 = 0, ty0 = the byte -- whoever read it would bin nothing)
    HIP_TRY(ctx, hipMemsetD32((hipDeviceptr_t)ctx->rect.p, (int)(kRectEmpty | (uint32_t)(byte & 255) << 8), ctx->rect.bytes / 4));
    HIP_TRY(ctx, hipDeviceSynchronize());
    return MSPLAT_OK;
}

// On-device check of the ordering contracts of the last Sort (+ the last Render's bin lists, if there was one):
// sorted keys ascend with ties in ascending splat index, every bin list ascends in draw-order rank.  A cheap guard
// for the lane-ordered LDS-atomic ranking (probed at msplat_create, not documented hardware behaviour): call it in
// debug builds or every few hundred frames; non-zero counts mean the context should be re-created with
// msplat_config.rank_mode = MSPLAT_RANK_BALLOT.
int msplat_debug_two_pass(msplat_ctx* ctx, float share, uint64_t* two_pass_frames, float* share_now)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!(share >= 0.0f && share <= 1.0f)) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_debug_two_pass: share %g not in [0, 1]", (double)share);
    ctx->two_pass.pin(share);
    if (two_pass_frames) *two_pass_frames = ctx->frames_two_pass;
    if (share_now) *share_now = ctx->two_pass.share;
    return MSPLAT_OK;
}

int msplat_get_two_pass_info(msplat_ctx* ctx, uint64_t out[8])
{
    drain_async(ctx);
    if (!ctx || !out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    for (int k = 0; k < 8; ++k) out[k] = 0;
    out[0] = ctx->frames_two_pass;
    if (!ctx->last_render_two_pass) { out[0] = 0; return MSPLAT_OK; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    out[1] = host_word(ctx, kHostPass1Splats);
    out[2] = host_word(ctx, kHostListedRanks);
    out[3] = host_word(ctx, kHostPass1Pairs);
    out[4] = host_word(ctx, kHostPass2Pairs);
    out[5] = host_word(ctx, kHostUnfinishedBins);
    out[6] = (uint64_t)ctx->last_fp.tiles_x * (uint64_t)ctx->last_fp.tiles_y;
    out[7] = host_word(ctx, kHostV);
    return MSPLAT_OK;
}

int msplat_debug_verify_order(msplat_ctx* ctx, uint32_t* key_violations, uint32_t* list_violations)
{
    drain_async(ctx);
    if (!ctx || !key_violations || !list_violations) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->has_sort) return fail(ctx, MSPLAT_ERR_NO_SORT, "no sort yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t* counters = (uint32_t*)ctx->counters.p;
    uint32_t* bad = counters + kCntOrderBad;
    HIP_TRY(ctx, hipMemsetAsync(bad, 0, 2 * sizeof(uint32_t), ctx->stream));
    const int nbins = ctx->has_render ? ctx->last_fp.tiles_x * ctx->last_fp.tiles_y : 0;
    hipLaunchKernelGGL(verify_order_kernel, dim3(1024), dim3(kThreads), 0, ctx->stream, (const uint32_t*)ctx->keyA.p,
                       (const uint32_t*)ctx->valA.p, (const uint32_t*)(counters + kCntV), nbins ? (const uint32_t*)ctx->tile_start.p : nullptr,
                       (const uint32_t*)ctx->pairsB.p, (uint32_t)ctx->pair_cap, nbins, bad);
    uint32_t h[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(h, bad, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *key_violations = h[0];
    *list_violations = h[1];
    return MSPLAT_OK;
}

int msplat_debug_get_tile_probe8(msplat_ctx* ctx, uint32_t* dst, uint32_t tile_cap)
{
    drain_async(ctx);
    if (!ctx || !dst) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->probe.p || !ctx->probe_on)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "tile probe not enabled (msplat_set_tile_probe)");
    if (!ctx->has_render) return fail(ctx, MSPLAT_ERR_NO_SORT, "no render yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t ntiles = (uint32_t)(ctx->last_fp.tiles_x * ctx->last_fp.tiles_y) * 4u;   // work items = (bin, quadrant)
    if (tile_cap < ntiles) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "tile capacity too small (work items = bins x 4)");
    HIP_TRY(ctx, hipMemcpy(dst, ctx->probe.p, (size_t)ntiles * kProbeWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MSPLAT_OK;
}

// sums the compositor probe of the last render (msplat_set_tile_probe): what the dominant kernel really fetched
// and evaluated, for the roofline (bench.py) -- list entries it would fetch without early termination, pair words
// and 48-byte records it did fetch, records that survived the exact footprint test, (pixel, splat) evaluations
int msplat_get_composite_work(msplat_ctx* ctx, msplat_composite_work* out)
{
    drain_async(ctx);
    if (!ctx || !out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    std::memset(out, 0, sizeof(*out));
    if (!ctx->probe.p || !ctx->probe_on)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "tile probe not enabled (msplat_set_tile_probe)");
    if (!ctx->has_render) return fail(ctx, MSPLAT_ERR_NO_SORT, "no render yet");
    const uint32_t items = (uint32_t)(ctx->last_fp.tiles_x * ctx->last_fp.tiles_y) * 4u;
    std::vector<uint32_t> h;
    try {
        h.resize((size_t)items * kProbeWords);
    } catch (const std::exception&) {
        return fail(ctx, MSPLAT_ERR_HIP, "out of host memory");
    }
    int rc = msplat_debug_get_tile_probe8(ctx, h.data(), items);
    if (rc) return rc;
    for (uint32_t t = 0; t < items; ++t) {
        const uint32_t* p = &h[(size_t)t * kProbeWords];
        if (!p[7]) continue;
        out->work_items += 1;
        out->clocks_sum += p[0];
        out->clocks_max = std::max<uint64_t>(out->clocks_max, p[0]);
        out->records_composited += p[1];
        out->pixel_evals += (uint64_t)p[1] * (uint64_t)(kTile * kTile);
        out->batches += p[2];
        out->inner_clocks_sum += p[3];
        out->pair_words_fetched += p[4];
        out->records_fetched += p[5];
        out->list_entries += p[6];
        out->useful_evals += (uint64_t)(p[7] - 1u);
    }
    return MSPLAT_OK;
}

// the context's latest compositor launch as issue_compositor chose it: work items, workgroups launched, bins walked heaviest-first,
// kernel kind (0 splat compositor, 1 draw-order depth / target-rounding compositor, 2 points).  grid < items: persistent waves
// that pull from the work queue; grid == items: every item on its own wave.  A two-pass frame reports its first pass.
int msplat_debug_get_compositor_launch(msplat_ctx* ctx, uint32_t out[4])
{
    drain_async(ctx);
    if (!ctx || !out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->has_render) return fail(ctx, MSPLAT_ERR_NO_SORT, "no render yet");
    for (int i = 0; i < 4; ++i) out[i] = ctx->comp_launch[i];
    return MSPLAT_OK;
}

// the heavy chunks of the context's latest column pass: how many chunks bin1_upsweep found over kHeavyPairs (the host-mapped word
// bin1_downsweep leaves for the next frame's launch) and the helper slots issue_binning gave that downsweep
int msplat_debug_get_heavy_chunks(msplat_ctx* ctx, uint32_t out[2])
{
    drain_async(ctx);
    if (!ctx || !out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->has_render) return fail(ctx, MSPLAT_ERR_NO_SORT, "no render yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    out[0] = host_word(ctx, kHostHeavyChunks);
    out[1] = ctx->heavy_slots_launched;
    return MSPLAT_OK;
}

// the order[slot] -> bin table the context's latest compositor launch walked (the first pass's of a two-pass frame), read back from
// the device: tiles_x * tiles_y words
int msplat_debug_get_bin_order(msplat_ctx* ctx, uint32_t* out, uint32_t cap)
{
    drain_async(ctx);
    if (!ctx || !out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->has_render || !ctx->comp_order) return fail(ctx, MSPLAT_ERR_NO_SORT, "no render yet");
    if (cap < ctx->comp_order_bins) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "capacity %u < %u bins", cap, ctx->comp_order_bins);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->comp_order, (size_t)ctx->comp_order_bins * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MSPLAT_OK;
}

// bin_order_xcd with the compiled-in block shape, on the host (no context, no device)
int msplat_debug_bin_order(int32_t tiles_x, int32_t rows, uint32_t* out)
{
    if (!out || tiles_x < 1 || rows < 1 || tiles_x > 256 || rows > 256) return MSPLAT_ERR_INVALID_ARG;
    bin_order_xcd(tiles_x, rows, kBinBlockW, kBinBlockH, out);
    return MSPLAT_OK;
}

// FrameParams::view_scale2 as make_frame_params computes it from viewMat = inverse(cameraMat), on the host (no context, no device)
int msplat_debug_view_scale2(const float viewMat[16], float* out)
{
    if (!viewMat || !out) return MSPLAT_ERR_INVALID_ARG;
    *out = view_scale2_of(viewMat);
    return MSPLAT_OK;
}

int msplat_debug_get_tile_lists(msplat_ctx* ctx, uint32_t* tile_start, uint32_t tile_cap,
                                uint32_t* pairs, uint64_t pair_cap)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!ctx->has_render) return fail(ctx, MSPLAT_ERR_NO_SORT, "no render yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t ntiles = (uint32_t)(ctx->last_fp.tiles_x * ctx->last_fp.tiles_y);
    if (tile_cap < ntiles + 1) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "tile capacity too small");
    if (tile_start) HIP_TRY(ctx, hipMemcpy(tile_start, ctx->tile_start.p, (size_t)(ntiles + 1) * 4, hipMemcpyDeviceToHost));
    uint32_t cnt[4];
    HIP_TRY(ctx, hipMemcpy(cnt, ctx->counters.p, sizeof(cnt), hipMemcpyDeviceToHost));
    const uint64_t d = std::min<uint64_t>(cnt[kCntD], ctx->pair_cap);
    if (pairs) {
        if (pair_cap < d) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "pair capacity too small");
        if (d) HIP_TRY(ctx, hipMemcpy(pairs, ctx->pairsB.p, d * 4, hipMemcpyDeviceToHost));
    }
    return MSPLAT_OK;
}

// the partition the context's own stream got (MSPLAT_CU_*; ALL when the caller's stream is used or the extension refused) and,
// when mask8 != NULL, the stream's CU mask as the runtime reports it (8 words)
int msplat_debug_cu_partition(msplat_ctx* ctx, uint32_t* mask8)
{
    if (!ctx) return MSPLAT_ERR_INVALID_ARG;
    if (mask8) {
        memset(mask8, 0, 8 * sizeof(uint32_t));
        if (hipSetDevice(ctx->device) != hipSuccess || hipExtStreamGetCUMask(ctx->stream, 8, mask8) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, MSPLAT_ERR_HIP, "msplat_debug_cu_partition: hipExtStreamGetCUMask failed");
        }
    }
    return ctx->cu_partition;
}

int msplat_debug_upload_kernel_ms(msplat_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_debug_upload_kernel_ms: NULL argument");
    *ms = ctx->upload_kernel_ms;      // (run_ingest has drained the stream)
    return MSPLAT_OK;
}

int msplat_debug_get_positions(msplat_ctx* ctx, float* pos4_out, uint64_t cap_floats)
{
    drain_async(ctx);
    if (!ctx || !pos4_out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_debug_get_positions: NULL argument");
    if (!ctx->has_cloud) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "msplat_debug_get_positions: no cloud uploaded");
    if (cap_floats < 4 * ctx->N)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_debug_get_positions: capacity %llu < 4 x %llu floats", (unsigned long long)cap_floats,
                    (unsigned long long)ctx->N);
    if (ctx->N == 0) return MSPLAT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(pos4_out, ctx->pos4.p, ctx->N * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MSPLAT_OK;
}
