// msplat_edit.hip.inc -- what the calls that edit or annotate an uploaded cloud share, each written once: the front-door refusals, the
// f_rest failure, the kernel timing pair, the pinned staging slot, the selection scan, and the fresh store with the planes it keeps
// (textually part of msplat_device.hip: included inside its extern "C" block, before msplat_upload.hip.inc -- run_ingest is the first user)
//
// A cloud edit (msplat_compact_cloud, msplat_transform_cloud, msplat_append_cloud, msplat_adjust_cloud) reads: refusals, sync, ensure_order_dev, its own
// kernels into a FreshStore, fresh_adopt.  A new edit writes its kernels and calls fresh_adopt; a new per-splat plane in upload
// numbering joins KeptPlanes.

// (the upload tail, beside prepare_cloud_buffers, and the planes' allocators: defined in msplat_upload / _visibility / _overlay .hip.inc)
static int spatial_reorder(msplat_ctx* ctx);
static int vis_alloc(msplat_ctx* ctx);
static int check_device_source(msplat_ctx* ctx, const char* who, const char* what, const void* p, uint64_t bytes);
static int ensure_order_dev(msplat_ctx* ctx);
static int overlay_slot_alloc(msplat_ctx* ctx);

// ---- front-door refusals ----------------------------------------------------------------------------------------------------------
// the context must hold a splat cloud.  for_what: the caller's parenthesis ("visibility is for splat clouds"); note: what its
// no-cloud sentence adds
static int require_splat_cloud(msplat_ctx* ctx, const char* who, const char* for_what, const char* note = "")
{
    if (ctx->has_cloud && ctx->point_mode) return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: the context holds a point cloud (%s)", who, for_what);
    if (!ctx->has_cloud || !ctx->store) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "%s: no cloud uploaded%s", who, note);
    return MSPLAT_OK;
}

// a caller's array `what`: aligned to its elements of elem_bytes bytes ...
static int check_aligned(msplat_ctx* ctx, const char* who, const char* what, const void* p, unsigned elem_bytes)
{
    if ((uintptr_t)p % elem_bytes == 0) return MSPLAT_OK;
    return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s (%p) is not %u-byte aligned", who, what, p, elem_bytes);
}

// ... and `count` of them in device memory of the context's device (none: nothing to query).  A NULL p is the caller's to refuse or allow
static int check_device_array(msplat_ctx* ctx, const char* who, const char* what, const void* p, unsigned elem_bytes, uint64_t count)
{
    const int rc = check_aligned(ctx, who, what, p, elem_bytes);
    return rc || count == 0 ? rc : check_device_source(ctx, who, what, p, elem_bytes * count);
}

// n bytes, one per splat in upload numbering (a mask, a selection), for the cloud the context holds.  for_what: require_splat_cloud's
static int check_splat_count(msplat_ctx* ctx, const char* who, const char* for_what, uint64_t n)
{
    const int rc = require_splat_cloud(ctx, who, for_what, " (a mask is in the cloud's upload numbering)");
    if (rc || n == ctx->N) return rc;
    return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %llu mask bytes for a cloud of %llu splats", who, (unsigned long long)n, (unsigned long long)ctx->N);
}

// what the selection calls refuse first: check_splat_count, then the bytes -- `what`, device memory (NULL allowed where `optional`).
// (msplat_mark_ids, msplat_mark_scores and set_mask have checks of their own between the two, so their order is written out there)
static int check_splat_bytes(msplat_ctx* ctx, const char* who, const char* what, const void* d_bytes, uint64_t n, bool optional)
{
    const int rc = check_splat_count(ctx, who, "selection is for splat clouds", n);
    if (rc || n == 0 || (optional && !d_bytes)) return rc;
    if (!d_bytes) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s is NULL", who, what);
    return check_device_source(ctx, who, what, d_bytes, n);
}

// a column-major 4x4 affine matrix `name`: rows 0..2 finite
static int check_affine_finite(msplat_ctx* ctx, const char* who, const char* name, const float M[16])
{
    for (int k = 0; k < 16; ++k)
        if (k % 4 != 3 && !std::isfinite(M[k]))       // (row 3 is not read)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s[%d] is not finite", who, name, k);
    return MSPLAT_OK;
}

// what a store of compact SH refuses: n_over values the pack routines counted.  what: "" / "transformed " / "appended " / "adjusted ";
// tail: "" / "; the cloud is unchanged"
static int f_rest_failure(msplat_ctx* ctx, const char* who, int storage, uint64_t n_over, const char* what, const char* tail)
{
    if (storage == kStorageShQ8)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %llu %sf_rest values are not finite: MSPLAT_STORAGE_SH_Q8 cannot quantise them%s", who,
                    (unsigned long long)n_over, what, tail);
    return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %llu %sf_rest values are beyond the fp16 range (|c| >= 65520) of MSPLAT_STORAGE_SH_FP16%s",
                who, (unsigned long long)n_over, what, tail);
}

// ---- the event pair behind msplat_debug_upload_kernel_ms (msplat_config.enable_timing) -----------------------------------------------
// start / stop bracket the caller's kernels on the stream, read() takes the time once the stream has drained; a call that does
// not get there leaves -1
struct KernelTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool on;
    explicit KernelTimer(msplat_ctx* ctx)
    {
        on = ctx->cfg.enable_timing > 0 && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
        ctx->upload_kernel_ms = -1.0f;
    }
    ~KernelTimer()
    {
        for (hipEvent_t v : ev)
            if (v) (void)hipEventDestroy(v);
    }
    void start(hipStream_t s) { if (on) (void)hipEventRecord(ev[0], s); }
    void stop(hipStream_t s) { if (on) (void)hipEventRecord(ev[1], s); }
    void read(msplat_ctx* ctx) { if (on && hipEventElapsedTime(&ctx->upload_kernel_ms, ev[0], ev[1]) != hipSuccess) ctx->upload_kernel_ms = -1.0f; }
};

extern "C++" {      // (templates)
// ---- a mark's launch: one lane per item (splat, pixel), asynchronous on the context's stream ------------------------------------------
template <class Kernel, class... Args>
static int launch_per_item(msplat_ctx* ctx, const char* who, uint64_t items, Kernel kernel, const Args&... args)
{
    hipLaunchKernelGGL(kernel, dim3(div_up(items, kThreads)), dim3(kThreads), 0, ctx->stream, args...);
    if (hipGetLastError() != hipSuccess) return fail(ctx, MSPLAT_ERR_HIP, "%s: the kernel launch failed", who);
    return MSPLAT_OK;
}

// ---- the host side of a row reduction (msplat_rows.hip.h) over n items: part holds kGridCap + 1 rows, the partials and the total -------
// launch_partial(grid, part) issues the call's grid-stride kernel, rows_finish_kernel folds its `grid` rows, and `row` is the total
// once the stream has drained; more_copies() issues what else the call copies out before that.  (KernelTimer: both kernels)
template <class Row, class Partial, class Copies>
static int reduce_rows(msplat_ctx* ctx, const char* who, Row* part, uint64_t n, Row& row, Partial&& launch_partial, Copies&& more_copies)
{
    Row* total = part + kGridCap;
    const int grid = grid_for(div_up(n, kThreads), ctx->grid_cap);
    KernelTimer timer(ctx);
    timer.start(ctx->stream);
    launch_partial(grid, part);
    hipLaunchKernelGGL(rows_finish_kernel<Row>, dim3(1), dim3(kThreads), 0, ctx->stream, (const Row*)part, (uint32_t)grid, total);
    timer.stop(ctx->stream);
    if (hipGetLastError() != hipSuccess) return fail(ctx, MSPLAT_ERR_HIP, "%s: a kernel launch failed", who);
    HIP_TRY(ctx, hipMemcpyAsync(&row, total, sizeof(Row), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, more_copies());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    timer.read(ctx);
    return MSPLAT_OK;
}
}  // extern "C++"

// ---- the pinned staging slot (StagingSlot, msplat_device.hip): host bytes to the device on a stream of the context's, the caller's
// array free on return and no drain of the frames queued before ------------------------------------------------------------------
// the slot's buffer, at least n bytes, once the copy that last read it has left it (an event: no drain)
static int stage_reserve(msplat_ctx* ctx, StagingSlot& sl, size_t n)
{
    if (sl.ev) HIP_TRY(ctx, hipEventSynchronize(sl.ev));
    else HIP_TRY(ctx, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (sl.bytes < n) {
        if (sl.host) (void)hipHostFree(sl.host);
        sl.host = nullptr;
        sl.bytes = 0;
        HIP_TRY(ctx, hipHostMalloc(&sl.host, n, hipHostMallocDefault));
        sl.bytes = n;
    }
    return MSPLAT_OK;
}

// the slot's first n bytes to dst, on stream s
static int stage_send(msplat_ctx* ctx, StagingSlot& sl, void* dst, size_t n, hipStream_t s)
{
    HIP_TRY(ctx, hipMemcpyAsync(dst, sl.host, n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(sl.ev, s));
    return MSPLAT_OK;
}

// n host bytes at src to dst through the slot, on the context's stream
static int stage_copy(msplat_ctx* ctx, StagingSlot& sl, void* dst, const void* src, size_t n)
{
    int rc = stage_reserve(ctx, sl, n);
    if (rc) return rc;
    std::memcpy(sl.host, src, n);
    return stage_send(ctx, sl, dst, n, ctx->stream);
}

static void stage_free(StagingSlot& sl)
{
    if (sl.host) (void)hipHostFree(sl.host);
    if (sl.ev) (void)hipEventDestroy(sl.ev);
    sl = StagingSlot{};
}

// ---- the selection scan (msplat_compact.hip.h): a flag byte per splat -> the rank of every flagged splat among the flagged, and K ----
// One scratch buffer: flags padded to whole chunks | chunk counts | K | the ranks, unless the caller's array takes them.  The
// caller's own kernel writes the flags between scan_reserve and scan_number
struct SelectionScan {
    msplat_ctx* ctx;
    Buf tmp;
    uint32_t n = 0, nchunks = 0, K = 0;
    size_t flag_bytes = 0;
    uint8_t* flags = nullptr;
    uint32_t *counts = nullptr, *total = nullptr, *rank = nullptr;
    explicit SelectionScan(msplat_ctx* c) : ctx(c) {}
    ~SelectionScan() { buf_free(ctx, tmp); }
};

static int scan_reserve(SelectionScan& sc, uint64_t n, uint32_t* caller_rank)
{
    sc.n = (uint32_t)n;
    sc.nchunks = div_up(n, kCompactChunk);
    sc.flag_bytes = (size_t)sc.nchunks * kCompactChunk;
    const size_t total_off = sc.flag_bytes + (size_t)sc.nchunks * 4, rank_off = (total_off + 4 + 15) & ~(size_t)15;
    int rc = buf_alloc(sc.ctx, sc.tmp, rank_off + (caller_rank ? 0 : (size_t)n * 4));
    if (rc) return rc;
    sc.flags = (uint8_t*)sc.tmp.p;
    sc.counts = (uint32_t*)((char*)sc.tmp.p + sc.flag_bytes);
    sc.total = (uint32_t*)((char*)sc.tmp.p + total_off);
    sc.rank = caller_rank ? caller_rank : (uint32_t*)((char*)sc.tmp.p + rank_off);
    return MSPLAT_OK;
}

// count, offsets and index behind the caller's flags kernel, then K on the host (the stream has drained).  e: what the caller's
// own launches returned; what: "kept" / "selected"
static int scan_number(SelectionScan& sc, const char* who, const char* what, hipError_t e)
{
    msplat_ctx* ctx = sc.ctx;
    hipStream_t s = ctx->stream;
    if (e == hipSuccess) {
        const int gchunks = grid_for(sc.nchunks, ctx->grid_cap);
        hipLaunchKernelGGL(compact_count_kernel, dim3(gchunks), dim3(kThreads), 0, s, (const uint8_t*)sc.flags, sc.nchunks, sc.counts);
        hipLaunchKernelGGL(compact_offsets_kernel, dim3(1), dim3(kThreads), 0, s, sc.counts, sc.nchunks, sc.total);
        hipLaunchKernelGGL(compact_index_kernel, dim3(gchunks), dim3(kThreads), 0, s, (const uint8_t*)sc.flags, (const uint32_t*)sc.counts,
                           sc.n, sc.nchunks, sc.rank);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&sc.K, sc.total, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ctx, MSPLAT_ERR_HIP, "%s: numbering the %s splats failed: %s", who, what, hipGetErrorString(e));
    return MSPLAT_OK;
}

// ---- planes in upload numbering that outlive an edit: the visibility mask and the overlay's classes ---------------------------------
// An edit that keeps the numbering, or extends it by `added` splats, keeps both.  A cloud that grows gets its longer planes built
// BEFORE the swap (kept_grow: the old bytes, then `added` bytes of 1 = visible / of class 0), so that running out of memory for
// them leaves the cloud unchanged.  fresh_adopt takes the planes out of prepare_cloud_buffers' hands, hands them back and makes them
// valid for the new store.  Whatever was not handed over goes with the struct
struct KeptPlanes {
    msplat_ctx* ctx;
    const bool had_mask, had_classes;
    Buf mask, cls;          // the planes of the cloud after the edit: built by kept_grow, or the context's own (kept_take)
    explicit KeptPlanes(msplat_ctx* c) : ctx(c), had_mask(c->has_mask), had_classes(c->has_classes) {}
    ~KeptPlanes() { buf_free(ctx, mask); buf_free(ctx, cls); }
};

// `out`: n_old bytes of `old`, then `added` bytes of `fill`, on the context's stream
static hipError_t kept_extend(msplat_ctx* ctx, const Buf& old, Buf& out, uint64_t n_old, uint64_t added, int fill)
{
    if (buf_alloc(ctx, out, std::max<uint64_t>(n_old + added, 1))) return hipErrorOutOfMemory;
    hipError_t e = hipSuccess;
    if (n_old) e = hipMemcpyAsync(out.p, old.p, n_old, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && added) e = hipMemsetAsync((char*)out.p + n_old, fill, added, ctx->stream);
    return e;
}

static hipError_t kept_grow(KeptPlanes& k, uint64_t n_old, uint64_t added)
{
    hipError_t e = hipSuccess;
    if (k.had_mask && added) e = kept_extend(k.ctx, k.ctx->vis_mask, k.mask, n_old, added, 1);
    if (e == hipSuccess && k.had_classes && added) e = kept_extend(k.ctx, k.ctx->ov_cls, k.cls, n_old, added, 0);
    return e;
}

// a plane that was not rebuilt is the context's own buffer: out of the context, so that prepare_cloud_buffers does not free it
static void kept_take(bool had, Buf& member, Buf& plane)
{
    if (!had || plane.p) return;
    plane = member;
    member = Buf{};
}

// the plane into the context's member (a member since the plane was set: msplat_destroy knows it), in place of what is left there
static void kept_give(msplat_ctx* ctx, Buf& member, Buf& plane)
{
    if (!plane.p) return;
    buf_free(ctx, member);
    member.p = plane.p;
    member.bytes = plane.bytes;
    plane = Buf{};
}

// ---- the fresh store of an edit, never the old allocation: until fresh_adopt swaps it in the context renders what it rendered
// before, so every failure up to there leaves the cloud unchanged --------------------------------------------------------------
struct FreshStore {
    std::shared_ptr<CloudStore> st;     // frees its records when an early return drops it
    uint32_t* d_over = nullptr;         // the pack routines' counter, zeroed on the stream, where the caller asked for one
    ~FreshStore() { if (d_over) (void)hipFree(d_over); }
};

// a store of the old one's kind with room for max(n, 1) rows of F4 float4
static hipError_t fresh_alloc(msplat_ctx* ctx, FreshStore& fs, uint64_t n, int F4, int storage, bool counter)
{
    try {      // the C ABI never throws
        fs.st = std::make_shared<CloudStore>();
    } catch (const std::exception&) {
        return hipErrorOutOfMemory;
    }
    CloudStore& st = *fs.st;
    st.device = ctx->device;
    st.storage = storage;
    st.F4 = F4;
    const size_t alloc_n = std::max<uint64_t>(n, 1);
    hipError_t e = hipMalloc(&st.pos4.p, alloc_n * 16);
    if (e == hipSuccess) st.pos4.bytes = alloc_n * 16;
    if (e == hipSuccess) e = hipMalloc(&st.recs.p, alloc_n * F4 * 16);
    if (e == hipSuccess) st.recs.bytes = alloc_n * F4 * 16;
    if (e == hipSuccess && counter) e = hipMalloc((void**)&fs.d_over, 16);
    if (e == hipSuccess && counter) e = hipMemsetAsync(fs.d_over, 0, 4, ctx->stream);
    return e;
}

// The tail every edit shares, the stream being idle and the records in place in upload order: from here on an upload of n splats.
// The store goes through prepare_cloud_buffers as a store to adopt (its `share` argument): that keeps the path from reusing the
// old allocation, takes the storage kind from the store and not from msplat_set_cloud_storage, and finds order / boxes empty as a
// fresh store has them.  kept: the planes that stay (null: the numbering changed, both go as at an upload)
static int fresh_adopt(msplat_ctx* ctx, FreshStore& fs, uint64_t n, bool full_sh, KeptPlanes* kept)
{
    const std::shared_ptr<CloudStore> st = std::move(fs.st);
    const size_t bytes = st->pos4.bytes + st->recs.bytes;
    if (kept) {
        kept_take(kept->had_mask, ctx->vis_mask, kept->mask);
        kept_take(kept->had_classes, ctx->ov_cls, kept->cls);
    }
    int rc = prepare_cloud_buffers(ctx, n, full_sh, st);
    if (kept) {
        kept_give(ctx, ctx->vis_mask, kept->mask);
        kept_give(ctx, ctx->ov_cls, kept->cls);
    }
    if (ctx->store == st) ctx->device_bytes += bytes;       // the adopted store is the context's own: it counts
    if (rc) return rc;
    if ((rc = spatial_reorder(ctx))) return rc;
    if (kept && kept->had_mask) {         // the plane, the boxes and the new store's order on the device, as set_mask leaves them
        if ((rc = vis_alloc(ctx)) || (rc = ensure_order_dev(ctx))) return rc;
        ctx->has_mask = true;
        ctx->vis_dirty = true;
    }
    if (kept && kept->had_classes) {      // the slot array and the order, as set_overlay_classes leaves them
        if ((rc = overlay_slot_alloc(ctx))) return rc;
        ctx->has_classes = true;
        ctx->overlay_dirty = true;
    }
    ctx->has_cloud = true;
    return MSPLAT_OK;
}
