// msplat_upload.hip.inc -- SplatRenderer::Init: per-cloud buffers, the spatial storage order, cloud / PLY / point uploads, the sprite, download
// (textually part of msplat_device.hip: included inside its extern "C" block, after struct msplat_ctx, the helpers and msplat_edit.hip.inc -- the
// f_rest failure and the kernel timing pair are written there; r6 split, VERDICT r5 item 7)

// a table the frame's kernels keep clean, zero-filled (the stream is idle whenever buffers are (re)allocated)
static int alloc_frame_table(msplat_ctx* ctx, Buf& b, size_t bytes)
{
    int rc = buf_alloc(ctx, b, bytes);
    if (rc) return rc;
    b.frame_table = true;
    HIP_TRY(ctx, hipMemsetAsync(b.p, 0, b.bytes, ctx->stream));
    return MSPLAT_OK;
}

// group table for `nchunks` chunk rows
static int alloc_group_table(msplat_ctx* ctx, GroupTable& t, uint64_t nchunks)
{
    t.sup = (uint32_t)((nchunks >> kSuperShift) + 2);                    // supergroup rows first, then the group rows
    int rc = alloc_frame_table(ctx, t.buf, (size_t)(t.sup + (nchunks >> kGroupShift) + 2) * 256 * sizeof(uint32_t));
    t.rows = (uint32_t)(t.buf.bytes / (256 * sizeof(uint32_t)));
    return rc;
}

static int ensure_pair_capacity(msplat_ctx* ctx, uint64_t cap)
{
    if (cap > 0x7FFFFFFFull) cap = 0x7FFFFFFFull;
    if (ctx->pair_cap >= cap && ctx->pairsA.p) return MSPLAT_OK;
    int rc = buf_alloc(ctx, ctx->pairsA, cap * sizeof(uint32_t));
    if (rc) return rc;
    rc = buf_alloc(ctx, ctx->pairsB, cap * sizeof(uint32_t));
    if (rc) return rc;
    ctx->hist2.stride = div_up(cap, kPairChunk);
    rc = buf_alloc(ctx, ctx->hist2.buf, (size_t)256 * ctx->hist2.stride * sizeof(uint32_t));
    if (rc) return rc;
    rc = alloc_group_table(ctx, ctx->gsumB2, ctx->hist2.stride);
    if (rc) return rc;
    ctx->pair_cap = cap;
    return MSPLAT_OK;
}

// What a cloud's size and the context's frame mode decide about the wide sort -- whether it runs, its threads, keys per thread and
// group shift -- and its tables, sized by that
static int plan_wide_sort(msplat_ctx* ctx, uint64_t n)
{
    WideSort& w = ctx->ws;
    // the three wide passes at every size.  (r3-r5: contexts with frames in flight took the four 8-bit passes beyond 2 M splats --
    // 6 M: 1616 against 1497 frames/s then.  Since the 16-key variants lost their spills (r6) the three passes win there too, with
    // two frames per half of the CUs: 6 M / 1080p 2384-2435 -> 2464-2473 frames/s, 6 M / 4096^2 1324-1331 -> 1381-1398; the scene-like
    // 6 M cloud -1 %: EXPERIMENTS.md.  MSPLAT_SORT=lsd8 still selects the 8-bit passes.)
    w.on = ctx->wide_sort_cfg;
    // frames in flight: the sort's 256-thread form (4096-key chunks of 4 waves find slots between other frames' workgroups) up to
    // 2 M splats, its 512-thread form beyond (r6: 6 M / 1080p 2478-2514 -> 2572-2591 frames/s, 6 M / 4096^2 unchanged; at 1 M the
    // 512-thread form loses 2 %: EXPERIMENTS.md)
    if (ctx->cfg.frame_mode == MSPLAT_FRAMES_IN_FLIGHT) w.threads = n > (2u << 20) ? (uint32_t)kWsThreads : (uint32_t)kWsThreadsSmall;
    if (!w.on) return MSPLAT_OK;
    // 4096-key chunks up to 2 M splats, 8192 beyond; groups of 16 chunk rows while
    // there are at most 512 rows, else of 32 (a downsweep sums <= nchunks / G + G - 1 rows)
    w.items = n > (2u << 20) ? 16u : 8u;
    // (the tables are sized for 8 keys per thread: passes 1 and 2 drop to that when few splats survive the cull, issue_wide_sort)
    const uint32_t nch = std::max(1u, div_up(n, (uint64_t)w.threads * 8u));
    w.gshift = nch <= 512u ? 4u : 5u;
    w.gsum_words = (uint32_t)(((nch >> w.gshift) + 2) * kWsMaxBins);
    int rc = buf_alloc(ctx, w.hist, (size_t)nch * kWsMaxBins * 4);
    for (auto& g : w.gsum)
        if (!rc) rc = alloc_frame_table(ctx, g, (size_t)w.gsum_words * 4);
    if (!rc) rc = buf_alloc(ctx, ctx->vmask, (size_t)div_up(std::max<uint64_t>(n, 1), 64) * 8 + 64);
    return rc;
}

// (host arithmetic: the uploads from device memory refuse the count before their first HIP call)
static int check_splat_count(msplat_ctx* ctx, uint64_t n)
{
    if (n > (1ull << 24))
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%llu splats > 2^24 (rank field is 24 bit)", (unsigned long long)n);
    return MSPLAT_OK;
}

// the plane and the boxes a context with a mask or a crop sorts from, for the N it holds
static int vis_alloc(msplat_ctx* ctx)
{
    const size_t n = std::max<uint64_t>(ctx->N, 1);
    int rc = buf_alloc(ctx, ctx->vis_pos4, n * sizeof(float4));
    if (!rc) rc = buf_alloc(ctx, ctx->vis_boxes, (size_t)div_up(n, kBoxSplats) * sizeof(CullBox));
    return rc;
}

// (re)allocates every per-cloud device buffer for n splats; leaves the context without a cloud.
// `share` != null: use that store's cloud instead of allocating one (msplat_attach_cloud).
static int prepare_cloud_buffers(msplat_ctx* ctx, uint64_t n, bool full_sh, const std::shared_ptr<CloudStore>& share)
{
    int rc_n = check_splat_count(ctx, n);
    if (rc_n) return rc_n;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->has_cloud = false;
    ctx->has_sort = false;
    ctx->has_render = false;
    ctx->N = n;
    ctx->full_sh = full_sh;
    // visibility: a mask speaks the old cloud's numbering and goes; a crop is world space and stays, evaluated on the new positions
    // by the next Sort (the stream is idle: the buffers may be freed)
    ctx->has_mask = ctx->vis_sorted = false;
    buf_free(ctx, ctx->vis_mask);
    // the overlay: the classes speak the old numbering too and go with the mask; the palette stays
    ctx->has_classes = ctx->overlay_dirty = false;
    buf_free(ctx, ctx->ov_cls);
    buf_free(ctx, ctx->ov_slot);
    if (ctx->crop_shape != 0 && !ctx->point_mode) {
        int rc_v = vis_alloc(ctx);
        if (rc_v) return rc_v;
        ctx->vis_dirty = true;
    } else {
        buf_free(ctx, ctx->vis_pos4);
        buf_free(ctx, ctx->vis_boxes);
    }
    // the storage kind belongs to the store: attached contexts render the owner's, point clouds are always FP32, and so is a
    // degree-1 cloud asked to be SH_Q8 (its FP32 record is one 128-B line already)
    int storage = share ? share->storage : (ctx->point_mode ? kStorageFp32 : ctx->storage_cfg);
    if (storage == kStorageShQ8 && !full_sh) storage = kStorageFp32;
    const int F4 = ctx->point_mode ? 1 : cloud_f4(storage, ctx->full_sh);
    const size_t alloc_n = std::max<uint64_t>(n, 1);
    int rc;
    if (share) {
        if (ctx->store && ctx->store != share && ctx->store.use_count() == 1)
            ctx->device_bytes -= ctx->store->pos4.bytes + ctx->store->recs.bytes;
        ctx->store = share;
    } else {
        const size_t need_pos = alloc_n * 16, need_rec = alloc_n * F4 * 16;
        // (a store of another storage kind is not reused: device_bytes then describes the records in use)
        const bool reuse = ctx->store && ctx->store.use_count() == 1 && ctx->store->pos4.bytes >= need_pos &&
                           ctx->store->recs.bytes >= need_rec && ctx->store->storage == storage;
        if (!reuse) {
            if (ctx->store && ctx->store.use_count() == 1)
                ctx->device_bytes -= ctx->store->pos4.bytes + ctx->store->recs.bytes;
            ctx->pos4 = Buf{};
            ctx->recs = Buf{};
            ctx->store.reset();
            auto st = std::make_shared<CloudStore>();
            st->device = ctx->device;
            HIP_TRY(ctx, hipMalloc(&st->pos4.p, need_pos));
            st->pos4.bytes = need_pos;
            HIP_TRY(ctx, hipMalloc(&st->recs.p, need_rec));
            st->recs.bytes = need_rec;
            ctx->device_bytes += need_pos + need_rec;
            ctx->store = st;
        }
        ctx->store->storage = storage;
        ctx->store->F4 = F4;
        // a fresh upload starts in upload order (spatial_reorder runs once the cloud is on the device)
        ctx->store->reordered = false;
        ctx->store->order_host.clear();
        if (ctx->store->order_dev.p) { (void)hipFree(ctx->store->order_dev.p); ctx->store->order_dev = Buf{}; }
        if (ctx->store->boxes.p) { (void)hipFree(ctx->store->boxes.p); ctx->store->boxes = Buf{}; }
        ctx->store->nboxes = 0;
    }
    ctx->pos4 = ctx->store->pos4;
    ctx->recs = ctx->store->recs;
    ctx->cloud_storage = ctx->store->storage;
    if ((rc = buf_alloc(ctx, ctx->keyA, alloc_n * 4))) return rc;
    if ((rc = buf_alloc(ctx, ctx->keyB, alloc_n * 4))) return rc;
    if ((rc = buf_alloc(ctx, ctx->valA, alloc_n * 4))) return rc;
    if ((rc = buf_alloc(ctx, ctx->valB, alloc_n * 4))) return rc;
    ctx->hist.stride = std::max(1u, div_up(n, kSortChunk));
    if ((rc = buf_alloc(ctx, ctx->hist.buf, (size_t)256 * ctx->hist.stride * 4))) return rc;
    // the sort's pair: every pass clears one table while it fills the other, so both are launched with the smaller row count
    for (auto& g : ctx->gsumS)
        if ((rc = alloc_group_table(ctx, g, ctx->hist.stride))) return rc;
    ctx->gsumS[0].rows = ctx->gsumS[1].rows = std::min(ctx->gsumS[0].rows, ctx->gsumS[1].rows);
    if ((rc = plan_wide_sort(ctx, n))) return rc;
    if ((rc = buf_alloc(ctx, ctx->live_list, ((size_t)div_up(div_up(alloc_n, kBoxSplats), kBoxGroup) * kBoxGroup + 16) * 4))) return rc;
    if ((rc = buf_alloc(ctx, ctx->live_cnt, 256 * 4))) return rc;
    ctx->rank_cap = alloc_n;
    if ((rc = buf_alloc(ctx, ctx->rec2d, alloc_n * 48))) return rc;
    if ((rc = buf_alloc(ctx, ctx->rect, alloc_n * 4))) return rc;
    if (ctx->depth_bits != 0 && (rc = buf_alloc(ctx, ctx->zq, alloc_n * 4))) return rc;
    // (column pass: 1024-rank chunks; 2048 measured r3 at 6 M: binning 183 -> 191 us at 1080p, 459 -> 453 us at 4096^2)
    if ((rc = alloc_frame_table(ctx, ctx->heavy, (size_t)2 * (1 + kHeavyCap) * 4))) return rc;
    if ((rc = buf_alloc(ctx, ctx->heavy_flag, (size_t)div_up(alloc_n, kBinChunk) + 64))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->heavy_flag.p, 0, ctx->heavy_flag.bytes, ctx->stream));
    ctx->hist1.stride = std::max(1u, div_up(n, kBinChunk));
    if ((rc = buf_alloc(ctx, ctx->hist1.buf, (size_t)256 * ctx->hist1.stride * 4))) return rc;
    if ((rc = alloc_group_table(ctx, ctx->gsumB1, ctx->hist1.stride))) return rc;
    uint64_t cap = ctx->cfg.pair_capacity ? ctx->cfg.pair_capacity
                                          : std::max<uint64_t>(1ull << 22, std::min<uint64_t>(32 * n, 1ull << 30));
    return ensure_pair_capacity(ctx, cap);
}

// Spatial storage order (r4, msplat_common.hip.h: box_live).  Called at the end of an upload, the cloud being on the device in
// UPLOAD order: Morton codes of the positions, a stable sort of (code, upload index) with the library's own 8-bit radix passes,
// the cloud gathered into that order, one bounding box per kBoxSplats slots.  From then on slot j holds upload index
// order_host[j]; everything that reports splat numbers (msplat_get_sorted_indices, msplat_download_cloud) maps back.
// Draw order = ascending key, ties in ascending STORAGE slot: for a cloud that is not reordered that is the upload index.
// Out of device memory for the second copy: the cloud simply stays in upload order.
static int spatial_reorder(msplat_ctx* ctx)
{
    const uint64_t n64 = ctx->N;
    const bool want = !ctx->point_mode && n64 > 1 &&
                      (ctx->spatial_mode == MSPLAT_SPATIAL_ON || (ctx->spatial_mode == MSPLAT_SPATIAL_AUTO && n64 >= kSpatialMinSplats));
    if (!want) return MSPLAT_OK;
    CloudStore& st = *ctx->store;
    hipStream_t s = ctx->stream;
    const uint32_t N = (uint32_t)n64;
    const int F4 = st.F4;
    const size_t need_pos = (size_t)N * 16, need_rec = (size_t)N * F4 * 16;
    void *npos = nullptr, *nrec = nullptr;
    if (hipMalloc(&npos, need_pos) != hipSuccess || hipMalloc(&nrec, need_rec) != hipSuccess) {
        (void)hipGetLastError();
        if (npos) (void)hipFree(npos);
        return MSPLAT_OK;
    }
    double* acc = (double*)ctx->totals1.p;          // 1 KB, idle outside a render
    uint32_t *kA = words(ctx->keyA), *vA = words(ctx->valA);
    const float4* pos = (const float4*)st.pos4.p;
    const uint32_t mrows = std::min(div_up(N, kThreads), 1024u);
    void* mpart = nullptr;
    hipError_t e = hipMalloc(&mpart, (size_t)mrows * kMoments * sizeof(double));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(npos); (void)hipFree(nrec);
        return MSPLAT_OK;
    }
    hipLaunchKernelGGL(cloud_moments_kernel, dim3(mrows), dim3(kThreads), 0, s, pos, N, (double*)mpart);
    hipLaunchKernelGGL(cloud_moments_finish, dim3(1), dim3(kThreads), 0, s, (const double*)mpart, mrows, acc);
    hipLaunchKernelGGL(morton_kernel, dim3(div_up(N, kThreads)), dim3(kThreads), 0, s, pos, N, (const double*)acc, kA, vA);
    const bool large = n64 > (2u << 20);
    const int grid = grid_for(div_up(N, (uint32_t)kThreads * (large ? kSortItemsLarge : kSortItems)), ctx->grid_cap);
    FrameParams fp0;
    std::memset(&fp0, 0, sizeof(fp0));
    RadixPass a;            // a static n, the scanned form, no group table touched
    a.n_static = a.n_cap = N;  a.fp = &fp0;
    a.hist = &ctx->hist;  a.totals = words(ctx->totals);
    for (int pass = 0; pass < 4; ++pass) {          // A -> B -> A -> B -> A
        a.buffers(ctx, pass & 1);
        a.shift = pass * 8;
        issue_radix_pass(ctx, int_t<MODE_KEYS>{}, flag_t<true>{}, large, grid, a);
    }
    hipLaunchKernelGGL(gather_cloud_kernel, dim3(2048), dim3(kThreads), 0, s, (const uint32_t*)vA, N, F4, pos,
                       (const float4*)st.recs.p, (float4*)npos, (float4*)nrec);
    const uint32_t nboxes = div_up(N, kBoxSplats);
    void* nbox = nullptr;
    if (e == hipSuccess) e = hipMalloc(&nbox, (size_t)nboxes * sizeof(CullBox));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cull_boxes_kernel, dim3(nboxes), dim3(kThreads), 0, s, (const float4*)npos, N, (CullBox*)nbox);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        try {
            st.order_host.resize(N);
        } catch (const std::exception&) {
            e = hipErrorOutOfMemory;
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(st.order_host.data(), vA, (size_t)N * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(mpart);
    if (e != hipSuccess) {
        (void)hipFree(npos); (void)hipFree(nrec);
        if (nbox) (void)hipFree(nbox);
        st.order_host.clear();
        return fail(ctx, MSPLAT_ERR_HIP, "spatial reordering of the cloud failed: %s", hipGetErrorString(e));
    }
    (void)hipFree(st.pos4.p); (void)hipFree(st.recs.p);
    st.pos4.p = npos; st.pos4.bytes = need_pos;
    st.recs.p = nrec; st.recs.bytes = need_rec;
    st.boxes.p = nbox; st.boxes.bytes = (size_t)nboxes * sizeof(CullBox);
    st.nboxes = nboxes;
    st.reordered = true;
    ctx->pos4 = st.pos4;
    ctx->recs = st.recs;
    return MSPLAT_OK;
}

int msplat_upload_cloud(msplat_ctx* ctx, const void* aos, uint64_t n, uint32_t stride_bytes,
                        const msplat_attr_offsets* off, int full_sh)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if ((!aos && n) || !off) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_upload_cloud: NULL argument");
    if (stride_bytes % 4 != 0) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "stride must be a multiple of 4");
    ctx->point_mode = false;
    int rc = prepare_cloud_buffers(ctx, n, full_sh != 0, nullptr);
    if (rc) return rc;
    const int F4 = ctx->store->F4;
    const bool sh16 = ctx->cloud_storage == kStorageShFp16, sh8 = ctx->cloud_storage == kStorageShQ8;
    uint64_t n_over = 0;

    // repack: reference AoS (100 B / 244 B, arbitrary offsets) -> 16-byte aligned padded records with the
    // reference's float order (gaussiancloud.cpp:32-56), plus the vec4(x,y,z,1) array of splatrenderer.cpp:106-111
    const size_t chunk = 1u << 18;
    std::vector<float> stage_rec, stage_pos;
    try {      // the C ABI never throws
        stage_rec.resize(chunk * F4 * 4);
        stage_pos.resize(chunk * 4);
    } catch (const std::exception&) {
        return fail(ctx, MSPLAT_ERR_HIP, "msplat_upload_cloud: out of host memory for the staging buffers");
    }
    const uint32_t src_off_base[7] = {off->pos_with_alpha, off->r_sh0, off->g_sh0, off->b_sh0,
                                      off->cov3_col0, off->cov3_col1, off->cov3_col2};
    const uint32_t src_off_full[9] = {off->r_sh1, off->r_sh2, off->r_sh3, off->g_sh1, off->g_sh2, off->g_sh3,
                                      off->b_sh1, off->b_sh2, off->b_sh3};
    for (int k = 0; k < 7; ++k)
        if (src_off_base[k] + (k < 4 ? 16u : 12u) > stride_bytes)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "attribute offset %u beyond stride %u", src_off_base[k], stride_bytes);
    if (ctx->full_sh)
        for (int k = 0; k < 9; ++k)
            if (src_off_full[k] + 16u > stride_bytes)
                return fail(ctx, MSPLAT_ERR_INVALID_ARG, "attribute offset %u beyond stride %u", src_off_full[k], stride_bytes);
    const uint8_t* src = static_cast<const uint8_t*>(aos);
    for (uint64_t base = 0; base < n; base += chunk) {
        const size_t cnt = (size_t)std::min<uint64_t>(chunk, n - base);
        for (size_t j = 0; j < cnt; ++j) {
            const uint8_t* rec = src + (base + j) * stride_bytes;
            float full[64];
            float* d = sh16 || sh8 ? full : stage_rec.data() + j * F4 * 4;
            std::memcpy(d + 0, rec + off->pos_with_alpha, 16);
            std::memcpy(d + 4, rec + off->r_sh0, 16);
            std::memcpy(d + 8, rec + off->g_sh0, 16);
            std::memcpy(d + 12, rec + off->b_sh0, 16);
            std::memcpy(d + 16, rec + off->cov3_col0, 12);
            std::memcpy(d + 19, rec + off->cov3_col1, 12);
            std::memcpy(d + 22, rec + off->cov3_col2, 12);
            if (ctx->full_sh) {
                for (int k = 0; k < 9; ++k) std::memcpy(d + 25 + 4 * k, rec + src_off_full[k], 16);
                d[61] = d[62] = d[63] = 0.0f;
            } else {
                for (int k = 25; k < 32; ++k) d[k] = 0.0f;
            }
            float* p = stage_pos.data() + j * 4;
            p[0] = d[0]; p[1] = d[1]; p[2] = d[2]; p[3] = footprint_bound(d + 16, d[3]);      // .w: footprint bound for the band cull
            if (sh16 || sh8) {
                uint32_t* w = reinterpret_cast<uint32_t*>(stage_rec.data() + j * F4 * 4);
                if (sh8) n_over += sh8_pack<true>(d, w);
                else n_over += ctx->full_sh ? sh16_pack<true>(d, w) : sh16_pack<false>(d, w);
            }
        }
        HIP_TRY(ctx, hipMemcpy((char*)ctx->recs.p + base * F4 * 16, stage_rec.data(), cnt * F4 * 16, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy((char*)ctx->pos4.p + base * 16, stage_pos.data(), cnt * 16, hipMemcpyHostToDevice));
    }
    if (n_over) return f_rest_failure(ctx, "msplat_upload_cloud", ctx->cloud_storage, n_over, "", "");
    if ((rc = spatial_reorder(ctx))) return rc;
    ctx->has_cloud = true;
    return MSPLAT_OK;
}


// ---- GPU ingest (SURVEY.md 8f-1): the upload kernels of msplat_cloud.hip.h, each run around one counter ------------------
// The launch every ingest route shares.  `e`: what the route's own staging copy (if any) returned; launch(SH, ST) issues the
// route's kernel for the store's <full SH, storage> pair with d_over as its counter.  Returns after the stream has drained; the
// f_rest failures are msplat_upload_cloud's, in its words, under the route's name.  (enable_timing: the kernel alone between two
// stream events, msplat_debug_upload_kernel_ms.)
extern "C++" {      // (a template)
template <class Launch>
static int run_ingest(msplat_ctx* ctx, const char* who, uint32_t* d_over, hipError_t e, Launch&& launch)
{
    uint32_t n_over = 0;
    const bool counted = ctx->cloud_storage == kStorageShQ8 || ctx->cloud_storage == kStorageShFp16;
    KernelTimer timer(ctx);
    if (e == hipSuccess) e = hipMemsetAsync(d_over, 0, 4, ctx->stream);
    if (e == hipSuccess) {
        timer.start(ctx->stream);
        with_flag(ctx->full_sh, [&](auto SH) {
            with_int<kStorageShQ8, kStorageShFp16, kStorageFp32>(ctx->cloud_storage, [&](auto ST) {
                if constexpr (ST.value == kStorageShQ8 && !SH.value) return;      // (no such store: prepare_cloud_buffers)
                else launch(SH, ST);
            });
        });
        e = hipGetLastError();
        timer.stop(ctx->stream);
    }
    if (e == hipSuccess && counted) e = hipMemcpyAsync(&n_over, d_over, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, MSPLAT_ERR_HIP, "GPU ingest failed: %s", hipGetErrorString(e));
    timer.read(ctx);
    return n_over ? f_rest_failure(ctx, who, ctx->cloud_storage, n_over, "", "") : MSPLAT_OK;
}
}  // extern "C++"

// what both vertex routes check of a layout; full: every f_rest property is there and the caller wants it
static int check_ply_layout(msplat_ctx* ctx, const msplat_ply_layout* layout, int full_sh, bool& full)
{
    const uint32_t vs = layout->vertex_size;
    if (vs == 0 || vs % 4 != 0 || vs > 1024)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "vertex size %u must be a multiple of 4 in (0, 1024]", vs);
    const int32_t* offs = &layout->x;
    constexpr int kProps = 3 + 3 + 45 + 1 + 3 + 4;     // x y z, f_dc, f_rest, opacity, scale, rot
    static_assert(sizeof(msplat_ply_layout) == 4 + 4 * kProps, "msplat_ply_layout must be packed int32s");
    for (int k = 0; k < kProps; ++k)
        if (offs[k] >= 0 && ((uint32_t)offs[k] + 4u > vs || offs[k] % 4 != 0))
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "property offset %d outside / misaligned in a %u-byte vertex", offs[k], vs);
    bool has_rest = true;
    for (int k = 0; k < 45; ++k) has_rest = has_rest && layout->f_rest[k] >= 0;
    full = full_sh != 0 && has_rest;      // f_rest is optional (gaussiancloud.cpp:188-205)
    return MSPLAT_OK;
}

// ingest_kernel over a vertex block that is on the device (d_raw: 16-byte aligned), into the prepared store
static int ingest_vertices(msplat_ctx* ctx, const char* who, const void* d_raw, uint64_t n, const msplat_ply_layout* layout,
                           uint32_t* d_over, hipError_t staged)
{
    const int grid = (int)div_up(n, 64);
    const size_t lds = (size_t)64 * layout->vertex_size + 16;
    PlyLayout kl;
    static_assert(sizeof(PlyLayout) == sizeof(msplat_ply_layout), "layout mirror out of sync");
    std::memcpy(&kl, layout, sizeof(kl));
    return run_ingest(ctx, who, d_over, staged, [&](auto SH, auto ST) {
        hipLaunchKernelGGL((ingest_kernel<SH.value, ST.value>), dim3(grid), dim3(64), lds, ctx->stream, (const char*)d_raw, n, kl,
                           (float4*)ctx->pos4.p, (float4*)ctx->recs.p, d_over);
    });
}

// GaussianCloud::ImportPly's per-vertex math (gaussiancloud.cpp:254-361) as a HIP kernel over the raw PLY vertex block.
// `vertices` is host memory (n * layout->vertex_size bytes).
int msplat_upload_ply_vertices(msplat_ctx* ctx, const void* vertices, uint64_t n, const msplat_ply_layout* layout,
                               int full_sh)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if ((!vertices && n) || !layout) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_upload_ply_vertices: NULL argument");
    bool full = false;
    int rc = check_ply_layout(ctx, layout, full_sh, full);
    if (rc) return rc;
    const uint32_t vs = layout->vertex_size;
    ctx->point_mode = false;
    if ((rc = prepare_cloud_buffers(ctx, n, full, nullptr))) return rc;
    if (n) {
        Buf raw;
        if ((rc = buf_alloc(ctx, raw, (size_t)n * vs + 16))) return rc;
        uint32_t* d_over = reinterpret_cast<uint32_t*>((char*)raw.p + (size_t)n * vs);      // (vs is a multiple of 4)
        rc = ingest_vertices(ctx, "msplat_upload_ply_vertices", raw.p, n, layout, d_over,
                             hipMemcpyAsync(raw.p, vertices, (size_t)n * vs, hipMemcpyHostToDevice, ctx->stream));
        buf_free(ctx, raw);
        if (rc) return rc;
    }
    if ((rc = spatial_reorder(ctx))) return rc;
    ctx->has_cloud = true;
    return MSPLAT_OK;
}

// ---- uploads from device memory: msplat_upload_cloud / _ply_vertices / msplat_cloud_from_attributes with the source on the
// context's device.  Every refusal comes before anything is launched or copied, and the pointer query is the first HIP call of
// each route: a host address that reached a kernel would fault the GPU.
// `p` .. p + bytes - 1 must be device memory of the context's device as hipPointerGetAttributes reports it (both ends are
// asked), inside one allocation where the runtime can name its range.  A failed query leaves a sticky error: cleared.
static int check_device_source(msplat_ctx* ctx, const char* who, const char* what, const void* p, uint64_t bytes)
{
    const char* ends[2] = {static_cast<const char*>(p), static_cast<const char*>(p) + (bytes - 1)};
    for (const char* q : ends) {
        hipPointerAttribute_t at;
        std::memset(&at, 0, sizeof(at));
        const hipError_t e = hipPointerGetAttributes(&at, q);
        if (e != hipSuccess) (void)hipGetLastError();
        if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->device)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s (%p, %llu bytes) is not device memory of device %d", who, what, p,
                        (unsigned long long)bytes, ctx->device);
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return MSPLAT_OK;
    }
    if (ends[1] >= static_cast<const char*>(base) + size)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s (%p, %llu bytes) runs past the end of its allocation", who, what, p,
                    (unsigned long long)bytes);
    return MSPLAT_OK;
}

// the 4-byte counter of run_ingest for the routes that stage nothing (kept: a re-upload allocates nothing)
static int ingest_counter(msplat_ctx* ctx, uint32_t*& d_over)
{
    int rc = buf_alloc(ctx, ctx->upload_over, 16);
    d_over = words(ctx->upload_over);
    return rc;
}

// msplat_upload_cloud with the records in device memory: repack_kernel instead of the host loop, the same context afterwards
int msplat_upload_cloud_device(msplat_ctx* ctx, const void* d_aos, uint64_t n, uint32_t stride_bytes,
                               const msplat_attr_offsets* off, int full_sh)
{
    static const char* who = "msplat_upload_cloud_device";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if ((!d_aos && n) || !off) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (reinterpret_cast<uintptr_t>(d_aos) % 16 != 0) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: d_aos must be 16-byte aligned", who);
    if (stride_bytes % 4 != 0) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "stride must be a multiple of 4");
    if (stride_bytes > 1024) return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: stride %u > 1024 bytes", who, stride_bytes);
    int rc = check_splat_count(ctx, n);
    if (rc) return rc;
    AttrOffsets ko;
    static_assert(sizeof(AttrOffsets) == sizeof(msplat_attr_offsets), "offsets mirror out of sync");
    std::memcpy(&ko, off, sizeof(ko));
    const uint32_t* o = &ko.pos_with_alpha;
    for (int k = 0; k < (full_sh ? 16 : 7); ++k)
        if ((uint64_t)o[k] + (k < 4 || k >= 7 ? 16u : 12u) > stride_bytes)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "attribute offset %u beyond stride %u", o[k], stride_bytes);
    if (n && (rc = check_device_source(ctx, who, "d_aos", d_aos, n * stride_bytes))) return rc;
    ctx->point_mode = false;
    if ((rc = prepare_cloud_buffers(ctx, n, full_sh != 0, nullptr))) return rc;
    if (n) {
        uint32_t* d_over = nullptr;
        if ((rc = ingest_counter(ctx, d_over))) return rc;
        const int grid = (int)div_up(n, 64);
        const size_t lds = (size_t)64 * stride_bytes;      // <= 64 KB
        rc = run_ingest(ctx, who, d_over, hipSuccess, [&](auto SH, auto ST) {
            hipLaunchKernelGGL((repack_kernel<SH.value, ST.value>), dim3(grid), dim3(64), lds, ctx->stream, (const char*)d_aos, n,
                               stride_bytes, ko, (float4*)ctx->pos4.p, (float4*)ctx->recs.p, d_over);
        });
        if (rc) return rc;
    }
    if ((rc = spatial_reorder(ctx))) return rc;
    ctx->has_cloud = true;
    return MSPLAT_OK;
}

// msplat_upload_ply_vertices with the vertex block in device memory: the same ingest_kernel launch, no staging copy
int msplat_upload_ply_vertices_device(msplat_ctx* ctx, const void* d_vertices, uint64_t n, const msplat_ply_layout* layout,
                                      int full_sh)
{
    static const char* who = "msplat_upload_ply_vertices_device";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if ((!d_vertices && n) || !layout) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (reinterpret_cast<uintptr_t>(d_vertices) % 16 != 0)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: d_vertices must be 16-byte aligned", who);
    bool full = false;
    int rc = check_ply_layout(ctx, layout, full_sh, full);
    if (rc) return rc;
    if ((rc = check_splat_count(ctx, n))) return rc;
    if (n && (rc = check_device_source(ctx, who, "d_vertices", d_vertices, n * layout->vertex_size))) return rc;
    ctx->point_mode = false;
    if ((rc = prepare_cloud_buffers(ctx, n, full, nullptr))) return rc;
    if (n) {
        uint32_t* d_over = nullptr;
        if ((rc = ingest_counter(ctx, d_over))) return rc;
        if ((rc = ingest_vertices(ctx, who, d_vertices, n, layout, d_over, hipSuccess))) return rc;
    }
    if ((rc = spatial_reorder(ctx))) return rc;
    ctx->has_cloud = true;
    return MSPLAT_OK;
}

// msplat_cloud_from_attributes + msplat_upload_gaussian_cloud with the six arrays in device memory: ingest_attributes_kernel,
// the vertex routes' math (one device function) on the same values
int msplat_upload_attributes_device(msplat_ctx* ctx, uint64_t n, const float* d_xyz, const float* d_f_dc, const float* d_f_rest,
                                    const float* d_opacity, const float* d_log_scale, const float* d_rot, int full_sh)
{
    static const char* who = "msplat_upload_attributes_device";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    const bool full = full_sh != 0 && d_f_rest != nullptr;      // f_rest is optional, as in msplat_cloud_from_attributes
    struct { const char* name; const float* p; uint32_t floats; } src[6] = {
        {"d_xyz", d_xyz, 3}, {"d_f_dc", d_f_dc, 3}, {"d_f_rest", full ? d_f_rest : nullptr, 45},
        {"d_opacity", d_opacity, 1}, {"d_log_scale", d_log_scale, 3}, {"d_rot", d_rot, 4}};
    for (int k = 0; k < 6; ++k) {
        if (k == 2 && !full) continue;
        if (!src[k].p && n) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s is NULL", who, src[k].name);
        if (reinterpret_cast<uintptr_t>(src[k].p) % 4 != 0)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s must be 4-byte aligned", who, src[k].name);
    }
    int rc = check_splat_count(ctx, n);
    if (rc) return rc;
    for (int k = 0; k < 6 && n; ++k)
        if (src[k].p && (rc = check_device_source(ctx, who, src[k].name, src[k].p, n * src[k].floats * 4))) return rc;
    ctx->point_mode = false;
    if ((rc = prepare_cloud_buffers(ctx, n, full, nullptr))) return rc;
    if (n) {
        uint32_t* d_over = nullptr;
        if ((rc = ingest_counter(ctx, d_over))) return rc;
        const AttrArrays arr{d_xyz, d_f_dc, full ? d_f_rest : nullptr, d_opacity, d_log_scale, d_rot};
        const int grid = (int)div_up(n, 64);
        rc = run_ingest(ctx, who, d_over, hipSuccess, [&](auto SH, auto ST) {
            hipLaunchKernelGGL((ingest_attributes_kernel<SH.value, ST.value>), dim3(grid), dim3(64), 0, ctx->stream, arr, n,
                               (float4*)ctx->pos4.p, (float4*)ctx->recs.p, d_over);
        });
        if (rc) return rc;
    }
    if ((rc = spatial_reorder(ctx))) return rc;
    ctx->has_cloud = true;
    return MSPLAT_OK;
}

// ---- point clouds (SURVEY 8f-4) ------------------------------------------------------------------------
static int build_sprite(msplat_ctx* ctx, const uint8_t* rgba8, uint32_t w, uint32_t h)
{
    // level 0 exactly as the reference prepares the texture: rows flipped so that t = 0 is the image's bottom row
    // (core/image.cpp:108-111), colour pre-multiplied by alpha in 8 bits with truncation (image.cpp:144-157),
    // texels decoded sRGB -> linear when the texture is flagged sRGB (pointrenderer.cpp:60, core/texture.cpp:63-70)
    std::vector<uint8_t> builtin;
    if (!rgba8) {
        // built-in sprite: a shaded sphere, alpha 1 inside the disc with a one-texel soft rim
        w = h = 128;
        builtin.resize((size_t)w * h * 4);
        for (uint32_t j = 0; j < h; ++j)
            for (uint32_t i = 0; i < w; ++i) {
                const float x = ((float)i + 0.5f) / (0.5f * w) - 1.0f, y = ((float)j + 0.5f) / (0.5f * h) - 1.0f;
                const float d = std::sqrt(x * x + y * y);
                const float a = std::min(1.0f, std::max(0.0f, (1.0f - d) * (0.5f * w)));
                const float shade = 0.35f + 0.65f * std::sqrt(std::max(0.0f, 1.0f - d * d));
                uint8_t* o = &builtin[((size_t)j * w + i) * 4];
                o[0] = o[1] = o[2] = (uint8_t)(shade * 255.0f + 0.5f);
                o[3] = (uint8_t)(a * 255.0f + 0.5f);
            }
        rgba8 = builtin.data();
    }
    if (w == 0 || h == 0 || w > 8192 || h > 8192) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "sprite size %ux%u outside [1,8192]^2", w, h);
    SpriteParams sp{};
    sp.w = (int)w;
    sp.h = (int)h;
    std::vector<float> chain;
    chain.resize((size_t)w * h * 4);
    const bool srgb = ctx->cfg.srgb != 0;
    for (uint32_t j = 0; j < h; ++j)
        for (uint32_t i = 0; i < w; ++i) {
            const uint8_t* s = rgba8 + ((size_t)(h - 1 - j) * w + i) * 4;
            float* o = &chain[((size_t)j * w + i) * 4];
            const float alpha = (float)s[3] / 255.0f;
            for (int c = 0; c < 3; ++c) {
                const uint8_t pm = (uint8_t)((((float)s[c] / 255.0f) * alpha) * 255.0f);
                const float v = (float)pm / 255.0f;
                o[c] = srgb ? (v <= 0.04045f ? v / 12.92f : std::pow((v + 0.055f) / 1.055f, 2.4f)) : v;
            }
            o[3] = alpha;
        }
    // mip chain: 2x2 box filter down to 1x1, every level stored at 8 bits like the GL_RGBA8 / GL_SRGB8_ALPHA8 texture's own
    // levels (glGenerateMipmap, core/texture.cpp:76)
    int lw = (int)w, lh = (int)h, level = 0;
    size_t off = 0;
    sp.off[0] = 0;
    while ((lw > 1 || lh > 1) && level + 1 < 14) {
        const int nw = std::max(lw / 2, 1), nh = std::max(lh / 2, 1);
        const size_t noff = off + (size_t)lw * lh;
        chain.resize((noff + (size_t)nw * nh) * 4);
        for (int j = 0; j < nh; ++j)
            for (int i = 0; i < nw; ++i) {
                const int i0 = std::min(2 * i, lw - 1), i1 = std::min(2 * i + 1, lw - 1);
                const int j0 = std::min(2 * j, lh - 1), j1 = std::min(2 * j + 1, lh - 1);
                for (int c = 0; c < 4; ++c) {
                    const float a = chain[(off + (size_t)j0 * lw + i0) * 4 + c], b = chain[(off + (size_t)j0 * lw + i1) * 4 + c];
                    const float cc = chain[(off + (size_t)j1 * lw + i0) * 4 + c], d = chain[(off + (size_t)j1 * lw + i1) * 4 + c];
                    float m = (((a + b) + cc) + d) * 0.25f;
                    // a derived level has the base level's 8-bit format (GL 4.6 8.14.4; sRGB-encoded colour for GL_SRGB8_ALPHA8):
                    // filtered on decoded values, stored rounded to 8 bits, decoded again for sampling
                    if (srgb && c < 3) {
                        const float e = m <= 0.0031308f ? m * 12.92f : 1.055f * std::pow(m, 1.0f / 2.4f) - 0.055f;
                        const float q = std::floor(e * 255.0f + 0.5f) / 255.0f;
                        m = q <= 0.04045f ? q / 12.92f : std::pow((q + 0.055f) / 1.055f, 2.4f);
                    } else {
                        m = std::floor(m * 255.0f + 0.5f) / 255.0f;
                    }
                    chain[(noff + (size_t)j * nw + i) * 4 + c] = m;
                }
            }
        off = noff;
        lw = nw;
        lh = nh;
        sp.off[++level] = (uint32_t)off;
    }
    sp.levels = level + 1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int rc = buf_alloc(ctx, ctx->sprite, chain.size() * sizeof(float));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->sprite.p, chain.data(), chain.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->sprite_params = sp;
    return MSPLAT_OK;
}

int msplat_set_point_sprite(msplat_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    return build_sprite(ctx, rgba8, width, height);
}

int msplat_upload_points(msplat_ctx* ctx, const void* aos, uint64_t n, uint32_t stride_bytes,
                         uint32_t position_offset, uint32_t color_offset)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!aos && n) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_upload_points: NULL argument");
    if (stride_bytes % 4 != 0 || position_offset + 16u > stride_bytes || color_offset + 16u > stride_bytes)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_upload_points: bad stride / offsets (%u, %u, %u)", stride_bytes,
                    position_offset, color_offset);
    if (ctx->rop != MSPLAT_ROP_NONE)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_upload_points: render-target emulation is set on this context and the "
                    "sprite compositor has none (msplat_set_target_emulation(ctx, MSPLAT_ROP_NONE) first)");
    if (ctx->target_mode != MSPLAT_TARGET_CLEAR)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_upload_points: a target mode is set on this context and the sprite compositor "
                    "overwrites its target (msplat_set_target_mode(ctx, MSPLAT_TARGET_CLEAR) first)");
    ctx->point_mode = true;
    int rc = prepare_cloud_buffers(ctx, n, false, nullptr);
    if (rc) { ctx->point_mode = false; return rc; }
    std::vector<float> pos, col;
    try {      // the C ABI never throws
        pos.resize((size_t)std::max<uint64_t>(n, 1) * 4);
        col.resize((size_t)std::max<uint64_t>(n, 1) * 4);
    } catch (const std::exception&) {
        return fail(ctx, MSPLAT_ERR_HIP, "msplat_upload_points: out of host memory for %llu points", (unsigned long long)n);
    }
    const uint8_t* src = static_cast<const uint8_t*>(aos);
    for (uint64_t i = 0; i < n; ++i) {
        std::memcpy(&pos[i * 4], src + i * stride_bytes + position_offset, 12);      // vec4(pos.xyz, pos[3]) -> w unused by the cull
        pos[i * 4 + 3] = 0.0f;                                                        // .w = footprint bound slot (none for points)
        std::memcpy(&col[i * 4], src + i * stride_bytes + color_offset, 16);
    }
    if (n) {
        HIP_TRY(ctx, hipMemcpy(ctx->pos4.p, pos.data(), n * 16, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->recs.p, col.data(), n * 16, hipMemcpyHostToDevice));
    }
    ctx->has_cloud = true;
    return MSPLAT_OK;
}

// device cloud -> reference AoS layout (100 B / 244 B records, gaussiancloud.cpp:32-56); parity tests
int msplat_download_cloud(msplat_ctx* ctx, void* aos_out, uint64_t cap_bytes)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!ctx->has_cloud) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "no cloud uploaded");
    if (ctx->point_mode) return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_download_cloud: the context holds a point cloud");
    const int F4 = ctx->store->F4;
    const bool sh16 = ctx->cloud_storage == kStorageShFp16, sh8 = ctx->cloud_storage == kStorageShQ8;      // widened back to fp32
    const size_t rec_floats = ctx->full_sh ? 61 : 25;
    if (cap_bytes < ctx->N * rec_floats * 4) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "output buffer too small");
    if (ctx->N == 0) return MSPLAT_OK;
    if (!aos_out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "aos_out is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t chunk = 1u << 18;
    std::vector<float> stage;
    try {
        stage.resize(chunk * F4 * 4);
    } catch (const std::exception&) {
        return fail(ctx, MSPLAT_ERR_HIP, "msplat_download_cloud: out of host memory");
    }
    float* dst = static_cast<float*>(aos_out);
    const bool ro = ctx->store && ctx->store->reordered;       // stored slot j = upload index order_host[j]
    for (uint64_t base = 0; base < ctx->N; base += chunk) {
        const size_t cnt = (size_t)std::min<uint64_t>(chunk, ctx->N - base);
        HIP_TRY(ctx, hipMemcpy(stage.data(), (const char*)ctx->recs.p + base * F4 * 16, cnt * F4 * 16, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < cnt; ++j) {
            const float* r = stage.data() + j * F4 * 4;
            float full[64];
            if (sh16 || sh8) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(r);
                if (sh8) sh8_unpack<true>(w, full);
                else if (ctx->full_sh) sh16_unpack<true>(w, full); else sh16_unpack<false>(w, full);
                r = full;
            }
            std::memcpy(dst + (ro ? (size_t)ctx->store->order_host[base + j] : base + j) * rec_floats, r, rec_floats * 4);
        }
    }
    return MSPLAT_OK;
}


// Storage of the higher-order SH (f_rest) for the context's NEXT splat upload (MSPLAT_STORAGE_*; see msplat_common.hip.h for the
// SH_FP16 and SH_Q8 records).  A cloud already on the device keeps its storage; an SH_Q8 upload without full SH stores FP32.
int msplat_set_cloud_storage(msplat_ctx* ctx, int32_t storage)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (storage != MSPLAT_STORAGE_FP32 && storage != MSPLAT_STORAGE_SH_FP16 && storage != MSPLAT_STORAGE_SH_Q8)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_set_cloud_storage: storage must be MSPLAT_STORAGE_FP32, _SH_FP16 or _SH_Q8 "
                    "(got %d)", storage);
    ctx->storage_cfg = storage;
    return MSPLAT_OK;
}

int msplat_get_cloud_storage(const msplat_ctx* ctx)
{
    if (!ctx || !ctx->has_cloud) return -1;
    return ctx->point_mode ? MSPLAT_STORAGE_FP32 : ctx->cloud_storage;
}

// the SH_Q8 quantiser on one reference record (msplat_debug.h): the pack / unpack pair of the uploads and the download, no device
int msplat_debug_sh_q8_round(const float rec_in[61], float rec_out[61], float steps_out[3], int8_t codes_out[45])
{
    if (!rec_in || !rec_out || !steps_out || !codes_out) return MSPLAT_ERR_INVALID_ARG;
    float full[64] = {}, back[64] = {};
    uint32_t w[32];
    std::memcpy(full, rec_in, 61 * 4);
    const uint32_t bad = sh8_pack<true>(full, w);
    sh8_unpack<true>(w, back);
    std::memcpy(rec_out, back, 61 * 4);
    std::memcpy(steps_out, w + 16, 12);
    for (int h = 0; h < 45; ++h) codes_out[h] = (int8_t)((w[19 + h / 4] >> (8 * (h & 3))) & 0xFFu);
    return (int)bad;
}
