// msplat_compact.hip.inc -- msplat_compact_cloud: the context's cloud reduced, on the device, to the splats its mask and crop let
// through; kernels in msplat_compact.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_visibility.hip.inc)
//
// The call is an upload whose source is the context's own store: flags, count, offsets and index give every splat its new upload
// index, the host reads K, the kept records are gathered into a FRESH store in the new upload order, and from there on the path is
// an upload's -- prepare_cloud_buffers for K splats, spatial_reorder, has_cloud.  The new store goes through prepare_cloud_buffers as
// a store to adopt (its `share` argument): that keeps the path from reusing the old allocation (never in place), takes the storage
// kind from the store and not from msplat_set_cloud_storage, and finds order / boxes empty as a fresh store has them.

int msplat_compact_cloud(msplat_ctx* ctx, uint32_t* d_index_map, uint64_t* n_kept_out)
{
    static const char* who = "msplat_compact_cloud";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (ctx->has_cloud && ctx->point_mode)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: the context holds a point cloud (visibility is for splat clouds)", who);
    if (!ctx->has_cloud || !ctx->store) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "%s: no cloud uploaded", who);
    const uint64_t N = ctx->N;
    int rc;
    if (d_index_map) {
        if ((uintptr_t)d_index_map % 4 != 0)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: d_index_map (%p) is not 4-byte aligned", who, (const void*)d_index_map);
        if (N && (rc = check_device_source(ctx, who, "d_index_map", d_index_map, N * 4))) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = ensure_order_dev(ctx))) return rc;
    const CloudStore* old = ctx->store.get();      // (no second owner here: prepare_cloud_buffers reads the use count)
    const int F4 = old->F4, storage = old->storage;
    const bool full_sh = ctx->full_sh;
    hipStream_t s = ctx->stream;

    // the scratch of one call: flags padded to whole chunks | chunk counts | K | the map, unless the caller's array takes it
    const uint32_t n = (uint32_t)N, nchunks = div_up(N, kCompactChunk);
    const size_t flag_bytes = (size_t)nchunks * kCompactChunk, count_off = flag_bytes, total_off = count_off + (size_t)nchunks * 4;
    const size_t map_off = (total_off + 4 + 15) & ~(size_t)15;
    Buf tmp;
    uint32_t K = 0;
    const uint32_t* map = d_index_map;
    hipEvent_t ev[2] = {nullptr, nullptr};
    const bool timed = ctx->cfg.enable_timing > 0 && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    ctx->upload_kernel_ms = -1.0f;
    auto done = [&](int code) {
        for (hipEvent_t v : ev)
            if (v) (void)hipEventDestroy(v);
        buf_free(ctx, tmp);
        return code;
    };
    if (N) {
        if ((rc = buf_alloc(ctx, tmp, map_off + (d_index_map ? 0 : (size_t)N * 4)))) return done(rc);
        uint8_t* flags = (uint8_t*)tmp.p;
        uint32_t* counts = (uint32_t*)((char*)tmp.p + count_off);
        uint32_t* total = (uint32_t*)((char*)tmp.p + total_off);
        uint32_t* map_out = d_index_map ? d_index_map : (uint32_t*)((char*)tmp.p + map_off);
        map = map_out;
        CompactFlagsArgs a;
        a.pos = (const float4*)old->pos4.p;
        a.mask = ctx->has_mask ? (const uint8_t*)ctx->vis_mask.p : nullptr;
        a.order = old->reordered ? (const uint32_t*)old->order_dev.p : nullptr;
        a.n = n;
        a.shape = ctx->crop_shape;
        std::memcpy(a.m, ctx->crop_mat, sizeof(a.m));
        a.flags = flags;
        hipError_t e = hipMemsetAsync(flags, 0, flag_bytes, s);      // (the padding of the last chunk counts as dropped)
        if (e == hipSuccess) {
            if (timed) (void)hipEventRecord(ev[0], s);
            const int gchunks = grid_for(nchunks, ctx->grid_cap);
            hipLaunchKernelGGL(compact_flags_kernel, dim3(grid_for(div_up(N, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s, a);
            hipLaunchKernelGGL(compact_count_kernel, dim3(gchunks), dim3(kThreads), 0, s, (const uint8_t*)flags, nchunks, counts);
            hipLaunchKernelGGL(compact_offsets_kernel, dim3(1), dim3(kThreads), 0, s, counts, nchunks, total);
            hipLaunchKernelGGL(compact_index_kernel, dim3(gchunks), dim3(kThreads), 0, s, (const uint8_t*)flags, (const uint32_t*)counts, n,
                               nchunks, map_out);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&K, total, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return done(fail(ctx, MSPLAT_ERR_HIP, "%s: numbering the kept splats failed: %s", who, hipGetErrorString(e)));
    }

    // the new store, never the old allocation: until the swap below the context renders what it rendered before
    const size_t alloc_k = std::max<uint32_t>(K, 1u), need_pos = alloc_k * 16, need_rec = alloc_k * F4 * 16;
    void *npos = nullptr, *nrec = nullptr;
    hipError_t e = hipMalloc(&npos, need_pos);
    if (e == hipSuccess) e = hipMalloc(&nrec, need_rec);
    if (e == hipSuccess && K) {
        hipLaunchKernelGGL(compact_gather_kernel, dim3(grid_for(div_up(N * (uint64_t)F4, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s, map,
                           old->reordered ? (const uint32_t*)old->order_dev.p : nullptr, n, F4, (const float4*)old->pos4.p,
                           (const float4*)old->recs.p, (float4*)npos, (float4*)nrec);
        e = hipGetLastError();
        if (timed) (void)hipEventRecord(ev[1], s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        // (flags, scan and gather between two stream events, the K readback and the allocation included: msplat_debug_upload_kernel_ms)
        if (e == hipSuccess && timed && hipEventElapsedTime(&ctx->upload_kernel_ms, ev[0], ev[1]) != hipSuccess) ctx->upload_kernel_ms = -1.0f;
    }
    std::shared_ptr<CloudStore> st;
    if (e == hipSuccess) {
        try {      // the C ABI never throws
            st = std::make_shared<CloudStore>();
        } catch (const std::exception&) {
            e = hipErrorOutOfMemory;
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (npos) (void)hipFree(npos);
        if (nrec) (void)hipFree(nrec);
        return done(fail(ctx, MSPLAT_ERR_HIP, "%s: the store of the %u kept splats could not be made: %s", who, K, hipGetErrorString(e)));
    }
    done(MSPLAT_OK);
    st->device = ctx->device;
    st->pos4.p = npos; st->pos4.bytes = need_pos;
    st->recs.p = nrec; st->recs.bytes = need_rec;
    st->storage = storage;
    st->F4 = F4;
    // from here on an upload of K splats whose records are in place.  The adopted store is the context's own: it counts
    rc = prepare_cloud_buffers(ctx, K, full_sh, st);
    if (ctx->store == st) ctx->device_bytes += need_pos + need_rec;
    if (rc) return rc;
    if ((rc = spatial_reorder(ctx))) return rc;
    ctx->has_cloud = true;
    if (n_kept_out) *n_kept_out = K;
    return MSPLAT_OK;
}
