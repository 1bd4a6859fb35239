// msplat_transform.hip.inc -- msplat_transform_cloud: the selected splats of the context's cloud moved, rotated and scaled by a
// matrix, on the device; kernel in msplat_transform.hip.h, the SH matrices: msplat_sh_rotation (host/gaussian_scene.cpp)
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_compact.hip.inc)
//
// The compaction's shape: an upload whose source is the context's own store.  One kernel writes every record -- transformed or
// copied -- into a FRESH store in upload order, the host reads the pack routines' counter, and from there on the path is an upload's:
// prepare_cloud_buffers adopting that store, spatial_reorder, has_cloud.  Until the swap the context renders what it rendered
// before, so every failure up to there leaves it alone.  Unlike an upload the numbering does not change: the mask is carried
// across prepare_cloud_buffers and the visibility plane marked stale.

int msplat_transform_cloud(msplat_ctx* ctx, const float M[16], const uint8_t* d_select, uint64_t n, int32_t flags)
{
    static const char* who = "msplat_transform_cloud";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!M) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: M is NULL", who);
    for (int k = 0; k < 16; ++k)
        if (k % 4 != 3 && !std::isfinite(M[k]))       // (row 3 is not read)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: M[%d] is not finite", who, k);
    if (flags & ~MSPLAT_TRANSFORM_KEEP_SH)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~MSPLAT_TRANSFORM_KEEP_SH));
    if (ctx->has_cloud && ctx->point_mode)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: the context holds a point cloud (the call is for splat clouds)", who);
    if (!ctx->has_cloud || !ctx->store) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "%s: no cloud uploaded", who);
    const uint64_t N = ctx->N;
    if (n != N)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: n = %llu for a cloud of %llu splats", who, (unsigned long long)n, (unsigned long long)N);
    int rc;
    if (d_select && N && (rc = check_device_source(ctx, who, "d_select", d_select, N))) return rc;
    TransformArgs a;
    std::memset(&a, 0, sizeof(a));
    a.keep_sh = (flags & MSPLAT_TRANSFORM_KEEP_SH) ? 1 : 0;
    if (!a.keep_sh && (rc = msplat_sh_rotation(M, a.d1, a.d2, a.d3, nullptr)))
        return fail(ctx, rc, "%s: M is not a rotation times a uniform positive scale, so the SH cannot follow it (MSPLAT_TRANSFORM_KEEP_SH "
                    "leaves them as they are)", who);
    for (int k = 0; k < 4; ++k)
        for (int r = 0; r < 3; ++r) a.m[3 * k + r] = M[4 * k + r];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = ensure_order_dev(ctx))) return rc;
    const CloudStore* old = ctx->store.get();      // (no second owner here: prepare_cloud_buffers reads the use count)
    const int F4 = old->F4, storage = old->storage;
    const bool full_sh = ctx->full_sh;
    hipStream_t s = ctx->stream;

    // the new store, never the old allocation: until the swap below the context renders what it rendered before
    const size_t alloc_n = std::max<uint64_t>(N, 1), need_pos = alloc_n * 16, need_rec = alloc_n * F4 * 16;
    void *npos = nullptr, *nrec = nullptr, *d_over = nullptr;
    uint32_t n_over = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    const bool timed = ctx->cfg.enable_timing > 0 && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    ctx->upload_kernel_ms = -1.0f;
    hipError_t e = hipMalloc(&npos, need_pos);
    if (e == hipSuccess) e = hipMalloc(&nrec, need_rec);
    if (e == hipSuccess) e = hipMalloc(&d_over, 16);
    if (e == hipSuccess) e = hipMemsetAsync(d_over, 0, 4, s);
    if (e == hipSuccess && N) {
        a.pos_in = (const float4*)old->pos4.p;
        a.recs_in = (const float4*)old->recs.p;
        a.order = old->reordered ? (const uint32_t*)old->order_dev.p : nullptr;
        a.select = d_select;
        a.pos_out = (float4*)npos;
        a.recs_out = (float4*)nrec;
        a.n_over = (uint32_t*)d_over;
        a.n = (uint32_t)N;
        if (timed) (void)hipEventRecord(ev[0], s);
        const int grid = grid_for(div_up(N, 64), ctx->grid_cap);
        with_flag(full_sh, [&](auto SH) {
            with_int<kStorageShQ8, kStorageShFp16, kStorageFp32>(storage, [&](auto ST) {
                if constexpr (ST.value == kStorageShQ8 && !SH.value) return;      // (no such store: prepare_cloud_buffers)
                else hipLaunchKernelGGL((transform_kernel<SH.value, ST.value>), dim3(grid), dim3(64), 0, s, a);
            });
        });
        e = hipGetLastError();
        if (timed) (void)hipEventRecord(ev[1], s);
        if (e == hipSuccess) e = hipMemcpyAsync(&n_over, d_over, 4, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    // (the one kernel between two stream events: msplat_debug_upload_kernel_ms)
    if (e == hipSuccess && N && timed && hipEventElapsedTime(&ctx->upload_kernel_ms, ev[0], ev[1]) != hipSuccess) ctx->upload_kernel_ms = -1.0f;
    for (hipEvent_t v : ev)
        if (v) (void)hipEventDestroy(v);
    if (d_over) (void)hipFree(d_over);
    std::shared_ptr<CloudStore> st;
    if (e == hipSuccess && !n_over) {
        try {      // the C ABI never throws
            st = std::make_shared<CloudStore>();
        } catch (const std::exception&) {
            e = hipErrorOutOfMemory;
        }
    }
    if (e != hipSuccess || n_over) {
        (void)hipGetLastError();
        if (npos) (void)hipFree(npos);
        if (nrec) (void)hipFree(nrec);
        if (e != hipSuccess)
            return fail(ctx, MSPLAT_ERR_HIP, "%s: the store of the transformed cloud could not be made: %s", who, hipGetErrorString(e));
        if (storage == kStorageShQ8)
            return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %u transformed f_rest values are not finite: MSPLAT_STORAGE_SH_Q8 cannot quantise "
                        "them; the cloud is unchanged", who, n_over);
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %u transformed f_rest values are beyond the fp16 range (|c| >= 65520) of "
                    "MSPLAT_STORAGE_SH_FP16; the cloud is unchanged", who, n_over);
    }
    st->device = ctx->device;
    st->pos4.p = npos; st->pos4.bytes = need_pos;
    st->recs.p = nrec; st->recs.bytes = need_rec;
    st->storage = storage;
    st->F4 = F4;
    // from here on an upload of N splats whose records are in place -- but for the mask: the numbering is the old one, so it stays
    // (prepare_cloud_buffers would free it: it is taken out of its hands and handed back)
    const bool had_mask = ctx->has_mask;
    const Buf mask = ctx->vis_mask;
    ctx->vis_mask = Buf{};
    const OverlayKept ov = overlay_take(ctx);      // (the overlay's classes likewise: a dragged selection stays tinted)
    rc = prepare_cloud_buffers(ctx, N, full_sh, st);
    ctx->vis_mask = mask;
    ctx->ov_cls = ov.cls;
    if (ctx->store == st) ctx->device_bytes += need_pos + need_rec;
    if (rc) return rc;
    if ((rc = spatial_reorder(ctx))) return rc;
    if (had_mask) {         // the plane, the boxes and the new store's order on the device, as set_mask leaves them
        if ((rc = vis_alloc(ctx)) || (rc = ensure_order_dev(ctx))) return rc;
        ctx->has_mask = true;
        ctx->vis_dirty = true;
    }
    if ((rc = overlay_restore(ctx, ov, N, 0))) return rc;
    ctx->has_cloud = true;
    return MSPLAT_OK;
}
