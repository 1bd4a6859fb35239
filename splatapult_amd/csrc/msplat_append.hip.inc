// msplat_append.hip.inc -- msplat_append_cloud: the selected splats of a source context's cloud appended, on the device, to the
// context's own; kernels in msplat_append.hip.h, the scan in msplat_compact.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_transform.hip.inc)
//
// The compaction's and the transform's shape: an upload whose source is two stores.  Flags, count, offsets and index rank the
// selected source splats, the host reads K (and refuses N + K > 2^24 with nothing allocated), the context's own rows and the selected
// source rows go into a FRESH store of N + K rows in upload order, the host reads the pack routines' counter, and from there on the
// path is an upload's: prepare_cloud_buffers adopting that store, spatial_reorder, has_cloud.  Until the swap the context renders what
// it rendered before, so every failure up to there leaves it alone.  The old numbering is a prefix of the new one: the mask is
// carried across prepare_cloud_buffers, K visible bytes longer, and the visibility plane marked stale.

int msplat_append_cloud(msplat_ctx* ctx, msplat_ctx* src, const uint8_t* d_select, uint64_t n, uint32_t* d_index_map, uint64_t* n_added_out)
{
    static const char* who = "msplat_append_cloud";
    drain_async(ctx);
    if (src != ctx) drain_async(src);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!src) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: src is NULL", who);
    if (src->device != ctx->device)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: contexts are on different devices (%d, %d)", who, ctx->device, src->device);
    if ((ctx->has_cloud && ctx->point_mode) || (src->has_cloud && src->point_mode))
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %s holds a point cloud (the call is for splat clouds)", who,
                    ctx->has_cloud && ctx->point_mode ? "the context" : "src");
    if (!ctx->has_cloud || !ctx->store) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "%s: no cloud uploaded", who);
    if (!src->has_cloud || !src->store) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "%s: src has no cloud uploaded", who);
    if (src->full_sh != ctx->full_sh)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: src holds %s and the context %s (SH degree conversion is out of scope)", who,
                    src->full_sh ? "full SH" : "degree-1 SH", ctx->full_sh ? "full SH" : "degree-1 SH");
    const uint64_t N = ctx->N, Ns = src->N;
    if (n != Ns)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: n = %llu for a source of %llu splats", who, (unsigned long long)n, (unsigned long long)Ns);
    int rc;
    if (d_select && Ns && (rc = check_device_source(ctx, who, "d_select", d_select, Ns))) return rc;
    if (d_index_map) {
        if ((uintptr_t)d_index_map % 4 != 0)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: d_index_map (%p) is not 4-byte aligned", who, (const void*)d_index_map);
        if (Ns && (rc = check_device_source(ctx, who, "d_index_map", d_index_map, Ns * 4))) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (src != ctx) HIP_TRY(ctx, hipStreamSynchronize(src->stream));
    if ((rc = ensure_order_dev(ctx))) return rc;
    if (src != ctx && (rc = ensure_order_dev(src))) return fail(ctx, rc, "%s: %s", who, src->err.c_str());
    // (both stores stay alive to the end: the source's through the caller's context, the own one to the swap)
    const CloudStore* old = ctx->store.get();
    const CloudStore* from = src->store.get();
    const int F4 = old->F4, storage = old->storage, sF4 = from->F4, sstorage = from->storage;
    const bool full_sh = ctx->full_sh;
    hipStream_t s = ctx->stream;

    // the scratch of one call: flags padded to whole chunks | chunk counts | K | the ranks
    const uint32_t ns = (uint32_t)Ns, nchunks = div_up(Ns, kCompactChunk);
    const size_t flag_bytes = (size_t)nchunks * kCompactChunk, count_off = flag_bytes, total_off = count_off + (size_t)nchunks * 4;
    const size_t rank_off = (total_off + 4 + 15) & ~(size_t)15;
    Buf tmp, nmask;
    uint32_t K = 0;
    const uint32_t* rank = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    const bool timed = ctx->cfg.enable_timing > 0 && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    ctx->upload_kernel_ms = -1.0f;
    auto done = [&](int code) {
        for (hipEvent_t v : ev)
            if (v) (void)hipEventDestroy(v);
        ev[0] = ev[1] = nullptr;
        buf_free(ctx, tmp);
        return code;
    };
    if (Ns) {
        if ((rc = buf_alloc(ctx, tmp, rank_off + (size_t)Ns * 4))) return done(rc);
        uint8_t* flags = (uint8_t*)tmp.p;
        uint32_t* counts = (uint32_t*)((char*)tmp.p + count_off);
        uint32_t* total = (uint32_t*)((char*)tmp.p + total_off);
        uint32_t* rank_out = (uint32_t*)((char*)tmp.p + rank_off);
        rank = rank_out;
        const int gchunks = grid_for(nchunks, ctx->grid_cap);
        hipLaunchKernelGGL(append_flags_kernel, dim3(gchunks), dim3(kThreads), 0, s, d_select, ns, nchunks, flags);
        hipLaunchKernelGGL(compact_count_kernel, dim3(gchunks), dim3(kThreads), 0, s, (const uint8_t*)flags, nchunks, counts);
        hipLaunchKernelGGL(compact_offsets_kernel, dim3(1), dim3(kThreads), 0, s, counts, nchunks, total);
        hipLaunchKernelGGL(compact_index_kernel, dim3(gchunks), dim3(kThreads), 0, s, (const uint8_t*)flags, (const uint32_t*)counts, ns,
                           nchunks, rank_out);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&K, total, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return done(fail(ctx, MSPLAT_ERR_HIP, "%s: numbering the selected splats failed: %s", who, hipGetErrorString(e)));
    }
    const uint64_t total_n = N + K;
    if (total_n > (1ull << 24))       // (check_splat_count's limit, before anything is allocated or the caller's map written)
        return done(fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %llu + %u splats > 2^24 (rank field is 24 bit); the cloud is unchanged", who,
                         (unsigned long long)N, K));

    // the new store, never an old allocation: until the swap below the context renders what it rendered before
    const size_t alloc_n = std::max<uint64_t>(total_n, 1), need_pos = alloc_n * 16, need_rec = alloc_n * F4 * 16;
    const bool had_mask = ctx->has_mask;
    void *npos = nullptr, *nrec = nullptr, *d_over = nullptr;
    uint32_t n_over = 0;
    hipError_t e = hipMalloc(&npos, need_pos);
    if (e == hipSuccess) e = hipMalloc(&nrec, need_rec);
    if (e == hipSuccess) e = hipMalloc(&d_over, 16);
    if (e == hipSuccess) e = hipMemsetAsync(d_over, 0, 4, s);
    if (e == hipSuccess && had_mask) {      // the mask of the merged cloud: the old bytes, then K visible ones
        if (buf_alloc(ctx, nmask, alloc_n)) e = hipErrorOutOfMemory;
        if (e == hipSuccess && N) e = hipMemcpyAsync(nmask.p, ctx->vis_mask.p, N, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess && K) e = hipMemsetAsync((char*)nmask.p + N, 1, K, s);
    }
    if (e == hipSuccess) {
        if (timed) (void)hipEventRecord(ev[0], s);
        if (N)      // the context's own rows, storage order -> upload order
            hipLaunchKernelGGL(append_gather_kernel, dim3(grid_for(div_up(N * (uint64_t)F4, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s,
                               (const uint32_t*)nullptr, old->reordered ? (const uint32_t*)old->order_dev.p : nullptr, (uint32_t)N, 0u, F4,
                               (const float4*)old->pos4.p, (const float4*)old->recs.p, (float4*)npos, (float4*)nrec);
        const uint32_t* sorder = from->reordered ? (const uint32_t*)from->order_dev.p : nullptr;
        if (K && sstorage == storage) {
            hipLaunchKernelGGL(append_gather_kernel, dim3(grid_for(div_up(Ns * (uint64_t)sF4, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s,
                               rank, sorder, ns, (uint32_t)N, sF4, (const float4*)from->pos4.p, (const float4*)from->recs.p, (float4*)npos,
                               (float4*)nrec);
        } else if (K) {
            AppendConvertArgs a;
            a.pos_in = (const float4*)from->pos4.p;
            a.recs_in = (const float4*)from->recs.p;
            a.order = sorder;
            a.rank = rank;
            a.pos_out = (float4*)npos;
            a.recs_out = (float4*)nrec;
            a.n_over = (uint32_t*)d_over;
            a.n = ns;
            a.base = (uint32_t)N;
            const int grid = grid_for(div_up(Ns, 64), ctx->grid_cap);
            // the pairs of kinds that differ; a Q8 store without full SH does not exist (prepare_cloud_buffers)
            with_flag(full_sh, [&](auto SH) {
                with_int<kStorageShQ8, kStorageShFp16, kStorageFp32>(sstorage, [&](auto SS) {
                    with_int<kStorageShQ8, kStorageShFp16, kStorageFp32>(storage, [&](auto DS) {
                        if constexpr (SS.value == DS.value || ((SS.value == kStorageShQ8 || DS.value == kStorageShQ8) && !SH.value)) return;
                        else hipLaunchKernelGGL((append_convert_kernel<SH.value, SS.value, DS.value>), dim3(grid), dim3(64), 0, s, a);
                    });
                });
            });
        }
        e = hipGetLastError();
        if (timed) (void)hipEventRecord(ev[1], s);
        if (e == hipSuccess) e = hipMemcpyAsync(&n_over, d_over, 4, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    // (the gathers and the conversion between two stream events: msplat_debug_upload_kernel_ms)
    if (e == hipSuccess && total_n && timed && hipEventElapsedTime(&ctx->upload_kernel_ms, ev[0], ev[1]) != hipSuccess) ctx->upload_kernel_ms = -1.0f;
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
        buf_free(ctx, nmask);
        done(MSPLAT_OK);
        if (e != hipSuccess)
            return fail(ctx, MSPLAT_ERR_HIP, "%s: the store of the merged cloud could not be made: %s", who, hipGetErrorString(e));
        if (storage == kStorageShQ8)
            return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %u appended f_rest values are not finite: MSPLAT_STORAGE_SH_Q8 cannot quantise "
                        "them; the cloud is unchanged", who, n_over);
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %u appended f_rest values are beyond the fp16 range (|c| >= 65520) of "
                    "MSPLAT_STORAGE_SH_FP16; the cloud is unchanged", who, n_over);
    }
    // the caller's map last of all that is launched: a call that fails has written nothing of the caller's
    if (d_index_map && Ns) {
        hipLaunchKernelGGL(append_map_kernel, dim3(grid_for(div_up(Ns, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s, rank, ns, (uint32_t)N,
                           d_index_map);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(npos); (void)hipFree(nrec);
            buf_free(ctx, nmask);
            return done(fail(ctx, MSPLAT_ERR_HIP, "%s: writing the index map failed: %s", who, hipGetErrorString(e)));
        }
    }
    done(MSPLAT_OK);
    st->device = ctx->device;
    st->pos4.p = npos; st->pos4.bytes = need_pos;
    st->recs.p = nrec; st->recs.bytes = need_rec;
    st->storage = storage;
    st->F4 = F4;
    // from here on an upload of N + K splats whose records are in place -- but for the mask: prepare_cloud_buffers frees the old one
    // (the stream is idle), the extended one takes its place
    const OverlayKept ov = overlay_take(ctx);      // (the overlay's classes stay as well; overlay_restore extends them by K bytes of class 0)
    rc = prepare_cloud_buffers(ctx, total_n, full_sh, st);
    ctx->ov_cls = ov.cls;
    if (ctx->store == st) ctx->device_bytes += need_pos + need_rec;
    if (rc) {
        buf_free(ctx, nmask);
        return rc;
    }
    if (had_mask) {      // (a member of the context since the mask was set: msplat_destroy knows it)
        ctx->vis_mask.p = nmask.p;
        ctx->vis_mask.bytes = nmask.bytes;
    }
    if ((rc = spatial_reorder(ctx))) return rc;
    if (had_mask) {         // the plane, the boxes and the new store's order on the device, as set_mask leaves them
        if ((rc = vis_alloc(ctx)) || (rc = ensure_order_dev(ctx))) return rc;
        ctx->has_mask = true;
        ctx->vis_dirty = true;
    }
    if ((rc = overlay_restore(ctx, ov, N, K))) return rc;
    ctx->has_cloud = true;
    if (n_added_out) *n_added_out = K;
    return MSPLAT_OK;
}
