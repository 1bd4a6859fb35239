// msplat_append.hip.inc -- msplat_append_cloud: the selected splats of a source context's cloud appended, on the device, to the
// context's own; kernels in msplat_append.hip.h, the scan in msplat_compact.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_transform.hip.inc)
//
// The compaction's and the transform's shape: an upload whose source is two stores.  The selection scan (msplat_edit.hip.inc) behind
// append_flags_kernel ranks the selected source splats and gives the host K (N + K > 2^24 is refused with nothing allocated), the
// context's own rows and the selected source rows go into a FreshStore of N + K rows in upload order, the host reads the pack
// routines' counter, and fresh_adopt makes it the context's cloud; every failure up to there leaves the cloud alone.  The old
// numbering is a prefix of the new one: the mask and the overlay's classes stay (KeptPlanes), K visible bytes / K bytes of class 0
// longer, both built before the swap.

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
    if (d_index_map && (rc = check_device_array(ctx, who, "d_index_map", d_index_map, 4, Ns))) return rc;
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

    KernelTimer timer(ctx);
    SelectionScan sc(ctx);
    const uint32_t ns = (uint32_t)Ns;
    if (Ns) {
        if ((rc = scan_reserve(sc, Ns, nullptr))) return rc;
        hipLaunchKernelGGL(append_flags_kernel, dim3(grid_for(sc.nchunks, ctx->grid_cap)), dim3(kThreads), 0, s, d_select, ns, sc.nchunks, sc.flags);
        if ((rc = scan_number(sc, who, "selected", hipSuccess))) return rc;
    }
    const uint32_t K = sc.K;
    const uint32_t* rank = sc.rank;
    const uint64_t total_n = N + K;
    if (total_n > (1ull << 24))       // (check_splat_count's limit, before anything is allocated or the caller's map written)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %llu + %u splats > 2^24 (rank field is 24 bit); the cloud is unchanged", who,
                    (unsigned long long)N, K);

    FreshStore fs;
    KeptPlanes kept(ctx);
    uint32_t n_over = 0;
    hipError_t e = fresh_alloc(ctx, fs, total_n, F4, storage, true);
    if (e == hipSuccess) e = kept_grow(kept, N, K);
    if (e == hipSuccess) {
        float4 *npos = (float4*)fs.st->pos4.p, *nrec = (float4*)fs.st->recs.p;
        timer.start(s);
        if (N)      // the context's own rows, storage order -> upload order
            hipLaunchKernelGGL(append_gather_kernel, dim3(grid_for(div_up(N * (uint64_t)F4, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s,
                               (const uint32_t*)nullptr, old->reordered ? (const uint32_t*)old->order_dev.p : nullptr, (uint32_t)N, 0u, F4,
                               (const float4*)old->pos4.p, (const float4*)old->recs.p, npos, nrec);
        const uint32_t* sorder = from->reordered ? (const uint32_t*)from->order_dev.p : nullptr;
        if (K && sstorage == storage) {
            hipLaunchKernelGGL(append_gather_kernel, dim3(grid_for(div_up(Ns * (uint64_t)sF4, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s,
                               rank, sorder, ns, (uint32_t)N, sF4, (const float4*)from->pos4.p, (const float4*)from->recs.p, npos, nrec);
        } else if (K) {
            AppendConvertArgs a;
            a.pos_in = (const float4*)from->pos4.p;
            a.recs_in = (const float4*)from->recs.p;
            a.order = sorder;
            a.rank = rank;
            a.pos_out = npos;
            a.recs_out = nrec;
            a.n_over = fs.d_over;
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
        timer.stop(s);
        if (e == hipSuccess) e = hipMemcpyAsync(&n_over, fs.d_over, 4, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && total_n) timer.read(ctx);      // (the gathers and the conversion between two stream events: msplat_debug_upload_kernel_ms)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, MSPLAT_ERR_HIP, "%s: the store of the merged cloud could not be made: %s", who, hipGetErrorString(e));
    }
    if (n_over) return f_rest_failure(ctx, who, storage, n_over, "appended ", "; the cloud is unchanged");
    // the caller's map last of all that is launched: a call that fails has written nothing of the caller's
    if (d_index_map && Ns) {
        hipLaunchKernelGGL(append_map_kernel, dim3(grid_for(div_up(Ns, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s, rank, ns, (uint32_t)N,
                           d_index_map);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, MSPLAT_ERR_HIP, "%s: writing the index map failed: %s", who, hipGetErrorString(e));
        }
    }
    buf_free(ctx, sc.tmp);
    if ((rc = fresh_adopt(ctx, fs, total_n, full_sh, &kept))) return rc;
    if (n_added_out) *n_added_out = K;
    return MSPLAT_OK;
}
