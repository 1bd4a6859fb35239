// msplat_compact.hip.inc -- msplat_compact_cloud: the context's cloud reduced, on the device, to the splats its mask and crop let
// through; kernels in msplat_compact.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_overlay.hip.inc)
//
// The call is an upload whose source is the context's own store: the selection scan (msplat_edit.hip.inc) behind compact_flags_kernel
// gives every splat its new upload index and the host K, the kept records are gathered into a FreshStore in the new upload order,
// and fresh_adopt makes it the context's cloud.  The numbering changes: no plane is kept, the mask and the classes go as at an upload.

int msplat_compact_cloud(msplat_ctx* ctx, uint32_t* d_index_map, uint64_t* n_kept_out)
{
    static const char* who = "msplat_compact_cloud";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    int rc;
    if ((rc = require_splat_cloud(ctx, who, "visibility is for splat clouds"))) return rc;
    const uint64_t N = ctx->N;
    if (d_index_map && (rc = check_device_array(ctx, who, "d_index_map", d_index_map, 4, N))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = ensure_order_dev(ctx))) return rc;
    const CloudStore* old = ctx->store.get();      // (no second owner here: prepare_cloud_buffers reads the use count)
    const int F4 = old->F4;
    const uint32_t* order = old->reordered ? (const uint32_t*)old->order_dev.p : nullptr;
    const bool full_sh = ctx->full_sh;
    hipStream_t s = ctx->stream;

    KernelTimer timer(ctx);
    SelectionScan sc(ctx);      // (the ranks are the map: in the caller's array where there is one)
    if (N) {
        if ((rc = scan_reserve(sc, N, d_index_map))) return rc;
        CompactFlagsArgs a;
        a.pos = (const float4*)old->pos4.p;
        a.mask = ctx->has_mask ? (const uint8_t*)ctx->vis_mask.p : nullptr;
        a.order = order;
        a.n = (uint32_t)N;
        a.shape = ctx->crop_shape;
        std::memcpy(a.m, ctx->crop_mat, sizeof(a.m));
        a.flags = sc.flags;
        const hipError_t e = hipMemsetAsync(sc.flags, 0, sc.flag_bytes, s);      // (the padding of the last chunk counts as dropped)
        if (e == hipSuccess) {
            timer.start(s);
            hipLaunchKernelGGL(compact_flags_kernel, dim3(grid_for(div_up(N, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s, a);
        }
        if ((rc = scan_number(sc, who, "kept", e))) return rc;
    }
    const uint32_t K = sc.K;

    FreshStore fs;
    hipError_t e = fresh_alloc(ctx, fs, K, F4, old->storage, false);
    if (e == hipSuccess && K) {
        hipLaunchKernelGGL(compact_gather_kernel, dim3(grid_for(div_up(N * (uint64_t)F4, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s,
                           (const uint32_t*)sc.rank, order, (uint32_t)N, F4, (const float4*)old->pos4.p, (const float4*)old->recs.p,
                           (float4*)fs.st->pos4.p, (float4*)fs.st->recs.p);
        e = hipGetLastError();
        timer.stop(s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        // (flags, scan and gather between two stream events, the K readback and the allocation included: msplat_debug_upload_kernel_ms)
        if (e == hipSuccess) timer.read(ctx);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, MSPLAT_ERR_HIP, "%s: the store of the %u kept splats could not be made: %s", who, K, hipGetErrorString(e));
    }
    buf_free(ctx, sc.tmp);
    if ((rc = fresh_adopt(ctx, fs, K, full_sh, nullptr))) return rc;
    if (n_kept_out) *n_kept_out = K;
    return MSPLAT_OK;
}
