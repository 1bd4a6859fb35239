// msplat_adjust.hip.inc -- msplat_adjust_cloud: the selected splats of the context's cloud recoloured by an affine colour map and /
// or faded by a factor on alpha, on the device; kernel in msplat_adjust.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_append.hip.inc)
//
// The transform's shape: an upload whose source is the context's own store.  One kernel writes every record -- adjusted or copied --
// into a FreshStore (msplat_edit.hip.inc) in upload order, the host reads the pack routines' counter, and fresh_adopt makes it the
// context's cloud; every failure up to there leaves the cloud alone.  The numbering does not change: the mask and the overlay's
// classes stay (KeptPlanes) -- a faded selection stays hidden or tinted.

int msplat_adjust_cloud(msplat_ctx* ctx, const float colour[12], float opacity_scale, const uint8_t* d_select, uint64_t n, int32_t flags)
{
    static const char* who = "msplat_adjust_cloud";
    constexpr int32_t kKnown = MSPLAT_ADJUST_COLOUR | MSPLAT_ADJUST_OPACITY;
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (flags & ~kKnown) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~kKnown));
    if (!flags) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: flags is 0: neither MSPLAT_ADJUST_COLOUR nor MSPLAT_ADJUST_OPACITY", who);
    AdjustArgs a;
    std::memset(&a, 0, sizeof(a));
    a.colour = (flags & MSPLAT_ADJUST_COLOUR) ? 1 : 0;
    a.opacity = (flags & MSPLAT_ADJUST_OPACITY) ? 1 : 0;
    if (a.colour) {
        if (!colour) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: colour is NULL with MSPLAT_ADJUST_COLOUR", who);
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(colour[k])) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: colour[%d] is not finite", who, k);
        for (int k = 0; k < 9; ++k) a.g[k] = colour[k];
        // every colour is 0.5 + SH: G acts on the 0.5 too, and the offset and that 0.5 arrive through the DC term, whose basis is constant
        for (int c = 0; c < 3; ++c)
            a.bias[c] = (float)((((0.5 * (((double)colour[c] + colour[3 + c]) + colour[6 + c])) + colour[9 + c]) - 0.5) / 0.28209479177387814);
    }
    if (a.opacity) {
        if (!std::isfinite(opacity_scale) || opacity_scale < 0.0f)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: opacity_scale = %g is not a finite factor >= 0", who, (double)opacity_scale);
        a.opacity_scale = opacity_scale;
    }
    int rc;
    if ((rc = require_splat_cloud(ctx, who, "the call is for splat clouds"))) return rc;
    const uint64_t N = ctx->N;
    if (n != N)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: n = %llu for a cloud of %llu splats", who, (unsigned long long)n, (unsigned long long)N);
    if (d_select && N && (rc = check_device_source(ctx, who, "d_select", d_select, N))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = ensure_order_dev(ctx))) return rc;
    const CloudStore* old = ctx->store.get();      // (no second owner here: prepare_cloud_buffers reads the use count)
    const int F4 = old->F4, storage = old->storage;
    const bool full_sh = ctx->full_sh;
    hipStream_t s = ctx->stream;

    KernelTimer timer(ctx);
    FreshStore fs;
    uint32_t n_over = 0;
    hipError_t e = fresh_alloc(ctx, fs, N, F4, storage, true);
    if (e == hipSuccess && N) {
        a.pos_in = (const float4*)old->pos4.p;
        a.recs_in = (const float4*)old->recs.p;
        a.order = old->reordered ? (const uint32_t*)old->order_dev.p : nullptr;
        a.select = d_select;
        a.pos_out = (float4*)fs.st->pos4.p;
        a.recs_out = (float4*)fs.st->recs.p;
        a.n_over = fs.d_over;
        a.n = (uint32_t)N;
        timer.start(s);
        const int grid = grid_for(div_up(N, 64), ctx->grid_cap);
        with_flag(full_sh, [&](auto SH) {
            with_int<kStorageShQ8, kStorageShFp16, kStorageFp32>(storage, [&](auto ST) {
                if constexpr (ST.value == kStorageShQ8 && !SH.value) return;      // (no such store: prepare_cloud_buffers)
                else hipLaunchKernelGGL((adjust_kernel<SH.value, ST.value>), dim3(grid), dim3(64), 0, s, a);
            });
        });
        e = hipGetLastError();
        timer.stop(s);
        if (e == hipSuccess) e = hipMemcpyAsync(&n_over, fs.d_over, 4, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && N) timer.read(ctx);      // (the one kernel between two stream events: msplat_debug_upload_kernel_ms)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, MSPLAT_ERR_HIP, "%s: the store of the adjusted cloud could not be made: %s", who, hipGetErrorString(e));
    }
    if (n_over) return f_rest_failure(ctx, who, storage, n_over, "adjusted ", "; the cloud is unchanged");
    KeptPlanes kept(ctx);       // (the planes are as long as they were: the context's own buffers stay)
    return fresh_adopt(ctx, fs, N, full_sh, &kept);
}
