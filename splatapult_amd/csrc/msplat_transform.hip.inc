// msplat_transform.hip.inc -- msplat_transform_cloud: the selected splats of the context's cloud moved, rotated and scaled by a
// matrix, on the device; kernel in msplat_transform.hip.h, the SH matrices: msplat_sh_rotation (host/gaussian_scene.cpp)
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_compact.hip.inc)
//
// The compaction's shape: an upload whose source is the context's own store.  One kernel writes every record -- transformed or
// copied -- into a FreshStore (msplat_edit.hip.inc) in upload order, the host reads the pack routines' counter, and fresh_adopt makes
// it the context's cloud; every failure up to there leaves the cloud alone.  Unlike an upload the numbering does not change: the
// mask and the overlay's classes stay (KeptPlanes) -- a dragged selection stays hidden or tinted.

int msplat_transform_cloud(msplat_ctx* ctx, const float M[16], const uint8_t* d_select, uint64_t n, int32_t flags)
{
    static const char* who = "msplat_transform_cloud";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!M) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: M is NULL", who);
    int rc;
    if ((rc = check_affine_finite(ctx, who, "M", M))) return rc;
    if (flags & ~MSPLAT_TRANSFORM_KEEP_SH)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~MSPLAT_TRANSFORM_KEEP_SH));
    if ((rc = require_splat_cloud(ctx, who, "the call is for splat clouds"))) return rc;
    const uint64_t N = ctx->N;
    if (n != N)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: n = %llu for a cloud of %llu splats", who, (unsigned long long)n, (unsigned long long)N);
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
                else hipLaunchKernelGGL((transform_kernel<SH.value, ST.value>), dim3(grid), dim3(64), 0, s, a);
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
        return fail(ctx, MSPLAT_ERR_HIP, "%s: the store of the transformed cloud could not be made: %s", who, hipGetErrorString(e));
    }
    if (n_over) return f_rest_failure(ctx, who, storage, n_over, "transformed ", "; the cloud is unchanged");
    KeptPlanes kept(ctx);       // (the planes are as long as they were: the context's own buffers stay)
    return fresh_adopt(ctx, fs, N, full_sh, &kept);
}
