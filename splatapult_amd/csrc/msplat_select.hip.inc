// msplat_select.hip.inc -- selection by position: msplat_mark_volume (the crop rule as a mask), msplat_mark_view (select through, by
// projected centre), msplat_measure_cloud (count, box, centroid sums of a selection) and the host helper msplat_measure_box; kernels
// in msplat_select.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_scores.hip.inc, whose window it shares)
//
// All three device calls read the STORE's position plane (ctx->pos4: the cloud, whatever the mask and the crop hide), speak upload
// numbering through the store's order table, need no Sort and leave the context, its frames and its timings alone.  The marks are
// asynchronous on the context's stream like msplat_mark_scores; the measure returns after its 112-byte copy like msplat_get_visibility.

int msplat_mark_volume(msplat_ctx* ctx, const float worldToVolume[16], int32_t shape, uint8_t* d_mask, uint64_t n, uint8_t value)
{
    static const char* who = "msplat_mark_volume";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!worldToVolume) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: worldToVolume is NULL", who);
    const int32_t base = shape & ~MSPLAT_CROP_INVERT;
    if (base != MSPLAT_CROP_BOX && base != MSPLAT_CROP_SPHERE)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: shape must be MSPLAT_CROP_BOX or _SPHERE, with or without MSPLAT_CROP_INVERT (got 0x%x)",
                    who, (unsigned)shape);
    int rc;
    if ((rc = check_affine_finite(ctx, who, "worldToVolume", worldToVolume))) return rc;
    if ((rc = check_splat_bytes(ctx, who, "d_mask", d_mask, n, false)) || n == 0) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_order_dev(ctx))) return rc;
    MarkVolumeArgs a;
    a.pos = (const float4*)ctx->pos4.p;
    a.order = ctx->store->reordered ? (const uint32_t*)ctx->store->order_dev.p : nullptr;
    a.n = (uint32_t)n;
    a.shape = shape;
    std::memcpy(a.m, worldToVolume, sizeof(a.m));
    a.mask = d_mask;
    a.value = value;
    return launch_per_item(ctx, who, n, mark_volume_kernel, a);
}

int msplat_mark_view(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2],
                     const int32_t window[4], const uint8_t* d_region, uint64_t region_pitch_bytes, uint8_t* d_mask, uint64_t n,
                     uint8_t value)
{
    static const char* who = "msplat_mark_view";
    (void)nearFar;                                          // (the frame calls' signature; the rule has no depth range)
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!cameraMat || !projMat || !viewport) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: NULL matrix/viewport argument", who);
    MarkViewArgs a;
    float view[16];
    msplat_mat4_inverse(cameraMat, view);                   // make_frame_params' two steps: the Sort's mvp, bit for bit
    msplat_mat4_mul(projMat, view, a.mvp);
    a.W = viewport[2];
    a.H = viewport[3];
    const int width = (int)viewport[2], height = (int)viewport[3];
    if (width < 1 || height < 1 || width > 8192 || height > 8192)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: viewport %dx%d outside [1,8192]^2", who, width, height);
    IdsWindow win{window != nullptr, {0, 0, 0, 0}};
    if (window) std::memcpy(win.v, window, sizeof(win.v));
    int rc;
    if ((rc = frame_window(ctx, who, width, height, win))) return rc;
    const int32_t* w = win.v;
    if ((rc = region_pitch(ctx, who, d_region, region_pitch_bytes, w[2]))) return rc;
    if ((rc = check_splat_bytes(ctx, who, "d_mask", d_mask, n, false)) || n == 0) return rc;
    if ((rc = check_region(ctx, who, d_region, region_pitch_bytes, w[2], w[3]))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_order_dev(ctx))) return rc;
    a.pos = (const float4*)ctx->pos4.p;
    a.order = ctx->store->reordered ? (const uint32_t*)ctx->store->order_dev.p : nullptr;
    a.n = (uint32_t)n;
    a.x0 = (float)w[0]; a.y0 = (float)w[1]; a.x1 = (float)(w[0] + w[2]); a.y1 = (float)(w[1] + w[3]);
    a.region = d_region;
    a.region_pitch = (size_t)region_pitch_bytes;
    a.mask = d_mask;
    a.value = value;
    return launch_per_item(ctx, who, n, mark_view_kernel, a);
}

int msplat_measure_cloud(msplat_ctx* ctx, const uint8_t* d_select, uint64_t n, msplat_cloud_measure* out)
{
    static const char* who = "msplat_measure_cloud";
    static_assert(sizeof(MeasureRow) == 112, "the scratch size msplat.h states");
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: out is NULL", who);
    if (out->struct_size < offsetof(msplat_cloud_measure, sum2) + sizeof(out->sum2))
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: struct_size %u ends before sum2 (sizeof(msplat_cloud_measure) is %zu)", who,
                    out->struct_size, sizeof(msplat_cloud_measure));
    int rc;
    if ((rc = check_splat_bytes(ctx, who, "d_select", d_select, n, true))) return rc;
    MeasureRow row;
    row.clear();
    if (n != 0) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if ((rc = buf_alloc(ctx, ctx->measure_rows, ((size_t)kGridCap + 1) * sizeof(MeasureRow))) || (d_select && (rc = ensure_order_dev(ctx)))) return rc;
        const uint32_t* order = d_select && ctx->store->reordered ? (const uint32_t*)ctx->store->order_dev.p : nullptr;
        rc = reduce_rows(ctx, who, (MeasureRow*)ctx->measure_rows.p, n, row, [&](int grid, MeasureRow* part) {
            hipLaunchKernelGGL(measure_cloud_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, (const float4*)ctx->pos4.p, order, d_select, (uint32_t)n, part);
        }, [] { return hipSuccess; });
        if (rc) return rc;
    }
    out->selected = row.selected;
    out->finite = row.finite;
    for (int k = 0; k < 3; ++k) { out->lo[k] = row.lo[k]; out->hi[k] = row.hi[k]; out->sum[k] = row.s[k]; }
    out->reach2_max = row.reach;
    for (int k = 0; k < 6; ++k) out->sum2[k] = row.s[3 + k];
    return MSPLAT_OK;
}

// host only, in double, rounded once: the axis-aligned worldToVolume whose BOX holds every measured centre under crop_inside's fp32
int msplat_measure_box(const msplat_cloud_measure* m, float pad, float worldToVolume[16])
{
    static const char* who = "msplat_measure_box";
    if (!m || !worldToVolume) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "%s: %s is NULL", who, m ? "worldToVolume" : "the measure");
    if (m->struct_size < offsetof(msplat_cloud_measure, reach2_max))
        return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "%s: struct_size %u ends before reach2_max", who, m->struct_size);
    if (m->finite == 0) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "%s: the measure holds no finite centre", who);
    if (!(pad >= 0.0f) || !std::isfinite(pad)) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "%s: pad must be finite and >= 0 (got %g)", who, (double)pad);
    double scale[3], shift[3];
    for (int k = 0; k < 3; ++k) {
        const double lo = m->lo[k], hi = m->hi[k];
        if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi)
            return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "%s: lo[%d] = %g, hi[%d] = %g is not a box", who, k, lo, k, hi);
        const double c = 0.5 * lo + 0.5 * hi;               // (halved first: lo + hi may overflow nothing in double, and stays exact)
        const double reach = std::max(std::fabs(lo), std::fabs(hi));
        const double h = std::max(0.5 * hi - 0.5 * lo, 0x1p-100) * (1.0 + 0x1p-20) + reach * 0x1p-21 + (double)pad;
        if (!(h <= 0x1p100)) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "%s: half-extent %g of axis %d is beyond 2^100", who, h, k);
        scale[k] = 1.0 / h;
        shift[k] = -c / h;
    }
    for (int k = 0; k < 16; ++k) worldToVolume[k] = 0.0f;
    for (int k = 0; k < 3; ++k) {
        worldToVolume[5 * k] = (float)scale[k];
        worldToVolume[12 + k] = (float)shift[k];
    }
    worldToVolume[15] = 1.0f;
    return MSPLAT_OK;
}
