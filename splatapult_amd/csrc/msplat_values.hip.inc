// msplat_values.hip.inc -- selection by attribute: msplat_cloud_values (one float per splat: a coordinate, alpha, the base colour, an
// axis length ...), msplat_mark_values (such an array compared with a closed range into a mask) and msplat_histogram_values (its
// histogram and summary); kernels in msplat_values.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_select.hip.inc)
//
// The split of the scores: one call produces a per-splat array, the others consume it.  Like the selection by position the calls read
// the STORE (whatever the mask and the crop hide), speak upload numbering, need no Sort and leave the context, its frames and its
// timings alone.  The first two are asynchronous on the context's stream; the histogram returns after its copies like msplat_measure_cloud.

static_assert(kValueX == MSPLAT_VALUE_X && kValueReach2 == MSPLAT_VALUE_REACH2 && kValueDistance2 == MSPLAT_VALUE_DISTANCE2 &&
              kValueAlpha == MSPLAT_VALUE_ALPHA && kValueRed == MSPLAT_VALUE_RED && kValueBlue == MSPLAT_VALUE_BLUE &&
              kValueColourDist2 == MSPLAT_VALUE_COLOUR_DIST2 && kValueScaleMin == MSPLAT_VALUE_SCALE_MIN && kValueScaleMax == MSPLAT_VALUE_SCALE_MAX,
              "the kernels' kinds mirror MSPLAT_VALUE_*");
constexpr uint32_t kValueBinsMax = 4096;

// d_values: n floats of device memory of the context's device, 4-byte aligned (n > 0)
static int check_values(msplat_ctx* ctx, const char* who, const float* d_values, uint64_t n)
{
    if (!d_values) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: d_values is NULL", who);
    return check_device_array(ctx, who, "d_values", d_values, 4, n);
}

int msplat_cloud_values(msplat_ctx* ctx, int32_t kind, const float param[4], float* d_values, uint64_t n)
{
    static const char* who = "msplat_cloud_values";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (kind < 0 || kind >= kValueKinds) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: kind %d is not one of MSPLAT_VALUE_* (0..%d)", who, kind, kValueKinds - 1);
    CloudValuesArgs a;
    std::memset(&a, 0, sizeof(a));
    if (kind == kValueDistance2 || kind == kValueColourDist2) {
        if (!param) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: param is NULL for a kind that reads it", who);
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(param[k])) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: param[%d] is not finite", who, k);
            a.p[k] = param[k];
        }
    }
    int rc;
    if ((rc = check_splat_bytes(ctx, who, "d_values", d_values, n, false)) || n == 0) return rc;
    if ((rc = check_values(ctx, who, d_values, n))) return rc;      // (the alignment, and all 4 n bytes)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_order_dev(ctx))) return rc;
    a.pos = (const float4*)ctx->pos4.p;
    a.recs = (const float4*)ctx->recs.p;
    a.order = ctx->store->reordered ? (const uint32_t*)ctx->store->order_dev.p : nullptr;
    a.n = (uint32_t)n;
    a.kind = kind;
    a.out = d_values;
    const dim3 grid(div_up(n, kThreads)), block(kThreads);
    hipStream_t s = ctx->stream;
    const int group = values_group(kind);
    if (group == kValuesOfPos) {
        hipLaunchKernelGGL((cloud_values_kernel<false, kStorageFp32, kValuesOfPos>), grid, block, 0, s, a);
    } else {
        with_flag(ctx->full_sh, [&](auto SH) {
            with_int<kStorageShQ8, kStorageShFp16, kStorageFp32>(ctx->store->storage, [&](auto ST) {
                if constexpr (ST.value == kStorageShQ8 && !SH.value) return;      // (no such store: prepare_cloud_buffers)
                else
                    with_int<kValuesOfScale, kValuesOfColour, kValuesOfAlpha>(group, [&](auto G) {
                        hipLaunchKernelGGL((cloud_values_kernel<SH.value, ST.value, G.value>), grid, block, 0, s, a);
                    });
            });
        });
    }
    if (hipGetLastError() != hipSuccess) return fail(ctx, MSPLAT_ERR_HIP, "%s: the kernel launch failed", who);
    return MSPLAT_OK;
}

int msplat_mark_values(msplat_ctx* ctx, const float* d_values, uint64_t n, float lo, float hi, int32_t op, uint8_t* d_mask, uint8_t value)
{
    static const char* who = "msplat_mark_values";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (op != MSPLAT_RANGE_INSIDE && op != MSPLAT_RANGE_OUTSIDE)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: op %d is neither MSPLAT_RANGE_INSIDE nor MSPLAT_RANGE_OUTSIDE", who, op);
    if (lo != lo || hi != hi) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s is NaN", who, lo != lo ? "lo" : "hi");
    int rc;
    if ((rc = check_splat_bytes(ctx, who, "d_mask", d_mask, n, false)) || n == 0) return rc;
    if ((rc = check_values(ctx, who, d_values, n))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_per_item(ctx, who, n, mark_values_kernel, d_values, (uint32_t)n, lo, hi, op == MSPLAT_RANGE_OUTSIDE ? 1 : 0, d_mask, value);
}

int msplat_histogram_values(msplat_ctx* ctx, const float* d_values, const uint8_t* d_select, uint64_t n, float lo, float hi, uint32_t bins,
                            uint32_t* counts, msplat_value_summary* out)
{
    static const char* who = "msplat_histogram_values";
    static_assert(sizeof(ValueRow) == 32, "the scratch size msplat.h states");
    constexpr size_t kScratch = (size_t)kValueBinsMax * 4 + ((size_t)kGridCap + 1) * sizeof(ValueRow);
    static_assert(kScratch == 81952, "the scratch size msplat.h states");
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!out) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: out is NULL", who);
    if (out->struct_size < offsetof(msplat_value_summary, vmax) + sizeof(out->vmax))
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: struct_size %u ends before vmax (sizeof(msplat_value_summary) is %zu)", who,
                    out->struct_size, sizeof(msplat_value_summary));
    float scale = 0.0f;
    if (bins == 0) {
        lo = hi = 0.0f;                                     // (not read)
    } else {
        if (bins > kValueBinsMax) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %u bins (at most %u)", who, bins, kValueBinsMax);
        if (!counts) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: counts is NULL with bins = %u", who, bins);
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi))
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: [lo, hi] = [%g, %g] is not a finite range with lo < hi", who, (double)lo, (double)hi);
        scale = (float)((double)bins / ((double)hi - (double)lo));
        if (!std::isnormal(scale))
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: bins / (hi - lo) = %g is not a normal fp32 number", who, (double)bins / ((double)hi - (double)lo));
    }
    int rc;
    if ((rc = check_splat_bytes(ctx, who, "d_select", d_select, n, true))) return rc;
    if (n != 0 && (rc = check_values(ctx, who, d_values, n))) return rc;
    ValueRow row;
    row.clear();
    if (n != 0) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if ((rc = buf_alloc(ctx, ctx->value_hist, kScratch))) return rc;
        uint32_t* d_counts = (uint32_t*)ctx->value_hist.p;                                    // counts first, then the rows
        hipStream_t s = ctx->stream;
        if (bins) HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)bins * 4, s));             // (outside the timed pair)
        rc = reduce_rows(ctx, who, (ValueRow*)(d_counts + kValueBinsMax), n, row, [&](int grid, ValueRow* part) {
            hipLaunchKernelGGL(histogram_values_kernel, dim3(grid), dim3(kThreads), (size_t)bins * 4, s, d_values, d_select, (uint32_t)n, lo, hi, scale,
                               bins, d_counts, part);
        }, [&] { return bins ? hipMemcpyAsync(counts, d_counts, (size_t)bins * 4, hipMemcpyDeviceToHost, s) : hipSuccess; });
        if (rc) return rc;
    } else {
        for (uint32_t b = 0; b < bins; ++b) counts[b] = 0u;
    }
    out->selected = row.selected;
    out->finite = row.finite;
    out->nan = row.nan;
    out->below = row.below;
    out->above = row.above;
    out->vmin = row.vmin;
    out->vmax = row.vmax;
    return MSPLAT_OK;
}
