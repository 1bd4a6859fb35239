// msplat_overlay.hip.inc -- the render-time overlay: msplat_set_overlay[_device], msplat_set_overlay_palette, msplat_get_overlay and the
// launches of overlay_classes_kernel / overlay_kernel (msplat_overlay.hip.h) behind the projection of a Render
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_visibility.hip.inc)
//
// A class byte per splat (upload numbering) and a palette of up to 256 RGBA entries tint the colours project_kernel left in the
// records, before the compositor reads them: the cloud, its Sort and its lists stay as they are, and a change shows at the next
// Render.  With no classes, no palette or a palette of a == 0 only, nothing here runs and a Render launches what it always did.
// The host routes stage through the context's slots (stage_copy) and the classes outlive a transform or an append as the mask does
// (KeptPlanes): both in msplat_edit.hip.inc.

// does a Render of the context tint its records?
static bool overlay_active(const msplat_ctx* ctx) { return !ctx->point_mode && ctx->has_classes && ctx->ov_tints; }

// what a Render with an active overlay refuses, before anything is launched: the draw-order compositors of the emulations blend
// in the target's precision record by record and the probe's frame is a measurement of the plain chain -- neither is an editing viewport
static int overlay_frame_checks(msplat_ctx* ctx)
{
    if (!overlay_active(ctx)) return MSPLAT_OK;
    const char* why = ctx->depth_bits != 0 ? "msplat_set_depth_test is on"
                      : ctx->rop != MSPLAT_ROP_NONE ? "msplat_set_target_emulation is not MSPLAT_ROP_NONE"
                      : ctx->probe_on ? "the tile probe (msplat_set_tile_probe) is on" : nullptr;
    if (why) return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_render: %s while an overlay is active (msplat_set_overlay: clear the classes or the palette)", why);
    return MSPLAT_OK;
}

// overlay_kernel over the records the projection just wrote (ranks: the cloud's N, 2 N + 64 for two views in one chain); before it,
// where the classes or the store's order changed, the classes in storage order
static void launch_overlay(msplat_ctx* ctx, hipStream_t s, const uint32_t* d_V, uint32_t ranks, bool two_views)
{
    const bool reordered = ctx->store && ctx->store->reordered;
    if (ctx->overlay_dirty && reordered && ctx->N != 0)
        hipLaunchKernelGGL(overlay_classes_kernel, dim3(grid_for(div_up(ctx->N, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s,
                           (const uint8_t*)ctx->ov_cls.p, (const uint32_t*)ctx->store->order_dev.p, (uint32_t)ctx->N, (uint8_t*)ctx->ov_slot.p);
    ctx->overlay_dirty = false;
    if (ctx->N == 0) return;
    hipLaunchKernelGGL(overlay_kernel, dim3(grid_for(div_up(ranks, kThreads), ctx->grid_cap)), dim3(kThreads), 0, s,
                       (const uint32_t*)ctx->valA.p, d_V, (const uint8_t*)(reordered ? ctx->ov_slot.p : ctx->ov_cls.p),
                       (const float4*)ctx->ov_pal.p, (float*)ctx->rec2d.p, two_views ? 1u : 0u);
}

// the slot array of a store in Morton order, and that store's order on the device
static int overlay_slot_alloc(msplat_ctx* ctx)
{
    if (!ctx->store || !ctx->store->reordered) return MSPLAT_OK;
    int rc = buf_alloc(ctx, ctx->ov_slot, std::max<uint64_t>(ctx->N, 1));
    return rc ? rc : ensure_order_dev(ctx);
}

// both class routes.  Every refusal comes before anything is allocated, launched or copied
static int set_overlay_classes(msplat_ctx* ctx, const char* who, const uint8_t* src, uint64_t n, bool on_device)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    int rc;
    if ((rc = require_splat_cloud(ctx, who, "the overlay is for splat clouds", " (classes are in the cloud's upload numbering)"))) return rc;
    if (!src) {                     // no classes
        ctx->has_classes = ctx->overlay_dirty = false;
        return MSPLAT_OK;
    }
    if (n != ctx->N)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %llu class bytes for a cloud of %llu splats", who, (unsigned long long)n,
                    (unsigned long long)ctx->N);
    if (on_device && n && (rc = check_device_source(ctx, who, "d_classes", src, n))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = buf_alloc(ctx, ctx->ov_cls, std::max<uint64_t>(n, 1))) || (rc = overlay_slot_alloc(ctx))) return rc;
    if (on_device) {
        if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->ov_cls.p, src, n, hipMemcpyDeviceToDevice, ctx->stream));
    } else if (n && (rc = stage_copy(ctx, ctx->ov_stage[0], ctx->ov_cls.p, src, n))) {
        return rc;
    }
    ctx->has_classes = true;
    ctx->overlay_dirty = true;
    return MSPLAT_OK;
}

int msplat_set_overlay(msplat_ctx* ctx, const uint8_t* classes, uint64_t n)
{
    return set_overlay_classes(ctx, "msplat_set_overlay", classes, n, false);
}

int msplat_set_overlay_device(msplat_ctx* ctx, const uint8_t* d_classes, uint64_t n)
{
    return set_overlay_classes(ctx, "msplat_set_overlay_device", d_classes, n, true);
}

int msplat_set_overlay_palette(msplat_ctx* ctx, const float* rgba, uint32_t count)
{
    static const char* who = "msplat_set_overlay_palette";
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!rgba) count = 0;
    if (count > (uint32_t)kOverlayEntries)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %u palette entries (at most %d)", who, count, kOverlayEntries);
    bool tints = false;
    for (uint32_t k = 0; k < 4 * count; ++k) {
        if (!std::isfinite(rgba[k])) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: rgba[%u] is not finite", who, k);
        if (k % 4 == 3) {
            if (!(rgba[k] >= 0.0f && rgba[k] <= 1.0f))
                return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: the a of entry %u is %g, outside [0, 1]", who, k / 4, (double)rgba[k]);
            tints = tints || rgba[k] != 0.0f;
        }
    }
    if (count) {            // all kOverlayEntries entries: those beyond count with a = 0, which is "no effect"
        float pal[4 * kOverlayEntries] = {};
        std::memcpy(pal, rgba, (size_t)count * 16);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        int rc;
        if ((rc = buf_alloc(ctx, ctx->ov_pal, sizeof(pal))) || (rc = stage_copy(ctx, ctx->ov_stage[1], ctx->ov_pal.p, pal, sizeof(pal)))) return rc;
    }
    ctx->ov_count = count;
    ctx->ov_tints = tints;
    return MSPLAT_OK;
}

int msplat_get_overlay(msplat_ctx* ctx, int32_t* has_classes, uint32_t* palette_count, int32_t* active)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (has_classes) *has_classes = ctx->has_classes ? 1 : 0;
    if (palette_count) *palette_count = ctx->ov_count;
    if (active) *active = overlay_active(ctx) ? 1 : 0;
    return MSPLAT_OK;
}
