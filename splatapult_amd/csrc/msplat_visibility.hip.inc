// msplat_visibility.hip.inc -- per-splat visibility: msplat_set_visibility[_device], msplat_set_crop, msplat_get_visibility and the launch of
// visibility_kernel (msplat_cloud.hip.h) a Sort starts with when something changed
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_upload.hip.inc)
//
// A hidden splat is a splat the presort cull rejects.  The context keeps a copy of the position plane with a NaN x where the mask
// or the crop hides a splat, and cull boxes over the visible ones; its Sorts read those instead of the store's (sort_positions,
// launch_box_cull).  With nothing set the pointers are the store's and nothing here runs.  The front-door refusals, the pinned staging
// slot of the host route and the rule by which the mask outlives a cloud edit (KeptPlanes) are msplat_edit.hip.inc's.

// does the context sort from its own plane?  (a crop set before the upload of a POINT cloud stays set and is not applied)
static bool vis_active(const msplat_ctx* ctx)
{
    return !ctx->point_mode && (ctx->has_mask || ctx->crop_shape != 0) && ctx->vis_pos4.p != nullptr;
}

// the plane pass 0 of the sort reads
static const float4* sort_positions(const msplat_ctx* ctx) { return (const float4*)(vis_active(ctx) ? ctx->vis_pos4.p : ctx->pos4.p); }

// visibility_kernel over the store's plane into the context's plane and boxes
static void launch_visibility(msplat_ctx* ctx)
{
    ctx->vis_dirty = false;
    if (ctx->N == 0) return;
    const CloudStore* st = ctx->store.get();
    VisibilityArgs a;
    a.pos = (const float4*)ctx->pos4.p;
    a.mask = ctx->has_mask ? (const uint8_t*)ctx->vis_mask.p : nullptr;
    a.order = ctx->has_mask && st->reordered ? (const uint32_t*)st->order_dev.p : nullptr;
    a.n = (uint32_t)ctx->N;
    a.shape = ctx->crop_shape;
    std::memcpy(a.m, ctx->crop_mat, sizeof(a.m));
    a.vis_pos = (float4*)ctx->vis_pos4.p;
    a.boxes = (CullBox*)ctx->vis_boxes.p;
    hipLaunchKernelGGL(visibility_kernel, dim3(div_up(ctx->N, kBoxSplats)), dim3(kThreads), 0, ctx->stream, a);
}

// the store's storage order on the device, once per reordered store (a blocking copy: complete before any launch that follows)
static int ensure_order_dev(msplat_ctx* ctx)
{
    CloudStore& st = *ctx->store;
    if (!st.reordered) return MSPLAT_OK;
    std::lock_guard<std::mutex> lk(st.mu);
    if (st.order_dev.p) return MSPLAT_OK;
    const size_t bytes = st.order_host.size() * sizeof(uint32_t);
    void* p = nullptr;
    HIP_TRY(ctx, hipMalloc(&p, bytes));
    const hipError_t e = hipMemcpy(p, st.order_host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(ctx, MSPLAT_ERR_HIP, "copying the storage order to the device failed: %s", hipGetErrorString(e));
    }
    st.order_dev.p = p;
    st.order_dev.bytes = bytes;
    return MSPLAT_OK;
}

// both mask routes.  Every refusal comes before anything is allocated, launched or copied
static int set_mask(msplat_ctx* ctx, const char* who, const uint8_t* src, uint64_t n, bool on_device)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    int rc;
    if ((rc = require_splat_cloud(ctx, who, "visibility is for splat clouds", " (a mask is in the cloud's upload numbering)"))) return rc;
    if (!src) {                     // no mask
        ctx->vis_dirty = ctx->vis_dirty || ctx->has_mask;
        ctx->has_mask = false;
        return MSPLAT_OK;
    }
    if (n != ctx->N)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %llu mask bytes for a cloud of %llu splats", who, (unsigned long long)n,
                    (unsigned long long)ctx->N);
    if (on_device && n && (rc = check_device_source(ctx, who, "d_visible", src, n))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = vis_alloc(ctx)) || (rc = buf_alloc(ctx, ctx->vis_mask, std::max<uint64_t>(n, 1))) || (rc = ensure_order_dev(ctx))) return rc;
    if (on_device) {
        if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->vis_mask.p, src, n, hipMemcpyDeviceToDevice, ctx->stream));
    } else if (n && (rc = stage_copy(ctx, ctx->vis_stage, ctx->vis_mask.p, src, n))) {      // (the caller's array is free on return)
        return rc;
    }
    ctx->has_mask = true;
    ctx->vis_dirty = true;
    return MSPLAT_OK;
}

int msplat_set_visibility(msplat_ctx* ctx, const uint8_t* visible, uint64_t n)
{
    return set_mask(ctx, "msplat_set_visibility", visible, n, false);
}

int msplat_set_visibility_device(msplat_ctx* ctx, const uint8_t* d_visible, uint64_t n)
{
    return set_mask(ctx, "msplat_set_visibility_device", d_visible, n, true);
}

int msplat_set_crop(msplat_ctx* ctx, const float worldToCrop[16], int32_t shape)
{
    static const char* who = "msplat_set_crop";
    drain_async(ctx);
    if (!worldToCrop) shape = MSPLAT_CROP_NONE;
    const int32_t base = shape & ~MSPLAT_CROP_INVERT;
    if (shape != MSPLAT_CROP_NONE && base != MSPLAT_CROP_BOX && base != MSPLAT_CROP_SPHERE)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: shape must be MSPLAT_CROP_NONE, or MSPLAT_CROP_BOX / _SPHERE with or without "
                    "MSPLAT_CROP_INVERT (got 0x%x)", who, (unsigned)shape);
    int rc;
    if (shape != MSPLAT_CROP_NONE && (rc = check_affine_finite(ctx, who, "worldToCrop", worldToCrop))) return rc;
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (ctx->has_cloud && (rc = require_splat_cloud(ctx, who, "visibility is for splat clouds"))) return rc;      // (a crop may precede the cloud)
    if (shape != MSPLAT_CROP_NONE && ctx->has_cloud) {       // (before the upload: prepare_cloud_buffers allocates)
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if ((rc = vis_alloc(ctx))) return rc;
    }
    ctx->vis_dirty = ctx->vis_dirty || shape != MSPLAT_CROP_NONE || ctx->crop_shape != 0;
    ctx->crop_shape = shape;
    if (shape != MSPLAT_CROP_NONE) std::memcpy(ctx->crop_mat, worldToCrop, sizeof(ctx->crop_mat));
    return MSPLAT_OK;
}

int msplat_get_visibility(msplat_ctx* ctx, int32_t* has_mask, int32_t* crop_shape, uint64_t* hidden)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (has_mask) *has_mask = ctx->has_mask ? 1 : 0;
    if (crop_shape) *crop_shape = ctx->crop_shape;
    if (hidden) {
        uint64_t h = 0;
        if (ctx->has_sort && ctx->vis_sorted && ctx->N != 0) {      // the boxes of the latest Sort's plane, 32 bytes per 256 splats
            std::vector<CullBox> boxes;
            try {
                boxes.resize(div_up(ctx->N, kBoxSplats));
            } catch (const std::exception&) {
                return fail(ctx, MSPLAT_ERR_HIP, "msplat_get_visibility: out of host memory");
            }
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipMemcpyAsync(boxes.data(), ctx->vis_boxes.p, boxes.size() * sizeof(CullBox), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (const CullBox& b : boxes) h += (uint64_t)b.hi.w;
        }
        *hidden = h;
    }
    return MSPLAT_OK;
}
