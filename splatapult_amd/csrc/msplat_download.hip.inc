// msplat_download.hip.inc -- the cloud out of the device: msplat_download_cloud_device (records), msplat_download_attributes_device and
// msplat_download_ply_vertices_device (the PLY attributes) into the caller's device memory, and msplat_export_ply, a file any 3DGS
// tool loads; kernels in msplat_download.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_append.hip.inc)
//
// The mirror image of the uploads from device memory: every refusal comes before anything is launched, the pointer query is the
// first HIP call, the kernel runs on the context's stream -- behind the frames queued there -- and the call returns after the stream
// has drained.  Nothing of the context changes: the store is only read (a reordered store gets its order on the device, as a mask
// gives it), the inverse order lives for the call.

// who may download: a context that holds a splat cloud
static int check_download(msplat_ctx* ctx, const char* who)
{
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "%s: ctx is NULL", who);
    return require_splat_cloud(ctx, who, "the call is for splat clouds");
}

// a destination of `bytes` bytes: there, aligned, memory of the context's device
static int check_download_target(msplat_ctx* ctx, const char* who, const char* what, const void* p, uint64_t bytes, uint32_t align)
{
    if (!p) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s is NULL", who, what);
    if (reinterpret_cast<uintptr_t>(p) % align != 0)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s must be %u-byte aligned", who, what, align);
    return check_device_source(ctx, who, what, p, bytes);
}

// upload index -> stored slot of a reordered store, for one call (inv.p stays null for a store in upload order); launched on the stream
static int download_inverse_order(msplat_ctx* ctx, const char* who, Buf& inv)
{
    const CloudStore& st = *ctx->store;
    if (!st.reordered) return MSPLAT_OK;
    int rc = ensure_order_dev(ctx);
    if (!rc) rc = buf_alloc(ctx, inv, (size_t)ctx->N * 4);
    if (rc) return rc;
    hipLaunchKernelGGL(invert_order_kernel, dim3(grid_for(div_up(ctx->N, kThreads), ctx->grid_cap)), dim3(kThreads), 0, ctx->stream,
                       (const uint32_t*)st.order_dev.p, (uint32_t)ctx->N, words(inv));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        buf_free(ctx, inv);
        return fail(ctx, MSPLAT_ERR_HIP, "%s: inverting the storage order failed: %s", who, hipGetErrorString(e));
    }
    return MSPLAT_OK;
}

extern "C++" {      // (templates)
// launch(SH, ST) for the store's <full SH, storage> pair
template <class Launch>
static void with_store_kind(msplat_ctx* ctx, Launch&& launch)
{
    with_flag(ctx->full_sh, [&](auto SH) {
        with_int<kStorageShQ8, kStorageShFp16, kStorageFp32>(ctx->cloud_storage, [&](auto ST) {
            if constexpr (ST.value == kStorageShQ8 && !SH.value) return;      // (no such store: prepare_cloud_buffers)
            else launch(SH, ST);
        });
    });
}

// The launch the three device routes share, N > 0: launch(SH, ST, inv) issues the route's kernel over all N rows.  Returns after the
// stream has drained.  (enable_timing: the kernel alone between two stream events, KernelTimer -> msplat_debug_upload_kernel_ms.)
template <class Launch>
static int run_download(msplat_ctx* ctx, const char* who, Launch&& launch)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Buf inv;
    int rc = download_inverse_order(ctx, who, inv);
    if (rc) return rc;
    KernelTimer timer(ctx);
    timer.start(ctx->stream);
    with_store_kind(ctx, [&](auto SH, auto ST) { launch(SH, ST, (const uint32_t*)inv.p); });
    hipError_t e = hipGetLastError();
    timer.stop(ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) timer.read(ctx);
    buf_free(ctx, inv);
    if (e != hipSuccess) return fail(ctx, MSPLAT_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    return MSPLAT_OK;
}
}  // extern "C++"

// msplat_download_cloud with the destination in device memory: unpack_kernel instead of the host loop, the same bytes
int msplat_download_cloud_device(msplat_ctx* ctx, void* d_aos, uint64_t cap_bytes)
{
    static const char* who = "msplat_download_cloud_device";
    drain_async(ctx);
    int rc = check_download(ctx, who);
    if (rc) return rc;
    const uint64_t N = ctx->N;
    if (N == 0) return MSPLAT_OK;
    const uint32_t rec = ctx->full_sh ? 244u : 100u;
    if (cap_bytes < N * rec)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %llu bytes for %llu records of %u", who, (unsigned long long)cap_bytes,
                    (unsigned long long)N, rec);
    if ((rc = check_download_target(ctx, who, "d_aos", d_aos, N * rec, 16))) return rc;
    return run_download(ctx, who, [&](auto SH, auto ST, const uint32_t* inv) {
        hipLaunchKernelGGL((unpack_kernel<SH.value, ST.value>), dim3(div_up(N, 64)), dim3(64), download_lds_bytes(ST.value, SH.value, rec),
                           ctx->stream, (const float4*)ctx->recs.p, inv, 0u, (uint32_t)N, (char*)d_aos);
    });
}

// the six arrays msplat_upload_attributes_device takes, written by egress_kernel: GaussianCloud::ExportPly's values of the cloud
int msplat_download_attributes_device(msplat_ctx* ctx, uint64_t n, float* d_xyz, float* d_f_dc, float* d_f_rest, float* d_opacity,
                                      float* d_log_scale, float* d_rot)
{
    static const char* who = "msplat_download_attributes_device";
    drain_async(ctx);
    int rc = check_download(ctx, who);
    if (rc) return rc;
    const uint64_t N = ctx->N;
    if (n != N)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: n = %llu for a cloud of %llu splats", who, (unsigned long long)n, (unsigned long long)N);
    if (N == 0) return MSPLAT_OK;
    const struct { const char* name; float* p; uint32_t floats; } dst[6] = {
        {"d_xyz", d_xyz, 3}, {"d_f_dc", d_f_dc, 3}, {"d_f_rest", d_f_rest, 45}, {"d_opacity", d_opacity, 1}, {"d_log_scale", d_log_scale, 3},
        {"d_rot", d_rot, 4}};
    for (int k = 0; k < 6; ++k) {      // (f_rest is optional)
        if (k == 2 && !d_f_rest) continue;
        if (!dst[k].p) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s is NULL", who, dst[k].name);
        if (reinterpret_cast<uintptr_t>(dst[k].p) % 4 != 0)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s must be 4-byte aligned", who, dst[k].name);
    }
    for (int k = 0; k < 6; ++k)
        if (dst[k].p && (rc = check_device_source(ctx, who, dst[k].name, dst[k].p, N * dst[k].floats * 4))) return rc;
    const AttrWriter W{d_xyz, d_f_dc, d_f_rest, d_opacity, d_log_scale, d_rot};
    return run_download(ctx, who, [&](auto SH, auto ST, const uint32_t* inv) {
        hipLaunchKernelGGL((egress_kernel<SH.value, ST.value, AttrWriter>), dim3(div_up(N, 64)), dim3(64),
                           download_lds_bytes(ST.value, SH.value, 45 * 4), ctx->stream, (const float4*)ctx->recs.p, inv, 0u, (uint32_t)N, W);
    });
}

// egress_kernel over rows row0 .. row0 + cnt - 1 into a vertex block whose first vertex is row row0 (d_vertices: 16-byte aligned)
static void launch_vertex_egress(msplat_ctx* ctx, const uint32_t* inv, uint32_t row0, uint32_t cnt, void* d_vertices, const PlyLayout& kl)
{
    VertexWriter W;
    W.out = (char*)d_vertices;
    W.L = kl;
    with_store_kind(ctx, [&](auto SH, auto ST) {
        hipLaunchKernelGGL((egress_kernel<SH.value, ST.value, VertexWriter>), dim3(div_up(cnt, 64)), dim3(64),
                           download_lds_bytes(ST.value, SH.value, kl.vertex_size), ctx->stream, (const float4*)ctx->recs.p, inv, row0, cnt, W);
    });
}

// the same values as one PLY vertex block of the caller's layout: what msplat_upload_ply_vertices_device reads
int msplat_download_ply_vertices_device(msplat_ctx* ctx, void* d_vertices, uint64_t cap_bytes, const msplat_ply_layout* layout)
{
    static const char* who = "msplat_download_ply_vertices_device";
    drain_async(ctx);
    int rc = check_download(ctx, who);
    if (rc) return rc;
    if (!layout) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: layout is NULL", who);
    bool full = false;
    if ((rc = check_ply_layout(ctx, layout, 1, full))) {
        const std::string why = ctx->err;
        return fail(ctx, rc, "%s: %s", who, why.c_str());
    }
    const uint64_t N = ctx->N;
    if (N == 0) return MSPLAT_OK;
    const uint32_t vs = layout->vertex_size;
    if (cap_bytes < N * vs)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %llu bytes for %llu vertices of %u", who, (unsigned long long)cap_bytes,
                    (unsigned long long)N, vs);
    if ((rc = check_download_target(ctx, who, "d_vertices", d_vertices, N * vs, 16))) return rc;
    PlyLayout kl;
    std::memcpy(&kl, layout, sizeof(kl));
    return run_download(ctx, who, [&](auto, auto, const uint32_t* inv) { launch_vertex_egress(ctx, inv, 0u, (uint32_t)N, d_vertices, kl); });
}

// The file GaussianCloud::ExportPly writes for a cloud of the context's full_sh: its header, then the vertex block of
// msplat_download_ply_vertices_device for that layout.  The block never exists whole: egress_kernel fills one of two device
// buffers of kExportRows vertices, a copy takes it to one of two pinned host buffers, and the host writes a chunk to the file
// while the device works on the next
int msplat_export_ply(msplat_ctx* ctx, const char* path)
{
    static const char* who = "msplat_export_ply";
    constexpr uint32_t kExportRows = 1u << 16;      // 16 MB of 248-byte vertices
    drain_async(ctx);
    int rc = check_download(ctx, who);
    if (rc) return rc;
    if (!path) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: path is NULL", who);
    const uint32_t N = (uint32_t)ctx->N;
    const bool full = ctx->full_sh;
    // ExportPly's properties in its order: x y z nx ny nz f_dc_0..2 [f_rest_0..44] opacity scale_0..2 rot_0..3, all float
    msplat_ply_layout lay;
    std::string header = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(N) + "\n";
    {
        int32_t at = 0;
        auto prop = [&](const std::string& name) { header += "property float " + name + "\n"; at += 4; return at - 4; };
        lay.x = prop("x"); lay.y = prop("y"); lay.z = prop("z");
        prop("nx"); prop("ny"); prop("nz");
        for (int k = 0; k < 3; ++k) lay.f_dc[k] = prop("f_dc_" + std::to_string(k));
        for (int k = 0; k < 45; ++k) lay.f_rest[k] = full ? prop("f_rest_" + std::to_string(k)) : -1;
        lay.opacity = prop("opacity");
        for (int k = 0; k < 3; ++k) lay.scale[k] = prop("scale_" + std::to_string(k));
        for (int k = 0; k < 4; ++k) lay.rot[k] = prop("rot_" + std::to_string(k));
        lay.vertex_size = (uint32_t)at;
        header += "end_header\n";
    }
    PlyLayout kl;
    std::memcpy(&kl, &lay, sizeof(kl));
    const uint32_t vs = lay.vertex_size;
    std::FILE* fp = std::fopen(path, "wb");
    if (!fp) return fail(ctx, MSPLAT_ERR_IO, "%s: cannot open %s for writing", who, path);
    bool io_ok = std::fwrite(header.data(), 1, header.size(), fp) == header.size();
    hipError_t e = hipSuccess;
    if (N && io_ok) {
        e = hipSetDevice(ctx->device);
        const uint32_t chunk = std::min(N, kExportRows), nchunks = div_up(N, chunk);
        const size_t bytes = (size_t)chunk * vs;
        void *d_buf[2] = {nullptr, nullptr}, *h_buf[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {nullptr, nullptr};
        Buf inv;
        for (int b = 0; b < (nchunks > 1 ? 2 : 1) && e == hipSuccess; ++b) {
            e = hipMalloc(&d_buf[b], bytes);
            if (e == hipSuccess) e = hipHostMalloc(&h_buf[b], bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[b], hipEventDisableTiming);
        }
        if (e == hipSuccess && (rc = download_inverse_order(ctx, who, inv))) e = hipErrorUnknown;      // (the message is set)
        auto rows_of = [&](uint32_t c) { return std::min(chunk, N - c * chunk); };
        for (uint32_t c = 0; c < nchunks && e == hipSuccess && io_ok; ++c) {
            const int b = (int)(c & 1u);
            launch_vertex_egress(ctx, (const uint32_t*)inv.p, c * chunk, rows_of(c), d_buf[b], kl);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(h_buf[b], d_buf[b], (size_t)rows_of(c) * vs, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(ev[b], ctx->stream);
            if (c > 0 && e == hipSuccess) {      // the chunk before this one, while the device works on this one
                e = hipEventSynchronize(ev[b ^ 1]);
                const size_t w = (size_t)rows_of(c - 1) * vs;
                if (e == hipSuccess) io_ok = std::fwrite(h_buf[b ^ 1], 1, w, fp) == w;
            }
        }
        const hipError_t drained = hipStreamSynchronize(ctx->stream);      // (whatever happened: the buffers are freed below)
        if (e == hipSuccess) e = drained;
        if (e == hipSuccess && io_ok) {
            const size_t w = (size_t)rows_of(nchunks - 1) * vs;
            io_ok = std::fwrite(h_buf[(nchunks - 1) & 1u], 1, w, fp) == w;
        }
        for (int b = 0; b < 2; ++b) {
            if (ev[b]) (void)hipEventDestroy(ev[b]);
            if (h_buf[b]) (void)hipHostFree(h_buf[b]);
            if (d_buf[b]) (void)hipFree(d_buf[b]);
        }
        buf_free(ctx, inv);
        if (e != hipSuccess) (void)hipGetLastError();
    }
    io_ok = (std::fclose(fp) == 0) && io_ok;
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, MSPLAT_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    if (!io_ok) return fail(ctx, MSPLAT_ERR_IO, "%s: writing %s failed", who, path);
    return MSPLAT_OK;
}
