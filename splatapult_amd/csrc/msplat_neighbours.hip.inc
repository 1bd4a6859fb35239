// msplat_neighbours.hip.inc -- selection by neighbourhood: msplat_neighbour_values (per splat, the number of source splats within a
// radius or the squared distance to the nearest one) and the debug tap that forces the grid's bucket count; kernels in
// msplat_neighbours.hip.h
// (textually part of msplat_device.hip: included inside its extern "C" block, after msplat_values.hip.inc, whose check_values it shares)
//
// One more producer of the per-splat float arrays msplat_mark_values and msplat_histogram_values consume.  Like the other selection
// calls it reads the STORE's position plane, speaks upload numbering, needs no Sort and leaves the context and its frames alone.  It
// is synchronous like msplat_measure_cloud: the budget is a decision the host takes between the grid's build and the search.

static_assert(kNearCount == MSPLAT_NEAR_COUNT && kNearDist2 == MSPLAT_NEAR_DIST2, "the kernels' kinds mirror MSPLAT_NEAR_*");
// max_tests = 0: 2^40 candidate pairs, about 2 s of search on an MI355X at the 5.9e11 tests per second measured where a query meets
// some 1700 candidates (1 M splats, tools/neighbours_timing.py; EXPERIMENTS.md round 37).  The sparse rate, 1.0e11 per second at 53
// candidates per query, cannot reach it: 2^24 queries of 53 candidates are 9e8 tests
constexpr uint64_t kNearDefaultTests = 1ull << 40;

// the scratch of one set's list inside ctx->near_cells[s]: cnt[cells] | start[cells] | sums[nchunks] | total
struct NearList {
    uint32_t *cnt, *start, *sums, *total;
    float4* ent;
};

static int near_reserve(msplat_ctx* ctx, int s, uint64_t n, uint32_t nchunks, NearList& l)
{
    const size_t cells = (size_t)nchunks * kNearChunk;
    int rc;
    if ((rc = buf_alloc(ctx, ctx->near_cells[s], (2 * cells + nchunks + 4) * 4)) || (rc = buf_alloc(ctx, ctx->near_ent[s], (size_t)n * 16))) return rc;
    l.cnt = (uint32_t*)ctx->near_cells[s].p;
    l.start = l.cnt + cells;
    l.sums = l.start + cells;
    l.total = l.sums + nchunks;
    l.ent = (float4*)ctx->near_ent[s].p;
    return MSPLAT_OK;
}

// count, scan (three launches), scatter: the members of `set` in bucket order
static hipError_t near_list(msplat_ctx* ctx, const NearList& l, const uint8_t* set, uint64_t n, const NearCells& g, uint32_t nchunks,
                            uint32_t* max_bucket)
{
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemsetAsync(l.cnt, 0, (size_t)nchunks * kNearChunk * 4, s);
    if (e != hipSuccess) return e;
    NearSetArgs a;
    a.pos = (const float4*)ctx->pos4.p;
    a.order = ctx->store->reordered ? (const uint32_t*)ctx->store->order_dev.p : nullptr;
    a.set = set;
    a.n = (uint32_t)n;
    a.g = g;
    a.cnt = l.cnt;
    a.start = l.start;
    a.ent = l.ent;
    const dim3 block(kThreads), slots(grid_for(div_up(n, kThreads), ctx->grid_cap)), chunks(grid_for(nchunks, ctx->grid_cap));
    hipLaunchKernelGGL(neighbour_count_kernel, slots, block, 0, s, a);
    hipLaunchKernelGGL(neighbour_sums_kernel, chunks, block, 0, s, (const uint32_t*)l.cnt, nchunks, l.sums, max_bucket);
    hipLaunchKernelGGL(compact_offsets_kernel, dim3(1), block, 0, s, l.sums, nchunks, l.total);
    hipLaunchKernelGGL(neighbour_starts_kernel, chunks, block, 0, s, (const uint32_t*)l.cnt, (const uint32_t*)l.sums, nchunks, l.start);
    hipLaunchKernelGGL(neighbour_scatter_kernel, slots, block, 0, s, a);
    return hipGetLastError();
}

int msplat_neighbour_values(msplat_ctx* ctx, int32_t kind, float radius, const uint8_t* d_source, const uint8_t* d_query, uint64_t n, uint32_t cap,
                            uint64_t max_tests, float* d_values, msplat_neighbour_info* info)
{
    static const char* who = "msplat_neighbour_values";
    static_assert(sizeof(msplat_neighbour_info) == 32 && offsetof(msplat_neighbour_info, tests) == 24, "the layout msplat.h states");
    static_assert(sizeof(TestsRow) == 8, "the scratch size msplat.h states");
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (kind != MSPLAT_NEAR_COUNT && kind != MSPLAT_NEAR_DIST2)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: kind %d is neither MSPLAT_NEAR_COUNT nor MSPLAT_NEAR_DIST2", who, kind);
    if (!std::isfinite(radius) || !(radius > 0.0f)) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: radius %g is not a finite number > 0", who, (double)radius);
    const float r2 = radius * radius;
    if (!std::isnormal(r2)) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: radius * radius = %g is not a normal fp32 number", who, (double)radius * (double)radius);
    if (kind == MSPLAT_NEAR_DIST2 && cap != 0) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: cap %u with MSPLAT_NEAR_DIST2 (a cap stops a count)", who, cap);
    if (info && info->struct_size < sizeof(msplat_neighbour_info))
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: struct_size %u ends before tests (sizeof(msplat_neighbour_info) is %zu)", who, info->struct_size,
                    sizeof(msplat_neighbour_info));
    int rc;
    if ((rc = check_splat_bytes(ctx, who, "d_source", d_source, n, true))) return rc;
    if (info) {
        info->sources = info->queries = info->buckets = info->max_bucket = info->reserved = 0u;
        info->tests = 0ull;
    }
    if (n == 0) return MSPLAT_OK;
    if ((rc = check_splat_bytes(ctx, who, "d_query", d_query, n, true)) || (rc = check_values(ctx, who, d_values, n))) return rc;
    const uintptr_t v0 = (uintptr_t)d_values, v1 = v0 + 4 * n;
    for (const uint8_t* m : {d_source, d_query})
        if (m && (uintptr_t)m < v1 && (uintptr_t)m + n > v0)
            return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: d_values overlaps %s", who, m == d_source ? "d_source" : "d_query");
    if (max_tests == 0) max_tests = kNearDefaultTests;

    // the cells: edge h slightly above the radius (kNearEdge: DESIGN.md), buckets a power of two >= N >= the sources
    uint32_t buckets = ctx->near_buckets;
    if (buckets == 0)
        for (buckets = 1; buckets < n && buckets < kNearBucketsMax; buckets <<= 1) {}
    const uint32_t nchunks = div_up((uint64_t)buckets + 1, kNearChunk);       // (bucket `buckets` is empty: its start is the total)
    const bool own_queries = d_query != d_source;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    NearList src, qry;
    if ((rc = ensure_order_dev(ctx)) || (rc = near_reserve(ctx, 0, n, nchunks, src))) return rc;
    qry = src;
    if (own_queries && (rc = near_reserve(ctx, 1, n, nchunks, qry))) return rc;
    constexpr size_t kRows = (size_t)kGridCap + 1;
    constexpr size_t kRowBytes = kRows * sizeof(TestsRow) + 16;
    static_assert(kRowBytes == 16408, "the scratch size msplat.h states");
    if ((rc = buf_alloc(ctx, ctx->near_rows, kRowBytes))) return rc;
    TestsRow* tests_rows = (TestsRow*)ctx->near_rows.p;
    uint32_t* d_max_bucket = (uint32_t*)(tests_rows + kRows);
    const float4* pos = (const float4*)ctx->pos4.p;
    const uint32_t* order = ctx->store->reordered ? (const uint32_t*)ctx->store->order_dev.p : nullptr;
    hipStream_t s = ctx->stream;
    const dim3 block(kThreads), slots(grid_for(div_up(n, kThreads), ctx->grid_cap));

    NearCells g;
    g.inv_h = 1.0 / ((double)radius * kNearEdge);
    g.mask = buckets - 1u;
    HIP_TRY(ctx, hipMemsetAsync(d_max_bucket, 0, 4, s));
    HIP_TRY(ctx, near_list(ctx, src, d_source, n, g, nchunks, d_max_bucket));
    if (own_queries) HIP_TRY(ctx, near_list(ctx, qry, d_query, n, g, nchunks, nullptr));
    NearQueryArgs a;
    a.qent = qry.ent;
    a.nq = qry.total;
    a.ent = src.ent;
    a.start = src.start;
    a.g = g;
    a.r2 = r2;
    a.cap = cap;
    a.values = d_values;
    hipLaunchKernelGGL(neighbour_tests_kernel, slots, block, 0, s, a, tests_rows);
    hipLaunchKernelGGL(rows_finish_kernel<TestsRow>, dim3(1), block, 0, s, (const TestsRow*)tests_rows, (uint32_t)slots.x, tests_rows + kGridCap);
    if (hipGetLastError() != hipSuccess) return fail(ctx, MSPLAT_ERR_HIP, "%s: a kernel launch failed", who);
    uint32_t sources = 0, queries = 0, max_bucket = 0;
    TestsRow tests;
    tests.clear();
    HIP_TRY(ctx, hipMemcpyAsync(&sources, src.total, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&queries, qry.total, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&max_bucket, d_max_bucket, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&tests, tests_rows + kGridCap, sizeof(tests), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (info) {
        info->sources = sources;
        info->queries = queries;
        info->buckets = buckets;
        info->max_bucket = max_bucket;
        info->tests = tests.tests;
    }
    if (tests.tests > max_tests)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: the search would test up to %llu candidate pairs, more than max_tests = %llu (radius %g is large for "
                    "this cloud: %u queries, %u sources); d_values is untouched", who, (unsigned long long)tests.tests, (unsigned long long)max_tests,
                    (double)radius, queries, sources);

    hipLaunchKernelGGL(neighbour_fill_kernel, slots, block, 0, s, pos, order, d_query, (uint32_t)n, kind == MSPLAT_NEAR_COUNT ? 0.0f : INFINITY, d_values);
    if (kind == MSPLAT_NEAR_COUNT) hipLaunchKernelGGL(neighbour_search_kernel<kNearCount>, slots, block, 0, s, a);
    else hipLaunchKernelGGL(neighbour_search_kernel<kNearDist2>, slots, block, 0, s, a);
    if (hipGetLastError() != hipSuccess) return fail(ctx, MSPLAT_ERR_HIP, "%s: a kernel launch failed", who);
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return MSPLAT_OK;
}

int msplat_debug_set_neighbour_buckets(msplat_ctx* ctx, uint32_t buckets)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (buckets > kNearBucketsMax || (buckets & (buckets - 1u)) != 0)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_debug_set_neighbour_buckets: %u is not a power of two 1 .. 2^24 (0: automatic)", buckets);
    ctx->near_buckets = buckets;
    return MSPLAT_OK;
}
