// msplat_device.hip -- context management + C-ABI entry points of libmsplat.so that touch the GPU.
// Host-only scene code (Ply / GaussianCloud / matrices) lives in msplat_host.cpp.
//
// Drop-in boundary: include/msplat.h (replaces SplatRenderer::Init/Sort/Render,
// /root/reference/src/splatrenderer.cpp:50-343).  There is NO CPU fallback: without a HIP device
// msplat_create fails with MSPLAT_ERR_NO_DEVICE.
#include "msplat_kernels.hip.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/msplat.h"
#include "../../include/msplat_debug.h"
#include "../host/two_pass_controller.hpp"
#include "msplat_bin_order.h"

using namespace msplat;

namespace {

thread_local std::string g_last_error;

struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    bool frame_table = false;   // zeroed from inside every frame: clear_frame_tables restores it after a failed launch
};

// The uploaded cloud (read-only after upload).  Held by shared_ptr so that several contexts -- one per
// frame in flight, each with its own stream and per-frame buffers -- can render the same cloud
// (msplat_attach_cloud); a re-upload allocates a new store when the old one is still shared.
struct CloudStore {
    int device = 0;
    Buf pos4, recs;
    int storage = kStorageFp32;   // MSPLAT_STORAGE_* of the records, and their float4 count (cloud_f4; 1 for a point cloud)
    int F4 = 0;
    // spatial storage order (r4): slot j holds the splat uploaded as order_host[j]; one bounding box per kBoxSplats slots
    bool reordered = false;
    std::vector<uint32_t> order_host;
    Buf boxes;
    uint32_t nboxes = 0;
    // order_host on the device, for visibility_kernel: a mask speaks upload numbering.  Made by the first mask set on a reordered
    // store (ensure_order_dev), under mu: the contexts that share the store may belong to different threads
    Buf order_dev;
    std::mutex mu;
    ~CloudStore()
    {
        (void)hipSetDevice(device);
        if (pos4.p) (void)hipFree(pos4.p);
        if (recs.p) (void)hipFree(recs.p);
        if (boxes.p) (void)hipFree(boxes.p);
        if (order_dev.p) (void)hipFree(order_dev.p);
    }
};

inline uint32_t* words(const Buf& b) { return (uint32_t*)b.p; }

// A pinned host buffer that host bytes go through on their way to the device, and the event behind the latest copy out of it: the
// buffer is written again only after that copy has left it (stage_reserve / stage_send / stage_copy, msplat_edit.hip.inc)
struct StagingSlot {
    void* host = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
};

// The tables of the 8-bit radix passes (msplat_sort.hip.h), each with the numbers its kernels are launched with.
// HistTable: chunk-major histogram rows, uint32[256 * stride].  GroupTable (the scan-free path): per-group sums, one row of 256 per
// 32 chunks, behind `sup` rows of supergroup sums; `rows` of them in all (alloc_group_table)
struct HistTable { Buf buf; uint32_t stride = 0; };
struct GroupTable { Buf buf; uint32_t rows = 0, sup = 0; };

// The wide-digit 3-pass sort (r3, msplat_sort.hip.h ws_*): whether the uploaded cloud gets it and in what shape (plan_wide_sort), the
// histogram rows of up to 2048 digits per chunk, one group table per pass
struct WideSort {
    bool on = true;             // off: the four 8-bit passes (MSPLAT_SORT=lsd8, no lane-ordered LDS atomics, a refused LDS request)
    uint32_t items = 8;         // keys per thread of pass 0: 8 or 16
    uint32_t threads = 512;     // 256 (4 waves, 40 / 56 KB of LDS) for contexts that share the GPU with other frames
    uint32_t gshift = 4, gsum_words = 0;       // groups of 1 << gshift chunk rows; words of each group table
    Buf hist, gsum[3];
};

// clouds of at least this many splats are stored in Morton order (msplat_config.spatial_order = AUTO): below it a pass-0
// chunk is a large part of the cloud and there is nothing to skip
constexpr uint64_t kSpatialMinSplats = 1ull << 18;

}  // namespace

// msplat_config.async_submit (r4): msplat_sort and device-output msplat_render of the context return at once and their launches
// are issued by a worker thread that belongs to the context.  One frame is ~14 launches = ~55 us of host time; with several frames
// in flight issued round-robin from ONE thread the k-th context starts k x 55 us after the first, and a short block of frames
// (the driver times 20) pays that stagger at its start and again at its end.  With a worker per context the caller's thread only
// copies 38 floats per call.  Everything else on the context first waits for the worker to have ISSUED what is queued (never
// for the GPU); a failed queued call is reported by the next msplat_synchronize.
struct AsyncWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv, cv_idle;
    std::deque<std::function<int()>> q;
    bool busy = false, quit = false;
    int err_code = 0;
    std::string err_msg;
    // a queued call found that an EARLIER device-output frame overflowed the pair buffer (its own work was done): kept until
    // the next msplat_synchronize / msplat_stream_wait hands it to the caller (it used to be dropped)
    bool warn = false;
    std::string warn_msg;

    void run()
    {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return quit || !q.empty(); });
            if (q.empty()) return;              // quit, nothing left
            std::function<int()> t = std::move(q.front());
            q.pop_front();
            busy = true;
            lk.unlock();
            t();
            lk.lock();
            busy = false;
            if (q.empty()) cv_idle.notify_all();
        }
    }
    void post(std::function<int()> t)
    {
        std::lock_guard<std::mutex> lk(mu);
        q.push_back(std::move(t));
        cv.notify_one();
    }
    void drain()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv_idle.wait(lk, [&] { return q.empty() && !busy; });
    }
};

constexpr uint32_t kFusedMaxChunks = 1u << 20;     // scan-free passes up to this many chunk rows: with the two-level group tables (r3) a
                                               // prefix is <= nchunks / 128 + 34 rows, so every table qualifies (r2, one level: 8192 rows,
                                               // beyond that the radix_scan kernels)
constexpr uint32_t kGridCap = 256u * 8u;           // most workgroups of a grid-stride launch (grid_for): 256 CUs x 8

// Slots of a timing-event set (msplat_ctx::ev).  The compositor's pair is the exact dispatch begin / end of the kernel
// (hipExtLaunchKernelGGL); kEvPass2*: the second pass of a two-pass frame -- after the first compositor, after gate and projection,
// after binning -- and kEvComp2* its compositor's pair
enum EvSlot : int { kEvSortBegin = 0, kEvSortEnd = 1, kEvRenderBegin = 2, kEvProjected = 3, kEvBinned = 4, kEvRenderEnd = 5, kEvCompBegin = 6,
                    kEvCompEnd = 7, kEvPass2Begin = 8, kEvPass2Projected = 9, kEvPass2Binned = 10, kEvComp2Begin = 11, kEvComp2End = 12,
                    kEvSlots = 13 };

struct msplat_ctx {
    msplat_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int cu_partition = MSPLAT_CU_ALL;      // what the context's own stream really got (msplat_config.cu_partition)
    std::string err;

    // cloud
    uint64_t N = 0;
    bool full_sh = false;
    int cloud_storage = kStorageFp32;    // the store's MSPLAT_STORAGE_* (what project_kernel reads)
    int storage_cfg = kStorageFp32;      // msplat_set_cloud_storage: what the next splat upload stores
    bool has_cloud = false;
    bool has_sort = false;
    std::shared_ptr<CloudStore> store;   // owns pos4 / recs (possibly shared with other contexts)
    Buf pos4;       // view: float4[N]  (x, y, z, bound)  -- the reference's posVec (splatrenderer.cpp:106-111)
    Buf recs;       // view: padded AoS, 16 (full SH) or 8 float4 per splat, reference float offsets preserved
    hipEvent_t join_ev = nullptr;        // msplat_stream_wait
    Buf upload_over;                     // uint32: the f_rest failures an upload kernel counted (the uploads from device memory)
    float upload_kernel_ms = -1.0f;      // the latest upload kernel alone, with enable_timing (msplat_debug_upload_kernel_ms)
    // sort state
    Buf keyA, keyB, valA, valB;   // uint32[N]; final sorted result in keyA/valA
    HistTable hist;
    // scan-free path (msplat_sort.hip.h, radix_upsweep)
    GroupTable gsumS[2];    // sort passes alternate between the two: same rows, same sup (prepare_cloud_buffers)
    GroupTable gsumB1, gsumB2;      // binning: column pass / row pass
    // the wide sort, one visibility bit per splat, the visible set's minimum key per frame parity (counters, kCntMinKey)
    WideSort ws;
    bool wide_sort_cfg = true;  // what the context asked for; ws.on = what the uploaded cloud gets (plan_wide_sort)
    Buf vmask;
    Buf live_list, live_cnt;    // live bounding boxes of the latest Sort that ran box_cull_kernel (spatially ordered clouds)
    int spatial_mode = 0;       // msplat_config.spatial_order: 0 auto, 1 always, 2 never
    bool last_sort_listed = false;   // the latest Sort's pass 0 walked the listed boxes only
    FrameParams last_sort_fp{};
    // per-splat visibility (msplat_set_visibility / msplat_set_crop; msplat_cloud.hip.h, visibility_kernel): the position plane and
    // the cull boxes the context's Sorts read INSTEAD of the store's while a mask or a crop is set.  Allocated by the set calls (and
    // by an upload / attach under a crop), never by a Sort
    Buf vis_pos4, vis_boxes;    // float4[N]: x = NaN where hidden; CullBox[N / kBoxSplats] over the visible splats
    Buf vis_mask;               // uint8[N], upload numbering: the caller's mask, copied on the stream
    bool has_mask = false;
    int crop_shape = 0;         // MSPLAT_CROP_*; 0: no crop
    float crop_mat[16]{};
    bool vis_dirty = false;     // the plane is older than the mask, the crop or the cloud: the next Sort starts with visibility_kernel
    bool vis_sorted = false;    // the latest Sort read the context's plane and boxes
    StagingSlot vis_stage;      // what the latest host mask's copy reads
    // render-time overlay (msplat_set_overlay* / msplat_set_overlay_palette; msplat_overlay.hip.h): a class byte per splat and a palette
    // tint the projected records of the context's Renders.  Allocated by the set calls, never by a Render
    Buf ov_cls;                 // uint8[N], upload numbering: the caller's classes, copied on the stream
    Buf ov_slot;                // uint8[N], storage order (a store in Morton order only): overlay_classes_kernel, where overlay_dirty
    Buf ov_pal;                 // float4[kOverlayEntries]: the palette, a = 0 beyond the caller's count
    bool has_classes = false;
    bool overlay_dirty = false; // ov_slot is older than the classes or the store's order: resolved by the next overlaid Render
    uint32_t ov_count = 0;      // palette entries the caller set ...
    bool ov_tints = false;      // ... and whether one of them has a != 0
    StagingSlot ov_stage[2];    // what the latest host classes' / palette's copy reads
    Buf measure_rows;           // msplat_measure_cloud's scratch (msplat_select.hip.h): MeasureRow[kGridCap] partials, then the total; first use
    Buf value_hist;             // msplat_histogram_values' scratch (msplat_values.hip.h): uint32[4096] counts, ValueRow[kGridCap] partials, the total; first use
    // msplat_neighbour_values' scratch (msplat_neighbours.hip.h), first use; [0] the sources' list, [1] a query set's that is another array
    Buf near_cells[2];          // uint32: cnt[cells] | start[cells] | sums[chunks] | total, cells = chunks * 4096 > the buckets
    Buf near_ent[2];            // float4[N]: (x, y, z, bits of the upload index) in bucket order
    Buf near_rows;              // TestsRow[kGridCap] partials, the total, the fullest bucket
    uint32_t near_buckets = 0;  // msplat_debug_set_neighbour_buckets: the forced bucket count; 0: automatic
    uint32_t sort_parity = 0;
    bool tables_dirty = false;  // a launch failed: clear every self-cleaning table before the next frame
    // per-bin pair counts taken by the row pass's upsweep (r3): list offsets + work order (no kernel of their own)
    Buf bincnt;
    // (XCD-contiguous chunk ranges: on for the sort's downsweeps -- 6 M splats 196 -> 185 us, no change at 1 M -- and the row
    //  pass's downsweep -- 6 M / 4096^2 binning 347 -> 327 us: a column's chunks write adjacent runs of every row --, off for the
    //  column pass's downsweep, where they were measured slower: 453 -> 509 us.  Fixed since r4.)
    Buf heavy, heavy_flag;      // column pass: chunks with far more pairs than the others are split over several workgroups
    uint32_t render_parity = 0;
    bool scan_free = true;  // MSPLAT_SCAN_KERNELS=1 forces the 3-kernel (upsweep, scan, downsweep) passes
    uint32_t grid_cap = kGridCap;   // grid_for's limit; MSPLAT_GRID_CAP=1..2048 lowers it (debug switch: the chunk loops take several turns)
    Buf totals;     // uint32[256]  digit totals of the current radix pass (rows in binning pass 2)
    Buf totals1;    // uint32[256]  column totals of binning pass 1
    Buf counters;   // uint32[kCounterCount]: Counter, msplat_common.hip.h
    Buf queue;      // uint32[kQueueShards * kQueueStride]: the compositors' sharded work queue heads
    // render state
    uint64_t rank_cap = 0;      // draw-order ranks rec2d / rect / hist1 ... are sized for: N, or 2 N + 64 once msplat_render_stereo ran
    Buf rec2d;      // float4[3*N]
    Buf rect;       // uint32[N]
    Buf zq;         // uint32[N] quantised window depth per rank (msplat_set_depth_test), or its float bits (msplat_render_depth)
    int depth_bits = 0;
    int rop = 0;            // render-target emulation for the draw-order compositor (msplat_set_target_emulation)
    int target_mode = MSPLAT_TARGET_CLEAR;     // what a Render does with the target's contents (msplat_set_target_mode)
    // point-cloud mode: pos4 = positions, recs = float4 colours, sprite = float4 mip chain
    bool point_mode = false;
    Buf sprite;
    SpriteParams sprite_params{};
    Buf tile_start; // uint32[65537]
    Buf tile_order; // uint32[65536] bins by descending list length, then uint32[65536] = 0, 1, 2, ... (storage order), then uint32[65536]
                    // = the XCD-local order persistent waves walk (msplat_bin_order.h), built for bin_order_tx x bin_order_rows bins
    int bin_order_tx = 0, bin_order_rows = 0;     // 0 x 0: none yet
    StagingSlot bin_order_stage;             // what the latest upload of that table reads
    const uint32_t* comp_order = nullptr;    // msplat_debug_get_bin_order: the table of the latest compositor launch and its bins
    uint32_t comp_order_bins = 0;
    HistTable hist1;      // column pass
    Buf pairsA, pairsB;   // uint32[pair_cap]
    uint64_t pair_cap = 0;
    HistTable hist2;      // row pass
    Buf fb;         // internal framebuffer for host-output renders
    Buf fbz;        // ... and their depth plane (msplat_render_depth): float[W * H]
    Buf fbo;        // ... and the caller's occluder plane (msplat_render_occluded), staged once per call: float[W * H]
    Buf fb_ids, fb_idz;   // the planes of a host-output id frame (msplat_render_ids): uint32 / float[w * h] of its window
    Buf probe;      // uint32[8 * work items] compositor probe (msplat_set_tile_probe)
    bool probe_on = false;
    // device-output renders never synchronise: a pair-buffer overflow is left in host-mapped memory by the
    // binning kernel and picked up by the next call on the context (poll_async_overflow)
    uint32_t* h_flags = nullptr;   // host view of the kHostWordCount status words (HostWord, msplat_common.hip.h; host_word reads one)
    uint32_t* d_flags = nullptr;   // device view of the same words
    // band
    // owned bin rows: blocks of band_block rows starting at band_first, band_first + band_stride, ..., at most band_count
    // rows (0 = as many as the image has); banded == false: the whole image (msplat_set_band_layout)
    bool banded = false;
    int band_first = 0, band_block = 1, band_stride = 1, band_count = 0;
    bool band_cull = false;
    // last frame
    FrameParams last_fp{};
    bool has_render = false;
    // timing
    // per-stage hipEvent sets, recorded on every `timing_stride`-th call so that the event markers
    // (a few us of pipeline bubble each) do not perturb a throughput run; averaged by msplat_get_timings
    static constexpr int kEvSets = 32;
    hipEvent_t ev[kEvSets][kEvSlots]{};      // slots: EvSlot, above
    bool ev_ok = false;
    int timing_stride = 1;
    uint64_t sort_calls = 0, render_calls = 0;
    uint32_t sort_sets = 0, render_sets = 0;      // sets recorded since the last msplat_get_timings
    int cur_render_set = -1;
    bool comp_kernel_timed = false;
    uint32_t comp_kernel_sets_mask = 0;
    uint32_t two_pass_sets_mask = 0;         // timing sets recorded by two-pass frames
    // two-pass frame with occlusion feedback (msplat_occlusion.hip.h)
    Buf occ, occ_mask, occ_fin, occ_state, occ_live, occ_boxdead, occ_unf;
    Buf occ_zstate;                          // float[W * H]: the depth accumulator beside occ_state (allocated by the first two-pass depth frame)
    int two_pass_mode = MSPLAT_TWO_PASS_AUTO;
    TwoPassController two_pass;              // ... when to run one, and with what share in pass 1 (host/two_pass_controller.hpp)
    bool last_render_two_pass = false;
    uint32_t heavy_slots_launched = 0;       // msplat_debug_get_heavy_chunks: helper slots of the latest bin1_downsweep launch
    uint32_t comp_launch[4] = {0, 0, 0, 0};  // msplat_debug_get_compositor_launch: items, grid, ordered, kernel kind of the latest compositor launch
    uint64_t frames_two_pass = 0;

    std::unique_ptr<AsyncWorker> worker;     // msplat_config.async_submit
    bool atomic_rank = true;    // LDS atomics hand out ranks in lane order (probed at create)
    int comp_waves = 8192;      // compositor grid (persistent waves; measured best of 2k..8k); msplat_config.compositor_waves overrides
    bool comp_waves_auto = true;   // nobody chose a pool size: up to 20 k work items every item gets its own wave (r2: a wave
                                   // that pulls a second item pays an atomic + two dependent loads; 17.6 k items: -8 %)
    uint64_t device_bytes = 0;
    std::vector<Buf*> bufs;     // every member Buf that buf_alloc has allocated: what msplat_destroy frees, clear_frame_tables walks
};

namespace {

int fail(msplat_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (c) c->err = buf;
    return code;
}

// one host-mapped status word (HostWord, msplat_common.hip.h) as some earlier frame left it: a relaxed load, never a wait
inline uint32_t host_word(const msplat_ctx* c, HostWord w) { return __atomic_load_n(c->h_flags + w, __ATOMIC_RELAXED); }

// waits until the context's worker thread (if any) has issued everything queued; no-op on the worker itself
thread_local const msplat_ctx* g_on_worker_of = nullptr;
inline void drain_async(msplat_ctx* c)
{
    if (c && c->worker && g_on_worker_of != c) c->worker->drain();
}

#define HIP_TRY(c, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail((c), MSPLAT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                      \
    } while (0)

int buf_alloc(msplat_ctx* c, Buf& b, size_t bytes)
{
    if (b.p && b.bytes >= bytes) return MSPLAT_OK;
    if (b.p) {
        (void)hipFree(b.p);
        c->device_bytes -= b.bytes;
        b.p = nullptr;
        b.bytes = 0;
    }
    if (bytes == 0) bytes = 16;
    HIP_TRY(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    c->device_bytes += bytes;
    // a member of the context (not a caller's temporary, which the caller frees): noted once for msplat_destroy
    const char* at = reinterpret_cast<const char*>(&b);
    if (at >= reinterpret_cast<const char*>(c) && at < reinterpret_cast<const char*>(c + 1) &&
        std::find(c->bufs.begin(), c->bufs.end(), &b) == c->bufs.end())
        c->bufs.push_back(&b);
    return MSPLAT_OK;
}

void buf_free(msplat_ctx* c, Buf& b)
{
    if (b.p) {
        (void)hipFree(b.p);
        c->device_bytes -= b.bytes;
    }
    b.p = nullptr;
    b.bytes = 0;
}

inline uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

constexpr size_t kProbeWords = 8;                                           // per compositor work item
constexpr size_t kProbeBytes = (size_t)65536 * 8 * kProbeWords * sizeof(uint32_t);   // 256x256 bins x 4 quadrants x 2 halves

int grid_for(uint32_t nchunks, uint32_t cap)
{
    // grid-stride kernels: enough workgroups to fill 256 CUs x 8, never more than the chunk count (cap = msplat_ctx::grid_cap)
    return (int)std::max(1u, std::min(nchunks, cap));
}

// ---- run-time value -> template argument.  A launch that exists for several values of a template parameter is written ONCE, in a
// generic lambda that receives each value as a tag:  with_flag(ctx->full_sh, [&](auto SH) { ... kernel<SH.value> ... });
// A dispatcher instantiates the lambda for every value it lists, nested dispatchers for the cross product of their lists: a selection
// that is not a cross product names its combinations at the call site (the wide sort's upsweep) or leaves out the ones that do not
// exist with `if constexpr` (project_kernel's stores, the splat compositor's probe forms).
template <bool B> using flag_t = std::bool_constant<B>;
template <int V> using int_t = std::integral_constant<int, V>;

template <class F> inline void with_flag(bool v, F&& f)
{
    if (v) f(flag_t<true>{}); else f(flag_t<false>{});
}

// v out of a fixed list; a value that is not listed takes the last one
template <int V0, int... Vs, class F> inline void with_int(int v, F&& f)
{
    if constexpr (sizeof...(Vs) == 0) f(int_t<V0>{});
    else if (v == V0) f(int_t<V0>{});
    else with_int<Vs...>(v, f);
}

// The (keys per thread, threads) forms of the wide sort's kernels: the ONE list behind sort_impl's dispatch (with_ws_shape) and
// msplat_create's dynamic-LDS requests.  ws.items is 8 or 16 and ws.threads kWsThreads or kWsThreadsSmall (plan_wide_sort).
template <class F> inline void for_each_ws_shape(F&& f)
{
    f(int_t<8>{}, int_t<kWsThreads>{});
    f(int_t<16>{}, int_t<kWsThreads>{});
    f(int_t<8>{}, int_t<kWsThreadsSmall>{});
    f(int_t<16>{}, int_t<kWsThreadsSmall>{});
}
template <class F> inline void with_ws_shape(uint32_t items, uint32_t threads, F&& f)
{
    for_each_ws_shape([&](auto I, auto T) { if (items == (uint32_t)I.value && threads == (uint32_t)T.value) f(I, T); });
}

// exclusive scan of a chunk-major histogram table along the chunks.  The element count is only known on the device,
// so the variant is picked from the cloud size: up to 2 M splats (a few thousand chunk rows at most) the 16-workgroup
// version, beyond that one workgroup per digit.
void launch_scan(hipStream_t s, bool small, const HistTable& hist, const uint32_t* d_n, uint32_t n_static, uint32_t n_cap, uint32_t chunk,
                 uint32_t* totals)
{
    if (small)
        hipLaunchKernelGGL(radix_scan_small, dim3(kScanSmallBlocks), dim3(kThreads), 0, s, words(hist.buf), d_n, n_static, n_cap, chunk, totals);
    else
        hipLaunchKernelGGL(radix_scan, dim3(256), dim3(kThreads), 0, s, words(hist.buf), hist.stride, d_n, n_static, n_cap, chunk, totals);
}

// ---- The arguments of a sort pass, by name.  A member's initialiser is what a pass without that feature passes; a call site states
// what its pass has, and launch_radix_* / launch_ws_* spell the kernels' positional lists (msplat_sort.hip.h), once each.
struct PassIO {                                 // what both kinds of pass read and write
    const uint32_t *keys_in = nullptr, *vals_in = nullptr;
    const float4* pos = nullptr;                // pass 0: the keys come from the positions
    const uint32_t* d_n = nullptr;              // the element count on the device; nullptr: n_static
    uint32_t n_static = 0, n_cap = 0;
    uint32_t *keys_out = nullptr, *vals_out = nullptr, *d_count_out = nullptr;
    const FrameParams* fp = nullptr;
    LiveBoxes lb{nullptr, nullptr, 0u, 0u};     // pass 0 over the listed live boxes (list_live_boxes)
    // the sort's ping-pong buffers: (keyA, valA) -> (keyB, valB), or back
    void buffers(const msplat_ctx* c, bool from_b)
    {
        keys_in = words(from_b ? c->keyB : c->keyA);   vals_in = words(from_b ? c->valB : c->valA);
        keys_out = words(from_b ? c->keyA : c->keyB);  vals_out = words(from_b ? c->valA : c->valB);
    }
};

// one 8-bit pass, radix_upsweep + radix_downsweep
struct RadixPass : PassIO {
    int shift = 0;
    const HistTable* hist = nullptr;
    uint32_t* totals = nullptr;                 // digit totals: radix_scan*'s, or (totals_out) the scan-free downsweep's own
    // scan-free (`fused`): the upsweep accumulates into gsum and the downsweep reads it; gsum's sup travels either way.  gsum_zero: the
    // table the upsweep clears for its successor pass
    const GroupTable *gsum = nullptr, *gsum_zero = nullptr;
    bool fused = false;
    // MODE_PAIR, the binning's row pass: column totals in; row totals, bin counts, list offsets, work order and queue heads out
    const uint32_t* col_totals = nullptr;
    uint32_t *totals_out = nullptr, *bincnt = nullptr, *tile_start = nullptr, *tile_order = nullptr, *queue = nullptr;
    int ntiles = 0, do_order = 0;
};

template <int MODE, int ITEMS, bool BAND>
void launch_radix_upsweep(hipStream_t s, int grid, const RadixPass& a)
{
    hipLaunchKernelGGL((radix_upsweep<MODE, ITEMS, BAND>), dim3(grid), dim3(kThreads), 0, s, a.keys_in, a.pos, a.d_n, a.n_static, a.n_cap,
                       a.shift, words(a.hist->buf), a.hist->stride, a.fused ? words(a.gsum->buf) : nullptr,
                       a.gsum_zero ? words(a.gsum_zero->buf) : nullptr, a.gsum_zero ? a.gsum_zero->rows : 0u, *a.fp, a.col_totals, a.bincnt,
                       a.gsum ? a.gsum->sup : 0u, a.lb);
}
template <int MODE, bool HAS_VALUES, bool ATOMIC_RANK, int ITEMS, bool BAND>
void launch_radix_downsweep(hipStream_t s, int grid, const RadixPass& a)
{
    hipLaunchKernelGGL((radix_downsweep<MODE, HAS_VALUES, ATOMIC_RANK, ITEMS, BAND>), dim3(grid), dim3(kThreads), 0, s, a.keys_in, a.vals_in,
                       a.pos, a.d_n, a.n_static, a.n_cap, a.shift, (const uint32_t*)words(a.hist->buf), a.hist->stride,
                       (const uint32_t*)a.totals, a.keys_out, a.vals_out, a.d_count_out, a.col_totals,
                       a.fused ? (const uint32_t*)words(a.gsum->buf) : nullptr, a.totals_out, *a.fp, a.bincnt, a.tile_start, a.tile_order,
                       a.queue, a.ntiles, a.do_order, a.gsum ? a.gsum->sup : 0u, a.lb);
}

// one digit of the sort's 8-bit passes over `grid` chunks: upsweep, the scan unless the pass is scan-free, downsweep.  large: the chunks
// of clouds beyond 2 M splats (keys per thread: msplat_common.hip.h, kSortItems)
template <class Mode, class Band>
void issue_radix_pass(msplat_ctx* ctx, Mode, Band, bool large, int grid, const RadixPass& a)
{
    with_int<kSortItemsLarge, kSortItems>(large ? kSortItemsLarge : kSortItems, [&](auto IT) {
        launch_radix_upsweep<Mode::value, IT.value, Band::value>(ctx->stream, grid, a);
        if (!a.fused) launch_scan(ctx->stream, !large, *a.hist, a.d_n, a.n_static, a.n_cap, (uint32_t)kThreads * IT.value, a.totals);
        with_flag(ctx->atomic_rank, [&](auto AR) {
            launch_radix_downsweep<Mode::value, true, AR.value, IT.value, Band::value>(ctx->stream, grid, a);
        });
    });
}

// one pass of the wide sort, ws_upsweep + ws_downsweep.  The tables, their group shift and size are the context's WideSort's: pass p
// accumulates into gsum[p % 3] and clears its predecessor's
struct WsPass : PassIO {
    int pass = 0;
    // pass 0: the upsweep leaves the keys in raw_keys with one visibility bit per splat; the downsweep reads both (raw_keys as its keys_in)
    uint32_t* raw_keys = nullptr;
    unsigned long long* vmask = nullptr;
    uint32_t *minkey_cur = nullptr, *minkey_next = nullptr;
};

template <int CULL, int ITEMS, int THREADS>
void launch_ws_upsweep(hipStream_t s, int grid, const WideSort& w, const WsPass& a)
{
    hipLaunchKernelGGL((ws_upsweep<CULL, ITEMS, THREADS>), dim3(grid), dim3(THREADS), 0, s, a.keys_in, a.pos, a.raw_keys, a.vmask, a.d_n,
                       a.n_static, a.n_cap, a.pass, a.minkey_cur, a.minkey_next, words(w.hist), words(w.gsum[a.pass % 3]), (int)w.gshift,
                       words(w.gsum[(a.pass + 2) % 3]), w.gsum_words, *a.fp, a.lb);
}
template <bool CULL, int ITEMS, int THREADS>
void launch_ws_downsweep(hipStream_t s, int grid, const WideSort& w, const WsPass& a)
{
    hipLaunchKernelGGL((ws_downsweep<CULL, ITEMS, THREADS>), dim3(grid), dim3(THREADS), ws_downsweep_lds(ITEMS, THREADS), s,
                       CULL ? (const uint32_t*)a.raw_keys : a.keys_in, a.vals_in, (const unsigned long long*)a.vmask, a.d_n, a.n_static,
                       a.n_cap, a.pass, (const uint32_t*)a.minkey_cur, (const uint32_t*)words(w.hist),
                       (const uint32_t*)words(w.gsum[a.pass % 3]), (int)w.gshift, a.keys_out, a.vals_out, a.d_count_out, a.lb);
}

}  // namespace

extern "C" {

const char* msplat_version_string(void) { return "msplat 0.1 (gfx950, HIP)"; }

int msplat_tile_size(void) { return kBin; }

const char* msplat_last_error(const msplat_ctx* ctx)
{
    drain_async(const_cast<msplat_ctx*>(ctx));          // (a queued call may be writing the text)
    if (ctx) return ctx->err.c_str();
    return g_last_error.c_str();
}

int msplat_create(msplat_ctx** out, const msplat_config* cfg)
{
    if (!out) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_create: out is NULL");
    *out = nullptr;
    msplat_config c{};
    c.struct_size = sizeof(msplat_config);
    c.t_epsilon = -1.0f;
    if (cfg) {
        // the struct grows at its end: a caller built against an older header passes a shorter struct_size
        constexpr size_t kMinConfig = offsetof(msplat_config, rank_mode);      // (spatial_order, added in r4, defaults to AUTO too)
        if (cfg->struct_size < kMinConfig || cfg->struct_size > sizeof(msplat_config))
            return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_create: config struct_size %u not in [%zu, %zu]",
                        cfg->struct_size, kMinConfig, sizeof(msplat_config));
        memcpy(&c, cfg, cfg->struct_size);
        c.struct_size = sizeof(msplat_config);
    }
    if (c.rank_mode != MSPLAT_RANK_AUTO && c.rank_mode != MSPLAT_RANK_BALLOT)
        return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_create: bad rank_mode %d", c.rank_mode);
    if (c.fb_format < MSPLAT_FB_RGBA32F || c.fb_format > MSPLAT_FB_SRGB8_ALPHA8)
        return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_create: bad fb_format %d (MSPLAT_FB_RGBA32F .. MSPLAT_FB_SRGB8_ALPHA8)", c.fb_format);
    if (c.spatial_order < MSPLAT_SPATIAL_AUTO || c.spatial_order > MSPLAT_SPATIAL_OFF)
        return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_create: bad spatial_order %d", c.spatial_order);
    if (c.two_pass < MSPLAT_TWO_PASS_AUTO || c.two_pass > MSPLAT_TWO_PASS_OFF)
        return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_create: bad two_pass %d", c.two_pass);
    if (c.cu_partition < MSPLAT_CU_ALL || c.cu_partition > MSPLAT_CU_ODD)
        return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_create: bad cu_partition %d", c.cu_partition);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, MSPLAT_ERR_NO_DEVICE, "msplat_create: no HIP device (%s); there is no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (c.device < 0 || c.device >= ndev)
        return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_create: device %d out of range [0,%d)", c.device, ndev);
    msplat_ctx* ctx = new msplat_ctx;
    ctx->cfg = c;
    ctx->device = c.device;
    if (ctx->cfg.t_epsilon < 0.0f) ctx->cfg.t_epsilon = 1.0f / 16384.0f;
    ctx->two_pass_mode = c.two_pass;
    e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        delete ctx;
        return fail(nullptr, MSPLAT_ERR_NO_DEVICE, "hipSetDevice(%d): %s", c.device, hipGetErrorString(e));
    }
    if (c.stream) {
        ctx->stream = (hipStream_t)c.stream;
    } else {
        // cu_partition (r6): the stream runs on the even or the odd CU positions of every XCD.  Mask bit 8 c + x is CU c of XCD x, and a
        // set bit enables CU c in EVERY XCD (tools/ubench_cumask.hip): a partition by XCD does not exist.  Two of four frames in
        // flight per half: each stream's launches compete with one other stream's instead of three (sort and binning stages -27 %,
        // projection and compositor slower, the frame 3-5 % faster: EXPERIMENTS.md, "Two frames per half of the CUs").  Without the extension: every CU, as before.
        e = hipErrorNotSupported;
        if (c.cu_partition == MSPLAT_CU_EVEN || c.cu_partition == MSPLAT_CU_ODD) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount == 256) {
                uint32_t mask[8] = {0};
                for (int i = 0; i < 256; ++i)
                    if ((i / 8) % 2 == c.cu_partition - MSPLAT_CU_EVEN) mask[i / 32] |= 1u << (i % 32);
                e = hipExtStreamCreateWithCUMask(&ctx->stream, 8, mask);
                ctx->cu_partition = e == hipSuccess ? c.cu_partition : MSPLAT_CU_ALL;
            }
            if (e != hipSuccess) (void)hipGetLastError();
        }
        if (e != hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete ctx;
            return fail(nullptr, MSPLAT_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        ctx->own_stream = true;
    }
    if (c.enable_timing > 0) {
        bool ok = true;
        for (auto& set : ctx->ev)
            for (auto& ev : set) ok = ok && (hipEventCreate(&ev) == hipSuccess);
        ctx->ev_ok = ok;
        ctx->timing_stride = c.enable_timing;
    }
    int rc = buf_alloc(ctx, ctx->totals, 256 * sizeof(uint32_t));
    if (rc == MSPLAT_OK) rc = buf_alloc(ctx, ctx->counters, kCounterCount * sizeof(uint32_t));
    if (rc == MSPLAT_OK) rc = buf_alloc(ctx, ctx->totals1, 256 * sizeof(uint32_t));
    if (rc == MSPLAT_OK) rc = buf_alloc(ctx, ctx->queue, kQueueShards * kQueueStride * sizeof(uint32_t));
    ctx->queue.frame_table = ctx->bincnt.frame_table = true;
    if (rc == MSPLAT_OK) rc = buf_alloc(ctx, ctx->tile_start, (65536 + 1024 + 16) * sizeof(uint32_t));
    if (rc == MSPLAT_OK) rc = buf_alloc(ctx, ctx->bincnt, (65536 + 1024 + 16) * sizeof(uint32_t));
    if (rc == MSPLAT_OK && hipMemsetAsync(ctx->bincnt.p, 0, ctx->bincnt.bytes, ctx->stream) != hipSuccess) rc = MSPLAT_ERR_HIP;
    if (rc == MSPLAT_OK) rc = buf_alloc(ctx, ctx->tile_order, 3 * 65536 * sizeof(uint32_t));

    if (c.compositor_waves > 0) { ctx->comp_waves = std::max(64, (int)c.compositor_waves); ctx->comp_waves_auto = false; }
    if (rc == MSPLAT_OK) {
        if (hipHostMalloc((void**)&ctx->h_flags, kHostWordCount * sizeof(uint32_t), hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void**)&ctx->d_flags, ctx->h_flags, 0) != hipSuccess)
            rc = fail(ctx, MSPLAT_ERR_HIP, "msplat_create: cannot allocate the host-mapped status words");
        else
            std::memset(ctx->h_flags, 0, kHostWordCount * sizeof(uint32_t));
    }
    if (rc == MSPLAT_OK && hipMemsetAsync(ctx->counters.p, 0, kCounterCount * sizeof(uint32_t), ctx->stream) != hipSuccess)
        rc = MSPLAT_ERR_HIP;
    if (rc == MSPLAT_OK && hipMemsetAsync((uint32_t*)ctx->counters.p + kCntMinKey, 0xFF, 2 * sizeof(uint32_t), ctx->stream) != hipSuccess)
        rc = MSPLAT_ERR_HIP;      // minimum key of the visible set, one word per frame parity
    if (rc == MSPLAT_OK) {
        // feature probe: stable ranks straight from LDS atomics need lane-ordered ds_add_rtn
        uint32_t* bad = (uint32_t*)ctx->counters.p + kCntLdsProbe;
        hipLaunchKernelGGL(iota_kernel, dim3(65536 / kThreads), dim3(kThreads), 0, ctx->stream, (uint32_t*)ctx->tile_order.p + 65536);
        hipLaunchKernelGGL(lds_atomic_order_probe, dim3(64), dim3(kThreads), 0, ctx->stream, bad);
        uint32_t hbad = 1;
        if (hipMemcpyAsync(&hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = fail(ctx, MSPLAT_ERR_HIP, "LDS atomic order probe failed to run");
        ctx->atomic_rank = (hbad == 0) && c.rank_mode != MSPLAT_RANK_BALLOT;
        ctx->scan_free = getenv("MSPLAT_SCAN_KERNELS") == nullptr;
        // frames in flight: kernels that co-schedule well (msplat.h); AUTO and any stale padding value = one frame at a time
        ctx->ws.threads = c.frame_mode == MSPLAT_FRAMES_IN_FLIGHT ? (uint32_t)kWsThreadsSmall : (uint32_t)kWsThreads;
        if (const char* sk = getenv("MSPLAT_SORT")) ctx->wide_sort_cfg = std::string(sk) != "lsd8";
        // debug switch: fewer workgroups than chunks, so that the chunk loops of the sort's and the binning's kernels take several turns
        if (const char* gc = getenv("MSPLAT_GRID_CAP")) ctx->grid_cap = (uint32_t)std::min(std::max(atol(gc), 1L), (long)kGridCap);
        if (!ctx->atomic_rank) ctx->wide_sort_cfg = false;       // the wide kernels rank with lane-ordered LDS atomics only
        ctx->spatial_mode = c.spatial_order;
        if (ctx->wide_sort_cfg) {
            // ws_downsweep needs 72 / 104 KB of dynamic LDS with 512 threads (40 / 56 KB with 256).  The attribute belongs to
            // the function ON A DEVICE (a kernel object per device): it is requested once per device, with that device current
            // (a process-wide flag left devices 1.. of a msplat_group without it)
            static std::mutex lds_mu;
            static int lds_state[64];          // per device ordinal: 0 = not asked yet, 1 = granted, -1 = refused
            const int dslot = ctx->device & 63;
            std::lock_guard<std::mutex> lk(lds_mu);
            if (lds_state[dslot] == 0) lds_state[dslot] = [] {
                bool ok = true;
                auto want = [&](const void* f, size_t bytes) { ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess; };
                for_each_ws_shape([&](auto I, auto T) {
                    want(reinterpret_cast<const void*>(&ws_downsweep<true, I.value, T.value>), ws_downsweep_lds(I.value, T.value));
                    want(reinterpret_cast<const void*>(&ws_downsweep<false, I.value, T.value>), ws_downsweep_lds(I.value, T.value));
                });
                return ok ? 1 : -1;
            }();
            if (lds_state[dslot] < 0) { (void)hipGetLastError(); ctx->wide_sort_cfg = false; }
        }
    }
    if (rc != MSPLAT_OK) {
        std::string msg = ctx->err;
        msplat_destroy(ctx);
        g_last_error = msg;
        return rc;
    }
    if (c.async_submit != 0) {
        try {
            ctx->worker.reset(new AsyncWorker);
            AsyncWorker* w = ctx->worker.get();
            const msplat_ctx* self = ctx;
            const int dev = ctx->device;
            w->th = std::thread([w, self, dev] {
                (void)hipSetDevice(dev);
                g_on_worker_of = self;
                w->run();
            });
        } catch (const std::exception&) {
            ctx->worker.reset();          // no thread: the context simply issues its own launches
        }
    }
    *out = ctx;
    return MSPLAT_OK;
}

static void stage_free(StagingSlot& sl);      // (msplat_edit.hip.inc)

void msplat_destroy(msplat_ctx* ctx)
{
    if (!ctx) return;
    if (ctx->worker) {
        ctx->worker->drain();
        { std::lock_guard<std::mutex> lk(ctx->worker->mu); ctx->worker->quit = true; }
        ctx->worker->cv.notify_all();
        if (ctx->worker->th.joinable()) ctx->worker->th.join();
        ctx->worker.reset();
    }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->pos4 = Buf{};
    ctx->recs = Buf{};
    ctx->store.reset();
    if (ctx->join_ev) (void)hipEventDestroy(ctx->join_ev);
    if (ctx->h_flags) (void)hipHostFree(ctx->h_flags);
    for (StagingSlot* sl : {&ctx->bin_order_stage, &ctx->vis_stage, &ctx->ov_stage[0], &ctx->ov_stage[1]}) stage_free(*sl);
    for (Buf* b : ctx->bufs) buf_free(ctx, *b);
    if (ctx->ev_ok)
        for (auto& set : ctx->ev)
            for (auto& ev : set) (void)hipEventDestroy(ev);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

static int ensure_pair_capacity(msplat_ctx* ctx, uint64_t cap);

// A device-output render (msplat_render with out_is_device = 1) cannot report a pair-buffer overflow when it is
// issued: the count is only known on the device.  bin1_downsweep leaves the number of pairs the frame needed in
// host-mapped memory; every later msplat_sort / msplat_render / msplat_synchronize on the context looks at that
// word (a plain host load, no synchronisation), grows the buffer when the capacity is automatic, and reports
// MSPLAT_ERR_PAIR_OVERFLOW once: the frame that overflowed is missing splats in its last bin columns.
// Returns MSPLAT_OK when nothing is pending; `msg` receives the text the caller reports after doing its own work.
static int poll_async_overflow(msplat_ctx* ctx, std::string& msg)
{
    uint32_t need = host_word(ctx, kHostOverflowPairs);
    if (need == 0) return MSPLAT_OK;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        return fail(ctx, MSPLAT_ERR_HIP, "hipStreamSynchronize failed while handling a pair-buffer overflow");
    need = std::max(need, host_word(ctx, kHostOverflowPairs));     // a later frame may have needed more
    __atomic_store_n(ctx->h_flags + kHostOverflowPairs, 0u, __ATOMIC_RELAXED);
    const uint64_t old_cap = ctx->pair_cap;
    char buf[384];
    if (ctx->cfg.pair_capacity == 0 && (uint64_t)need + (need >> 2) + 1024 <= 0x7FFFFFFFull &&
        ensure_pair_capacity(ctx, (uint64_t)need + (need >> 2) + 1024) == MSPLAT_OK) {
        snprintf(buf, sizeof(buf), "an earlier device-output render overflowed the pair buffer (needed %u pairs, capacity "
                 "was %llu): that frame lacks splats in its last bin columns; capacity grown to %llu", need,
                 (unsigned long long)old_cap, (unsigned long long)ctx->pair_cap);
    } else {
        snprintf(buf, sizeof(buf), "an earlier device-output render overflowed the pair buffer (needed %u pairs, capacity "
                 "%llu%s): that frame lacks splats in its last bin columns", need, (unsigned long long)old_cap,
                 ctx->cfg.pair_capacity ? ", fixed by msplat_config.pair_capacity" : "");
    }
    msg = buf;
    return MSPLAT_ERR_PAIR_OVERFLOW;
}

// the overflow warning a queued call left behind (async_submit), once
static bool take_async_warning(msplat_ctx* ctx, std::string& msg)
{
    if (!ctx->worker) return false;
    std::lock_guard<std::mutex> lk(ctx->worker->mu);
    if (!ctx->worker->warn) return false;
    ctx->worker->warn = false;
    msg = ctx->worker->warn_msg;
    return true;
}

int msplat_synchronize(msplat_ctx* ctx)
{
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (ctx->worker && g_on_worker_of != ctx) {
        ctx->worker->drain();
        int code = 0;
        std::string msg;
        { std::lock_guard<std::mutex> lk(ctx->worker->mu); code = ctx->worker->err_code; msg = ctx->worker->err_msg; ctx->worker->err_code = 0; }
        if (code) {
            (void)hipSetDevice(ctx->device);
            (void)hipStreamSynchronize(ctx->stream);
            return fail(ctx, code, "a queued msplat_sort / msplat_render failed: %s", msg.c_str());
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::string msg;
    if (poll_async_overflow(ctx, msg) != MSPLAT_OK) return fail(ctx, MSPLAT_ERR_PAIR_OVERFLOW, "%s", msg.c_str());
    if (take_async_warning(ctx, msg)) return fail(ctx, MSPLAT_ERR_PAIR_OVERFLOW_EARLIER, "%s", msg.c_str());
    return MSPLAT_OK;
}

// per-work-item compositor counters for the following renders (performance analysis / bench statistics;
// costs a few clock reads per batch, so it is off by default)
int msplat_set_tile_probe(msplat_ctx* ctx, int enable)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (enable && !ctx->probe.p) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        int rc = buf_alloc(ctx, ctx->probe, kProbeBytes);
        if (rc) return rc;
    }
    ctx->probe_on = enable != 0;
    return MSPLAT_OK;
}

static int prepare_cloud_buffers(msplat_ctx* ctx, uint64_t n, bool full_sh, const std::shared_ptr<CloudStore>& share);

// Emulated depth buffer for subsequent renders (app.cpp:163 enables GL_DEPTH_TEST, which is live
// on targets with a depth attachment).  bits = 0: colour-only target, the default.
int msplat_set_depth_test(msplat_ctx* ctx, int depth_bits)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (depth_bits != 0 && depth_bits != 24 && depth_bits != 32)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_set_depth_test: depth_bits must be 0, 24 or 32 (got %d)", depth_bits);
    if (depth_bits != 0) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        int rc = buf_alloc(ctx, ctx->zq, std::max<uint64_t>(ctx->N, 1) * 4);
        if (rc) return rc;
    }
    ctx->depth_bits = depth_bits;
    return MSPLAT_OK;
}

// What the render target does to the running colour, for diffing against the GL app's own output (SURVEY 8a-12,
// src/app.cpp:1012-1020): MSPLAT_ROP_NONE = float accumulation, rounded once at the end (default, the colour-only fp32 FBO);
// MSPLAT_ROP_RGBA8 = the default back buffer (clamp to [0,1] + 8-bit unorm after every blend, GL 4.6 17.3.6);
// MSPLAT_ROP_RGBA16F = the --fp16 target (fp16 rounding after every blend).  Renders then walk every bin list in draw
// order without early termination (the draw-order compositor of msplat_set_depth_test, with or without a depth buffer).
int msplat_set_target_emulation(msplat_ctx* ctx, int rop)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (rop != MSPLAT_ROP_NONE && rop != MSPLAT_ROP_RGBA8 && rop != MSPLAT_ROP_RGBA16F)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_set_target_emulation: rop must be MSPLAT_ROP_NONE, _RGBA8 or _RGBA16F (got %d)", rop);
    if (rop != MSPLAT_ROP_NONE && ctx->cfg.fb_format == MSPLAT_FB_SRGB8_ALPHA8)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_set_target_emulation: the emulation rounds LINEAR values after every blend, an "
                    "MSPLAT_FB_SRGB8_ALPHA8 target holds sRGB-encoded ones: out of scope (use MSPLAT_FB_RGBA8)");
    if (rop != MSPLAT_ROP_NONE && ctx->point_mode)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_set_target_emulation: the point-cloud sprite compositor has no render-target "
                    "emulation (the context holds a point cloud)");
    if (rop != MSPLAT_ROP_NONE && ctx->target_mode != MSPLAT_TARGET_CLEAR)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_set_target_emulation: per-blend rounding over a loaded or premultiplied target is "
                    "not defined (msplat_set_target_mode is not MSPLAT_TARGET_CLEAR)");
    ctx->rop = rop;
    return MSPLAT_OK;
}

// What a Render does with the target's contents (include/msplat.h): CLEAR overwrites with (C, 1), PREMULTIPLIED writes the layer
// (C, 1 - T), LOAD blends the frame over the pixels the target holds.  Only the compositors' final stores differ
// (msplat_composite.hip.h, TM); a combination they are not instantiated for is refused here, at msplat_set_target_emulation, at the
// point uploads or -- the tile probe -- by the Render.
int msplat_set_target_mode(msplat_ctx* ctx, int32_t mode)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (mode != MSPLAT_TARGET_CLEAR && mode != MSPLAT_TARGET_LOAD && mode != MSPLAT_TARGET_PREMULTIPLIED)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_set_target_mode: mode must be MSPLAT_TARGET_CLEAR, _LOAD or _PREMULTIPLIED (got %d)", mode);
    if (mode != MSPLAT_TARGET_CLEAR && ctx->rop != MSPLAT_ROP_NONE)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_set_target_mode: per-blend rounding over a loaded or premultiplied target is not "
                    "defined (msplat_set_target_emulation is not MSPLAT_ROP_NONE)");
    if (mode != MSPLAT_TARGET_CLEAR && ctx->point_mode)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_set_target_mode: the point-cloud sprite compositor overwrites its target (the "
                    "context holds a point cloud)");
    ctx->target_mode = mode;
    return MSPLAT_OK;
}

int msplat_get_target_mode(const msplat_ctx* ctx) { return ctx ? ctx->target_mode : -1; }

// Frames in flight: `ctx` renders `owner`'s cloud (no copy).  Each context keeps its own stream and
// per-frame buffers, so consecutive frames issued round-robin over several contexts overlap on the GPU
// (one frame's latency-bound sort/binning launches fill the gaps of another frame's compositor).
int msplat_attach_cloud(msplat_ctx* ctx, msplat_ctx* owner)
{
    drain_async(ctx);
    drain_async(owner);
    if (!ctx || !owner) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_attach_cloud: NULL argument");
    if (ctx == owner) return MSPLAT_OK;
    if (!owner->has_cloud || !owner->store) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "msplat_attach_cloud: owner has no cloud");
    if (owner->device != ctx->device)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_attach_cloud: contexts are on different devices (%d, %d)",
                    ctx->device, owner->device);
    if (owner->point_mode && ctx->target_mode != MSPLAT_TARGET_CLEAR)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_attach_cloud: the owner holds a point cloud, and the sprite compositor overwrites "
                    "its target (msplat_set_target_mode is not MSPLAT_TARGET_CLEAR)");
    ctx->point_mode = owner->point_mode;
    int rc = prepare_cloud_buffers(ctx, owner->N, owner->full_sh, owner->store);
    if (rc) return rc;
    ctx->has_cloud = true;       // uploads are synchronous: the store is complete
    return MSPLAT_OK;
}

void* msplat_get_stream(msplat_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int msplat_get_fb_format(const msplat_ctx* ctx) { return ctx ? ctx->cfg.fb_format : -1; }


// Makes `stream` (a hipStream_t, NULL = the legacy default stream) wait for everything enqueued so far on
// the context's stream, without blocking the host.
int msplat_stream_wait(msplat_ctx* ctx, void* stream)
{
    drain_async(ctx);
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((hipStream_t)stream != ctx->stream) {
        if (!ctx->join_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->join_ev, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventRecord(ctx->join_ev, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent((hipStream_t)stream, ctx->join_ev, 0));
    }
    std::string msg;
    if (take_async_warning(ctx, msg)) return fail(ctx, MSPLAT_ERR_PAIR_OVERFLOW_EARLIER, "%s", msg.c_str());
    return MSPLAT_OK;
}

// The context's stream waits for `event` (a hipEvent_t recorded by the caller, e.g. after the consumer of a
// framebuffer that the next frame on this context will overwrite).
int msplat_wait_event(msplat_ctx* ctx, void* event)
{
    drain_async(ctx);
    if (!ctx || !event) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "msplat_wait_event: NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, (hipEvent_t)event, 0));
    return MSPLAT_OK;
}

#include "msplat_edit.hip.inc"
#include "msplat_upload.hip.inc"

#include "msplat_bands.hip.inc"

static int make_frame_params(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16],
                             const float viewport[4], const float nearFar[2], FrameParams& fp)
{
    if (!cameraMat || !projMat || !viewport || !nearFar)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL matrix/viewport argument");
    std::memset(&fp, 0, sizeof(fp));
    msplat_mat4_inverse(cameraMat, fp.view);               // splatrenderer.cpp:161 / :327
    msplat_mat4_mul(projMat, fp.view, fp.mvp);             // splatrenderer.cpp:175
    std::memcpy(fp.proj, projMat, 16 * sizeof(float));
    fp.eye[0] = cameraMat[12]; fp.eye[1] = cameraMat[13]; fp.eye[2] = cameraMat[14];   // :328
    fp.W = viewport[2];
    fp.H = viewport[3];
    fp.zn = nearFar[0];
    fp.zf = nearFar[1];
    fp.X0 = viewport[0] * (0.00001f * nearFar[0]);         // splat_vert.glsl:160
    fp.Y0 = viewport[1];
    fp.width = (int)viewport[2];
    fp.height = (int)viewport[3];
    if (fp.width < 1 || fp.height < 1 || fp.width > 8192 || fp.height > 8192)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "viewport %dx%d outside [1,8192]^2 (256x256 bins of 32 px)",
                    fp.width, fp.height);
    fp.tiles_x = (fp.width + kBin - 1) / kBin;
    const int rows_full = (fp.height + kBin - 1) / kBin;
    fp.banded = ctx->banded ? 1 : 0;
    fp.band_first = ctx->band_first;
    fp.band_block = ctx->band_block;
    fp.band_stride = ctx->band_stride;
    fp.band_inv_stride = 1.0f / (float)std::max(1, ctx->band_stride);
    fp.tiles_y = rows_full;
    if (ctx->banded) {           // owned rows below rows_full, at most band_count of them
        int owned = 0;
        if (rows_full > ctx->band_first) {
            const int d = rows_full - ctx->band_first, k = d / ctx->band_stride, j = d - k * ctx->band_stride;
            owned = k * ctx->band_block + std::min(j, ctx->band_block);
        }
        if (ctx->band_count > 0) owned = std::min(owned, ctx->band_count);
        fp.tiles_y = owned;
    }
    fp.full_sh = ctx->full_sh ? 1 : 0;
    fp.srgb = ctx->cfg.srgb ? 1 : 0;
    fp.t_eps = ctx->cfg.t_epsilon;
    fp.band_cull = (ctx->band_cull && ctx->banded && !ctx->point_mode) ? 1 : 0;   // points carry no footprint bound
    fp.depth_bits = ctx->depth_bits;
    fp.rop = ctx->rop;
    fp.views = 1;
    fp.rows_view = rows_full;
    fp.view_scale2 = view_scale2_of(fp.view);
    return MSPLAT_OK;
}

// The scan-free passes keep their tables clean for the NEXT frame from inside the frame (every group table is zeroed by a
// later kernel of the same frame, the bin counts by their consumer, the minimum-key words by the other parity's pass 0), so
// a frame whose launches did not all go out leaves them in an unknown state: after any launch error the context is marked
// dirty and the next msplat_sort restores every table with memsets before it issues its kernels.
static int clear_frame_tables(msplat_ctx* ctx)
{
    hipStream_t s = ctx->stream;
    for (Buf* b : ctx->bufs)        // (the group tables, the bin counts, the queue heads, the heavy-chunk lists)
        if (b->frame_table && b->p) HIP_TRY(ctx, hipMemsetAsync(b->p, 0, b->bytes, s));
    HIP_TRY(ctx, hipMemsetAsync((uint32_t*)ctx->counters.p + kCntMinKey, 0xFF, 2 * sizeof(uint32_t), s));
    ctx->tables_dirty = false;
    return MSPLAT_OK;
}

#include "msplat_visibility.hip.inc"
#include "msplat_overlay.hip.inc"
#include "msplat_compact.hip.inc"
#include "msplat_transform.hip.inc"
#include "msplat_append.hip.inc"
#include "msplat_adjust.hip.inc"
#include "msplat_download.hip.inc"

// box_cull_kernel over the store's boxes or (vis) the context's own, for list_live_boxes and msplat_debug_get_cull_boxes; returns
// its workgroups
static uint32_t launch_box_cull(msplat_ctx* ctx, const CloudStore* st, bool vis, const FrameParams& fp, uint32_t* list, uint32_t* cnt)
{
    const uint32_t wgs = div_up(st->nboxes, kBoxGroup);
    hipLaunchKernelGGL(box_cull_kernel, dim3(wgs), dim3(kBoxGroup), 0, ctx->stream, (const CullBox*)(vis ? ctx->vis_boxes.p : st->boxes.p),
                       st->nboxes, fp, list, cnt);
    return wgs;
}

// Chunk-level cull (msplat_common.hip.h, box_live): for a spatially ordered cloud of which an EARLIER frame saw less than 70 %
// (host-mapped V, read without synchronising; 0 = no frame yet) Sort starts with box_cull_kernel and pass 0 walks the listed
// live boxes only.  Either form gives the same visible set, keys and order; the choice only matters for speed: the extra launch
// costs ~4 us, which a view of the whole cloud (BASELINE configs[1]: V = 0.99 N) would pay for nothing.
static LiveBoxes list_live_boxes(msplat_ctx* ctx, const FrameParams& fp, uint32_t last_V)
{
    LiveBoxes lb{nullptr, nullptr, 0u, (uint32_t)ctx->N};
    ctx->last_sort_fp = fp;
    ctx->last_sort_listed = false;
    const CloudStore* st = ctx->store.get();
    if (!st || !st->reordered || !st->boxes.p || ctx->point_mode) return lb;
    if (last_V == 0u || (uint64_t)last_V * 10u >= ctx->N * 7u) return lb;
    lb.list = (const uint32_t*)ctx->live_list.p;
    lb.cnt = (const uint32_t*)ctx->live_cnt.p;
    lb.wgs = launch_box_cull(ctx, st, vis_active(ctx), fp, (uint32_t*)ctx->live_list.p, (uint32_t*)ctx->live_cnt.p);
    ctx->last_sort_listed = true;
    return lb;
}

struct FrameArgs {            // the caller's four arrays, copied: a queued call outlives them
    float cam[16], proj[16], vp[4], nf[2];
    bool load(const float* c, const float* p, const float* v, const float* n)
    {
        if (!c || !p || !v || !n) return false;
        std::memcpy(cam, c, sizeof(cam)); std::memcpy(proj, p, sizeof(proj)); std::memcpy(vp, v, sizeof(vp)); std::memcpy(nf, n, sizeof(nf));
        return true;
    }
};

// A frame's planes in the colour's memory space, each kind with one pitch: the depth plane it writes (msplat_render_depth; NULL: none)
// and the plane of window depths its splats are tested against (msplat_render_occluded; NULL: no test, read-only).  [1]: the second
// view's planes of two views in one chain, as d_out1 is its target.  Copied by value into a queued call
struct FramePlanes {
    float* depth[2] = {nullptr, nullptr};
    const float* occluder[2] = {nullptr, nullptr};
    size_t depth_pitch = 0, occluder_pitch = 0;
    bool any() const { return depth[0] || occluder[0]; }
    bool paired() const { return !depth[0] == !depth[1] && !occluder[0] == !occluder[1]; }
    FramePlanes view(int v) const { return {{depth[v]}, {occluder[v]}, depth_pitch, occluder_pitch}; }      // one view's, for a frame of its own
};

// "this frame goes to a draw-order compositor" (sprites, the emulated depth buffer, the target emulation), not to the front-to-back
// splat compositor: no work queue, no two passes, no two views in one chain, no planes
static bool draw_order_frame(const msplat_ctx* ctx) { return ctx->point_mode || ctx->depth_bits != 0 || ctx->rop != 0; }

// result of a queued call: the first real failure is kept for msplat_synchronize; MSPLAT_ERR_PAIR_OVERFLOW_EARLIER (a past frame
// was composited from truncated lists; the buffer has grown since) is kept as a warning for the next msplat_synchronize /
// msplat_stream_wait, which return it once
static int note_async_result(msplat_ctx* ctx, int rc)
{
    if (rc == MSPLAT_ERR_PAIR_OVERFLOW_EARLIER) {
        std::lock_guard<std::mutex> lk(ctx->worker->mu);
        ctx->worker->warn = true;
        ctx->worker->warn_msg = ctx->err;
    } else if (rc != MSPLAT_OK) {
        std::lock_guard<std::mutex> lk(ctx->worker->mu);
        if (ctx->worker->err_code == 0) { ctx->worker->err_code = rc; ctx->worker->err_msg = ctx->err; }
    }
    return rc;
}

// What every frame call checks first, in this order; `who` names the entry point in the messages, `missing` says what a Render
// lacks of its targets (NULL: nothing; a Sort has none and need not follow a Sort)
static int begin_frame(msplat_ctx* ctx, const char* who, bool render, const char* missing, const float cameraMat[16],
                       const float projMat[16], const float viewport[4], const float nearFar[2], FrameParams& fp)
{
    if (!ctx) return fail(nullptr, MSPLAT_ERR_INVALID_ARG, "ctx is NULL");
    if (!ctx->has_cloud) return fail(ctx, MSPLAT_ERR_NO_CLOUD, "%s: no cloud uploaded", who);
    if (render && !ctx->has_sort) return fail(ctx, MSPLAT_ERR_NO_SORT, "%s: msplat_sort has not been called", who);
    if (missing) return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s", who, missing);
    return make_frame_params(ctx, cameraMat, projMat, viewport, nearFar, fp);
}

extern "C++" {      // (templates)

// The async wrapper of msplat_sort / msplat_render / msplat_render_stereo: impl(cam0, proj0, cam1, proj1, viewport, nearFar) issues the
// frame (one view: cam1 / proj1 repeat cam0 / proj0).  On a context with a worker a call that hands nothing back to its caller
// (`deferrable`) is queued with copies of its arrays; any other call first waits until the worker has issued what is queued.
// (TWO_VIEWS is a template argument so that a one-view call copies and queues one set of arrays, as it always did)
template <bool TWO_VIEWS, class Impl>
static int submit_frame(msplat_ctx* ctx, bool deferrable, const float* cam0, const float* proj0, const float* cam1, const float* proj1,
                        const float* viewport, const float* nearFar, Impl impl)
{
    if (ctx && ctx->worker && g_on_worker_of != ctx) {
        if (deferrable) {
            FrameArgs a, b;
            if (!a.load(cam0, proj0, viewport, nearFar) || (TWO_VIEWS && !b.load(cam1, proj1, viewport, nearFar))) {
                ctx->worker->drain();           // (ctx->err is the worker's while it runs)
                return fail(ctx, MSPLAT_ERR_INVALID_ARG, "NULL matrix/viewport argument");
            }
            if constexpr (TWO_VIEWS)
                ctx->worker->post([ctx, a, b, impl] { return note_async_result(ctx, impl(a.cam, a.proj, b.cam, b.proj, a.vp, a.nf)); });
            else
                ctx->worker->post([ctx, a, impl] { return note_async_result(ctx, impl(a.cam, a.proj, a.cam, a.proj, a.vp, a.nf)); });
            return MSPLAT_OK;
        }
        ctx->worker->drain();           // a host image is filled before the call returns: nothing to defer
    }
    return impl(cam0, proj0, cam1, proj1, viewport, nearFar);
}

// A frame's work between the poll for an EARLIER device-output frame's pair overflow (the buffer grows; this frame is still done)
// and the report of that overflow, which follows work that succeeded
template <class Work>
static int with_pending_overflow(msplat_ctx* ctx, Work&& work)
{
    std::string pending_msg;
    const int pending = poll_async_overflow(ctx, pending_msg);
    if (pending == MSPLAT_ERR_HIP) return pending;
    const int rc = work();
    if (rc) return rc;
    if (pending) return fail(ctx, MSPLAT_ERR_PAIR_OVERFLOW_EARLIER, "%s", pending_msg.c_str());
    return MSPLAT_OK;
}

}  // extern "C++"

static int sort_impl(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2]);

int msplat_sort(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16],
                const float viewport[4], const float nearFar[2])
{
    return submit_frame<false>(ctx, true, cameraMat, projMat, cameraMat, projMat, viewport, nearFar,
                        [ctx](const float* cam, const float* proj, const float*, const float*, const float* vp, const float* nf) {
                            return sort_impl(ctx, cam, proj, vp, nf);
                        });
}

static int issue_sort(msplat_ctx* ctx, const FrameParams& fp);

static int sort_impl(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16],
                     const float viewport[4], const float nearFar[2])
{
    FrameParams fp;
    int rc = begin_frame(ctx, "msplat_sort", false, nullptr, cameraMat, projMat, viewport, nearFar, fp);
    if (rc) return rc;
    return with_pending_overflow(ctx, [&] { return issue_sort(ctx, fp); });     // the sort itself is still performed
}

// three passes of 10 + (8..11) + (8..11) key bits (msplat_sort.hip.h, ws_*): 6 launches.
// pass 0: positions -> raw keys + visibility bits in keyB / vmask -> (keyA, valA); pass 1: A -> B; pass 2: B -> A
static void issue_wide_sort(msplat_ctx* ctx, const FrameParams& fp)
{
    hipStream_t s = ctx->stream;
    const WideSort& w = ctx->ws;
    const uint32_t N = (uint32_t)ctx->N;
    uint32_t* counters = words(ctx->counters);
    // Passes 1 and 2 see only the V splats that survived the cull.  With 8192-key chunks and V << N (a band-culled rank of a
    // multi-GPU frame keeps 17 %, a camera inside a scene 40 %) they would run on ~100 workgroups: they take 4096-key chunks
    // when an EARLIER frame's V (host-mapped word, read without synchronising) was below 2 M.  Any choice is correct at any V.
    const uint32_t last_V = host_word(ctx, kHostV);
    const uint32_t items12 = (w.items == 16u && last_V != 0u && (uint64_t)last_V + (last_V >> 2) <= (2u << 20)) ? 8u : w.items;
    WsPass a;               // what the three passes share
    a.n_cap = N;  a.fp = &fp;
    a.minkey_cur = counters + kCntMinKey + (ctx->sort_parity & 1u);
    a.minkey_next = counters + kCntMinKey + ((ctx->sort_parity ^ 1u) & 1u);
    ctx->sort_parity ^= 1u;
    WsPass p0 = a;
    p0.pos = sort_positions(ctx);  p0.raw_keys = words(ctx->keyB);  p0.vmask = (unsigned long long*)ctx->vmask.p;  p0.n_static = N;
    p0.keys_out = words(ctx->keyA);  p0.vals_out = words(ctx->valA);  p0.d_count_out = counters + kCntV;
    p0.lb = list_live_boxes(ctx, fp, last_V);       // (launches box_cull_kernel when the view is a partial one)
    // pass 0 over listed boxes: fewer chunks than the cloud has, so 4096-key chunks keep the CUs covered (as for passes 1, 2)
    uint32_t items = p0.lb.list != nullptr ? 8u : w.items;
    int wgrid = grid_for(div_up(N, w.threads * items), ctx->grid_cap);
    auto upsweep = [&](auto CULL, const WsPass& p) {
        // The upsweeps have no order to keep.  One frame at a time and 4096-key chunks (up to 2 M splats): twice the threads per
        // chunk, half the keys per thread -- 241 workgroups of 16 waves instead of 8 at 1 M: sort 57.4 -> 55.7 us.  Not at 6 M
        // (158 -> 166 us) and not for frames in flight (-0.5 %): EXPERIMENTS.md, "The upsweeps keep no order".
        if (items == 8u && w.threads == (uint32_t)kWsThreads)
            launch_ws_upsweep<CULL.value, 4, 2 * kWsThreads>(s, wgrid, w, p);
        else
            with_ws_shape(items, w.threads, [&](auto I, auto T) { launch_ws_upsweep<CULL.value, I.value, T.value>(s, wgrid, w, p); });
    };
    auto downsweep = [&](auto CULL, const WsPass& p) {
        with_ws_shape(items, w.threads, [&](auto I, auto T) { launch_ws_downsweep<CULL.value, I.value, T.value>(s, wgrid, w, p); });
    };
    with_int<2, 1>(fp.band_cull ? 2 : 1, [&](auto CULL) { upsweep(CULL, p0); });
    downsweep(flag_t<true>{}, p0);
    items = items12;
    wgrid = grid_for(div_up(N, w.threads * items), ctx->grid_cap);
    a.d_n = counters + kCntV;
    for (a.pass = 1; a.pass < 3; ++a.pass) {
        a.buffers(ctx, a.pass == 2);
        upsweep(int_t<0>{}, a);
        downsweep(flag_t<false>{}, a);
    }
}

// the four 8-bit passes (MSPLAT_SORT=lsd8): scan-free, 2 launches each, while the chunk table is small, else upsweep + scan + downsweep
static void issue_lsd8_sort(msplat_ctx* ctx, const FrameParams& fp)
{
    const uint32_t N = (uint32_t)ctx->N;
    uint32_t* d_V = words(ctx->counters) + kCntV;
    // chunk size by cloud size (msplat_common.hip.h, kSortItems): 2048 keys up to 2 M splats, 4096 beyond
    const bool large = ctx->N > (2u << 20);
    const uint32_t nchunks = div_up(N, (uint32_t)kThreads * (large ? kSortItemsLarge : kSortItems));
    const int grid = grid_for(nchunks, ctx->grid_cap);
    RadixPass a;            // what the four passes share
    a.n_cap = N;  a.fp = &fp;
    a.hist = &ctx->hist;  a.totals = words(ctx->totals);  a.fused = ctx->scan_free && nchunks <= kFusedMaxChunks;
    // pass 0: cull + key fused into the first radix pass (presort_compute.glsl + byte 0 of the sort)
    RadixPass p0 = a;
    p0.pos = sort_positions(ctx);  p0.n_static = N;
    p0.keys_out = words(ctx->keyB);  p0.vals_out = words(ctx->valB);  p0.d_count_out = d_V;
    p0.gsum = &ctx->gsumS[0];  p0.gsum_zero = &ctx->gsumS[1];       // (gsum_zero always, scan-free or not: keeps both tables clean)
    p0.lb = list_live_boxes(ctx, fp, host_word(ctx, kHostV));
    // (r6: frames without the band-restricted cull -- every single-GPU frame -- run instantiations that leave its code out)
    with_flag(fp.band_cull != 0, [&](auto BAND) { issue_radix_pass(ctx, int_t<MODE_CULL>{}, BAND, large, grid, p0); });
    // passes 1..3 on the V survivors (V stays on the device; splatrenderer.cpp:195-204's readback is gone)
    a.d_n = d_V;
    for (int pass = 1; pass < 4; ++pass) {
        a.buffers(ctx, pass & 1);
        a.shift = pass * 8;
        a.gsum = &ctx->gsumS[pass & 1];  a.gsum_zero = &ctx->gsumS[(pass + 1) & 1];
        issue_radix_pass(ctx, int_t<MODE_KEYS>{}, flag_t<true>{}, large, grid, a);
    }
}

static int issue_sort(msplat_ctx* ctx, const FrameParams& fp)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (ctx->tables_dirty) {
        int rc = clear_frame_tables(ctx);
        if (rc) return rc;
    }
    const bool timed = ctx->ev_ok && (ctx->sort_calls++ % ctx->timing_stride) == 0;
    const int tset = (int)(ctx->sort_sets % msplat_ctx::kEvSets);
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev[tset][kEvSortBegin], s));
    // a mask or a crop: pass 0 and the box cull read the context's plane and boxes, rebuilt first when something changed
    ctx->vis_sorted = vis_active(ctx);
    if (ctx->vis_sorted && ctx->vis_dirty) launch_visibility(ctx);
    const bool wide = ctx->ws.on;
    if (wide) issue_wide_sort(ctx, fp);
    else issue_lsd8_sort(ctx, fp);
    if (timed) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev[tset][kEvSortEnd], s));
        ctx->sort_sets++;
    }
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        ctx->tables_dirty = ctx->vis_dirty = true;
        if (!wide) return fail(ctx, MSPLAT_ERR_HIP, "msplat_sort: a kernel launch failed");
        // e.g. the dynamic-LDS request was not honoured on this device: later frames take the four 8-bit passes, which
        // need no opt-in (this frame is lost; the tables are restored before the next one)
        ctx->ws.on = ctx->wide_sort_cfg = false;
        return fail(ctx, MSPLAT_ERR_HIP, "msplat_sort: a kernel launch of the three-pass sort failed (%s); the context falls back "
                    "to the 8-bit passes from the next frame on", hipGetErrorString(le));
    }
    ctx->has_sort = true;
    return MSPLAT_OK;
}

// Should this Render run as two passes (msplat_occlusion.hip.h), and with what share of the visible splats in pass 1?  The policy
// is host/two_pass_controller.hpp; here: what the context allows, the snapshot of the feedback words, the passes' buffers.
constexpr int kProjGridTwoPass = 4096;       // one-wave workgroups of the grid-stride forms of project_kernel (9 fit a CU)
static bool occlusion_plan(msplat_ctx* ctx, const FrameParams& fp, bool stereo, float& frac)
{
    const size_t nbins = (size_t)std::max(fp.tiles_x * fp.tiles_y, 0);
    // (scan_free: the chunk offset of pass 1's column pass exists in the scan-free form only; kOccSatMax: the table of unfinished bins)
    // (an overlaid frame is a one-pass frame: overlay_kernel tints the records of ONE projection over all ranks)
    const bool eligible = !stereo && !draw_order_frame(ctx) && !ctx->probe_on && ctx->scan_free && !overlay_active(ctx) &&
                          nbins != 0 && (fp.tiles_x + 1) * (fp.tiles_y + 1) <= kOccSatMax;
    const TwoPassFrame frame{ctx->two_pass_mode, eligible, ctx->cfg.frame_mode == MSPLAT_FRAMES_IN_FLIGHT, ctx->N, host_word(ctx, kHostV), nbins};
    const TwoPassFeedback fb{host_word(ctx, kHostPass1Pairs), host_word(ctx, kHostUnfinishedBins), host_word(ctx, kHostPass2Pairs),
                             host_word(ctx, kHostPass1Seq), host_word(ctx, kHostPass2Seq)};
    if (!ctx->two_pass.decide(frame, fb)) return false;
    if (buf_alloc(ctx, ctx->occ, kOccWordCount * sizeof(uint32_t)) || buf_alloc(ctx, ctx->occ_mask, (size_t)kOccSatMax * 2 + 64) ||
        buf_alloc(ctx, ctx->occ_fin, nbins * 16 + 64) || buf_alloc(ctx, ctx->occ_state, (size_t)fp.width * fp.height * 16 + 64) ||
        buf_alloc(ctx, ctx->occ_live, ((size_t)ctx->N + 64) * 4) || buf_alloc(ctx, ctx->occ_boxdead, 2048 * 4 + 64) ||
        buf_alloc(ctx, ctx->occ_unf, nbins * 4 + 64)) {
        ctx->err.clear();                        // (no memory for the extra buffers: the frame runs in one pass)
        return false;
    }
    ctx->two_pass.commit();                      // this frame's number
    frac = ctx->two_pass.share;
    return true;
}

// One Render's decision (occlusion_plan), taken ONCE per Render: the retries of a host-output frame whose pair buffer overflowed
// re-issue the chain with the same plan (every retry used to advance the controller).
struct RenderPlan {
    bool decided = false, two_pass = false;
    float frac = 0.0f;
};

// ---- one Render = a chain of launches on the context's stream.  r5: one function per stage and one per kind of chain, instead of
// r4's single 260-line launch_render with a lambda inside.  What the stages share: -------------------------------
struct RenderChain {
    msplat_ctx* ctx;
    const FrameParams& fp;
    hipStream_t s;
    bool stereo;                 // two views in one chain: ranks [0, V) and [V1, V1 + V), bin rows stacked
    uint32_t N;                  // rank-indexed launches cover this many ranks (the cloud; 2 N + 64 with two views)
    uint32_t *d_Vsort, *d_D, *d_overflow, *d_queue;
    uint32_t* d_Vframe;          // ranks the binning walks (written by project_kernel for two views)
    uint32_t* occ;               // two-pass frames: cut / counters (msplat_occlusion.hip.h)
    int ntiles;
    uint32_t cap;
    bool timed;
    int tset, pgrid;
    void *d_out, *d_out1;
    size_t pitch;
    bool async_overflow_flag;
    FramePlanes planes;          // device memory
    // the compositor's schedule, decided where the bins are ordered (issue_binning) and used by issue_compositor
    bool ordered = true;
    uint32_t comp_items = 0, comp_pool = 0;
    bool want_zw = false;        // an id frame: z_w per rank although the chain has no planes
    bool overlay = false;        // a Render with an active overlay: overlay_kernel behind the projection (never an id or a score frame)
};

// vertex + geometry stage.  mode: PROJ_PLAIN / PROJ_TWO_VIEWS (chosen from the chain), PROJ_PASS1 or PROJ_LISTED (two-pass frames)
static void issue_projection(RenderChain& rc, int mode, float occ_frac)
{
    msplat_ctx* ctx = rc.ctx;
    const FrameParams& fp = rc.fp;
    hipStream_t s = rc.s;
    uint32_t *d_Vsort = rc.d_Vsort, *occ = rc.occ;
    const int pgrid = rc.pgrid;
    if (ctx->point_mode) {
        hipLaunchKernelGGL(point_project_kernel, dim3(pgrid), dim3(kProjThreads), 0, s, (const uint32_t*)ctx->valA.p, rc.d_Vframe,
                           (const float4*)ctx->pos4.p, (const float4*)ctx->recs.p, fp, ctx->sprite_params,
                           (float4*)ctx->rec2d.p, (uint32_t*)ctx->rect.p, ctx->depth_bits ? (uint32_t*)ctx->zq.p : nullptr);
        return;
    }
    ProjParams pp = proj_params(fp);
    uint32_t* zq = (mode != PROJ_LISTED && ctx->depth_bits) ? (uint32_t*)ctx->zq.p : nullptr;
    if (rc.planes.any() || rc.want_zw) {
        // a depth frame, or one tested against an occluder plane: every projection of the frame leaves z_w = (float)(0.5 ndc.z + 0.5)
        // per rank -- quantise_depth's 32-bit form is that float's bits (one product by 0.5, exact, and one rounded sum)
        pp.depth_bits = 32;
        zq = (uint32_t*)ctx->zq.p;
    }
    auto project = [&](auto MODE, int grid, const uint32_t* dV, const ProjExtra& ex, const auto& v1) {
        with_flag(ctx->full_sh, [&](auto SH) {
            with_int<kStorageShQ8, kStorageShFp16, kStorageFp32>(ctx->cloud_storage, [&](auto ST) {
                if constexpr (ST.value == kStorageShQ8 && !SH.value) return;      // (no such store: prepare_cloud_buffers)
                else
                    hipLaunchKernelGGL((project_kernel<SH.value, MODE.value, ST.value>), dim3(grid), dim3(kProjThreads), 0, s,
                                       (const uint32_t*)ctx->valA.p, dV, (const float4*)ctx->recs.p, pp, (float4*)ctx->rec2d.p,
                                       (uint32_t*)ctx->rect.p, zq, ex, v1);
            });
        });
    };
    if (mode == PROJ_PASS1) {
        // (project_kernel's first pass computes the cut and leaves it in occ[kOccCut])
        const ProjExtra ex{nullptr, occ, nullptr, occ_frac};
        project(int_t<PROJ_PASS1>{}, std::min(pgrid, kProjGridTwoPass), (const uint32_t*)d_Vsort, ex, ProjNoView1{0});
    } else if (mode == PROJ_LISTED) {
        // the listed ranks behind the cut (occ[kOccListed] of them)
        const ProjExtra ex{ctx->d_flags ? ctx->d_flags + kHostListedRanks : (uint32_t*)nullptr, nullptr, (const uint32_t*)ctx->occ_live.p, 0.0f};
        project(int_t<PROJ_LISTED>{}, std::min(pgrid, kProjGridTwoPass), (const uint32_t*)(occ + kOccListed), ex, ProjNoView1{0});
    } else if (rc.stereo) {
        const ProjExtra ex{rc.d_Vframe, nullptr, nullptr, 0.0f};
        project(int_t<PROJ_TWO_VIEWS>{}, pgrid, (const uint32_t*)d_Vsort, ex, proj_view1(fp));
    } else {
        const ProjExtra ex{nullptr, nullptr, nullptr, 0.0f};
        project(int_t<PROJ_PLAIN>{}, pgrid, (const uint32_t*)d_Vsort, ex, ProjNoView1{0});
    }
    if (rc.overlay) launch_overlay(ctx, s, (const uint32_t*)d_Vsort, rc.N, rc.stereo);      // (a one-pass frame: occlusion_plan)
}

// bin lists over the current rectangles: column pass (bin1_*), row pass (radix_*<MODE_PAIR>), list offsets + work order.
// occ_pass: 0 one pass, 1 / 2 the passes of a two-pass frame; keep_overflow: second chain of a two-pass frame
static void issue_binning(RenderChain& rc, int keep_overflow, int occ_pass)
{
    msplat_ctx* ctx = rc.ctx;
    const FrameParams& fp = rc.fp;
    hipStream_t s = rc.s;
    const uint32_t N = rc.N, cap = rc.cap;
    const bool stereo = rc.stereo, async_overflow_flag = rc.async_overflow_flag;
    const int ntiles = rc.ntiles;
    uint32_t *d_Vsort = rc.d_Vsort, *d_D = rc.d_D, *d_overflow = rc.d_overflow, *d_queue = rc.d_queue, *occ = rc.occ, *d_Vframe = rc.d_Vframe;
    // second chain of a two-pass frame: the binning walks occ[kOccRanks2] ranks (V, or 0 when pass 1 left no bin unfinished)
    uint32_t* d_V = occ_pass == 2 ? occ + kOccRanks2 : d_Vframe;
    const uint32_t* d_first = occ_pass == 1 ? occ + kOccCut : nullptr;      // pass 1 bins the ranks from the cut on

    // pass 1: stable partition by tile column, enumerated from the rank-ordered rectangles
    uint32_t* totals1 = (uint32_t*)ctx->totals1.p;
    uint32_t* totals2 = (uint32_t*)ctx->totals.p;
    const uint32_t bchunk = (uint32_t)kBinChunk;
    const int g1 = grid_for(div_up(N, bchunk), ctx->grid_cap);
    // heavy chunks of the column pass (bin1_upsweep): list per frame parity, helper workgroups in front of the downsweep's grid
    uint32_t* hv_cur = (uint32_t*)ctx->heavy.p + (ctx->render_parity & 1u) * (1u + kHeavyCap);
    uint32_t* hv_next = (uint32_t*)ctx->heavy.p + ((ctx->render_parity ^ 1u) & 1u) * (1u + kHeavyCap);
    ctx->render_parity ^= 1u;
    // helper workgroups for as many split chunks as an EARLIER frame asked for (host-mapped word, read without synchronising),
    // with headroom; a frame that needs more runs its extra heavy chunks unsplit and the next launch adapts
    const uint32_t last_heavy = host_word(ctx, kHostHeavyChunks);
    const uint32_t heavy_slots = last_heavy != 0u ? std::min<uint32_t>(kHeavyCap, 2u * last_heavy + 8u) : 0u;
    const int nhelp = (int)(heavy_slots * (kHeavyParts - 1u));
    ctx->heavy_slots_launched = heavy_slots;
    // scan-free variants while the chunk tables are small; the row pass's size (D) is only known on the device, so
    // its choice uses the D of an EARLIER frame that the binning kernel left in host-mapped memory (0 = none yet);
    // either variant is correct at any size, the choice only matters for speed
    // (r2, one-level group tables: the column pass's table was scanned by a kernel from 4096 rows on; with two levels every
    //  table that fits the supergroup rows is scan-free)
    const bool fused1 = ctx->scan_free && div_up(N, bchunk) <= kFusedMaxChunks;
    const uint32_t last_D = host_word(ctx, kHostD);
    const bool fused2 = ctx->scan_free && last_D != 0u && div_up((uint64_t)last_D + (last_D >> 2), kPairChunk) <= kFusedMaxChunks &&
                        div_up(cap, kPairChunk) <= ctx->hist2.stride;                  // (the tables hold every chunk the capacity allows)
    uint32_t *gB1 = words(ctx->gsumB1.buf), *gB2 = words(ctx->gsumB2.buf);
    // column pass: groups of 8 consecutive chunks share an XCD (xcd_grouped): the seams between the runs neighbouring chunks write
    // merge in that XCD's L2.  Measured r4 (serial binning, groups of 0 / 2 / 4 / 8 / 16 / 32): 6 M / 4096^2 328 / 320 / 316 / 315 /
    // 315 / 313 us, scene-like 6 M 201 / 194 / 194 / 195, 1 M unchanged (57); the fully XCD-contiguous mapping of r3 was slower.
    const int xcdg = 8;
    const bool small = ctx->N <= (2u << 20);      // (launch_scan)
    // (bin1_upsweep also clears the row pass's group table: its consumer, the previous frame's row downsweep, is long done)
    hipLaunchKernelGGL(bin1_upsweep<kBinChunk>, dim3(g1), dim3(kThreads), 0, s, (const uint32_t*)ctx->rect.p, d_V,
                       words(ctx->hist1.buf), ctx->hist1.stride, d_overflow, fused1 ? gB1 : nullptr, gB2,
                       ctx->gsumB2.rows, hv_cur, hv_next, (uint8_t*)ctx->heavy_flag.p, heavy_slots, ctx->gsumB1.sup,
                       keep_overflow, d_first);
    if (!fused1)
        launch_scan(s, small, ctx->hist1, d_V, 0u, N, bchunk, totals1);
    with_flag(ctx->atomic_rank, [&](auto AR) {
        hipLaunchKernelGGL((bin1_downsweep<AR.value, kBinChunk>), dim3(g1 + nhelp), dim3(kThreads), 0, s,
                           (const uint32_t*)ctx->rect.p, d_V, (const uint32_t*)words(ctx->hist1.buf), ctx->hist1.stride,
                           (const uint32_t*)totals1, (uint32_t*)ctx->pairsA.p, cap, d_D, d_overflow, ctx->d_flags,
                           async_overflow_flag ? 1 : 0, fused1 ? (const uint32_t*)gB1 : nullptr, fused1 ? totals1 : nullptr,
                           xcdg, (const uint32_t*)hv_cur, (const uint8_t*)ctx->heavy_flag.p,
                           (uint32_t)nhelp, fp.tiles_x, ctx->gsumB1.sup, (const uint32_t*)d_Vsort,
                           (keep_overflow && ctx->d_flags) ? ctx->d_flags + kHostPass2Pairs : (uint32_t*)nullptr, ctx->two_pass.seq, d_first);
    });
    // pass 2: stable partition by tile row (one generic radix pass on the top byte); words become (tx<<24)|rank
    // The heaviest-first order of the bins only pays when every work item has its own wave (the hardware then starts the
    // waves in item order: 83 -> 97 us without it at config 2); persistent waves that pull items from the queue balance
    // themselves: they walk the bins in the XCD-local order (ensure_bin_order).
    const bool wave_comp = !draw_order_frame(ctx);
    const uint32_t comp_items = (uint32_t)ntiles * 4u;
    // (every item on its own wave up to 20 k items, 40 k for two views in one chain: BASELINE configs[4] has 2 x 17.6 k)
    const uint32_t comp_pool = (ctx->comp_waves_auto && comp_items <= (stereo ? 40960u : 20480u)) ? comp_items : (uint32_t)ctx->comp_waves;
    const bool ordered = !(wave_comp && comp_pool < comp_items);
    // r3: the upsweep of the row pass also counts the pairs per bin, and one extra workgroup of its downsweep turns the
    // counts into the list offsets (+ the heaviest-first order when it is wanted).  (r3-r5: contexts with frames in flight
    // searched the offsets in the partitioned array with a kernel of their own, 1 % faster then; equal in r6 under the CU halves
    // -- 6290 / 6298, 2478-2514 / 2485-2494, 1363-1403 / 1384-1403 frames/s at 1 M, 6 M, 6 M / 4096^2 -- and removed: one launch less.)
    const int g2 = grid_for(div_up(cap, kPairChunk), ctx->grid_cap);
    RadixPass a;
    a.keys_in = (const uint32_t*)ctx->pairsA.p;  a.keys_out = (uint32_t*)ctx->pairsB.p;
    a.d_n = d_D;  a.n_cap = cap;  a.shift = 24;  a.fp = &fp;
    a.hist = &ctx->hist2;  a.totals = totals2;  a.totals_out = fused2 ? totals2 : nullptr;
    a.gsum = &ctx->gsumB2;  a.gsum_zero = &ctx->gsumB1;  a.fused = fused2;
    a.col_totals = totals1;  a.bincnt = (uint32_t*)ctx->bincnt.p;  a.queue = d_queue;
    a.tile_start = (uint32_t*)ctx->tile_start.p;  a.tile_order = (uint32_t*)ctx->tile_order.p;  a.ntiles = ntiles;  a.do_order = (ordered ? 1 : 0) | 2;
    launch_radix_upsweep<MODE_PAIR, kSortItems, true>(s, g2, a);
    if (!fused2)
        launch_scan(s, small, ctx->hist2, d_D, 0u, cap, (uint32_t)kPairChunk, totals2);
    with_flag(ctx->atomic_rank, [&](auto AR) { launch_radix_downsweep<MODE_PAIR, false, AR.value, kSortItems, true>(s, g2 + 1, a); });
    rc.ordered = ordered;
    rc.comp_items = comp_items;
    rc.comp_pool = comp_pool;
}

// The XCD-local bin order (msplat_bin_order.h) for a grid of tiles_x x rows bins -- rows as the compositor indexes them: stacked for two
// views in one chain, owned virtual rows for a banded context -- at tile_order + 2 * 65536.  Built on the host and uploaded on the
// context's stream only when the geometry differs from the table's: a steady-state frame issues nothing.
static int ensure_bin_order(msplat_ctx* ctx, int tiles_x, int rows, hipStream_t s)
{
    if (ctx->bin_order_tx == tiles_x && ctx->bin_order_rows == rows) return MSPLAT_OK;
    int rc = stage_reserve(ctx, ctx->bin_order_stage, 65536 * sizeof(uint32_t));      // (the upload before this one read it long ago)
    if (rc) return rc;
    bin_order_xcd(tiles_x, rows, kBinBlockW, kBinBlockH, (uint32_t*)ctx->bin_order_stage.host);
    ctx->bin_order_tx = ctx->bin_order_rows = 0;
    if ((rc = stage_send(ctx, ctx->bin_order_stage, (uint32_t*)ctx->tile_order.p + 2 * 65536, (size_t)tiles_x * rows * sizeof(uint32_t), s))) return rc;
    ctx->bin_order_tx = tiles_x;
    ctx->bin_order_rows = rows;
    return MSPLAT_OK;
}

// fragment stage + blend over the bin lists: the splat compositor (front to back), the draw-order compositor of the emulations,
// or the sprite compositor.  ev_c0 / ev_c1: the timing set's slots for the kernel's dispatch begin / end
static int issue_compositor(RenderChain& rc, int occ_pass, int ev_c0, int ev_c1)
{
    msplat_ctx* ctx = rc.ctx;
    const FrameParams& fp = rc.fp;
    hipStream_t s = rc.s;
    const uint32_t cap = rc.cap, comp_items = rc.comp_items, comp_pool = rc.comp_pool;
    const bool stereo = rc.stereo, timed = rc.timed, ordered = rc.ordered;
    const int ntiles = rc.ntiles, tset = rc.tset;
    uint32_t *d_queue = rc.d_queue, *occ = rc.occ;
    void *d_out = rc.d_out, *d_out1 = rc.d_out1;
    const size_t pitch = rc.pitch;
    uint32_t* fin = occ_pass ? (uint32_t*)ctx->occ_fin.p : nullptr;
    float4* state = occ_pass ? (float4*)ctx->occ_state.p : nullptr;
    const uint32_t* d_nbins = occ_pass == 2 ? occ + kOccUnfinished : nullptr;      // second chain of a two-pass frame: the listed unfinished bins
    const FramePlanes& pl = rc.planes;
    const bool draw_order = draw_order_frame(ctx);
    // the target's pixel format (kFb* = MSPLAT_FB_*: msplat_create let nothing else in); only the kernels' load_px / store_px differ
    auto with_format = [&](auto&& f) { with_int<kFbF16, kFbUnorm8, kFbSrgb8, kFbF32>(ctx->cfg.fb_format, f); };

    // persistent compositor: a fixed pool of waves pulls (bin, quadrant) items; never more waves than items
    const int cgrid = std::min(ntiles * 4, ctx->comp_waves);     // work items = (bin, quadrant) (the draw-order compositors)
    // what msplat_debug_get_compositor_launch reports (host bookkeeping only).  The second pass of a two-pass frame keeps pass 1's
    // numbers: its item count (the unfinished bins) exists on the device alone, its grid is computed like pass 1's
    if (ntiles > 0 && occ_pass != 2) {
        ctx->comp_launch[0] = draw_order ? (uint32_t)ntiles * 4u : comp_items;
        ctx->comp_launch[1] = draw_order ? (uint32_t)cgrid : std::min(comp_items, comp_pool);
        ctx->comp_launch[2] = ordered ? 1u : 0u;
        ctx->comp_launch[3] = ctx->point_mode ? 2u : draw_order ? 1u : 0u;
        ctx->comp_order = (const uint32_t*)ctx->tile_order.p;      // (the splat compositor names its table below)
        ctx->comp_order_bins = (uint32_t)ntiles;
    }
    // (frames in flight: serialising the compositor launches of the contexts sharing a cloud with an event
    //  gate was measured r1 -- no gain over letting the hardware queues interleave them, dropped)
    if (ntiles > 0 && ctx->probe_on && ctx->probe.p && draw_order)
        // the draw-order compositors do not write the probe: leave zeros, not an earlier frame's counters
        HIP_TRY(ctx, hipMemsetAsync(ctx->probe.p, 0, (size_t)ntiles * 8 * kProbeWords * sizeof(uint32_t), s));
    if (ntiles > 0 && ctx->point_mode) {
        // sprites in draw order (optionally against the emulated depth buffer)
        const uint32_t* zqp = ctx->depth_bits ? (const uint32_t*)ctx->zq.p : nullptr;
        with_format([&](auto FMT) {
            hipLaunchKernelGGL(composite_points_kernel<FMT.value>, dim3(cgrid), dim3(kCompThreads), 0, s,
                               (const uint32_t*)ctx->tile_start.p, (const uint32_t*)ctx->pairsB.p,
                               (const float4*)ctx->rec2d.p, zqp, (const float4*)ctx->sprite.p, ctx->sprite_params, d_out,
                               pitch, fp, cap, (const uint32_t*)ctx->tile_order.p, d_queue, (uint32_t)ntiles * 4u);
        });
        ctx->comp_kernel_timed = false;
    } else if (ntiles > 0 && draw_order) {
        // emulated depth buffer: draw-order walk, no early termination
        with_format([&](auto FMT) {
            with_int<kTargetLoad, kTargetPremultiplied, kTargetClear>(ctx->target_mode, [&](auto TM) {
                hipLaunchKernelGGL((composite_depth_kernel<FMT.value, TM.value>), dim3(cgrid), dim3(kCompThreads), 0, s,
                                   (const uint32_t*)ctx->tile_start.p, (const uint32_t*)ctx->pairsB.p,
                                   (const float4*)ctx->rec2d.p, (const uint32_t*)ctx->zq.p, d_out, pitch, fp, cap,
                                   (const uint32_t*)ctx->tile_order.p, d_queue, (uint32_t)ntiles * 4u);
            });
        });
        ctx->comp_kernel_timed = false;
    } else if (ntiles > 0) {
        // on sampled frames the dominant kernel gets exact dispatch begin/end events (the plain stream
        // markers around the stages can be processed while the previous kernel is still draining)
        hipEvent_t e0 = timed ? ctx->ev[tset][ev_c0] : nullptr, e1 = timed ? ctx->ev[tset][ev_c1] : nullptr;
        uint32_t* probe = ctx->probe_on ? (uint32_t*)ctx->probe.p : nullptr;
        if (probe) HIP_TRY(ctx, hipMemsetAsync(probe, 0, (size_t)ntiles * 8 * kProbeWords * sizeof(uint32_t), s));
        const uint32_t* ts = (const uint32_t*)ctx->tile_start.p;
        const uint32_t* pb = (const uint32_t*)ctx->pairsB.p;
        const float4* r2 = (const float4*)ctx->rec2d.p;
        // persistent waves walk the XCD-local order; a probed frame walks storage order, so that probe slot i stays storage-order item i
        const bool xcd_order = !ordered && occ_pass != 2 && !probe;
        if (xcd_order) {
            const int rc_order = ensure_bin_order(ctx, fp.tiles_x, fp.tiles_y, s);
            if (rc_order != MSPLAT_OK) return rc_order;
        }
        const uint32_t* ord = occ_pass == 2 ? (const uint32_t*)ctx->occ_unf.p
                                            : (const uint32_t*)ctx->tile_order.p + (ordered ? 0 : xcd_order ? 2 * 65536 : 65536);
        if (occ_pass != 2) { ctx->comp_order = ord; ctx->comp_order_bins = (uint32_t)ntiles; }
        // wave issue priority by item number where the items are numbered heaviest-first (every item on its own wave); none for
        // persistent waves, whose items are not numbered by weight (r3, in storage order, 4 frames in flight: none / by item number / by list length
        // = 5.82 / 5.76 / 5.79 k frames/s, i.e. no effect there)
        const int prio_mode = ordered ? 1 : 0;
        const int grid = (int)std::min<uint32_t>(comp_items, comp_pool);
        const CompParams cp = comp_params(fp);
        const CompExtra ex{d_out1, fin, state, d_nbins, probe, (const float*)ctx->zq.p, pl.depth[0], pl.depth_pitch,
                           occ_pass ? (float*)ctx->occ_zstate.p : nullptr, pl.occluder[0], pl.occluder_pitch, pl.occluder[1], pl.depth[1]};
        const int prio = occ_pass == 2 ? 0 : prio_mode;
        auto composite = [&](auto OCC, auto TWO, auto PROBE, auto TM, auto DEPTH, auto ZTEST) {
            with_format([&](auto FMT) {
                hipExtLaunchKernelGGL((composite_kernel<FMT.value, OCC.value, TWO.value, PROBE.value, TM.value, DEPTH.value, ZTEST.value>),
                                      dim3(grid), dim3(kCompThreads), 0, s, e0, e1, 0, ts, pb, r2, d_out, pitch, cp, cap, ord, d_queue,
                                      comp_items, prio, ex);
            });
        };
        constexpr flag_t<true> yes{};
        constexpr flag_t<false> no{};
        // The forms that exist per format: (OCC, TWO_VIEWS) = one pass, either pass of a two-pass frame, or the one pass of two views in
        // one chain (occlusion_plan never chooses two passes for those); each per target mode; each of those with any set of planes --
        // or, for one pass without planes in MSPLAT_TARGET_CLEAR, with the probe (render_frame / plane_checks refuse it elsewhere)
        auto form = [&](auto OCC, auto TWO) {
            with_int<kTargetLoad, kTargetPremultiplied, kTargetClear>(ctx->target_mode, [&](auto TM) {
                if constexpr (OCC.value == 0 && TM.value == kTargetClear) {
                    if (probe && !pl.any()) return composite(OCC, TWO, yes, TM, no, no);
                }
                with_flag(!!pl.depth[0], [&](auto DEPTH) {
                    with_flag(!!pl.occluder[0], [&](auto ZTEST) { composite(OCC, TWO, no, TM, DEPTH, ZTEST); });
                });
            });
        };
        if (stereo) form(int_t<0>{}, yes);
        else with_int<1, 2, 0>(occ_pass, [&](auto OCC) { form(OCC, no); });
        ctx->comp_kernel_timed = timed;
    } else {
        ctx->comp_kernel_timed = false;
    }
    return MSPLAT_OK;
}

// between the passes of a two-pass frame: the map of unfinished bins, dead boxes, the gate over the ranks behind the cut
static void issue_occlusion_gate(RenderChain& rc)
{
    msplat_ctx* ctx = rc.ctx;
    const FrameParams& fp = rc.fp;
    hipStream_t s = rc.s;
    const uint32_t N = rc.N;
    uint32_t *d_Vsort = rc.d_Vsort, *d_D = rc.d_D, *occ = rc.occ;
    hipLaunchKernelGGL(occ_mask_kernel, dim3(1), dim3(kOccMaskThreads), 0, s, (const uint32_t*)ctx->occ_fin.p, fp.tiles_x, fp.tiles_y,
                       (uint16_t*)ctx->occ_mask.p, occ, (const uint32_t*)d_Vsort, (uint32_t*)ctx->occ_unf.p);
    // spatially ordered cloud: whole boxes of 256 stored splats are dropped before any centre is fetched.  (The STORE's boxes and
    // plane, also under a mask or a crop: its boxes hold the visible splats' too, a superset and so conservative, and the ranks the
    // gate looks up are visible splats, whose positions the context's plane keeps bit for bit.)
    const uint32_t nboxes = (ctx->store && ctx->store->reordered && ctx->store->boxes.p) ? ctx->store->nboxes : 0u;
    const uint32_t boxwords = ((nboxes + (uint32_t)kThreads - 1u) / (uint32_t)kThreads) * ((uint32_t)kThreads / 32u);
    const bool use_boxes = nboxes != 0u && boxwords <= 2048u && ctx->occ_boxdead.p != nullptr;
    if (use_boxes)
        hipLaunchKernelGGL(occ_box_kernel, dim3(div_up(nboxes, kThreads)), dim3(kThreads), 0, s, (const CullBox*)ctx->store->boxes.p,
                           nboxes, fp, (const uint16_t*)ctx->occ_mask.p, (uint32_t*)ctx->occ_boxdead.p);
    hipLaunchKernelGGL(occ_gate_kernel, dim3(std::max(1u, div_up(N, kOccGateRanks))), dim3(kThreads), 0, s, (const uint32_t*)ctx->valA.p,
                       (const uint32_t*)d_Vsort, occ, (const float4*)ctx->pos4.p, (uint32_t*)ctx->rect.p, fp,
                       (const uint16_t*)ctx->occ_mask.p, (uint32_t*)ctx->occ_live.p, ctx->d_flags, (const uint32_t*)d_D, ctx->two_pass.seq,
                       use_boxes ? (const uint32_t*)ctx->occ_boxdead.p : (const uint32_t*)nullptr, boxwords);
}

// d_out1: the second view's target of two in one chain (else NULL); plan: a host-output frame's, kept over its retries (else NULL);
// pl: the frame's planes in device memory
static int launch_render(msplat_ctx* ctx, const FrameParams& fp, void* d_out, void* d_out1, size_t pitch, bool async_overflow_flag,
                         RenderPlan* plan, const FramePlanes& pl)
{
    hipStream_t s = ctx->stream;
    const bool stereo = fp.views == 2;
    uint32_t* counters = (uint32_t*)ctx->counters.p;
    const uint32_t N = stereo ? (uint32_t)(2 * ctx->N + 64) : (uint32_t)ctx->N;
    RenderChain rc{ctx, fp, s, stereo, N, counters + kCntV, counters + kCntD, counters + kCntOverflow, (uint32_t*)ctx->queue.p,
                   stereo ? counters + kCntVframe2 : counters + kCntV, (uint32_t*)ctx->occ.p, fp.tiles_x * fp.tiles_y, (uint32_t)ctx->pair_cap,
                   false, 0, (int)std::max(1u, div_up(N, kProjThreads)), d_out, d_out1, pitch, async_overflow_flag, pl};
    // Two-pass frame with occlusion feedback (msplat_occlusion.hip.h): the nearest R1 splats first, then only what the bins
    // they did not saturate still need.  Same pixels; chosen once per Render (occlusion_plan).  The retries of a host-output
    // frame whose pair buffer overflowed reuse the plan AND count as the same Render: the sampling counter, the two-pass
    // statistics and the feedback's frame number advance once.
    RenderPlan local_plan;
    if (!plan) plan = &local_plan;
    const bool first_attempt = !plan->decided;
    if (first_attempt) {
        plan->two_pass = occlusion_plan(ctx, fp, stereo, plan->frac);
        plan->decided = true;
        ctx->render_calls++;
    }
    const bool two_pass = plan->two_pass;
    if (pl.any()) {
        // z_w per rank; (depth) the accumulator plane two passes hand over.  (A buffer that has to grow is freed first: hipFree waits for the
        // frames that still read it.)
        int arc = buf_alloc(ctx, ctx->zq, std::max<uint64_t>(std::max(ctx->rank_cap, ctx->N), 1) * 4);
        if (!arc && two_pass && pl.depth[0]) arc = buf_alloc(ctx, ctx->occ_zstate, (size_t)fp.width * fp.height * 4 + 64);
        if (arc) return arc;
    }
    const bool timed = rc.timed = ctx->ev_ok && ((ctx->render_calls - 1) % ctx->timing_stride) == 0;
    const int tset = rc.tset = (int)(ctx->render_sets % msplat_ctx::kEvSets);
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev[tset][kEvRenderBegin], s));
    rc.occ = (uint32_t*)ctx->occ.p;              // (allocated by occlusion_plan with a context's first two-pass frame)
    rc.overlay = overlay_active(ctx);

    // ---- the plain chain (also: both eyes in one chain, points, the emulations), or pass 1 of a two-pass frame ----
    issue_projection(rc, two_pass ? PROJ_PASS1 : PROJ_PLAIN, plan->frac);
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev[tset][kEvProjected], s));
    issue_binning(rc, 0, two_pass ? 1 : 0);
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev[tset][kEvBinned], s));
    int crc = issue_compositor(rc, two_pass ? 1 : 0, kEvCompBegin, kEvCompEnd);
    if (crc) return crc;
    if (two_pass) {
        // ---- pass 2: gate, the listed ranks, the bins pass 1 left unfinished ----
        if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev[tset][kEvPass2Begin], s));
        issue_occlusion_gate(rc);
        issue_projection(rc, PROJ_LISTED, 0.0f);
        if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev[tset][kEvPass2Projected], s));
        const bool timed1 = ctx->comp_kernel_timed;
        issue_binning(rc, 1, 2);
        if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev[tset][kEvPass2Binned], s));
        crc = issue_compositor(rc, 2, kEvComp2Begin, kEvComp2End);
        if (crc) return crc;
        ctx->comp_kernel_timed = ctx->comp_kernel_timed && timed1;
        if (first_attempt) ctx->frames_two_pass++;
    }
    ctx->last_render_two_pass = two_pass;
    if (timed) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev[tset][kEvRenderEnd], s));
        if (ctx->comp_kernel_timed) ctx->comp_kernel_sets_mask |= 1u << tset; else ctx->comp_kernel_sets_mask &= ~(1u << tset);
        if (two_pass) ctx->two_pass_sets_mask |= 1u << tset; else ctx->two_pass_sets_mask &= ~(1u << tset);
        ctx->render_sets++;
    }
    if (hipGetLastError() != hipSuccess) {
        ctx->tables_dirty = true;
        return fail(ctx, MSPLAT_ERR_HIP, "msplat_render: a kernel launch failed");
    }
    return MSPLAT_OK;
}

// rows of the target: 0 = tightly packed (`tight` bytes)
static int resolve_pitch(msplat_ctx* ctx, const char* who, const FrameParams& fp, uint64_t& pitch_bytes, size_t& tight)
{
    const size_t bpp = MSPLAT_FB_BYTES_PER_PIXEL(ctx->cfg.fb_format);
    tight = (size_t)fp.width * bpp;
    if (pitch_bytes == 0) pitch_bytes = tight;
    if (pitch_bytes < tight || pitch_bytes % bpp != 0)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: pitch %llu too small / misaligned for width %d of %zu-byte pixels (at least %zu, a multiple of %zu)",
                    who, (unsigned long long)pitch_bytes, fp.width, bpp, tight, bpp);
    return MSPLAT_OK;
}

// The rows of a host image that belong to the context, between the caller's buffer and the internal framebuffer: the whole image, or
// (band mode) only the owned bin rows -- as documented for msplat_set_band, so several bands can be assembled in one host image.
// `fb`: the internal plane (ctx->fb, or ctx->fbz for the depth plane of msplat_render_depth), rows of `tight` bytes
static int copy_host_rows(msplat_ctx* ctx, const FrameParams& fp, void* rgba, uint64_t pitch_bytes, const Buf& fb, size_t tight, bool to_host)
{
    auto copy = [&](int y0, int rows) {
        char* host = (char*)rgba + (size_t)y0 * pitch_bytes;
        char* dev = (char*)fb.p + (size_t)y0 * tight;
        return to_host ? hipMemcpy2D(host, pitch_bytes, dev, tight, tight, rows, hipMemcpyDeviceToHost)
                       : hipMemcpy2DAsync(dev, tight, host, pitch_bytes, tight, rows, hipMemcpyHostToDevice, ctx->stream);
    };
    if (!ctx->banded) {
        HIP_TRY(ctx, copy(0, fp.height));
        return MSPLAT_OK;
    }
    for (int vy = 0; vy < fp.tiles_y;) {
        const int y0 = band_real_row(fp, vy) * kBin;
        int run = 1;                  // consecutive owned rows travel in one copy
        while (vy + run < fp.tiles_y && band_real_row(fp, vy + run) == band_real_row(fp, vy) + run) ++run;
        vy += run;
        const int rows = std::min(kBin * run, fp.height - y0);
        if (rows <= 0) break;
        HIP_TRY(ctx, copy(y0, rows));
    }
    return MSPLAT_OK;
}

// host output: render into an internal device framebuffer, copy back, grow the pair buffer on overflow.
// pl.depth[0] (msplat_render_depth): a host plane of pl.depth_pitch bytes per row, filled the same way from ctx->fbz -- every attempt
// writes the whole internal plane, and the rows are copied after the one that did not overflow
// pl.occluder[0] (msplat_render_occluded): the caller's host plane, staged into ctx->fbo once -- it is only read, so a retry reuses it
static int render_to_host(msplat_ctx* ctx, const FrameParams& fp, void* rgba, uint64_t pitch_bytes, size_t tight, const FramePlanes& pl)
{
    int rc;
    if ((rc = buf_alloc(ctx, ctx->fb, tight * fp.height))) return rc;
    const size_t ztight = (size_t)fp.width * sizeof(float);
    FramePlanes staged{{}, {}, ztight, ztight};      // the internal planes the chain sees
    if (pl.depth[0]) {
        if ((rc = buf_alloc(ctx, ctx->fbz, ztight * fp.height))) return rc;
        staged.depth[0] = (float*)ctx->fbz.p;
    }
    if (pl.occluder[0]) {
        if ((rc = buf_alloc(ctx, ctx->fbo, ztight * fp.height))) return rc;
        if ((rc = copy_host_rows(ctx, fp, const_cast<float*>(pl.occluder[0]), pl.occluder_pitch, ctx->fbo, ztight, false))) return rc;
        staged.occluder[0] = (const float*)ctx->fbo.p;
    }
    RenderPlan plan;
    for (int attempt = 0; attempt < 6; ++attempt) {
        // MSPLAT_TARGET_LOAD: the caller's rows are the destination -- before EVERY attempt, because blending over the target is
        // not idempotent: a retry would otherwise run over the half-blended frame of the attempt that overflowed
        if (ctx->target_mode == MSPLAT_TARGET_LOAD && (rc = copy_host_rows(ctx, fp, rgba, pitch_bytes, ctx->fb, tight, false))) return rc;
        rc = launch_render(ctx, fp, ctx->fb.p, nullptr, tight, false, &plan, staged);
        if (rc) return rc;
        uint32_t cnt[4];
        HIP_TRY(ctx, hipMemcpyAsync(cnt, ctx->counters.p, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (cnt[kCntOverflow] == 0) {
            if ((rc = copy_host_rows(ctx, fp, rgba, pitch_bytes, ctx->fb, tight, true))) return rc;
            return pl.depth[0] ? copy_host_rows(ctx, fp, pl.depth[0], pl.depth_pitch, ctx->fbz, ztight, true) : MSPLAT_OK;
        }
        // overflow: the word holds the required pair count
        const uint64_t need = (uint64_t)cnt[kCntOverflow] + (cnt[kCntOverflow] >> 2) + 1024;
        if (ctx->cfg.pair_capacity != 0 || need > 0x7FFFFFFFull)
            return fail(ctx, MSPLAT_ERR_PAIR_OVERFLOW, "pair buffer too small: need %u, capacity %llu", cnt[kCntOverflow],
                        (unsigned long long)ctx->pair_cap);
        if ((rc = ensure_pair_capacity(ctx, need))) return rc;
    }
    return fail(ctx, MSPLAT_ERR_PAIR_OVERFLOW, "pair buffer could not be grown");
}

// what every Render does once its FrameParams and pitch stand (rgba1: the second view of two in one chain)
static int render_frame(msplat_ctx* ctx, const FrameParams& fp, void* rgba, void* rgba1, uint64_t pitch_bytes, size_t tight,
                        int out_is_device, const FramePlanes& pl)
{
    int rc;
    if ((rc = overlay_frame_checks(ctx))) return rc;
    ctx->last_fp = fp;
    if (ctx->tables_dirty && (rc = clear_frame_tables(ctx))) return rc;
    if (ctx->point_mode && !ctx->sprite.p && (rc = build_sprite(ctx, nullptr, 0, 0))) return rc;   // built-in sphere sprite
    // (no compositor instantiation counts per work item AND reads the target: refused, never rendered as MSPLAT_TARGET_CLEAR)
    if (ctx->target_mode != MSPLAT_TARGET_CLEAR && ctx->probe_on)
        return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "msplat_render: the tile probe (msplat_set_tile_probe) exists for MSPLAT_TARGET_CLEAR only");
    return with_pending_overflow(ctx, [&] {      // an EARLIER frame; this one is still rendered
        const int r = out_is_device ? launch_render(ctx, fp, rgba, rgba1, pitch_bytes, true, nullptr, pl)
                                    : render_to_host(ctx, fp, rgba, pitch_bytes, tight, pl);
        if (r == MSPLAT_OK) ctx->has_render = true;
        return r;
    });
}

// One kind of plane in the messages.  Both come from the front-to-back compositor -- the depth plane from its accumulators, the test
// from its inner loop -- so the draw-order compositors (sprites, depth test, target emulation) and the probe's instantiations have none
struct PlaneKind {
    const char* name;
    const char* why[4];          // refused: a point cloud, msplat_set_depth_test, msplat_set_target_emulation, the tile probe
};
static const PlaneKind kDepthPlane{"depth", {"the context holds a point cloud (the sprite compositor has no depth output)",
                                             "msplat_set_depth_test is on (the draw-order compositor has no depth output)",
                                             "msplat_set_target_emulation is not MSPLAT_ROP_NONE (the draw-order compositor has no depth output)",
                                             "the tile probe (msplat_set_tile_probe) has no instantiation with a depth output"}};
static const PlaneKind kOccluderPlane{"occluder", {"the context holds a point cloud (the sprite compositor has no occluder test)",
                                                   "msplat_set_depth_test is on (the draw-order compositor's emulated depth buffer starts at the clear value)",
                                                   "msplat_set_target_emulation is not MSPLAT_ROP_NONE (the draw-order compositor has no occluder test)",
                                                   "the tile probe (msplat_set_tile_probe) has no instantiation with an occluder test"}};

// What a frame checks for a plane it was given, once its FrameParams stand: the configurations without such an instantiation are
// refused, the plane's pitch resolved (0 = tight).  `who`: the entry point the messages name
static int plane_checks(msplat_ctx* ctx, const char* who, const FrameParams& fp, const PlaneKind& kind, size_t& pitch_bytes)
{
    const int cause = ctx->point_mode ? 0 : ctx->depth_bits != 0 ? 1 : ctx->rop != MSPLAT_ROP_NONE ? 2 : ctx->probe_on ? 3 : -1;
    if (cause >= 0) return fail(ctx, MSPLAT_ERR_UNSUPPORTED, "%s: %s", who, kind.why[cause]);
    const size_t ztight = (size_t)fp.width * sizeof(float);
    if (pitch_bytes == 0) pitch_bytes = ztight;
    if (pitch_bytes < ztight || pitch_bytes % sizeof(float) != 0)
        return fail(ctx, MSPLAT_ERR_INVALID_ARG, "%s: %s pitch %llu too small / misaligned for width %d", who, kind.name,
                    (unsigned long long)pitch_bytes, fp.width);
    return MSPLAT_OK;
}

// ... for the planes that are present: the depth plane first
static int plane_checks(msplat_ctx* ctx, const char* who, const FrameParams& fp, FramePlanes& pl)
{
    const int rc = pl.depth[0] ? plane_checks(ctx, who, fp, kDepthPlane, pl.depth_pitch) : MSPLAT_OK;
    return rc || !pl.occluder[0] ? rc : plane_checks(ctx, who, fp, kOccluderPlane, pl.occluder_pitch);
}

// who: the entry point the messages name (NULL: the one that takes exactly these planes)
static int render_impl(msplat_ctx* ctx, const char* who, const float cameraMat[16], const float projMat[16], const float viewport[4],
                       const float nearFar[2], void* rgba, uint64_t pitch_bytes, int out_is_device, FramePlanes pl)
{
    if (!who) who = pl.depth[0] ? "msplat_render_depth" : pl.occluder[0] ? "msplat_render_occluded" : "msplat_render";
    FrameParams fp;
    int rc = begin_frame(ctx, who, true, rgba ? nullptr : "rgba is NULL", cameraMat, projMat, viewport, nearFar, fp);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t tight = 0;
    if ((rc = resolve_pitch(ctx, who, fp, pitch_bytes, tight))) return rc;
    if ((rc = plane_checks(ctx, who, fp, pl))) return rc;
    return render_frame(ctx, fp, rgba, nullptr, pitch_bytes, tight, out_is_device, pl);
}

// The four one-view entry points (include/msplat.h) are one frame: a NULL plane degrades to the call without it.  Queued when the
// image stays on the device; the planes travel by value
static int submit_render(msplat_ctx* ctx, const char* who, const float cameraMat[16], const float projMat[16], const float viewport[4],
                         const float nearFar[2], void* rgba, uint64_t pitch_bytes, int out_is_device, FramePlanes pl)
{
    return submit_frame<false>(ctx, out_is_device && rgba, cameraMat, projMat, cameraMat, projMat, viewport, nearFar,
                        [=](const float* cam, const float* proj, const float*, const float*, const float* vp, const float* nf) {
                            return render_impl(ctx, who, cam, proj, vp, nf, rgba, pitch_bytes, out_is_device, pl);
                        });
}

int msplat_render(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16],
                  const float viewport[4], const float nearFar[2],
                  void* rgba, uint64_t pitch_bytes, int out_is_device)
{
    return submit_render(ctx, nullptr, cameraMat, projMat, viewport, nearFar, rgba, pitch_bytes, out_is_device, FramePlanes{});
}

// msplat_render plus a per-pixel depth plane
int msplat_render_depth(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4],
                        const float nearFar[2], void* rgba, uint64_t pitch_bytes, float* depth, uint64_t depth_pitch_bytes,
                        int out_is_device)
{
    return submit_render(ctx, nullptr, cameraMat, projMat, viewport, nearFar, rgba, pitch_bytes, out_is_device, {{depth}, {}, depth_pitch_bytes, 0});
}

// msplat_render with GL_LESS against a caller's plane of window depths
int msplat_render_occluded(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4],
                           const float nearFar[2], void* rgba, uint64_t pitch_bytes, const float* occluder,
                           uint64_t occluder_pitch_bytes, int out_is_device)
{
    return submit_render(ctx, nullptr, cameraMat, projMat, viewport, nearFar, rgba, pitch_bytes, out_is_device, {{}, {occluder}, 0, occluder_pitch_bytes});
}

// msplat_render_occluded and msplat_render_depth in one frame: the depth plane is blended over the occluder's values
int msplat_render_layers(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4],
                         const float nearFar[2], void* rgba, uint64_t pitch_bytes, float* depth, uint64_t depth_pitch_bytes,
                         const float* occluder, uint64_t occluder_pitch_bytes, int out_is_device)
{
    return submit_render(ctx, "msplat_render_layers", cameraMat, projMat, viewport, nearFar, rgba, pitch_bytes, out_is_device,
                         {{depth}, {occluder}, depth_pitch_bytes, occluder_pitch_bytes});
}

// buffers indexed by draw-order rank, for 2 N + 64 ranks (two views in one chain)
static int ensure_stereo_ranks(msplat_ctx* ctx)
{
    const uint64_t need = 2 * std::max<uint64_t>(ctx->N, 1) + 64;
    if (ctx->rank_cap >= need) return MSPLAT_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int rc;
    if ((rc = buf_alloc(ctx, ctx->rec2d, need * 48))) return rc;
    if ((rc = buf_alloc(ctx, ctx->rect, need * 4))) return rc;
    if ((rc = buf_alloc(ctx, ctx->heavy_flag, (size_t)div_up(need, kBinChunk) + 64))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->heavy_flag.p, 0, ctx->heavy_flag.bytes, ctx->stream));
    ctx->hist1.stride = std::max(1u, div_up(need, kBinChunk));
    if ((rc = buf_alloc(ctx, ctx->hist1.buf, (size_t)256 * ctx->hist1.stride * 4))) return rc;
    if ((rc = alloc_group_table(ctx, ctx->gsumB1, ctx->hist1.stride))) return rc;
    ctx->rank_cap = need;
    return MSPLAT_OK;
}

// Two views of ONE Sort (the reference's VR frame: Sort with the first eye, Render per eye -- src/app.cpp:603-607) as a single
// chain of launches: projection, binning and compositing each run once over both views' work instead of twice in a row (half
// the launches, twice the work per launch: 0.50 -> 0.44 ms at BASELINE configs[4]).  Per view the arithmetic, the bin lists and
// the pixels are exactly those of two msplat_render calls.  Falls back to those two calls for banded contexts, point clouds,
// depth-test / render-target emulation, clouds beyond 2^23 splats and viewports taller than 4096 (128 bin rows per view).
// pl: a depth plane and / or an occluder plane per eye, one pitch per kind (msplat_render_stereo_layers); the fallback is then
// msplat_render_layers view by view -- the same pixels and planes either way
static int render_stereo_impl(msplat_ctx* ctx, const char* who, const float cam0[16], const float proj0[16], const float cam1[16],
                              const float proj1[16], const float viewport[4], const float nearFar[2], void* rgba0, void* rgba1,
                              uint64_t pitch_bytes, int out_is_device, FramePlanes pl)
{
    FrameParams fp, fp1;
    const char* missing = !(rgba0 && rgba1) ? "a target is NULL"
                          : !pl.paired() ? "depth0 / depth1 are both given or both NULL, and so are occluder0 / occluder1" : nullptr;
    int rc = begin_frame(ctx, who, true, missing, cam0, proj0, viewport, nearFar, fp);
    if (!rc) rc = make_frame_params(ctx, cam1, proj1, viewport, nearFar, fp1);
    if (rc) return rc;
    const bool batched = !ctx->banded && !draw_order_frame(ctx) && ctx->N <= (1ull << 23) && 2 * fp.tiles_y <= 256 && out_is_device;
    if (!batched) {      // the plain form: one render per view (host targets are filled one after the other anyway)
        const char* who1 = pl.any() ? who : nullptr;     // (the plain stereo call's views have always spoken as msplat_render)
        rc = render_impl(ctx, who1, cam0, proj0, viewport, nearFar, rgba0, pitch_bytes, out_is_device, pl.view(0));
        if (rc && rc != MSPLAT_ERR_PAIR_OVERFLOW_EARLIER) return rc;
        const int rc1 = render_impl(ctx, who1, cam1, proj1, viewport, nearFar, rgba1, pitch_bytes, out_is_device, pl.view(1));
        return rc1 ? rc1 : rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t tight = 0;
    if ((rc = resolve_pitch(ctx, who, fp, pitch_bytes, tight))) return rc;
    if ((rc = plane_checks(ctx, who, fp, pl))) return rc;
    if ((rc = ensure_stereo_ranks(ctx))) return rc;
    fp.views = 2;
    fp.rows_view = fp.tiles_y;
    fp.tiles_y = 2 * fp.rows_view;
    std::memcpy(fp.view1, fp1.view, sizeof(fp.view1));
    std::memcpy(fp.proj1, fp1.proj, sizeof(fp.proj1));
    std::memcpy(fp.eye1, fp1.eye, sizeof(fp.eye1));
    return render_frame(ctx, fp, rgba0, rgba1, pitch_bytes, tight, 1, pl);
}

// The two two-view entry points (include/msplat.h) are one frame too.  Half-given pairs of planes are refused at once, not queued
static int submit_render_stereo(msplat_ctx* ctx, const char* who, const float cameraMat0[16], const float projMat0[16],
                                const float cameraMat1[16], const float projMat1[16], const float viewport[4], const float nearFar[2],
                                void* rgba0, void* rgba1, uint64_t pitch_bytes, int out_is_device, FramePlanes pl)
{
    return submit_frame<true>(ctx, out_is_device && rgba0 && rgba1 && pl.paired(), cameraMat0, projMat0, cameraMat1, projMat1, viewport, nearFar,
                        [=](const float* cam0, const float* proj0, const float* cam1, const float* proj1, const float* vp, const float* nf) {
                            return render_stereo_impl(ctx, who, cam0, proj0, cam1, proj1, vp, nf, rgba0, rgba1, pitch_bytes, out_is_device, pl);
                        });
}

int msplat_render_stereo(msplat_ctx* ctx, const float cameraMat0[16], const float projMat0[16], const float cameraMat1[16],
                         const float projMat1[16], const float viewport[4], const float nearFar[2], void* rgba0, void* rgba1,
                         uint64_t pitch_bytes, int out_is_device)
{
    return submit_render_stereo(ctx, "msplat_render_stereo", cameraMat0, projMat0, cameraMat1, projMat1, viewport, nearFar, rgba0, rgba1,
                                pitch_bytes, out_is_device, FramePlanes{});
}

int msplat_render_stereo_layers(msplat_ctx* ctx, const float cameraMat0[16], const float projMat0[16], const float cameraMat1[16],
                                const float projMat1[16], const float viewport[4], const float nearFar[2], void* rgba0, void* rgba1,
                                uint64_t pitch_bytes, float* depth0, float* depth1, uint64_t depth_pitch_bytes, const float* occluder0,
                                const float* occluder1, uint64_t occluder_pitch_bytes, int out_is_device)
{
    return submit_render_stereo(ctx, "msplat_render_stereo_layers", cameraMat0, projMat0, cameraMat1, projMat1, viewport, nearFar, rgba0, rgba1,
                                pitch_bytes, out_is_device, {{depth0, depth1}, {occluder0, occluder1}, depth_pitch_bytes, occluder_pitch_bytes});
}

#include "msplat_ids.hip.inc"
#include "msplat_scores.hip.inc"
#include "msplat_select.hip.inc"
#include "msplat_values.hip.inc"
#include "msplat_neighbours.hip.inc"

#include "msplat_getters.hip.inc"

}  // extern "C"
