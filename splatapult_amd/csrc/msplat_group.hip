// msplat_group.hip -- single-process multi-GPU rendering behind the C ABI (include/msplat.h, msplat_group_*).
//
// The reference is ONE single-threaded C++ process that calls SplatRenderer::Sort / Render once per frame
// (/root/reference/src/sdl_main.cpp:49-204, src/app.cpp:1067-1068).  A maintainer who wants the frame spread over the
// GPUs of a node keeps that shape: one msplat_group = one context per device, the cloud replicated, the screen's bin rows
// partitioned over the devices, msplat_group_sort / msplat_group_render with the arguments of
// msplat_sort / msplat_render.  The only exchange step is the row gather, and it is zero-copy where the hardware allows:
// device i's compositor stores its rows STRAIGHT into device 0's framebuffer through the peer mapping
// (hipDeviceEnablePeerAccess: every band travels over its own direct xGMI link, 7 links into device 0 concurrently, no
// ring), else its rows are staged locally and moved with one hipMemcpy2DAsync per run of consecutive rows.
//
// r5: the same gather over RCCL (the north star's "RCCL over xGMI only for the final row gather"), for both process shapes:
//   msplat_band_exchange       one process per GPU (the caller owns the ncclComm_t, e.g. made with ncclCommInitRank): rank `root`
//                              posts one ncclRecv per run of foreign bin rows straight into its framebuffer, the owners ncclSend
//                              their runs from where the compositor left them -- one ncclGroupStart/End, no pack / staging;
//   MSPLAT_EXCHANGE_RCCL       this file's one-process group with communicators from ncclCommInitAll.
// librccl is resolved with dlopen at the first use (the copy already in the process, e.g. PyTorch's, else /opt/rocm's): the
// library has no link-time dependency on it and loads on a box without RCCL.
//
// Host side: launching ~12 kernels on each of 8 devices from one thread costs more host time than the frame lasts on the
// GPUs, so every device beyond the first has a worker thread that issues its context's calls; the caller's thread drives
// device 0 and then waits for the workers to have ISSUED their work (the GPUs keep running asynchronously; device 0's
// stream is made to wait for the others' streams, so "synchronise device 0's stream" = "the frame is complete").
// Uses only the public C ABI of the single-device library plus HIP runtime calls.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/msplat.h"
#include "../../include/msplat_debug.h"

namespace {

struct Worker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> task;
    bool has_task = false, done = true, quit = false;
    int rc = MSPLAT_OK;

    void run()
    {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return has_task || quit; });
            if (quit) return;
            std::function<int()> t = std::move(task);
            has_task = false;
            lk.unlock();
            const int r = t();
            lk.lock();
            rc = r;
            done = true;
            cv.notify_all();
        }
    }
    void post(std::function<int()> t)
    {
        std::lock_guard<std::mutex> lk(mu);
        task = std::move(t);
        has_task = true;
        done = false;
        cv.notify_all();
    }
    int wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done; });
        return rc;
    }
};

// ---- RCCL, resolved at run time --------------------------------------------------------------------------------------------
// (signatures: /opt/rocm/include/rccl/rccl.h:187-260,700-722,923-933; ncclUint8 = 1, ncclSuccess = 0)
struct Rccl {
    void* lib = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string why;             // why it is not available
    bool ok() const { return lib != nullptr; }
};

const Rccl& rccl()
{
    static Rccl r = [] {
        Rccl x;
        void* h = nullptr;
        // the copy the process already uses (its communicators belong to THAT copy), then the system's
        // (MSPLAT_RCCL_LIB, when set, is the only candidate: a wrong path is reported, not papered over)
        if (const char* e = getenv("MSPLAT_RCCL_LIB")) {
            h = dlopen(e, RTLD_NOW | RTLD_LOCAL);
        } else {
            for (const char* n : {"librccl.so.1", "librccl.so"})
                if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
            for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
                if (!h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        }
        if (!h) {
            const char* de = dlerror();          // (ONE call: dlerror() clears the error it returns -- ADVICE r5)
            x.why = std::string("librccl not found (") + (de ? de : "?") + "); set MSPLAT_RCCL_LIB";
            return x;
        }
        auto load = [&](auto& fn, const char* n) {           // (the pointer type is the member's)
            fn = reinterpret_cast<std::decay_t<decltype(fn)>>(dlsym(h, n));
            if (!fn) x.why = std::string("librccl lacks ") + n;
        };
        load(x.GroupStart, "ncclGroupStart");
        load(x.GroupEnd, "ncclGroupEnd");
        load(x.Send, "ncclSend");
        load(x.Recv, "ncclRecv");
        load(x.CommInitAll, "ncclCommInitAll");
        load(x.CommDestroy, "ncclCommDestroy");
        load(x.GetErrorString, "ncclGetErrorString");
        if (x.why.empty()) x.lib = h;
        return x;
    }();
    return r;
}
constexpr int kNcclUint8 = 1;

// a run of consecutive pixel rows [y0, y0 + nrows) that travels to / from rank `peer`
struct Run { int peer, y0, nrows; };

// appends the runs of consecutive bin rows rank `rank` of `world` owns under a standard layout, as pixel rows of an image of H
// rows, to `out`.  (Runs end at block boundaries; contiguous bands are one run.)
int append_runs(int32_t kind, int32_t block_rows, int32_t world, int32_t rank, int H, int peer, std::vector<Run>* out)
{
    const int T = msplat_tile_size(), rows_full = (H + T - 1) / T;
    int32_t first, count, block, stride;
    const int pr = msplat_band_plan(kind, rows_full, world, rank, block_rows, &first, &count, &block, &stride);
    if (pr) return pr;
    for (int v = 0; v < count;) {
        const int k = v / block, row = first + k * stride + (v - k * block);
        int run = std::min(block - (v - k * block), count - v);          // the rest of this block
        // (stride == block: the next block follows immediately -- contiguous bands arrive here as count rows in one block)
        const int y0 = row * T, nrows = std::min(run * T, H - y0);
        v += run;
        if (nrows <= 0) break;
        out->push_back(Run{peer, y0, nrows});
    }
    return MSPLAT_OK;
}

// one RCCL group: step(run, index) posts the sends / receives of every run until one fails; a group that was opened is closed
// either way.  Returns the first non-zero nccl code.
template <class Step>
int post_group(const Rccl& R, const std::vector<Run>& runs, Step&& step)
{
    int nrc = R.GroupStart();
    if (nrc != 0) return nrc;
    for (size_t k = 0; k < runs.size() && nrc == 0; ++k) nrc = step(runs[k], k);
    const int erc = R.GroupEnd();
    return nrc != 0 ? nrc : erc;
}

// rows of `width` >= 1 pixels of a framebuffer format: bytes per pixel and per tight row, and whether a pitch can hold them
struct RowGeom {
    size_t bpp, tight;
    RowGeom(int fb_format, int width) : bpp(MSPLAT_FB_BYTES_PER_PIXEL(fb_format)), tight((size_t)width * bpp) {}
    bool fits(size_t pitch) const { return pitch >= tight && pitch % bpp == 0; }
};

// ---- fp16 on the wire (MSPLAT_EXCHANGE_WIRE_FP16): the rows of an RGBA32F target travel as RGBA16F ---------------------------------
// One thread per pixel of a run: float4 <-> four halves (round to nearest even).  `rows` pitch rows of `width` pixels; the packed side
// is tight (width * 8 bytes per row).
__global__ __launch_bounds__(256) void pack_rows_f16(const char* __restrict__ src, size_t pitch, int width, int rows, uint2* __restrict__ dst)
{
    const size_t n = (size_t)width * rows;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t y = i / (size_t)width, x = i - y * (size_t)width;
        const float4 v = reinterpret_cast<const float4*>(src + y * pitch)[x];
        union { _Float16 h[4]; uint2 u; } pk;
        pk.h[0] = (_Float16)v.x; pk.h[1] = (_Float16)v.y; pk.h[2] = (_Float16)v.z; pk.h[3] = (_Float16)v.w;
        dst[i] = pk.u;
    }
}
__global__ __launch_bounds__(256) void unpack_rows_f16(const uint2* __restrict__ src, char* __restrict__ dst, size_t pitch, int width, int rows)
{
    const size_t n = (size_t)width * rows;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t y = i / (size_t)width, x = i - y * (size_t)width;
        union { _Float16 h[4]; uint2 u; } pk;
        pk.u = src[i];
        reinterpret_cast<float4*>(dst + y * pitch)[x] = make_float4((float)pk.h[0], (float)pk.h[1], (float)pk.h[2], (float)pk.h[3]);
    }
}
dim3 rows_grid(int width, int rows) { return dim3((unsigned)std::min<size_t>(((size_t)width * rows + 255) / 256, 4096)); }

}  // namespace

struct msplat_group {
    std::vector<int> devices;
    std::vector<msplat_ctx*> ctx;
    std::vector<std::unique_ptr<Worker>> workers;      // [i - 1] drives ctx[i]
    std::vector<bool> peer_store;                      // ctx[i] stores into device 0's memory directly (the exchange in use)
    std::vector<bool> peer_ok;                         // ... and whether the peer mapping exists at all
    std::vector<void*> stage;                          // per-rank staging framebuffer when it may not
    std::vector<size_t> stage_bytes;
    int fb_format = MSPLAT_FB_RGBA32F;
    int kind = MSPLAT_BANDS_CONTIGUOUS, block_rows = 1;
    bool band_cull = false;
    int planned_rows = -1;                             // rows_full the contexts' layouts were set for
    hipEvent_t order_ev = nullptr;                     // "everything queued on context 0's stream so far" (msplat_group_render)
    int exchange = MSPLAT_EXCHANGE_PEER_STORE;         // what msplat_group_render is asked to use; last_exchange: what it used
    int last_exchange = MSPLAT_EXCHANGE_PEER_STORE;
    std::vector<void*> comms;                          // MSPLAT_EXCHANGE_RCCL: one ncclComm_t per device (ncclCommInitAll)
    std::string err;
    std::vector<std::string> rank_err;                 // [i]: text of a failure on rank i's worker thread that is not the
                                                       // context's own (HIP calls of the staged exchange); merged by for_all
};

namespace {

thread_local std::string g_group_error;

std::string vformat(const char* fmt, va_list ap)
{
    char buf[512];
    vsnprintf(buf, sizeof(buf), fmt, ap);
    return buf;
}

int gfail(msplat_group* g, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    g_group_error = vformat(fmt, ap);
    va_end(ap);
    if (g) g->err = g_group_error;
    return code;
}
#define GROUP_OR_FAIL(g) do { if (!(g)) return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "group is NULL"); } while (0)

// failure inside rank i's part of a for_all (possibly on a worker thread): the text goes to the rank's own slot -- several
// ranks may fail at once (they raced on g->err) -- and for_all reports it from the caller's thread
int rfail(msplat_group* g, uint32_t i, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    g->rank_err[i] = vformat(fmt, ap);
    va_end(ap);
    return code;
}

// runs f(i) for every rank: ranks >= 1 on their worker threads, rank 0 on the caller's; returns the first real error
// (MSPLAT_ERR_PAIR_OVERFLOW[_EARLIER] -- a deferred report about an EARLIER frame -- only if nothing worse happened)
int for_all(msplat_group* g, const std::function<int(uint32_t)>& f)
{
    GROUP_OR_FAIL(g);            // (f is not called: the entry points that only fan out leave the check to this line)
    const uint32_t n = (uint32_t)g->ctx.size();
    for (auto& e : g->rank_err) e.clear();
    for (uint32_t i = 1; i < n; ++i) g->workers[i - 1]->post([&f, i] { return f(i); });
    std::vector<int> rc(n, MSPLAT_OK);
    rc[0] = f(0);
    for (uint32_t i = 1; i < n; ++i) rc[i] = g->workers[i - 1]->wait();
    int soft = MSPLAT_OK;
    for (uint32_t i = 0; i < n; ++i) {
        if (rc[i] == MSPLAT_OK) continue;
        if (rc[i] == MSPLAT_ERR_PAIR_OVERFLOW || rc[i] == MSPLAT_ERR_PAIR_OVERFLOW_EARLIER) {
            if (!soft) { soft = rc[i]; g->err = msplat_last_error(g->ctx[i]); }
            continue;
        }
        g->err = std::string("device ") + std::to_string(g->devices[i]) + ": " +
                 (g->rank_err[i].empty() ? std::string(msplat_last_error(g->ctx[i])) : g->rank_err[i]);
        g_group_error = g->err;
        return rc[i];
    }
    if (soft) g_group_error = g->err;
    return soft;
}

// (re)assigns the bin rows when the viewport's row count changes
int plan_rows(msplat_group* g, const float viewport[4])
{
    if (!viewport) return gfail(g, MSPLAT_ERR_INVALID_ARG, "NULL viewport");
    const int H = (int)viewport[3], T = msplat_tile_size();
    if (H < 1) return gfail(g, MSPLAT_ERR_INVALID_ARG, "viewport height %d", H);
    const int rows = (H + T - 1) / T;
    const uint32_t n = (uint32_t)g->ctx.size();
    if (rows == g->planned_rows) return MSPLAT_OK;
    for (uint32_t i = 0; i < n; ++i) {
        int rc;
        if (n == 1) {
            rc = msplat_set_band(g->ctx[i], 1, 0);
        } else {
            int32_t first, count, block, stride;
            rc = msplat_band_plan(g->kind, rows, (int32_t)n, (int32_t)i, g->block_rows, &first, &count, &block, &stride);
            if (rc) return gfail(g, rc, "%s", msplat_last_error(nullptr));
            rc = msplat_set_band_layout(g->ctx[i], first, count, block, stride);
            if (!rc) rc = msplat_set_band_cull(g->ctx[i], g->band_cull ? 1 : 0);
        }
        if (rc) return gfail(g, rc, "%s", msplat_last_error(g->ctx[i]));
    }
    g->planned_rows = rows;
    return MSPLAT_OK;
}

// ---- msplat_group_render with a device target: what one rank does under each exchange ------------------------------------------
struct Frame {
    const float *cam, *proj, *vp, *nf;
    void *rgba, *stream0;       // the target on device 0 (H rows `pitch` bytes apart, `tight` bytes of pixels in each); context 0's stream
    size_t pitch, tight;
    int H;
};

// rank i's staging framebuffer holds at least `need` bytes
int ensure_stage(msplat_group* g, uint32_t i, size_t need)
{
    if (hipSetDevice(g->devices[i]) != hipSuccess) return rfail(g, i, MSPLAT_ERR_HIP, "hipSetDevice(%d) failed", g->devices[i]);
    if (g->stage_bytes[i] >= need) return MSPLAT_OK;
    (void)msplat_synchronize(g->ctx[i]);
    if (g->stage[i]) (void)hipFree(g->stage[i]);
    g->stage[i] = nullptr;
    g->stage_bytes[i] = 0;
    if (hipMalloc(&g->stage[i], need) != hipSuccess) return rfail(g, i, MSPLAT_ERR_HIP, "staging framebuffer: out of device memory");
    g->stage_bytes[i] = need;
    return MSPLAT_OK;
}

// no peer mapping: rank i renders into its staging framebuffer, as H rows of `pitch` bytes
int render_staged(msplat_group* g, uint32_t i, const Frame& f, size_t pitch)
{
    const int e = ensure_stage(g, i, pitch * (size_t)f.H);
    return e ? e : msplat_render(g->ctx[i], f.cam, f.proj, f.vp, f.nf, g->stage[i], pitch, 1);
}

// copy: a tight local image, then one copy per run of consecutive owned rows
int render_and_copy(msplat_group* g, uint32_t i, const Frame& f)
{
    const int r = render_staged(g, i, f, f.tight);
    if (r && r != MSPLAT_ERR_PAIR_OVERFLOW_EARLIER) return r;
    std::vector<Run> runs;
    const int pr = append_runs(g->kind, g->block_rows, (int32_t)g->ctx.size(), (int32_t)i, f.H, 0, &runs);
    if (pr) return rfail(g, i, pr, "%s", msplat_last_error(nullptr));
    hipStream_t s = (hipStream_t)msplat_get_stream(g->ctx[i]);
    for (const Run& run : runs)
        if (hipMemcpy2DAsync((char*)f.rgba + (size_t)run.y0 * f.pitch, f.pitch, (const char*)g->stage[i] + (size_t)run.y0 * f.tight,
                             f.tight, f.tight, (size_t)run.nrows, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return rfail(g, i, MSPLAT_ERR_HIP, "hipMemcpy2DAsync (device %d -> %d) failed", g->devices[i], g->devices[0]);
    return r;
}

// rank i's part of the frame: ranks >= 1 wait for the ordering event first, and context 0's stream waits for what they queued
// (RCCL: they only render, with the target's pitch -- post_staged_rows makes context 0's stream receive their rows)
int render_rank(msplat_group* g, uint32_t i, const Frame& f, bool use_rccl)
{
    msplat_ctx* c = g->ctx[i];
    if (i != 0) { const int e = msplat_wait_event(c, g->order_ev); if (e) return e; }
    if (i != 0 && use_rccl) return render_staged(g, i, f, f.pitch);
    // rank 0 and peer store -- zero-copy: this device's compositor writes its rows where they belong in device 0's framebuffer
    const int r = (i == 0 || g->peer_store[i]) ? msplat_render(c, f.cam, f.proj, f.vp, f.nf, f.rgba, f.pitch, 1) : render_and_copy(g, i, f);
    if (i == 0 || (r && r != MSPLAT_ERR_PAIR_OVERFLOW_EARLIER)) return r;
    const int j = msplat_stream_wait(c, f.stream0);
    return j ? j : r;
}

// RCCL: every rank has rendered its rows into an image of its own with the target's pitch (a run of rows is then one contiguous
// range on both sides); the caller's thread issues ALL sends and receives as one group: rank i's sends on its stream behind
// its compositor, device 0's receives on context 0's stream -- synchronising that stream = frame complete
int post_staged_rows(msplat_group* g, const Frame& f)
{
    const uint32_t n = (uint32_t)g->ctx.size();
    // (contexts created with async_submit: every rank's worker has issued its render before the sends are queued behind it)
    for (uint32_t i = 0; i < n; ++i) {
        const int w = msplat_stream_wait(g->ctx[i], msplat_get_stream(g->ctx[i]));
        if (w != MSPLAT_OK && w != MSPLAT_ERR_PAIR_OVERFLOW_EARLIER) return gfail(g, w, "msplat_group_render: %s", msplat_last_error(g->ctx[i]));
    }
    std::vector<Run> runs;                                             // (peer = the rank that owns and sends the run)
    int pr = MSPLAT_OK;
    for (uint32_t i = 1; i < n && pr == MSPLAT_OK; ++i) pr = append_runs(g->kind, g->block_rows, (int32_t)n, (int32_t)i, f.H, (int)i, &runs);
    if (pr) return gfail(g, pr, "msplat_group_render: %s", msplat_last_error(nullptr));
    const Rccl& R = rccl();
    const int nrc = post_group(R, runs, [&](const Run& run, size_t) {
        const size_t off = (size_t)run.y0 * f.pitch, bytes = (size_t)(run.nrows - 1) * f.pitch + f.tight;
        const int e = R.Send((const char*)g->stage[run.peer] + off, bytes, kNcclUint8, 0, g->comms[run.peer],
                             (hipStream_t)msplat_get_stream(g->ctx[run.peer]));
        return e != 0 ? e : R.Recv((char*)f.rgba + off, bytes, kNcclUint8, run.peer, g->comms[0], (hipStream_t)f.stream0);
    });
    return nrc != 0 ? gfail(g, MSPLAT_ERR_HIP, "msplat_group_render: RCCL row exchange failed: %s", R.GetErrorString(nrc)) : MSPLAT_OK;
}

}  // namespace

extern "C" {

const char* msplat_group_last_error(const msplat_group* g) { return g ? g->err.c_str() : g_group_error.c_str(); }

int msplat_group_create(msplat_group** out, const int32_t* devices, uint32_t n, const msplat_config* cfg)
{
    if (!out) return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_group_create: out is NULL");
    *out = nullptr;
    if (!devices || n < 1 || n > 64) return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_group_create: need 1..64 devices");
    if (cfg && cfg->stream && n > 1)
        return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_group_create: a caller stream can only be used with one device");
    msplat_config c{};
    c.struct_size = sizeof(c);
    c.t_epsilon = -1.0f;
    if (cfg) {
        if (cfg->struct_size > sizeof(c) || cfg->struct_size < 16)
            return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_group_create: bad config struct_size %u", cfg->struct_size);
        std::memcpy(&c, cfg, cfg->struct_size);
        c.struct_size = sizeof(c);
    }
    // (from here a failure is gfail(nullptr, ...): g_group_error keeps the text, `owner` destroys the half-built group)
    std::unique_ptr<msplat_group, decltype(&msplat_group_destroy)> owner(new msplat_group, &msplat_group_destroy);
    msplat_group* g = owner.get();
    g->fb_format = c.fb_format;
    for (uint32_t i = 0; i < n; ++i) {
        c.device = devices[i];
        msplat_ctx* h = nullptr;
        const int rc = msplat_create(&h, &c);
        if (rc) return gfail(nullptr, rc, "msplat_group_create: device %d: %s", devices[i], msplat_last_error(nullptr));
        g->ctx.push_back(h);
        g->devices.push_back(devices[i]);
    }
    g->peer_store.assign(n, true);
    g->stage.assign(n, nullptr);
    g->stage_bytes.assign(n, 0);
    g->rank_err.assign(n, std::string());
    if (n > 1 && (hipSetDevice(devices[0]) != hipSuccess || hipEventCreateWithFlags(&g->order_ev, hipEventDisableTiming) != hipSuccess))
        return gfail(nullptr, MSPLAT_ERR_HIP, "msplat_group_create: cannot create the ordering event on device %d", devices[0]);
    // peer mapping towards device 0: the other devices' compositors then write their rows into its framebuffer directly
    for (uint32_t i = 1; i < n; ++i) {
        if (devices[i] == devices[0]) continue;            // same device (tests): plain device memory
        int can = 0;
        bool ok = hipSetDevice(devices[i]) == hipSuccess && hipDeviceCanAccessPeer(&can, devices[i], devices[0]) == hipSuccess && can;
        if (ok) {
            const hipError_t e = hipDeviceEnablePeerAccess(devices[0], 0);
            ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
        }
        (void)hipGetLastError();
        g->peer_store[i] = ok;
    }
    g->peer_ok = g->peer_store;
    for (uint32_t i = 1; i < n; ++i) {
        g->workers.emplace_back(new Worker);
        Worker* w = g->workers.back().get();
        w->th = std::thread([w] { w->run(); });
    }
    if (const char* e = getenv("MSPLAT_GROUP_EXCHANGE")) {
        static const struct { const char* name; int exchange; } names[] = {
            {"peer", MSPLAT_EXCHANGE_PEER_STORE}, {"peer_store", MSPLAT_EXCHANGE_PEER_STORE}, {"rccl", MSPLAT_EXCHANGE_RCCL}, {"copy", MSPLAT_EXCHANGE_COPY}};
        int want = -1;
        for (const auto& x : names)
            if (std::strcmp(e, x.name) == 0) want = x.exchange;
        if (want < 0)                   // a typo ("nccl") must not silently select the default
            return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_group_create: MSPLAT_GROUP_EXCHANGE=%s: expected peer | peer_store | rccl | copy", e);
        const int rc = msplat_group_set_exchange(g, want);
        if (rc)                         // asked for in the environment and not available: say so instead of silently doing something else
            return gfail(nullptr, rc, "msplat_group_create: MSPLAT_GROUP_EXCHANGE=%s: %s", e, g->err.c_str());
    }
    *out = owner.release();
    return MSPLAT_OK;
}

int msplat_group_set_exchange(msplat_group* g, int32_t exchange)
{
    GROUP_OR_FAIL(g);
    const uint32_t n = (uint32_t)g->ctx.size();
    if (exchange == MSPLAT_EXCHANGE_PEER_STORE || exchange == MSPLAT_EXCHANGE_COPY) {
        for (uint32_t i = 1; i < n; ++i) g->peer_store[i] = exchange == MSPLAT_EXCHANGE_PEER_STORE && g->peer_ok[i];
        g->exchange = exchange;
        return MSPLAT_OK;
    }
    if (exchange != MSPLAT_EXCHANGE_RCCL) return gfail(g, MSPLAT_ERR_INVALID_ARG, "msplat_group_set_exchange: unknown exchange %d", exchange);
    if (n == 1) { g->exchange = exchange; return MSPLAT_OK; }          // one device: there is nothing to exchange
    const Rccl& R = rccl();
    if (!R.ok()) return gfail(g, MSPLAT_ERR_UNSUPPORTED, "msplat_group_set_exchange: %s", R.why.c_str());
    if (g->comms.empty()) {
        // one communicator per device of this process (rccl.h:236).  RCCL refuses a device that is listed twice.
        std::vector<void*> comms(n, nullptr);
        const int rc = R.CommInitAll(comms.data(), (int)n, g->devices.data());
        if (rc != 0) {
            (void)hipGetLastError();
            return gfail(g, MSPLAT_ERR_UNSUPPORTED, "msplat_group_set_exchange: ncclCommInitAll over %u devices failed: %s", n,
                         R.GetErrorString(rc));
        }
        g->comms = comms;
    }
    for (uint32_t i = 1; i < n; ++i) g->peer_store[i] = false;          // rows are rendered locally and sent
    g->exchange = exchange;
    return MSPLAT_OK;
}

int msplat_group_get_exchange(const msplat_group* g) { return g ? g->last_exchange : -1; }

void msplat_group_destroy(msplat_group* g)
{
    if (!g) return;
    for (auto& w : g->workers) {
        { std::lock_guard<std::mutex> lk(w->mu); w->quit = true; w->cv.notify_all(); }
        if (w->th.joinable()) w->th.join();
    }
    for (size_t i = 0; i < g->ctx.size(); ++i)
        if (g->ctx[i]) (void)msplat_synchronize(g->ctx[i]);
    for (void* c : g->comms)
        if (c && rccl().ok()) (void)rccl().CommDestroy(c);
    for (size_t i = 0; i < g->ctx.size(); ++i) {
        if (i < g->stage.size() && g->stage[i]) { (void)hipSetDevice(g->devices[i]); (void)hipFree(g->stage[i]); }
        msplat_destroy(g->ctx[i]);
    }
    if (g->order_ev) { (void)hipSetDevice(g->devices[0]); (void)hipEventDestroy(g->order_ev); }
    delete g;
}

uint32_t msplat_group_size(const msplat_group* g) { return g ? (uint32_t)g->ctx.size() : 0u; }

msplat_ctx* msplat_group_context(msplat_group* g, uint32_t i) { return (g && i < g->ctx.size()) ? g->ctx[i] : nullptr; }

int msplat_group_peer_store(const msplat_group* g, uint32_t i) { return (g && i < g->ctx.size() && g->peer_store[i]) ? 1 : 0; }

int msplat_group_upload_cloud(msplat_group* g, const void* aos, uint64_t n, uint32_t stride_bytes, const msplat_attr_offsets* off,
                              int full_sh)
{
    return for_all(g, [&](uint32_t i) { return msplat_upload_cloud(g->ctx[i], aos, n, stride_bytes, off, full_sh); });
}

int msplat_group_upload_gaussian_cloud(msplat_group* g, const msplat_cloud* c)
{
    return for_all(g, [&](uint32_t i) { return msplat_upload_gaussian_cloud(g->ctx[i], c); });
}

int msplat_group_upload_ply(msplat_group* g, const char* path, int import_full_sh)
{
    return for_all(g, [&](uint32_t i) { return msplat_upload_ply(g->ctx[i], path, import_full_sh); });
}

int msplat_group_set_cloud_storage(msplat_group* g, int32_t storage)
{
    GROUP_OR_FAIL(g);
    if (storage != MSPLAT_STORAGE_FP32 && storage != MSPLAT_STORAGE_SH_FP16 && storage != MSPLAT_STORAGE_SH_Q8)
        return gfail(g, MSPLAT_ERR_INVALID_ARG, "msplat_group_set_cloud_storage: unknown storage %d", storage);
    for (msplat_ctx* c : g->ctx) {
        const int rc = msplat_set_cloud_storage(c, storage);
        if (rc) return gfail(g, rc, "%s", msplat_last_error(c));
    }
    return MSPLAT_OK;
}

// msplat_set_target_mode on every context.  PREMULTIPLIED reads nothing and works with every exchange; LOAD is refused: the staging
// exchanges (copy, RCCL) render a rank's rows into a framebuffer of its own, which holds no destination rows to blend over.
int msplat_group_set_target_mode(msplat_group* g, int32_t mode)
{
    GROUP_OR_FAIL(g);
    if (mode != MSPLAT_TARGET_CLEAR && mode != MSPLAT_TARGET_LOAD && mode != MSPLAT_TARGET_PREMULTIPLIED)
        return gfail(g, MSPLAT_ERR_INVALID_ARG, "msplat_group_set_target_mode: unknown mode %d", mode);
    if (mode == MSPLAT_TARGET_LOAD)
        return gfail(g, MSPLAT_ERR_UNSUPPORTED, "msplat_group_set_target_mode: MSPLAT_TARGET_LOAD is not available on a group (a rank "
                     "that stages its rows has no destination rows to blend over); MSPLAT_TARGET_PREMULTIPLIED is");
    for (msplat_ctx* c : g->ctx) {
        const int rc = msplat_set_target_mode(c, mode);
        if (rc) return gfail(g, rc, "%s", msplat_last_error(c));
    }
    return MSPLAT_OK;
}

int msplat_group_set_layout(msplat_group* g, int32_t kind, int32_t block_rows)
{
    GROUP_OR_FAIL(g);
    if (kind != MSPLAT_BANDS_CONTIGUOUS && kind != MSPLAT_BANDS_INTERLEAVED && kind != MSPLAT_BANDS_BLOCK_INTERLEAVED &&
        kind != MSPLAT_BANDS_ROOT_WEIGHTED)
        return gfail(g, MSPLAT_ERR_INVALID_ARG, "msplat_group_set_layout: unknown kind %d", kind);
    if ((kind == MSPLAT_BANDS_BLOCK_INTERLEAVED || kind == MSPLAT_BANDS_ROOT_WEIGHTED) && block_rows < 1)
        return gfail(g, MSPLAT_ERR_INVALID_ARG, "msplat_group_set_layout: block_rows (rows per block / root weight in percent) must be >= 1");
    g->kind = kind;
    g->block_rows = std::max(1, block_rows);
    g->planned_rows = -1;
    return MSPLAT_OK;
}

int msplat_group_set_band_cull(msplat_group* g, int enable)
{
    GROUP_OR_FAIL(g);
    g->band_cull = enable != 0;
    g->planned_rows = -1;
    return MSPLAT_OK;
}

int msplat_group_sort(msplat_group* g, const float cameraMat[16], const float projMat[16], const float viewport[4],
                      const float nearFar[2])
{
    GROUP_OR_FAIL(g);
    const int rc = plan_rows(g, viewport);
    return rc ? rc : for_all(g, [&](uint32_t i) { return msplat_sort(g->ctx[i], cameraMat, projMat, viewport, nearFar); });
}

int msplat_group_render(msplat_group* g, const float cameraMat[16], const float projMat[16], const float viewport[4],
                        const float nearFar[2], void* rgba, uint64_t pitch_bytes, int out_is_device)
{
    GROUP_OR_FAIL(g);
    if (!rgba) return gfail(g, MSPLAT_ERR_INVALID_ARG, "msplat_group_render: rgba is NULL");
    int rc = plan_rows(g, viewport);
    if (rc) return rc;
    const uint32_t n = (uint32_t)g->ctx.size();
    const int W = (int)viewport[2], H = (int)viewport[3];
    const RowGeom q(g->fb_format, W);
    const size_t pitch = pitch_bytes ? (size_t)pitch_bytes : q.tight;
    if (W < 1 || H < 1 || !q.fits(pitch))
        return gfail(g, MSPLAT_ERR_INVALID_ARG, "msplat_group_render: pitch %llu too small / misaligned for a %dx%d target of %zu bytes per pixel",
                     (unsigned long long)pitch, W, H, q.bpp);
    if (!out_is_device)         // host image: every context copies its own rows into it (msplat_render's band rule)
        return for_all(g, [&](uint32_t i) { return msplat_render(g->ctx[i], cameraMat, projMat, viewport, nearFar, rgba, pitch, 0); });

    // The frame inherits context 0's stream order on EVERY rank: whatever the caller queued on that stream before
    // this call -- typically the consumer of the previous frame in the same framebuffer -- is finished before any rank's
    // compositor or row copy writes into `rgba`, exactly as with a single context.  One event record + n - 1 stream waits.
    const Frame f{cameraMat, projMat, viewport, nearFar, rgba, msplat_get_stream(g->ctx[0]), pitch, q.tight, H};
    if (n > 1 && (hipSetDevice(g->devices[0]) != hipSuccess || hipEventRecord(g->order_ev, (hipStream_t)f.stream0) != hipSuccess))
        return gfail(g, MSPLAT_ERR_HIP, "msplat_group_render: cannot record the ordering event on device %d", g->devices[0]);
    const bool use_rccl = n > 1 && g->exchange == MSPLAT_EXCHANGE_RCCL && !g->comms.empty();
    g->last_exchange = n == 1 ? g->exchange : (use_rccl ? MSPLAT_EXCHANGE_RCCL : MSPLAT_EXCHANGE_COPY);
    for (uint32_t i = 1; i < n && !use_rccl; ++i)
        if (g->peer_store[i]) g->last_exchange = MSPLAT_EXCHANGE_PEER_STORE;
    rc = for_all(g, [&](uint32_t i) { return render_rank(g, i, f, use_rccl); });
    if (!use_rccl || (rc && rc != MSPLAT_ERR_PAIR_OVERFLOW_EARLIER)) return rc;
    const int prc = post_staged_rows(g, f);
    return prc ? prc : rc;
}

// ---- the exchange for one process per GPU --------------------------------------------------------------------------------------
static int band_exchange_impl(msplat_ctx* ctx, void* comm, int32_t rank, int32_t world, int32_t root, int32_t kind, int32_t block_rows,
                              const void* src, void* dst, uint64_t pitch_bytes, int32_t width, int32_t height, int32_t flags, bool loopback)
{
    if (!ctx) return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_band_exchange: ctx is NULL");
    if (world < 1 || rank < 0 || rank >= world || root < 0 || root >= world)
        return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_band_exchange: rank %d / root %d of %d", rank, root, world);
    if (world == 1 && !loopback) return MSPLAT_OK;                     // the whole image is this rank's
    if (!comm || !src || !dst || width < 1 || height < 1)
        return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_band_exchange: NULL communicator / framebuffer or empty image");
    const bool wire16 = (flags & MSPLAT_EXCHANGE_WIRE_FP16) != 0;
    // the pixel size is the CONTEXT's target format (it used to be inferred from the pitch)
    const RowGeom q(msplat_get_fb_format(ctx), width);
    if (wire16 && q.bpp != 16u)
        return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_band_exchange: MSPLAT_EXCHANGE_WIRE_FP16 needs an RGBA32F target");
    if (!q.fits((size_t)pitch_bytes))
        return gfail(nullptr, MSPLAT_ERR_INVALID_ARG, "msplat_band_exchange: pitch %llu too small / misaligned for width %d of %zu-byte pixels",
                     (unsigned long long)pitch_bytes, width, q.bpp);
    const Rccl& R = rccl();
    if (!R.ok()) return gfail(nullptr, MSPLAT_ERR_UNSUPPORTED, "msplat_band_exchange: %s", R.why.c_str());
    hipStream_t s = (hipStream_t)msplat_get_stream(ctx);
    // an async_submit context: its worker thread must have ISSUED the frame before the exchange is queued behind it (a wait on the
    // context's own stream is just that; it may also hand over a queued call's overflow warning, which is passed on at the end)
    const int wrc = msplat_stream_wait(ctx, s);
    if (wrc != MSPLAT_OK && wrc != MSPLAT_ERR_PAIR_OVERFLOW_EARLIER) return gfail(nullptr, wrc, "msplat_band_exchange: %s", msplat_last_error(ctx));

    // the runs this call sends (an owner: its own, to the root), then from nsend on the runs it receives (the root: every other rank's);
    // loopback (tests, one rank): this rank plays owner and root at once -- its runs travel from src to dst through ncclSend / ncclRecv to itself
    std::vector<Run> runs;
    size_t nsend = 0;
    int prc = MSPLAT_OK;
    auto add = [&](int32_t r, int peer) { if (!prc) prc = append_runs(kind, block_rows, world, r, height, peer, &runs); return runs.size(); };
    if (loopback) {
        nsend = add(rank, 0);
        add(rank, 0);
    } else if (rank != root) {
        nsend = add(rank, root);
    } else {
        for (int32_t r = 0; r < world; ++r)
            if (r != root) add(r, r);
    }
    if (prc) return gfail(nullptr, prc, "msplat_band_exchange: %s", msplat_last_error(nullptr));

    // fp16 on the wire: a run is packed into (and received into) stream-ordered scratch; half the bytes cross the link
    char* scratch = nullptr;
    std::vector<size_t> woff(runs.size());
    if (wire16) {
        size_t total = 0;
        for (size_t i = 0; i < runs.size(); ++i) { woff[i] = total; total += (size_t)runs[i].nrows * width * 8; }
        if (total != 0 && hipMallocAsync((void**)&scratch, total, s) != hipSuccess) {
            (void)hipGetLastError();
            return gfail(nullptr, MSPLAT_ERR_HIP, "msplat_band_exchange: no memory for %zu bytes of fp16 rows", total);
        }
        for (size_t i = 0; i < nsend; ++i)
            hipLaunchKernelGGL(pack_rows_f16, rows_grid(width, runs[i].nrows), dim3(256), 0, s, (const char*)src + (size_t)runs[i].y0 * pitch_bytes,
                               (size_t)pitch_bytes, width, runs[i].nrows, (uint2*)(scratch + woff[i]));
    }
    // a run travels as ONE message when the rows are tight (pitch == width x pixel size: the usual case), else row by row inside
    // the same group: nothing outside the target's own pixels is read or written -- a target that is a window of a wider
    // surface keeps its neighbours, and the last row need not be followed by a full pitch; or as tight fp16 rows
    const bool tight_rows = (size_t)pitch_bytes == q.tight;
    const int nrc = post_group(R, runs, [&](const Run& r, size_t i) -> int {
        const bool send = i < nsend;          // (a send reads from `from`, a receive writes to `to`)
        auto post = [&](const void* from, void* to, size_t bytes) {
            return send ? R.Send(from, bytes, kNcclUint8, r.peer, comm, s) : R.Recv(to, bytes, kNcclUint8, r.peer, comm, s);
        };
        if (wire16) return post(scratch + woff[i], scratch + woff[i], (size_t)r.nrows * width * 8);
        const size_t off = (size_t)r.y0 * (size_t)pitch_bytes;
        if (tight_rows) return post((const char*)src + off, (char*)dst + off, (size_t)r.nrows * q.tight);
        int e = 0;
        for (int k = 0; k < r.nrows && e == 0; ++k)
            e = post((const char*)src + off + k * (size_t)pitch_bytes, (char*)dst + off + k * (size_t)pitch_bytes, q.tight);
        return e;
    });
    if (wire16) {
        if (nrc == 0)
            for (size_t i = nsend; i < runs.size(); ++i)
                hipLaunchKernelGGL(unpack_rows_f16, rows_grid(width, runs[i].nrows), dim3(256), 0, s, (const uint2*)(scratch + woff[i]),
                                   (char*)dst + (size_t)runs[i].y0 * pitch_bytes, (size_t)pitch_bytes, width, runs[i].nrows);
        if (scratch) (void)hipFreeAsync(scratch, s);
        if (hipGetLastError() != hipSuccess) return gfail(nullptr, MSPLAT_ERR_HIP, "msplat_band_exchange: a pack / unpack launch failed");
    }
    if (nrc != 0) return gfail(nullptr, MSPLAT_ERR_HIP, "msplat_band_exchange: RCCL: %s", R.GetErrorString(nrc));
    if (wrc != MSPLAT_OK) return gfail(nullptr, wrc, "%s", msplat_last_error(ctx));
    return MSPLAT_OK;
}

int msplat_band_exchange(msplat_ctx* ctx, void* comm, int32_t rank, int32_t world, int32_t root, int32_t kind, int32_t block_rows,
                         void* rgba, uint64_t pitch_bytes, int32_t width, int32_t height, int32_t flags)
{
    return band_exchange_impl(ctx, comm, rank, world, root, kind, block_rows, rgba, rgba, pitch_bytes, width, height, flags, false);
}

int msplat_debug_band_exchange_loopback(msplat_ctx* ctx, void* comm, int32_t kind, int32_t block_rows, int32_t world, int32_t rank,
                                        const void* src, void* dst, uint64_t pitch_bytes, int32_t width, int32_t height, int32_t flags)
{
    return band_exchange_impl(ctx, comm, rank, world, 0, kind, block_rows, src, dst, pitch_bytes, width, height, flags, true);
}

int msplat_group_synchronize(msplat_group* g)
{
    return for_all(g, [&](uint32_t i) { return msplat_synchronize(g->ctx[i]); });
}

}  // extern "C"
