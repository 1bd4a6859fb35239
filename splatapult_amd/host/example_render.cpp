// example_render.cpp -- the reference's per-frame sequence (App::Render, /root/reference/src/app.cpp:1037-1068)
// written against the drop-in C++ surface: GaussianCloud::ImportPly -> SplatRenderer::Init ->
// Sort + Render into an explicit RGBA32F framebuffer, dumped as a binary PPM-like float file.
//
//   g++ -std=c++17 -I. splatapult_amd/host/example_render.cpp -Lsplatapult_amd/lib -lmsplat -o example_render
//   ./example_render scene.ply out.f32 [width height] [--nosh] [--frames-in-flight N] [--devices 0,1,2,...] [--over-gradient] [--depth out_depth.f32] [--srgb8 out.png] [--crop-sphere cx cy cz r] [--pick X,Y] [--min-score S] [--highlight R,G,B,A] [--compact] [--append OTHER.ply] [--save OUT.ply] [--fade S] [--tint R,G,B,A] [--select-sphere CX,CY,CZ,R] [--min-alpha T] [--min-neighbours K,R]
// With --frames-in-flight N the same frame is issued N + 1 times round-robin over N contexts that share the cloud
// (SplatRenderer::SetFramesInFlight); the last one is written.  With --devices the frame's bin rows are dealt to the
// listed GPUs (SplatRenderer::ConfigureDevices, msplat_group_*): same pixels.  With --over-gradient the target is first filled with
// a vertical gradient -- standing in for what App::Render draws before the splats (app.cpp:1046-1063) -- and the frame is blended
// over it (SplatRenderer::SetTargetMode(MSPLAT_TARGET_LOAD)), as the reference's Render does with its bound framebuffer.
// With --depth the frame also hands out its depth plane (SplatRenderer::RenderWithDepth: W x H float32 window depth over the clear
// depth 1.0, row 0 = bottom), written to the named file; one device only.
// With --srgb8 the target is an MSPLAT_FB_SRGB8_ALPHA8 one -- the reference's sRGB window: 4 bytes per pixel, encoded by the compositor's
// final store -- and the PNG is written from those bytes (WritePNG), with no float frame in between; out.f32 is then not written.
// With --crop-sphere only the splats whose centre lies in the sphere of radius r around (cx, cy, cz) are drawn (SplatRenderer::SetCrop,
// MSPLAT_CROP_SPHERE): the cloud is uploaded whole, the Sort and everything behind it work on what the crop keeps.  One device only.
// With --pick X,Y the splat that contributes most to pixel (X, Y) (row 0 = bottom) and its window depth are printed (SplatRenderer::Pick,
// msplat_render_ids through a 1 x 1 window).  One device only.
// With --min-score S the rendered view is scored (SplatRenderer::RenderScores), every splat that contributes less than S fully covered
// pixels to it is hidden (MarkScores below S * MSPLAT_SCORE_ONE into a mask of ones, SetVisibilityDevice), and the frame is sorted and
// rendered again: what is written is the pruned view; the number of hidden splats is printed.  One device, one frame in flight.
// With --highlight R,G,B,A (the record's colour space: linear values, A in [0, 1]) nothing is hidden: --min-score then TINTS the splats it
// selects and --pick the picked splat (SplatRenderer::SetOverlayPalette + SetOverlayDevice / SetOverlay, msplat_set_overlay*: class 1 of a
// two-entry palette) and the frame is rendered again -- without another Sort: the overlay changes the projected records, not the cloud.
// With --fade S every splat's opacity is multiplied by S (clamped to [0, 1]) and with --tint R,G,B,A every splat's colour is blended
// towards R,G,B with weight A in every view direction -- col' = (1 - A) col + A (R, G, B) on the SH coefficients, the record's colour
// space -- IN THE CLOUD (SplatRenderer::AdjustCloud, msplat_adjust_cloud), and the frame is sorted and rendered again; --save writes
// the adjusted cloud.  With --min-score (and no --highlight) the splats it selects are not hidden but adjusted: floaters fade or
// change colour, the rest of the cloud keeps its bits.  One device, one frame in flight.
// With --select-sphere CX,CY,CZ,R every splat whose centre lies in that sphere is marked into a device mask (SplatRenderer::MarkVolume,
// msplat_mark_volume: the crop's rule, hidden and occluded splats included) and the selection's count, box, centroid and reach are
// printed (SplatRenderer::MeasureCloud); with --highlight the selection is tinted and the frame rendered again.  One device, one frame in flight.
// With --min-alpha T a 16-bin histogram of every splat's longest axis (SplatRenderer::CloudValues with MSPLAT_VALUE_SCALE_MAX,
// SplatRenderer::HistogramValues: first the range, then the counts) is printed, the splats with alpha below T are hidden
// (MSPLAT_VALUE_ALPHA, SplatRenderer::MarkValues of 0 into a mask of ones, SetVisibilityDevice) and the frame is sorted and rendered
// again.  One device, one frame in flight.
// With --min-neighbours K,R the splats with fewer than K other splats within R of their centre -- floaters are isolated splats -- are
// hidden (SplatRenderer::NeighbourValues with MSPLAT_NEAR_COUNT and cap K, SplatRenderer::MarkValues of 0 into a mask of ones,
// SetVisibilityDevice), the grid's numbers are printed and the frame is sorted and rendered again; --compact and --save then drop
// and write them.  One device, one frame in flight.
// With --compact, after --min-score / --crop-sphere, the hidden splats are dropped for good (SplatRenderer::CompactCloud,
// msplat_compact_cloud: the kept records gathered into a new store on the device), the splat counts before and after are printed and
// the frame is sorted and rendered once more from the smaller cloud: the same pixels.  One device only.
// With --append OTHER.ply a second renderer uploads that file and its splats are appended to the scene's before the frame
// (SplatRenderer::AppendCloud, msplat_append_cloud: both stores' records gathered into a new one on the device); the counts are
// printed.  OTHER.ply is read with the scene's SH degree.  One device only.
// With --save OUT.ply the cloud as it is on the device after --append, --crop-sphere and --compact have run is written as a PLY
// (SplatRenderer::ExportPly, msplat_export_ply: the per-splat math of GaussianCloud::ExportPly as a HIP kernel).  A crop that was not
// made permanent with --compact is not applied: what is saved is the cloud.  One device only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <memory>
#include <vector>

#include "msplat_host.hpp"
#include "scene_config.hpp"

// device memory without the HIP headers: four calls of the runtime libmsplat.so already brought into the process
struct DeviceMemory {
    int (*alloc)(void**, size_t) = nullptr;
    int (*fill)(void*, int, size_t) = nullptr;
    int (*release)(void*) = nullptr;
    int (*wait)() = nullptr;
    bool Load()
    {
        void* hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!hip) return false;
        alloc = reinterpret_cast<int (*)(void**, size_t)>(dlsym(hip, "hipMalloc"));
        fill = reinterpret_cast<int (*)(void*, int, size_t)>(dlsym(hip, "hipMemset"));
        release = reinterpret_cast<int (*)(void*)>(dlsym(hip, "hipFree"));
        wait = reinterpret_cast<int (*)()>(dlsym(hip, "hipDeviceSynchronize"));
        return alloc && fill && release && wait;
    }
};

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s scene.ply out.f32 [width height] [--nosh]\n", argv[0]);
        return 2;
    }
    int W = 1024, H = 768;   // the reference's default window (sdl_main.cpp:92)
    bool nosh = false, overGradient = false, compact = false;
    if (argc >= 5 && argv[3][0] != '-') { W = std::atoi(argv[3]); H = std::atoi(argv[4]); }
    int inFlight = 1;
    int pickX = -1, pickY = -1;      // --pick: print the splat under this pixel (row 0 = bottom) and its window depth
    double minScore = -1.0;          // --min-score: hide the splats that contribute less than this many pixels, render again
    float highlight[8] = {0, 0, 0, 0, 0, 0, 0, -1.0f};      // --highlight: palette entry 0 (no effect) and entry 1; A < 0: not given
    float fade = -1.0f;              // --fade: the factor on alpha; < 0: not given
    float tintTo[4] = {0, 0, 0, -1.0f};       // --tint: the colour and the weight; A < 0: not given
    const char* depthPath = nullptr;
    const char* srgb8Path = nullptr;
    const char* appendPath = nullptr;
    const char* savePath = nullptr;
    std::vector<int> devices;
    float cropSphere[4] = {0.0f, 0.0f, 0.0f, 0.0f};       // centre, radius; radius 0: no crop
    float selectSphere[4] = {0.0f, 0.0f, 0.0f, 0.0f};     // --select-sphere: centre, radius; radius 0: not given
    int minNeighbours = 0;           // --min-neighbours K,R: hide the splats with fewer than K neighbours within R; 0: not given
    float neighbourRadius = 0.0f;
    float minAlpha = -1.0f;          // --min-alpha: hide the splats whose alpha is below it; < 0: not given
    for (int i = 3; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--select-sphere") && i + 1 < argc &&
            std::sscanf(argv[i + 1], "%f,%f,%f,%f", &selectSphere[0], &selectSphere[1], &selectSphere[2], &selectSphere[3]) != 4)
            selectSphere[3] = 0.0f;
        if (!std::strcmp(argv[i], "--crop-sphere") && i + 4 < argc)
            for (int k = 0; k < 4; ++k) cropSphere[k] = (float)std::atof(argv[i + 1 + k]);
        nosh = nosh || !std::strcmp(argv[i], "--nosh");
        overGradient = overGradient || !std::strcmp(argv[i], "--over-gradient");
        compact = compact || !std::strcmp(argv[i], "--compact");
        if (!std::strcmp(argv[i], "--frames-in-flight") && i + 1 < argc) inFlight = std::atoi(argv[i + 1]);
        if (!std::strcmp(argv[i], "--depth") && i + 1 < argc) depthPath = argv[i + 1];
        if (!std::strcmp(argv[i], "--pick") && i + 1 < argc && std::sscanf(argv[i + 1], "%d,%d", &pickX, &pickY) != 2) pickX = pickY = -1;
        if (!std::strcmp(argv[i], "--srgb8") && i + 1 < argc) srgb8Path = argv[i + 1];
        if (!std::strcmp(argv[i], "--append") && i + 1 < argc) appendPath = argv[i + 1];
        if (!std::strcmp(argv[i], "--save") && i + 1 < argc) savePath = argv[i + 1];
        if (!std::strcmp(argv[i], "--min-score") && i + 1 < argc) minScore = std::atof(argv[i + 1]);
        if (!std::strcmp(argv[i], "--highlight") && i + 1 < argc &&
            std::sscanf(argv[i + 1], "%f,%f,%f,%f", &highlight[4], &highlight[5], &highlight[6], &highlight[7]) != 4)
            highlight[7] = -1.0f;
        if (!std::strcmp(argv[i], "--min-alpha") && i + 1 < argc) minAlpha = (float)std::atof(argv[i + 1]);
        if (!std::strcmp(argv[i], "--min-neighbours") && i + 1 < argc &&
            (std::sscanf(argv[i + 1], "%d,%f", &minNeighbours, &neighbourRadius) != 2 || minNeighbours < 1 || !(neighbourRadius > 0.0f))) {
            std::fprintf(stderr, "--min-neighbours takes K,R with K >= 1 and R > 0\n");
            return 1;
        }
        if (!std::strcmp(argv[i], "--fade") && i + 1 < argc) fade = (float)std::atof(argv[i + 1]);
        if (!std::strcmp(argv[i], "--tint") && i + 1 < argc && std::sscanf(argv[i + 1], "%f,%f,%f,%f", &tintTo[0], &tintTo[1], &tintTo[2], &tintTo[3]) != 4)
            tintTo[3] = -1.0f;
        if (!std::strcmp(argv[i], "--devices") && i + 1 < argc)
            for (const char* p = argv[i + 1]; *p;) {
                devices.push_back(std::atoi(p));
                while (*p && *p != ',') ++p;
                if (*p == ',') ++p;
            }
    }

    auto cloud = std::make_shared<GaussianCloud>(GaussianCloud::Options{!nosh, false});
    if (!cloud->ImportPly(argv[1])) return 1;

    SplatRenderer renderer;
    renderer.SetFramesInFlight(inFlight);
    if (srgb8Path) renderer.Configure(/*device*/0, MSPLAT_FB_SRGB8_ALPHA8);
    if (devices.size() > 1) renderer.ConfigureDevices(devices, MSPLAT_BANDS_BLOCK_INTERLEAVED, 2);
    if (!renderer.Init(cloud, /*isFramebufferSRGBEnabled=*/false, /*useRgcSortOverride=*/false)) return 1;

    if (appendPath && devices.size() <= 1) {
        auto other = std::make_shared<GaussianCloud>(GaussianCloud::Options{!nosh, false});
        if (!other->ImportPly(appendPath)) return 1;
        SplatRenderer second;
        uint64_t added = 0;
        if (!second.Init(other, false, false) || !renderer.AppendCloud(second, nullptr, nullptr, &added)) return 1;
        std::printf("appended: %zu + %llu of %zu splats\n", cloud->GetNumGaussians(), (unsigned long long)added, other->GetNumGaussians());
    }

    if (cropSphere[3] > 0.0f) {
        // world -> crop space: the sphere becomes the unit sphere, q = (p - c) / r
        const float s = 1.0f / cropSphere[3];
        const float worldToCrop[16] = {s, 0, 0, 0, 0, s, 0, 0, 0, 0, s, 0, -cropSphere[0] * s, -cropSphere[1] * s, -cropSphere[2] * s, 1};
        if (!renderer.SetCrop(worldToCrop, MSPLAT_CROP_SPHERE)) return 1;
    }

    // app.cpp:73-75,1039-1042: camera at the identity pose pulled back along +Z, 45 degree fovy
    msplat::mat4 cameraMat{}, projMat{};
    for (int i = 0; i < 4; ++i) cameraMat.m[i * 4 + i] = 1.0f;
    cameraMat.m[14] = 5.0f;
    const float zn = 0.1f, zf = 1000.0f;
    msplat_perspective(45.0f * 3.14159265358979f / 180.0f, (float)W / (float)H, zn, zf, projMat.m);
    msplat::vec4 viewport{{0.0f, 0.0f, (float)W, (float)H}};
    msplat::vec2 nearFar{{zn, zf}};

    std::vector<float> fb((size_t)W * H * 4);
    std::vector<float> depth(depthPath ? (size_t)W * H : 0);
    if (srgb8Path) {
        // the window's own format: bytes R G B A, row 0 = GL's bottom row; the PNG wants the top row first
        std::vector<uint8_t> fb8((size_t)W * H * 4), png((size_t)W * H * 4);
        renderer.SetRenderTarget(fb8.data(), 0, /*isDevicePointer=*/false);
        renderer.Sort(cameraMat, projMat, viewport, nearFar);
        renderer.Render(cameraMat, projMat, viewport, nearFar);
        renderer.Synchronize();
        for (int y = 0; y < H; ++y) std::memcpy(&png[(size_t)y * W * 4], &fb8[(size_t)(H - 1 - y) * W * 4], (size_t)W * 4);
        if (!WritePNG(srgb8Path, png.data(), W, H)) return 1;
        std::printf("%zu splats -> %dx%d SRGB8_ALPHA8 written to %s\n", cloud->GetNumGaussians(), W, H, srgb8Path);
        return 0;
    }
    renderer.SetRenderTarget(fb.data(), 0, /*isDevicePointer=*/false);
    if (overGradient && !renderer.SetTargetMode(MSPLAT_TARGET_LOAD)) return 1;
    for (int k = 0; k < (inFlight > 1 ? inFlight + 1 : 1); ++k) {
        if (overGradient)            // every frame starts from the backdrop: LOAD blends over whatever the target holds
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    float* px = &fb[((size_t)y * W + x) * 4];
                    px[0] = 0.1f; px[1] = 0.2f; px[2] = 0.2f + 0.6f * (float)y / (float)H; px[3] = 1.0f;
                }
        renderer.Sort(cameraMat, projMat, viewport, nearFar);       // moves on to the next context
        if (depthPath) renderer.RenderWithDepth(cameraMat, projMat, viewport, nearFar, depth.data());
        else renderer.Render(cameraMat, projMat, viewport, nearFar);
    }
    renderer.Synchronize();
    const bool tint = highlight[7] >= 0.0f && inFlight == 1 && devices.size() <= 1;
    // --fade / --tint: the 3 x 4 map [G | o], column-major, G = (1 - A) I and o = A (R, G, B); d_select = nullptr: the whole cloud
    const bool adjust = (fade >= 0.0f || tintTo[3] >= 0.0f) && inFlight == 1 && devices.size() <= 1;
    auto adjustCloud = [&](const uint8_t* d_select) {
        const float t = 1.0f - tintTo[3], a = tintTo[3];
        const float map[12] = {t, 0, 0, 0, t, 0, 0, 0, t, a * tintTo[0], a * tintTo[1], a * tintTo[2]};
        if (!renderer.AdjustCloud(tintTo[3] >= 0.0f ? map : nullptr, fade, d_select)) return false;
        renderer.Sort(cameraMat, projMat, viewport, nearFar);
        if (depthPath) renderer.RenderWithDepth(cameraMat, projMat, viewport, nearFar, depth.data());
        else renderer.Render(cameraMat, projMat, viewport, nearFar);
        renderer.Synchronize();
        return true;
    };
    if (pickX >= 0 && pickY >= 0) {
        uint32_t index = MSPLAT_ID_NONE;
        float zw = 1.0f;
        if (!renderer.Pick(cameraMat, projMat, viewport, nearFar, pickX, pickY, &index, &zw)) return 1;
        if (index == MSPLAT_ID_NONE) std::printf("pick (%d, %d): no splat, z_w %.9g\n", pickX, pickY, zw);
        else std::printf("pick (%d, %d): splat %u, z_w %.9g\n", pickX, pickY, index, zw);
        if (tint && index != MSPLAT_ID_NONE && minScore < 0.0) {
            std::vector<uint8_t> classes(cloud->GetNumGaussians(), 0);
            if (index < classes.size()) classes[index] = 1;
            if (!renderer.SetOverlayPalette(highlight, 2) || !renderer.SetOverlay(classes.data(), classes.size())) return 1;
            if (depthPath) renderer.RenderWithDepth(cameraMat, projMat, viewport, nearFar, depth.data());      // the latest Sort: no new one
            else renderer.Render(cameraMat, projMat, viewport, nearFar);
            renderer.Synchronize();
            std::printf("splat %u highlighted\n", index);
        }
    }
    if (minScore >= 0.0 && inFlight == 1 && devices.size() <= 1) {
        const size_t n = cloud->GetNumGaussians();
        DeviceMemory dm;
        void *score = nullptr, *mask = nullptr;
        if (!dm.Load() || dm.alloc(&score, n * 8) != 0 || dm.alloc(&mask, n) != 0) return 1;
        if (dm.fill(score, 0, n * 8) != 0 || dm.fill(mask, tint || adjust ? 0 : 1, n) != 0 || dm.wait() != 0) return 1;      // filled before the context's stream starts
        if (!renderer.RenderScores(cameraMat, projMat, viewport, nearFar, nullptr, static_cast<uint64_t*>(score), n)) return 1;
        if (!renderer.MarkScores(static_cast<const uint64_t*>(score), n, MSPLAT_SCORE_BELOW, (uint64_t)(minScore * (double)MSPLAT_SCORE_ONE),
                                 static_cast<uint8_t*>(mask), tint || adjust ? 1 : 0))
            return 1;
        // adjusted in the cloud (--fade / --tint: nothing is hidden), hidden (a mask of ones with zeros marked: the next Sort drops them),
        // or shown: classes of zeros with ones marked, tinted by the palette's entry 1 at the next Render
        if (adjust && !tint) {
            if (!adjustCloud(static_cast<const uint8_t*>(mask))) return 1;
            std::printf("min score %g: the splats below it are adjusted (fade %g, tint weight %g)\n", minScore, fade, tintTo[3]);
        } else {
            if (tint ? !(renderer.SetOverlayPalette(highlight, 2) && renderer.SetOverlayDevice(static_cast<const uint8_t*>(mask), n))
                     : !renderer.SetVisibilityDevice(static_cast<const uint8_t*>(mask), n))
                return 1;
            if (!tint) renderer.Sort(cameraMat, projMat, viewport, nearFar);
            if (depthPath) renderer.RenderWithDepth(cameraMat, projMat, viewport, nearFar, depth.data());
            else renderer.Render(cameraMat, projMat, viewport, nearFar);
            renderer.Synchronize();
            uint64_t hidden = 0;
            if (msplat_get_visibility(renderer.GetContext(), nullptr, nullptr, &hidden) != MSPLAT_OK) return 1;
            if (tint) std::printf("min score %g: the splats below it are highlighted\n", minScore);
            else std::printf("min score %g: %llu of %zu splats hidden\n", minScore, (unsigned long long)hidden, n);
        }
        dm.release(score);
        dm.release(mask);
    } else if (adjust) {
        if (!adjustCloud(nullptr)) return 1;
        std::printf("adjusted: every splat (fade %g, tint weight %g)\n", fade, tintTo[3]);
    }

    if (selectSphere[3] > 0.0f && inFlight == 1 && devices.size() <= 1) {
        const size_t n = cloud->GetNumGaussians();
        DeviceMemory dm;
        void* mask = nullptr;
        if (!dm.Load() || dm.alloc(&mask, n) != 0 || dm.fill(mask, 0, n) != 0 || dm.wait() != 0) return 1;
        const float s = 1.0f / selectSphere[3];
        const float worldToVolume[16] = {s, 0, 0, 0, 0, s, 0, 0, 0, 0, s, 0, -selectSphere[0] * s, -selectSphere[1] * s, -selectSphere[2] * s, 1};
        msplat_cloud_measure m;
        if (!renderer.MarkVolume(worldToVolume, MSPLAT_CROP_SPHERE, static_cast<uint8_t*>(mask), n, 1) ||
            !renderer.MeasureCloud(static_cast<const uint8_t*>(mask), n, &m))
            return 1;
        std::printf("select sphere: %llu of %zu splats", (unsigned long long)m.selected, n);
        if (m.finite)
            std::printf(", box (%g, %g, %g) .. (%g, %g, %g), centroid (%g, %g, %g), reach %g", m.lo[0], m.lo[1], m.lo[2], m.hi[0], m.hi[1], m.hi[2],
                        m.sum[0] / (double)m.finite, m.sum[1] / (double)m.finite, m.sum[2] / (double)m.finite, std::sqrt((double)m.reach2_max));
        std::printf("\n");
        if (tint) {              // the selection as class 1 of the two-entry palette: shown at the next Render, no Sort
            if (!renderer.SetOverlayPalette(highlight, 2) || !renderer.SetOverlayDevice(static_cast<const uint8_t*>(mask), n)) return 1;
            if (depthPath) renderer.RenderWithDepth(cameraMat, projMat, viewport, nearFar, depth.data());
            else renderer.Render(cameraMat, projMat, viewport, nearFar);
            renderer.Synchronize();
            std::printf("the selection is highlighted\n");
        }
        renderer.Synchronize();
        dm.release(mask);
    }

    if (minAlpha >= 0.0f && inFlight == 1 && devices.size() <= 1) {
        const size_t n = cloud->GetNumGaussians();
        DeviceMemory dm;
        void *values = nullptr, *mask = nullptr;
        if (!dm.Load() || dm.alloc(&values, n * 4) != 0 || dm.alloc(&mask, n) != 0 || dm.fill(mask, 1, n) != 0 || dm.wait() != 0) return 1;
        float* v = static_cast<float*>(values);
        // the longest axis of every splat: the summary alone gives the range, a second call the 16 counts over it
        // (the printed edges are vmin + (vmax - vmin) b / 16 in fp32, for reading only: a value is counted by the library's rule,
        //  t = (v - lo) * scale, so a value within an ulp or two of a printed edge may sit in the neighbouring bin)
        msplat_value_summary sum;
        uint32_t counts[16] = {};
        if (!renderer.CloudValues(MSPLAT_VALUE_SCALE_MAX, nullptr, v, n) || !renderer.HistogramValues(v, nullptr, n, 0.0f, 0.0f, 0, nullptr, &sum)) return 1;
        std::printf("longest axis: %llu finite of %llu, %g .. %g (bin edges below are approximate)\n", (unsigned long long)sum.finite, (unsigned long long)sum.selected, sum.vmin, sum.vmax);
        if (sum.finite && sum.vmin < sum.vmax && renderer.HistogramValues(v, nullptr, n, sum.vmin, sum.vmax, 16, counts, &sum))
            for (int b = 0; b < 16; ++b)
                std::printf("  [%10.4g, %10.4g%c %u\n", sum.vmin + (sum.vmax - sum.vmin) * (float)b / 16.0f,
                            sum.vmin + (sum.vmax - sum.vmin) * (float)(b + 1) / 16.0f, b == 15 ? ']' : ')', counts[b]);
        // alpha < T: outside [T, +inf] (a NaN alpha goes too)
        if (!renderer.CloudValues(MSPLAT_VALUE_ALPHA, nullptr, v, n) ||
            !renderer.MarkValues(v, n, minAlpha, INFINITY, MSPLAT_RANGE_OUTSIDE, static_cast<uint8_t*>(mask), 0) ||
            !renderer.SetVisibilityDevice(static_cast<const uint8_t*>(mask), n))
            return 1;
        renderer.Sort(cameraMat, projMat, viewport, nearFar);
        if (depthPath) renderer.RenderWithDepth(cameraMat, projMat, viewport, nearFar, depth.data());
        else renderer.Render(cameraMat, projMat, viewport, nearFar);
        renderer.Synchronize();
        uint64_t hidden = 0;
        if (msplat_get_visibility(renderer.GetContext(), nullptr, nullptr, &hidden) != MSPLAT_OK) return 1;
        std::printf("min alpha %g: %llu of %zu splats hidden\n", minAlpha, (unsigned long long)hidden, n);
        dm.release(values);
        dm.release(mask);
    }

    if (minNeighbours > 0 && inFlight == 1 && devices.size() <= 1) {
        const size_t n = cloud->GetNumGaussians();
        DeviceMemory dm;
        void *values = nullptr, *mask = nullptr;
        if (!dm.Load() || dm.alloc(&values, n * 4) != 0 || dm.alloc(&mask, n) != 0 || dm.fill(mask, 1, n) != 0 || dm.wait() != 0) return 1;
        float* v = static_cast<float*>(values);
        // count up to K neighbours (a lane stops there), then hide the counts below K: inside [0, K - 1]
        msplat_neighbour_info info;
        if (!renderer.NeighbourValues(MSPLAT_NEAR_COUNT, neighbourRadius, nullptr, nullptr, n, (uint32_t)minNeighbours, 0, v, &info) ||
            !renderer.MarkValues(v, n, 0.0f, (float)(minNeighbours - 1), MSPLAT_RANGE_INSIDE, static_cast<uint8_t*>(mask), 0) ||
            !renderer.SetVisibilityDevice(static_cast<const uint8_t*>(mask), n))
            return 1;
        renderer.Sort(cameraMat, projMat, viewport, nearFar);
        if (depthPath) renderer.RenderWithDepth(cameraMat, projMat, viewport, nearFar, depth.data());
        else renderer.Render(cameraMat, projMat, viewport, nearFar);
        renderer.Synchronize();
        uint64_t hidden = 0;
        if (msplat_get_visibility(renderer.GetContext(), nullptr, nullptr, &hidden) != MSPLAT_OK) return 1;
        std::printf("fewer than %d neighbours within %g: %llu of %zu splats hidden (%u buckets, fullest %u, %llu candidate pairs)\n", minNeighbours,
                    neighbourRadius, (unsigned long long)hidden, n, info.buckets, info.max_bucket, (unsigned long long)info.tests);
        dm.release(values);
        dm.release(mask);
    }

    if (compact && devices.size() <= 1) {
        uint64_t kept = 0;
        if (!renderer.CompactCloud(nullptr, &kept)) return 1;
        std::printf("compacted: %zu -> %llu splats\n", cloud->GetNumGaussians(), (unsigned long long)kept);
        if (overGradient)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    float* px = &fb[((size_t)y * W + x) * 4];
                    px[0] = 0.1f; px[1] = 0.2f; px[2] = 0.2f + 0.6f * (float)y / (float)H; px[3] = 1.0f;
                }
        renderer.Sort(cameraMat, projMat, viewport, nearFar);
        if (depthPath) renderer.RenderWithDepth(cameraMat, projMat, viewport, nearFar, depth.data());
        else renderer.Render(cameraMat, projMat, viewport, nearFar);
        renderer.Synchronize();
    }

    if (savePath && devices.size() <= 1) {
        if (!renderer.ExportPly(savePath)) return 1;
        std::printf("saved the cloud on the device to %s\n", savePath);
    }

    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 1;
    std::fwrite(fb.data(), sizeof(float), fb.size(), f);
    std::fclose(f);
    if (depthPath) {
        FILE* fz = std::fopen(depthPath, "wb");
        if (!fz) return 1;
        std::fwrite(depth.data(), sizeof(float), depth.size(), fz);
        std::fclose(fz);
    }
    std::printf("%zu splats -> %dx%d RGBA32F (row 0 = bottom) written to %s\n", cloud->GetNumGaussians(), W, H, argv[2]);
    return 0;
}
