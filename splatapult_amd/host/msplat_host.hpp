// msplat_host.hpp -- C++ drop-in shim: the reference's SplatRenderer class surface
// (/root/reference/src/splatrenderer.h:23-67) on top of the C ABI in include/msplat.h.
//
//   bool Init(std::shared_ptr<GaussianCloud>, bool isFramebufferSRGBEnabled, bool useRgcSortOverride);
//   void Sort  (cameraMat, projMat, viewport, nearFar);
//   void Render(cameraMat, projMat, viewport, nearFar);
//
// Matrix/vector arguments are templated on anything that is laid out like glm's types (a mat4 is
// 16 contiguous column-major floats, vec4/vec2 are 4/2 floats): glm::mat4, glm::vec4, glm::vec2 or
// the msplat::mat4/vec4/vec2 PODs below all work unchanged, so App::Render's two call sites
// (app.cpp:603-607, :1067-1068) compile as they are.
//
// The reference draws into "whatever GL framebuffer is bound"; here the target is explicit:
// SetRenderTarget(ptr, pitch, isDevice) once (or per frame), then Render writes RGBA32F / 16F / 8-bit rows,
// row 0 = GL bottom row, alpha = 1.
#pragma once

#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/msplat.h"
#include "../../include/msplat_debug.h"
#include "gaussian_scene.hpp"
#include "point_scene.hpp"

namespace msplat {
struct mat4 { float m[16]; };   // column-major, m[col*4 + row]
struct vec4 { float v[4]; };
struct vec2 { float v[2]; };
}  // namespace msplat

class SplatRenderer
{
public:
    SplatRenderer() = default;
    ~SplatRenderer() { DestroyContexts(); }
    SplatRenderer(const SplatRenderer&) = delete;
    SplatRenderer& operator=(const SplatRenderer&) = delete;

    // optional, before Init: device ordinal, framebuffer format (MSPLAT_FB_*: RGBA32F, RGBA16F, or the 4-byte RGBA8 / SRGB8_ALPHA8 --
    // INTEGRATION.md 15; the render target then holds bytes R G B A), stream (hipStream_t)
    void Configure(int device, int fbFormat, void* stream = nullptr, float tEpsilon = -1.0f)
    {
        cfg.device = device;
        cfg.fb_format = fbFormat;
        cfg.stream = stream;
        cfg.t_epsilon = tEpsilon;
    }

    // optional, before Init: render on several GPUs from this one process (msplat_group_* in msplat.h).  The
    // cloud is replicated, the screen's bin rows are partitioned over `devices` (MSPLAT_BANDS_*: contiguous bands by
    // default) and every device writes its rows into the render target, which must be host memory or memory of
    // devices[0] (the other devices reach it through the xGMI peer mapping).  Sort / Render are unchanged.
    // bandCull: Sort also drops splats that cannot reach a device's rows (mono rendering only: every Render must use its
    // Sort's camera).  Frames in flight are not combined with a device group.
    void ConfigureDevices(const std::vector<int>& devicesIn, int bandKind = MSPLAT_BANDS_CONTIGUOUS, int blockRows = 1,
                          bool bandCull = false)
    {
        groupDevices.assign(devicesIn.begin(), devicesIn.end());
        groupKind = bandKind;
        groupBlockRows = blockRows;
        groupBandCull = bandCull;
    }

    // optional, before Init, with ConfigureDevices: how the other devices' rows reach devices[0]'s render target --
    // MSPLAT_EXCHANGE_PEER_STORE (default: their compositors store through the peer mapping), MSPLAT_EXCHANGE_RCCL (grouped
    // ncclSend / ncclRecv over communicators from ncclCommInitAll) or MSPLAT_EXCHANGE_COPY.  Not available (RCCL missing, a
    // device listed twice): logged, the group keeps its previous exchange.
    void SetGroupExchange(int exchange) { groupExchange = exchange; }

    // One process per GPU (the other multi-GPU shape): this process renders the bin rows of rank `rank` of `world`
    // (msplat_band_plan's layouts) and, after Render into a device target, ExchangeBands() gathers every rank's rows into rank
    // `root`'s target with ONE group of ncclSend / ncclRecv on the context's stream (msplat_band_exchange; `comm` = the host's
    // ncclComm_t).  Call SetBandPlan after Init.
    bool SetBandPlan(int rank, int world, int rowsFull, int bandKind = MSPLAT_BANDS_CONTIGUOUS, int blockRows = 1, bool bandCull = false)
    {
        int32_t first = 0, count = 0, block = 1, stride = 1;
        if (msplat_band_plan(bandKind, rowsFull, world, rank, blockRows, &first, &count, &block, &stride) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] SetBandPlan: %s\n", msplat_last_error(nullptr));
            return false;
        }
        bandRank = rank; bandWorld = world; bandKindSet = bandKind; bandBlockRows = blockRows;
        for (msplat_ctx* h : ctxs)
            if (msplat_set_band_layout(h, first, count, block, stride) != MSPLAT_OK || msplat_set_band_cull(h, bandCull ? 1 : 0) != MSPLAT_OK) {
                std::fprintf(stderr, "[msplat][E] SetBandPlan: %s\n", msplat_last_error(h));
                return false;
            }
        return true;
    }
    bool ExchangeBands(void* comm, int root, int width, int height, int flags = 0)        // flags: MSPLAT_EXCHANGE_WIRE_FP16
    {
        if (!ctx || !targetIsDevice || !target) return false;
        const uint64_t pitch = targetPitch ? targetPitch : (uint64_t)width * MSPLAT_FB_BYTES_PER_PIXEL(cfg.fb_format);
        const int rc = msplat_band_exchange(ctx, comm, bandRank, bandWorld, root, bandKindSet, bandBlockRows, target, pitch, width, height, flags);
        if (rc != MSPLAT_OK) std::fprintf(stderr, "[msplat][E] ExchangeBands: %s\n", msplat_group_last_error(nullptr));
        return rc == MSPLAT_OK;
    }

    // optional, before Init: number of frames in flight (default 1).  With depth > 1 every Sort moves on to
    // the next of `depth` contexts (own stream + per-frame buffers, one shared cloud), so successive frames
    // overlap on the GPU the way a GL driver overlaps queued frames; the following Render(s) use the context
    // of the latest Sort.  Each context creates its own stream (a stream given to Configure is only used
    // with depth 1): use WaitOnStream / Synchronize before consuming a frame, and one render target per
    // frame in flight.
    void SetFramesInFlight(int depth) { framesInFlight = depth < 1 ? 1 : depth; }

    // msplat_config.two_pass (before Init): MSPLAT_TWO_PASS_AUTO (default) / _ON / _OFF -- Render in two passes with occlusion
    // feedback, the same pixels (include/msplat.h).  TwoPassInfo: what the current context's latest two-pass Render did
    // (msplat_get_two_pass_info; out[0] == 0: it ran in one pass).
    void SetTwoPass(int mode) { cfg.two_pass = mode; }
    bool TwoPassInfo(uint64_t out[8]) const { return ctx != nullptr && msplat_get_two_pass_info(ctx, out) == MSPLAT_OK; }

    // msplat_set_cloud_storage (before Init; also on the ConfigureDevices path): MSPLAT_STORAGE_FP32 (default) or
    // MSPLAT_STORAGE_SH_FP16 -- f_rest stored as IEEE fp16, pixels equal to an FP32 render of the fp16-rounded cloud (msplat.h)
    // or MSPLAT_STORAGE_SH_Q8 -- f_rest as 8-bit codes with a step per SH band, one 128-B record per splat (full-SH clouds only)
    void SetCloudStorage(int storage) { cloudStorage = storage; }

    // splatrenderer.cpp:50-151.  false after logging on failure.  The cloud is copied to the device and
    // not retained; useRgcSortOverride is accepted and ignored (one HIP sort replaces both GL sorters).
    bool Init(std::shared_ptr<GaussianCloud> gaussianCloud, bool isFramebufferSRGBEnabledIn, bool useRgcSortOverrideIn)
    {
        (void)useRgcSortOverrideIn;
        DestroyContexts();
        cfg.struct_size = sizeof(cfg);
        cfg.srgb = isFramebufferSRGBEnabledIn ? 1 : 0;
        if (groupDevices.size() > 1) return InitGroup(*gaussianCloud);
        if (!CreateContexts()) return false;
        msplat_attr_offsets off{};
        off.pos_with_alpha = (uint32_t)gaussianCloud->GetPosWithAlphaAttrib().offset;
        off.r_sh0 = (uint32_t)gaussianCloud->GetR_SH0Attrib().offset;
        off.g_sh0 = (uint32_t)gaussianCloud->GetG_SH0Attrib().offset;
        off.b_sh0 = (uint32_t)gaussianCloud->GetB_SH0Attrib().offset;
        off.cov3_col0 = (uint32_t)gaussianCloud->GetCov3_Col0Attrib().offset;
        off.cov3_col1 = (uint32_t)gaussianCloud->GetCov3_Col1Attrib().offset;
        off.cov3_col2 = (uint32_t)gaussianCloud->GetCov3_Col2Attrib().offset;
        if (gaussianCloud->HasFullSH()) {
            off.r_sh1 = (uint32_t)gaussianCloud->GetR_SH1Attrib().offset;
            off.r_sh2 = (uint32_t)gaussianCloud->GetR_SH2Attrib().offset;
            off.r_sh3 = (uint32_t)gaussianCloud->GetR_SH3Attrib().offset;
            off.g_sh1 = (uint32_t)gaussianCloud->GetG_SH1Attrib().offset;
            off.g_sh2 = (uint32_t)gaussianCloud->GetG_SH2Attrib().offset;
            off.g_sh3 = (uint32_t)gaussianCloud->GetG_SH3Attrib().offset;
            off.b_sh1 = (uint32_t)gaussianCloud->GetB_SH1Attrib().offset;
            off.b_sh2 = (uint32_t)gaussianCloud->GetB_SH2Attrib().offset;
            off.b_sh3 = (uint32_t)gaussianCloud->GetB_SH3Attrib().offset;
        }
        if (msplat_upload_cloud(ctx, gaussianCloud->GetRawDataPtr(), gaussianCloud->GetNumGaussians(),
                                (uint32_t)gaussianCloud->GetStride(), &off, gaussianCloud->HasFullSH() ? 1 : 0) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] %s\n", msplat_last_error(ctx));
            return false;
        }
        return AttachContexts();
    }

    // Init from a cloud that is already in device memory (msplat_upload_cloud_device / msplat_upload_attributes_device):
    // contexts as Init creates them -- SetFramesInFlight and SetCloudStorage are honoured -- and the cloud read from the caller's
    // device memory on context 0's stream; on return the source may be overwritten or freed.  Whatever produced it must have
    // completed.  Not with ConfigureDevices of more than one device (a replicated cloud needs peer copies): false after logging.
    bool InitDevice(const void* dRecords, uint64_t n, uint32_t strideBytes, const msplat_attr_offsets& off, bool fullSH,
                    bool isFramebufferSRGBEnabledIn)
    {
        return InitDeviceWith("InitDevice", isFramebufferSRGBEnabledIn,
                              [&] { return msplat_upload_cloud_device(ctx, dRecords, n, strideBytes, &off, fullSH ? 1 : 0); });
    }
    // the arrays of msplat_cloud_from_attributes in device memory; dFRest may be NULL (SH degree 0)
    bool InitDeviceAttributes(uint64_t n, const float* dXyz, const float* dFDc, const float* dFRest, const float* dOpacity,
                              const float* dLogScale, const float* dRot, bool fullSH, bool isFramebufferSRGBEnabledIn)
    {
        return InitDeviceWith("InitDeviceAttributes", isFramebufferSRGBEnabledIn, [&] {
            return msplat_upload_attributes_device(ctx, n, dXyz, dFDc, dFRest, dOpacity, dLogScale, dRot, fullSH ? 1 : 0);
        });
    }

    // splatrenderer.cpp:153-312
    template <class Mat4, class Vec4, class Vec2>
    void Sort(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar)
    {
        static_assert(sizeof(Mat4) == 64 && sizeof(Vec4) == 16 && sizeof(Vec2) == 8, "glm-compatible layout expected");
        if (group) {
            const int grc = msplat_group_sort(group, reinterpret_cast<const float*>(&cameraMat), reinterpret_cast<const float*>(&projMat),
                                              reinterpret_cast<const float*>(&viewport), reinterpret_cast<const float*>(&nearFar));
            if (grc != MSPLAT_OK) std::fprintf(stderr, "[msplat][%c] Sort: %s\n", Level(grc), msplat_group_last_error(group));
            return;
        }
        if (ctxs.empty()) return;
        cur = (cur + 1) % (int)ctxs.size();
        ctx = ctxs[cur];
        const int rc = msplat_sort(ctx, reinterpret_cast<const float*>(&cameraMat), reinterpret_cast<const float*>(&projMat),
                                   reinterpret_cast<const float*>(&viewport), reinterpret_cast<const float*>(&nearFar));
        if (rc != MSPLAT_OK)         // void, like the reference
            std::fprintf(stderr, "[msplat][%c] Sort: %s\n", Level(rc), msplat_last_error(ctx));
    }

    // splatrenderer.cpp:315-343 (+ the GL pipeline behind glDrawElements)
    template <class Mat4, class Vec4, class Vec2>
    void Render(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar)
    {
        RenderCall<Mat4, Vec4, Vec2>("Render", target != nullptr, "no render target set (SetRenderTarget)", nullptr, [&] {
            return group ? msplat_group_render(group, F(cameraMat), F(projMat), F(viewport), F(nearFar), target, targetPitch, targetIsDevice ? 1 : 0)
                         : msplat_render(ctx, F(cameraMat), F(projMat), F(viewport), F(nearFar), target, targetPitch, targetIsDevice ? 1 : 0);
        });
    }

    // Render plus the per-pixel depth plane (msplat_render_depth): W x H float32 rows of depthPitchBytes (0 = tight) in the render
    // target's memory space -- the splats' expected window depth over the clear depth 1.0, for compositing the layer with geometry
    // or as an XR depth layer.  Uses the context of the latest Sort, like Render.  A device group has no depth output.
    template <class Mat4, class Vec4, class Vec2>
    void RenderWithDepth(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar, float* depth,
                         uint64_t depthPitchBytes = 0)
    {
        RenderCall<Mat4, Vec4, Vec2>("RenderWithDepth", target && depth, "no render target set (SetRenderTarget) or no depth plane",
                                     "a device group has no depth output", [&] {
            return msplat_render_depth(ctx, F(cameraMat), F(projMat), F(viewport), F(nearFar), target, targetPitch, depth, depthPitchBytes,
                                       targetIsDevice ? 1 : 0);
        });
    }

    // Render behind the caller's geometry (msplat_render_occluded): `occluder` = W x H float32 window depths, rows of pitchBytes (0 = tight)
    // in the render target's memory space, e.g. the depth attachment of the mesh pass -- GL_LESS, as app.cpp:160-163 sets it: a splat with
    // !(z_w < occluder) at a pixel is not blended there.  Read-only; with a device target it must stay valid until the frame has run.
    // Uses the context of the latest Sort, like Render.  A device group takes no occluder plane.
    template <class Mat4, class Vec4, class Vec2>
    void RenderOccluded(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar, const float* occluder,
                        uint64_t pitchBytes = 0)
    {
        RenderCall<Mat4, Vec4, Vec2>("RenderOccluded", target && occluder, "no render target set (SetRenderTarget) or no occluder plane",
                                     "a device group takes no occluder plane", [&] {
            return msplat_render_occluded(ctx, F(cameraMat), F(projMat), F(viewport), F(nearFar), target, targetPitch, occluder, pitchBytes,
                                          targetIsDevice ? 1 : 0);
        });
    }

    // RenderOccluded and RenderWithDepth in one frame (msplat_render_layers): the colour behind the caller's geometry plus the depth
    // layer of the result -- the splats that pass the test over the occluder's values clamped to [0, 1].  Either plane may be NULL
    // (the call without it); `depth` may be the occluder's own memory with the same pitch: a depth attachment read and written in
    // place.  Uses the context of the latest Sort, like Render.  A device group has no layers frame.
    template <class Mat4, class Vec4, class Vec2>
    void RenderLayers(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar, float* depth,
                      uint64_t depthPitchBytes, const float* occluder, uint64_t occluderPitchBytes)
    {
        RenderCall<Mat4, Vec4, Vec2>("RenderLayers", target != nullptr, "no render target set (SetRenderTarget)",
                                     "a device group has no layers frame", [&] {
            return msplat_render_layers(ctx, F(cameraMat), F(projMat), F(viewport), F(nearFar), target, targetPitch, depth, depthPitchBytes,
                                        occluder, occluderPitchBytes, targetIsDevice ? 1 : 0);
        });
    }

    // RenderStereo with RenderLayers' planes per eye (msplat_render_stereo_layers): the reference's XR frame -- geometry first, the
    // splats blended over it under GL_LESS, per eye (app.cpp:570-607) -- in one chain of launches for device targets.  depth0 / depth1
    // are both given or both NULL, and so are occluder0 / occluder1; each kind's pitch is shared by the eyes.
    template <class Mat4, class Vec4, class Vec2>
    void RenderStereoLayers(const Mat4& cameraMat0, const Mat4& projMat0, const Mat4& cameraMat1, const Mat4& projMat1, const Vec4& viewport,
                            const Vec2& nearFar, void* target1, float* depth0, float* depth1, uint64_t depthPitchBytes,
                            const float* occluder0, const float* occluder1, uint64_t occluderPitchBytes)
    {
        RenderCall<Mat4, Vec4, Vec2>("RenderStereoLayers", target && target1, "no render target set (SetRenderTarget / target1)",
                                     "a device group has no layers frame", [&] {
            return msplat_render_stereo_layers(ctx, F(cameraMat0), F(projMat0), F(cameraMat1), F(projMat1), F(viewport), F(nearFar), target,
                                               target1, targetPitch, depth0, depth1, depthPitchBytes, occluder0, occluder1,
                                               occluderPitchBytes, targetIsDevice ? 1 : 0);
        });
    }

    // Both eyes of the latest Sort in one chain of launches (msplat_render_stereo): what the XR callback does with two Render
    // calls (app.cpp:603-607), for device targets at half the launches.  target1: the second eye's image (same pitch / kind as
    // the SetRenderTarget one, which receives the first eye).
    template <class Mat4, class Vec4, class Vec2>
    void RenderStereo(const Mat4& cameraMat0, const Mat4& projMat0, const Mat4& cameraMat1, const Mat4& projMat1, const Vec4& viewport,
                      const Vec2& nearFar, void* target1)
    {
        if (group && target && target1) {         // a device group renders its rows per view
            Render(cameraMat0, projMat0, viewport, nearFar);
            void* keep = target;
            target = target1;
            Render(cameraMat1, projMat1, viewport, nearFar);
            target = keep;
            return;
        }
        RenderCall<Mat4, Vec4, Vec2>("RenderStereo", target && target1, "no render target set (SetRenderTarget / target1)", nullptr, [&] {
            return msplat_render_stereo(ctx, F(cameraMat0), F(projMat0), F(cameraMat1), F(projMat1), F(viewport), F(nearFar), target, target1,
                                        targetPitch, targetIsDevice ? 1 : 0);
        });
    }

    // replaces "the currently bound GL framebuffer" (app.cpp:1000-1035)
    void SetRenderTarget(void* rgba, uint64_t pitchBytes, bool isDevicePointer)
    {
        target = rgba;
        targetPitch = pitchBytes;
        targetIsDevice = isDevicePointer;
    }

    // emulated depth buffer for targets that have one in the GL app (app.cpp:163; 24 = default back buffer)
    void SetDepthTest(int depthBits)
    {
        for (msplat_ctx* h : ctxs) msplat_set_depth_test(h, depthBits);
    }

    // the blend as the GL app's own render target performs it (MSPLAT_ROP_RGBA8: default back buffer, MSPLAT_ROP_RGBA16F: --fp16)
    void SetTargetEmulation(int rop)
    {
        for (msplat_ctx* h : ctxs) msplat_set_target_emulation(h, rop);
    }

    // what Render does with the render target's contents (msplat_set_target_mode; after Init, on every context of the rotation):
    // MSPLAT_TARGET_CLEAR (default) overwrites with (C, 1); MSPLAT_TARGET_LOAD blends the splats over what the target holds -- the
    // reference's Render, which never clears (app.cpp:154-156,1046-1068); MSPLAT_TARGET_PREMULTIPLIED writes the layer (C, 1 - T).
    // A device group takes CLEAR and PREMULTIPLIED.
    bool SetTargetMode(int mode)
    {
        if (group && msplat_group_set_target_mode(group, mode) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] SetTargetMode: %s\n", msplat_group_last_error(group));
            return false;
        }
        for (msplat_ctx* h : ctxs)
            if (msplat_set_target_mode(h, mode) != MSPLAT_OK) {
                std::fprintf(stderr, "[msplat][E] SetTargetMode: %s\n", msplat_last_error(h));
                return false;
            }
        return true;
    }

    // per-splat visibility (msplat_set_visibility / msplat_set_crop; after Init, on every context of the rotation): for the following
    // Sorts splat i (upload numbering) takes part iff visible[i] != 0 and the crop keeps it; nullptr = no mask.  An upload drops the
    // mask and keeps the crop.  A device group has no visibility (out of scope): false.
    bool SetVisibility(const uint8_t* visible, size_t n) { return SetMask(visible, n, false); }
    // the mask in memory of the renderer's device: read asynchronously on each context's stream, valid until Synchronize()
    bool SetVisibilityDevice(const uint8_t* d_visible, size_t n) { return SetMask(d_visible, n, true); }
    // render-time overlay (msplat_set_overlay* / msplat_set_overlay_palette; on every context of the rotation): splat i (upload numbering)
    // of class classes[i] = k is shown tinted by palette entry k = (h_r, h_g, h_b, a), lane by lane c' = (1 - a) c + a h; a class >= count
    // or an entry with a == 0 has no effect; nullptr = no classes.  Shows at the next Render, no Sort needed.  Set the classes after Init;
    // an upload and CompactCloud drop them, TransformCloud / AppendCloud keep context 0's and drop those of the contexts they attach again:
    // with frames in flight call SetOverlay[Device] again afterwards.  A device group has no overlay (out of scope): false.
    bool SetOverlay(const uint8_t* classes, size_t n) { return SetClasses(classes, n, false); }
    // the classes in memory of the renderer's device (what MarkIds / MarkScores wrote): read asynchronously on each context's stream, valid until Synchronize()
    bool SetOverlayDevice(const uint8_t* d_classes, size_t n) { return SetClasses(d_classes, n, true); }
    // count <= 256 entries of 4 floats; nullptr or 0 = no palette.  May come before Init: it is kept and handed to every context created later
    bool SetOverlayPalette(const float* rgba, uint32_t count)
    {
        if (group) {
            std::fprintf(stderr, "[msplat][E] SetOverlayPalette: a device group has no overlay\n");
            return false;
        }
        if (!rgba) count = 0;
        for (msplat_ctx* h : ctxs)
            if (msplat_set_overlay_palette(h, rgba, count) != MSPLAT_OK) {
                std::fprintf(stderr, "[msplat][E] SetOverlayPalette: %s\n", msplat_last_error(h));
                return false;
            }
        overlayPalette.assign(rgba, rgba + 4 * (size_t)count);
        return true;
    }
    // crop volume: worldToCrop (column-major, affine) and MSPLAT_CROP_BOX / _SPHERE, | MSPLAT_CROP_INVERT; nullptr or MSPLAT_CROP_NONE = none
    bool SetCrop(const float* worldToCrop, int shape)
    {
        if (group) {
            std::fprintf(stderr, "[msplat][E] SetCrop: a device group has no per-splat visibility\n");
            return false;
        }
        for (msplat_ctx* h : ctxs)
            if (msplat_set_crop(h, worldToCrop, shape) != MSPLAT_OK) {
                std::fprintf(stderr, "[msplat][E] SetCrop: %s\n", msplat_last_error(h));
                return false;
            }
        return true;
    }

    // Makes the mask and the crop permanent, on the device (msplat_compact_cloud): the cloud becomes the K splats they let through,
    // renumbered 0..K-1 in ascending old index, records copied bit for bit -- the renderer afterwards is one Init'ed with those rows.
    // d_index_map (may be nullptr): the old N uint32 of device memory, [i] = new index of splat i or MSPLAT_ID_NONE.  Every frame in
    // flight is finished first; context 0 is compacted, the others are attached again and the next Sort lands on context 0, as after
    // InitDevice.  The masks of all contexts are gone, the crop stays; Sort before the next Render.  *kept (may be nullptr) = K.
    bool CompactCloud(uint32_t* d_index_map = nullptr, uint64_t* kept = nullptr)
    {
        if (group || ctxs.empty()) {
            std::fprintf(stderr, "[msplat][E] CompactCloud: %s\n", group ? "a device group has no per-splat visibility" : "no cloud (Init first)");
            return false;
        }
        Synchronize();
        ctx = ctxs[0];
        cur = (int)ctxs.size() - 1;           // the next Sort lands on context 0
        if (msplat_compact_cloud(ctx, d_index_map, kept) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] CompactCloud: %s\n", msplat_last_error(ctx));
            return false;
        }
        return AttachContexts();
    }

    // Moves, rotates and scales splats on the device (msplat_transform_cloud): every splat i with d_select[i] != 0 (n bytes of device
    // memory; nullptr: every splat) gets centre M x, covariance A S A^T and, unless keepSH, SH bands 1..3 rotated by msplat_sh_rotation(M);
    // the others are copied bit for bit.  Without keepSH M must be a rotation times a uniform positive scale.  Every frame in flight is
    // finished first; context 0 is transformed and keeps its mask (the numbering does not change), the others are attached again, which
    // drops THEIR masks: with frames in flight call SetVisibility[Device] again afterwards.  The crop stays; Sort before the next Render.
    template <class Mat4>
    bool TransformCloud(const Mat4& M, const uint8_t* d_select = nullptr, bool keepSH = false)
    {
        static_assert(sizeof(Mat4) == 64, "glm-compatible layout expected");
        if (group || ctxs.empty()) {
            std::fprintf(stderr, "[msplat][E] TransformCloud: %s\n", group ? "a device group has no cloud editing" : "no cloud (Init first)");
            return false;
        }
        Synchronize();
        ctx = ctxs[0];
        cur = (int)ctxs.size() - 1;           // the next Sort lands on context 0
        msplat_stats st;
        if (msplat_get_stats(ctx, &st) != MSPLAT_OK ||
            msplat_transform_cloud(ctx, F(M), d_select, st.num_splats, keepSH ? MSPLAT_TRANSFORM_KEEP_SH : 0) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] TransformCloud: %s\n", msplat_last_error(ctx));
            return false;
        }
        return AttachContexts();
    }

    // Puts splats into the cloud on the device (msplat_append_cloud): every splat i of src's cloud (another renderer on this device,
    // or this one: a duplicate) with d_select[i] != 0 (one byte per splat of src in device memory; nullptr: every splat) is appended
    // behind this renderer's own in ascending source index; the old splats keep their indices, the K new ones get N..N+K-1.  Rows are
    // copied bit for bit where both clouds are stored alike and converted through their FP32 values where not.  d_index_map (may be
    // nullptr): src's Ns uint32 of device memory, [i] = new index of source splat i or MSPLAT_ID_NONE; *added (may be nullptr) = K.
    // Every frame in flight of both renderers is finished first; context 0 appends and keeps its mask, K visible bytes longer, the
    // others are attached again, which drops THEIR masks: with frames in flight call SetVisibility[Device] again afterwards.  The crop
    // stays; Sort before the next Render.
    bool AppendCloud(SplatRenderer& src, const uint8_t* d_select = nullptr, uint32_t* d_index_map = nullptr, uint64_t* added = nullptr)
    {
        if (group || src.group || ctxs.empty() || src.ctxs.empty()) {
            std::fprintf(stderr, "[msplat][E] AppendCloud: %s\n", group || src.group ? "a device group has no cloud editing" : "no cloud (Init first)");
            return false;
        }
        Synchronize();
        if (&src != this) src.Synchronize();
        ctx = ctxs[0];
        cur = (int)ctxs.size() - 1;           // the next Sort lands on context 0
        msplat_stats st;
        if (msplat_get_stats(src.ctxs[0], &st) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] AppendCloud: %s\n", msplat_last_error(src.ctxs[0]));
            return false;
        }
        if (msplat_append_cloud(ctx, src.ctxs[0], d_select, st.num_splats, d_index_map, added) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] AppendCloud: %s\n", msplat_last_error(ctx));
            return false;
        }
        return AttachContexts();
    }

    // Recolours and fades splats on the device (msplat_adjust_cloud): every splat i with d_select[i] != 0 (n bytes of device memory;
    // nullptr: every splat) gets, with colour != nullptr, the affine map col' = G col + o of its colour in every view direction
    // (12 floats, column-major: G's three columns, then o; applied to the SH coefficients, in the record's colour space) and, with
    // opacityScale >= 0, alpha' = clamp(opacityScale * alpha, 0, 1); the others are copied bit for bit, and a part that is not asked
    // for keeps its bits.  Every frame in flight is finished first; context 0 is adjusted and keeps its mask and overlay classes (the
    // numbering does not change), the others are attached again, which drops THEIRS: with frames in flight call
    // SetVisibility[Device] / SetOverlay[Device] again afterwards.  The crop stays; Sort before the next Render.
    bool AdjustCloud(const float* colour, float opacityScale = -1.0f, const uint8_t* d_select = nullptr)
    {
        if (group || ctxs.empty()) {
            std::fprintf(stderr, "[msplat][E] AdjustCloud: %s\n", group ? "a device group has no cloud editing" : "no cloud (Init first)");
            return false;
        }
        Synchronize();
        ctx = ctxs[0];
        cur = (int)ctxs.size() - 1;           // the next Sort lands on context 0
        const int32_t flags = (colour ? MSPLAT_ADJUST_COLOUR : 0) | (opacityScale >= 0.0f ? MSPLAT_ADJUST_OPACITY : 0);
        msplat_stats st;
        if (msplat_get_stats(ctx, &st) != MSPLAT_OK || msplat_adjust_cloud(ctx, colour, opacityScale, d_select, st.num_splats, flags) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] AdjustCloud: %s\n", msplat_last_error(ctx));
            return false;
        }
        return AttachContexts();
    }

    // The cloud out of the device (msplat_export_ply, msplat_download_cloud_device, msplat_download_attributes_device): as it is on the
    // device -- moved, pasted into, compacted --, upload numbering, the mask and the crop ignored; nothing of the renderer changes.
    // ExportPly writes the PLY GaussianCloud::ExportPly writes; DownloadDevice N tight reference records (244 B with full SH, 100 B
    // without) at d_aos (16-byte aligned, capBytes large): what InitDevice takes with the reference offsets; DownloadDeviceAttributes
    // the six arrays InitDeviceAttributes takes (n = the cloud's N; d_f_rest may be nullptr).  A device group has no download.
    bool ExportPly(const std::string& plyFilename) { return Download("ExportPly", [&](msplat_ctx* h) { return msplat_export_ply(h, plyFilename.c_str()); }); }
    bool DownloadDevice(void* d_aos, uint64_t capBytes) { return Download("DownloadDevice", [&](msplat_ctx* h) { return msplat_download_cloud_device(h, d_aos, capBytes); }); }
    bool DownloadDeviceAttributes(uint64_t n, float* d_xyz, float* d_f_dc, float* d_f_rest, float* d_opacity, float* d_log_scale, float* d_rot)
    {
        return Download("DownloadDeviceAttributes", [&](msplat_ctx* h) { return msplat_download_attributes_device(h, n, d_xyz, d_f_dc, d_f_rest, d_opacity, d_log_scale, d_rot); });
    }
    template <class Call>
    bool Download(const char* who, Call&& call)
    {
        if (group || !ctx) {
            std::fprintf(stderr, "[msplat][E] %s: %s\n", who, group ? "a device group has no download" : "no cloud (Init first)");
            return false;
        }
        const int rc = call(ctx);
        if (rc != MSPLAT_OK) std::fprintf(stderr, "[msplat][E] %s: %s\n", who, msplat_last_error(ctx));
        return rc == MSPLAT_OK;
    }

    // Which splat each pixel shows (msplat_render_ids): per pixel of window = {x0, y0, w, h} (viewport pixels, row 0 = GL bottom; nullptr =
    // the whole viewport) the upload index of the splat of the latest Sort that contributes most to it, MSPLAT_ID_NONE where none
    // reaches; idDepth (may be nullptr) = that splat's window depth, 1.0 at MSPLAT_ID_NONE.  Both planes are w x h of the WINDOW, rows
    // of their pitch (0 = tight), in host or device memory alike (isDevicePointer).  Needs no render target.  A device group has no id frame.
    template <class Mat4, class Vec4, class Vec2>
    bool RenderIds(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar, const int32_t* window, uint32_t* ids,
                   uint64_t idsPitchBytes = 0, float* idDepth = nullptr, uint64_t idDepthPitchBytes = 0, bool isDevicePointer = false)
    {
        static_assert(sizeof(Mat4) == 64 && sizeof(Vec4) == 16 && sizeof(Vec2) == 8, "glm-compatible layout expected");
        if (group || !ctx) {
            std::fprintf(stderr, "[msplat][E] RenderIds: %s\n", group ? "a device group has no id frame" : "no cloud (Init first)");
            return false;
        }
        const int rc = msplat_render_ids(ctx, F(cameraMat), F(projMat), F(viewport), F(nearFar), window, ids, idsPitchBytes, idDepth,
                                         idDepthPitchBytes, isDevicePointer ? 1 : 0);
        if (rc != MSPLAT_OK) std::fprintf(stderr, "[msplat][%c] RenderIds: %s\n", Level(rc), msplat_last_error(ctx));
        return rc == MSPLAT_OK || rc == MSPLAT_ERR_PAIR_OVERFLOW_EARLIER;
    }
    // the splat under pixel (x, y) of the viewport: RenderIds through a 1 x 1 window.  *index = MSPLAT_ID_NONE, *zw = 1.0 where none reaches
    template <class Mat4, class Vec4, class Vec2>
    bool Pick(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar, int x, int y, uint32_t* index, float* zw = nullptr)
    {
        const int32_t window[4] = {x, y, 1, 1};
        return RenderIds(cameraMat, projMat, viewport, nearFar, window, index, 0, zw, 0, false);
    }
    // d_mask[id] = value for every pixel of the w x h id plane d_ids that d_region selects (nonzero byte; nullptr = every pixel) and whose
    // id is a splat (msplat_mark_ids).  Device memory only; d_mask: one byte per splat, what SetVisibilityDevice takes.  Asynchronous on
    // the stream of the latest Sort's context, behind the RenderIds that wrote the plane.
    bool MarkIds(const uint32_t* d_ids, uint64_t idsPitchBytes, uint32_t w, uint32_t h, uint8_t* d_mask, size_t n, uint8_t value,
                 const uint8_t* d_region = nullptr, uint64_t regionPitchBytes = 0)
    {
        if (group || !ctx) {
            std::fprintf(stderr, "[msplat][E] MarkIds: %s\n", group ? "a device group has no per-splat visibility" : "no cloud (Init first)");
            return false;
        }
        if (msplat_mark_ids(ctx, d_ids, idsPitchBytes, w, h, d_region, regionPitchBytes, d_mask, n, value) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] MarkIds: %s\n", msplat_last_error(ctx));
            return false;
        }
        return true;
    }
    // How much of the frame each splat contributes (msplat_render_scores): d_score[i] += the sum over the pixels of window (nullptr = the
    // whole viewport) that d_region selects (nonzero byte of a w x h plane of the window; nullptr = all) of rint(T_i w_i 2^23), i in upload
    // numbering; MSPLAT_SCORE_ONE is one fully covered pixel; d_pixels (may be nullptr) += the number of those pixels with a nonzero term.
    // Device memory only, n = the cloud's splats; the arrays are accumulated into: zero them first, call once per camera to sum over views.
    // Asynchronous on the stream of the latest Sort's context.  A device group has no score frame.
    template <class Mat4, class Vec4, class Vec2>
    bool RenderScores(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar, const int32_t* window,
                      uint64_t* d_score, size_t n, uint32_t* d_pixels = nullptr, const uint8_t* d_region = nullptr, uint64_t regionPitchBytes = 0)
    {
        static_assert(sizeof(Mat4) == 64 && sizeof(Vec4) == 16 && sizeof(Vec2) == 8, "glm-compatible layout expected");
        if (group || !ctx) {
            std::fprintf(stderr, "[msplat][E] RenderScores: %s\n", group ? "a device group has no score frame" : "no cloud (Init first)");
            return false;
        }
        const int rc = msplat_render_scores(ctx, F(cameraMat), F(projMat), F(viewport), F(nearFar), window, d_region, regionPitchBytes, d_score,
                                            d_pixels, n);
        if (rc != MSPLAT_OK) std::fprintf(stderr, "[msplat][%c] RenderScores: %s\n", Level(rc), msplat_last_error(ctx));
        return rc == MSPLAT_OK || rc == MSPLAT_ERR_PAIR_OVERFLOW_EARLIER;
    }
    // d_mask[i] = value for every splat with d_score[i] < threshold (op = MSPLAT_SCORE_BELOW) or >= threshold (MSPLAT_SCORE_AT_LEAST)
    // (msplat_mark_scores); other bytes stay.  Device memory only; asynchronous on the stream, behind the RenderScores that wrote d_score.
    bool MarkScores(const uint64_t* d_score, size_t n, int32_t op, uint64_t threshold, uint8_t* d_mask, uint8_t value)
    {
        if (group || !ctx) {
            std::fprintf(stderr, "[msplat][E] MarkScores: %s\n", group ? "a device group has no per-splat visibility" : "no cloud (Init first)");
            return false;
        }
        if (msplat_mark_scores(ctx, d_score, n, op, threshold, d_mask, value) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] MarkScores: %s\n", msplat_last_error(ctx));
            return false;
        }
        return true;
    }
    // Selection by position (msplat_mark_volume, msplat_mark_view, msplat_measure_cloud): the cloud itself is tested, whatever a mask or
    // a crop hides, in upload numbering; no Sort is needed.  Device memory only; the marks are asynchronous on the stream of the latest
    // Sort's context, the measure returns after its copy.  A device group has none of them.
    // MarkVolume: d_mask[i] = value where the centre satisfies SetCrop's rule for worldToVolume and shape (MSPLAT_CROP_BOX / _SPHERE,
    // | MSPLAT_CROP_INVERT); other bytes stay.
    bool MarkVolume(const float* worldToVolume, int32_t shape, uint8_t* d_mask, size_t n, uint8_t value)
    {
        return Select("MarkVolume", [&](msplat_ctx* h) { return msplat_mark_volume(h, worldToVolume, shape, d_mask, n, value); });
    }
    // MarkView, select through: d_mask[i] = value where the projected centre lies in front of the camera on a pixel of window (nullptr =
    // the whole viewport) that d_region selects (nullptr = all; RenderScores' conventions), occluded splats included.
    template <class Mat4, class Vec4, class Vec2>
    bool MarkView(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar, const int32_t* window, uint8_t* d_mask,
                  size_t n, uint8_t value, const uint8_t* d_region = nullptr, uint64_t regionPitchBytes = 0)
    {
        static_assert(sizeof(Mat4) == 64 && sizeof(Vec4) == 16 && sizeof(Vec2) == 8, "glm-compatible layout expected");
        return Select("MarkView", [&](msplat_ctx* h) {
            return msplat_mark_view(h, F(cameraMat), F(projMat), F(viewport), F(nearFar), window, d_region, regionPitchBytes, d_mask, n, value);
        });
    }
    // MeasureCloud: count, box, largest footprint bound and moment sums of the splats d_select selects (nullptr: all) into *out.
    // MeasureBox (host only): the axis-aligned worldToVolume whose box holds every measured centre, pad world units wider per side.
    bool MeasureCloud(const uint8_t* d_select, size_t n, msplat_cloud_measure* out)
    {
        if (out) out->struct_size = sizeof(msplat_cloud_measure);
        return Select("MeasureCloud", [&](msplat_ctx* h) { return msplat_measure_cloud(h, d_select, n, out); });
    }
    static bool MeasureBox(const msplat_cloud_measure& m, float pad, float worldToVolume[16])
    {
        if (msplat_measure_box(&m, pad, worldToVolume) == MSPLAT_OK) return true;
        std::fprintf(stderr, "[msplat][E] MeasureBox: %s\n", msplat_last_error(nullptr));
        return false;
    }
    // Selection by attribute (msplat_cloud_values, msplat_mark_values, msplat_histogram_values): the same contract.
    // CloudValues: d_values[i] = what splat i is (kind = MSPLAT_VALUE_*; param: the point of _DISTANCE2, the colour of _COLOUR_DIST2).
    bool CloudValues(int32_t kind, const float* param, float* d_values, size_t n)
    {
        return Select("CloudValues", [&](msplat_ctx* h) { return msplat_cloud_values(h, kind, param, d_values, n); });
    }
    // MarkValues: d_mask[i] = value where lo <= d_values[i] <= hi (op = MSPLAT_RANGE_INSIDE) or where not (_OUTSIDE: NaN values too).
    bool MarkValues(const float* d_values, size_t n, float lo, float hi, int32_t op, uint8_t* d_mask, uint8_t value)
    {
        return Select("MarkValues", [&](msplat_ctx* h) { return msplat_mark_values(h, d_values, n, lo, hi, op, d_mask, value); });
    }
    // HistogramValues: `bins` counts over [lo, hi] into counts (host memory) and the summary of the values d_select selects (nullptr:
    // all) into *out; bins == 0: the summary alone.
    bool HistogramValues(const float* d_values, const uint8_t* d_select, size_t n, float lo, float hi, uint32_t bins, uint32_t* counts,
                         msplat_value_summary* out)
    {
        if (out) out->struct_size = sizeof(msplat_value_summary);
        return Select("HistogramValues", [&](msplat_ctx* h) { return msplat_histogram_values(h, d_values, d_select, n, lo, hi, bins, counts, out); });
    }
    // Selection by neighbourhood (msplat_neighbour_values): d_values[i] = how many splats of d_source (nullptr: all) lie within `radius`
    // of splat i (kind = MSPLAT_NEAR_COUNT, at most cap; 0: no cap) or the squared distance to the nearest (MSPLAT_NEAR_DIST2), for the
    // splats d_query selects (nullptr: all).  max_tests == 0: the library's budget.  info may be nullptr.  Synchronous.
    bool NeighbourValues(int32_t kind, float radius, const uint8_t* d_source, const uint8_t* d_query, size_t n, uint32_t cap, uint64_t max_tests,
                         float* d_values, msplat_neighbour_info* info = nullptr)
    {
        if (info) info->struct_size = sizeof(msplat_neighbour_info);
        return Select("NeighbourValues", [&](msplat_ctx* h) {
            return msplat_neighbour_values(h, kind, radius, d_source, d_query, n, cap, max_tests, d_values, info);
        });
    }
    template <class Call>
    bool Select(const char* who, Call&& call)
    {
        if (group || !ctx) {
            std::fprintf(stderr, "[msplat][E] %s: %s\n", who, group ? "a device group has no selection by position or attribute" : "no cloud (Init first)");
            return false;
        }
        const int rc = call(ctx);
        if (rc != MSPLAT_OK) std::fprintf(stderr, "[msplat][E] %s: %s\n", who, msplat_last_error(ctx));
        return rc == MSPLAT_OK;
    }

    // blocks until every frame in flight has finished
    // (also where a pair-buffer overflow of an earlier device-target Render is reported, see msplat_render)
    void Synchronize()
    {
        if (group && msplat_group_synchronize(group) != MSPLAT_OK)
            std::fprintf(stderr, "[msplat][E] Synchronize: %s\n", msplat_group_last_error(group));
        for (msplat_ctx* h : ctxs) {
            // (MSPLAT_ERR_PAIR_OVERFLOW_EARLIER: a queued call of an async_submit context found an earlier frame's overflow)
            const int rc = msplat_synchronize(h);
            if (rc != MSPLAT_OK) std::fprintf(stderr, "[msplat][%c] Synchronize: %s\n", Level(rc), msplat_last_error(h));
        }
    }
    // device-side join: `stream` (hipStream_t) waits for the frame issued last (the latest Sort's context)
    void WaitOnStream(void* stream)
    {
        if (!ctx) return;
        const int rc = msplat_stream_wait(ctx, stream);
        if (rc != MSPLAT_OK) std::fprintf(stderr, "[msplat][%c] WaitOnStream: %s\n", Level(rc), msplat_last_error(ctx));
    }

    // reverse join: the context the NEXT Sort will use waits for `event` (hipEvent_t), e.g. recorded after the
    // consumer of the render target that frame is going to overwrite
    void NextFrameWaitEvent(void* event)
    {
        if (!ctxs.empty()) msplat_wait_event(ctxs[(cur + 1) % (int)ctxs.size()], event);
    }
    int GetFrameSlot() const { return cur; }

    msplat_ctx* GetContext() { return group ? msplat_group_context(group, 0) : ctx; }   // the context of the latest Sort
    msplat_group* GetGroup() { return group; }

public:
    uint32_t numBlocksPerWorkgroup = 1024;   // accepted and ignored (splatrenderer.h:39)

protected:
    // one context per frame in flight, the storage kind set on context 0 (cfg.struct_size / srgb are the caller's)
    bool CreateContexts()
    {
        msplat_config c = cfg;
        if (framesInFlight > 1) {
            c.stream = nullptr;
            c.compositor_waves = 1280;       // frames share the CUs (measured r3: 768 .. 2048)
            c.frame_mode = MSPLAT_FRAMES_IN_FLIGHT;   // kernels that co-schedule well with other frames' kernels (+2-3 %)
            c.async_submit = 1;                       // a worker thread per context issues its launches (msplat.h)
        }
        // r6: an even number >= 4 of frames in flight: the contexts' streams alternate between the even and the odd CU positions of
        // every XCD -- two frames per half of the CUs instead of four on all of them (+3-5 %)
        const bool halves = framesInFlight >= 4 && framesInFlight % 2 == 0 && cfg.cu_partition == MSPLAT_CU_ALL;
        for (int k = 0; k < framesInFlight; ++k) {
            msplat_ctx* h = nullptr;
            if (halves) c.cu_partition = MSPLAT_CU_EVEN + (k & 1);
            if (msplat_create(&h, &c) != MSPLAT_OK) {
                std::fprintf(stderr, "[msplat][E] %s\n", msplat_last_error(nullptr));
                DestroyContexts();
                return false;
            }
            ctxs.push_back(h);
        }
        ctx = ctxs[0];
        cur = framesInFlight - 1;            // the first Sort lands on context 0
        if (msplat_set_cloud_storage(ctx, cloudStorage) != MSPLAT_OK) {      // (attached contexts render ctxs[0]'s storage)
            std::fprintf(stderr, "[msplat][E] %s\n", msplat_last_error(ctx));
            return false;
        }
        for (msplat_ctx* h : ctxs)           // the overlay's palette outlives the contexts (SetOverlayPalette)
            if (!overlayPalette.empty() && msplat_set_overlay_palette(h, overlayPalette.data(), (uint32_t)(overlayPalette.size() / 4)) != MSPLAT_OK) {
                std::fprintf(stderr, "[msplat][E] %s\n", msplat_last_error(h));
                return false;
            }
        return true;
    }

    // every other context of the rotation renders context 0's cloud
    bool AttachContexts()
    {
        for (size_t k = 1; k < ctxs.size(); ++k)
            if (msplat_attach_cloud(ctxs[k], ctxs[0]) != MSPLAT_OK) {
                std::fprintf(stderr, "[msplat][E] %s\n", msplat_last_error(ctxs[k]));
                return false;
            }
        return true;
    }

    template <class Upload>
    bool InitDeviceWith(const char* name, bool srgb, Upload upload)
    {
        DestroyContexts();
        cfg.struct_size = sizeof(cfg);
        cfg.srgb = srgb ? 1 : 0;
        if (groupDevices.size() > 1) {
            std::fprintf(stderr, "[msplat][E] %s: a device group takes no cloud from device memory (the replicated cloud needs peer "
                         "copies): Init from host memory, or ConfigureDevices with one device\n", name);
            return false;
        }
        if (!CreateContexts()) return false;
        if (upload() != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] %s: %s\n", name, msplat_last_error(ctx));
            return false;
        }
        return AttachContexts();
    }

    bool InitGroup(GaussianCloud& cloud)
    {
        std::vector<int32_t> devs(groupDevices.begin(), groupDevices.end());
        if (msplat_group_create(&group, devs.data(), (uint32_t)devs.size(), &cfg) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] %s\n", msplat_group_last_error(nullptr));
            group = nullptr;
            return false;
        }
        msplat_group_set_layout(group, groupKind, groupBlockRows);
        msplat_group_set_band_cull(group, groupBandCull ? 1 : 0);
        if (groupExchange != MSPLAT_EXCHANGE_PEER_STORE && msplat_group_set_exchange(group, groupExchange) != MSPLAT_OK)
            std::fprintf(stderr, "[msplat][W] SetGroupExchange: %s\n", msplat_group_last_error(group));
        if (msplat_group_set_cloud_storage(group, cloudStorage) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] %s\n", msplat_group_last_error(group));
            return false;
        }
        msplat_attr_offsets off{};
        off.pos_with_alpha = (uint32_t)cloud.GetPosWithAlphaAttrib().offset;
        off.r_sh0 = (uint32_t)cloud.GetR_SH0Attrib().offset;
        off.g_sh0 = (uint32_t)cloud.GetG_SH0Attrib().offset;
        off.b_sh0 = (uint32_t)cloud.GetB_SH0Attrib().offset;
        off.cov3_col0 = (uint32_t)cloud.GetCov3_Col0Attrib().offset;
        off.cov3_col1 = (uint32_t)cloud.GetCov3_Col1Attrib().offset;
        off.cov3_col2 = (uint32_t)cloud.GetCov3_Col2Attrib().offset;
        if (cloud.HasFullSH()) {
            off.r_sh1 = (uint32_t)cloud.GetR_SH1Attrib().offset; off.r_sh2 = (uint32_t)cloud.GetR_SH2Attrib().offset;
            off.r_sh3 = (uint32_t)cloud.GetR_SH3Attrib().offset; off.g_sh1 = (uint32_t)cloud.GetG_SH1Attrib().offset;
            off.g_sh2 = (uint32_t)cloud.GetG_SH2Attrib().offset; off.g_sh3 = (uint32_t)cloud.GetG_SH3Attrib().offset;
            off.b_sh1 = (uint32_t)cloud.GetB_SH1Attrib().offset; off.b_sh2 = (uint32_t)cloud.GetB_SH2Attrib().offset;
            off.b_sh3 = (uint32_t)cloud.GetB_SH3Attrib().offset;
        }
        if (msplat_group_upload_cloud(group, cloud.GetRawDataPtr(), cloud.GetNumGaussians(), (uint32_t)cloud.GetStride(), &off,
                                      cloud.HasFullSH() ? 1 : 0) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] %s\n", msplat_group_last_error(group));
            return false;
        }
        return true;
    }

    // SetOverlay / SetOverlayDevice: the classes on every context of the rotation
    bool SetClasses(const uint8_t* classes, size_t n, bool onDevice)
    {
        if (group) {
            std::fprintf(stderr, "[msplat][E] SetOverlay: a device group has no overlay\n");
            return false;
        }
        for (msplat_ctx* h : ctxs)
            if ((onDevice ? msplat_set_overlay_device(h, classes, n) : msplat_set_overlay(h, classes, n)) != MSPLAT_OK) {
                std::fprintf(stderr, "[msplat][E] SetOverlay: %s\n", msplat_last_error(h));
                return false;
            }
        return true;
    }

    // SetVisibility / SetVisibilityDevice: the mask on every context of the rotation
    bool SetMask(const uint8_t* mask, size_t n, bool onDevice)
    {
        if (group) {
            std::fprintf(stderr, "[msplat][E] SetVisibility: a device group has no per-splat visibility\n");
            return false;
        }
        for (msplat_ctx* h : ctxs)
            if ((onDevice ? msplat_set_visibility_device(h, mask, n) : msplat_set_visibility(h, mask, n)) != MSPLAT_OK) {
                std::fprintf(stderr, "[msplat][E] SetVisibility: %s\n", msplat_last_error(h));
                return false;
            }
        return true;
    }

    // log level of a status code: MSPLAT_ERR_PAIR_OVERFLOW_EARLIER reports a PAST frame, the call itself did its work
    static char Level(int rc) { return rc == MSPLAT_ERR_PAIR_OVERFLOW_EARLIER ? 'W' : 'E'; }

    template <class T> static const float* F(const T& v) { return reinterpret_cast<const float*>(&v); }

    // What every Render method does around its library call: the layout check; "[msplat][E] <name>: <missing>" unless `ready`; the
    // same with `noGroup` on a device group (NULL: the call serves a group too); call(), and its failure (void, like the reference)
    template <class Mat4, class Vec4, class Vec2, class Call>
    void RenderCall(const char* name, bool ready, const char* missing, const char* noGroup, Call call)
    {
        static_assert(sizeof(Mat4) == 64 && sizeof(Vec4) == 16 && sizeof(Vec2) == 8, "glm-compatible layout expected");
        if (!ready || (group && noGroup)) {
            std::fprintf(stderr, "[msplat][E] %s: %s\n", name, ready ? noGroup : missing);
            return;
        }
        const int rc = call();
        if (rc != MSPLAT_OK)
            std::fprintf(stderr, "[msplat][%c] %s: %s\n", Level(rc), name, group ? msplat_group_last_error(group) : msplat_last_error(ctx));
    }

    void DestroyContexts()
    {
        if (group) msplat_group_destroy(group);
        group = nullptr;
        for (msplat_ctx* h : ctxs) msplat_destroy(h);
        ctxs.clear();
        ctx = nullptr;
    }

    msplat_group* group = nullptr;       // set when ConfigureDevices named more than one device
    std::vector<int> groupDevices;
    int groupKind = MSPLAT_BANDS_CONTIGUOUS, groupBlockRows = 1;
    bool groupBandCull = false;
    int groupExchange = MSPLAT_EXCHANGE_PEER_STORE;
    int bandRank = 0, bandWorld = 1, bandKindSet = MSPLAT_BANDS_CONTIGUOUS, bandBlockRows = 1;

    std::vector<msplat_ctx*> ctxs;       // one per frame in flight; ctxs[0] owns the cloud
    msplat_ctx* ctx = nullptr;           // == ctxs[cur]
    int cur = 0;
    int framesInFlight = 1;
    int cloudStorage = MSPLAT_STORAGE_FP32;
    std::vector<float> overlayPalette;   // SetOverlayPalette's entries, for the contexts Init creates
    msplat_config cfg{sizeof(msplat_config), 0, MSPLAT_FB_RGBA32F, 0, -1.0f, 0, nullptr, 0, 0, 0, 0};
    void* target = nullptr;
    uint64_t targetPitch = 0;
    bool targetIsDevice = false;
};

// The SfM point-cloud view: PointRenderer's surface (/root/reference/src/pointrenderer.h:23-57).
// Render sorts and draws in one call, like the reference (pointrenderer.cpp:113-196).
class PointRenderer
{
public:
    PointRenderer() = default;
    ~PointRenderer() { msplat_destroy(ctx); }
    PointRenderer(const PointRenderer&) = delete;
    PointRenderer& operator=(const PointRenderer&) = delete;

    void Configure(int device, int fbFormat, void* stream = nullptr)
    {
        cfg.device = device;
        cfg.fb_format = fbFormat;
        cfg.stream = stream;
    }
    // optional, before Init: the sprite (the reference loads texture/sphere.png, pointrenderer.cpp:54-64);
    // RGBA8, top row first as decoded from the file (ReadPNG).  Default: the library's built-in sphere.
    void SetSprite(const uint8_t* rgba8, uint32_t width, uint32_t height)
    {
        sprite.assign(rgba8, rgba8 + (size_t)width * height * 4);
        spriteW = width;
        spriteH = height;
    }

    bool Init(std::shared_ptr<PointCloud> pointCloud, bool isFramebufferSRGBEnabledIn)
    {
        msplat_destroy(ctx);
        ctx = nullptr;
        cfg.struct_size = sizeof(cfg);
        cfg.srgb = isFramebufferSRGBEnabledIn ? 1 : 0;
        if (msplat_create(&ctx, &cfg) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] %s\n", msplat_last_error(nullptr));
            return false;
        }
        if (msplat_upload_points(ctx, pointCloud->GetRawDataPtr(), pointCloud->GetNumPoints(), (uint32_t)pointCloud->GetStride(),
                                 (uint32_t)pointCloud->GetPositionAttrib().offset,
                                 (uint32_t)pointCloud->GetColorAttrib().offset) != MSPLAT_OK ||
            msplat_set_point_sprite(ctx, sprite.empty() ? nullptr : sprite.data(), spriteW, spriteH) != MSPLAT_OK) {
            std::fprintf(stderr, "[msplat][E] %s\n", msplat_last_error(ctx));
            return false;
        }
        return true;
    }

    template <class Mat4, class Vec4, class Vec2>
    void Render(const Mat4& cameraMat, const Mat4& projMat, const Vec4& viewport, const Vec2& nearFar)
    {
        static_assert(sizeof(Mat4) == 64 && sizeof(Vec4) == 16 && sizeof(Vec2) == 8, "glm-compatible layout expected");
        if (!target) {
            std::fprintf(stderr, "[msplat][E] Render: no render target set (SetRenderTarget)\n");
            return;
        }
        const float* c = reinterpret_cast<const float*>(&cameraMat);
        const float* p = reinterpret_cast<const float*>(&projMat);
        const float* v = reinterpret_cast<const float*>(&viewport);
        const float* nf = reinterpret_cast<const float*>(&nearFar);
        if (msplat_sort(ctx, c, p, v, nf) != MSPLAT_OK ||
            msplat_render(ctx, c, p, v, nf, target, targetPitch, targetIsDevice ? 1 : 0) != MSPLAT_OK)
            std::fprintf(stderr, "[msplat][E] PointRenderer::Render: %s\n", msplat_last_error(ctx));
    }

    void SetRenderTarget(void* rgba, uint64_t pitchBytes, bool isDevicePointer)
    {
        target = rgba;
        targetPitch = pitchBytes;
        targetIsDevice = isDevicePointer;
    }
    msplat_ctx* GetContext() { return ctx; }

protected:
    msplat_ctx* ctx = nullptr;
    msplat_config cfg{sizeof(msplat_config), 0, MSPLAT_FB_RGBA32F, 0, -1.0f, 0, nullptr, 0, 0, 0, 0};
    std::vector<uint8_t> sprite;
    uint32_t spriteW = 0, spriteH = 0;
    void* target = nullptr;
    uint64_t targetPitch = 0;
    bool targetIsDevice = false;
};
