/*
 * msplat.h -- C ABI of libmsplat.so, the MI355X-native (gfx950 / CDNA4, HIP) replacement for the reference's SplatRenderer::Sort()/Render() hot path.  This header is what an integrator binds; parity-test taps, probes and experiment switches are in msplat_debug.h; the reasoning behind every default is in INTEGRATION.md (Appendix A) and DESIGN.md.
 * The reference's seam is the C++ class SplatRenderer (src/splatrenderer.h:23-67) fed by GaussianCloud (src/gaussiancloud.h:17-91); every entry point names the reference interface it replaces; splatapult_amd/host/msplat_host.hpp re-creates that class surface.
 * Conventions (the reference's): matrices are float[16], column-major like glm; cameraMat = camera-to-world; viewport = (x, y, W, H); nearFar = (near, far).  Functions return 0 (MSPLAT_OK) or a negative MSPLAT_ERR_* and never throw.  A context is not thread-safe (the reference's single GL thread).  No torch / framework / HIP types cross this boundary.
 */
#ifndef MSPLAT_H
#define MSPLAT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define MSPLAT_VERSION 1
enum {
    MSPLAT_OK = 0,
    MSPLAT_ERR_INVALID_ARG = -1,
    MSPLAT_ERR_NO_DEVICE = -2,     /* no HIP device / runtime failure at create: there is no CPU fallback */
    MSPLAT_ERR_HIP = -3,           /* a HIP call failed; see msplat_last_error */
    MSPLAT_ERR_NO_CLOUD = -4,      /* sort / render before upload */
    MSPLAT_ERR_NO_SORT = -5,       /* render before sort */
    MSPLAT_ERR_UNSUPPORTED = -6,   /* more than 2^24 splats, viewport beyond 8192 x 8192 */
    MSPLAT_ERR_PAIR_OVERFLOW = -7, /* (splat, bin) pair buffer too small, see msplat_render */
    MSPLAT_ERR_IO = -8,            /* PLY / JSON / image open or parse failure */
    MSPLAT_ERR_PAIR_OVERFLOW_EARLIER = -9  /* a WARNING: this call did its work, but an earlier device-output render had overflowed the pair buffer (that frame lacks splats; the buffer has grown) */
};
enum { MSPLAT_FB_RGBA32F = 0, MSPLAT_FB_RGBA16F = 1, MSPLAT_FB_RGBA8 = 2, MSPLAT_FB_SRGB8_ALPHA8 = 3 };   /* msplat_config.fb_format; 8-bit: bytes R G B A */
#define MSPLAT_FB_BYTES_PER_PIXEL(fb_format) ((fb_format) == MSPLAT_FB_RGBA32F ? 16u : (fb_format) == MSPLAT_FB_RGBA16F ? 8u : 4u)
enum { MSPLAT_ROP_NONE = 0, MSPLAT_ROP_RGBA8 = 1, MSPLAT_ROP_RGBA16F = 2 };          /* msplat_set_target_emulation */
enum { MSPLAT_TWO_PASS_AUTO = 0, MSPLAT_TWO_PASS_ON = 1, MSPLAT_TWO_PASS_OFF = 2 };  /* msplat_config.two_pass */
enum { MSPLAT_SPATIAL_AUTO = 0, MSPLAT_SPATIAL_ON = 1, MSPLAT_SPATIAL_OFF = 2 };     /* msplat_config.spatial_order */
enum { MSPLAT_FRAMES_AUTO = 0, MSPLAT_FRAMES_SERIAL = 1, MSPLAT_FRAMES_IN_FLIGHT = 2 }; /* msplat_config.frame_mode */
enum { MSPLAT_RANK_AUTO = 0, MSPLAT_RANK_BALLOT = 1 };                               /* msplat_config.rank_mode */
enum { MSPLAT_CU_ALL = 0, MSPLAT_CU_EVEN = 1, MSPLAT_CU_ODD = 2 };   /* msplat_config.cu_partition: every CU, or the even / odd CU positions of every XCD (4 frames in flight alternate: +3-5 %, INTEGRATION 6) */
enum { MSPLAT_TARGET_CLEAR = 0, MSPLAT_TARGET_LOAD = 1, MSPLAT_TARGET_PREMULTIPLIED = 2 };   /* msplat_set_target_mode */
enum { MSPLAT_BANDS_CONTIGUOUS = 0, MSPLAT_BANDS_INTERLEAVED = 1, MSPLAT_BANDS_BLOCK_INTERLEAVED = 2, MSPLAT_BANDS_ROOT_WEIGHTED = 3 };
typedef struct msplat_ctx msplat_ctx;
typedef struct msplat_cloud msplat_cloud;
typedef struct msplat_group msplat_group;
typedef struct msplat_points msplat_points;

/* Construction parameters: the implicit GL state the reference's renderer lives in -- device = the GL context's GPU
 * (sdl_main.cpp:98-100), fb_format = App's --fp16 / --fp32 FBO or its 8-bit window, sRGB-encoded or not (app.cpp:1000-1035), srgb = SplatRenderer::Init's
 * isFramebufferSRGBEnabled (splatrenderer.cpp:60-72).  Fields were appended over time: a struct_size that ends before a field
 * selects its AUTO value.  Pixels, keys and lists do not depend on any field below `stream` (INTEGRATION.md Appendix A). */
typedef struct msplat_config {
    uint32_t struct_size;      /* sizeof(msplat_config) */
    int32_t device;            /* HIP device ordinal */
    int32_t fb_format;         /* MSPLAT_FB_* */
    int32_t srgb;              /* FRAMEBUFFER_SRGB path of splat_vert.glsl:129-151,209-218 */
    float t_epsilon;           /* front-to-back early-out below this transmittance; 0 = never, negative = default 2^-14 */
    uint64_t pair_capacity;    /* max (splat, bin) pairs per render; 0 = automatic (grows) */
    void* stream;              /* hipStream_t to launch on; NULL = a stream of the library's own */
    int32_t enable_timing;     /* n > 0: per-stage events on every n-th sort / render (msplat_get_timings) */
    int32_t compositor_waves;  /* persistent compositor waves per render; 0 = default */
    int32_t rank_mode;         /* MSPLAT_RANK_*: lane-ordered LDS atomics (probed at create) or ballots for the stable ranking */
    int32_t frame_mode;        /* MSPLAT_FRAMES_*: the only context working on the GPU, or one of several frames in flight */
    int32_t spatial_order;     /* MSPLAT_SPATIAL_*: may the cloud be STORED in Morton order (chunk-level cull; sort ties then in storage order) */
    int32_t async_submit;      /* != 0: msplat_sort / device-output msplat_render return at once, a worker thread of the context issues their
                                  launches; a queued call's failure or overflow warning is returned by the next msplat_synchronize / _stream_wait */
    int32_t two_pass;          /* MSPLAT_TWO_PASS_*: may a Render run as two passes with occlusion feedback (same pixels) */
    int32_t cu_partition;      /* MSPLAT_CU_*: the CUs a stream the library creates itself (stream == NULL) may use; frames in flight */
} msplat_config;
/* Byte offsets of the attributes inside one AoS record: the BinaryAttribute offsets SplatRenderer::BuildVertexArrayObject binds
 * (splatrenderer.cpp:345-391; gaussiancloud.cpp:633-657).  r_sh1 .. b_sh3 are ignored unless full_sh. */
typedef struct msplat_attr_offsets {
    uint32_t pos_with_alpha, r_sh0, g_sh0, b_sh0, cov3_col0, cov3_col1, cov3_col2, r_sh1, r_sh2, r_sh3, g_sh1, g_sh2, g_sh3, b_sh1, b_sh2, b_sh3;
} msplat_attr_offsets;
typedef struct msplat_stats {
    uint64_t num_splats;       /* N */
    uint32_t sort_count;       /* V: splats that survived the presort cull (sortCount) */
    uint32_t drawn;            /* splats that passed the geometry-stage guard band */
    uint64_t pairs;            /* (splat, bin) pairs binned (bins of msplat_tile_size() pixels) */
    uint32_t tiles_x, tiles_y;
    uint32_t width, height;
    uint64_t pair_capacity;
    uint64_t device_bytes;     /* device memory held by the context */
    uint64_t pairs_tile16;     /* (splat, 16x16 tile) pairs covered by the footprints: SURVEY.md 8d's D */
} msplat_stats;
typedef struct msplat_timings {   /* milliseconds, averaged; names follow the reference's Tracy zones (splatrenderer.cpp:156-318) */
    float sort_total;          /* "SplatRenderer::Sort" (cull + key + sort) */
    float render_total;        /* "SplatRenderer::Render" */
    float project;             /* vertex + geometry stage */
    float binning;             /* bin lists */
    float composite;           /* fragment + blend */
    float reserved[3];         /* [0] frames averaged, [1] compositor KERNEL time (dispatch begin / end events), [2] its launches */
} msplat_timings;
/* ---- context: SplatRenderer::SplatRenderer / ~SplatRenderer (splatrenderer.cpp:41-48) ---- */
int msplat_create(msplat_ctx** out, const msplat_config* cfg);
void msplat_destroy(msplat_ctx* ctx);
const char* msplat_last_error(const msplat_ctx* ctx);   /* ctx may be NULL: global last error */
const char* msplat_version_string(void);
int msplat_tile_size(void);                             /* edge of the square screen bins (pixels) band rows refer to */
/* ---- upload: SplatRenderer::Init + BuildVertexArrayObject (splatrenderer.cpp:50-151,345-391).  Copies the interleaved
 * cloud (host memory, n records of stride_bytes) to the device; the caller may free it afterwards. */
int msplat_upload_cloud(msplat_ctx* ctx, const void* aos, uint64_t n, uint32_t stride_bytes, const msplat_attr_offsets* off, int full_sh);
/* GPU ingest (SURVEY.md 8f-1): GaussianCloud::ImportPly's per-vertex math (gaussiancloud.cpp:254-361) as a HIP kernel over the raw PLY vertex block.
 * Byte offsets of the float properties in one vertex; -1 = absent (reads as 0, like BinaryAttribute::Read); without all of f_rest, or full_sh == 0: SH degree 0 (:188-205). */
typedef struct msplat_ply_layout { uint32_t vertex_size; int32_t x, y, z, f_dc[3], f_rest[45], opacity, scale[3], rot[4]; } msplat_ply_layout;
int msplat_upload_ply_vertices(msplat_ctx* ctx, const void* vertices, uint64_t n, const msplat_ply_layout* layout, int full_sh);
/* Ply::Parse (ply.cpp:72-87) on the host + the ingest kernel: GaussianCloud::ImportPly + SplatRenderer::Init in one call */
int msplat_upload_ply(msplat_ctx* ctx, const char* path, int import_full_sh);
/* ---- uploads from DEVICE memory (INTEGRATION.md 18): a trainer's tensors, a streamed or decompressed cloud.  `off` / `layout` are host structs; every d_* pointer is memory of the context's device.  The source is read on the context's stream and
 * the call returns after that stream has drained, as the host uploads do: on return the caller may overwrite or free it.  Whatever produced the source must have completed before the call, or the context's stream must have been made to wait for it (msplat_wait_event).
 * Refused before anything is launched or copied -- MSPLAT_ERR_INVALID_ARG: a NULL pointer with n > 0, d_aos / d_vertices off a 16-byte or an attribute array off a 4-byte boundary, a pointer hipPointerGetAttributes does not report as device memory of the context's
 * device (host memory, another device's), stride / offset / layout errors as the host calls; MSPLAT_ERR_UNSUPPORTED: stride_bytes > 1024, n > 2^24.  The f_rest failures (SH_FP16: |c| >= 65520, SH_Q8: non-finite) are the host routes'; after any failure the context holds no cloud.
 * An unattached context that uploads the same or a smaller n again, same full_sh and storage, allocates nothing.  Out of scope: the device group (a replicated cloud needs peer copies), point clouds, updates of a sub-range, skipping the stream drain. */
int msplat_upload_cloud_device(msplat_ctx* ctx, const void* d_aos, uint64_t n, uint32_t stride_bytes, const msplat_attr_offsets* off, int full_sh);   /* = msplat_upload_cloud of the same bytes: records, footprint bounds, storage kind and order, cull boxes, bit for bit */
int msplat_upload_ply_vertices_device(msplat_ctx* ctx, const void* d_vertices, uint64_t n, const msplat_ply_layout* layout, int full_sh);   /* = msplat_upload_ply_vertices, bit for bit: the same kernel launch without the staging copy */
/* = msplat_cloud_from_attributes + msplat_upload_gaussian_cloud on its arrays (f_rest n x 45 in PLY order f_rest_0..44, rot as w x y z; d_f_rest == NULL or full_sh == 0: SH degree 0); bit for bit msplat_upload_ply_vertices of the same values packed into one vertex block */
int msplat_upload_attributes_device(msplat_ctx* ctx, uint64_t n, const float* d_xyz, const float* d_f_dc, const float* d_f_rest, const float* d_opacity, const float* d_log_scale, const float* d_rot, int full_sh);
/* the device cloud in the reference's interleaved layout (100 B / 244 B records), upload numbering */
int msplat_download_cloud(msplat_ctx* ctx, void* aos_out, uint64_t cap_bytes);
/* f_rest storage of the context's NEXT splat upload, any route (INTEGRATION.md 12).  SH_FP16: IEEE fp16, nearest even, 160 / 96-B
 * records; pixels = FP32 of the fp16-rounded cloud; a finite |f_rest| >= 65520 fails the upload (MSPLAT_ERR_UNSUPPORTED).  Attached
 * contexts render the owner's storage; points ignore it.  get: storage of the cloud rendered (-1: no cloud / NULL).
 * SH_Q8 (full SH only; a degree-1 cloud is stored, and reported, as FP32): one 128-B record.  Per splat and SH band (9 / 15 / 21 values,
 * r g b together), fp32: m = max |c|; step = m / 127 (0, codes 0, when m < 2^-64); code = clamp(rint(c / step), -127, 127), halves to even;
 * stored c' = (float)code * step: |c - c'| <= (1/2 + 2^-16) step.  Pixels = FP32 of the cloud of c', which the download returns; a second
 * Q8 round may move c' once more; a non-finite f_rest value fails the upload (MSPLAT_ERR_UNSUPPORTED, no cloud). */
enum { MSPLAT_STORAGE_SH_Q8 = 3 }; enum { MSPLAT_STORAGE_FP32 = 0, MSPLAT_STORAGE_SH_FP16 = 1 }; int msplat_set_cloud_storage(msplat_ctx* ctx, int32_t storage); int msplat_get_cloud_storage(const msplat_ctx* ctx);
/* ---- SplatRenderer::Sort (splatrenderer.cpp:153-312): cull + depth key (presort_compute.glsl:31-57), stable ascending 32-bit
 * radix sort; the sorted index list stays context state for the following renders.  Asynchronous: the reference's 4-byte
 * readback stall (splatrenderer.cpp:195-204) is not reproduced. */
int msplat_sort(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2]);
/* ---- per-splat visibility (INTEGRATION.md 19): hide splats without another upload.  For the context's FOLLOWING msplat_sort calls splat i (upload numbering) takes part iff mask(i) && crop(i); a hidden splat is exactly a splat the presort cull rejected: not in sort_count, sorted keys or indices, never projected, binned or composited.  Visible splats keep their keys, their relative order (ties by storage slot) and their upload indices.  msplat_render* draws the latest Sort: a change shows at the next Sort.  With nothing set a Sort launches and reads what it always did.
 * Mask: n bytes, one per splat, nonzero = visible (a bool array); n must be the cloud's N (else MSPLAT_ERR_INVALID_ARG); NULL = no mask.  Crop: M = worldToCrop (column-major, affine: M[3], M[7], M[11], M[15] are not read) and a shape.  Per splat centre (x, y, z), every operation rounded to fp32, no fused multiply-add, in this order:
 *   qx = ((M[0] x + M[4] y) + M[8] z) + M[12];  qy = ((M[1] x + M[5] y) + M[9] z) + M[13];  qz = ((M[2] x + M[6] y) + M[10] z) + M[14];  BOX: inside = |qx| <= 1 && |qy| <= 1 && |qz| <= 1;  SPHERE: inside = (qx qx + qy qy) + qz qz <= 1
 * (a centre on the surface is inside; a NaN makes every comparison false).  crop(i) = inside, with MSPLAT_CROP_INVERT or-ed in = !inside.  Per context (frames in flight: set it on every context of the rotation), ordered with the context's frames on its stream: no drain, no race with frames in flight.  Any upload or msplat_attach_cloud drops the mask (the numbering is new) and keeps the crop, evaluated on the new positions.
 * Costs one kernel at the next Sort after a change, 16 B (+ 1 B mask) per splat per context, 4 B per splat of a cloud stored in Morton order.  MSPLAT_ERR_UNSUPPORTED: the context holds a point cloud (it stays usable); _NO_CLOUD: a mask before the upload (a crop may come first); _INVALID_ARG: NULL context, unknown shape, non-finite M (rows 0-2), d_visible not memory of the context's device -- all before anything is launched or copied.  Out of scope: the device group, sub-range updates, bit-packed masks. */
enum { MSPLAT_CROP_NONE = 0, MSPLAT_CROP_BOX = 1, MSPLAT_CROP_SPHERE = 2, MSPLAT_CROP_INVERT = 0x100 };
int msplat_set_visibility(msplat_ctx* ctx, const uint8_t* visible, uint64_t n);             /* host memory; copied before return (waits at most for the PREVIOUS mask's copy) */
int msplat_set_visibility_device(msplat_ctx* ctx, const uint8_t* d_visible, uint64_t n);    /* device memory of the context's device; asynchronous on the context's stream, never waits: the source stays valid until that work has run (msplat_synchronize / msplat_stream_wait) */
int msplat_set_crop(msplat_ctx* ctx, const float worldToCrop[16], int32_t shape);           /* NULL or MSPLAT_CROP_NONE: no crop */
int msplat_get_visibility(msplat_ctx* ctx, int32_t* has_mask, int32_t* crop_shape, uint64_t* hidden);   /* hidden: splats the latest Sort's plane hides (synchronises); any out pointer may be NULL */ /* ---- msplat_compact_cloud (INTEGRATION.md 22) makes the mask and the crop permanent, on the device: it keeps splat i (upload numbering) iff mask(i) && crop(i), the rule above as the context's NEXT Sort would apply it (a NaN centre: kept by a mask alone, dropped by a crop, kept by an inverted crop), and renumbers the K kept splats 0..K-1 in ascending old upload index.  d_index_map (NULL: none; else N uint32 of device memory of the context's device, 4-byte aligned, checked as msplat_mark_ids checks its pointers): d_index_map[i] = new upload index of splat i, the exclusive prefix sum of the keep flags, or MSPLAT_ID_NONE where it was dropped.  n_kept_out (host, may be NULL) receives K.  pos4 and the stored records are copied bit for bit -- nothing is unpacked, re-rounded or re-quantised -- and the store keeps the storage kind and full_sh it had (msplat_set_cloud_storage still speaks of the next upload): msplat_download_cloud afterwards = the kept rows of msplat_download_cloud before, bit for bit, in every storage.  The context afterwards is what msplat_upload_cloud of the kept source rows, same storage and spatial_order, leaves: records, storage order (the spatial reorder runs on the compacted cloud: under AUTO it may enter or leave Morton storage where K crosses 2^18), cull boxes, the keys, indices and frames of every later Sort / Render, bit for bit; K == 0 is an upload of n = 0, K == N has the same postconditions and an identity map.  The mask is dropped (the numbering is new), the crop kept and evaluated on the new cloud at the next Sort; a render before that Sort returns MSPLAT_ERR_NO_SORT.  Synchronous like the uploads: drains async_submit work and the stream, returns after the stream has drained.  Never in place: the kept records are gathered into a fresh store (peak = old + new store, + the reorder's second copy of the new one); if that allocation fails: MSPLAT_ERR_HIP and the context renders what it rendered before; a failure after the swap leaves no cloud, as a failed upload does.  A store shared with attached contexts is not modified: this context gets a store of its own, the others render the old cloud until msplat_attach_cloud is called again.  Refused before anything is launched -- _INVALID_ARG: NULL ctx, a bad d_index_map; _NO_CLOUD; _UNSUPPORTED (the context stays usable): a point cloud.  Out of scope: the device group, a mask other than the context's own, a device-memory download of the records. */ int msplat_compact_cloud(msplat_ctx* ctx, uint32_t* d_index_map, uint64_t* n_kept_out); /* ---- msplat_transform_cloud (INTEGRATION.md 23) moves, rotates and scales splats on the device: every splat i (upload numbering) with d_select == NULL or d_select[i] != 0 (n bytes of device memory of the context's device, checked as msplat_mark_ids checks its pointers; n must be the cloud's N) is transformed by M (column-major; A[k][r] = M[4k + r] its upper 3x3; row 3 is not read), the others are copied.  The record is decoded to its FP32 floats (SH_FP16 / SH_Q8: the values msplat_download_cloud returns); then, every operation rounded to fp32, left to right, no fused multiply-add:  centre x' = ((M[0] x + M[4] y) + M[8] z) + M[12], y' and z' likewise (the crop's form);  covariance S[c][r] (column c, row r): T[c][r] = (A[0][r] S[c][0] + A[1][r] S[c][1]) + A[2][r] S[c][2], S'[c][r] = (T[0][r] A[0][c] + T[1][r] A[1][c]) + T[2][r] A[2][c] -- A S A^T, all nine entries, nothing symmetrised; a scale arrives through A, alpha is untouched;  SH, per channel, unless MSPLAT_TRANSFORM_KEEP_SH: band 1 = coefficients 1..3, band 2 = 4..8, band 3 = 9..15 (bands 2 and 3: full-SH clouds), sh'[k] = (..(D[k][0] sh[0] + D[k][1] sh[1]) + ..) + D[k][last] sh[last] over the band, D exactly what msplat_sh_rotation(M) returns; the DC term is untouched;  the footprint bound is recomputed from S'.  A transformed record is encoded again in the store's own kind (SH_Q8 is quantised again); an unselected splat's position and stored record are copied bit for bit, nothing unpacked: msplat_download_cloud afterwards = msplat_download_cloud before on those rows, bit for bit, in every storage.  An identity M is not a bit-for-bit no-op for -0 and inf (-0 + 0 = +0, 0 * inf = NaN).  The context afterwards is what msplat_upload_cloud of those rows, same storage, full_sh and spatial_order, leaves -- records, storage order (the spatial reorder runs on the moved cloud), cull boxes, the keys, indices and frames of every later Sort / Render, bit for bit -- except that the numbering has not changed, so the MASK IS KEPT; the crop is kept too and evaluated on the new centres at the next Sort; a render before that Sort returns MSPLAT_ERR_NO_SORT.  Never in place: the rows go into a fresh store (peak = old + new store, + the reorder's second copy); a store shared with attached contexts is not modified: this context gets a store of its own, the others render the old cloud until msplat_attach_cloud is called again.  Synchronous like the uploads: drains async_submit work and the stream.  Refused before anything is launched -- _UNSUPPORTED: M is not a rotation times a uniform positive scale (msplat_sh_rotation's gate) and KEEP_SH is not set, whatever the cloud's SH hold; with KEEP_SH any M with finite rows 0-2 is taken (shear, mirror, non-uniform scale) and the SH stay as they are; a point cloud (the context stays usable); _INVALID_ARG: NULL ctx, NULL M, a non-finite M (rows 0-2), unknown flag bits, a bad d_select, n != N; _NO_CLOUD.  After the kernel has run -- MSPLAT_ERR_HIP: the new store could not be allocated; _UNSUPPORTED: a transformed f_rest value is beyond SH_FP16's range (|c| >= 65520) or not finite under SH_Q8 -- the context renders what it rendered before; a failure after the swap leaves no cloud, as a failed upload does.  Out of scope: the device group, host-memory selections, mirrored SH (improper rotations), a per-splat matrix, merging two clouds. */ enum { MSPLAT_TRANSFORM_KEEP_SH = 1 }; int msplat_transform_cloud(msplat_ctx* ctx, const float M[16], const uint8_t* d_select, uint64_t n, int32_t flags); /* ---- msplat_append_cloud (INTEGRATION.md 24) puts splats INTO a cloud, on the device: ctx holds a splat cloud of N splats, src one of Ns (either may be 0); splat i of src (upload numbering) is appended iff d_select == NULL or d_select[i] != 0 (n bytes of device memory of the context's device, checked as msplat_mark_ids checks its pointers; n must be Ns).  The K selected splats follow ctx's own in ascending source index: they get upload indices N .. N+K-1, the splats ctx had keep 0 .. N-1; src is only read.  d_index_map (NULL: none; else Ns uint32 of device memory, 4-byte aligned, checked as msplat_compact_cloud checks its map): d_index_map[i] = N + the exclusive prefix sum of the select flags, or MSPLAT_ID_NONE where splat i was not selected; written only by a call that succeeds.  n_added_out (host, may be NULL) receives K.  The store keeps ctx's storage kind and full_sh (msplat_set_cloud_storage still speaks of the next upload); src's full_sh must be ctx's.  ctx's own N positions and stored records are copied bit for bit, nothing unpacked; so are the appended rows, pos4 and record, of a source of the SAME storage kind -- an SH_Q8 object pasted into an SH_Q8 scene is not quantised a second time.  Appended rows of a source of ANOTHER kind are decoded to their FP32 record floats (the values msplat_download_cloud(src) returns) and encoded by the destination kind's pack routine exactly as an upload of those floats encodes them; their pos4 -- centre and footprint bound -- is copied: the bound depends on covariance and alpha only, and centre, alpha and covariance are fp32 in every storage kind (the 16-float head of an SH_FP16 / SH_Q8 record is bit for bit the FP32 values).  The context afterwards is what msplat_upload_cloud of those N+K rows, same storage, full_sh and spatial_order, leaves -- records, storage order (the spatial reorder runs on the merged cloud: under AUTO it may enter Morton storage where N+K reaches 2^18), cull boxes, the keys, indices and frames of every later Sort / Render, bit for bit -- except that the old numbering has not changed, so the MASK IS KEPT and extended by K visible bytes; the crop is kept too and evaluated on all N+K centres at the next Sort; a render before that Sort returns MSPLAT_ERR_NO_SORT.  Never in place: all rows go into a fresh store (peak = both old stores + the new one, + the reorder's second copy); a store shared with attached contexts is not modified: this context gets a store of its own, the others render the old cloud until msplat_attach_cloud is called again.  src == ctx is allowed and duplicates the selection; src may be an attached context; K == 0 has the same postconditions as any other K; an empty destination (an upload of n = 0) extracts the selection into a cloud of its own.  Synchronous like the uploads: drains the async_submit work and the streams of both contexts; the kernels run on ctx's stream.  Refused before anything is launched -- _INVALID_ARG: NULL ctx or src, contexts on different devices, n != Ns, a bad d_select or d_index_map; _NO_CLOUD: either context has none; _UNSUPPORTED (the contexts stay usable): a point cloud in either, different full_sh.  After the count, with nothing allocated and the context unchanged -- _UNSUPPORTED: N + K > 2^24.  After the kernels have run -- MSPLAT_ERR_HIP: the new store could not be allocated; _UNSUPPORTED: a converted f_rest value is beyond SH_FP16's range (|c| >= 65520) or not finite under SH_Q8 -- the context renders what it rendered before; a failure after the swap leaves no cloud, as a failed upload does.  Out of scope: the device group, host-memory selections, a matrix applied on the way (msplat_transform_cloud before or after, with the index map), SH degree conversion, a device-memory download. */ int msplat_append_cloud(msplat_ctx* ctx, msplat_ctx* src, const uint8_t* d_select, uint64_t n, uint32_t* d_index_map, uint64_t* n_added_out);
/* ---- SplatRenderer::Render (splatrenderer.cpp:315-343) plus the GL pipeline behind its glDrawElements: splat_vert / _geom / _frag.glsl and
 * the blend / clear state of app.cpp:144-164.  Writes W x H RGBA (float, half or 4 bytes), row 0 = GL bottom row, alpha = 1 (msplat_set_target_mode: or
 * over the target's contents).  out_is_device != 0: `rgba` is device memory, the call is asynchronous on the stream; else host memory, the
 * call returns after the copy.  pitch_bytes = bytes between rows (0 = tight; else >= W pixels and a multiple of the pixel size, or MSPLAT_ERR_INVALID_ARG).
 * 8-bit targets (INTEGRATION.md 15) round the fp32 value x an RGBA32F context stores, once: v = x > 0 ? (x > 1 ? 1 : x) : 0 (NaN -> 0), code = (uint8)(v * 255.0f + 0.5f),
 * fp32 multiply, fp32 add, truncation.  MSPLAT_FB_SRGB8_ALPHA8: alpha so; r g b from e = v <= 0.0031308 ? 12.92 v : 1.055 v^(1/2.4) - 0.055 with |255 e - code| <= 0.5 + 2^-10.
 * Pair-buffer overflow: a host-output render grows the buffer and retries.  A device-output render cannot know; the NEXT msplat_sort / msplat_render / msplat_synchronize
 * of the context grows the buffer (unless pair_capacity fixed it) and reports it once -- msplat_synchronize: MSPLAT_ERR_PAIR_OVERFLOW; sort / render, whose own work is done: _EARLIER.  That frame lacks splats in its last bin columns: render it again. */
int msplat_render(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2], void* rgba, uint64_t pitch_bytes, int out_is_device);
/* ---- msplat_render plus a depth plane (INTEGRATION.md 14).  depth == NULL: msplat_render.  Else W x H float32 on every context (fp16 cannot resolve z_w near
 * 1), row 0 = GL bottom, depth_pitch_bytes between rows (0 = tight), in `rgba`'s memory space.  With z_i = 0.5 ndc.z + 0.5 (window depth of splat i), T as above:
 * depth = sum_i T_i w_i z_i + T * 1.0 -- the expected window depth over GL's clear depth 1.0 (app.cpp:160), MSPLAT_TARGET_LOAD's formula with colour z, dst = 1:
 * in [0, 1], exactly 1.0 where no splat reaches.  Early termination leaves T below t_epsilon, not at its limit: the plane is high by <= t_epsilon; t_epsilon = 0
 * removes the error.  Colour: msplat_render's bit for bit; the plane is the same in every target mode; banded contexts write owned rows.  MSPLAT_ERR_UNSUPPORTED
 * with msplat_set_depth_test, a target emulation, points or the tile probe; _INVALID_ARG: depth pitch < 4 W or not a multiple of 4.  Both eyes in one chain, or the
 * plane over an occluder's values: msplat_render_stereo_layers / msplat_render_layers.  Out of scope: the device group, msplat_band_exchange of the plane. */
int msplat_render_depth(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2], void* rgba, uint64_t pitch_bytes, float* depth, uint64_t depth_pitch_bytes, int out_is_device);
/* ---- msplat_render behind the caller's geometry (INTEGRATION.md 16): GL_LESS as app.cpp:160-163 sets it.  occluder == NULL: msplat_render.  Else W x H float32 window depths (the plane msplat_render_depth writes), row 0 = GL bottom, occluder_pitch_bytes between rows (0 = tight; else >= 4 W and a multiple of 4, or _INVALID_ARG), in `rgba`'s memory space, read-only.
 * Per pixel p: msplat_render's frame with every splat i with !(z_i < occluder[p]) absent at p; z_i = 0.5 ndc.z + 0.5, one per splat (splat_geom.glsl:98).  A splat AT the plane's depth is hidden; NaN hides everything at its pixel; +inf or any value above 1 nothing.  Formats, target modes (LOAD: a pixel no surviving splat reaches keeps its bits), banded contexts (owned rows of the plane), pitches, host output and its retry, frames in flight, two-pass frames: msplat_render's.
 * Device output, also with async_submit: the plane must stay valid and unchanged until the frame has run.  MSPLAT_ERR_UNSUPPORTED (the context stays usable): a point cloud, msplat_set_depth_test, a target emulation, the tile probe.  Both eyes in one chain, or msplat_render_depth's output in the same frame: msplat_render_stereo_layers / msplat_render_layers.  Out of scope: the device group, seeding msplat_set_depth_test's emulated depth buffer. */
int msplat_render_occluded(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2], void* rgba, uint64_t pitch_bytes, const float* occluder, uint64_t occluder_pitch_bytes, int out_is_device);
/* ---- msplat_render_occluded and msplat_render_depth in ONE frame (INTEGRATION.md 17): colour behind the caller's geometry plus the depth layer of the result, what the reference's XR frame (app.cpp:570-607: lines, camera path and carpet first, the splats blended over them under GL_LESS) hands an XR runtime.  Planes, pitches, memory space, lifetime, banded contexts, host output and its retry, frames in flight, async_submit: as for those two calls.  A NULL plane degrades: both NULL = msplat_render, depth only = msplat_render_depth, occluder only = msplat_render_occluded, the same kernels launched.  With both, per pixel p, o = occluder[p], z_i and T as above:  colour = msplat_render_occluded's, bit for bit, in every format and target mode;  depth[p] = min(fma(T, d0, sum_{i: z_i < o} T_i w_i z_i), 1),  d0 = o > 0 ? (o > 1 ? 1 : o) : 0 (NaN -> 0; the 8-bit targets' clamp) -- the expected window depth of the splats that pass the test over what the depth attachment holds, MSPLAT_TARGET_LOAD's formula with colour z and dst = the attachment.  An open plane (d0 = 1) gives msplat_render_depth's plane bit for bit; a pixel no surviving splat reaches holds d0 exactly; early termination leaves the plane high by <= t_epsilon * d0. In place: `depth` may be the occluder's own memory -- the same pointer AND the same pitch -- a depth attachment read and written in place (every pixel is read before it is written, by the lane that writes it; a two-pass frame never reads a tile again once it has written it).  Any other overlap of the two planes is undefined.  Like MSPLAT_TARGET_LOAD such a frame is not idempotent: after MSPLAT_ERR_PAIR_OVERFLOW[_EARLIER] a device-output caller restores the attachment before rendering the frame again (host output retries from the staged plane). MSPLAT_ERR_UNSUPPORTED (the context stays usable): a point cloud, msplat_set_depth_test, a target emulation, the tile probe.  Out of scope: the device group. */
int msplat_render_layers(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2], void* rgba, uint64_t pitch_bytes, float* depth, uint64_t depth_pitch_bytes, const float* occluder, uint64_t occluder_pitch_bytes, int out_is_device);
/* the reference's VR frame -- Sort with the first eye, Render per eye (app.cpp:603-607) -- as ONE chain of launches; the same pixels as two msplat_render calls, bit for bit.  Host targets, banded contexts, points and the emulations go view by view. */
int msplat_render_stereo(msplat_ctx* ctx, const float cameraMat0[16], const float projMat0[16], const float cameraMat1[16], const float projMat1[16], const float viewport[4], const float nearFar[2], void* rgba0, void* rgba1, uint64_t pitch_bytes, int out_is_device);
/* msplat_render_stereo with msplat_render_layers' planes per eye; the pitch of each kind is shared by the eyes.  depth0 / depth1 are both given or both NULL, and so are occluder0 / occluder1 (else MSPLAT_ERR_INVALID_ARG); all NULL = msplat_render_stereo.  One chain where msplat_render_stereo runs as one (device output, no bands, <= 2^23 splats, <= 128 bin rows per view), else view by view; either way each eye's colour and depth are bit for bit msplat_render_layers' with that eye's matrices after the same Sort. */
int msplat_render_stereo_layers(msplat_ctx* ctx, const float cameraMat0[16], const float projMat0[16], const float cameraMat1[16], const float projMat1[16], const float viewport[4], const float nearFar[2], void* rgba0, void* rgba1, uint64_t pitch_bytes, float* depth0, float* depth1, uint64_t depth_pitch_bytes, const float* occluder0, const float* occluder1, uint64_t occluder_pitch_bytes, int out_is_device);
/* ---- which splat each pixel shows (INTEGRATION.md 20): the read half of msplat_set_visibility -- click, brush and lasso on the device.  Over the splats of the latest Sort (hidden ones are not in it), walked near to far at pixel centre p: w_i(p) = alpha times the Gaussian, 0 where splat_frag.glsl:37-40 discards (w <= 1/256); T_i = prod_{j in front of i}(1 - w_j); c_i = T_i w_i.  ids[p] = upload index (the numbering of msplat_get_sorted_indices, also for a cloud stored in Morton order) of the splat with the largest c_i, the nearest of equals; MSPLAT_ID_NONE where no splat has w_i(p) > 0.  id_depth[p] (NULL: no plane) = that splat's window depth 0.5 ndc.z + 0.5, the per-splat value msplat_render_depth blends and msplat_render_occluded tests; exactly 1.0 at MSPLAT_ID_NONE.  The walk ends only where no later splat can win (T <= best): the planes do not depend on t_epsilon, compositor_waves, frame_mode, two_pass, the fb format or the target mode.  window = x0, y0, w, h in viewport pixels, row 0 = GL bottom; NULL = the whole viewport.  Both planes are w x h OF THE WINDOW, 4-byte elements, in one memory space; a pitch of 0 = tight rows, else >= 4 w and a multiple of 4; padding bytes are not written; a window's planes equal that rectangle of the whole viewport's, bit for bit.  Host output returns after the copy and grows the pair buffer like msplat_render; device output is asynchronous on the stream, queued under async_submit, and reports pair overflow as a device-output msplat_render does.  The frame is a plain one-pass frame's projection and binning plus one kernel over the 16 x 16 tiles the window touches; it is never a two-pass frame and leaves msplat_get_two_pass_info and msplat_get_timings as they were.
 * Refused before anything is launched -- _INVALID_ARG: NULL ids, a window with w or h <= 0 or not inside the viewport, a bad pitch; _NO_CLOUD / _NO_SORT as msplat_render; _UNSUPPORTED (the context stays usable): a point cloud, msplat_set_depth_test, a target emulation, the tile probe, a banded context.  Out of scope: the device group, two views in one chain, an occluder plane for the id walk.  msplat_mark_ids: device memory only (pointers checked as msplat_set_visibility_device checks its own); for every pixel of the w x h plane d_ids whose d_region byte is nonzero (NULL: every pixel; region pitch 0 = w) and whose id is not MSPLAT_ID_NONE: d_mask[id] = value.  n must be the cloud's N (else _INVALID_ARG); an id >= n is skipped, never stored through.  Asynchronous on the context's stream, so ordered behind the id frame that wrote the plane.  value = 0 on a mask of ones, handed to msplat_set_visibility_device, hides what was brushed; value = 1 on zeros is a selection. */
#define MSPLAT_ID_NONE 0xFFFFFFFFu
int msplat_render_ids(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2], const int32_t window[4], uint32_t* ids, uint64_t ids_pitch_bytes, float* id_depth, uint64_t id_depth_pitch_bytes, int out_is_device); int msplat_mark_ids(msplat_ctx* ctx, const uint32_t* d_ids, uint64_t ids_pitch_bytes, uint32_t w, uint32_t h, const uint8_t* d_region, uint64_t region_pitch_bytes, uint8_t* d_mask, uint64_t n, uint8_t value);
/* ---- how much of the frame each splat contributes (INTEGRATION.md 21): the scatter half of msplat_render_ids -- select through a lasso, prune by importance, find floaters.  Over the splats of the latest Sort, walked near to far at pixel centre p, with w_i(p), T_i and c_i = T_i w_i exactly msplat_render_ids' (w = 0 where splat_frag.glsl:37-40 discards): q_i(p) = (uint32) rint(c_i(p) * 2^23), the multiply fp32 and exact, rounding to nearest, ties to even; MSPLAT_SCORE_ONE is one fully covered pixel.  For every splat i in upload numbering (the numbering of msplat_get_sorted_indices, also for a cloud stored in Morton order): score[i] += sum_p q_i(p); pixels[i] += #{p : q_i(p) >= 1} (NULL: none), p over the pixels of window (x0, y0, w, h in viewport pixels, row 0 = GL bottom; NULL = the whole viewport) whose d_region byte is nonzero (NULL: all; a w x h byte plane of the WINDOW, region pitch 0 = w, as msplat_mark_ids takes it).  The arrays are accumulated into, not overwritten: the caller zeroes them, one call per camera sums over views.  A pixel is finished when T <= 2^-24 (every later c <= T, so c * 2^23 <= 0.5 and q = 0): the sums do not depend on t_epsilon, compositor_waves, frame_mode, two_pass, the fb format, the target mode or how pixels are grouped; they are integers, so the order of the additions does not matter, and a window's scores plus its complement's equal the whole viewport's exactly.  A 16 x 16 tile adds at most 256 * 2^23 = 2^31 at once, an 8192^2 frame at most 2^49 per call.  Device memory only (pointers checked as msplat_mark_ids checks its own; d_score 8-byte, d_pixels 4-byte aligned); n must be the cloud's N (else _INVALID_ARG).  Asynchronous on the context's stream, queued under async_submit; pair overflow is reported as for a device-output msplat_render and, as with MSPLAT_TARGET_LOAD, the call is not idempotent: after MSPLAT_ERR_PAIR_OVERFLOW[_EARLIER] the caller zeroes the arrays and runs it again.  Refused before anything is launched -- _INVALID_ARG: NULL d_score, an empty window or one not inside the viewport, region pitch < w; _NO_CLOUD / _NO_SORT as msplat_render_ids; _UNSUPPORTED (the context stays usable): a point cloud, msplat_set_depth_test, a target emulation, the tile probe, a banded context.  Never a two-pass frame; msplat_get_two_pass_info and msplat_get_timings stay as they were.  Out of scope: the device group, host-memory arrays, two views in one chain, an occluder plane for the score walk.  msplat_mark_scores: for every i < n, MSPLAT_SCORE_BELOW: d_score[i] < threshold, MSPLAT_SCORE_AT_LEAST: d_score[i] >= threshold sets d_mask[i] = value; other bytes are untouched.  Checks as msplat_mark_ids (n == N, device pointers, a point cloud refused); asynchronous on the stream, so ordered behind the score frames that wrote d_score.  BELOW with value = 0 on a mask of ones, handed to msplat_set_visibility_device, prunes; AT_LEAST with value = 1 on zeros selects. */
#define MSPLAT_SCORE_ONE 8388608u
enum { MSPLAT_SCORE_BELOW = 0, MSPLAT_SCORE_AT_LEAST = 1 }; int msplat_render_scores(msplat_ctx* ctx, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2], const int32_t window[4], const uint8_t* d_region, uint64_t region_pitch_bytes, uint64_t* d_score, uint32_t* d_pixels, uint64_t n); int msplat_mark_scores(msplat_ctx* ctx, const uint64_t* d_score, uint64_t n, int32_t op, uint64_t threshold, uint8_t* d_mask, uint8_t value);
/* blocks until everything queued on the context (and issued by its worker thread) has finished */
int msplat_synchronize(msplat_ctx* ctx);
/* ---- frames in flight.  The reference queues successive frames on one GL command stream and the driver overlaps them; here the overlap is
 * explicit: one context per frame in flight (own stream and per-frame buffers), the cloud uploaded into the first and attached to the others, frame k
 * on context k % depth.  Bit-identical to a single context.  The shims rotate (SetFramesInFlight).  Start with GPU_MAX_HW_QUEUES=8 (INTEGRATION.md 6). */
int msplat_attach_cloud(msplat_ctx* ctx, msplat_ctx* owner);        /* `ctx` renders `owner`'s cloud (same device), no copy */
int msplat_stream_wait(msplat_ctx* ctx, void* stream);              /* `stream` (hipStream_t) waits for the context's work so far */
int msplat_wait_event(msplat_ctx* ctx, void* event);                /* the context's stream waits for `event` (hipEvent_t) */
void* msplat_get_stream(msplat_ctx* ctx);                           /* the hipStream_t the context launches on */
int msplat_get_fb_format(const msplat_ctx* ctx);                    /* MSPLAT_FB_* the context was created with (-1: NULL) */
/* ---- rows of the screen on several GPUs (SURVEY.md 8e; no reference counterpart).  The context owns blocks of `block` consecutive bin rows
 * (msplat_tile_size() pixels; row 0 = GL bottom) starting at first_row, first_row + stride, ..., at most row_count rows (0 = all).  msplat_render
 * is always handed the full image; only owned rows are written (and read), bit-identical to the unbanded frame.  msplat_set_band(mod, rem) = interleaved single rows. */
int msplat_set_band(msplat_ctx* ctx, int32_t row_mod, int32_t row_rem);
int msplat_set_band_layout(msplat_ctx* ctx, int32_t first_row, int32_t row_count, int32_t block, int32_t stride);
/* the standard layouts (MSPLAT_BANDS_*) for rank `rank` of `world` over rows_full bin rows; host arithmetic only */
int msplat_band_plan(int32_t kind, int32_t rows_full, int32_t world, int32_t rank, int32_t block_rows, int32_t* first_row, int32_t* row_count, int32_t* block, int32_t* stride);
/* MSPLAT_BANDS_ROOT_WEIGHTED: contiguous bands, rank 0 (the gather's root: sends nothing) weighted `block_rows` PERCENT of another rank;
 * msplat_band_root_weight picks the percentage from a linear cost model (INTEGRATION.md 5); _plan_weighted: rows ~ weights[], bounds[world + 1] */
int msplat_band_plan_weighted(int32_t rows_full, int32_t world, const float* weights, int32_t* bounds_out);
int msplat_band_root_weight(int32_t rows_full, int32_t world, double fixed_ms, double ms_per_row, double row_bytes, double link_gbps, int overlap);
/* msplat_sort also drops splats whose footprint cannot reach an owned row (mono rendering; msplat_sort_count describes the band only) */
int msplat_set_band_cull(msplat_ctx* ctx, int enable);
/* The exchange, one process per GPU (the north star's "RCCL over xGMI only for the final row gather"): rank `root` posts one receive per run of
 * foreign rows straight into its framebuffer, the owners send their runs from where the compositor left them, all in ONE ncclGroupStart/End, on
 * the context's stream.  `comm` = the caller's ncclComm_t (librccl is loaded at the first call: no link-time dependency), `kind` / `block_rows` =
 * the layout every rank set with msplat_band_plan.  `rgba` = device memory of `height` rows of pitch_bytes, pixels of the context's fb_format (tight
 * rows: one message per run; else row by row in the same group, so a window of a wider surface keeps its neighbours).  world == 1: nothing to do.
 * flags: MSPLAT_EXCHANGE_WIRE_FP16 (RGBA32F targets only): rows cross the link as RGBA16F -- half the bytes; the gathered rows
 * then differ from the owners' by one fp16 rounding, |d| <= 2^-11 |value| (values beyond 65504 become inf), root's own rows not. */
enum { MSPLAT_EXCHANGE_WIRE_FP16 = 1 };
int msplat_band_exchange(msplat_ctx* ctx, void* comm, int32_t rank, int32_t world, int32_t root, int32_t kind, int32_t block_rows, void* rgba, uint64_t pitch_bytes, int32_t width, int32_t height, int32_t flags);
/* ---- several GPUs, ONE process: the reference's shape, a single-threaded host calling Sort / Render (app.cpp:1067-1068).  One context per
 * listed device, replicated cloud, bin rows partitioned (default MSPLAT_BANDS_CONTIGUOUS).  The only exchange is the row gather into `rgba` on
 * devices[0]: peer stores from the other devices' compositors (default; no staging), RCCL send / recv (msplat_group_set_exchange), or a 2-D copy
 * where no peer mapping exists.  Context 0's stream waits for the others: synchronising it, or msplat_group_synchronize, means the frame is complete.  cfg as msplat_create (device ignored). */
enum { MSPLAT_EXCHANGE_PEER_STORE = 0, MSPLAT_EXCHANGE_RCCL = 1, MSPLAT_EXCHANGE_COPY = 2 };
int msplat_group_create(msplat_group** out, const int32_t* devices, uint32_t n, const msplat_config* cfg);
void msplat_group_destroy(msplat_group* g);
const char* msplat_group_last_error(const msplat_group* g);     /* g may be NULL */
uint32_t msplat_group_size(const msplat_group* g);
msplat_ctx* msplat_group_context(msplat_group* g, uint32_t i);  /* borrowed: stats, timings of rank i */
int msplat_group_peer_store(const msplat_group* g, uint32_t i); /* 1: rank i writes device 0's framebuffer directly */
int msplat_group_set_exchange(msplat_group* g, int32_t exchange);  /* MSPLAT_EXCHANGE_*; also MSPLAT_GROUP_EXCHANGE=rccl|copy|peer */
int msplat_group_get_exchange(const msplat_group* g);              /* the exchange the latest msplat_group_render used */
int msplat_group_upload_cloud(msplat_group* g, const void* aos, uint64_t n, uint32_t stride_bytes, const msplat_attr_offsets* off, int full_sh);
int msplat_group_upload_gaussian_cloud(msplat_group* g, const msplat_cloud* c);
int msplat_group_upload_ply(msplat_group* g, const char* path, int import_full_sh);
int msplat_group_set_cloud_storage(msplat_group* g, int32_t storage);   /* msplat_set_cloud_storage on every context */
/* msplat_set_target_mode on every context.  LOAD: MSPLAT_ERR_UNSUPPORTED (the staging exchanges hold no destination rows to blend over) */
int msplat_group_set_target_mode(msplat_group* g, int32_t mode);
int msplat_group_set_layout(msplat_group* g, int32_t kind, int32_t block_rows);
int msplat_group_set_band_cull(msplat_group* g, int enable);
int msplat_group_sort(msplat_group* g, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2]);
int msplat_group_render(msplat_group* g, const float cameraMat[16], const float projMat[16], const float viewport[4], const float nearFar[2], void* rgba, uint64_t pitch_bytes, int out_is_device);
int msplat_group_synchronize(msplat_group* g);
/* ---- results of the latest Sort / Render (these synchronise) ---- */
int msplat_sort_count(msplat_ctx* ctx, uint32_t* v);            /* sortCount (splatrenderer.cpp:198-199) */
/* the element buffer of splatrenderer.cpp:296-311: upload indices of the visible splats in draw order (ascending key = far to near; ties by storage slot) */
int msplat_get_sorted_indices(msplat_ctx* ctx, uint32_t* dst, uint32_t cap);
int msplat_get_sorted_keys(msplat_ctx* ctx, uint32_t* dst, uint32_t cap);
/* dst[slot] = upload index (identity unless the cloud was reordered; *reordered says which); dst may be NULL */
int msplat_get_storage_order(msplat_ctx* ctx, uint32_t* dst, uint64_t cap, int* reordered);
int msplat_get_stats(msplat_ctx* ctx, msplat_stats* out);
int msplat_get_timings(msplat_ctx* ctx, msplat_timings* out);
/* ---- what the GL app's render target does (for callers who diff against its pixels; draw-order walk, several times slower).  Depth test
 * (SURVEY.md 8f-4): GL_DEPTH_TEST is on (app.cpp:163) and live wherever the target has a depth attachment (default back buffer, 24 bits,
 * sdl_main.cpp:79; XR swapchains); bits = 0 (default) models the colour-only --fp16 / --fp32 FBO.  Target rounding (SURVEY.md 8a-12, app.cpp:1012-1020):
 * the RGBA8 back buffer clamps and stores 8-bit unorm after EVERY blend, --fp16 rounds to fp16 after every blend; MSPLAT_ROP_NONE (default): fp32, rounded once. */
int msplat_set_depth_test(msplat_ctx* ctx, int depth_bits);
int msplat_set_target_emulation(msplat_ctx* ctx, int rop);         /* MSPLAT_ERR_UNSUPPORTED on an MSPLAT_FB_SRGB8_ALPHA8 context: it rounds linear values */
/* ---- the target's contents: the reference never clears in Render; it blends (GL_ONE, GL_ONE_MINUS_SRC_ALPHA, app.cpp:154-156) over what app.cpp drew
 * before.  For the following msplat_render / _stereo of the context, per pixel with C = the splats' premultiplied colour and T = the transmittance WHERE
 * THE WALK STOPPED (early termination leaves it below t_epsilon, not at its limit: an error <= t_epsilon |dst|; t_epsilon = 0 removes it):
 * CLEAR (default) writes (C, 1); PREMULTIPLIED (C, 1 - T), that blend over a target cleared to (0,0,0,0), a layer for a compositor; LOAD reads dst, the
 * pixel `rgba` holds (host output: the caller's array), and writes rgb = fma(T, dst.rgb, C), a = fma(T, dst.a - 1, 1) -- RGBA16F: read as half, 8-bit: as (float)code / 255.0f
 * (SRGB8_ALPHA8 r g b: decoded, c <= 0.04045 ? c / 12.92 : ((c + 0.055) / 1.055)^2.4), blended in fp32, rounded once; a pixel no splat reaches (T == 1) keeps its bits; dst lies behind every splat (also under msplat_set_depth_test).  LOAD is not idempotent: after MSPLAT_ERR_PAIR_OVERFLOW[_EARLIER]
 * a device-output caller restores dst before rendering the frame again.  Banded contexts read and write owned rows only.  MSPLAT_ERR_UNSUPPORTED, at
 * whichever call comes second: a non-CLEAR mode with a target emulation != MSPLAT_ROP_NONE, a point cloud, or (at the Render) msplat_set_tile_probe. */
int msplat_set_target_mode(msplat_ctx* ctx, int32_t mode);
int msplat_get_target_mode(const msplat_ctx* ctx);          /* -1: NULL */
/* ---- scene data: GaussianCloud / Ply (gaussiancloud.h:17-91, ply.h:19-46) ---- */
msplat_cloud* msplat_cloud_create(int import_full_sh);          /* GaussianCloud::GaussianCloud(Options{importFullSH}) */
void msplat_cloud_destroy(msplat_cloud* c);
int msplat_cloud_import_ply(msplat_cloud* c, const char* path); /* GaussianCloud::ImportPly (gaussiancloud.cpp:138-365) */
/* ImportPly's per-vertex math (gaussiancloud.cpp:254-361) on raw attribute arrays (synthetic scenes); f_rest may be NULL */
int msplat_cloud_from_attributes(msplat_cloud* c, uint64_t n, const float* xyz, const float* f_dc, const float* f_rest, const float* opacity, const float* log_scale, const float* rot);
int msplat_cloud_export_ply(msplat_cloud* c, const char* path); /* ExportPly / InitDebugCloud / PruneSplats */
int msplat_cloud_init_debug(msplat_cloud* c);                   /*   (gaussiancloud.cpp:367-626) */
int msplat_cloud_prune(msplat_cloud* c, const float origin[3], uint32_t keep);
uint64_t msplat_cloud_num_gaussians(const msplat_cloud* c);     /* GetNumGaussians */
uint64_t msplat_cloud_stride(const msplat_cloud* c);            /* GetStride */
uint64_t msplat_cloud_total_size(const msplat_cloud* c);        /* GetTotalSize */
const void* msplat_cloud_raw_data(const msplat_cloud* c);       /* GetRawDataPtr */
int msplat_cloud_has_full_sh(const msplat_cloud* c);            /* HasFullSH */
int msplat_cloud_attr_offsets(const msplat_cloud* c, msplat_attr_offsets* out);   /* Get*Attrib */
int msplat_upload_gaussian_cloud(msplat_ctx* ctx, const msplat_cloud* c);
/* ---- scene config files + image output (SURVEY.md 8f-2, 8f-3; host only) ---- */
/* CamerasConfig::ImportJson (camerasconfig.cpp:20-67): camera-to-world matrices (float[16] each) and the two fov angles */
int msplat_cameras_import_json(const char* path, float* mats16_out, float* fovs2_out, uint32_t cap, uint32_t* count_out);
int msplat_cameras_floor_plane(const char* path, float normal_out[3], float pos_out[3]);   /* EstimateFloorPlane (:69-95) */
int msplat_vrconfig_import_json(const char* path, float floor_mat_out[16]);                /* VrConfig (vrconfig.cpp:20-65) */
int msplat_vrconfig_export_json(const char* path, const float floor_mat[16]);
int msplat_find_config_file(const char* ply_path, const char* config_name, char* out, uint32_t cap);   /* app.cpp:89-119 */
/* W x H float RGBA (row 0 = bottom) -> 8-bit ".ppm" / PNG, top row first: clamp + round like an RGBA8 target, optional LinearToSRGB (util.cpp:357-367) */
int msplat_write_image(const char* path, const float* rgba, int width, int height, int encode_srgb);
/* 8-bit non-interlaced PNG (what Image::Load accepts, core/image.cpp:72-101) -> RGBA8, top row first; NULL queries the size */
int msplat_read_image(const char* path, uint8_t* rgba8_out, uint64_t cap, uint32_t* width_out, uint32_t* height_out);
/* ---- point-cloud renderer (SURVEY.md 8f-4): PointCloud (pointcloud.h:15-48) + PointRenderer (pointrenderer.h:23-57, pointrenderer.cpp:48-196).
 * A context holds EITHER a splat cloud or a point cloud; with points, msplat_sort is the same presort + radix sort and msplat_render the sprite
 * pipeline (point_*.glsl + the blend state of app.cpp:153-156): PointRenderer::Render == msplat_sort + msplat_render with the same matrices. */
msplat_points* msplat_points_create(int use_linear_colors);
void msplat_points_destroy(msplat_points* p);
int msplat_points_import_ply(msplat_points* p, const char* path);
int msplat_points_export_ply(const msplat_points* p, const char* path);
void msplat_points_init_debug(msplat_points* p);
uint64_t msplat_points_num(const msplat_points* p);
uint32_t msplat_points_stride(const msplat_points* p);          /* 32: position.xyzw, color.rgba */
const void* msplat_points_data(const msplat_points* p);
int msplat_upload_points(msplat_ctx* ctx, const void* aos, uint64_t n, uint32_t stride_bytes, uint32_t position_offset, uint32_t color_offset);   /* PointRenderer::Init's buffers (pointrenderer.cpp:95-110) */
int msplat_upload_point_cloud(msplat_ctx* ctx, const msplat_points* p);
/* the sprite (texture/sphere.png, pointrenderer.cpp:54-64): RGBA8, top row first (Image::Load's flip + premultiplication, mip chain); NULL = built-in sphere */
int msplat_set_point_sprite(msplat_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height);
/* ---- host matrix helpers used by the shims (glm closed forms; app.cpp:1042, util.cpp:420) ---- */
void msplat_mat4_inverse(const float m[16], float out[16]);
void msplat_mat4_mul(const float a[16], const float b[16], float out[16]); /* msplat_sh_rotation (host only, no device): A[k][r] = M[4k + r]; s = cbrt(det A), Q = A / s (double); MSPLAT_ERR_UNSUPPORTED, nothing written, unless det A > 0 and max |Q^T Q - I| <= 1e-4 (a gate: an fp32 rotation has 1e-7 there, a 1 % shear 1e-2); _INVALID_ARG: NULL M or a non-finite value in rows 0-2.  Else *scale_out = s (may be NULL) and d1 [3x3], d2 [5x5], d3 [7x7] (each may be NULL) = the row-major matrices of SH bands 1, 2, 3 for the rotation Q in the basis b[1..15] of splat_vert.glsl:51-105, its signs and order: b_l(Q^T v)^T = b_l(v)^T D_l for every unit v, so a splat whose coefficients become sh' = D_l sh shows at direction Q v the colour it showed at v.  Computed in double (a least-squares fit of that identity over 64 directions), rounded once to fp32; |entry| < 1e-12 is stored as 0. */ int msplat_sh_rotation(const float M[16], float d1[9], float d2[25], float d3[49], float* scale_out);
void msplat_perspective(float fovy, float aspect, float zn, float zf, float out[16]);
void msplat_create_projection(float tanL, float tanR, float tanU, float tanD, float zn, float zf, float out[16]);
#ifdef __cplusplus
}
#endif
#endif /* MSPLAT_H */
