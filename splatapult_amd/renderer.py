"""SplatRenderer: Python mirror of the reference's renderer seam
(/root/reference/src/splatrenderer.h:23-67): Init(gaussianCloud, isFramebufferSRGBEnabled,
useRgcSortOverride) -> bool, Sort(cameraMat, projMat, viewport, nearFar), Render(same four).
The reference renders into the currently bound GL framebuffer; here Render takes/returns an explicit
RGBA framebuffer.  Everything runs in libmsplat.so's HIP kernels -- there is no CPU path."""
import ctypes as C

import numpy as np

from . import _capi
from .scene import GaussianCloud


class _FrameArgs:
    """cameraMat, projMat, viewport, nearFar of one Sort / Render call, marshalled into ONE preallocated float buffer whose
    four pointers are made once: building four ctypes pointers per call cost 20 us, a third of the time it takes the host
    to issue a frame's launches (r3, bench.py's host_enqueue_ms_per_frame).  The library copies what it needs
    during the call, so the buffer is free again when the call returns."""
    __slots__ = ("buf", "cam", "proj", "vp", "nf", "p_cam", "p_proj", "p_vp", "p_nf")

    def __init__(self):
        self.buf = np.zeros(38, np.float32)
        self.cam, self.proj, self.vp, self.nf = self.buf[0:16], self.buf[16:32], self.buf[32:36], self.buf[36:38]
        base = self.buf.ctypes.data
        fp = C.POINTER(C.c_float)
        self.p_cam, self.p_proj = C.cast(base, fp), C.cast(base + 64, fp)
        self.p_vp, self.p_nf = C.cast(base + 128, fp), C.cast(base + 144, fp)

    @staticmethod
    def _flat(a, n):
        a = np.asarray(a, np.float32).reshape(-1)
        if a.shape[0] != n:
            raise AssertionError("expected %d floats" % n)
        return a

    def load(self, cameraMat, projMat, viewport, nearFar):
        f = self._flat
        self.cam[:] = f(cameraMat, 16)
        self.proj[:] = f(projMat, 16)
        self.vp[:] = f(viewport, 4)
        self.nf[:] = f(nearFar, 2)
        return self.p_cam, self.p_proj, self.p_vp, self.p_nf


def _storage_kind(name):
    """cloud_storage argument -> MSPLAT_STORAGE_*"""
    if name not in _capi.CLOUD_STORAGE_NAMES:
        raise ValueError("cloud_storage must be one of %s (got %r)" % (sorted(_capi.CLOUD_STORAGE_NAMES), name))
    return _capi.CLOUD_STORAGE_NAMES[name]


def _aos_upload(cloud):
    """(N, 25|61) float32 array in the reference AoS layout -> (the array, the arguments of msplat[_group]_upload_cloud after the handle)"""
    aos = np.ascontiguousarray(cloud, np.float32)
    assert aos.shape[1] in (25, 61)
    off = _capi.AttrOffsets(0, 16, 32, 48, 64, 76, 88, 100, 116, 132, 148, 164, 180, 196, 212, 228)
    return aos, (aos.ctypes.data, aos.shape[0], aos.shape[1] * 4, C.byref(off), 1 if aos.shape[1] == 61 else 0)


def _tensor_upload(xyz, f_dc, f_rest, opacity, log_scale, rot, full_sh):
    """six device tensors (duck-typed: data_ptr(), is_contiguous(), dtype, shape, device) -> the arguments of
    msplat_upload_attributes_device after the handle.  ValueError for anything but contiguous float32 of the right shape.  The
    current stream of a torch tensor's device is synchronised: what produced the tensors has then completed."""
    n = int(xyz.shape[0])
    want = {"xyz": (xyz, [(n, 3)]), "f_dc": (f_dc, [(n, 3)]), "f_rest": (f_rest, [(n, 45), (n, 3, 15)]),
            "opacity": (opacity, [(n,), (n, 1)]), "log_scale": (log_scale, [(n, 3)]), "rot": (rot, [(n, 4)])}
    for name, (t, shapes) in want.items():
        if t is None and name == "f_rest":
            continue
        if str(t.dtype).split(".")[-1] != "float32":
            raise ValueError("%s must be float32, not %s" % (name, t.dtype))
        if tuple(int(s) for s in t.shape) not in shapes:
            raise ValueError("%s must have shape %s, not %s" % (name, " or ".join(str(s) for s in shapes), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous (pass %s.contiguous())" % (name, name))
        if getattr(t.device, "type", "cuda") not in ("cuda", "hip"):
            raise ValueError("%s must live in device memory, not on %s" % (name, t.device))
    ptrs = {name: None if t is None else int(t.data_ptr()) for name, (t, _) in want.items()}
    import sys
    torch = sys.modules.get("torch")
    for t in (xyz, f_dc, f_rest, opacity, log_scale, rot):
        if torch is not None and isinstance(t, torch.Tensor):
            torch.cuda.current_stream(t.device).synchronize()
            break
    full = bool(full_sh) and ptrs["f_rest"] is not None
    return (n, C.c_void_p(ptrs["xyz"]), C.c_void_p(ptrs["f_dc"]), C.c_void_p(ptrs["f_rest"] if full else None),
            C.c_void_p(ptrs["opacity"]), C.c_void_p(ptrs["log_scale"]), C.c_void_p(ptrs["rot"]), 1 if full else 0)


def _target_mode(name):
    """set_target_mode argument -> MSPLAT_TARGET_*"""
    if name not in _capi.TARGET_MODES:
        raise ValueError("target mode must be one of %s (got %r)" % (sorted(_capi.TARGET_MODES), name))
    return _capi.TARGET_MODES[name]


def _host_frame(fb_format, vp, out=None, load=False):
    """the (H, W, 4) host array a Render into host memory fills: `out` checked, or a new one (load: the array's content is the
    destination the frame is blended over, so there has to be one)"""
    W, H = int(vp[2]), int(vp[3])
    dt = _capi.FB_DTYPES[fb_format]      # float32, float16, or uint8 for the two 8-bit targets (bytes R G B A)
    if out is None and load:
        raise ValueError('target mode "load" blends over the target\'s contents: pass out= (or out_ptr=)')
    if out is None:
        out = np.zeros((H, W, 4), dt)
    if not isinstance(out, np.ndarray) or out.dtype != dt or out.shape != (H, W, 4) or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("a %s target of %d x %d takes a C-contiguous %s array of shape (%d, %d, 4), not %s %s" % (
            _capi.FB_NAMES[fb_format], W, H, np.dtype(dt).name, H, W, getattr(out, "dtype", type(out).__name__),
            getattr(out, "shape", "")))
    return out


# what the ValueError says when a plane is not in the image's memory space: (with out_ptr, with host output), per plane the call names
_LIVES = {"depth": ("the depth plane lives in the colour's memory space: pass depth_ptr= with out_ptr=",
                    "the depth plane lives in the colour's memory space: pass depth= with host output"),
          "occluder": ("the occluder plane lives in the colour's memory space: pass occluder_ptr= with out_ptr=",
                       "the occluder plane lives in the colour's memory space: pass occluder= with host output"),
          "planes": ("the planes live in the colour's memory space: pass depth_ptr= / occluder_ptr= with out_ptr=",
                     "the planes live in the colour's memory space: pass depth= / occluder= with host output")}


_KEEP = object()        # SetOverlay: an argument left out stays as it is


def tint_matrix(rgb, a):
    """The (3, 4) colour map [G | o] of AdjustCloud that blends every colour towards rgb with weight a: G = (1 - a) I, o = a rgb --
    the overlay's rule t c + a h made permanent (in the record's colour space)."""
    rgb = np.asarray(rgb, np.float64).reshape(-1)
    if rgb.shape[0] != 3:
        raise ValueError("rgb must be three values, not %d" % rgb.shape[0])
    a = float(a)
    return np.concatenate([(1.0 - a) * np.eye(3), (a * rgb)[:, None]], axis=1).astype(np.float32)


def gain_matrix(gain, offset=0.0):
    """The (3, 4) colour map [G | o] of AdjustCloud with G = diag(gain) and o = offset; each a scalar or one value per channel:
    white balance, exposure, a lift."""
    g = np.broadcast_to(np.asarray(gain, np.float64), (3,))
    o = np.broadcast_to(np.asarray(offset, np.float64), (3,))
    return np.concatenate([np.diag(g), o[:, None]], axis=1).astype(np.float32)


def measure_box(measure, pad=0.0):
    """The axis-aligned worldToVolume (float32[16], column-major) whose box holds every centre of a MeasureCloud result, widened by
    pad >= 0 world units per side (msplat_measure_box): pass np.sqrt(measure["reach2_max"]) to include the splats' extent.  Feeds
    MarkVolume and SetCrop.  Host arithmetic; MsplatError for a measure without a finite centre or a bad pad."""
    m = _capi.CloudMeasure(struct_size=C.sizeof(_capi.CloudMeasure), selected=int(measure["selected"]), finite=int(measure["finite"]),
                           reach2_max=float(measure.get("reach2_max", 0.0)))
    for k in range(3):
        m.lo[k], m.hi[k] = float(measure["lo"][k]), float(measure["hi"][k])
    out = np.zeros(16, np.float32)
    _capi.check(None, _capi.lib().msplat_measure_box(C.byref(m), C.c_float(float(pad)), out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


class SplatRenderer:
    def __init__(self, device=0, fb_format="fp32", t_epsilon=-1.0, pair_capacity=0, stream=None,
                 enable_timing=False, frames_in_flight=1, rank_mode=_capi.RANK_AUTO, frame_mode=None,
                 spatial_order=_capi.SPATIAL_AUTO, async_submit=None, two_pass=_capi.TWO_PASS_AUTO, compositor_waves=None,
                 cu_partition=None, cloud_storage="fp32"):
        """frames_in_flight > 1: every Sort moves on to the next of that many contexts (own stream and
        per-frame buffers, ONE shared cloud -- msplat_attach_cloud), so successive frames overlap on the
        GPU; Render and the getters use the context of the latest Sort.  `stream` is only used with depth 1;
        consume a frame after wait_on_stream() / synchronize(), one framebuffer per frame in flight.
        cloud_storage: "fp32" (default), "sh_fp16" -- f_rest stored as IEEE fp16 -- or "sh_q8" -- f_rest as 8-bit codes with a
        step per SH band, one 128-B record per splat; a degree-1 cloud stays "fp32" (msplat_set_cloud_storage)."""
        self._storage = _storage_kind(cloud_storage)
        self.numBlocksPerWorkgroup = 1024      # accepted and ignored (splatrenderer.h:39)
        self._lib = _capi.lib()
        self._ctx = None
        self._ctxs = []
        self._cur = 0
        self._depth = max(1, int(frames_in_flight))
        self._args = _FrameArgs()
        self._device = device
        self._fb_format = _capi.fb_format(fb_format)
        self._t_eps = t_epsilon
        self._pair_cap = pair_capacity
        self._stream = stream
        self._timing = enable_timing
        self._rank_mode = int(rank_mode)       # msplat_config.rank_mode (RANK_AUTO / RANK_BALLOT)
        self._spatial = int(spatial_order)     # msplat_config.spatial_order (SPATIAL_AUTO / _ON / _OFF)
        # msplat_config.async_submit: Sort / device-output Render are queued to a worker thread of their context (default: on
        # with frames in flight -- the frames' launches are then issued concurrently instead of one context after the other)
        self._async = (self._depth > 1) if async_submit is None else bool(async_submit)
        # msplat_config.two_pass: may a Render run as two passes with occlusion feedback (same pixels, less work)?
        self._two_pass = int(two_pass)
        # msplat_config.compositor_waves: persistent compositor waves per render (None: every item its own wave for one frame at a
        # time, 1280 with frames in flight -- measured r3: pool sweep 768 .. 2048)
        self._comp_waves = compositor_waves
        # msplat_config.cu_partition (r6): None = the shims' rule -- with an even number >= 4 of frames in flight the contexts' streams
        # alternate between the even and the odd CU positions of every XCD (two frames per half: +3-5 %), else every CU;
        # False / 0 = every CU; or one MSPLAT_CU_* per context
        self._cu_partition = cu_partition
        # msplat_config.frame_mode: kernels for one frame at a time, or for contexts that share the GPU with other frames in
        # flight (msplat.h, MSPLAT_FRAMES_*)
        self._frame_mode = int(frame_mode) if frame_mode is not None else (_capi.FRAMES_IN_FLIGHT if self._depth > 1 else _capi.FRAMES_AUTO)
        self._n = 0
        self._load = False                     # set_target_mode("load"): a host Render needs the destination in out=
        self._ov_arg = None                    # SetOverlay's classes, for the contexts TransformCloud / AppendCloud / AdjustCloud attach again
        self._ov_palette = None                # ... and its palette, which new contexts (Init*) receive again

    def __del__(self):
        self.close()

    def close(self):
        ctxs, self._ctxs, self._ctx = getattr(self, "_ctxs", []), [], None
        for ctx in ctxs:
            self._lib.msplat_destroy(ctx)

    # -- reference surface ------------------------------------------------------------------
    def Init(self, gaussianCloud, isFramebufferSRGBEnabled=False, useRgcSortOverride=False):
        """splatrenderer.cpp:50-151.  Returns False (error text via last_error()) on failure, like the reference."""
        del useRgcSortOverride   # one HIP sort replaces both GL sorters
        if not self._create(isFramebufferSRGBEnabled):
            return False
        if isinstance(gaussianCloud, GaussianCloud):
            rc = self._lib.msplat_upload_gaussian_cloud(self._ctx, gaussianCloud.handle)
            self._n = gaussianCloud.GetNumGaussians()
        else:
            aos, args = _aos_upload(gaussianCloud)
            rc = self._lib.msplat_upload_cloud(self._ctx, *args)
            self._n = aos.shape[0]
        if rc != _capi.OK:
            self._err = self._lib.msplat_last_error(self._ctx).decode()
            return False
        return self._attach_all()

    def _create(self, isFramebufferSRGBEnabled):
        """one context per frame in flight; context 0 receives the cloud"""
        self.close()
        self._load = False                   # (new contexts start in MSPLAT_TARGET_CLEAR)
        cfg = _capi.Config()
        cfg.struct_size = C.sizeof(_capi.Config)
        cfg.device = self._device
        cfg.fb_format = self._fb_format
        cfg.srgb = 1 if isFramebufferSRGBEnabled else 0
        cfg.t_epsilon = self._t_eps
        cfg.pair_capacity = self._pair_cap
        cfg.enable_timing = int(self._timing)
        cfg.compositor_waves = int(self._comp_waves) if self._comp_waves is not None else (0 if self._depth == 1 else 1280)
        cfg.rank_mode = self._rank_mode
        cfg.frame_mode = self._frame_mode
        cfg.spatial_order = self._spatial
        cfg.async_submit = 1 if self._async else 0
        cfg.two_pass = self._two_pass
        halves = self._depth >= 4 and self._depth % 2 == 0 if self._cu_partition is None else False
        for k in range(self._depth):
            if isinstance(self._cu_partition, (list, tuple)):
                cfg.cu_partition = int(self._cu_partition[k])
            else:
                cfg.cu_partition = (_capi.CU_EVEN + (k & 1)) if halves else int(self._cu_partition or 0)
            if isinstance(self._stream, (list, tuple)):       # one caller-owned stream per frame in flight
                cfg.stream = self._stream[k]
            else:
                cfg.stream = self._stream if self._depth == 1 else None
            h = C.c_void_p()
            rc = self._lib.msplat_create(C.byref(h), C.byref(cfg))
            if rc != _capi.OK:
                self._err = self._lib.msplat_last_error(None).decode()
                self.close()
                return False
            self._ctxs.append(h)
        self._ctx = self._ctxs[0]
        self._cur = self._depth - 1          # the first Sort lands on context 0
        for h in self._ctxs:                 # (the attached contexts render context 0's storage anyway)
            if self._lib.msplat_set_cloud_storage(h, self._storage) != _capi.OK:
                self._err = self._lib.msplat_last_error(h).decode()
                self.close()
                return False
        if self._ov_palette is not None:     # the overlay's palette outlives the contexts (SetOverlay)
            for h in self._ctxs:
                if self._lib.msplat_set_overlay_palette(h, self._ov_palette.ctypes.data, self._ov_palette.shape[0]) != _capi.OK:
                    self._err = self._lib.msplat_last_error(h).decode()
                    self.close()
                    return False
        return True

    def _attach_all(self):
        for h in self._ctxs[1:]:
            if self._lib.msplat_attach_cloud(h, self._ctxs[0]) != _capi.OK:
                self._err = self._lib.msplat_last_error(h).decode()
                return False
        return True

    def InitFromPly(self, plyFilename, importFullSH=True, isFramebufferSRGBEnabled=False):
        """GPU ingest: Ply::Parse on the host, then GaussianCloud::ImportPly's per-vertex
        math (gaussiancloud.cpp:254-361) as a HIP kernel straight into the renderer's device layout."""
        if not self._create(isFramebufferSRGBEnabled):
            return False
        rc = self._lib.msplat_upload_ply(self._ctx, str(plyFilename).encode(), 1 if importFullSH else 0)
        if rc != _capi.OK:
            self._err = self._lib.msplat_last_error(self._ctx).decode() or "PLY open/parse failure"
            return False
        self._n = self.stats()["num_splats"]
        return self._attach_all()

    # -- clouds that are already in device memory (msplat_upload_*_device) ---------
    def InitFromDevice(self, ptr, n, stride_bytes, offsets, full_sh, isFramebufferSRGBEnabled=False):
        """Init from n interleaved records of stride_bytes in device memory (msplat_upload_cloud_device): ptr = device pointer (int,
        16-byte aligned), offsets = _capi.AttrOffsets or the 16 byte offsets in its field order.  The same context as Init with the
        same bytes in host memory.  The records must be complete when this is called (it does not know their producer's stream);
        on return they may be overwritten or freed."""
        return self._create(isFramebufferSRGBEnabled) and self.UpdateFromDevice(ptr, n, stride_bytes, offsets, full_sh)

    def InitFromTensors(self, xyz, f_dc, f_rest, opacity, log_scale, rot, full_sh=True, isFramebufferSRGBEnabled=False):
        """Init from a trainer's parameter tensors on this renderer's device (msplat_upload_attributes_device): GaussianCloud
        .FromAttributes' arrays -- xyz (N, 3), f_dc (N, 3), f_rest (N, 45) in PLY order or (N, 3, 15) or None, opacity (N,) or
        (N, 1), log_scale (N, 3), rot (N, 4) as w x y z -- float32 and contiguous, else ValueError.  Tensors are duck-typed
        (data_ptr(), is_contiguous(), dtype, shape, device); the current stream of torch tensors' device is synchronised first.
        f_rest=None or full_sh=False: SH degree 0."""
        args = _tensor_upload(xyz, f_dc, f_rest, opacity, log_scale, rot, full_sh)      # (refused before a context exists)
        return self._create(isFramebufferSRGBEnabled) and self._upload_device(self._lib.msplat_upload_attributes_device, args)

    def UpdateFromDevice(self, ptr, n, stride_bytes, offsets, full_sh):
        """InitFromDevice into the contexts that exist: the cloud goes into context 0, the others are attached again, nothing is
        re-created (a single context re-uses its store for the same or a smaller n).  Every frame in flight is finished first."""
        off = offsets if isinstance(offsets, _capi.AttrOffsets) else _capi.AttrOffsets(*[int(o) for o in offsets])
        return self._upload_device(self._lib.msplat_upload_cloud_device,
                                   (C.c_void_p(int(ptr)), int(n), int(stride_bytes), C.byref(off), 1 if full_sh else 0))

    def UpdateFromTensors(self, xyz, f_dc, f_rest, opacity, log_scale, rot, full_sh=True):
        """InitFromTensors into the contexts that exist -- the loop of a viewer that follows a training run: UpdateFromTensors,
        Sort, Render per step"""
        return self._upload_device(self._lib.msplat_upload_attributes_device,
                                   _tensor_upload(xyz, f_dc, f_rest, opacity, log_scale, rot, full_sh))

    def _upload_device(self, fn, args):
        if not self._ctxs:
            self._err = "no context: InitFromDevice / InitFromTensors (or Init) first"
            return False
        own = self._ctx = self._ctxs[0]
        self._cur = self._depth - 1          # the next Sort lands on context 0, as after Init
        rc = fn(own, *args)
        if rc != _capi.OK:
            self._err = self._lib.msplat_last_error(own).decode()
            return False
        self._n = int(args[1] if fn is self._lib.msplat_upload_cloud_device else args[0])
        return self._attach_all()

    def download_cloud(self, full_sh):
        """device cloud as (N, 25|61) float32 in the reference record layout (parity tests)"""
        out = np.zeros((max(self._n, 1), 61 if full_sh else 25), np.float32)
        _capi.check(self._ctx, self._lib.msplat_download_cloud(self._ctx, out.ctypes.data, out.nbytes))
        return out[:self._n]

    # -- the cloud out of the device (msplat_download_*_device, msplat_export_ply) --------
    def _download(self, what, call):
        """run call(ctx) -> code on the current context; False (and last_error) instead of an exception"""
        if not self._ctx:
            self._err = what + ": no context (Init first)"
            return False
        rc = call(self._ctx)
        if rc != _capi.OK:
            self._err = self._lib.msplat_last_error(self._ctx).decode()
            return False
        return True

    def ExportPly(self, plyFilename):
        """Write the cloud as it is on the device -- moved, pasted into, compacted -- as a PLY any 3DGS tool loads
        (msplat_export_ply): GaussianCloud.ExportPly's header and per-splat values, upload numbering, the mask and the crop
        ignored.  Returns False (see last_error()) on failure, like GaussianCloud.ExportPly."""
        return self._download("ExportPly", lambda h: self._lib.msplat_export_ply(h, str(plyFilename).encode()))

    def DownloadTensors(self, f_rest=True):
        """The cloud as the six tensors InitFromTensors takes, on this renderer's device (msplat_download_attributes_device): a dict
        xyz (N, 3), f_dc (N, 3), f_rest (N, 45) in PLY order (zeros for a cloud of SH degree 0; None with f_rest=False),
        opacity (N,), log_scale (N, 3), rot (N, 4) as w x y z, float32.  Returns None (see last_error()) on failure."""
        if not self._ctx:
            self._err = "DownloadTensors: no context (Init first)"
            return None
        import torch
        n, dev = self._n, torch.device("cuda", self._device)
        shapes = dict(xyz=(n, 3), f_dc=(n, 3), f_rest=(n, 45), opacity=(n,), log_scale=(n, 3), rot=(n, 4))
        t = {k: None if k == "f_rest" and not f_rest else torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
        torch.cuda.current_stream(dev).synchronize()
        p = [C.c_void_p(t[k].data_ptr() if t[k] is not None and n else None) for k in shapes]
        return t if self._download("DownloadTensors", lambda h: self._lib.msplat_download_attributes_device(h, n, *p)) else None

    def DownloadDevice(self, ptr, cap_bytes):
        """The cloud as N tight reference records (244 B with full SH, 100 B without: download_cloud's bytes) at the device pointer
        ptr (int, 16-byte aligned, cap_bytes large; msplat_download_cloud_device) -- what InitFromDevice takes with the reference
        offsets.  Returns False (see last_error()) on failure."""
        return self._download("DownloadDevice", lambda h: self._lib.msplat_download_cloud_device(h, C.c_void_p(int(ptr) or None), int(cap_bytes)))

    def cloud_storage(self):
        """"fp32" / "sh_fp16" / "sh_q8": how the uploaded cloud is stored (msplat_get_cloud_storage); None without a cloud"""
        k = self._lib.msplat_get_cloud_storage(self._ctx) if self._ctx else -1
        return {v: n for n, v in _capi.CLOUD_STORAGE_NAMES.items()}.get(k)

    def last_error(self):
        if self._ctx:
            return self._lib.msplat_last_error(self._ctx).decode()
        return getattr(self, "_err", "")

    def Sort(self, cameraMat, projMat, viewport, nearFar):
        """splatrenderer.cpp:153-312"""
        c, p, v, nf = self._args.load(cameraMat, projMat, viewport, nearFar)
        self._cur = (self._cur + 1) % len(self._ctxs)
        self._ctx = self._ctxs[self._cur]
        _capi.check(self._ctx, self._lib.msplat_sort(self._ctx, c, p, v, nf))

    def Render(self, cameraMat, projMat, viewport, nearFar, out=None, out_ptr=None, pitch_bytes=0, depth=None, depth_ptr=None,
               depth_pitch_bytes=0, occluder=None, occluder_ptr=None, occluder_pitch_bytes=0):
        """splatrenderer.cpp:315-343 + the GL pipeline behind it.
        out=None      -> returns a new (H, W, 4) numpy array (float32, float16 or -- the 8-bit targets -- uint8), row 0 = GL bottom row
        out=ndarray   -> filled in place
        out_ptr=int   -> device pointer (e.g. torch tensor .data_ptr()); asynchronous on the stream
        The depth plane (msplat_render_depth: the splats' expected window depth over the clear depth 1.0, float32 on every
        context) lives where the colour does: depth=(H, W) float32 array to fill, or True to have one allocated, with host
        output -- the call then returns (image, depth); depth_ptr=int (rows of depth_pitch_bytes, 0 = tight) with out_ptr.
        The occluder plane (msplat_render_occluded: window depths of the caller's geometry, GL_LESS -- a splat with
        !(z_w < occluder) at a pixel is absent there) lives where the colour does too and is only read: occluder=(H, W) float32
        array with host output, occluder_ptr=int (rows of occluder_pitch_bytes, 0 = tight; valid until the frame has run) with
        out_ptr.  Render takes a depth output or an occluder plane, not both (MsplatError(ERR_UNSUPPORTED)): the frame with both
        is RenderLayers'"""
        f = self._args.load(cameraMat, projMat, viewport, nearFar)
        kind = "occluder" if occluder is not None or occluder_ptr is not None else "depth"
        if kind == "occluder":
            if (depth is not None and depth is not False) or depth_ptr is not None:
                raise _capi.MsplatError(_capi.ERR_UNSUPPORTED, "Render takes either a depth output (msplat_render_depth) or an occluder "
                                        "plane (msplat_render_occluded), not both: that frame is RenderLayers' (msplat_render_layers)")
            depth = None

        def call(rgba, pitch, d, o, dev):
            if o is not None:
                return self._lib.msplat_render_occluded(self._ctx, *f, C.c_void_p(rgba), pitch, C.c_void_p(o), occluder_pitch_bytes, dev)
            if d is not None:
                return self._lib.msplat_render_depth(self._ctx, *f, C.c_void_p(rgba), pitch, C.c_void_p(d), depth_pitch_bytes if dev else 0, dev)
            return self._lib.msplat_render(self._ctx, *f, C.c_void_p(rgba), pitch, dev)

        return self._render_one(call, out, out_ptr, pitch_bytes, depth, depth_ptr, occluder, occluder_ptr, self._asserted_plane,
                                _LIVES[kind])

    @staticmethod
    def _asserted_plane(name, plane, H, W):
        assert plane.dtype == np.float32 and plane.shape == (H, W) and plane.flags["C_CONTIGUOUS"]
        return plane

    @staticmethod
    def _host_plane(name, plane, H, W):
        if not isinstance(plane, np.ndarray) or plane.dtype != np.float32 or plane.shape != (H, W) or not plane.flags["C_CONTIGUOUS"]:
            raise ValueError("%s takes a C-contiguous float32 array of shape (%d, %d)" % (name, H, W))
        return plane

    def _render_one(self, call, out, out_ptr, pitch_bytes, depth, depth_ptr, occluder, occluder_ptr, plane, refusals):
        """One view, behind Render and RenderLayers: the image and the planes are the caller's device pointers (returns None) or host
        arrays -- `out` checked or made, depth=True allocated, each plane checked by `plane` -- and never one of each (`refusals`:
        what the ValueError says with out_ptr / with host output).  call(rgba, pitch_bytes, depth, occluder, out_is_device) issues
        the frame with the library function of its choice and returns its code"""
        if out_ptr is not None:
            if depth is not None or occluder is not None:
                raise ValueError(refusals[0])
            _capi.check(self._ctx, call(out_ptr, pitch_bytes, depth_ptr, occluder_ptr, 1))
            return None
        if depth_ptr is not None or occluder_ptr is not None:
            raise ValueError(refusals[1])
        out = _host_frame(self._fb_format, self._args.vp, out, self._load)
        H, W = out.shape[:2]
        if depth is False:
            depth = None
        if depth is True:
            depth = np.empty((H, W), np.float32)
        d = plane("depth=", depth, H, W).ctypes.data if depth is not None else None
        o = plane("occluder=", occluder, H, W).ctypes.data if occluder is not None else None
        _capi.check(self._ctx, call(out.ctypes.data, 0, d, o, 0))
        return out if depth is None else (out, depth)

    def _render_two(self, call, cameraMats, projMats, viewport, nearFar, out_ptrs, pitch_bytes, depth=None, depth_ptrs=None,
                    occluders=None, occluder_ptrs=None):
        """Two views, behind RenderStereo and RenderStereoLayers: as _render_one, with pairs.  call(frame, rgba0, rgba1, pitch_bytes,
        (depth0, depth1), (occluder0, occluder1), out_is_device); frame: the six marshalled arrays"""
        a0, a1 = self._args, getattr(self, "_args1", None)
        if a1 is None:
            a1 = self._args1 = _FrameArgs()
        c0, p0, v, nf = a0.load(cameraMats[0], projMats[0], viewport, nearFar)
        c1, p1, _, _ = a1.load(cameraMats[1], projMats[1], viewport, nearFar)
        f, none = (c0, p0, c1, p1, v, nf), (None, None)
        if out_ptrs is not None:
            if depth is not None or occluders is not None:
                raise ValueError("the planes live in the colour's memory space: pass depth_ptrs= / occluder_ptrs= with out_ptrs=")
            _capi.check(self._ctx, call(f, out_ptrs[0], out_ptrs[1], pitch_bytes, depth_ptrs if depth_ptrs is not None else none,
                                        occluder_ptrs if occluder_ptrs is not None else none, 1))
            return None
        if depth_ptrs is not None or occluder_ptrs is not None:
            raise ValueError("the planes live in the colour's memory space: pass depth= / occluders= with host output")
        outs = [_host_frame(self._fb_format, a0.vp, None, self._load), _host_frame(self._fb_format, a0.vp, None, self._load)]
        H, W = outs[0].shape[:2]
        if depth is True:
            depth = [np.empty((H, W), np.float32), np.empty((H, W), np.float32)]
        d = [self._host_plane("depth=", z, H, W).ctypes.data for z in depth] if depth is not None else none
        o = [self._host_plane("occluders=", z, H, W).ctypes.data for z in occluders] if occluders is not None else none
        _capi.check(self._ctx, call(f, outs[0].ctypes.data, outs[1].ctypes.data, 0, d, o, 0))
        return outs if depth is None else (outs, list(depth))

    def RenderStereo(self, cameraMats, projMats, viewport, nearFar, out_ptrs=None, pitch_bytes=0):
        """both eyes of the latest Sort in ONE chain of launches (msplat_render_stereo; the reference renders them one after the
        other, app.cpp:603-607): same pixels as two Render calls.  out_ptrs: two device pointers (asynchronous), else two host
        arrays are returned -- not in target mode "load", which needs the destinations: ValueError without out_ptrs (render the
        eyes with two Render(out=...) calls instead)"""
        def call(f, rgba0, rgba1, pitch, d, o, dev):
            return self._lib.msplat_render_stereo(self._ctx, *f, C.c_void_p(rgba0), C.c_void_p(rgba1), pitch, dev)

        return self._render_two(call, cameraMats, projMats, viewport, nearFar, out_ptrs, pitch_bytes)

    def RenderLayers(self, cameraMat, projMat, viewport, nearFar, out=None, out_ptr=None, pitch_bytes=0, depth=None, depth_ptr=None,
                     depth_pitch_bytes=0, occluder=None, occluder_ptr=None, occluder_pitch_bytes=0):
        """msplat_render_layers: Render's occluder plane and depth output in ONE frame -- the colour is the occluded frame's, the
        depth plane the expected window depth of the splats that pass the test over the occluder's values clamped to [0, 1]
        (min(fma(T, d0, sum T_i w_i z_i), 1)).  The arguments are Render's; a plane that is not given degrades the call to
        msplat_render_depth / msplat_render_occluded / msplat_render.  The depth plane may BE the occluder plane (the same array,
        or the same pointer and pitch): a depth attachment read and written in place.
        Host output returns the image, or (image, depth) when a depth plane was asked for; device output returns None."""
        f = self._args.load(cameraMat, projMat, viewport, nearFar)

        def call(rgba, pitch, d, o, dev):
            return self._lib.msplat_render_layers(self._ctx, *f, C.c_void_p(rgba), pitch, C.c_void_p(d), depth_pitch_bytes if dev else 0,
                                                  C.c_void_p(o), occluder_pitch_bytes if dev else 0, dev)

        return self._render_one(call, out, out_ptr, pitch_bytes, None if depth is False else depth, depth_ptr, occluder, occluder_ptr,
                                self._host_plane, _LIVES["planes"])

    def RenderStereoLayers(self, cameraMats, projMats, viewport, nearFar, out_ptrs=None, pitch_bytes=0, depth_ptrs=None,
                           depth_pitch_bytes=0, occluder_ptrs=None, occluder_pitch_bytes=0, depth=False, occluders=None):
        """msplat_render_stereo_layers: RenderStereo with RenderLayers' planes per eye; each eye's colour and depth plane are
        RenderLayers' with that eye's matrices.  out_ptrs (two device pointers; asynchronous) with depth_ptrs / occluder_ptrs --
        pairs of device pointers, one pitch per kind, None = no such plane -- runs as one chain; returns None.
        Without out_ptrs host arrays are used, view by view: occluders = a pair of (H, W) float32 arrays or None, depth = True to
        have the depth planes allocated (or a pair of arrays to fill); returns [image0, image1], or ([image0, image1], [depth0,
        depth1]) when depth planes were asked for.  Not in target mode "load" (as for RenderStereo)."""
        def call(f, rgba0, rgba1, pitch, d, o, dev):
            return self._lib.msplat_render_stereo_layers(self._ctx, *f, C.c_void_p(rgba0), C.c_void_p(rgba1), pitch, C.c_void_p(d[0]),
                                                         C.c_void_p(d[1]), depth_pitch_bytes if dev else 0, C.c_void_p(o[0]),
                                                         C.c_void_p(o[1]), occluder_pitch_bytes if dev else 0, dev)

        return self._render_two(call, cameraMats, projMats, viewport, nearFar, out_ptrs, pitch_bytes, None if depth is False else depth,
                                depth_ptrs, occluders, occluder_ptrs)

    # -- extensions -------------------------------------------------------------------------
    def set_band(self, row_mod, row_rem, band_cull=False):
        """interleaved rows: this renderer owns the bin rows t with t % row_mod == row_rem"""
        for h in self._ctxs:
            _capi.check(h, self._lib.msplat_set_band(h, row_mod, row_rem))
            _capi.check(h, self._lib.msplat_set_band_cull(h, 1 if band_cull else 0))

    def set_band_layout(self, first_row, row_count, block, stride, band_cull=False):
        """general form (msplat_set_band_layout): blocks of `block` bin rows at first_row, first_row + stride, ..."""
        for h in self._ctxs:
            _capi.check(h, self._lib.msplat_set_band_layout(h, first_row, row_count, block, stride))
            _capi.check(h, self._lib.msplat_set_band_cull(h, 1 if band_cull else 0))

    def set_band_plan(self, kind, rows_full, world, rank, block_rows=1, band_cull=False):
        """rank `rank` of `world` under the layout `kind` ("contiguous" | "interleaved" | "block"); returns the parameters"""
        lay = _capi.band_plan(kind, rows_full, world, rank, block_rows)
        self.set_band_layout(*lay, band_cull=band_cull)
        return lay

    def set_depth_test(self, depth_bits):
        """emulated depth buffer: 0 = colour-only target (default), 24 = default back buffer,
        32 = float depth attachment"""
        for h in self._ctxs:
            _capi.check(h, self._lib.msplat_set_depth_test(h, int(depth_bits)))

    def set_target_emulation(self, rop):
        """the blend as the GL app's render target performs it: "rgba8" = clamp + 8-bit unorm after every
        blend (default back buffer), "fp16" = fp16 rounding after every blend (--fp16), None = float accumulation"""
        mode = {None: _capi.ROP_NONE, "none": _capi.ROP_NONE, "rgba8": _capi.ROP_RGBA8, "fp16": _capi.ROP_RGBA16F}[rop]
        for h in self._ctxs:
            _capi.check(h, self._lib.msplat_set_target_emulation(h, mode))

    def set_target_mode(self, mode):
        """what Render does with the target's contents (msplat_set_target_mode), on every context of the rotation: "clear"
        (default) overwrites with (C, 1); "premultiplied" writes the layer (C, 1 - T); "load" blends the frame over the pixels the
        target holds -- with a host out= array its content is the destination, and out=None is an error"""
        m = _target_mode(mode)
        for h in self._ctxs:
            _capi.check(h, self._lib.msplat_set_target_mode(h, m))
        self._load = m == _capi.TARGET_LOAD

    def target_mode(self):
        """"clear" / "load" / "premultiplied" of the current context (msplat_get_target_mode); None without a context"""
        k = self._lib.msplat_get_target_mode(self._ctx) if self._ctx else -1
        return {v: n for n, v in _capi.TARGET_MODES.items()}.get(k)

    # -- per-splat visibility (msplat_set_visibility / msplat_set_crop) ---------------
    def SetVisibility(self, mask=None):
        """Hide splats without another upload: for the following Sorts splat i (upload numbering) takes part iff mask[i] (and the
        crop keeps it).  mask: N values, numpy bool / uint8 (nonzero = visible; copied before the call returns), or an object with
        data_ptr() that lives on the device -- a torch bool / uint8 tensor on this renderer's device, read asynchronously on each
        context's stream: keep it alive and unchanged until synchronize() -- or None for no mask.  Set on every context of the
        frames-in-flight rotation; a Render shows it after the next Sort.  An upload (Init*, Update*) drops the mask.
        The argument is remembered: TransformCloud keeps the mask and hands it to the contexts it attaches again, so a
        device-tensor mask must still hold the mask at that point.
        ValueError for a wrong length or dtype, before the library is called."""
        if mask is None:
            args, fn = (None, 0), self._lib.msplat_set_visibility
        elif hasattr(mask, "data_ptr"):
            if str(mask.dtype).split(".")[-1] not in ("bool", "uint8"):
                raise ValueError("the mask must be bool or uint8, not %s" % mask.dtype)
            if tuple(int(s) for s in mask.shape) != (self._n,):
                raise ValueError("the mask must have shape (%d,), one value per splat, not %s" % (self._n, tuple(mask.shape)))
            if not mask.is_contiguous():
                raise ValueError("the mask must be contiguous (pass mask.contiguous())")
            if getattr(mask.device, "type", "cuda") not in ("cuda", "hip"):
                raise ValueError("a mask with data_ptr() must live in device memory, not on %s (pass mask.numpy())" % mask.device)
            import sys
            torch = sys.modules.get("torch")
            if torch is not None and isinstance(mask, torch.Tensor):
                torch.cuda.current_stream(mask.device).synchronize()       # what produced the tensor has completed
            args, fn = (C.c_void_p(int(mask.data_ptr())), self._n), self._lib.msplat_set_visibility_device
        else:
            if not isinstance(mask, np.ndarray) or mask.dtype not in (np.bool_, np.uint8):
                raise ValueError("the mask must be a numpy bool / uint8 array, a device tensor or None, not %s %s"
                                 % (type(mask).__name__, getattr(mask, "dtype", "")))
            if mask.shape != (self._n,):
                raise ValueError("the mask must have shape (%d,), one value per splat, not %s" % (self._n, mask.shape))
            mask = np.ascontiguousarray(mask)
            args, fn = (mask.ctypes.data, self._n), self._lib.msplat_set_visibility
        if not self._ctxs:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "SetVisibility: no cloud (Init first)")
        for h in self._ctxs:
            _capi.check(h, fn(h, *args))
        self._vis_arg = mask                 # (TransformCloud hands it to the contexts it attaches again)

    def SetCrop(self, worldToCrop=None, shape="box", invert=False):
        """Crop volume for the following Sorts, on every context: worldToCrop = 16 floats, column-major, world -> crop space (affine),
        shape "box" (|q| <= 1 per axis) or "sphere" (|q|^2 <= 1) in crop space, invert = keep what is OUTSIDE.  None = no crop.
        A centre on the surface is inside; the exact fp32 rule is msplat.h's.  An upload keeps the crop."""
        if worldToCrop is None:
            m, code = None, _capi.CROP_NONE
        else:
            if shape not in _capi.CROP_SHAPES:
                raise ValueError("shape must be one of %s (got %r)" % (sorted(_capi.CROP_SHAPES), shape))
            m = np.ascontiguousarray(_FrameArgs._flat(worldToCrop, 16))
            code = _capi.CROP_SHAPES[shape] | (_capi.CROP_INVERT if invert else 0)
        for h in self._ctxs:
            _capi.check(h, self._lib.msplat_set_crop(h, None if m is None else m.ctypes.data_as(C.POINTER(C.c_float)), code))

    def visibility(self):
        """dict(has_mask, crop, hidden) of the current context (msplat_get_visibility): crop = None or (shape, invert); hidden =
        splats the latest Sort's mask and crop hid (synchronises)"""
        a, b, h = C.c_int32(), C.c_int32(), C.c_uint64()
        _capi.check(self._ctx, self._lib.msplat_get_visibility(self._ctx, C.byref(a), C.byref(b), C.byref(h)))
        names = {v: n for n, v in _capi.CROP_SHAPES.items()}
        crop = None if b.value == _capi.CROP_NONE else (names[b.value & ~_capi.CROP_INVERT], bool(b.value & _capi.CROP_INVERT))
        return dict(has_mask=bool(a.value), crop=crop, hidden=int(h.value))

    # -- render-time overlay (msplat_set_overlay* / msplat_set_overlay_palette) -------
    def SetOverlay(self, classes=_KEEP, palette=_KEEP):
        """Tint splats by class at render time, without touching the cloud: splat i (upload numbering) of class classes[i] = k is
        shown with each colour lane c of its projected record replaced by (1 - a) c + a h, (h_r, h_g, h_b, a) = palette[k]; a class
        >= len(palette) or an entry with a == 0 has no effect; the exact fp32 rule is msplat.h's.  Shows at the next Render, no Sort
        needed.  classes: N values, numpy uint8 / bool (copied before the call returns), or an object with data_ptr() that lives on
        the device -- a torch uint8 / bool tensor on this renderer's device, e.g. the array MarkIds / MarkScores wrote, read
        asynchronously on each context's stream: keep it alive and unchanged until synchronize() -- or None for no classes.
        palette: (count, 4) floats, count <= 256, finite, a in [0, 1], or None for no palette.  An argument left out stays as it is.
        Set on every context of the frames-in-flight rotation.  An upload (Init*, Update*) and CompactCloud drop the classes and keep
        the palette (Init* hands it to the new contexts); TransformCloud and AppendCloud keep the classes and hand the remembered
        argument to the contexts they attach again -- AppendCloud extended by K values of class 0 -- so a device-tensor argument must
        still hold the classes at that point.  ValueError for a wrong length, shape or dtype, before the library is called."""
        if palette is not _KEEP and palette is not None:
            palette = np.ascontiguousarray(np.asarray(palette, dtype=np.float32))
            if palette.ndim != 2 or palette.shape[1] != 4 or palette.shape[0] > 256:
                raise ValueError("the palette must have shape (count, 4) with count <= 256, not %s" % (palette.shape,))
            if not np.isfinite(palette).all() or (palette[:, 3] < 0).any() or (palette[:, 3] > 1).any():
                raise ValueError("the palette must be finite with a in [0, 1]")
        if classes is _KEEP:
            args = fn = None
        elif classes is None:
            args, fn = (None, 0), self._lib.msplat_set_overlay
        elif hasattr(classes, "data_ptr"):
            if str(classes.dtype).split(".")[-1] not in ("bool", "uint8"):
                raise ValueError("the classes must be uint8 or bool, not %s" % classes.dtype)
            if tuple(int(s) for s in classes.shape) != (self._n,):
                raise ValueError("the classes must have shape (%d,), one value per splat, not %s" % (self._n, tuple(classes.shape)))
            if not classes.is_contiguous():
                raise ValueError("the classes must be contiguous (pass classes.contiguous())")
            if getattr(classes.device, "type", "cuda") not in ("cuda", "hip"):
                raise ValueError("classes with data_ptr() must live in device memory, not on %s (pass classes.numpy())" % classes.device)
            import sys
            torch = sys.modules.get("torch")
            if torch is not None and isinstance(classes, torch.Tensor):
                torch.cuda.current_stream(classes.device).synchronize()    # what produced the tensor has completed
            args, fn = (C.c_void_p(int(classes.data_ptr())), self._n), self._lib.msplat_set_overlay_device
        else:
            if not isinstance(classes, np.ndarray) or classes.dtype not in (np.bool_, np.uint8):
                raise ValueError("the classes must be a numpy uint8 / bool array, a device tensor or None, not %s %s"
                                 % (type(classes).__name__, getattr(classes, "dtype", "")))
            if classes.shape != (self._n,):
                raise ValueError("the classes must have shape (%d,), one value per splat, not %s" % (self._n, classes.shape))
            classes = np.ascontiguousarray(classes)
            args, fn = (classes.ctypes.data, self._n), self._lib.msplat_set_overlay
        if fn is not None and classes is not None and not self._ctxs:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "SetOverlay: no cloud (Init first)")
        if palette is not _KEEP:
            for h in self._ctxs:
                _capi.check(h, self._lib.msplat_set_overlay_palette(h, None if palette is None else palette.ctypes.data,
                                                                    0 if palette is None else palette.shape[0]))
            self._ov_palette = palette
        if fn is not None:
            for h in self._ctxs:
                _capi.check(h, fn(h, *args))
            self._ov_arg = classes

    def overlay(self):
        """dict(has_classes, palette_count, active) of the current context (msplat_get_overlay)"""
        a, b, c = C.c_int32(), C.c_uint32(), C.c_int32()
        _capi.check(self._ctx, self._lib.msplat_get_overlay(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return dict(has_classes=bool(a.value), palette_count=int(b.value), active=bool(c.value))

    def _overlay_again(self, classed, added=0):
        """the contexts TransformCloud / AppendCloud / AdjustCloud attached again receive the remembered classes, `added` values of class 0 longer"""
        ov = self._ov_arg
        if not classed or ov is None:
            return
        if added:
            if hasattr(ov, "data_ptr"):
                import torch
                ov = torch.cat([ov.to(torch.uint8), torch.zeros(added, dtype=torch.uint8, device=ov.device)])
            else:
                ov = np.concatenate([ov.view(np.uint8), np.zeros(added, np.uint8)])
        ctxs, self._ctxs = self._ctxs, self._ctxs[1:]
        try:
            if self._ctxs:
                self.SetOverlay(ov)
            self._ov_arg = ov
        finally:
            self._ctxs = ctxs

    def CompactCloud(self, index_map=False):
        """Make the mask and the crop permanent, on the device (msplat_compact_cloud): the cloud becomes the K
        splats SetVisibility's mask and SetCrop's volume let through, renumbered 0..K-1 in ascending old index, their records
        copied bit for bit -- the renderer afterwards is one that was Init'ed with those rows.  Every frame in flight is finished
        first; context 0 (it holds the mask SetVisibility set on every context) is compacted, the others are attached again and
        the next Sort lands on context 0, as after Init.  The masks of all contexts are gone, the crop stays; Sort before the
        next Render.  Returns K, or with index_map=True (K, map): a torch int32 tensor of the old N on this renderer's device,
        map[i] = new index of splat i, -1 where it was dropped -- what the caller's per-splat arrays follow."""
        if not self._ctxs:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "CompactCloud: no cloud (Init first)")
        self.synchronize()
        own = self._ctxs[0]
        m = None
        if index_map:
            import torch
            m = torch.empty(max(self._n, 1), dtype=torch.int32, device=torch.device("cuda", self._device))
            torch.cuda.current_stream(m.device).synchronize()
        k = C.c_uint64()
        _capi.check(own, self._lib.msplat_compact_cloud(own, C.c_void_p(m.data_ptr()) if m is not None else None, C.byref(k)))
        n_old, self._n = self._n, int(k.value)
        self._ctx = own
        self._cur = self._depth - 1          # the next Sort lands on context 0, as after Init
        if not self._attach_all():
            raise _capi.MsplatError(_capi.ERR_HIP, "CompactCloud: attaching the compacted cloud failed: " + self._err)
        return (self._n, m[:n_old]) if index_map else self._n

    def _device_select(self, select, n):
        """a select argument (None, numpy bool / uint8 -- staged to the device through torch -- or a torch bool / uint8 tensor on
        this renderer's device) of n values as the c_void_p the library takes (None: every splat, or n == 0); SetVisibility's
        checks, ValueError before the library is called.  The tensor is kept alive in self._select_arg until the next call."""
        self._select_arg = None
        if select is None:
            return None
        if not hasattr(select, "data_ptr"):
            if not isinstance(select, np.ndarray) or select.dtype not in (np.bool_, np.uint8):
                raise ValueError("select must be a numpy bool / uint8 array, a device tensor or None, not %s %s"
                                 % (type(select).__name__, getattr(select, "dtype", "")))
            if select.shape != (n,):
                raise ValueError("select must have shape (%d,), one value per splat, not %s" % (n, select.shape))
            import torch
            select = torch.from_numpy(np.ascontiguousarray(select).view(np.uint8)).to(torch.device("cuda", self._device))
        if str(select.dtype).split(".")[-1] not in ("bool", "uint8"):
            raise ValueError("select must be bool or uint8, not %s" % select.dtype)
        if tuple(int(s) for s in select.shape) != (n,):
            raise ValueError("select must have shape (%d,), one value per splat, not %s" % (n, tuple(select.shape)))
        if not select.is_contiguous():
            raise ValueError("select must be contiguous (pass select.contiguous())")
        if getattr(select.device, "type", "cuda") not in ("cuda", "hip"):
            raise ValueError("a select with data_ptr() must live in device memory, not on %s (pass select.numpy())" % select.device)
        import sys
        torch = sys.modules.get("torch")
        if torch is not None and isinstance(select, torch.Tensor):
            torch.cuda.current_stream(select.device).synchronize()     # what produced the tensor has completed
        self._select_arg = select
        return C.c_void_p(int(select.data_ptr())) if n else None

    def TransformCloud(self, M, select=None, keep_sh=False):
        """Move, rotate and scale splats on the device (msplat_transform_cloud): every splat i with select[i]
        (None: every splat) gets centre M x, covariance A S A^T (A = M's upper 3x3) and, unless keep_sh, SH bands 1..3 rotated by
        msplat_sh_rotation(M); the others are copied bit for bit.  M: 16 floats, column-major; without keep_sh it must be a rotation
        times a uniform positive scale (MsplatError ERR_UNSUPPORTED else).  select: N values, numpy bool / uint8 (staged to the
        device through torch) or a torch bool / uint8 tensor on this renderer's device -- SetVisibility's checks, ValueError before
        the library is called.  The renderer afterwards is one that was Init'ed with those rows, except that the numbering, and
        with it the mask, stays: every frame in flight is finished first; context 0 is transformed, the others are attached again
        (attaching drops their masks) and are handed SetVisibility's last argument again -- a device-tensor mask must still hold
        the mask at that point.  The crop stays; Sort before the next Render."""
        if not self._ctxs:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "TransformCloud: no cloud (Init first)")
        m = np.ascontiguousarray(_FrameArgs._flat(M, 16))
        sel = self._device_select(select, self._n)
        self.synchronize()
        own = self._ctxs[0]
        masked, classed = C.c_int32(), C.c_int32()
        _capi.check(own, self._lib.msplat_get_visibility(own, C.byref(masked), None, None))
        _capi.check(own, self._lib.msplat_get_overlay(own, C.byref(classed), None, None))
        _capi.check(own, self._lib.msplat_transform_cloud(own, m.ctypes.data_as(C.POINTER(C.c_float)), sel, self._n,
                                                          _capi.TRANSFORM_KEEP_SH if keep_sh else 0))
        self._ctx = own
        self._cur = self._depth - 1          # the next Sort lands on context 0, as after Init
        if not self._attach_all():
            raise _capi.MsplatError(_capi.ERR_HIP, "TransformCloud: attaching the transformed cloud failed: " + self._err)
        if masked.value and len(self._ctxs) > 1 and getattr(self, "_vis_arg", None) is not None:
            ctxs, self._ctxs = self._ctxs, self._ctxs[1:]
            try:
                self.SetVisibility(self._vis_arg)
            finally:
                self._ctxs = ctxs
        self._overlay_again(classed.value)

    def AdjustCloud(self, colour=None, opacity=None, select=None):
        """Recolour and fade splats on the device (msplat_adjust_cloud): every splat i with select[i] (None:
        every splat) gets, with colour, the affine map col' = G col + o of its colour in every view direction -- applied to its SH
        coefficients, in the record's colour space -- and, with opacity, alpha' = clamp(opacity * alpha, 0, 1) and the footprint
        bound that goes with it; the others are copied bit for bit.  colour: a (3, 4) array-like in the row form [G | o]
        (tint_matrix, gain_matrix); opacity: a finite factor >= 0.  An argument left None leaves its part of the record alone (a
        fade never re-quantises an "sh_q8" cloud); both None is a ValueError.  select: N values, as TransformCloud takes them.
        The renderer afterwards is one that was Init'ed with those rows, except that the numbering, and with it the mask and the
        overlay's classes, stays: every frame in flight is finished first; context 0 is adjusted, the others are attached again
        and are handed SetVisibility's and SetOverlay's last arguments again, exactly as after TransformCloud.  The crop stays;
        Sort before the next Render."""
        if colour is None and opacity is None:
            raise ValueError("AdjustCloud: pass colour=, opacity= or both")
        flags, c12, scale = 0, None, 1.0
        if colour is not None:
            g = np.asarray(colour, np.float32)
            if g.shape != (3, 4):
                raise ValueError("colour must have shape (3, 4), the rows of [G | o], not %s" % (g.shape,))
            if not np.isfinite(g).all():
                raise ValueError("colour must be finite")
            c12 = np.ascontiguousarray(g.T.reshape(12))          # column-major: G's columns, then o
            flags |= _capi.ADJUST_COLOUR
        if opacity is not None:
            scale = float(opacity)
            if not np.isfinite(scale) or scale < 0.0:
                raise ValueError("opacity must be a finite factor >= 0, not %r" % (opacity,))
            flags |= _capi.ADJUST_OPACITY
        if not self._ctxs:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "AdjustCloud: no cloud (Init first)")
        sel = self._device_select(select, self._n)
        self.synchronize()
        own = self._ctxs[0]
        masked, classed = C.c_int32(), C.c_int32()
        _capi.check(own, self._lib.msplat_get_visibility(own, C.byref(masked), None, None))
        _capi.check(own, self._lib.msplat_get_overlay(own, C.byref(classed), None, None))
        _capi.check(own, self._lib.msplat_adjust_cloud(own, c12.ctypes.data_as(C.POINTER(C.c_float)) if c12 is not None else None,
                                                       C.c_float(scale), sel, self._n, flags))
        self._ctx = own
        self._cur = self._depth - 1          # the next Sort lands on context 0, as after Init
        if not self._attach_all():
            raise _capi.MsplatError(_capi.ERR_HIP, "AdjustCloud: attaching the adjusted cloud failed: " + self._err)
        if masked.value and len(self._ctxs) > 1 and getattr(self, "_vis_arg", None) is not None:
            ctxs, self._ctxs = self._ctxs, self._ctxs[1:]
            try:
                self.SetVisibility(self._vis_arg)
            finally:
                self._ctxs = ctxs
        self._overlay_again(classed.value)

    def AppendCloud(self, src, select=None, index_map=False):
        """Put splats into the cloud on the device (msplat_append_cloud): every splat i of src -- another
        SplatRenderer on this device, or this one: a duplicate -- with select[i] (None: every splat) is appended behind this
        renderer's own, in ascending source index; the old splats keep their indices 0..N-1, the K new ones get N..N+K-1.  Rows are
        copied bit for bit where both clouds are stored alike and converted through their FP32 values where not; the cloud keeps
        its storage kind.  select: Ns values, as TransformCloud takes them.  The renderer afterwards is one that was Init'ed with
        the N+K rows, except that the old numbering, and with it the mask, stays, K visible values longer: every frame in flight
        of both renderers is finished first; context 0 appends, the others are attached again (attaching drops their masks) and
        are handed SetVisibility's last argument, K visible values longer -- a device-tensor mask must still hold the mask.  The crop
        stays; Sort before the next Render.  Returns (K, map): map = None, or with index_map=True a torch int32 tensor of Ns on
        this renderer's device, map[i] = new index of source splat i, -1 where it was not selected."""
        if not self._ctxs:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "AppendCloud: no cloud (Init first; Init of 0 rows makes an empty one)")
        if not isinstance(src, SplatRenderer) or not src._ctxs:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "AppendCloud: src is not a SplatRenderer with a cloud")
        ns = src._n
        sel = self._device_select(select, ns)
        self.synchronize()
        if src is not self:
            src.synchronize()
        own = self._ctxs[0]
        m = None
        if index_map:
            import torch
            m = torch.empty(max(ns, 1), dtype=torch.int32, device=torch.device("cuda", self._device))
            torch.cuda.current_stream(m.device).synchronize()
        k, masked, classed = C.c_uint64(), C.c_int32(), C.c_int32()
        _capi.check(own, self._lib.msplat_get_visibility(own, C.byref(masked), None, None))
        _capi.check(own, self._lib.msplat_get_overlay(own, C.byref(classed), None, None))
        _capi.check(own, self._lib.msplat_append_cloud(own, src._ctxs[0], sel, ns, C.c_void_p(m.data_ptr()) if m is not None else None,
                                                       C.byref(k)))
        self._select_arg = None
        self._n += int(k.value)
        self._ctx = own
        self._cur = self._depth - 1          # the next Sort lands on context 0, as after Init
        if not self._attach_all():
            raise _capi.MsplatError(_capi.ERR_HIP, "AppendCloud: attaching the merged cloud failed: " + self._err)
        vis = getattr(self, "_vis_arg", None)
        if masked.value and vis is not None:
            if hasattr(vis, "data_ptr"):
                import torch
                vis = torch.cat([vis.to(torch.uint8), torch.ones(int(k.value), dtype=torch.uint8, device=vis.device)])
            else:
                vis = np.concatenate([vis.view(np.uint8), np.ones(int(k.value), np.uint8)])
            ctxs, self._ctxs = self._ctxs, self._ctxs[1:]
            try:
                if self._ctxs:
                    self.SetVisibility(vis)
                self._vis_arg = vis
            finally:
                self._ctxs = ctxs
        self._overlay_again(classed.value, int(k.value))
        return int(k.value), (m[:ns] if index_map else None)

    # -- which splat each pixel shows (msplat_render_ids / msplat_mark_ids) -----------
    def RenderIds(self, cameraMat, projMat, viewport, nearFar, window=None, out=None, out_ptr=None, pitch_bytes=0, depth=False,
                  depth_ptr=None, depth_pitch_bytes=0):
        """Per pixel the upload index of the splat of the latest Sort that contributes most to it (ID_NONE = 0xFFFFFFFF where no
        splat reaches), over window = (x0, y0, w, h) in viewport pixels, row 0 = GL bottom; None = the whole viewport.
        out=None -> returns a new (h, w) uint32 array; out=ndarray -> filled in place; depth=True (or an (h, w) float32 array) ->
        returns (ids, depth), depth = that splat's window depth, 1.0 at ID_NONE.  out_ptr=int -> device memory, rows of pitch_bytes
        (0 = tight), asynchronous on the stream, returns None; depth_ptr=int (rows of depth_pitch_bytes) goes with out_ptr.
        ValueError for a window, array or pitch that cannot be right, before the library is called."""
        f = self._args.load(cameraMat, projMat, viewport, nearFar)
        W, H = int(self._args.vp[2]), int(self._args.vp[3])
        if window is None:
            win, (w, h) = None, (W, H)
        else:
            if len(window) != 4 or any(int(v) != v for v in window):
                raise ValueError("window must be four integers (x0, y0, w, h), not %r" % (window,))
            x0, y0, w, h = (int(v) for v in window)
            if w <= 0 or h <= 0 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
                raise ValueError("window %r is empty or not inside the %d x %d viewport" % (tuple(window), W, H))
            win = (C.c_int32 * 4)(x0, y0, w, h)
        for name, pitch in (("pitch_bytes", pitch_bytes), ("depth_pitch_bytes", depth_pitch_bytes)):
            if pitch and (pitch < 4 * w or pitch % 4):
                raise ValueError("%s must be 0 (tight rows) or at least %d and a multiple of 4, not %d" % (name, 4 * w, pitch))
        if out_ptr is not None:
            if out is not None or (depth is not None and depth is not False):
                raise ValueError("the planes live in one memory space: pass depth_ptr= with out_ptr=")
            _capi.check(self._ctx, self._lib.msplat_render_ids(self._ctx, *f, win, C.c_void_p(out_ptr), pitch_bytes,
                                                               C.c_void_p(depth_ptr) if depth_ptr is not None else None, depth_pitch_bytes, 1))
            return None
        if depth_ptr is not None:
            raise ValueError("the planes live in one memory space: pass depth= with host output")
        if pitch_bytes or depth_pitch_bytes:
            raise ValueError("host arrays have tight rows: pitch_bytes / depth_pitch_bytes go with out_ptr=")
        if out is None:
            out = np.empty((h, w), np.uint32)
        elif not isinstance(out, np.ndarray) or out.dtype != np.uint32 or out.shape != (h, w) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out= takes a C-contiguous uint32 array of shape (%d, %d)" % (h, w))
        if depth is False:
            depth = None
        if depth is True:
            depth = np.empty((h, w), np.float32)
        d = self._host_plane("depth=", depth, h, w).ctypes.data if depth is not None else None
        _capi.check(self._ctx, self._lib.msplat_render_ids(self._ctx, *f, win, out.ctypes.data, 0, d, 0, 0))
        return out if depth is None else (out, depth)

    def Pick(self, cameraMat, projMat, viewport, nearFar, x, y):
        """(index, z_w) of the splat pixel (x, y) of the viewport shows (row 0 = GL bottom): RenderIds through a 1 x 1 window.
        index is None, and z_w 1.0, where no splat reaches."""
        ids, z = self.RenderIds(cameraMat, projMat, viewport, nearFar, window=(x, y, 1, 1), depth=True)
        i = int(ids[0, 0])
        return (None if i == _capi.ID_NONE else i), float(z[0, 0])

    def MarkIds(self, ids_ptr, pitch_bytes, w, h, mask_ptr, value, region_ptr=None, region_pitch_bytes=0):
        """mask[id] = value for every pixel of the w x h id plane at device pointer ids_ptr (rows of pitch_bytes, 0 = tight) that
        the byte plane region_ptr selects (nonzero; None = every pixel; rows of region_pitch_bytes, 0 = w) and whose id is a
        splat.  mask_ptr: N bytes of device memory -- what SetVisibility takes.  Asynchronous on the current context's stream,
        behind the RenderIds(out_ptr=) that wrote the plane."""
        w, h, value = int(w), int(h), int(value)
        if w < 0 or h < 0:
            raise ValueError("w and h must not be negative (got %d x %d)" % (w, h))
        if not 0 <= value <= 255:
            raise ValueError("value is one byte, 0..255 (got %d)" % value)
        if pitch_bytes and (pitch_bytes < 4 * w or pitch_bytes % 4):
            raise ValueError("pitch_bytes must be 0 (tight rows) or at least %d and a multiple of 4, not %d" % (4 * w, pitch_bytes))
        if region_ptr is not None and region_pitch_bytes and region_pitch_bytes < w:
            raise ValueError("region_pitch_bytes must be 0 (tight rows) or at least %d, not %d" % (w, region_pitch_bytes))
        if not ids_ptr or not mask_ptr:
            raise ValueError("ids_ptr and mask_ptr are device pointers, not %r / %r" % (ids_ptr, mask_ptr))
        if not self._ctx:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "MarkIds: no cloud (Init first)")
        _capi.check(self._ctx, self._lib.msplat_mark_ids(self._ctx, C.c_void_p(int(ids_ptr)), pitch_bytes, w, h,
                                                         C.c_void_p(int(region_ptr)) if region_ptr is not None else None,
                                                         region_pitch_bytes, C.c_void_p(int(mask_ptr)), self._n, value))

    # -- how much of the frame each splat contributes (msplat_render_scores / msplat_mark_scores) --
    def _device_vector(self, name, t, dtype):
        """a contiguous torch tensor of N values of `dtype` on this renderer's device (ValueError otherwise)"""
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (self._n,) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous torch %s tensor of shape (%d,)" % (name, str(dtype).split(".")[-1], self._n))
        if t.device.type != "cuda" or (t.device.index or 0) != self._device:
            raise ValueError("%s must live on device %d, not on %s" % (name, self._device, t.device))
        return t

    def _window_and_region(self, window, region):
        """the window and region arguments of RenderScores / MarkView for the viewport self._args holds, as the library takes them:
        (c_int32[4] or None, the region tensor -- kept alive by the caller --, its pointer or None, its pitch).  ValueError for
        arguments that cannot be right"""
        import torch
        W, H = int(self._args.vp[2]), int(self._args.vp[3])
        if window is None:
            win, (w, h) = None, (W, H)
        else:
            if len(window) != 4 or any(int(v) != v for v in window):
                raise ValueError("window must be four integers (x0, y0, w, h), not %r" % (window,))
            x0, y0, w, h = (int(v) for v in window)
            if w <= 0 or h <= 0 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
                raise ValueError("window %r is empty or not inside the %d x %d viewport" % (tuple(window), W, H))
            win = (C.c_int32 * 4)(x0, y0, w, h)
        dev = torch.device("cuda", self._device)
        region_ptr, region_pitch = None, 0
        if region is not None:
            if isinstance(region, np.ndarray):
                region = torch.from_numpy(np.ascontiguousarray(region)).to(dev)
            if (not isinstance(region, torch.Tensor) or region.dtype not in (torch.uint8, torch.bool) or tuple(region.shape) != (h, w)
                    or (w > 1 and region.stride(1) != 1) or (h > 1 and region.stride(0) < w)):
                raise ValueError("region must be a uint8 / bool plane of shape (%d, %d) with unit column stride" % (h, w))
            if region.device != dev:
                raise ValueError("region must live on %s, not on %s" % (dev, region.device))
            region_ptr, region_pitch = C.c_void_p(region.data_ptr()), (region.stride(0) if h > 1 else w)
        return win, region, region_ptr, region_pitch

    def RenderScores(self, cameraMat, projMat, viewport, nearFar, window=None, region=None, score=None, pixels=False):
        """Per splat of the cloud (upload numbering) what it contributes to the view: score[i] += the sum over the pixels of
        window = (x0, y0, w, h) (viewport pixels, row 0 = GL bottom; None = the whole viewport) of rint(T_i w_i 2^23), over the
        splats of the latest Sort; _capi.SCORE_ONE is one fully covered pixel.  region: an (h, w) uint8 / bool plane of the WINDOW,
        nonzero = the pixel counts -- a torch tensor on this renderer's device (rows may be strided) or a numpy array; None = all.
        Returns a torch int64 tensor on the renderer's device (the values stay below 2^63), or (score, hits) with pixels=True
        (or an int32 tensor): hits[i] += the number of those pixels with a nonzero term.  score=None allocates zeroed tensors,
        waits for the frame and runs it once more from fresh zeros if the pair buffer overflowed; a given score (int64) / pixels
        (int32) tensor is accumulated into -- one call per camera sums over views -- asynchronously on the context's stream,
        which torch's current stream is made to wait for.  ValueError for arguments that cannot be right, before the library is
        called."""
        import torch
        f = self._args.load(cameraMat, projMat, viewport, nearFar)
        dev = torch.device("cuda", self._device)
        win, region, region_ptr, region_pitch = self._window_and_region(window, region)
        own = score is None
        if own and isinstance(pixels, torch.Tensor):
            raise ValueError("a pixels tensor goes with a score tensor: both are accumulated into")
        if not own:
            self._device_vector("score", score, torch.int64)
            if pixels is True:
                raise ValueError("with a score tensor pass the int32 tensor to accumulate the hit counts into as pixels=")
        hits = self._device_vector("pixels", pixels, torch.int32) if isinstance(pixels, torch.Tensor) else None
        if not self._ctx:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "RenderScores: no cloud (Init first)")

        def issue():
            torch.cuda.current_stream(dev).synchronize()                # what produced the tensors has completed
            _capi.check(self._ctx, self._lib.msplat_render_scores(self._ctx, *f, win, region_ptr, region_pitch, C.c_void_p(score.data_ptr()),
                                                                  C.c_void_p(hits.data_ptr()) if hits is not None else None, self._n))
        if not own:
            issue()
            self.wait_on_stream(torch.cuda.current_stream(dev).cuda_stream)
            return score if hits is None else (score, hits)
        for attempt in range(2):
            score = torch.zeros(self._n, dtype=torch.int64, device=dev)
            hits = torch.zeros(self._n, dtype=torch.int32, device=dev) if pixels else None
            issue()
            try:
                _capi.check(self._ctx, self._lib.msplat_synchronize(self._ctx))
                break
            except _capi.MsplatError as e:                              # this frame's overflow: the buffer has grown
                if e.code != _capi.ERR_PAIR_OVERFLOW or attempt:
                    raise
        return score if hits is None else (score, hits)

    def MarkScores(self, score, op, threshold, mask, value):
        """mask[i] = value for every splat whose score[i] is below `threshold` (op "below") or at least it ("at_least"); other
        bytes stay (msplat_mark_scores).  score: the int64 tensor RenderScores returns; mask: a torch uint8 / bool tensor of N
        bytes on the same device -- what SetVisibility takes.  "below" with value 0 on a mask of ones prunes, "at_least" with
        value 1 on zeros selects.  Asynchronous on the current context's stream, behind the score frames that wrote `score`;
        torch's current stream is made to wait for it.  threshold: 0 .. 2^64 - 1."""
        import torch
        if op not in _capi.SCORE_OPS:
            raise ValueError("op must be one of %s (got %r)" % (sorted(_capi.SCORE_OPS), op))
        value, threshold = int(value), int(threshold)
        if not 0 <= value <= 255:
            raise ValueError("value is one byte, 0..255 (got %d)" % value)
        if not 0 <= threshold < 2 ** 64:
            raise ValueError("threshold is an unsigned 64-bit value (got %d)" % threshold)
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError("mask must be a torch uint8 / bool tensor")
        self._device_vector("score", score, torch.int64)
        self._device_vector("mask", mask, mask.dtype)
        if not self._ctx:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "MarkScores: no cloud (Init first)")
        dev = torch.device("cuda", self._device)
        torch.cuda.current_stream(dev).synchronize()
        _capi.check(self._ctx, self._lib.msplat_mark_scores(self._ctx, C.c_void_p(score.data_ptr()), self._n, _capi.SCORE_OPS[op], threshold,
                                                            C.c_void_p(mask.data_ptr()), value))
        self.wait_on_stream(torch.cuda.current_stream(dev).cuda_stream)

    # -- selection by position (msplat_mark_volume / msplat_mark_view / msplat_measure_cloud) --
    def _mark_target(self, who, mask, value):
        """MarkScores' checks of a mask tensor and a byte; torch's current stream has completed on return"""
        import torch
        value = int(value)
        if not 0 <= value <= 255:
            raise ValueError("value is one byte, 0..255 (got %d)" % value)
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError("mask must be a torch uint8 / bool tensor")
        self._device_vector("mask", mask, mask.dtype)
        if not self._ctx:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "%s: no cloud (Init first)" % who)
        torch.cuda.current_stream(torch.device("cuda", self._device)).synchronize()
        return value

    def MarkVolume(self, worldToVolume, mask, value, shape="box", invert=False):
        """mask[i] = value for every splat whose centre lies in the volume (invert: outside it); other bytes stay
        (msplat_mark_volume).  worldToVolume, shape, invert: exactly SetCrop's arguments and SetCrop's fp32 rule -- a centre on
        the surface is inside, a NaN centre outside -- applied to the cloud itself: splats a mask or a crop hides are marked like
        any other.  mask: a torch uint8 / bool tensor of N bytes on this renderer's device, what SetVisibility, SetOverlay and the
        select= of the cloud edits take.  No Sort is needed.  Asynchronous on the current context's stream; torch's current
        stream is made to wait for it."""
        import torch
        if shape not in _capi.CROP_SHAPES:
            raise ValueError("shape must be one of %s (got %r)" % (sorted(_capi.CROP_SHAPES), shape))
        m = np.ascontiguousarray(_FrameArgs._flat(worldToVolume, 16))
        value = self._mark_target("MarkVolume", mask, value)
        code = _capi.CROP_SHAPES[shape] | (_capi.CROP_INVERT if invert else 0)
        _capi.check(self._ctx, self._lib.msplat_mark_volume(self._ctx, m.ctypes.data_as(C.POINTER(C.c_float)), code, C.c_void_p(mask.data_ptr()),
                                                            self._n, value))
        self.wait_on_stream(torch.cuda.current_stream(torch.device("cuda", self._device)).cuda_stream)

    def MarkView(self, cameraMat, projMat, viewport, nearFar, mask, value, window=None, region=None):
        """Select through: mask[i] = value for every splat in front of the camera whose projected CENTRE falls on a pixel of
        window = (x0, y0, w, h) (viewport pixels, row 0 = GL bottom; None = the whole viewport) that region selects -- an (h, w)
        uint8 / bool plane of the window as RenderScores takes it; None = all; other bytes stay (msplat_mark_view).  Occluded
        splats are marked like visible ones: a rectangle or lasso takes the whole object, not its visible skin; intersect with a
        RenderScores mask for the visible part.  The cloud itself is tested, whatever a mask or crop hides; no Sort is needed;
        nearFar is not read.  Asynchronous on the current context's stream; torch's current stream is made to wait for it."""
        import torch
        f = self._args.load(cameraMat, projMat, viewport, nearFar)
        win, region, region_ptr, region_pitch = self._window_and_region(window, region)
        value = self._mark_target("MarkView", mask, value)
        _capi.check(self._ctx, self._lib.msplat_mark_view(self._ctx, *f, win, region_ptr, region_pitch, C.c_void_p(mask.data_ptr()), self._n, value))
        self.wait_on_stream(torch.cuda.current_stream(torch.device("cuda", self._device)).cuda_stream)

    def MeasureCloud(self, select=None):
        """Where a selection is (msplat_measure_cloud): a dict of selected, finite (ints), lo, hi (float32[3]), reach2_max
        (float32), sum (float64[3]), sum2 (float64[6]: xx yy zz xy xz yz) over the splats with select[i] (None: all; N values as
        TransformCloud takes them) -- finite and everything after it over the finite centres among them -- plus, derived here in
        float64, mean (None when finite == 0) and covariance (3 x 3, the population covariance sum2 / finite - mean mean^T).  The
        cloud itself is measured, whatever a mask or crop hides.  Synchronous."""
        if not self._ctx:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "MeasureCloud: no cloud (Init first)")
        sel = self._device_select(select, self._n)
        m = _capi.CloudMeasure(struct_size=C.sizeof(_capi.CloudMeasure))
        _capi.check(self._ctx, self._lib.msplat_measure_cloud(self._ctx, sel, self._n, C.byref(m)))
        out = dict(selected=int(m.selected), finite=int(m.finite), lo=np.array(m.lo, np.float32), hi=np.array(m.hi, np.float32),
                   reach2_max=np.float32(m.reach2_max), sum=np.array(m.sum, np.float64), sum2=np.array(m.sum2, np.float64))
        out["mean"] = out["covariance"] = None
        if out["finite"]:
            mean = out["sum"] / out["finite"]
            xx, yy, zz, xy, xz, yz = out["sum2"] / out["finite"]
            out["mean"] = mean
            out["covariance"] = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]) - np.outer(mean, mean)
        return out

    # -- selection by attribute (msplat_cloud_values / msplat_mark_values / msplat_histogram_values) --
    def CloudValues(self, kind, param=None, out=None):
        """What every splat is, one float32 per splat in upload numbering (msplat_cloud_values).  kind: a name of
        _capi.VALUE_KINDS ("x", "y", "z", "reach2", "distance2", "alpha", "red", "green", "blue", "colour_dist2", "scale_min",
        "scale_mid", "scale_max") or its MSPLAT_VALUE_* number; param: three floats, the point of "distance2" or the colour of
        "colour_dist2" (no other kind takes one).  out: a float32 tensor of N values on this renderer's device to write into
        (None: a new one).  The cloud itself is read, whatever a mask or crop hides; no Sort is needed.  Asynchronous on the
        current context's stream; torch's current stream is made to wait for it.  Returns the tensor."""
        import torch
        if isinstance(kind, str):
            if kind not in _capi.VALUE_KINDS:
                raise ValueError("kind must be one of %s (got %r)" % (sorted(_capi.VALUE_KINDS), kind))
            code = _capi.VALUE_KINDS[kind]
        else:
            code = int(kind)
            if code not in _capi.VALUE_KINDS.values():
                raise ValueError("kind %r is not an MSPLAT_VALUE_* number" % (kind,))
        needs = code in tuple(_capi.VALUE_KINDS[k] for k in _capi.VALUE_KINDS_WITH_PARAM)
        if needs != (param is not None):
            raise ValueError("param goes with the kinds %s and with no other" % (_capi.VALUE_KINDS_WITH_PARAM,))
        p = None
        if needs:
            p = np.zeros(4, np.float32)
            p[0:3] = np.asarray(param, np.float64).reshape(3)
            if not np.isfinite(p).all():
                raise ValueError("param must be three finite floats (got %r)" % (param,))
        if not self._ctx:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "CloudValues: no cloud (Init first)")
        dev = torch.device("cuda", self._device)
        if out is None:
            out = torch.empty(self._n, dtype=torch.float32, device=dev)
        else:
            self._device_vector("out", out, torch.float32)
        torch.cuda.current_stream(dev).synchronize()
        _capi.check(self._ctx, self._lib.msplat_cloud_values(self._ctx, code, p.ctypes.data_as(C.POINTER(C.c_float)) if needs else None,
                                                             C.c_void_p(out.data_ptr()), self._n))
        self.wait_on_stream(torch.cuda.current_stream(dev).cuda_stream)
        return out

    def MarkValues(self, values, lo, hi, mask, value, outside=False):
        """mask[i] = value for every splat whose values[i] lies in the closed range lo <= v <= hi (outside=True: for every other
        one, NaN values included); other bytes stay (msplat_mark_values).  values: a float32 tensor of N values on this
        renderer's device, what CloudValues returns; mask: a torch uint8 / bool tensor of N bytes, what SetVisibility and the
        select= of the cloud edits take.  lo and hi may be infinite; lo > hi is an empty range.  Asynchronous on the current
        context's stream; torch's current stream is made to wait for it."""
        import torch
        lo, hi = float(lo), float(hi)
        if lo != lo or hi != hi:
            raise ValueError("lo and hi must not be NaN (got %r, %r)" % (lo, hi))
        self._device_vector("values", values, torch.float32)
        value = self._mark_target("MarkValues", mask, value)
        _capi.check(self._ctx, self._lib.msplat_mark_values(self._ctx, C.c_void_p(values.data_ptr()), self._n, lo, hi,
                                                            _capi.RANGE_OUTSIDE if outside else _capi.RANGE_INSIDE, C.c_void_p(mask.data_ptr()), value))
        self.wait_on_stream(torch.cuda.current_stream(torch.device("cuda", self._device)).cuda_stream)

    def HistogramValues(self, values, bins=0, lo=None, hi=None, select=None):
        """Histogram and summary of values[i] over the splats with select[i] (None: all; N values as TransformCloud takes them)
        (msplat_histogram_values): a dict of selected, finite, nan, below, above (ints), vmin, vmax (float32: the extremes of the
        finite values, +inf / -inf when there is none) and counts (numpy uint32[bins]).  bins=0 (lo, hi not given): the summary
        alone, the first call of a range slider.  1 <= bins <= 4096: finite lo < hi; bin b counts the values with
        b <= (v - lo) * bins / (hi - lo) < b + 1, v == hi in the last bin; below / above count the values outside [lo, hi],
        infinities included.  Synchronous."""
        import torch
        bins = int(bins)
        if not 0 <= bins <= _capi.VALUE_BINS_MAX:
            raise ValueError("bins must be 0 .. %d (got %d)" % (_capi.VALUE_BINS_MAX, bins))
        if bins == 0:
            if lo is not None or hi is not None:
                raise ValueError("lo and hi go with bins > 0")
            lo = hi = 0.0
        else:
            if lo is None or hi is None:
                raise ValueError("bins > 0 needs lo and hi")
            lo, hi = float(lo), float(hi)
            if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
                raise ValueError("lo and hi must be finite with lo < hi (got %r, %r)" % (lo, hi))
        self._device_vector("values", values, torch.float32)
        if not self._ctx:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "HistogramValues: no cloud (Init first)")
        sel = self._device_select(select, self._n)
        torch.cuda.current_stream(torch.device("cuda", self._device)).synchronize()
        counts = np.zeros(bins, np.uint32)
        s = _capi.ValueSummary(struct_size=C.sizeof(_capi.ValueSummary))
        _capi.check(self._ctx, self._lib.msplat_histogram_values(self._ctx, C.c_void_p(values.data_ptr()), sel, self._n, lo, hi, bins,
                                                                 counts.ctypes.data_as(C.POINTER(C.c_uint32)) if bins else None, C.byref(s)))
        return dict(selected=int(s.selected), finite=int(s.finite), nan=int(s.nan), below=int(s.below), above=int(s.above),
                    vmin=np.float32(s.vmin), vmax=np.float32(s.vmax), counts=counts)

    # -- selection by neighbourhood (msplat_neighbour_values) --
    def NeighbourValues(self, radius, kind="count", source=None, query=None, cap=0, max_tests=None, out=None, info=False):
        """What is around every splat, one float32 per splat in upload numbering (msplat_neighbour_values).  kind "count": the
        number of source splats within `radius` of the splat's centre, itself excluded, at most `cap` (0: no cap); "dist2": the
        squared distance to the nearest one within the radius, +inf if there is none.  source / query: N values as TransformCloud's
        select takes them (None: every splat) -- which splats count as neighbours, and which values are written; the words of
        unselected queries keep their bytes (a new tensor starts as zeros).  max_tests: the budget of candidate pairs (None: the
        library's default); a radius that is too large for the cloud raises MsplatError ERR_UNSUPPORTED and writes nothing.
        out: a float32 tensor of N values on this renderer's device to write into (None: a new one).  The cloud itself is read,
        whatever a mask or crop hides; no Sort is needed.  Synchronous.  Returns the tensor, or (tensor, dict of sources, queries,
        buckets, max_bucket, tests) with info=True."""
        import torch
        if isinstance(kind, str):
            if kind not in _capi.NEAR_KINDS:
                raise ValueError("kind must be one of %s (got %r)" % (sorted(_capi.NEAR_KINDS), kind))
            code = _capi.NEAR_KINDS[kind]
        else:
            code = int(kind)
            if code not in _capi.NEAR_KINDS.values():
                raise ValueError("kind %r is not an MSPLAT_NEAR_* number" % (kind,))
        radius, cap = float(radius), int(cap)
        if not (np.isfinite(radius) and radius > 0.0):
            raise ValueError("radius must be finite and > 0 (got %r)" % radius)
        if not 0 <= cap < 2 ** 32:
            raise ValueError("cap is an unsigned 32-bit value (got %d)" % cap)
        if cap and code == _capi.NEAR_KINDS["dist2"]:
            raise ValueError("cap goes with kind \"count\" (a cap stops a count)")
        max_tests = 0 if max_tests is None else int(max_tests)
        if not 0 <= max_tests < 2 ** 64:
            raise ValueError("max_tests is an unsigned 64-bit value (got %d)" % max_tests)
        if not self._ctx:
            raise _capi.MsplatError(_capi.ERR_NO_CLOUD, "NeighbourValues: no cloud (Init first)")
        dev = torch.device("cuda", self._device)
        src = self._device_select(source, self._n)
        src_alive = self._select_arg
        qry = src if query is source else self._device_select(query, self._n)
        self._select_arg = (src_alive, self._select_arg)
        if out is None:
            out = torch.zeros(self._n, dtype=torch.float32, device=dev)
        else:
            self._device_vector("out", out, torch.float32)
        torch.cuda.current_stream(dev).synchronize()
        ni = _capi.NeighbourInfo(struct_size=C.sizeof(_capi.NeighbourInfo))
        _capi.check(self._ctx, self._lib.msplat_neighbour_values(self._ctx, code, radius, src, qry, self._n, cap, max_tests,
                                                                 C.c_void_p(out.data_ptr()), C.byref(ni)))
        if not info:
            return out
        return out, {k: int(getattr(ni, k)) for k in ("sources", "queries", "buckets", "max_bucket", "tests")}

    def GrowSelection(self, mask, radius, steps=1, max_tests=None):
        """The selection grown by `radius`, `steps` times: a copy of `mask` (a torch uint8 / bool tensor of N bytes on this
        renderer's device) in which, per step, every splat with a selected splat within the radius gets byte 1; other bytes stay.
        NeighbourValues(cap=1, source=the mask so far) plus MarkValues per step; compose with MeasureCloud's count for a flood
        fill.  Returns the new mask."""
        import torch
        steps = int(steps)
        if steps < 0:
            raise ValueError("steps must be >= 0 (got %d)" % steps)
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError("mask must be a torch uint8 / bool tensor")
        self._device_vector("mask", mask, mask.dtype)
        grown = mask.clone()
        near = None
        for _ in range(steps):
            near = self.NeighbourValues(radius, "count", source=grown, cap=1, max_tests=max_tests, out=near)
            self.MarkValues(near, 1.0, 1.0, grown, 1)
        return grown

    def synchronize(self):
        """blocks until every frame in flight has been issued (async_submit) AND has finished on the GPU"""
        for h in self._ctxs:
            _capi.check(h, self._lib.msplat_synchronize(h))

    def wait_on_stream(self, stream):
        """device-side join: `stream` (hipStream_t handle, e.g. torch.cuda.Stream.cuda_stream; None or 0 = the
        default stream) waits for the frame issued last"""
        _capi.check(self._ctx, self._lib.msplat_stream_wait(self._ctx, C.c_void_p(stream or 0)))

    def band_exchange(self, comm, rank, world, root, kind, block_rows, fb_ptr, pitch_bytes, width, height, loopback_src=None,
                      wire_fp16=False):
        """msplat_band_exchange on the current context's stream (comm = ncclComm_t handle, e.g. dist.RcclComm().handle): rank
        `root` receives every other rank's runs of bin rows straight into its framebuffer, the owners send theirs.
        loopback_src: one-rank test form (msplat_debug_band_exchange_loopback): this rank's runs travel from loopback_src to fb_ptr;
        wire_fp16 (RGBA32F targets): the rows cross the link as RGBA16F (MSPLAT_EXCHANGE_WIRE_FP16)"""
        flags = _capi.EXCHANGE_WIRE_FP16 if wire_fp16 else 0
        if loopback_src is not None:
            rc = self._lib.msplat_debug_band_exchange_loopback(self._ctx, comm, kind, block_rows, world, rank, C.c_void_p(loopback_src),
                                                               C.c_void_p(fb_ptr), pitch_bytes, width, height, flags)
        else:
            rc = self._lib.msplat_band_exchange(self._ctx, comm, rank, world, root, kind, block_rows, C.c_void_p(fb_ptr), pitch_bytes,
                                                width, height, flags)
        if rc != _capi.OK:
            raise _capi.MsplatError(rc, self._lib.msplat_group_last_error(None).decode())

    def next_frame_wait_event(self, event):
        """the context the NEXT Sort will use waits for `event` (hipEvent_t handle, e.g. torch.cuda.Event
        .cuda_event recorded after the consumer of the framebuffer that frame is going to overwrite)"""
        h = self._ctxs[(self._cur + 1) % len(self._ctxs)]
        _capi.check(h, self._lib.msplat_wait_event(h, C.c_void_p(event)))

    @property
    def frames_in_flight(self):
        return self._depth

    @property
    def frame_slot(self):
        """index of the context the latest Sort ran on (0 .. frames_in_flight-1)"""
        return self._cur

    def sort_count(self):
        v = C.c_uint32()
        _capi.check(self._ctx, self._lib.msplat_sort_count(self._ctx, C.byref(v)))
        return v.value

    def sorted_indices(self):
        out = np.empty(max(self._n, 1), np.uint32)
        _capi.check(self._ctx, self._lib.msplat_get_sorted_indices(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                   out.shape[0]))
        return out[:self.sort_count()].copy()

    def storage_order(self):
        """None when the cloud is stored in upload order, else the permutation slot -> upload index of the library's spatial
        storage order (msplat_config.spatial_order): equal depth keys are drawn in ascending storage slot"""
        ro = C.c_int(0)
        _capi.check(self._ctx, self._lib.msplat_get_storage_order(self._ctx, None, 0, C.byref(ro)))
        if not ro.value:
            return None
        out = np.empty(max(self._n, 1), np.uint32)
        _capi.check(self._ctx, self._lib.msplat_get_storage_order(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                  out.shape[0], None))
        return out[:self._n]

    def cull_boxes(self):
        """(live, total, listed): bounding boxes that can hold a visible splat for the latest Sort's camera / boxes in the cloud
        ((0, 0) for a cloud in upload order); listed: that Sort's first pass walked only the listed live boxes"""
        a, b, l = C.c_uint32(), C.c_uint32(), C.c_int()
        _capi.check(self._ctx, self._lib.msplat_debug_get_cull_boxes(self._ctx, C.byref(a), C.byref(b), C.byref(l)))
        return a.value, b.value, bool(l.value)

    def debug_positions(self):
        """the store's position plane as the kernels read it (msplat_debug_get_positions): (N, 4) float32 of x, y, z and the
        footprint bound, in UPLOAD numbering (the storage order undone); synchronises"""
        out = np.zeros((max(self._n, 1), 4), np.float32)
        _capi.check(self._ctx, self._lib.msplat_debug_get_positions(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        out = out[:self._n]
        order = self.storage_order()
        if order is not None:
            up = np.empty_like(out)
            up[order] = out
            out = up
        return out

    def sorted_keys(self):
        out = np.empty(max(self._n, 1), np.uint32)
        _capi.check(self._ctx, self._lib.msplat_get_sorted_keys(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                out.shape[0]))
        return out[:self.sort_count()].copy()

    def stats(self):
        s = _capi.Stats()
        _capi.check(self._ctx, self._lib.msplat_get_stats(self._ctx, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _capi.Stats._fields_}

    def timings(self):
        """stage times averaged over the sampled frames of every context (frames in flight)"""
        keys = ("sort_total", "render_total", "project", "binning", "composite")
        acc = {k: 0.0 for k in keys + ("composite_kernel",)}
        frames = 0.0
        for h in self._ctxs:
            t = _capi.Timings()
            _capi.check(h, self._lib.msplat_get_timings(h, C.byref(t)))
            nf = t.reserved[0]
            frames += nf
            for k in keys:
                acc[k] += getattr(t, k) * nf
            acc["composite_kernel"] += t.reserved[1] * nf    # exact dispatch begin/end of composite_kernel
        d = {k: (v / frames if frames > 0 else 0.0) for k, v in acc.items()}
        d["frames_averaged"] = frames
        return d

    def debug_projected(self):
        v = self.sort_count()
        rec = np.zeros((max(v, 1), 12), np.float32)
        rect = np.zeros(max(v, 1), np.uint32)
        _capi.check(self._ctx, self._lib.msplat_debug_get_projected(
            self._ctx, rec.ctypes.data_as(C.POINTER(C.c_float)), rect.ctypes.data_as(C.POINTER(C.c_uint32)), rec.shape[0]))
        return rec[:v], rect[:v]

    def debug_projected_view(self, view=0, extra=0):
        """debug_projected() for one view of the latest Render (1: the second eye of RenderStereo) and `extra` ranks beyond the
        visible ones: what the buffers held before (msplat_debug_get_projected_view)"""
        n = self.sort_count() + int(extra)
        rec = np.zeros((max(n, 1), 12), np.float32)
        rect = np.zeros(max(n, 1), np.uint32)
        _capi.check(self._ctx, self._lib.msplat_debug_get_projected_view(
            self._ctx, int(view), rec.ctypes.data_as(C.POINTER(C.c_float)), rect.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return rec[:n], rect[:n]

    def debug_fill_projected(self, byte):
        """fills the projection's record and rectangle buffers (msplat_debug_fill_projected)"""
        _capi.check(self._ctx, self._lib.msplat_debug_fill_projected(self._ctx, int(byte)))

    def set_tile_probe(self, enable=True):
        """per-work-item compositor counters for the following renders (off by default: a few clock reads per batch)"""
        for h in self._ctxs:
            _capi.check(h, self._lib.msplat_set_tile_probe(h, 1 if enable else 0))

    def composite_work(self):
        """what the compositor fetched and evaluated in the last render (needs set_tile_probe)"""
        w = _capi.CompositeWork()
        _capi.check(self._ctx, self._lib.msplat_get_composite_work(self._ctx, C.byref(w)))
        return {k: int(getattr(w, k)) for k, _ in _capi.CompositeWork._fields_}

    def compositor_launch(self):
        """(work items, grid, ordered, kind) of the current context's latest compositor launch (msplat_debug_get_compositor_launch):
        grid < items = persistent waves on the work queue, grid == items = every item on its own wave; kind 0 splats, 1 the
        draw-order depth / target-rounding compositor, 2 points; a two-pass Render reports its first pass"""
        out = (C.c_uint32 * 4)()
        _capi.check(self._ctx, self._lib.msplat_debug_get_compositor_launch(self._ctx, out))
        return tuple(int(v) for v in out)

    def heavy_chunks(self):
        """(chunks over the heavy threshold, helper slots) of the current context's latest column pass (msplat_debug_get_heavy_chunks):
        min of the two were split over 8 workgroups; the second chain's numbers after a two-pass Render"""
        out = (C.c_uint32 * 2)()
        _capi.check(self._ctx, self._lib.msplat_debug_get_heavy_chunks(self._ctx, out))
        return int(out[0]), int(out[1])

    def bin_order(self):
        """the order[slot] -> bin table the current context's latest compositor launch walked, read back from the device
        (msplat_debug_get_bin_order): one word per bin"""
        out = np.zeros(max(self.compositor_launch()[0] // 4, 1), np.uint32)
        _capi.check(self._ctx, self._lib.msplat_debug_get_bin_order(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.shape[0]))
        return out

    def two_pass_state(self, share=0.0):
        """(two-pass Renders so far, share of the visible splats the next one puts into its first pass) summed / taken over the
        contexts; share > 0 pins the share (msplat_debug_two_pass), 0 leaves it to the feedback loop"""
        frames, now = 0, 0.0
        for h in self._ctxs:
            a, b = C.c_uint64(), C.c_float()
            _capi.check(h, self._lib.msplat_debug_two_pass(h, float(share), C.byref(a), C.byref(b)))
            frames += a.value
            now = b.value
        return frames, now

    def two_pass_info(self):
        """what the latest two-pass Render of the current context did (msplat_get_two_pass_info), None if its latest Render ran in
        one pass"""
        out = (C.c_uint64 * 8)()
        _capi.check(self._ctx, self._lib.msplat_get_two_pass_info(self._ctx, out))
        if out[0] == 0:
            return None
        keys = ("frames", "splats_pass1", "splats_pass2", "pairs_pass1", "pairs_pass2", "bins_unfinished", "bins", "visible")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def verify_order(self):
        """on-device self-check: (violations of the sorted-key / tie order, violations of the bin-list order); (0, 0) = healthy"""
        a, b = C.c_uint32(), C.c_uint32()
        _capi.check(self._ctx, self._lib.msplat_debug_verify_order(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def cu_partitions(self):
        """per context: (MSPLAT_CU_* its stream got, the stream's CU mask as the runtime reports it: 8 words)"""
        out = []
        for h in self._ctxs:
            m = (C.c_uint32 * 8)()
            rc = self._lib.msplat_debug_cu_partition(h, m)
            _capi.check(h, rc if rc < 0 else 0)
            out.append((rc, list(m)))
        return out

    def debug_tile_probe(self):
        st = self.stats()
        nt = st["tiles_x"] * st["tiles_y"] * 8        # one slot per work item: (bin, quadrant[, half])
        out = np.zeros((max(nt, 1), 8), np.uint32)
        _capi.check(self._ctx, self._lib.msplat_debug_get_tile_probe8(
            self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.shape[0]))
        return out[out[:, 7] > 0]

    def debug_tile_probe_table(self):
        """the probe's eight words per work item of the current context's latest probed render, row = work item (debug_tile_probe
        drops the rows of the items that did not run, and with them the index); rows of items outside the image are zero"""
        items = self.compositor_launch()[0]
        out = np.zeros((max(items, 1), 8), np.uint32)
        _capi.check(self._ctx, self._lib.msplat_debug_get_tile_probe8(
            self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.shape[0]))
        return out[:items]

    def debug_tile_lists(self, want_pairs=True):
        st = self.stats()
        nt = st["tiles_x"] * st["tiles_y"]
        ts = np.zeros(nt + 1, np.uint32)
        if not want_pairs:          # only the list offsets
            _capi.check(self._ctx, self._lib.msplat_debug_get_tile_lists(
                self._ctx, ts.ctypes.data_as(C.POINTER(C.c_uint32)), ts.shape[0], None, 0))
            return ts, None
        pairs = np.zeros(max(int(st["pairs"]), 1), np.uint32)
        _capi.check(self._ctx, self._lib.msplat_debug_get_tile_lists(
            self._ctx, ts.ctypes.data_as(C.POINTER(C.c_uint32)), ts.shape[0],
            pairs.ctypes.data_as(C.POINTER(C.c_uint32)), pairs.shape[0]))
        return ts, pairs[:int(st["pairs"])]


class SplatRendererGroup:
    """Several GPUs, one process: the Python mirror of msplat_group_* (include/msplat.h).  Same Init / Sort / Render
    surface as SplatRenderer; the screen's bin rows are partitioned over `devices`, every device renders its rows, and
    with a device framebuffer (memory of devices[0]) the other devices' compositors write into it directly over xGMI."""

    def __init__(self, devices, fb_format="fp32", t_epsilon=-1.0, layout="contiguous", block_rows=1, band_cull=False,
                 enable_timing=False, cloud_storage="fp32"):
        self._storage = _storage_kind(cloud_storage)
        self._lib = _capi.lib()
        self._g = None
        self._args = _FrameArgs()
        self._devices = [int(d) for d in devices]
        self._fb_format = _capi.fb_format(fb_format)
        self._t_eps = t_epsilon
        self._layout, self._block_rows, self._band_cull = layout, int(block_rows), bool(band_cull)
        self._timing = enable_timing
        self._err = ""
        self._gerr = self._lib.msplat_group_last_error      # the error getter of _capi.check for a group handle

    def __del__(self):
        self.close()

    def close(self):
        g, self._g = getattr(self, "_g", None), None
        if g:
            self._lib.msplat_group_destroy(g)

    def last_error(self):
        return self._lib.msplat_group_last_error(self._g).decode() if self._g else self._err

    def Init(self, gaussianCloud, isFramebufferSRGBEnabled=False, useRgcSortOverride=False):
        del useRgcSortOverride
        self.close()
        cfg = _capi.Config()
        cfg.struct_size = C.sizeof(_capi.Config)
        cfg.fb_format = self._fb_format
        cfg.srgb = 1 if isFramebufferSRGBEnabled else 0
        cfg.t_epsilon = self._t_eps
        cfg.enable_timing = int(self._timing)
        devs = (C.c_int32 * len(self._devices))(*self._devices)
        g = C.c_void_p()
        rc = self._lib.msplat_group_create(C.byref(g), devs, len(self._devices), C.byref(cfg))
        if rc != _capi.OK:
            self._err = self._lib.msplat_group_last_error(None).decode()
            return False
        self._g = g
        _capi.check(self._g, self._lib.msplat_group_set_layout(g, _capi.BAND_KINDS[self._layout], self._block_rows), self._gerr)
        _capi.check(self._g, self._lib.msplat_group_set_band_cull(g, 1 if self._band_cull else 0), self._gerr)
        _capi.check(self._g, self._lib.msplat_group_set_cloud_storage(g, self._storage), self._gerr)
        if isinstance(gaussianCloud, GaussianCloud):
            rc = self._lib.msplat_group_upload_gaussian_cloud(g, gaussianCloud.handle)
        else:
            aos, args = _aos_upload(gaussianCloud)       # (aos: the memory args points into, kept until the call returns)
            rc = self._lib.msplat_group_upload_cloud(g, *args)
        if rc != _capi.OK:
            self._err = self._lib.msplat_group_last_error(g).decode()
            return False
        return True

    @property
    def size(self):
        return int(self._lib.msplat_group_size(self._g))

    def peer_store(self, i):
        return bool(self._lib.msplat_group_peer_store(self._g, i))

    def context(self, i):
        """borrowed msplat_ctx handle of rank i (for the C-ABI getters)"""
        return C.c_void_p(self._lib.msplat_group_context(self._g, i))

    def sort_count(self, i):
        v = C.c_uint32()
        h = self.context(i)
        _capi.check(h, self._lib.msplat_sort_count(h, C.byref(v)))
        return v.value

    def Sort(self, cameraMat, projMat, viewport, nearFar):
        c, p, v, nf = self._args.load(cameraMat, projMat, viewport, nearFar)
        _capi.check(self._g, self._lib.msplat_group_sort(self._g, c, p, v, nf), self._gerr)

    def Render(self, cameraMat, projMat, viewport, nearFar, out=None, out_ptr=None, pitch_bytes=0, depth=None, depth_ptr=None,
               depth_pitch_bytes=0, occluder=None, occluder_ptr=None, occluder_pitch_bytes=0):
        """out_ptr: device pointer ON devices[0] (asynchronous; synchronize() or wait on context 0's stream);
        otherwise a host array is filled / returned.  A depth plane (SplatRenderer.Render's depth= / depth_ptr=) is refused:
        the group's row gather moves the colour only; so is an occluder plane (occluder= / occluder_ptr=): it lives on one device"""
        if occluder is not None or occluder_ptr is not None:
            raise _capi.MsplatError(_capi.ERR_UNSUPPORTED, "a device group takes no occluder plane (msplat_render_occluded is per context): "
                                    "render behind geometry with a SplatRenderer")
        del occluder_pitch_bytes
        if (depth is not None and depth is not False) or depth_ptr is not None:
            raise _capi.MsplatError(_capi.ERR_UNSUPPORTED, "a device group has no depth output (msplat_render_depth is per context): "
                                    "render the depth plane with a SplatRenderer")
        del depth_pitch_bytes
        c, p, v, nf = self._args.load(cameraMat, projMat, viewport, nearFar)
        if out_ptr is not None:
            _capi.check(self._g, self._lib.msplat_group_render(self._g, c, p, v, nf, C.c_void_p(out_ptr), pitch_bytes, 1), self._gerr)
            return None
        out = _host_frame(self._fb_format, self._args.vp, out)
        _capi.check(self._g, self._lib.msplat_group_render(self._g, c, p, v, nf, out.ctypes.data, 0, 0), self._gerr)
        return out

    def RenderLayers(self, *args, **kw):
        """refused (MsplatError(ERR_UNSUPPORTED), before a device is touched): the planes of msplat_render_layers live on one device,
        and the group's row gather moves the colour only"""
        raise _capi.MsplatError(_capi.ERR_UNSUPPORTED, "a device group has no layers frame (msplat_render_layers / "
                                "msplat_render_stereo_layers are per context): render depth and occluder planes with a SplatRenderer")

    RenderStereoLayers = RenderLayers

    def set_target_mode(self, mode):
        """msplat_group_set_target_mode: "clear" or "premultiplied"; "load" is refused (MSPLAT_ERR_UNSUPPORTED: a rank that stages
        its rows has no destination rows to blend over)"""
        _capi.check(self._g, self._lib.msplat_group_set_target_mode(self._g, _target_mode(mode)), self._gerr)

    def synchronize(self):
        _capi.check(self._g, self._lib.msplat_group_synchronize(self._g), self._gerr)

    EXCHANGES = ("peer_store", "rccl", "copy")      # MSPLAT_EXCHANGE_*

    def set_exchange(self, name):
        """how the other devices' rows reach devices[0]'s framebuffer: "peer_store" (default), "rccl" (ncclSend / ncclRecv over
        communicators from ncclCommInitAll) or "copy" (hipMemcpy2DAsync per run)"""
        _capi.check(self._g, self._lib.msplat_group_set_exchange(self._g, self.EXCHANGES.index(name)), self._gerr)

    def exchange(self):
        """the exchange the latest device-output Render used"""
        return self.EXCHANGES[self._lib.msplat_group_get_exchange(self._g)]
