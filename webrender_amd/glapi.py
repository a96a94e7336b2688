"""ctypes binding of the GL-shaped C ABI shared by libwrhip (the product) and the
reference's swgl (the oracle, tests only).

The symbol set and signatures are the `extern "C"` block of the reference's
Rust shim, swgl/src/swgl_fns.rs:23-322 (99 functions); `include/wrhip.h`
declares the same set for libwrhip.  Method names here are the C names, so a
call sequence written against this class reads like the reference's
`impl Gl for Context` forwarding code (swgl_fns.rs:500-2489).

Every call can optionally be recorded into a `Trace` (see trace.py) so the same
call stream can be replayed against another backend or by the native replayer.
"""
import ctypes as C
import os

c_void_p, c_char_p = C.c_void_p, C.c_char_p
i32, u32, u8, f32, f64 = C.c_int32, C.c_uint32, C.c_uint8, C.c_float, C.c_double
u64, isz, usz = C.c_uint64, C.c_ssize_t, C.c_size_t
P = c_void_p

# name -> (restype, argtypes).  Order follows swgl_fns.rs:23-322.
SIGNATURES = {
    "ActiveTexture": (None, [u32]),
    "BindTexture": (None, [u32, u32]),
    "BindBuffer": (None, [u32, u32]),
    "BindVertexArray": (None, [u32]),
    "BindFramebuffer": (None, [u32, u32]),
    "BindRenderbuffer": (None, [u32, u32]),
    "BlendFunc": (None, [u32, u32, u32, u32]),
    "BlendColor": (None, [f32, f32, f32, f32]),
    "BlendEquation": (None, [u32]),
    "Enable": (None, [u32]),
    "Disable": (None, [u32]),
    "GenQueries": (None, [i32, P]),
    "BeginQuery": (None, [u32, u32]),
    "EndQuery": (None, [u32]),
    "GetQueryObjectui64v": (None, [u32, u32, P]),
    "GenBuffers": (None, [i32, P]),
    "GenTextures": (None, [i32, P]),
    "GenFramebuffers": (None, [i32, P]),
    "GenRenderbuffers": (None, [i32, P]),
    "BufferData": (None, [u32, usz, P, u32]),
    "BufferSubData": (None, [u32, isz, usz, P]),
    "MapBuffer": (P, [u32, u32]),
    "MapBufferRange": (P, [u32, isz, usz, u32]),
    "UnmapBuffer": (u8, [u32]),
    "TexStorage2D": (None, [u32, i32, u32, i32, i32]),
    "FramebufferTexture2D": (None, [u32, u32, u32, u32, i32]),
    "CheckFramebufferStatus": (u32, [u32]),
    "InvalidateFramebuffer": (None, [u32, i32, P]),
    "TexImage2D": (None, [u32, i32, i32, i32, i32, i32, u32, u32, P]),
    "TexSubImage2D": (None, [u32, i32, i32, i32, i32, i32, u32, u32, P]),
    "GenerateMipmap": (None, [u32]),
    "GetUniformLocation": (i32, [u32, c_char_p]),
    "BindAttribLocation": (None, [u32, u32, c_char_p]),
    "GetAttribLocation": (i32, [u32, c_char_p]),
    "GenVertexArrays": (None, [i32, P]),
    "VertexAttribPointer": (None, [u32, i32, u32, u8, i32, P]),
    "VertexAttribIPointer": (None, [u32, i32, u32, i32, P]),
    "CreateShader": (u32, [u32]),
    "AttachShader": (None, [u32, u32]),
    "CreateProgram": (u32, []),
    "Uniform1i": (None, [i32, i32]),
    "Uniform4fv": (None, [i32, i32, P]),
    "UniformMatrix4fv": (None, [i32, i32, u8, P]),
    "DrawElementsInstanced": (None, [u32, i32, u32, isz, i32]),
    "EnableVertexAttribArray": (None, [u32]),
    "VertexAttribDivisor": (None, [u32, u32]),
    "LinkProgram": (None, [u32]),
    "GetLinkStatus": (i32, [u32]),
    "UseProgram": (None, [u32]),
    "SetViewport": (None, [i32, i32, i32, i32]),
    "FramebufferRenderbuffer": (None, [u32, u32, u32, u32]),
    "RenderbufferStorage": (None, [u32, u32, i32, i32]),
    "DepthMask": (None, [u8]),
    "DepthFunc": (None, [u32]),
    "SetScissor": (None, [i32, i32, i32, i32]),
    "ClearColor": (None, [f32, f32, f32, f32]),
    "ClearDepth": (None, [f64]),
    "Clear": (None, [u32]),
    "ClearTexSubImage": (None, [u32, i32, i32, i32, i32, i32, i32, i32, u32, u32, P]),
    "ClearTexImage": (None, [u32, i32, u32, u32, P]),
    "ClearColorRect": (None, [u32, i32, i32, i32, i32, f32, f32, f32, f32]),
    "PixelStorei": (None, [u32, i32]),
    "ReadPixels": (None, [i32, i32, i32, i32, u32, u32, P]),
    "Finish": (None, []),
    "ShaderSourceByName": (None, [u32, c_char_p]),
    "TexParameteri": (None, [u32, u32, i32]),
    "CopyImageSubData": (None, [u32, u32, i32, i32, i32, i32, u32, u32, i32, i32, i32, i32, i32, i32, i32]),
    "CopyTexSubImage2D": (None, [u32, i32, i32, i32, i32, i32, i32, i32]),
    "BlitFramebuffer": (None, [i32, i32, i32, i32, i32, i32, i32, i32, u32, u32]),
    "GetIntegerv": (None, [u32, P]),
    "GetBooleanv": (None, [u32, P]),
    "GetString": (c_char_p, [u32]),
    "GetStringi": (c_char_p, [u32, u32]),
    "GetError": (u32, []),
    "InitDefaultFramebuffer": (None, [i32, i32, i32, i32, i32, P]),
    "GetColorBuffer": (P, [u32, u8, P, P, P]),
    "ResolveFramebuffer": (None, [u32]),
    "SetTextureBuffer": (None, [u32, u32, i32, i32, i32, P, i32, i32]),
    "SetTextureParameter": (None, [u32, u32, i32]),
    "DeleteTexture": (None, [u32]),
    "DeleteRenderbuffer": (None, [u32]),
    "DeleteFramebuffer": (None, [u32]),
    "DeleteBuffer": (None, [u32]),
    "DeleteVertexArray": (None, [u32]),
    "DeleteQuery": (None, [u32]),
    "DeleteShader": (None, [u32]),
    "DeleteProgram": (None, [u32]),
    "LockFramebuffer": (P, [u32]),
    "LockTexture": (P, [u32]),
    "LockResource": (None, [P]),
    "UnlockResource": (None, [P]),
    "GetResourceBuffer": (P, [P, P, P, P]),
    "Composite": (None, [P, P, i32, i32, i32, i32, i32, i32, i32, i32, u8, u8, u8, u32, i32, i32, i32, i32]),
    "CompositeYUV": (None, [P, P, P, P, i32, u32, i32, i32, i32, i32, i32, i32, i32, i32, u8, u8, i32, i32, i32, i32]),
    "CreateContext": (P, []),
    "ReferenceContext": (None, [P]),
    "DestroyContext": (None, [P]),
    "MakeCurrent": (None, [P]),
    "ReportMemory": (usz, [P, P]),
}
assert len(SIGNATURES) == 99

# libwrhip-only introspection hooks (include/wrhip.h, "libwrhip additions").
EXTRA_SIGNATURES = {
    "WrhipGetStats": (None, [P]),
    "WrhipResetStats": (None, []),
    "WrhipSetProfiling": (None, [i32]),
    "WrhipGetKernelStats": (i32, [P, i32]),
    "WrhipSetShard": (None, [i32, i32]),
    "WrhipSetTargetRows": (None, [u32, i32, i32]),
    "WrhipGetTextureDevicePtr": (P, [u32, P, P, P]),
    "WrhipGetFramebufferTexture": (u32, [u32]),
    "WrhipGetTextureSize": (i32, [u32, P, P]),
    "WrhipDeviceName": (c_char_p, []),
    "WrhipFlush": (None, []),
    "WrhipFlushHeld": (i32, []),
    "WrhipGetStream": (P, []),
    "WrhipTapTexture": (i32, [u32, i32, i32, i32, i32, u32]),
    "WrhipTapResultGet": (i32, [i32, P, i32]),
    "WrhipGrabTexture": (i32, [u32, P, i32, u32]),
    "WrhipGrabTextureScaled": (i32, [u32, P, i32, i32, u32]),
    "WrhipGrabResultGet": (i32, [i32, P, P, C.c_int64, i32]),
    "WrhipGrabPayloadGet": (i32, [i32, P, u64, P, i32]),
    "WrhipGrabDecode": (i32, [P, u64, u32, u32, i32, i32, P, C.c_int64, P, P]),
    "WrhipGrabTextureTensor": (i32, [u32, P, P]),
    "WrhipDeviceAlloc": (P, [u64]),
    "WrhipDeviceFree": (None, [P]),
    "WrhipDeviceRead": (i32, [P, P, u64]),
    "WrhipDeviceWrite": (i32, [P, P, u64]),
    "WrhipPutTextureTensor": (i32, [u32, P, P]),
    "WrhipPutTexturePayload": (i32, [u32, P, P, u64, u32]),
    "WrhipGrabTextureYuv": (i32, [u32, P, P]),
    "WrhipGrabTextureYuvDelta": (i32, [u32, P, P, u32]),
    "WrhipGrabDecodeYuv": (i32, [P, u64, u32, i32, i32, P, C.c_int64, P, P, C.c_int64, P, P]),
    "WrhipGrabTextureYuvScaled": (i32, [u32, P, i32, i32, P, i32]),
}


class WrhipStats(C.Structure):
    _fields_ = [(n, u64) for n in (
        "flushes", "kernel_launches", "raster_launches", "raster_ns",
        "raster_algo_bytes", "raster_pixels", "prims", "h2d_bytes", "d2h_bytes",
        "host_record_ns", "host_upload_ns", "host_flush_ns", "host_wait_ns", "row_launches",
        "setup_carried", "carrier_lost", "scratch_grown_held", "forwarded_targets", "cell_bins")]


class WrhipKernelStat(C.Structure):
    _fields_ = [(n, i32) for n in ("kind", "fmt", "depth", "feat")] + [(n, u64) for n in ("launches", "ns", "algo_bytes", "workgroups")]


class WrhipTapResult(C.Structure):
    _fields_ = [("status", i32), ("width", u32), ("height", u32), ("format", u32), ("digest", u64 * 2),
                ("max_diff", u32), ("differing", u32), ("hist", u32 * 256)]


# WrhipGrabTexture flags, and the bytes that cross ahead of every grab's payload (include/wrhip.h)
GRAB_FLIP_ROWS, GRAB_SWAP_RB, GRAB_DELTA, GRAB_KEY, GRAB_PACKED = 1, 2, 4, 8, 32
GRAB_SCALED = 64          # reported in a scaled grab's info["flags"] (WrhipGrabTextureScaled); no flag of WrhipGrabTexture
GRAB_TENSOR = 128         # reported in a tensor grab's info["flags"] (WrhipGrabTextureTensor); no flag of the other grab calls
GRAB_YUV = 512            # reported in a YUV grab's info["flags"] (WrhipGrabTextureYuv); no flag of the other grab calls
GRAB_SCROLL = 1024        # with GRAB_DELTA | GRAB_PACKED: the scroll grab (scrolled blocks cross as 16-byte COPY entries)
GRAB_SCROLL_MAX = 512     # the largest |scroll_dy| that is looked for
GRAB_SCROLL_LAUNCHES = 4  # launches of a scroll grab that is no keyframe
GRAB_YUV_SCROLL_LAUNCHES = 3  # launches of a delta YUV grab with GRAB_SCROLL that is no keyframe
GRAB_MAX_RECTS, GRAB_HEADER, GRAB_BLOCK = 16, 16, 64
# WrhipGrabTextureYuv: plane layouts, and the YuvRangedColorSpace values it converts to
YUV_I420, YUV_NV12, YUV_I444 = 0, 1, 2
YUV_REC601_NARROW, YUV_REC601_FULL, YUV_REC709_NARROW, YUV_REC709_FULL, YUV_REC2020_NARROW, YUV_REC2020_FULL = range(6)
# WrhipGrabTextureTensor: element types, layouts, and the flag that keeps the stored channel order
TENSOR_U8, TENSOR_F16, TENSOR_BF16, TENSOR_F32 = 0, 1, 2, 3
TENSOR_CHW, TENSOR_HWC = 0, 1
TENSOR_BGR = 256
TENSOR_ELEM_BYTES = {TENSOR_U8: 1, TENSOR_F16: 2, TENSOR_BF16: 2, TENSOR_F32: 4}


class WrhipGrabInfo(C.Structure):
    _fields_ = [("status", i32), ("format", u32), ("flags", u32), ("nrects", i32), ("rects", (i32 * 4) * GRAB_MAX_RECTS),
                ("keyframe", u32), ("blocks", u32), ("blocks_total", u32), ("damage", i32 * 4), ("bytes", u64),
                ("scaled_w", i32), ("scaled_h", i32), ("levels", u32), ("renditions", u32),
                ("scroll_dy", i32), ("copied", u32)]


class WrhipTensorDesc(C.Structure):
    _fields_ = [("dst", P), ("dst_bytes", u64), ("out_w", i32), ("out_h", i32), ("dtype", u32), ("layout", u32), ("channels", u32),
                ("row_stride", C.c_int64), ("plane_stride", C.c_int64), ("scale", C.c_float * 4), ("bias", C.c_float * 4), ("flags", u32)]


class WrhipTensorSrc(C.Structure):
    _fields_ = [("src", P), ("src_bytes", u64), ("dtype", u32), ("layout", u32), ("channels", u32),
                ("row_stride", C.c_int64), ("plane_stride", C.c_int64), ("scale", C.c_float * 4), ("bias", C.c_float * 4),
                ("alpha", u32), ("flags", u32)]


class WrhipYuvDesc(C.Structure):
    _fields_ = [("format", u32), ("color_space", u32), ("flags", u32), ("dst", P), ("dst_bytes", u64),
                ("y_stride", C.c_int64), ("c_stride", C.c_int64)]


def yuv_plane_shapes(w, h, format):
    """The planes of a w x h YUV grab as (rows, bytes per tight row): Y, then Cb and Cr, or NV12's one plane of (Cb, Cr) pairs"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if format == YUV_I444:
        return [(h, w), (h, w), (h, w)]
    if format == YUV_NV12:
        return [(h, w), (ch, 2 * cw)]
    return [(h, w), (ch, cw), (ch, cw)]


def yuv_split(flat, w, h, format):
    """The flat uint8 array a YUV ticket delivers (grab_result) as its planes: [Y (h, w), Cb, Cr] of (ch, cw) or (h, w) samples, or
    [Y, CbCr (ch, cw, 2)] for NV12 -- views, not copies"""
    out, at = [], 0
    for rows, row in yuv_plane_shapes(w, h, format):
        out.append(flat[at:at + rows * row].reshape(rows, row))
        at += rows * row
    assert at == len(flat), (at, len(flat))
    if format == YUV_NV12:
        out[1] = out[1].reshape(out[1].shape[0], -1, 2)
    return out


def yuv_split_renditions(flat, size, renditions, format):
    """The flat uint8 array a scaled YUV ticket delivers (grab_texture_yuv_scaled to the host) as its renditions: a list of
    yuv_split's lists, rendition k -- level k of the chain, (size[0] << k) x (size[1] << k) -- at index k; views, not copies"""
    out, at = [], 0
    for k in range(renditions):
        w, h = size[0] << k, size[1] << k
        n = sum(rows * row for rows, row in yuv_plane_shapes(w, h, format))
        out.append(yuv_split(flat[at:at + n], w, h, format))
        at += n
    assert at == len(flat), (at, len(flat))
    return out


def _as_ptr(x):
    """bytes / bytearray / numpy array / ctypes object / int / None -> void*."""
    if x is None:
        return None, None
    if isinstance(x, int):
        return x, None
    if isinstance(x, (bytes, bytearray)):
        buf = (C.c_char * len(x)).from_buffer_copy(x) if isinstance(x, bytes) \
            else (C.c_char * len(x)).from_buffer(x)
        return C.addressof(buf), buf
    if hasattr(x, "ctypes"):  # numpy
        return x.ctypes.data, x
    return C.addressof(x), x


class GL:
    """One loaded backend library.  `lib.Name(args)` calls the C symbol."""

    def __init__(self, path, trace=None):
        self.path = os.path.abspath(path)
        self._dll = C.CDLL(self.path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
        self.trace = trace
        self.is_wrhip = hasattr(self._dll, "WrhipGetStats")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(self._dll, name)  # AttributeError if symbol missing
            fn.restype, fn.argtypes = res, args
            setattr(self, name, self._wrap(name, fn, args))
        if self.is_wrhip:
            for name, (res, args) in EXTRA_SIGNATURES.items():
                # (WRHIP_LIB_PATH may name an older build, for A/B runs: an addition it lacks is an AttributeError where it is used)
                fn = getattr(self._dll, name, None)
                if fn is None:
                    continue
                fn.restype, fn.argtypes = res, args
                setattr(self, name, fn)

    def _wrap(self, name, fn, argtypes):
        ptr_idx = [i for i, t in enumerate(argtypes) if t is P]
        gl = self

        def call(*a):
            if gl.trace is not None and name == "GetUniformLocation":
                # uniform locations are backend-specific (swgl numbers them per program, gl.cc:1461-1470 via the generated
                # get_uniform): the trace keeps the location this backend returned so that a replayer can translate
                loc = fn(*a)
                gl.trace.record(name, a, ret=loc)
                return loc
            if gl.trace is not None:
                gl.trace.record(name, a)
            if ptr_idx:
                a = list(a)
                keep = []
                for i in ptr_idx:
                    a[i], k = _as_ptr(a[i])
                    keep.append(k)
            return fn(*a)
        call.__name__ = name
        return call

    # --- small conveniences (not part of the ABI) -------------------------
    def gen(self, fn_name):
        out = u32(0)
        getattr(self, fn_name)(1, out)
        return out.value

    def stats(self):
        s = WrhipStats()
        self.WrhipGetStats(C.byref(s))
        return {n: getattr(s, n) for n, _ in s._fields_}

    def tap_texture(self, tex, rect=None, expected=0):
        """Enqueue a tap (include/wrhip.h, WrhipTapTexture) of `rect` = (x, y, w, h) of texture id `tex` -- None: all of it --
        against texture id `expected` (0: digest only).  Returns the ticket, or -1 (GL_INVALID_VALUE is then set)."""
        if rect is None:
            w, h = i32(0), i32(0)
            if not self.WrhipGetTextureSize(tex, C.byref(w), C.byref(h)):
                return self.WrhipTapTexture(tex, 0, 0, 0, 0, expected)
            rect = (0, 0, w.value, h.value)
        return self.WrhipTapTexture(tex, *[int(v) for v in rect], expected)

    def tap_result(self, ticket, wait=True):
        """The result of a tap as a dict (digest: two ints, hist: 256 ints), None if it has not arrived (wait=False only).
        A ticket the ring no longer holds raises KeyError."""
        r = WrhipTapResult()
        rc = self.WrhipTapResultGet(ticket, C.byref(r), 1 if wait else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise KeyError(f"tap ticket {ticket} is unknown or has been overwritten")
        return {"status": r.status, "width": r.width, "height": r.height, "format": r.format, "digest": (int(r.digest[0]), int(r.digest[1])),
                "max_diff": r.max_diff, "differing": r.differing, "hist": list(r.hist)}


    def grab_texture(self, tex, rects=None, flags=0):
        """Enqueue a grab (include/wrhip.h, WrhipGrabTexture) of texture id `tex`: `rects` is None (all of it), one rect
        (x, y, w, h) or a list of rects.  Returns the ticket, or -1 (GL_INVALID_VALUE / GL_OUT_OF_MEMORY is then set)."""
        if rects is None:
            w, h = i32(0), i32(0)
            if not self.WrhipGetTextureSize(tex, C.byref(w), C.byref(h)):
                w = h = i32(0)
            rects = [(0, 0, w.value, h.value)]
        elif len(rects) == 4 and not hasattr(rects[0], "__len__"):
            rects = [rects]
        flat = [int(v) for r in rects for v in r]
        arr = (i32 * max(1, len(flat)))(*flat)
        return self.WrhipGrabTexture(tex, C.addressof(arr), len(rects), flags)

    def grab_texture_scaled(self, tex, rect, size, flags=0):
        """Enqueue a scaled grab (include/wrhip.h, WrhipGrabTextureScaled) of `rect` = (x, y, w, h) of the RGBA8 texture id `tex`
        -- None: all of it -- scaled down to `size` = (width, height) as the reference's chain of linear blits scales it.
        `flags`: GRAB_FLIP_ROWS and / or GRAB_SWAP_RB.  Returns the ticket, or -1 (GL_INVALID_VALUE / GL_OUT_OF_MEMORY is then set)."""
        if rect is None:
            w, h = i32(0), i32(0)
            if not self.WrhipGetTextureSize(tex, C.byref(w), C.byref(h)):
                w = h = i32(0)
            rect = (0, 0, w.value, h.value)
        arr = (i32 * 4)(*[int(v) for v in rect])
        return self.WrhipGrabTextureScaled(tex, C.addressof(arr), int(size[0]), int(size[1]), flags)

    def grab_texture_tensor(self, tex, rect, dst, dst_bytes, size=None, dtype=TENSOR_F32, layout=TENSOR_CHW, channels=3, strides=(0, 0),
                            scale=(1.0, 1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0, 0.0), flags=0):
        """Enqueue a tensor grab (include/wrhip.h, WrhipGrabTextureTensor) of `rect` = (x, y, w, h) of texture id `tex` -- None: all
        of it -- into the device memory `dst` (an address: device_alloc's, or any the context's runtime can write), of which
        `dst_bytes` may be written.  size = (width, height): scaled down as grab_texture_scaled scales; None: the rect's size.
        strides = (row, plane) in elements, 0: tight; scale, bias: per output channel (up to four values; float32).
        `flags`: GRAB_FLIP_ROWS and / or TENSOR_BGR.  Returns the ticket, or -1 (GL_INVALID_VALUE / GL_OUT_OF_MEMORY is then set)."""
        if rect is None:
            w, h = i32(0), i32(0)
            if not self.WrhipGetTextureSize(tex, C.byref(w), C.byref(h)):
                w = h = i32(0)
            rect = (0, 0, w.value, h.value)
        arr = (i32 * 4)(*[int(v) for v in rect])
        size = (rect[2], rect[3]) if size is None else size
        d = WrhipTensorDesc()
        d.dst, d.dst_bytes = int(dst) or None, int(dst_bytes)
        d.out_w, d.out_h = int(size[0]), int(size[1])
        d.dtype, d.layout, d.channels = int(dtype), int(layout), int(channels)
        d.row_stride, d.plane_stride = int(strides[0]), int(strides[1])
        for k in range(4):
            d.scale[k] = float(scale[k]) if k < len(scale) else 1.0
            d.bias[k] = float(bias[k]) if k < len(bias) else 0.0
        d.flags = int(flags)
        return self.WrhipGrabTextureTensor(tex, C.addressof(arr), C.addressof(d))

    def grab_texture_yuv(self, tex, rect, format, color_space, flags=0, dst=None, dst_bytes=0, strides=(0, 0)):
        """Enqueue a YUV grab (include/wrhip.h, WrhipGrabTextureYuv) of `rect` = (x, y, w, h) of the RGBA8 texture id `tex` -- None:
        all of it -- as 8-bit planes in `format` (YUV_I420, YUV_NV12, YUV_I444) of the ranged colour space `color_space` (0 .. 5).
        dst None: the planes cross to the host, grab_result delivers them; otherwise a device address of which `dst_bytes` may be
        written, strides = (Y, chroma) in bytes, 0: tight.  `flags`: 0 or GRAB_FLIP_ROWS.  Returns the ticket, or -1
        (GL_INVALID_VALUE / GL_OUT_OF_MEMORY is then set)."""
        if rect is None:
            w, h = i32(0), i32(0)
            if not self.WrhipGetTextureSize(tex, C.byref(w), C.byref(h)):
                w = h = i32(0)
            rect = (0, 0, w.value, h.value)
        arr = (i32 * 4)(*[int(v) for v in rect])
        d = WrhipYuvDesc()
        d.format, d.color_space, d.flags = int(format), int(color_space), int(flags)
        d.dst, d.dst_bytes = (int(dst) or None) if dst is not None else None, int(dst_bytes)
        d.y_stride, d.c_stride = int(strides[0]), int(strides[1])
        return self.WrhipGrabTextureYuv(tex, C.addressof(arr), C.addressof(d))

    def grab_texture_yuv_delta(self, tex, rect, format, color_space, flags=0, dst=None, dst_bytes=0, strides=(0, 0), key=False, scroll=False):
        """Enqueue a delta YUV grab (include/wrhip.h, WrhipGrabTextureYuvDelta): grab_texture_yuv's arguments, but only the 64 x 64
        blocks whose samples differ from the texture's retained planes are sent -- to the host as entries that grab_result patches
        into the caller's planes (`into`), or straight into the device planes at `dst`.  key: GRAB_KEY, every block is sent (an int is
        passed on as the call's raw `flags`).  scroll: GRAB_DELTA | GRAB_SCROLL beside it -- blocks found scroll_dy rows away in the retained planes are
        sent as 16-byte COPY entries, or written into the device planes from the retained ones.  Returns the ticket, or -1 (GL_INVALID_VALUE / GL_OUT_OF_MEMORY is then set)."""
        if rect is None:
            w, h = i32(0), i32(0)
            if not self.WrhipGetTextureSize(tex, C.byref(w), C.byref(h)):
                w = h = i32(0)
            rect = (0, 0, w.value, h.value)
        arr = (i32 * 4)(*[int(v) for v in rect])
        d = WrhipYuvDesc()
        d.format, d.color_space, d.flags = int(format), int(color_space), int(flags)
        d.dst, d.dst_bytes = (int(dst) or None) if dst is not None else None, int(dst_bytes)
        d.y_stride, d.c_stride = int(strides[0]), int(strides[1])
        return self.WrhipGrabTextureYuvDelta(tex, C.addressof(arr), C.addressof(d), (GRAB_KEY if key is True else int(key)) | (GRAB_DELTA | GRAB_SCROLL if scroll else 0))

    def grab_texture_yuv_scaled(self, tex, rect, size, format, color_space, flags=0, renditions=1, dsts=None, strides=None):
        """Enqueue a scaled YUV grab (include/wrhip.h, WrhipGrabTextureYuvScaled) of `rect` = (x, y, w, h) of the RGBA8 texture id
        `tex` -- None: all of it -- scaled down to `size` = (width, height) as grab_texture_scaled scales it, as 8-bit planes in
        `format` of the ranged colour space `color_space`: `renditions` of them, rendition k being level k of the chain, size << k.
        dsts None: all planes cross to the host, grab_result delivers them flat (yuv_split_renditions cuts them); otherwise one
        (device address, dst_bytes) per rendition, with strides = one (Y, chroma) pair in bytes per rendition (None: tight).
        `flags`: 0 or GRAB_FLIP_ROWS.  Returns the ticket, or -1 (GL_INVALID_VALUE / GL_OUT_OF_MEMORY is then set)."""
        if rect is None:
            w, h = i32(0), i32(0)
            if not self.WrhipGetTextureSize(tex, C.byref(w), C.byref(h)):
                w = h = i32(0)
            rect = (0, 0, w.value, h.value)
        arr = (i32 * 4)(*[int(v) for v in rect])
        n = int(renditions)
        descs = (WrhipYuvDesc * max(1, n))()
        for k in range(max(0, min(n, len(descs)))):
            d = descs[k]
            d.format, d.color_space, d.flags = int(format), int(color_space), int(flags)
            if dsts is not None:
                d.dst, d.dst_bytes = int(dsts[k][0]) or None, int(dsts[k][1])
            if strides is not None:
                d.y_stride, d.c_stride = int(strides[k][0]), int(strides[k][1])
        return self.WrhipGrabTextureYuvScaled(tex, C.addressof(arr), int(size[0]), int(size[1]), C.addressof(descs), n)

    def device_alloc(self, nbytes):
        """Device memory for tensor grabs (WrhipDeviceAlloc): its address, 16-byte aligned; 0 with GL_OUT_OF_MEMORY set"""
        return self.WrhipDeviceAlloc(int(nbytes)) or 0

    def device_free(self, ptr):
        """WrhipDeviceFree: parked grabs are sent and the draw stream is waited for first"""
        self.WrhipDeviceFree(int(ptr) or None)

    def device_read(self, ptr, nbytes):
        """`nbytes` of device memory as a uint8 array (WrhipDeviceRead: a copy on the draw stream behind everything issued so far)"""
        import numpy as np
        out = np.empty(int(nbytes), np.uint8)
        rc = self.WrhipDeviceRead(out.ctypes.data, int(ptr), int(nbytes))
        assert rc == 0, rc
        return out

    def device_write(self, ptr, data):
        """The bytes of `data` (bytes, or a C-contiguous numpy array) into device memory at `ptr` (WrhipDeviceWrite: a copy on the draw
        stream behind everything issued so far, waited for)"""
        import numpy as np
        buf = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data)
        rc = self.WrhipDeviceWrite(int(ptr), buf.ctypes.data, int(buf.nbytes))
        assert rc == 0, rc

    def put_texture_tensor(self, tex, rect, src, src_bytes, dtype=TENSOR_F32, layout=TENSOR_CHW, channels=3, strides=(0, 0),
                           scale=(1.0, 1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0, 0.0), alpha=255, flags=0):
        """A tensor put (include/wrhip.h, WrhipPutTextureTensor): the tensor of rect.w x rect.h pixels in the device memory `src` (an
        address: device_alloc's, or any the context's runtime can read), of which `src_bytes` may be read, becomes the stored bytes
        of `rect` = (x, y, w, h) of texture id `tex` -- None: all of it.  strides = (row, plane) in elements, 0: tight; scale, bias:
        per input channel (up to four values; float32); alpha: the A byte of a 3-channel tensor.  `flags`: GRAB_FLIP_ROWS and / or
        TENSOR_BGR.  Returns 0, or -1 (GL_INVALID_VALUE is then set)."""
        if rect is None:
            w, h = i32(0), i32(0)
            if not self.WrhipGetTextureSize(tex, C.byref(w), C.byref(h)):
                w = h = i32(0)
            rect = (0, 0, w.value, h.value)
        arr = (i32 * 4)(*[int(v) for v in rect])
        d = WrhipTensorSrc()
        d.src, d.src_bytes = int(src) or None, int(src_bytes)
        d.dtype, d.layout, d.channels = int(dtype), int(layout), int(channels)
        d.row_stride, d.plane_stride = int(strides[0]), int(strides[1])
        for k in range(4):
            d.scale[k] = float(scale[k]) if k < len(scale) else 1.0
            d.bias[k] = float(bias[k]) if k < len(bias) else 0.0
        d.alpha, d.flags = int(alpha), int(flags)
        return self.WrhipPutTextureTensor(tex, C.addressof(arr), C.addressof(d))

    def put_texture_payload(self, tex, rect, payload, flags):
        """A payload put (include/wrhip.h, WrhipPutTexturePayload): the delta, packed or scroll payload `payload` (grab_payload's
        bytes, header included; `flags`: the producing grab's) is decoded on the device into `rect` = (x, y, w, h) of texture id
        `tex` -- None: all of it.  Returns 0, or -1 (GL_INVALID_VALUE is then set)."""
        if rect is None:
            w, h = i32(0), i32(0)
            if not self.WrhipGetTextureSize(tex, C.byref(w), C.byref(h)):
                w = h = i32(0)
            rect = (0, 0, w.value, h.value)
        arr = (i32 * 4)(*[int(v) for v in rect])
        if payload is None:
            return self.WrhipPutTexturePayload(tex, C.addressof(arr), None, 0, int(flags))
        src = (C.c_char * max(1, len(payload))).from_buffer_copy(bytes(payload).ljust(1, b"\0"))
        return self.WrhipPutTexturePayload(tex, C.addressof(arr), src, len(payload), int(flags))

    def grab_result(self, ticket, wait=True, into=None):
        """The result of a grab: (info dict, pixels).  Full mode: one array per rect ((h, w, 4) stored B, G, R, A bytes, or (h, w)
        for R8) -- the array itself for a single rect, a list for several.  A scaled grab: the (scaled_h, scaled_w, 4) array.  A tensor grab: None.  A YUV grab: the planes as one flat uint8 array (yuv_split cuts it; empty for a device sink).  A delta YUV grab: the caller's flat planes `into` (that layout) with the sent blocks patched in -- left alone by a device sink's ticket; None: the info alone.  Delta mode: the caller's image `into` of the rect (a
        C-contiguous uint8 array of the rect's shape; None: a fresh one of zeros) with the sent blocks patched in.  None if the
        result has not arrived (wait=False only); a ticket the ring no longer holds raises KeyError."""
        import numpy as np
        r = WrhipGrabInfo()
        rc = self.WrhipGrabResultGet(ticket, C.byref(r), None, 0, 1 if wait else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise KeyError(f"grab ticket {ticket} is unknown or has been overwritten")
        rects = [tuple(r.rects[i]) for i in range(r.nrects)]
        bpp = 1 if r.format == 0x8229 else 4          # GL_R8
        shape = lambda w, h: (h, w) if bpp == 1 else (h, w, 4)
        if r.flags & GRAB_TENSOR:
            pixels = buf = None          # (the elements are in the caller's device memory)
        elif r.flags & GRAB_YUV and r.flags & GRAB_DELTA:
            # (a delta YUV grab: `into` is the caller's flat planes -- a full YUV grab's payload layout, yuv_split cuts it -- and the
            # sent blocks are patched in.  A device sink's ticket carries records of 16 bytes: nothing to patch, `into` is left alone.
            # `into` None: the info alone)
            assert into is None or (into.dtype == np.uint8 and into.flags["C_CONTIGUOUS"] and into.ndim == 1), "grab_result: `into` is not flat uint8 planes"
            if into is not None and r.blocks and not r.flags & GRAB_SCROLL:      # (a scroll grab's entries differ in size)
                w, h = rects[0][2:]
                entry = (int(r.bytes) - GRAB_HEADER) // r.blocks      # (16: records alone; I420 and NV12 planes are the same size)
                fmt = YUV_I444 if entry == 16 + 3 * GRAB_BLOCK * GRAB_BLOCK else YUV_I420
                assert entry == 16 or len(into) == sum(rows * row for rows, row in yuv_plane_shapes(w, h, fmt)), "grab_result: `into` is not the rect's planes"
            pixels = buf = into
        elif r.flags & GRAB_YUV:
            # (the planes, tight, one after another -- yuv_split cuts them apart; a device sink's ticket carries none)
            pixels = buf = np.empty(int(r.bytes) - GRAB_HEADER, np.uint8)
        elif r.flags & GRAB_SCALED:
            pixels = buf = np.empty((r.scaled_h, r.scaled_w, 4), np.uint8)
        elif r.flags & GRAB_DELTA:
            out = np.zeros(shape(*rects[0][2:]), np.uint8) if into is None else into
            assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.shape == shape(*rects[0][2:]), "grab_result: `into` is not the rect's image"
            pixels, buf = out, out
        else:
            buf = np.empty(sum(w * h * bpp for _, _, w, h in rects), np.uint8)
            parts, at = [], 0
            for _, _, w, h in rects:
                parts.append(buf[at:at + w * h * bpp].reshape(shape(w, h)))
                at += w * h * bpp
            pixels = parts[0] if len(parts) == 1 else parts
        if buf is not None:
            rc = self.WrhipGrabResultGet(ticket, C.byref(r), buf.ctypes.data, 0, 1)
            assert rc == 0, rc
        info = {"status": r.status, "format": r.format, "flags": r.flags, "rects": rects, "keyframe": r.keyframe, "blocks": r.blocks,
                "blocks_total": r.blocks_total, "damage": tuple(r.damage), "bytes": int(r.bytes),
                "scaled_w": r.scaled_w, "scaled_h": r.scaled_h, "levels": r.levels, "renditions": r.renditions,
                "scroll_dy": r.scroll_dy, "copied": r.copied}
        return info, pixels

    def grab_payload(self, ticket, wait=True):
        """The bytes of a grab as they crossed to the host (include/wrhip.h, WrhipGrabPayloadGet): the 16-byte header, then the
        payload.  None if they have not arrived (wait=False only); a ticket the ring no longer holds raises KeyError."""
        n = u64(0)
        rc = self.WrhipGrabPayloadGet(ticket, None, 0, C.byref(n), 1 if wait else 0)
        if rc == 1:
            return None
        if rc != 0:
            raise KeyError(f"grab ticket {ticket} is unknown or has been overwritten")
        buf = C.create_string_buffer(n.value)
        rc = self.WrhipGrabPayloadGet(ticket, buf, n.value, C.byref(n), 1)
        assert rc == 0 and n.value == len(buf), (rc, n.value)
        return buf.raw

    def grab_decode(self, payload, fmt, flags, into):
        """Patch a delta payload (grab_payload's bytes; `flags`: the grab's, GRAB_PACKED or not) into `into`, the caller's image of
        the rect (a C-contiguous uint8 array, (h, w, 4) for GL_RGBA8, (h, w) for GL_R8): (damage, blocks).  A pure host function
        (WrhipGrabDecode); a malformed payload raises ValueError and leaves `into` as it was."""
        import numpy as np
        bpp = 1 if fmt == 0x8229 else 4          # GL_R8
        assert into.dtype == np.uint8 and into.flags["C_CONTIGUOUS"] and into.ndim == (2 if bpp == 1 else 3), "grab_decode: `into` is not an image of the rect"
        damage, blocks = (i32 * 4)(), u32(0)
        src = (C.c_char * len(payload)).from_buffer_copy(payload)
        rc = self.WrhipGrabDecode(src, len(payload), fmt, flags, into.shape[1], into.shape[0], into.ctypes.data, 0, damage, C.byref(blocks))
        if rc != 0:
            raise ValueError("grab_decode: malformed payload")
        return tuple(damage), blocks.value

    def grab_decode_yuv(self, payload, format, w, h, into, scroll=False):
        """Patch a host-sink delta YUV payload (grab_payload's bytes) into `into`, the caller's flat planes of the w x h image in a
        full YUV grab's payload layout (yuv_split cuts it); None: only checked.  (damage, blocks).  scroll: the payload is a
        GRAB_SCROLL grab's -- COPY entries are applied in place first.  A pure host function
        (WrhipGrabDecodeYuv); a malformed payload raises ValueError and leaves `into` as it was."""
        import numpy as np
        shapes = yuv_plane_shapes(w, h, format)
        ptrs = [None, None, None]
        if into is not None:
            assert into.dtype == np.uint8 and into.flags["C_CONTIGUOUS"] and into.shape == (sum(rows * row for rows, row in shapes),), "grab_decode_yuv: `into` is not the image's planes"
            at = 0
            for k, (rows, row) in enumerate(shapes):
                ptrs[k] = into.ctypes.data + at
                at += rows * row
        damage, blocks = (i32 * 4)(), u32(0)
        src = (C.c_char * len(payload)).from_buffer_copy(payload)
        rc = self.WrhipGrabDecodeYuv(src, len(payload), int(format) | (GRAB_SCROLL if scroll else 0), int(w), int(h), ptrs[0], 0, ptrs[1], ptrs[2], 0, damage, C.byref(blocks))
        if rc != 0:
            raise ValueError("grab_decode_yuv: malformed payload")
        return tuple(damage), blocks.value


def repo_root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wrhip_path():
    # WRHIP_LIB_PATH: another build of the same library (A/B measurements of kernel variants on one GPU box)
    return os.environ.get("WRHIP_LIB_PATH") or os.path.join(repo_root(), "webrender_amd", "csrc", "libwrhip.so")


def load_wrhip(trace=None):
    """Load the product backend.  Fails loudly if the HIP library is not built:
    there is no CPU fallback in the product path."""
    p = wrhip_path()
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} not built -- run `python -c 'import __graft_entry__ as g; g.build()'`")
    return GL(p, trace)
