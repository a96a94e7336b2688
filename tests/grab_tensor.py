"""Helpers of tests/test_grab_tensor.py: the contract of a tensor grab (include/wrhip.h, WrhipGrabTextureTensor) restated in numpy
-- which stored byte an output channel takes, the value an element holds, the two roundings, where the element lies -- and a
destination in device memory that is filled with a guard byte first and compared WHOLE afterwards.

Stored bytes are the grabs' (tests/frame_grabs.py): an RGBA8 pixel holds B, G, R, A.  Expected values are raw bits: uint8 for U8,
the uint16 pattern for F16 and BF16, the uint32 pattern for F32.  Nothing here has a tolerance."""
import ctypes as C
import numpy as np
from webrender_amd import glapi

U8, F16, BF16, F32 = glapi.TENSOR_U8, glapi.TENSOR_F16, glapi.TENSOR_BF16, glapi.TENSOR_F32
CHW, HWC = glapi.TENSOR_CHW, glapi.TENSOR_HWC
BGR, FLIP, TENSOR = glapi.TENSOR_BGR, glapi.GRAB_FLIP_ROWS, glapi.GRAB_TENSOR
ELEM = {U8: 1, F16: 2, BF16: 2, F32: 4}
BITS = {U8: np.uint8, F16: np.uint16, BF16: np.uint16, F32: np.uint32}
GUARD = 0xA5

# the ImageNet normalisation of a byte, 1 / (255 * std) and -mean / std, computed in float32 on the host; the fourth (alpha): v / 255
_MEAN = np.array([0.485, 0.456, 0.406, 0.0], np.float32)
_STD = np.array([0.229, 0.224, 0.225, 1.0], np.float32)
SCALE = np.float32(1.0) / (np.float32(255.0) * _STD)
BIAS = -_MEAN / _STD


def bf16_bits(x):
    """float32 array -> the uint16 patterns of its values rounded to nearest even (finite values)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def expected(px, dtype, layout, channels, scale=SCALE, bias=BIAS, flags=0):
    """The tensor the contract gives for the stored bytes `px` ((h, w, 4) B, G, R, A or (h, w) R8), as raw bits: (C, h, w) for
    CHW, (h, w, C) for HWC"""
    if px.ndim == 2:
        assert channels == 1
        v = px[:, :, None]
    else:
        order = [0, 1, 2, 3] if flags & BGR else [2, 1, 0, 3]
        v = px[:, :, order[:channels]]
    if flags & FLIP:
        v = v[::-1]
    if dtype == U8:
        out = v
    else:
        s, b = np.asarray(scale, np.float32)[:channels], np.asarray(bias, np.float32)[:channels]
        x = v.astype(np.float32) * s + b                    # two float32 operations, each rounded once
        assert x.dtype == np.float32
        if dtype == F32:
            out = x.view(np.uint32)
        elif dtype == F16:
            with np.errstate(over="ignore"):
                out = x.astype(np.float16).view(np.uint16)
        else:
            out = bf16_bits(x)
    if layout == CHW:
        out = out.transpose(2, 0, 1)
    return np.ascontiguousarray(out).astype(BITS[dtype], copy=False)


def geometry(shape, layout, row=0, plane=0):
    """-> (row stride, plane stride, extent), in elements, of a tensor of `shape` with the given strides (0: tight)"""
    if layout == CHW:
        c, h, w = shape
        row = row or w
        plane = plane or h * row
        return row, plane, (c - 1) * plane + (h - 1) * row + w
    h, w, c = shape
    row = row or w * c
    return row, 0, (h - 1) * row + w * c


def on_device(gl):
    return bool(gl.WrhipGetStream())


def fill(gl, ptr, nbytes, value=GUARD):
    """Every byte of a WrhipDeviceAlloc'd buffer set to `value`, complete before the call returns"""
    if not on_device(gl):
        C.memset(ptr, value, nbytes)
        return
    import torch
    from webrender_amd.dist import DeviceArray
    torch.as_tensor(DeviceArray(ptr, nbytes), device="cuda").fill_(value)
    torch.cuda.synchronize()


class Dest:
    """A destination: `off` elements of guard ahead of `dst`, the tensor's extent, 48 bytes of guard behind it -- all GUARD at first"""

    def __init__(self, gl, shape, dtype, layout, off=0, row=0, plane=0):
        self.gl, self.shape, self.dtype, self.layout = gl, tuple(shape), dtype, layout
        self.elem = ELEM[dtype]
        self.row, self.plane, self.extent = geometry(shape, layout, row, plane)
        self.strides = (row, plane)
        self.off = off * self.elem
        self.nbytes = (self.off + self.extent * self.elem + 48 + 15) & ~15
        self.base = gl.device_alloc(self.nbytes)
        assert self.base and self.base % 16 == 0, self.base
        fill(gl, self.base, self.nbytes)
        self.dst = self.base + self.off
        self.dst_bytes = self.extent * self.elem          # exactly what the tensor needs: the library may ask for no more

    def image(self, want):
        """The whole buffer as it has to read after the grab: `want` at the contract's addresses, GUARD everywhere else"""
        assert want.shape == self.shape and want.dtype == BITS[self.dtype], (want.shape, want.dtype, self.shape)
        img = np.full(self.nbytes, GUARD, np.uint8)
        el = img[self.off:self.off + self.extent * self.elem].view(BITS[self.dtype])
        e = self.elem
        if self.layout == CHW:
            strides = (self.plane * e, self.row * e, e)
        else:
            strides = (self.row * e, self.shape[2] * e, e)
        np.lib.stride_tricks.as_strided(el, self.shape, strides)[...] = want
        return img

    def read(self):
        return self.gl.device_read(self.base, self.nbytes)

    def check(self, want, what=""):
        got, img = self.read(), self.image(want)
        bad = int((got != img).sum())
        inside = self.image(np.zeros_like(want)) != self.image(np.full_like(want, 0xFF))      # (the bytes of the contract's elements)
        assert bad == 0, f"{what}: {int((got != img)[inside].sum())} bytes of the tensor differ, {int((got != img)[~inside].sum())} bytes outside it were written"

    def free(self):
        self.gl.device_free(self.base)
        self.base = 0


def grab(s, tex, rect, d, size=None, channels=None, scale=SCALE, bias=BIAS, flags=0):
    """A tensor grab of `rect` of texture id `tex` into the Dest `d`: the ticket"""
    ch = channels if channels is not None else (d.shape[0] if d.layout == CHW else d.shape[2])
    t = s.gl.grab_texture_tensor(tex, rect, d.dst, d.dst_bytes, size=size, dtype=d.dtype, layout=d.layout, channels=ch,
                                 strides=d.strides, scale=scale, bias=bias, flags=flags)
    assert t >= 0, (t, s.gl.GetError())
    return t


def check_info(info, rect, flags, fmt, scaled=None):
    """What WrhipGrabResultGet reports for a tensor ticket; scaled: (w, h, L), None for an unscaled grab"""
    assert (info["status"], info["format"], info["flags"], info["rects"]) == (0, fmt, flags | TENSOR, [tuple(rect)]), info
    assert (info["scaled_w"], info["scaled_h"], info["levels"]) == (scaled or (0, 0, 0)), info
    assert info["bytes"] == glapi.GRAB_HEADER, info


def send_held(gl):
    """What the library holds back goes out without a wait: a WrhipFlushHeld that finds nothing recorded since the one before"""
    gl.WrhipFlushHeld()
    assert gl.WrhipFlushHeld() == 0


def shape_of(w, h, layout, channels):
    return (channels, h, w) if layout == CHW else (h, w, channels)
