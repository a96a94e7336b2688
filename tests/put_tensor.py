"""Helpers of tests/test_put_tensor.py: the contract of a tensor put (include/wrhip.h, WrhipPutTextureTensor) restated in numpy --
the value an element stands for, the clamp, the rounding, which stored byte an input channel supplies, where it lands -- a source
tensor laid out in device memory at given strides, and a session that runs one call script on either backend: on libwrhip a put is
WrhipPutTextureTensor, on the oracle it is TexSubImage2D of the bytes the restatement gives.

Stored bytes are the grabs' (tests/frame_grabs.py): an RGBA8 pixel holds B, G, R, A; an RG8 pixel its two bytes; R8 the one.
Tensors are raw bits: uint8 for U8, the uint16 pattern for F16 and BF16, the uint32 pattern for F32.  Nothing here has a tolerance."""
import numpy as np
from webrender_amd import glapi, glconst as G
import frame_grabs as fg
import grab_tensor as gt
from grab_tensor import U8, F16, BF16, F32, CHW, HWC, BGR, FLIP, ELEM, BITS

BPP = {G.GL_RGBA8: 4, G.GL_RG8: 2, G.GL_R8: 1}
UPLOAD = {G.GL_RGBA8: G.GL_BGRA, G.GL_RG8: G.GL_RG, G.GL_R8: G.GL_RED}
GUARD = 0xA5

# per input channel: 255 (colours in [0, 1]), and three pairs of powers of two and short fractions, under which y = k + 0.5 is hit
# exactly by elements every format holds
SCALE = np.array([255.0, 64.0, 2.0, 1.0], np.float32)
BIAS = np.array([0.0, -8.0, 0.5, -3.25], np.float32)


def to_f32(bits, dtype):
    """Raw element bits -> the float32 of the same value, exactly"""
    if dtype == F32:
        return np.ascontiguousarray(bits, np.uint32).view(np.float32)
    if dtype == F16:
        return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float32)
    return (np.ascontiguousarray(bits).astype(np.uint32) << 16).view(np.float32)


def from_f32(x, dtype):
    """float32 values -> raw bits of elements near them (how near does not matter: expectations start from the bits)"""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == F32:
        return x.view(np.uint32).copy()
    if dtype == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16).copy()
    return gt.bf16_bits(x)


def y_of(bits, dtype, scale, bias):
    """(..., C) raw bits -> y = x * scale[c] + bias[c]: two float32 operations, each rounded once"""
    c = bits.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        y = to_f32(bits, dtype) * np.asarray(scale, np.float32)[:c] + np.asarray(bias, np.float32)[:c]
    assert y.dtype == np.float32
    return y


def byte_of(y):
    """float32 y -> the stored byte: 0 for a NaN or y < 0, 255 for y >= 255, np.rint (ties to even) otherwise"""
    with np.errstate(invalid="ignore"):
        inside = (y >= 0) & (y < 255)                       # (a NaN is not inside)
        r = np.rint(np.where(inside, y, np.float32(0)))
        return np.where(y >= 255, 255, r).astype(np.uint8)


def expected(t, dtype, layout, fmt, scale=SCALE, bias=BIAS, alpha=255, flags=0):
    """The stored bytes the contract gives for the tensor `t` of raw bits, (C, h, w) for CHW or (h, w, C) for HWC, put into a texture
    of format `fmt`: (h, w, 4) B, G, R, A, (h, w, 2), or (h, w)"""
    assert t.dtype == BITS[dtype]
    el = t.transpose(1, 2, 0) if layout == CHW else t
    h, w, c = el.shape
    b = el if dtype == U8 else byte_of(y_of(el, dtype, scale, bias))
    if flags & FLIP:
        b = b[::-1]                                          # tensor row r -> rect row h - 1 - r
    if fmt == G.GL_R8:
        assert c == 1
        return np.ascontiguousarray(b[:, :, 0])
    if fmt == G.GL_RG8:
        assert c == 2
        return np.ascontiguousarray(b)
    assert c in (3, 4)
    out = np.empty((h, w, 4), np.uint8)
    src = (0, 1, 2) if flags & BGR else (2, 1, 0)            # stored B, G, R come from these input channels
    for k in range(3):
        out[:, :, k] = b[:, :, src[k]]
    out[:, :, 3] = b[:, :, 3] if c == 4 else alpha
    return out


def tensor(rng, w, h, dtype, layout, channels, scale=SCALE, bias=BIAS):
    """A tensor of raw bits whose y values fall below 0, above 255, on ties, on whole numbers and anywhere between"""
    n = h * w
    if dtype == U8:
        el = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    else:
        kind = rng.integers(0, 10, (n, channels))
        y = rng.uniform(-60.0, 330.0, (n, channels))
        y = np.where(kind < 3, rng.integers(0, 255, (n, channels)) + 0.5, y)
        y = np.where(kind == 3, rng.integers(0, 256, (n, channels)), y)
        x = (y - np.asarray(bias, np.float64)[:channels]) / np.asarray(scale, np.float64)[:channels]
        el = from_f32(x.astype(np.float32), dtype).reshape(h, w, channels)
    return np.ascontiguousarray(el.transpose(2, 0, 1) if layout == CHW else el)


def covers_the_rule(t, dtype, layout, scale=SCALE, bias=BIAS):
    """Does the tensor's y fall below 0, reach 255, and sit on ties that round down and up?"""
    if dtype == U8:
        return True
    y = y_of(t.transpose(1, 2, 0) if layout == CHW else t, dtype, scale, bias).astype(np.float64)
    tie = (y > 0) & (y < 255) & (y - np.floor(y) == 0.5)
    down, up = tie & (np.floor(y) % 2 == 0), tie & (np.floor(y) % 2 == 1)
    return bool((y < 0).any() and (y >= 255).any() and down.any() and up.any())


class Src:
    """A tensor in device memory: `off` elements of guard ahead of `src`, the elements at their strides with guard bytes in the
    padding, 48 bytes of guard behind; src_bytes is exactly the extent"""

    def __init__(self, gl, t, dtype, layout, off=0, row=0, plane=0):
        self.gl, self.dtype, self.layout = gl, dtype, layout
        e = ELEM[dtype]
        self.row, self.plane, self.extent = gt.geometry(t.shape, layout, row, plane)
        self.strides = (row, plane)
        self.channels = t.shape[0] if layout == CHW else t.shape[2]
        nbytes = (off * e + self.extent * e + 48 + 15) & ~15
        img = np.full(nbytes, GUARD, np.uint8)
        el = img[off * e:off * e + self.extent * e].view(BITS[dtype])
        st = (self.plane * e, self.row * e, e) if layout == CHW else (self.row * e, t.shape[2] * e, e)
        np.lib.stride_tricks.as_strided(el, t.shape, st)[...] = t
        self.base = gl.device_alloc(nbytes)
        assert self.base and self.base % 16 == 0, self.base
        gl.device_write(self.base, img)
        self.src = self.base + off * e
        self.src_bytes = self.extent * e

    def free(self):
        self.gl.device_free(self.base)
        self.base = 0


def put(gl, tex_id, rect, src, scale=SCALE, bias=BIAS, alpha=255, flags=0):
    return gl.put_texture_tensor(tex_id, rect, src.src, src.src_bytes, dtype=src.dtype, layout=src.layout, channels=src.channels,
                                 strides=src.strides, scale=scale, bias=bias, alpha=alpha, flags=flags)


class Session(fg.Session):
    """fg.Session on either backend, with textures of the three formats and puts"""

    def __init__(self, lib, w=64, h=64):
        from webrender_amd.renderer import Renderer
        self.gl = glapi.GL(lib)
        self.r = Renderer(self.gl, w, h)
        self.d = self.r.device
        self.wrhip = self.gl.is_wrhip
        self.window = self.gl.WrhipGetFramebufferTexture(0) if self.wrhip else 0

    def make(self, px, fmt, render_target=True):
        h, w = px.shape[:2]
        t = self.d.create_texture(w, h, fmt, render_target=render_target)
        self.write(t, 0, 0, px)
        return t

    def write(self, t, x, y, px):
        """TexSubImage2D of stored bytes"""
        h, w = px.shape[:2]
        self.d.upload_texture(t, x, y, w, h, UPLOAD[t.format], G.GL_UNSIGNED_BYTE, np.ascontiguousarray(px))

    def read(self, t):
        """The texture's stored bytes, whole"""
        if t.format != G.GL_RG8:
            return self.d.read_texture(t).copy()
        gl = self.gl
        out = np.empty((t.height, t.width, 2), np.uint8)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, t.fbo)
        gl.ReadPixels(0, 0, t.width, t.height, G.GL_RG, G.GL_UNSIGNED_BYTE, out)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)
        return out

    def put(self, t, rect, tens, dtype, layout, scale=SCALE, bias=BIAS, alpha=255, flags=0, off=0, row=0, plane=0, quiet=True, what=""):
        """The put under test.  libwrhip: the tensor goes to device memory (its copy is waited for) and is put -- quiet: nothing
        pending touches the texture, so exactly one launch, no flush, no byte from the host.  The oracle: TexSubImage2D of the
        restatement's bytes."""
        if not self.wrhip:
            self.write(t, rect[0], rect[1], expected(tens, dtype, layout, t.format, scale, bias, alpha, flags))
            return
        src = Src(self.gl, tens, dtype, layout, off, row, plane)
        a = self.stats()
        rc = put(self.gl, t.id, rect, src, scale, bias, alpha, flags)
        b = self.stats()
        assert rc == 0, (what, rc, self.gl.GetError())
        if quiet:
            assert b["kernel_launches"] == a["kernel_launches"] + 1 and b["flushes"] == a["flushes"], (what, a, b)
            assert b["h2d_bytes"] == a["h2d_bytes"] and b["d2h_bytes"] == a["d2h_bytes"], (what, a, b)
        src.free()


def differing(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a != b).sum())
