"""Helpers of tests/test_grab_yuv.py: the contract of a YUV grab (include/wrhip.h, WrhipGrabTextureYuv) restated in numpy -- the
table of the six ranged colour spaces typed in from the contract, luma, per-pixel and 2 x 2 chroma, the plane layouts -- and a
destination in device memory that is filled with a guard byte first and compared WHOLE afterwards.

Stored bytes are the grabs' (tests/frame_grabs.py): an RGBA8 pixel holds B, G, R, A.  Nothing here has a tolerance."""
import numpy as np
from webrender_amd import glapi
import grab_tensor as gt

I420, NV12, I444 = glapi.YUV_I420, glapi.YUV_NV12, glapi.YUV_I444
FORMATS = (I420, NV12, I444)
SPACES = tuple(range(6))
FLIP, YUV = glapi.GRAB_FLIP_ROWS, glapi.GRAB_YUV
GUARD = gt.GUARD

# colour space: (Y, Cb, Cr), each R, G, B in 16.16 fixed point
TABLE = {
    0: ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681)),        # Rec601Narrow
    1: ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),       # Rec601Full
    2: ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639)),        # Rec709Narrow
    3: ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005)),        # Rec709Full
    4: ((14786, 38160, 3338), (-8038, -20746, 28784), (28784, -26469, -2315)),        # Rec2020Narrow
    5: ((17216, 44434, 3886), (-9151, -23617, 32768), (32768, -30133, -2635)),        # Rec2020Full
}
KR_KB = {0: (0.299, 0.114), 1: (0.299, 0.114), 2: (0.2126, 0.0722), 3: (0.2126, 0.0722), 4: (0.2627, 0.0593), 5: (0.2627, 0.0593)}


def full_range(space):
    return space % 2 == 1


def y0_of(space):
    return 0 if full_range(space) else 16


def real_rows(space):
    """The float64 rows (Y, Cb, Cr over R, G, B) the table is derived from, range scale included"""
    kr, kb = KR_KB[space]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range(space) else (219.0 / 255.0, 224.0 / 255.0)
    y = np.array([kr, kg, kb]) * ys
    cb = np.array([-kr, -kg, 1.0 - kb]) / (2.0 * (1.0 - kb)) * cs
    cr = np.array([1.0 - kr, -kg, -kb]) / (2.0 * (1.0 - kr)) * cs
    return y, cb, cr


def derived_table(space):
    """The derivation rule of the contract: each entry times 65536 rounded to nearest, then the green entry takes up the difference
    to the row's sum -- round(scale * 65536) for Y, 0 for chroma"""
    out = []
    for k, row in enumerate(real_rows(space)):
        q = [int(np.floor(v * 65536.0 + 0.5)) for v in row]
        total = (65536 if full_range(space) else int(np.floor(219.0 / 255.0 * 65536.0 + 0.5))) if k == 0 else 0
        q[1] = total - q[0] - q[2]
        out.append(tuple(q))
    return tuple(out)


def _rgb(px):
    """(h, w, 4) stored B, G, R, A -> R, G, B as int64"""
    v = px.astype(np.int64)
    return v[..., 2], v[..., 1], v[..., 0]


def luma(px, space):
    r, g, b = _rgb(px)
    c = TABLE[space][0]
    return (c[0] * r + c[1] * g + c[2] * b + (y0_of(space) << 16) + 0x8000) >> 16


def chroma444_raw(px, space, k):
    """plane k (1: Cb, 2: Cr) per pixel, BEFORE the clamp"""
    r, g, b = _rgb(px)
    c = TABLE[space][k]
    return (c[0] * r + c[1] * g + c[2] * b + (128 << 16) + 0x8000) >> 16


def sums420(px):
    """The channel-wise sums (R, G, B) of the 2 x 2 blocks of the image, positions clamped to it: (ch, cw) each"""
    h, w = px.shape[:2]
    ys = np.minimum(np.arange(0, 2 * ((h + 1) // 2)), h - 1)
    xs = np.minimum(np.arange(0, 2 * ((w + 1) // 2)), w - 1)
    v = px[ys][:, xs].astype(np.int64)
    s = v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]
    return s[..., 2], s[..., 1], s[..., 0]


def chroma420_raw(px, space, k):
    r, g, b = sums420(px)
    c = TABLE[space][k]
    return (c[0] * r + c[1] * g + c[2] * b + (128 << 18) + (1 << 17)) >> 18


def planes(px, format, space, flags=0):
    """The planes the contract gives for the stored bytes `px` of a rect: [Y, Cb, Cr], or [Y, CbCr (ch, cw, 2)] for NV12, uint8"""
    if flags & FLIP:
        px = px[::-1]
    y = luma(px, space)
    assert y.min() >= 0 and y.max() <= 255
    raw = chroma444_raw if format == I444 else chroma420_raw
    cb, cr = (np.clip(raw(px, space, k), 0, 255) for k in (1, 2))
    out = [y, cb, cr] if format != NV12 else [y, np.stack([cb, cr], axis=-1)]
    return [np.ascontiguousarray(p).astype(np.uint8) for p in out]


def expected(px, format, space, flags=0):
    """The payload of a host-sink grab: the planes, each tight, one after another"""
    return np.concatenate([p.reshape(-1) for p in planes(px, format, space, flags)])


def clamped(px, format, space):
    """How many chroma samples of the expected planes the clamp changed: (below 0, above 255)"""
    raw = chroma444_raw if format == I444 else chroma420_raw
    v = np.concatenate([raw(px, space, k).reshape(-1) for k in (1, 2)])
    return int((v < 0).sum()), int((v > 255).sum())


def row_bytes(w, h, format):
    """-> (rows, bytes per tight row) of each plane"""
    return glapi.yuv_plane_shapes(w, h, format)


class Dest:
    """A device destination: `off` bytes of guard ahead of `dst`, the planes at the given byte strides (0: tight), 48 bytes of guard
    behind the last sample -- all GUARD at first"""

    def __init__(self, gl, w, h, format, off=0, y_stride=0, c_stride=0):
        self.gl, self.w, self.h, self.format = gl, w, h, format
        self.strides = (y_stride, c_stride)
        shapes = row_bytes(w, h, format)
        ys, cs = y_stride or w, c_stride or shapes[1][1]
        # where each plane starts, and the extent: the last plane's last row ends it
        self.layout, at = [], 0
        for k, (rows, row) in enumerate(shapes):
            st = ys if k == 0 else cs
            self.layout.append((at, rows, row, st))
            at += rows * st
        last = self.layout[-1]
        self.extent = last[0] + (last[1] - 1) * last[3] + last[2]
        self.off = off
        self.nbytes = (off + self.extent + 48 + 15) & ~15
        self.base = gl.device_alloc(self.nbytes)
        assert self.base and self.base % 16 == 0, self.base
        gt.fill(gl, self.base, self.nbytes)
        self.dst = self.base + off
        self.dst_bytes = self.extent               # exactly what the planes need: the library may ask for no more

    def image(self, want):
        """The whole buffer as it has to read after the grab: the planes `want` at the contract's addresses, GUARD everywhere else"""
        img = np.full(self.nbytes, GUARD, np.uint8)
        for (at, rows, row, st), p in zip(self.layout, want):
            p = p.reshape(rows, row)
            for r in range(rows):
                a = self.off + at + r * st
                img[a:a + row] = p[r]
        return img

    def read(self):
        return self.gl.device_read(self.base, self.nbytes)

    def check(self, want, what=""):
        got, img = self.read(), self.image(want)
        inside = self.image([np.zeros_like(p) for p in want]) != self.image([np.full_like(p, 0xFF) for p in want])
        bad = got != img
        assert not bad.any(), f"{what}: {int(bad[inside].sum())} bytes of the planes differ, {int(bad[~inside].sum())} bytes outside them were written"

    def untouched(self):
        return bool((self.read() == GUARD).all())

    def free(self):
        self.gl.device_free(self.base)
        self.base = 0


def grab(s, tex, rect, format, space, flags=0, d=None):
    """A YUV grab of `rect` of texture id `tex`, to the host or into the Dest `d`: the ticket"""
    if d is None:
        t = s.gl.grab_texture_yuv(tex, rect, format, space, flags)
    else:
        t = s.gl.grab_texture_yuv(tex, rect, format, space, flags, dst=d.dst, dst_bytes=d.dst_bytes, strides=d.strides)
    assert t >= 0, (t, s.gl.GetError())
    return t


def check_info(info, rect, flags, payload):
    assert (info["status"], info["format"], info["flags"], info["rects"]) == (0, 0x8058, flags | YUV, [tuple(rect)]), info      # GL_RGBA8
    assert (info["scaled_w"], info["scaled_h"], info["levels"]) == (0, 0, 0), info
    assert info["bytes"] == glapi.GRAB_HEADER + payload, info
