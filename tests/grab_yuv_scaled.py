"""Helpers of tests/test_grab_yuv_scaled.py: the chain of include/wrhip.h (WrhipGrabTextureYuvScaled) issued as the BlitFramebuffer
calls it is defined by, on whatever backend the session runs -- tests/grab_scaled.py's blit_chain, but EVERY level is kept --, the
planes of level k through tests/grab_yuv.py's restatement, and a destination in device memory that holds all renditions of a grab in
ONE buffer, filled with the guard byte first and compared whole afterwards.  Nothing here has a tolerance."""
import numpy as np
from webrender_amd import glapi, glconst as G
import grab_tensor as gt
import grab_yuv as gy
from grab_scaled import levels_of

GUARD = gy.GUARD
FLIP, YUV, SCALED = glapi.GRAB_FLIP_ROWS, glapi.GRAB_YUV, glapi.GRAB_SCALED


def blit_levels(gl, d, tex, rect, size):
    """Levels 0 .. L of the chain, stored bytes (B, G, R, A): `rect` of `tex` (a device.Texture with an fbo) blitted GL_LINEAR to
    level L at the origin, then level k + 1 to level k for every k < L, each level a render-target texture of its own, all of them
    read back: the list, level k at index k.  `d`: the session's Device."""
    x, y, w, h = rect
    dw, dh = size
    L = levels_of(w, dw)
    levels = [d.create_texture(dw << k, dh << k, G.GL_RGBA8, render_target=True) for k in range(L + 1)]

    def blit(src, s, dst, dd):
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, src.fbo)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, dst.fbo)
        gl.BlitFramebuffer(s[0], s[1], s[2], s[3], dd[0], dd[1], dd[2], dd[3], G.GL_COLOR_BUFFER_BIT, G.GL_LINEAR)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, 0)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)
    blit(tex, (x, y, x + w, y + h), levels[L], (0, 0, dw << L, dh << L))
    for k in range(L - 1, -1, -1):
        blit(levels[k + 1], (0, 0, dw << (k + 1), dh << (k + 1)), levels[k], (0, 0, dw << k, dh << k))
    out = [d.read_texture(t).copy() for t in levels]
    for t in levels:
        d.delete_texture(t)
    return out


def planes(levels, n, format, space, flags=0):
    """The renditions the contract gives: gy.planes of level k for k < n"""
    return [gy.planes(levels[k], format, space, flags) for k in range(n)]


def expected(levels, n, format, space, flags=0):
    """The payload of a host-sink grab: rendition 0's planes, then rendition 1's, ..., each tight"""
    return np.concatenate([p.reshape(-1) for r in planes(levels, n, format, space, flags) for p in r])


def launches(L, size, format, flags):
    """The header's cost rule: 1 + L / 4, and one more for FLIP_ROWS with a 4:2:0 format and an odd out_h"""
    return 1 + L // 4 + (1 if (flags & FLIP) and format != gy.I444 and size[1] % 2 == 1 else 0)


class Ladder:
    """One device buffer for all renditions of a grab of `size` x `n`: `off` bytes of guard ahead of rendition 0, each rendition's
    planes at its byte strides (geoms[k]: dict of y_stride / c_stride, 0 or absent: tight), `gap` bytes of guard between one
    rendition's last sample and the next one's first, 48 bytes of guard behind the last -- all GUARD at first"""

    def __init__(self, gl, size, n, format, off=0, gap=0, geoms=None):
        self.gl, self.n, self.format = gl, n, format
        geoms = geoms or [{}] * n
        self.rend, at = [], off
        for k in range(n):
            w, h = size[0] << k, size[1] << k
            shapes = gy.row_bytes(w, h, format)
            ys, cs = geoms[k].get("y_stride", 0), geoms[k].get("c_stride", 0)
            layout, p = [], 0
            for i, (rows, row) in enumerate(shapes):
                st = (ys or w) if i == 0 else (cs or shapes[1][1])
                layout.append((p, rows, row, st))
                p += rows * st
            last = layout[-1]
            extent = last[0] + (last[1] - 1) * last[3] + last[2]
            self.rend.append({"at": at, "layout": layout, "extent": extent, "strides": (ys, cs)})
            at += extent + gap
        self.nbytes = (at + 48 + 15) & ~15
        self.base = gl.device_alloc(self.nbytes)
        assert self.base and self.base % 16 == 0, self.base
        gt.fill(gl, self.base, self.nbytes)

    def dsts(self, short=None):
        """(address, dst_bytes) per rendition: exactly the extent -- the library may ask for no more; short=k: rendition k a byte less"""
        return [(self.base + r["at"], r["extent"] - (1 if short == k else 0)) for k, r in enumerate(self.rend)]

    def strides(self):
        return [r["strides"] for r in self.rend]

    def image(self, want):
        img = np.full(self.nbytes, GUARD, np.uint8)
        for r, pl in zip(self.rend, want):
            for (at, rows, row, st), p in zip(r["layout"], pl):
                p = p.reshape(rows, row)
                for y in range(rows):
                    a = r["at"] + at + y * st
                    img[a:a + row] = p[y]
        return img

    def read(self):
        return self.gl.device_read(self.base, self.nbytes)

    def check(self, want, what=""):
        got, img = self.read(), self.image(want)
        inside = self.image([[np.zeros_like(p) for p in pl] for pl in want]) != self.image([[np.full_like(p, 0xFF) for p in pl] for pl in want])
        bad = got != img
        assert not bad.any(), f"{what}: {int(bad[inside].sum())} bytes of the planes differ, {int(bad[~inside].sum())} bytes outside them were written"

    def untouched(self):
        return bool((self.read() == GUARD).all())

    def free(self):
        self.gl.device_free(self.base)
        self.base = 0


def grab(s, tex, rect, size, n, format, space, flags=0, d=None):
    """A scaled YUV grab of `rect` of texture id `tex` to `size` with n renditions, to the host or into the Ladder `d`: the ticket"""
    if d is None:
        t = s.gl.grab_texture_yuv_scaled(tex, rect, size, format, space, flags, renditions=n)
    else:
        t = s.gl.grab_texture_yuv_scaled(tex, rect, size, format, space, flags, renditions=n, dsts=d.dsts(), strides=d.strides())
    assert t >= 0, (t, s.gl.GetError())
    return t


def check_info(info, rect, size, L, n, flags, payload):
    assert (info["status"], info["format"], info["flags"], info["rects"]) == (0, G.GL_RGBA8, flags | YUV | SCALED, [tuple(rect)]), info
    assert (info["scaled_w"], info["scaled_h"], info["levels"], info["renditions"]) == (size[0], size[1], L, n), info
    assert info["bytes"] == glapi.GRAB_HEADER + payload, info
