"""Helpers of tests/test_grab_yuv_delta.py: the contract of a delta YUV grab (include/wrhip.h, WrhipGrabTextureYuvDelta) restated in
numpy on top of tests/grab_yuv.py -- which 64 x 64 blocks of two successive plane images differ, what a ticket has to report, and
the two kinds of planes a consumer keeps: a flat host array and a device destination, both filled with a guard byte first and
compared WHOLE.  Nothing here has a tolerance."""
import numpy as np
from webrender_amd import glapi
import frame_grabs as fg
import grab_yuv as gy
from grab_yuv import I420, NV12, I444, FLIP, GUARD

BLOCK = fg.BLOCK
DELTA, KEY, YUV = glapi.GRAB_DELTA, glapi.GRAB_KEY, glapi.GRAB_YUV


def entry_bytes(fmt, device):
    """One sent block: a 16-byte record, and on the host sink Y (64 x 64) and the chroma at their fixed pitches"""
    if device:
        return 16
    return 16 + (3 * BLOCK * BLOCK if fmt == I444 else BLOCK * BLOCK * 3 // 2)


def changed_blocks(a, b, fmt):
    """The records (x, y, w, h in luma samples) of the blocks in which any SAMPLE of the plane lists `a` and `b` (gy.planes' of one
    image size) differs: numpy's comparison of two successive plane images"""
    h, w = a[0].shape
    out = set()
    for (x, y, bw, bh) in fg.blocks_of(w, h):
        diff = np.any(a[0][y:y + bh, x:x + bw] != b[0][y:y + bh, x:x + bw])
        for pa, pb in zip(a[1:], b[1:]):
            if fmt == I444:
                diff = diff or np.any(pa[y:y + bh, x:x + bw] != pb[y:y + bh, x:x + bw])
            else:                                   # (ch, cw) samples, or (ch, cw, 2) pairs: the block's (bh + 1) / 2 x (bw + 1) / 2
                sl = (slice(y // 2, y // 2 + (bh + 1) // 2), slice(x // 2, x // 2 + (bw + 1) // 2))
                diff = diff or np.any(pa[sl] != pb[sl])
        if diff:
            out.add((x, y, bw, bh))
    return out


def touched_blocks(rect, flags, patch):
    """The records of the blocks of the image of `rect` that own a pixel of the texture rect `patch` (x, y, w, h): geometry alone --
    the flip counted in, rows from the flipped image's top"""
    rx, ry, w, h = rect
    x0, y0 = max(patch[0], rx) - rx, max(patch[1], ry) - ry
    x1, y1 = min(patch[0] + patch[2], rx + w) - rx, min(patch[1] + patch[3], ry + h) - ry
    if x1 <= x0 or y1 <= y0:
        return set()
    if flags & FLIP:
        y0, y1 = h - y1, h - y0
    return {(x, y, bw, bh) for (x, y, bw, bh) in fg.blocks_of(w, h) if x < x1 and x0 < x + bw and y < y1 and y0 < y + bh}


def flat(planes):
    return np.concatenate([p.reshape(-1) for p in planes])


def grab(s, tex, rect, fmt, sp, flags=0, d=None, key=False):
    """A delta YUV grab of `rect` of texture id `tex`, to the host or into the Dest `d`: the ticket"""
    if d is None:
        t = s.gl.grab_texture_yuv_delta(tex, rect, fmt, sp, flags, key=key)
    else:
        t = s.gl.grab_texture_yuv_delta(tex, rect, fmt, sp, flags, dst=d.dst, dst_bytes=d.dst_bytes, strides=d.strides, key=key)
    assert t >= 0, (t, s.gl.GetError())
    return t


def check_info(info, rect, fmt, flags, device, sent, keyframe, key=False):
    w, h = rect[2:]
    assert (info["status"], info["format"], info["rects"]) == (0, 0x8058, [tuple(rect)]), info      # GL_RGBA8
    assert info["flags"] == (flags | YUV | DELTA | (KEY if key else 0)), info
    assert (info["scaled_w"], info["scaled_h"], info["levels"]) == (0, 0, 0), info
    assert info["keyframe"] == (1 if keyframe else 0), info
    assert info["blocks_total"] == len(fg.blocks_of(w, h)), info
    assert info["blocks"] == len(sent), (info, sorted(sent))
    assert tuple(info["damage"]) == fg.damage_of(sent), (info, fg.damage_of(sent))
    assert info["bytes"] == fg.HEADER + len(sent) * entry_bytes(fmt, device), info


class Consumer:
    """The planes a consumer keeps across the grabs of one rect: a flat host array (sink "host") or a gy.Dest in device memory,
    GUARD at first.  `have`: what they have to hold, GUARD where no block has been sent yet."""

    def __init__(self, s, rect, fmt, sink, **geom):
        self.s, self.rect, self.fmt, self.sink = s, tuple(rect), fmt, sink
        w, h = rect[2:]
        self.d = gy.Dest(s.gl, w, h, fmt, **geom) if sink == "device" else None
        self.host = np.full(sum(rows * row for rows, row in gy.row_bytes(w, h, fmt)), GUARD, np.uint8)

    def grab(self, tex, sp, flags=0, key=False):
        return grab(self.s, tex, self.rect, self.fmt, sp, flags, self.d, key)

    def check(self, ticket, want, sent, keyframe, flags=0, key=False, what=""):
        """The ticket's info, and the planes after it, compared whole with `want` (gy.planes' list: every block has been sent by now)"""
        info, out = self.s.gl.grab_result(ticket, into=self.host)
        assert out is self.host
        check_info(info, self.rect, self.fmt, flags, self.d is not None, sent, keyframe, key)
        if self.d is None:
            bad = int((self.host != flat(want)).sum())
            assert bad == 0, f"{what}: {bad} bytes of the patched planes differ"
        else:
            assert (self.host == GUARD).all(), f"{what}: a device sink's ticket wrote the host planes"
            self.d.check(want, what)
        return info

    def free(self):
        if self.d is not None:
            self.d.free()
