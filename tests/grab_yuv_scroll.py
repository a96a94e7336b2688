"""Helpers of tests/test_grab_yuv_scroll.py: the contract of a delta YUV grab with WRHIP_GRAB_SCROLL (include/wrhip.h,
WrhipGrabTextureYuvDelta, `scroll`) restated in numpy on top of tests/grab_yuv.py and tests/grab_scroll.py -- the vote over the LUMA
segments with the candidates a format allows, the classification of the blocks by every plane, the payload's entries and the
in-place decoder over three planes -- independently of the library's kernels and of its codec.  Segment equality is exact here.

Planes are gy.planes' lists: [Y, Cb, Cr], or [Y, CbCr (ch, cw, 2)] for NV12."""
import numpy as np
from webrender_amd import glapi
import frame_grabs as fg
import grab_yuv as gy
import grab_yuv_delta as gd
import grab_scroll as gs
from grab_yuv import I420, NV12, I444

BLOCK, HEADER = fg.BLOCK, fg.HEADER
SAMPLES, COPY = 0, 3
SCROLL = glapi.GRAB_SCROLL
SCROLL_MAX = glapi.GRAB_SCROLL_MAX


def candidate(dy, fmt):
    return dy != 0 and (fmt == I444 or dy % 2 == 0)


def votes(prev, cur, fmt):
    """{dy: votes} over the candidates: gs.votes on the luma planes -- the segments with cur_Y != prev_Y at their own place and
    cur_Y == prev_Y dy rows away"""
    return {dy: n for dy, n in gs.votes(prev[0], cur[0]).items() if candidate(dy, fmt)}


def scroll_dy(prev, cur, fmt):
    v = votes(prev, cur, fmt)
    if not v:
        return 0
    return max(v, key=lambda dy: (v[dy], -abs(dy), dy > 0))


def block_slices(rec, fmt, k, dy=0):
    """The slices of plane k that hold block `rec`'s samples, moved by dy luma rows"""
    x, y, bw, bh = rec
    if k == 0 or fmt == I444:
        return (slice(y + dy, y + dy + bh), slice(x, x + bw))
    return (slice((y + dy) // 2, (y + dy) // 2 + (bh + 1) // 2), slice(x // 2, x // 2 + (bw + 1) // 2))


def classify(prev, cur, fmt):
    """-> (scroll_dy, {record: "same" | "copy" | "send"}) by exact comparison of every plane's samples"""
    h, w = cur[0].shape
    dy = scroll_dy(prev, cur, fmt)
    kinds = {}
    for rec in fg.blocks_of(w, h):
        _, y, _, bh = rec
        same = lambda d: all(np.array_equal(c[block_slices(rec, fmt, k)], p[block_slices(rec, fmt, k, d)]) for k, (c, p) in enumerate(zip(cur, prev)))
        if same(0):
            kinds[rec] = "same"
        elif dy != 0 and 0 <= y + dy and y + dy + bh <= h and same(dy):
            kinds[rec] = "copy"
        else:
            kinds[rec] = "send"
    return dy, kinds


def entry_size(fmt, mode, device):
    return 16 if mode == COPY or device else gd.entry_bytes(fmt, False)


def split(payload, fmt, device=False):
    """A SCROLL payload as it crossed (header first) -> (dy, {record: (mode, the entry's body)})"""
    assert len(payload) >= HEADER and int(np.frombuffer(payload, "<u4", 1)[0]) == len(payload) - HEADER, "the header's count is not the payload's size"
    dy = int(np.frombuffer(payload, "<i4", 1, 4)[0])
    assert bytes(payload[8:16]) == bytes(8)
    out, at = {}, HEADER
    while at < len(payload):
        assert at % 16 == 0 and at + 16 <= len(payload)
        x, y, whm, zero = (int(q) for q in np.frombuffer(payload, "<u4", 4, at))
        w, h, mode = whm & 255, (whm >> 8) & 255, whm >> 16
        assert mode in (SAMPLES, COPY) and zero == 0 and 1 <= w <= BLOCK and 1 <= h <= BLOCK, (x, y, w, h, mode, zero)
        size = entry_size(fmt, mode, device)
        assert at + size <= len(payload) and (x, y, w, h) not in out
        out[(x, y, w, h)] = (mode, payload[at + 16:at + size])
        at += size
    return dy, out


def body_samples(body, rec, fmt):
    """The cut block's samples of a SAMPLES entry's body, plane by plane (no byte beyond them is looked at)"""
    _, _, bw, bh = rec
    b = np.frombuffer(body, np.uint8)
    B = BLOCK
    y = b[:B * B].reshape(B, B)[:bh, :bw]
    if fmt == I444:
        return [y, b[B * B:2 * B * B].reshape(B, B)[:bh, :bw], b[2 * B * B:3 * B * B].reshape(B, B)[:bh, :bw]]
    cw, ch = (bw + 1) // 2, (bh + 1) // 2
    if fmt == NV12:
        return [y, b[B * B:B * B + B * B // 2].reshape(B // 2, B // 2, 2)[:ch, :cw]]
    q = B * B // 4
    return [y, b[B * B:B * B + q].reshape(B // 2, B // 2)[:ch, :cw], b[B * B + q:B * B + 2 * q].reshape(B // 2, B // 2)[:ch, :cw]]


def decode(payload, fmt, planes):
    """Patch a host-sink SCROLL payload into `planes` (writable arrays), in place: the COPY entries first -- by ascending y for
    dy > 0, descending y for dy < 0, every plane's rows in the order that keeps a row's source intact --, then the SAMPLES entries.
    -> (entries, COPY entries)"""
    dy, entries = split(payload, fmt)
    h = planes[0].shape[0]
    copies = sorted((rec for rec, (mode, _) in entries.items() if mode == COPY), key=lambda rec: rec[1], reverse=dy < 0)
    for rec in copies:
        _, y, _, bh = rec
        assert candidate(dy, fmt) and abs(dy) <= SCROLL_MAX and 0 <= y + dy and y + dy + bh <= h
        for k, p in enumerate(planes):
            rows, cols = block_slices(rec, fmt, k)
            d = dy if k == 0 or fmt == I444 else dy // 2
            for r in (range(rows.start, rows.stop) if dy > 0 else range(rows.stop - 1, rows.start - 1, -1)):
                p[r, cols] = p[r + d, cols]
    for rec, (mode, body) in entries.items():
        if mode == SAMPLES:
            for k, (p, v) in enumerate(zip(planes, body_samples(body, rec, fmt))):
                p[block_slices(rec, fmt, k)] = v
    return len(entries), len(copies)


def views(flat, w, h, fmt):
    """Writable plane views of a flat array in a full YUV grab's payload layout"""
    out, at = [], 0
    for k, (rows, row) in enumerate(gy.row_bytes(w, h, fmt)):
        v = flat[at:at + rows * row]
        out.append(v.reshape(rows, row // 2, 2) if fmt == NV12 and k == 1 else v.reshape(rows, row))
        at += rows * row
    return out


def page(rows, w, seed, bands=()):
    """A tall page of stored B, G, R, A noise -- every luma segment of it is unique -- with flat bands (first row, rows, B, G, R)
    mixed in, where all segments are equal"""
    px = gs.page(rows, w, 4, seed)
    for (r0, n, b, g, r) in bands:
        px[r0:r0 + n] = (b, g, r, 255)
    return px
