"""Delta YUV grabs (include/wrhip.h: WrhipGrabTextureYuvDelta, WrhipGrabDecodeYuv): the YUV grab's planes, but only the 64 x 64
blocks whose samples changed since the previous such grab, patched into the consumer's planes on the host or on the card.
Expected planes are tests/grab_yuv.py's numpy restatement applied to the ORACLE's stored bytes; the expected block set is numpy's
comparison of successive plane images (tests/grab_yuv_delta.py).  Everything is 0 differing bytes; destinations are filled with
0xA5 first and compared whole.  Each check runs on the host simulation and, under -m gpu, on the MI355X."""
import ctypes as C
import itertools
import os
import shutil
import subprocess
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref, ROOT
import frame_grabs as fg
import grab_tensor as gt
import grab_yuv as gy
import grab_yuv_delta as gd
from grab_yuv import I420, NV12, I444, FORMATS, SPACES, FLIP, GUARD
from grab_yuv_delta import DELTA, KEY, YUV
from test_grab_scaled import W, H, TW, TH, _noise, _frame
from test_grab_tensor import _oracle_stored
from webrender_amd import glapi, glconst as G, device, scenes
from webrender_amd.renderer import Renderer
from webrender_amd.harness import render_streamed, render_streamed_yuv

FULL = (0, 0, TW, TH)                        # 6 x 4 blocks, the edge ones 13 wide and 9 tall: the chroma clamp is live in them
INNER = (3, 5, 130, 67)                      # odd origin; edge blocks 2 wide and 3 tall
_cache = {}

# what the delta cases do to the texture, one after the other: name, the texture rect written, how
STEPS = [
    ("nothing", None, None),
    ("column 63, row 63", (63, 63, 1, 1), "invert"),
    ("column 64", (64, 63, 1, 1), "invert"),
    ("the last column", (TW - 1, 100, 1, 1), "invert"),
    ("the last row", (150, TH - 1, 1, 1), "invert"),
    ("alpha alone", (10, 10, 150, 100), "alpha"),
    ("four blocks", (120, 60, 16, 10), "noise"),
    ("the first row", (5, 0, 1, 1), "invert"),
    ("the inner rect's corner block", (131, 69, 1, 1), "invert"),
]


def _patched(px, rect, how, seed):
    x, y, w, h = rect
    out = px[y:y + h, x:x + w].copy()
    if how == "invert":
        out[..., :3] = 255 - out[..., :3]
    elif how == "alpha":
        out[..., 3] = 255 - out[..., 3]
    else:
        out = fg.noise(h, w, G.GL_RGBA8, seed)
    return out


def _oracle_steps(ref):
    """The ORACLE's stored bytes of the noise texture after each step: uploaded, patched by TexSubImage2D and read back there.
    Computed once, never modified.  -> (the patches as uploaded, the images)"""
    if (ref, "steps") not in _cache:
        gl = glapi.GL(ref)
        r = Renderer(gl, 64, 64)
        d = r.device
        tex = d.create_texture(TW, TH, G.GL_RGBA8, render_target=True)
        d.upload_texture(tex, 0, 0, TW, TH, G.GL_BGRA, G.GL_UNSIGNED_BYTE, _noise())
        cur = d.read_texture(tex).copy()
        patches, images = [], [cur]
        for k, (name, rect, how) in enumerate(STEPS):
            p = None
            if rect is not None:
                p = _patched(cur, rect, how, 5000 + k)
                d.upload_texture(tex, rect[0], rect[1], rect[2], rect[3], G.GL_BGRA, G.GL_UNSIGNED_BYTE, np.ascontiguousarray(p))
                cur = d.read_texture(tex).copy()
            patches.append(p)
            images.append(cur)
        r.destroy()
        _cache[(ref, "steps")] = (patches, images)
    return _cache[(ref, "steps")]


def _noise_session(lib):
    s = fg.Session(lib, 64, 64)
    tex = s.make(_noise(), G.GL_RGBA8)
    s.r.finish()
    return s, tex


def _geoms(rect, fmt):
    """Device strides: tight, odd, a multiple of 16; dst offsets 1 and 16"""
    w = rect[2]
    crow = gy.row_bytes(w, rect[3], fmt)[1][1]
    return [dict(), dict(off=1, y_stride=w + 3 | 1, c_stride=crow + 2 | 1), dict(off=16, y_stride=(w + 15) // 16 * 16 + 16, c_stride=(crow + 15) // 16 * 16),
            dict(off=1), dict(off=16, y_stride=w + 1)]


# ---------------------------------------------------------------------------- 1. keyframes

def _keyframe(lib, ref, rect):
    px = fg.crop(_oracle_stored(ref)["rgba"], rect)
    s, tex = _noise_session(lib)
    total = set(fg.blocks_of(rect[2], rect[3]))
    combos = list(itertools.product(FORMATS, (0, 3), (0, FLIP), ("host", "device")))
    if rect == FULL:
        combos += [(FORMATS[sp % 3], sp, FLIP if sp % 2 else 0, ("host", "device")[sp // 3]) for sp in SPACES]      # all six spaces once
    for k, (fmt, sp, flags, sink) in enumerate(combos):
        what = f"{rect} fmt {fmt} space {sp} flags {flags} {sink}"
        want = gy.planes(px, fmt, sp, flags)
        c = gd.Consumer(s, rect, fmt, sink, **(_geoms(rect, fmt)[k % 5] if sink == "device" else {}))
        a = s.stats()
        t = c.grab(tex.id, sp, flags, key=True)         # (KEY: two combinations in a row may name the same planes)
        b = s.stats()
        assert b["kernel_launches"] == a["kernel_launches"] + 1 and b["flushes"] == a["flushes"], (what, a, b)
        c.check(t, want, total, True, flags, key=True, what=what)
        if sink == "host":
            # the full YUV grab's planes, and the bytes that crossed: entry i is block i
            full = s.gl.grab_result(gy.grab(s, tex.id, rect, fmt, sp, flags))[1]
            assert np.array_equal(full, c.host), what
            raw = s.gl.grab_payload(t)
            entry = gd.entry_bytes(fmt, False)
            assert len(raw) == fg.HEADER + len(total) * entry and int.from_bytes(raw[:4], "little") == len(total) * entry
            recs = [tuple(np.frombuffer(raw, "<u4", 4, fg.HEADER + i * entry)) for i in range(len(total))]
            assert recs == fg.blocks_of(rect[2], rect[3]), what
            into = np.full_like(c.host, GUARD)
            assert s.gl.grab_decode_yuv(raw, fmt, rect[2], rect[3], into) == (fg.damage_of(total), len(total))
            assert np.array_equal(into, c.host), what
        c.free()
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 2. deltas

DELTA_COMBOS = [(I420, 2, 0, "host", FULL), (NV12, 3, FLIP, "device", FULL), (I444, 0, 0, "device", FULL), (I420, 5, FLIP, "host", INNER),
                (NV12, 1, 0, "host", INNER), (I444, 4, FLIP, "host", FULL), (I420, 0, 0, "device", INNER)]


def _deltas(lib, ref):
    patches, images = _oracle_steps(ref)
    s, tex = _noise_session(lib)
    for n, (fmt, sp, flags, sink, rect) in enumerate(DELTA_COMBOS):
        s.upload(tex, 0, 0, _noise())
        c = gd.Consumer(s, rect, fmt, sink, **(_geoms(rect, fmt)[n % 5] if sink == "device" else {}))
        total = set(fg.blocks_of(rect[2], rect[3]))
        before = gy.planes(fg.crop(images[0], rect), fmt, sp, flags)
        c.check(c.grab(tex.id, sp, flags, key=True), before, total, True, flags, key=True, what=f"combo {n} keyframe")
        partial = 0
        for k, (name, prect, how) in enumerate(STEPS):
            what = f"combo {n} ({fmt}, {sp}, {flags}, {sink}, {rect}) step '{name}'"
            if prect is not None:
                s.upload(tex, prect[0], prect[1], patches[k])
            after = gy.planes(fg.crop(images[k + 1], rect), fmt, sp, flags)
            sent = gd.changed_blocks(before, after, fmt)
            # the precondition, on the numpy side: the changed set is what the case intends
            intent = set() if how in (None, "alpha") else gd.touched_blocks(rect, flags, prect)
            assert sent == intent, (what, sorted(sent), sorted(intent))
            if how == "noise" and rect == FULL and not flags:
                assert len(sent) == 4
            partial += 0 < len(sent) < len(total)
            a = s.stats()
            t = c.grab(tex.id, sp, flags)
            b = s.stats()
            # (one launch; behind an upload the queued rows go out ahead of it, in a launch of their own)
            assert b["kernel_launches"] == a["kernel_launches"] + (1 if prect is None else 2) and b["flushes"] == a["flushes"], (what, a, b)
            c.check(t, after, sent, False, flags, what=what)
            before = after
        assert partial >= 3, (n, partial)
        c.free()
    # the flip: the texture's first row is the image's last one
    assert gd.touched_blocks(FULL, FLIP, (5, 0, 1, 1)) == {(0, 192, 64, 9)} and gd.touched_blocks(FULL, 0, (5, 0, 1, 1)) == {(0, 0, 64, 64)}
    assert gd.touched_blocks(FULL, 0, (63, 63, 1, 1)) == {(0, 0, 64, 64)} and gd.touched_blocks(FULL, 0, (64, 63, 1, 1)) == {(64, 0, 64, 64)}
    assert gd.touched_blocks(FULL, 0, (TW - 1, 100, 1, 1)) == {(320, 64, 13, 64)} and gd.touched_blocks(FULL, 0, (150, TH - 1, 1, 1)) == {(128, 192, 64, 9)}
    assert gd.touched_blocks(INNER, 0, (131, 69, 1, 1)) == {(128, 64, 2, 3)}
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 3. validity of the retained copy

def _validity(lib, ref):
    stored = _oracle_stored(ref)["rgba"]
    s, tex = _noise_session(lib)
    gl = s.gl

    def one(rect, fmt, sp, flags, c, keyframe, key=False, px=stored):
        want = gy.planes(fg.crop(px, rect), fmt, sp, flags)
        sent = set(fg.blocks_of(rect[2], rect[3])) if keyframe else set()
        c.check(c.grab(tex.id, sp, flags, key=key), want, sent, keyframe, flags, key=key, what=f"{rect} {fmt} {sp} {flags} key {key}")
    host = gd.Consumer(s, FULL, I420, "host")
    one(FULL, I420, 2, 0, host, True)
    one(FULL, I420, 2, 0, host, False)
    # another rect, and back
    inner = gd.Consumer(s, INNER, I420, "host")
    one(INNER, I420, 2, 0, inner, True)
    one(INNER, I420, 2, 0, inner, False)
    one(FULL, I420, 2, 0, host, True)
    # another format (planes of one size: the same consumer would do, a fresh one shows every block arriving), space, flip
    nv = gd.Consumer(s, FULL, NV12, "host")
    one(FULL, NV12, 2, 0, nv, True)
    one(FULL, NV12, 2, 0, nv, False)
    one(FULL, NV12, 3, 0, nv, True)
    one(FULL, NV12, 3, 0, nv, False)
    one(FULL, NV12, 3, FLIP, nv, True)
    one(FULL, NV12, 3, FLIP, nv, False)
    # another sink, another destination, another stride
    d1, d2 = gd.Consumer(s, FULL, NV12, "device"), gd.Consumer(s, FULL, NV12, "device", off=16)
    d3 = gd.Consumer(s, FULL, NV12, "device", y_stride=TW + 3)
    one(FULL, NV12, 3, FLIP, d1, True)
    one(FULL, NV12, 3, FLIP, d1, False)
    one(FULL, NV12, 3, FLIP, d2, True)
    one(FULL, NV12, 3, FLIP, d2, False)
    one(FULL, NV12, 3, FLIP, d3, True)
    one(FULL, NV12, 3, FLIP, d3, False)
    one(FULL, NV12, 3, FLIP, nv, True)
    # KEY
    one(FULL, NV12, 3, FLIP, nv, True, key=True)
    one(FULL, NV12, 3, FLIP, nv, False)
    # a plain delta grab and a delta YUV grab of one texture, alternating: neither makes the other a keyframe
    img = np.zeros((TH, TW, 4), np.uint8)
    fg.check_delta(gl, gl.grab_texture(tex.id, FULL, DELTA), img, stored, fg.blocks_of(TW, TH), keyframe=True)
    for _ in range(2):
        one(FULL, NV12, 3, FLIP, nv, False)
        fg.check_delta(gl, gl.grab_texture(tex.id, FULL, DELTA), img, stored, [], keyframe=False)
    # new storage of the same size, the same bytes uploaded again: a keyframe
    gl.ActiveTexture(G.GL_TEXTURE0)
    gl.BindTexture(G.GL_TEXTURE_2D, tex.id)
    gl.TexStorage2D(G.GL_TEXTURE_2D, 1, G.GL_RGBA8, TW, TH)
    s.upload(tex, 0, 0, _noise())
    one(FULL, NV12, 3, FLIP, nv, True)
    one(FULL, NV12, 3, FLIP, nv, False)
    for c in (d1, d2, d3):
        c.free()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 4. ordering

def _later_upload(lib, ref):
    """A grab, then an upload over the rect: the grab is unchanged, and the next one sends what the upload changed"""
    stored = _oracle_stored(ref)["rgba"]
    s, tex = _noise_session(lib)
    h, d = gd.Consumer(s, INNER, NV12, "host"), gd.Consumer(s, FULL, I420, "device")
    th = h.grab(tex.id, 3)
    s.upload(tex, 0, 0, fg.noise(60, 80, G.GL_RGBA8, 78))
    h.check(th, gy.planes(fg.crop(stored, INNER), NV12, 3), set(fg.blocks_of(*INNER[2:])), True, what="host grab ahead of an upload")
    s.upload(tex, 0, 0, _noise())
    td = d.grab(tex.id, 0, FLIP)
    s.upload(tex, 0, 0, fg.noise(60, 80, G.GL_RGBA8, 78))
    d.check(td, gy.planes(stored, I420, 0, FLIP), set(fg.blocks_of(TW, TH)), True, FLIP, what="device grab ahead of an upload")
    for c in (h, d):
        c.free()
    assert s.gl.GetError() == 0
    s.close()


def _rendered_frame(lib, ref):
    """The window behind its held-back launches, no Finish: the grabs are parked; a later write to the window is not seen by them
    and is what the next grab sends"""
    px = _oracle_stored(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    rect = (0, 0, W, H)
    total = set(fg.blocks_of(W, H))
    win = device.Texture(s.window, W, H, G.GL_RGBA8)
    for sink, fmt, sp in (("host", I420, 2), ("device", NV12, 5)):
        s.r.render(_frame())
        c = gd.Consumer(s, rect, fmt, sink)
        t = c.grab(s.window, sp)                        # (submits what was recorded; the frame's raster launches stay held back)
        assert s.gl.grab_result(t, wait=False) is None  # parked
        patch = fg.noise(40, 70, G.GL_RGBA8, 77)
        s.upload(win, 100, 60, patch)
        want = gy.planes(px, fmt, sp)
        c.check(t, want, total, True, what=f"rendered frame, {sink}")
        after = px.copy()
        after[60:100, 100:170] = patch
        want2 = gy.planes(after, fmt, sp)
        sent = gd.changed_blocks(want, want2, fmt)
        assert sent == gd.touched_blocks(rect, 0, (100, 60, 70, 40)) and 0 < len(sent) < len(total)
        c.check(c.grab(s.window, sp), want2, sent, False, what=f"the upload over the frame, {sink}")
        # the same frame once more: the grab is parked behind it and finds the frame's own bytes again -- the patch's blocks
        s.r.render(_frame())
        t = c.grab(s.window, sp)
        assert s.gl.grab_result(t, wait=False) is None
        c.check(t, want, sent, False, what=f"the frame again, {sink}")
        s.r.finish()
        c.free()
    assert s.gl.GetError() == 0
    s.close()


def _ring(lib, ref):
    """Nine grabs against the ring of 8, parked and not.  Host sink, parked: the first is dropped with its ticket, so the second is
    the keyframe.  Device sink: all nine are issued; planes and retained copy stay consistent."""
    px = _oracle_stored(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    gl = s.gl
    rect = (0, 0, W, H)
    total = set(fg.blocks_of(W, H))
    win = device.Texture(s.window, W, H, G.GL_RGBA8)
    out = glapi.WrhipGrabInfo()
    for sink, fmt, sp in (("host", NV12, 1), ("device", I420, 4)):
        want = gy.planes(px, fmt, sp)
        for parked in (True, False):
            c = gd.Consumer(s, rect, fmt, sink)
            if parked:
                s.r.render(_frame())
            tickets = [c.grab(s.window, sp, key=(k == 0)) for k in range(9)]
            assert len(set(tickets)) == 9
            if parked:
                assert all(gl.WrhipGrabResultGet(t, C.byref(out), None, 0, 0) == 1 for t in tickets[1:])
            assert gl.WrhipGrabResultGet(tickets[0], C.byref(out), None, 0, 1) == -1
            if parked:
                gt.send_held(gl)
            # host, parked: grab 0 never ran, grab 1 sends every block in its place.  Otherwise grab 0 ran, ticket or not
            second_key = sink == "host" and parked
            if sink == "host" and not parked:
                c.host[:] = gd.flat(want)               # (the dead ticket carried the keyframe's blocks: a consumer would ask for KEY)
            c.check(tickets[1], want, total if second_key else set(), second_key, what=f"{sink} parked {parked} grab 1")
            for k in range(2, 9):
                c.check(tickets[k], want, set(), False, what=f"{sink} parked {parked} grab {k}")
            # the retained copy is the window's planes: an upload is sent as its blocks alone
            patch = fg.noise(30, 50, G.GL_RGBA8, 91)
            s.upload(win, 200, 130, patch)
            after = px.copy()
            after[130:160, 200:250] = patch
            want2 = gy.planes(after, fmt, sp)
            sent = gd.changed_blocks(want, want2, fmt)
            assert 0 < len(sent) < len(total)
            c.check(c.grab(s.window, sp), want2, sent, False, what=f"{sink} parked {parked} after the nine")
            s.r.finish()
            s.upload(win, 200, 130, np.ascontiguousarray(px[130:160, 200:250]))
            c.free()
    assert gl.GetError() == 0
    s.close()


def _put_from_parked(lib, ref):
    """A put that reads a parked device grab's destination sees the grab's bytes"""
    px = _oracle_stored(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    gl = s.gl
    rect = (5, 6, 64, 32)
    r8 = s.d.create_texture(64, 32, G.GL_R8, render_target=True)
    s.upload(r8, 0, 0, np.zeros((32, 64), np.uint8))
    s.r.finish()
    s.r.render(_frame())
    c = gd.Consumer(s, rect, I444, "device")
    t = c.grab(s.window, 3)
    assert gl.grab_result(t, wait=False) is None
    assert gl.put_texture_tensor(r8.id, (0, 0, 64, 32), c.d.dst, 64 * 32, dtype=gt.U8, layout=gt.CHW, channels=1) == 0
    want = gy.planes(fg.crop(px, rect), I444, 3)
    assert np.array_equal(s.d.read_texture(r8), want[0])
    c.check(t, want, {(0, 0, 64, 32)}, True, what="the grab a put read from")
    c.free()
    s.r.finish()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 5. streamed

STREAM_RECTS = (6, 6, 7, 8, 8, 9, 10, 11, 11, 12)          # ten frames: how many of the twelve rects each draws


def _stream_frame(m):
    """A mostly still page: the first `m` of twelve small translucent rects over white -- one more rect changes a few blocks"""
    rng, rects = scenes.random_rects(12, W, H, 32, 160, 40)
    rgba = np.concatenate([rng.integers(0, 256, size=(12, 3), dtype=np.uint8), np.full((12, 1), 160, np.uint8)], axis=1)
    return scenes.build_rect_frame(W, H, rects[:m], scenes.premultiply(rgba[:m]), np.zeros(m, bool), "brush")


def _oracle_stream(ref):
    """The oracle's render of every distinct frame of the stream: computed once, never modified"""
    if (ref, "stream") not in _cache:
        gl = glapi.GL(ref)
        r = Renderer(gl, W, H)
        out = {}
        for m in sorted(set(STREAM_RECTS)):
            r.render(_stream_frame(m))
            r.finish()
            out[m] = r.device.read_texture(device.Texture(0, W, H, G.GL_RGBA8, fbo=0)).copy()
        r.destroy()
        _cache[(ref, "stream")] = out
    return _cache[(ref, "stream")]


def _stream(lib, ref):
    seeds = list(STREAM_RECTS)
    frames = lambda: [_stream_frame(m) for m in seeds]
    _, plain = render_streamed(lib, frames())
    want = _oracle_stream(ref)
    for dev, fmt, sp in ((False, I420, 2), (True, NV12, 1)):
        planes, st, infos = render_streamed_yuv(lib, frames(), fmt, sp, device=dev, delta=True)
        assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
        assert st["setup_carried"] == plain["setup_carried"] and st["setup_carried"] >= len(seeds) - 1, (st, plain)
        assert len(planes) == len(infos) == len(seeds) == 10
        bad = [k for k, sd in enumerate(seeds) if not all(np.array_equal(a, b) for a, b in zip(planes[k], gy.planes(want[sd], fmt, sp)))]
        assert not bad, f"frames whose accumulated planes are not the restatement on the oracle's render: {bad}"
        prev = None
        for k, sd in enumerate(seeds):
            cur = gy.planes(want[sd], fmt, sp)
            sent = set(fg.blocks_of(W, H)) if prev is None else gd.changed_blocks(prev, cur, fmt)
            gd.check_info(infos[k], (0, 0, W, H), fmt, 0, dev, sent, prev is None)
            prev = cur
        assert any(0 < i["blocks"] < i["blocks_total"] for i in infos), [i["blocks"] for i in infos]
        assert [infos[k]["blocks"] for k in (1, 4, 8)] == [0, 0, 0]          # (the same frame again)
    # key_every: the keyframes are where they were asked for
    _, _, infos = render_streamed_yuv(lib, frames()[:4], I420, 2, delta=True, key_every=2)
    assert [(i["keyframe"], bool(i["flags"] & KEY)) for i in infos] == [(1, True), (0, False), (1, True), (0, False)]


# ---------------------------------------------------------------------------- 6. the contract's rejections

def _contract(lib):
    s = fg.Session(lib, W, H)
    gl = s.gl
    s.r.render(_frame())
    s.r.finish()
    r8 = s.make(fg.noise(37, 61, G.GL_R8, 611), G.GL_R8)
    f32 = s.d.create_texture(8, 8, G.GL_RGBA32F)
    s.r.finish()
    assert gl.GetError() == 0
    win = s.window
    size = 1 << 16
    buf = gl.device_alloc(size)
    gt.fill(gl, buf, size)
    good = dict(tex=win, rect=(0, 0, 64, 32), fmt=I420, sp=0, flags=0, dst=buf, dst_bytes=64 * 32 * 3 // 2, strides=(0, 0), key=0)

    def call(**kw):
        a = dict(good, **kw)
        return gl.grab_texture_yuv_delta(a["tex"], a["rect"], a["fmt"], a["sp"], a["flags"], dst=a["dst"], dst_bytes=a["dst_bytes"], strides=a["strides"], key=a["key"])
    # a retained copy to be left as it was
    t0 = call()
    assert t0 >= 0 and gl.grab_result(t0)[0]["keyframe"] == 1
    n0, f0 = s.stats()["kernel_launches"], s.stats()["flushes"]
    rect4 = (C.c_int32 * 4)(0, 0, 64, 32)
    bad = [
        lambda: call(tex=9999),
        lambda: call(tex=f32.id, rect=(0, 0, 8, 8)), lambda: call(tex=r8.id, rect=(0, 0, 8, 8)),
        lambda: call(rect=(0, 0, 0, 4)), lambda: call(rect=(0, 0, 4, 0)),
        lambda: call(rect=(500, 0, 13, 1)), lambda: call(rect=(0, -1, 4, 4)), lambda: call(rect=(0, 500, 4, 13)),
        lambda: call(fmt=3), lambda: call(sp=6), lambda: call(sp=7),
        lambda: call(flags=glapi.GRAB_SWAP_RB), lambda: call(flags=DELTA), lambda: call(flags=YUV), lambda: call(flags=glapi.GRAB_TENSOR), lambda: call(flags=KEY),
        lambda: gl.WrhipGrabTextureYuvDelta(win, C.addressof(rect4), None, 0),
        lambda: call(dst=None, strides=(64, 0)), lambda: call(dst=None, strides=(0, 32)), lambda: call(dst=None, dst_bytes=1),
        lambda: call(strides=(63, 0)), lambda: call(strides=(0, 31)), lambda: call(strides=(-64, 0)),
        lambda: call(fmt=NV12, strides=(0, 63)), lambda: call(fmt=I444, strides=(0, 63)),
        lambda: call(strides=((1 << 40) + 1, 0), dst_bytes=1 << 62), lambda: call(strides=(0, (1 << 40) + 1), dst_bytes=1 << 62),
        lambda: call(dst_bytes=64 * 32 * 3 // 2 - 1),
        lambda: call(fmt=I444, dst_bytes=64 * 32 * 3 - 1),
        lambda: call(strides=(80, 40), dst_bytes=32 * 80 + 31 * 40 + 32 - 1),
    ] + [(lambda bit=bit: call(key=bit)) for bit in (1, 2, 4, 16, 32, 64, 128, 256, 512, 1 << 31, KEY | 1)]      # any flags bit but KEY
    for k, c in enumerate(bad):
        assert c() == -1, k
        assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0, k
    gl.WrhipSetShard(0, 2)
    assert call() == -1 and gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    gl.WrhipSetShard(0, 1)
    gl.WrhipSetTargetRows(win, 0, 256)
    assert call() == -1 and gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    gl.WrhipSetTargetRows(win, 0, 0)
    assert s.stats()["kernel_launches"] == n0 and s.stats()["flushes"] == f0
    # the retained copy is as it was: the good call again sends nothing
    t1 = call()
    info = gl.grab_result(t1)[0]
    assert (info["keyframe"], info["blocks"], info["bytes"]) == (0, 0, 16), info
    assert s.stats()["kernel_launches"] == n0 + 1 and gl.GetError() == 0
    # a host-sink ticket delivers into tight planes: a dst_stride is rejected
    t = call(dst=None, dst_bytes=0)
    host = np.full(64 * 32 * 3 // 2, GUARD, np.uint8)
    out = glapi.WrhipGrabInfo()
    assert gl.WrhipGrabResultGet(t, C.byref(out), host.ctypes.data, 64, 1) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert (host == GUARD).all()
    assert gl.WrhipGrabResultGet(t, C.byref(out), host.ctypes.data, 0, 1) == 0 and out.bytes == fg.HEADER + gd.entry_bytes(I420, False)
    assert not (host == GUARD).all()
    gl.device_free(buf)
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 7. the decoder; the kernel's notes (CPU only)

def _decode_cases(lib):
    """WrhipGrabDecodeYuv through ctypes on payloads made here: good ones patch exactly their blocks, hostile ones write nothing"""
    gl = glapi.GL(lib)
    rng = np.random.default_rng(5)
    w, h = 130, 67
    for fmt in FORMATS:
        entry = gd.entry_bytes(fmt, False)
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        planes = gy.planes(img, fmt, 3)
        blocks = fg.blocks_of(w, h)

        def body(rec):
            x, y, bw, bh = rec
            e = rng.integers(0, 256, entry, dtype=np.uint8)            # (bytes beyond the cut block: anything)
            e[:16] = np.array(rec, "<u4").view(np.uint8)
            yv = e[16:16 + 4096].reshape(64, 64)
            yv[:bh, :bw] = planes[0][y:y + bh, x:x + bw]
            if fmt == I444:
                for k in (1, 2):
                    e[16 + 4096 * k:16 + 4096 * (k + 1)].reshape(64, 64)[:bh, :bw] = planes[k][y:y + bh, x:x + bw]
            elif fmt == NV12:
                cw, ch = (bw + 1) // 2, (bh + 1) // 2
                e[16 + 4096:].reshape(32, 32, 2)[:ch, :cw] = planes[1][y // 2:y // 2 + ch, x // 2:x // 2 + cw]
            else:
                cw, ch = (bw + 1) // 2, (bh + 1) // 2
                for k in (1, 2):
                    e[16 + 4096 + 1024 * (k - 1):16 + 4096 + 1024 * k].reshape(32, 32)[:ch, :cw] = planes[k][y // 2:y // 2 + ch, x // 2:x // 2 + cw]
            return e

        def payload(entries, count=None):
            p = np.concatenate([np.zeros(16, np.uint8)] + entries) if entries else np.zeros(16, np.uint8)
            p[:4] = np.array([len(p) - 16 if count is None else count], "<u4").view(np.uint8)
            return p.tobytes()
        flatp = gd.flat(planes)
        into = np.full_like(flatp, GUARD)
        order = [blocks[i] for i in (5, 0, 3, 1, 4, 2)]                   # (the order of the entries is free)
        assert gl.grab_decode_yuv(payload([body(r) for r in order]), fmt, w, h, into) == ((0, 0, w, h), 6)
        assert np.array_equal(into, flatp), fmt
        # one block: nothing else is touched; check-only mode writes nothing and reports the same
        into = np.full_like(flatp, GUARD)
        one = payload([body(blocks[5])])
        assert gl.grab_decode_yuv(one, fmt, w, h, None) == ((128, 64, 2, 3), 1)
        assert gl.grab_decode_yuv(one, fmt, w, h, into) == ((128, 64, 2, 3), 1)
        probe =[np.zeros_like(p) for p in planes]
        probe[0][64:67, 128:130] = 1
        if fmt == I444:
            probe[1][64:67, 128:130] = probe[2][64:67, 128:130] = 1
        else:
            for p in probe[1:]:
                p[32:34, 64:65] = 1
        mask = gd.flat(probe).astype(bool)
        assert np.array_equal(into[mask], flatp[mask]) and (into[~mask] == GUARD).all(), fmt
        assert gl.grab_decode_yuv(payload([]), fmt, w, h, into) == ((0, 0, 0, 0), 0)
        # hostile
        good = body(blocks[0])

        def rec(x, y, bw, bh):
            e = good.copy()
            e[:16] = np.array([x, y, bw, bh], "<u4").view(np.uint8)
            return e
        hostile = {
            "truncated": payload([good])[:-1],
            "a count larger than what is held": payload([good], count=2 * entry),
            "a count that is not k entries": payload([good], count=entry - 16),
            "fewer bytes than a header": payload([])[:15],
            "a misaligned x": payload([rec(32, 0, 64, 64)]), "a misaligned y": payload([rec(0, 1, 64, 64)]),
            "x outside": payload([rec(192, 0, 64, 64)]), "y outside": payload([rec(0, 128, 64, 64)]),
            "a negative x": payload([rec(0xFFFFFFC0, 0, 64, 64)]),
            "a wrong w": payload([rec(128, 0, 64, 64)]), "a wrong h": payload([rec(0, 64, 64, 64)]), "w of 0": payload([rec(0, 0, 0, 64)]),
            "a cut block where a whole one is": payload([rec(0, 0, 2, 3)]),
            "too many entries": payload([body(blocks[i % 6]) for i in range(7)]),
            "a good entry ahead of a bad one": payload([good, rec(32, 0, 64, 64)]),
        }
        for name, p in hostile.items():
            into = np.full_like(flatp, GUARD)
            for target in (into, None):
                with pytest.raises(ValueError):
                    gl.grab_decode_yuv(p, fmt, w, h, target)
            assert (into == GUARD).all(), (fmt, name)
    # planes given in part, a stride below a row, an unknown format
    p = np.zeros(16, np.uint8)
    buf = np.zeros(130 * 67 * 3, np.uint8)
    a = buf.ctypes.data
    dec = lambda fmt, y, ys, c0, c1, cs: gl.WrhipGrabDecodeYuv(p.ctypes.data, 16, fmt, 130, 67, y, ys, c0, c1, cs, None, None)
    assert dec(0, a, 0, a, a, 0) == 0 and dec(1, a, 0, a, None, 0) == 0 and dec(2, None, 0, None, None, 0) == 0
    assert dec(0, a, 0, a, None, 0) == -1 and dec(0, None, 0, a, a, 0) == -1 and dec(1, a, 0, a, a, 0) == -1
    assert dec(0, a, 129, a, a, 0) == -1 and dec(0, a, 0, a, a, 64) == -1 and dec(1, a, 0, a, None, 129) == -1 and dec(3, a, 0, a, a, 0) == -1


def test_decoder_on_hostile_input(tmp_path):
    """tools/grab_yuv_codec_check.cpp -- wr_grab_codec.h alone, its own main -- under AddressSanitizer and UBSan, as a process of its own"""
    cxx = shutil.which("g++")
    flags = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    trivial = tmp_path / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    if cxx is None or subprocess.run([cxx] + flags + [str(trivial), "-o", str(tmp_path / "trivial")], capture_output=True).returncode != 0:
        pytest.skip("no g++ that links with -fsanitize=address,undefined")
    exe = tmp_path / "grab_yuv_codec_check"
    subprocess.run([cxx] + flags + ["-I", os.path.join(ROOT, "webrender_amd", "csrc"), os.path.join(ROOT, "tools", "grab_yuv_codec_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "grab_yuv_codec_check: ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_yuv_delta_kernel_has_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    assert "wr_grab_yuv_delta_kernel" in notes, sorted(notes)
    vgprs, scratch = notes["wr_grab_yuv_delta_kernel"]
    print("wr_grab_yuv_delta_kernel:", vgprs, "VGPRs,", scratch, "bytes of private segment")
    assert scratch == 0, (vgprs, scratch)


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("rect", [FULL, INNER], ids=["full", "inner"])
def test_hostsim_keyframe(hostsim, oracle_gcc, rect):
    _keyframe(hostsim, oracle_gcc, rect)


def test_hostsim_deltas(hostsim, oracle_gcc):
    _deltas(hostsim, oracle_gcc)


def test_hostsim_validity(hostsim, oracle_gcc):
    _validity(hostsim, oracle_gcc)


def test_hostsim_later_upload(hostsim, oracle_gcc):
    _later_upload(hostsim, oracle_gcc)


def test_hostsim_rendered_frame(hostsim, oracle_gcc):
    _rendered_frame(hostsim, oracle_gcc)


def test_hostsim_ring(hostsim, oracle_gcc):
    _ring(hostsim, oracle_gcc)


def test_hostsim_put_from_parked(hostsim, oracle_gcc):
    _put_from_parked(hostsim, oracle_gcc)


def test_hostsim_stream(hostsim, oracle_gcc):
    _stream(hostsim, oracle_gcc)


def test_hostsim_contract(hostsim):
    _contract(hostsim)


def test_hostsim_decode(hostsim):
    _decode_cases(hostsim)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("rect", [FULL, INNER], ids=["full", "inner"])
def test_gpu_keyframe(rect):
    _keyframe(wrhip_lib(), _gpu_ref(), rect)


@pytest.mark.gpu
def test_gpu_deltas():
    _deltas(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_validity():
    _validity(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_later_upload():
    _later_upload(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_rendered_frame():
    _rendered_frame(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_ring():
    _ring(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_put_from_parked():
    _put_from_parked(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_stream():
    _stream(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_contract():
    _gpu_ref()
    _contract(wrhip_lib())
