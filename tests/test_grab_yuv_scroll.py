"""Scroll-aware delta YUV grabs (include/wrhip.h: WrhipGrabTextureYuvDelta with WRHIP_GRAB_SCROLL): the vector, the entries that
crossed, the info and the planes after the three decoders -- or the caller's device planes -- are compared with a numpy restatement
of the contract (tests/grab_yuv_scroll.py) that shares nothing with the library's kernels or codec.  Content is a tall page of
noise, with flat bands mixed in, of which a texture filled by uploads shows a slice.  Everything is 0 differing bytes.  Each check
runs on the host simulation and, under -m gpu, on the MI355X; the decoder's hostile-input check and the kernels' budget need
neither."""
import os
import shutil
import subprocess
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref, ROOT
import frame_taps as ft
import frame_grabs as fg
import grab_tensor as gt
import grab_yuv as gy
import grab_yuv_delta as gd
import grab_yuv_scroll as ys
import test_frame_grabs as tfg
from grab_yuv import I420, NV12, I444, FLIP, GUARD
from grab_yuv_delta import DELTA, KEY, YUV
from grab_yuv_scroll import SCROLL, SAMPLES, COPY
from webrender_amd import glapi, glconst as G, device, scenes
from webrender_amd.renderer import Renderer
from webrender_amd.harness import render_streamed_yuv

W, H = 192, 330          # 3 x 6 blocks, the last block row 10 rows; 165 chroma rows in 4:2:0
BANDS = ((90, 40, 30, 200, 90), (500, 24, 200, 10, 60), (700, 70, 128, 128, 128))
_cache = {}


class Hosts:
    """The three host decoders' planes, flat: WrhipGrabResultGet's, WrhipGrabDecodeYuv's, the numpy decoder's"""

    def __init__(self, w, h, fmt):
        n = sum(rows * row for rows, row in gy.row_bytes(w, h, fmt))
        self.lib, self.pure, self.numpy = (np.full(n, GUARD, np.uint8) for _ in range(3))


def check_scroll(gl, ticket, fmt, prev, want, hosts=None, dest=None, flags=0, keyframe=False, key=False, canary=None):
    """A SCROLL ticket against the retained planes `prev` and the planes `want` of the image now (gy.planes' lists): the vector, the
    entries as a set, the samples they carry, info, and the decoders' planes (`hosts`) or the device planes (`dest`).  -> info"""
    h, w = want[0].shape
    device_sink = dest is not None
    if keyframe:
        dy, kinds = 0, {rec: "send" for rec in fg.blocks_of(w, h)}
    else:
        dy, kinds = ys.classify(prev, want, fmt)
    expect = {rec: COPY if k == "copy" else SAMPLES for rec, k in kinds.items() if k != "same"}
    payload = gl.grab_payload(ticket)
    got_dy, entries = ys.split(payload, fmt, device_sink)
    assert got_dy == dy, (got_dy, dy)
    assert {rec: mode for rec, (mode, _) in entries.items()} == expect, (sorted(entries), sorted(expect.items()))
    if keyframe:
        assert list(entries) == fg.blocks_of(w, h), "on a keyframe entry i is block i"
    for rec, (mode, body) in entries.items():
        assert len(body) == (0 if mode == COPY or device_sink else gd.entry_bytes(fmt, False) - 16)
        if body:
            for k, (v, p) in enumerate(zip(ys.body_samples(body, rec, fmt), want)):
                assert np.array_equal(v, p[ys.block_slices(rec, fmt, k)]), f"plane {k} of the entry of block {rec}"
    copied = sum(1 for m in expect.values() if m == COPY)
    info, out = gl.grab_result(ticket, into=None if hosts is None else hosts.lib)
    assert (info["status"], info["format"], info["rects"][0][2:]) == (0, G.GL_RGBA8, (w, h)), info
    assert info["flags"] == (flags | YUV | DELTA | SCROLL | (KEY if key else 0)), info
    assert info["keyframe"] == (1 if keyframe else 0) and info["blocks_total"] == len(fg.blocks_of(w, h)), info
    assert (info["scroll_dy"], info["copied"], info["blocks"]) == (dy, copied, len(expect)), (info, dy, copied, len(expect))
    assert tuple(info["damage"]) == fg.damage_of(set(expect)), (info, sorted(expect))
    assert info["bytes"] == len(payload) == fg.HEADER + sum(ys.entry_size(fmt, m, device_sink) for m in expect.values()), info
    if device_sink:
        assert info["bytes"] == fg.HEADER + 16 * len(expect)
        img = dest.image(want)
        for at, v in (canary or {}).items():
            img[at:at + len(v)] = v
        got = dest.read()
        assert np.array_equal(got, img), f"{int((got != img).sum())} bytes of the device buffer differ"
    else:
        assert gl.grab_decode_yuv(payload, fmt, w, h, hosts.pure, scroll=True) == (fg.damage_of(set(expect)), len(expect))
        assert ys.decode(payload, fmt, ys.views(hosts.numpy, w, h, fmt)) == (len(expect), copied)
        for name, flat in (("grab_result", hosts.lib), ("grab_decode_yuv", hosts.pure), ("the numpy decoder", hosts.numpy)):
            bad = int((flat != gd.flat(want)).sum())
            assert bad == 0, f"{name}: {bad} bytes of the patched planes differ"
    info["modes"] = expect
    return info


class Scroller:
    """A texture that shows rows [at, at + h) of a tall page, delta-YUV-grabbed with SCROLL into host planes or a device Dest"""

    def __init__(self, s, page, h, at, fmt, sp, flags=0, dest=None):
        self.s, self.page, self.h, self.at, self.fmt, self.sp, self.flags, self.dest = s, page, h, at, fmt, sp, flags, dest
        self.shown = np.ascontiguousarray(page[at:at + h])
        self.w = self.shown.shape[1]
        self.t = s.make(self.shown, G.GL_RGBA8)
        self.hosts = Hosts(self.w, h, fmt) if dest is None else None
        self.prev = None

    def planes(self):
        return gy.planes(self.shown, self.fmt, self.sp, self.flags)

    def show(self, img):
        self.shown = np.ascontiguousarray(img)
        self.s.upload(self.t, 0, 0, self.shown)

    def scroll(self, dy, patch=None):
        """the content moves up by dy rows; patch: (x, y, w, h, seed) of the shown image rewritten with other noise"""
        self.at += dy
        img = self.page[self.at:self.at + self.h].copy()
        if patch:
            x, y, w, h, seed = patch
            img[y:y + h, x:x + w] = fg.noise(h, w, G.GL_RGBA8, seed)
        self.show(img)

    def ticket(self, scroll=True, key=False):
        kw = dict(dst=self.dest.dst, dst_bytes=self.dest.dst_bytes, strides=self.dest.strides) if self.dest else {}
        t = self.s.gl.grab_texture_yuv_delta(self.t.id, None, self.fmt, self.sp, self.flags, key=key, scroll=scroll, **kw)
        assert t >= 0, (t, self.s.gl.GetError())
        return t

    def grab(self, keyframe=False, key=False, canary=None):
        want = self.planes()
        info = check_scroll(self.s.gl, self.ticket(key=key), self.fmt, self.prev, want, self.hosts, self.dest, self.flags, keyframe, key, canary)
        self.prev = want
        return info

    def grab_plain(self):
        """a delta YUV grab without SCROLL of the same texture, rect and desc, patched into the same planes"""
        want = self.planes()
        t = self.ticket(scroll=False)
        sent = gd.changed_blocks(self.prev, want, self.fmt)
        info, _ = self.s.gl.grab_result(t, into=self.hosts.lib)
        gd.check_info(info, (0, 0, self.w, self.h), self.fmt, self.flags, False, sent, False)
        assert info["scroll_dy"] == 0 and info["copied"] == 0, info
        assert np.array_equal(self.hosts.lib, gd.flat(want))
        self.hosts.pure[...] = self.hosts.numpy[...] = self.hosts.lib
        self.prev = want

    def full(self):
        """the planes equal a full WrhipGrabTextureYuv of the frame"""
        info, flat = self.s.gl.grab_result(self.s.gl.grab_texture_yuv(self.t.id, None, self.fmt, self.sp, self.flags))
        assert np.array_equal(flat, gd.flat(self.prev)), "the model's planes are not the full YUV grab's"
        if self.hosts:
            assert np.array_equal(flat, self.hosts.lib)

    def still(self):
        info = self.grab()
        assert info["bytes"] == fg.HEADER and info["scroll_dy"] == 0 and info["blocks"] == 0, info


# ---------------------------------------------------------------------------- 1. wire and vector; 2. odd vectors

def _wire_and_vector(lib, fmt, sp):
    s = fg.Session(lib, 64, 64)
    sc = Scroller(s, ys.page(H + 800, W, 11 + fmt, BANDS), H, 300, fmt, sp)
    sc.grab(keyframe=True)
    sc.full()
    sc.still()
    for k, dy in enumerate((2, -2, 34, -34, 130)):
        sc.scroll(dy, patch=(70, 200, 20, 12, 100 + k))
        info = sc.grab()
        assert info["scroll_dy"] == dy and info["copied"] > 0 and info["modes"][(64, 192, 64, 64)] == SAMPLES, (dy, info)
        sc.full()
    sc.still()
    # 70 x 130: a cut block column of 6, a last block row of 2
    sm = Scroller(s, ys.page(130 + 200, 70, 21 + fmt), 130, 100, fmt, sp)
    sm.grab(keyframe=True)
    for dy in (34, -2):
        sm.scroll(dy)
        info = sm.grab()
        assert info["scroll_dy"] == dy and info["copied"] > 0, (dy, info)
        sm.full()
    assert s.gl.GetError() == 0
    s.close()


def _odd_vectors(lib):
    s = fg.Session(lib, 64, 64)
    for fmt in (I444, I420, NV12):
        sc = Scroller(s, ys.page(H + 200, W, 31 + fmt), H, 100, fmt, 2)      # (noise alone: no even candidate has a vote)
        sc.grab(keyframe=True)
        sc.scroll(33)
        info = sc.grab()
        if fmt == I444:
            assert info["scroll_dy"] == 33 and info["copied"] == 12, info
        else:
            assert info["scroll_dy"] == 0 and info["copied"] == 0 and info["blocks"] == info["blocks_total"], info
        sc.full()
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 3. bounds

def _bounds(lib):
    s = fg.Session(lib, 64, 64)
    h = 700
    for fmt in (I420, I444):
        sc = Scroller(s, ys.page(h + 1100, 64, 41 + fmt), h, 550, fmt, 3)
        sc.grab(keyframe=True)
        for dy, (want_dy, copied) in ((512, (512, 2)), (-512, (-512, 3)), (514, (0, 0))):
            sc.scroll(550 - sc.at)           # (from the first slice each time)
            sc.grab()
            sc.scroll(dy)
            info = sc.grab()
            # (dy 512: the blocks at y = 0 and 64 have their source inside the image; from y = 128 on it is partly outside)
            assert (info["scroll_dy"], info["copied"], info["blocks"]) == (want_dy, copied, 11), (dy, info)
            if dy == 512:
                assert info["modes"][(0, 128, 64, 64)] == SAMPLES and info["modes"][(0, 64, 64, 64)] == COPY, info
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 4. chroma-only and luma-only changes

def _same_luma_pair(sp):
    """Two stored colours the model maps to one Y and different Cb, Cr"""
    a = np.array([[[40, 120, 200, 255]]], np.uint8)
    for db in range(-12, 13):
        for dg in range(-12, 13):
            for dr in range(-12, 13):
                b = a.copy()
                b[0, 0, :3] = (40 + db, 120 + dg, 200 + dr)
                pa, pb = gy.planes(a, I444, sp), gy.planes(b, I444, sp)
                if pa[0] == pb[0] and pa[1] != pb[1] and pa[2] != pb[2]:
                    return a[0, 0], b[0, 0]
    raise AssertionError("no such pair")


def _chroma_and_luma_only(lib):
    s = fg.Session(lib, 64, 64)
    sp = 2
    a, b = _same_luma_pair(sp)
    grey = a.copy()
    grey[:3] += 9                      # (the chroma rows sum to 0: the same Cb, Cr, another Y)
    blk = (64, 64, 64, 64)
    for fmt in (I420, I444):
        base = ys.page(H, W, 51 + fmt)
        base[64:128, 64:128] = a
        sc = Scroller(s, base, H, 0, fmt, sp)
        sc.grab(keyframe=True)
        for colour, what in ((b, "chroma"), (a, "chroma"), (grey, "luma"), (b, "both")):
            img = sc.shown.copy()
            img[64:128, 64:128] = colour
            before = sc.planes()
            sc.show(img)
            after = sc.planes()
            luma_same = np.array_equal(before[0], after[0])
            chroma_same = all(np.array_equal(p, q) for p, q in zip(before[1:], after[1:]))
            assert (luma_same, chroma_same) == {"chroma": (True, False), "luma": (False, True), "both": (False, False)}[what]
            info = sc.grab()
            # (the block's rows are all equal: had a row that differs in chroma alone voted, +-1 .. 63 would have votes)
            assert info["scroll_dy"] == 0 and info["modes"] == {blk: SAMPLES}, (what, info)
            sc.full()
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 5. still frame, keyframe, mixing; 6. FLIP_ROWS

def _still_key_mixing(lib):
    s = fg.Session(lib, 64, 64)
    gl = s.gl
    sc = Scroller(s, ys.page(H + 400, W, 61, BANDS), H, 200, I420, 4)
    # a keyframe costs what the delta YUV grab's keyframe costs (the first grabs send the uploads ahead of them)
    plain = Scroller(s, sc.page, H, 200, I420, 4)
    gl.grab_result(plain.ticket(scroll=False), into=plain.hosts.lib)
    sc.grab(keyframe=True)
    n0 = s.stats()["kernel_launches"]
    gl.grab_result(plain.ticket(scroll=False, key=True), into=plain.hosts.lib)
    n1 = s.stats()["kernel_launches"]
    info = sc.grab(keyframe=True, key=True)
    n2 = s.stats()["kernel_launches"]
    assert n2 - n1 == n1 - n0 == 1 and info["scroll_dy"] == 0 and info["copied"] == 0, (n0, n1, n2, info)
    sc.still()
    sc.scroll(34)
    sc.grab(keyframe=True, key=True)
    sc.still()
    # five frames, with and without SCROLL in turn, no keyframe: the planes are exact after each
    for k, (scroll, dy) in enumerate(((True, 34), (False, 2), (True, -34), (False, -2), (True, 130))):
        sc.scroll(dy)
        if scroll:
            info = sc.grab()
            assert info["scroll_dy"] == dy and info["copied"] > 0 and info["keyframe"] == 0, (k, info)
        else:
            sc.grab_plain()
        sc.full()
    sc.still()
    assert gl.GetError() == 0
    s.close()


def _flip_rows(lib):
    s = fg.Session(lib, 64, 64)
    for fmt in (I420, I444):
        sc = Scroller(s, ys.page(H + 400, W, 71 + fmt, BANDS), H, 200, fmt, 0, flags=FLIP)
        sc.grab(keyframe=True)
        for dy in (34, -2):
            sc.scroll(dy)
            info = sc.grab()
            # (the texture's content moved up: the flipped image's moved down)
            assert info["scroll_dy"] == -dy and info["copied"] > 0, (dy, info)
            sc.full()
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 7. device sink

def _device_sink(lib):
    s = fg.Session(lib, 64, 64)
    gl = s.gl
    for fmt, geom in ((I420, dict(off=16, y_stride=W + 13, c_stride=W // 2 + 7)), (NV12, dict(off=1, y_stride=W + 3, c_stride=W + 5)), (I444, dict())):
        page = ys.page(H + 400, W, 81 + fmt, BANDS)
        chrome = ys.page(H, 64, 91 + fmt)
        d = gy.Dest(gl, W, H, fmt, **geom)
        sc = Scroller(s, page, H, 200, fmt, 2, dest=d)

        def shown(at):
            img = page[at:at + H].copy()
            img[:, :64] = chrome          # (the first block column does not move)
            return img
        sc.show(shown(200))
        sc.grab(keyframe=True)
        at = 200
        for dy in (34, -34, 2):
            at += dy
            sc.show(shown(at))
            want = sc.planes()
            kinds = ys.classify(sc.prev, want, fmt)[1]
            assert kinds[(0, 64, 64, 64)] == "same" and "copy" in kinds.values()
            copy = next(rec for rec, k in kinds.items() if k == "copy")
            ystride = geom.get("y_stride") or W
            # the caller scribbles over a block that becomes a COPY -- restored from the retained planes -- and over a block
            # that is not sent: nothing writes there, the bytes stay
            junk = np.full(16, 0x3C, np.uint8)
            for r in range(4):
                gl.device_write(d.dst + (copy[1] + 5 + r) * ystride + copy[0] + 9, junk)
            keep_at = d.off + (64 + 7) * ystride + 20
            gl.device_write(d.base + keep_at, junk)
            info = sc.grab(canary={keep_at: junk})
            assert info["scroll_dy"] == dy and info["copied"] > 0 and info["blocks"] < info["blocks_total"], (dy, info)
            # (the canary is the test's own: the planes are whole again)
            gl.device_write(d.base + keep_at, d.image(want)[keep_at:keep_at + 16])
        sc.still()
        d.free()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 8. stream and parking

SW, SH = 256, 256
STREAM_DY = (0, 34, 34, 0, -20, 2)          # frame k's content against frame k - 1's


def _stream_frame(off):
    """A small built scene whose rects lie `off` rows further up"""
    rng, rects = scenes.random_rects(14, SW, SH + 200, 24, 120, 77)
    rects = rects.copy()
    rects[:, [1, 3]] -= off
    rgba = np.concatenate([rng.integers(0, 256, size=(14, 3), dtype=np.uint8), np.full((14, 1), 255, np.uint8)], axis=1)
    return scenes.build_rect_frame(SW, SH, rects, scenes.premultiply(rgba), np.ones(14, bool), "brush")


def _stream_offsets():
    return list(np.cumsum(STREAM_DY) + 60)


def _oracle_stream(ref):
    """The oracle's render of every frame of the stream: computed once, never modified"""
    if (ref, "stream") not in _cache:
        gl = glapi.GL(ref)
        r = Renderer(gl, SW, SH)
        out = {}
        for off in sorted(set(_stream_offsets())):
            r.render(_stream_frame(off))
            r.finish()
            out[off] = r.device.read_texture(device.Texture(0, SW, SH, G.GL_RGBA8, fbo=0)).copy()
        r.destroy()
        _cache[(ref, "stream")] = out
    return _cache[(ref, "stream")]


def _stream(lib, ref):
    offs = _stream_offsets()
    want = _oracle_stream(ref)
    for dev, fmt, sp in ((False, I420, 2), (True, I444, 1)):
        planes, st, infos = render_streamed_yuv(lib, [_stream_frame(o) for o in offs], fmt, sp, device=dev, delta=True, scroll=True)
        assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
        assert st["setup_carried"] >= len(offs) - 1, st
        assert len(planes) == len(infos) == len(offs)
        prev = None
        for k, off in enumerate(offs):
            cur = gy.planes(want[off], fmt, sp)
            assert all(np.array_equal(a, b) for a, b in zip(planes[k], cur)), f"frame {k}: the accumulated planes are not the restatement on the oracle's render"
            info = infos[k]
            if prev is None:
                assert (info["keyframe"], info["scroll_dy"], info["copied"], info["blocks"]) == (1, 0, 0, info["blocks_total"]), info
            else:
                dy, kinds = ys.classify(prev, cur, fmt)
                copied = sum(1 for v in kinds.values() if v == "copy")
                assert (info["keyframe"], info["scroll_dy"], info["copied"]) == (0, dy, copied), (k, info, dy, copied)
                assert info["blocks"] == sum(1 for v in kinds.values() if v != "same"), (k, info)
                # (the window's stored rows run bottom-up: a scene that moves up moves down in the image)
                assert dy == -STREAM_DY[k] and (copied > 0) == (STREAM_DY[k] != 0), (k, dy, copied)
            assert info["status"] == 0 and info["flags"] & SCROLL, info
            prev = cur


def _parked(lib, ref):
    TW_, TH_ = tfg.W, tfg.H
    stored = ft.window_stored(tfg._ref_render(ref, "cfg2", tfg._frame))
    s = fg.Session(lib, TW_, TH_)
    gl = s.gl
    win = device.Texture(s.window, TW_, TH_, G.GL_RGBA8)
    fmt, sp = I420, 2
    p1 = gy.planes(stored, fmt, sp)
    grab = lambda: gl.grab_texture_yuv_delta(s.window, None, fmt, sp, scroll=True)
    # a SCROLL grab parked behind held-back raster launches; a later upload -- the window scrolled by 10 -- does not change its result
    s.r.render(tfg._frame())
    hosts = Hosts(TW_, TH_, fmt)
    t = grab()
    moved = stored.copy()
    moved[:TH_ - 10] = stored[10:]
    s.upload(win, 0, 0, moved)
    t2 = grab()
    p2 = gy.planes(moved, fmt, sp)
    check_scroll(gl, t, fmt, None, p1, hosts, keyframe=True)
    info = check_scroll(gl, t2, fmt, p1, p2, hosts)
    assert info["scroll_dy"] == 10 and info["copied"] > 0, info
    s.r.finish()
    # nine tickets against the ring of 8, parked: the first is dropped with its ticket -- it would have left the image in the
    # second set of planes --, so the second sends every block in its place
    s.upload(win, 0, 0, stored)
    s.r.render(tfg._frame())
    tickets = [grab() for _ in range(9)]
    assert len(set(tickets)) == 9
    with pytest.raises(KeyError):
        gl.grab_result(tickets[0])
    gt.send_held(gl)
    hosts = Hosts(TW_, TH_, fmt)
    check_scroll(gl, tickets[1], fmt, None, p1, hosts, keyframe=True)
    for t in tickets[2:]:
        info = check_scroll(gl, t, fmt, p1, p1, hosts)
        assert info["bytes"] == fg.HEADER, info
    back = stored.copy()
    back[12:] = stored[:TH_ - 12]
    s.upload(win, 0, 0, back)
    info = check_scroll(gl, grab(), fmt, p1, gy.planes(back, fmt, sp), hosts)
    assert info["scroll_dy"] == -12 and info["copied"] > 0, info
    s.r.finish()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 9. refusals and cost

def _refusals_and_cost(lib):
    s = fg.Session(lib, 64, 64)
    gl = s.gl
    assert glapi.GRAB_YUV_SCROLL_LAUNCHES == 3
    sc = Scroller(s, ys.page(H + 100, W, 95), H, 50, I420, 2)
    sc.grab(keyframe=True)
    rect = (0, 0, W, H)
    a = s.stats()
    DS = DELTA | SCROLL                # (the flag's spelling on this call; either bit alone is refused, as it always was)
    for k, flags in enumerate((SCROLL, DELTA, SCROLL | KEY, DELTA | KEY, DS | 1, DS | 2, DS | 16, DS | 32, DS | 64, DS | 128, DS | 512, DS | KEY | 2048, 2048)):
        assert gl.grab_texture_yuv_delta(sc.t.id, rect, I420, 2, key=flags) == -1, k
        assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0, k
    # what the call refuses without the flag, it refuses with it
    for k, kw in enumerate((dict(rect=(0, 0, W + 1, H)), dict(format=3), dict(color_space=6), dict(flags=SCROLL), dict(flags=2), dict(strides=(8, 0)))):
        args = dict(rect=rect, format=I420, color_space=2, flags=0)
        args.update(kw)
        assert gl.grab_texture_yuv_delta(sc.t.id, args["rect"], args["format"], args["color_space"], args["flags"], strides=args.get("strides", (0, 0)), scroll=True) == -1, k
        assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0, k
    assert gl.grab_texture_yuv(sc.t.id, rect, I420, 2, flags=SCROLL) == -1
    assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    assert gl.grab_texture_yuv_scaled(sc.t.id, rect, (W // 2, H // 2), I420, 2, flags=SCROLL) == -1
    assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    b = s.stats()
    assert (b["kernel_launches"], b["flushes"]) == (a["kernel_launches"], a["flushes"]), (a, b)
    sc.still()                         # (the retained copy is still valid: no keyframe)
    # cost: WRHIP_GRAB_YUV_SCROLL_LAUNCHES launches and no flush for a grab that is no keyframe
    sc.scroll(34)
    gl.grab_result(gl.grab_texture(sc.t.id, None, 0))      # (the upload goes out ahead of this one)
    a = s.stats()
    t = sc.ticket()
    b = s.stats()
    assert (b["kernel_launches"] - a["kernel_launches"], b["flushes"] - a["flushes"]) == (glapi.GRAB_YUV_SCROLL_LAUNCHES, 0), (a, b)
    want = sc.planes()
    info = check_scroll(gl, t, I420, sc.prev, want, sc.hosts)
    assert info["scroll_dy"] == 34, info
    # the pure decoder from Python: a SCROLL payload without the bit, and the other way round, is malformed
    payload = gl.grab_payload(t)
    into = np.full_like(sc.hosts.pure, 7)
    with pytest.raises(ValueError):
        gl.grab_decode_yuv(payload, I420, W, H, into)
    assert (into == 7).all()
    sc.prev = want
    sc.scroll(2)
    t = sc.ticket(scroll=False)
    with pytest.raises(ValueError):
        gl.grab_decode_yuv(gl.grab_payload(t), I420, W, H, into, scroll=True)
    assert (into == 7).all()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 10. budget; 11. hostile payloads (CPU only)

def test_yuv_scroll_kernels_have_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    for name in ("wr_grab_yuv_scroll_probe_kernel", "wr_grab_yuv_scroll_pack_kernel"):
        assert name in notes, sorted(notes)
        vgprs, scratch = notes[name]
        assert scratch == 0, (name, vgprs, scratch)


def test_yuv_scroll_decoder_on_hostile_input(tmp_path):
    """tools/grab_yuv_scroll_check.cpp -- wr_grab_codec.h alone, its own main -- under AddressSanitizer and UBSan, as a process of its own"""
    cxx = shutil.which("g++")
    flags = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    trivial = tmp_path / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    if cxx is None or subprocess.run([cxx] + flags + [str(trivial), "-o", str(tmp_path / "trivial")], capture_output=True).returncode != 0:
        pytest.skip("no g++ that links with -fsanitize=address,undefined")
    exe = tmp_path / "grab_yuv_scroll_check"
    subprocess.run([cxx] + flags + ["-I", os.path.join(ROOT, "webrender_amd", "csrc"), os.path.join(ROOT, "tools", "grab_yuv_scroll_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "grab_yuv_scroll_check: ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


# ---------------------------------------------------------------------------- CPU: the host simulation

WIRE = [(I420, 2), (NV12, 1), (I444, 0)]
WIRE_IDS = ["i420", "nv12", "i444"]


@pytest.mark.parametrize("fmt,sp", WIRE, ids=WIRE_IDS)
def test_hostsim_wire_and_vector(hostsim, fmt, sp):
    _wire_and_vector(hostsim, fmt, sp)


def test_hostsim_odd_vectors(hostsim):
    _odd_vectors(hostsim)


def test_hostsim_bounds(hostsim):
    _bounds(hostsim)


def test_hostsim_chroma_and_luma_only(hostsim):
    _chroma_and_luma_only(hostsim)


def test_hostsim_still_key_mixing(hostsim):
    _still_key_mixing(hostsim)


def test_hostsim_flip_rows(hostsim):
    _flip_rows(hostsim)


def test_hostsim_device_sink(hostsim):
    _device_sink(hostsim)


def test_hostsim_stream(hostsim, oracle_gcc):
    _stream(hostsim, oracle_gcc)


def test_hostsim_parked(hostsim, oracle_gcc):
    _parked(hostsim, oracle_gcc)


def test_hostsim_refusals_and_cost(hostsim):
    _refusals_and_cost(hostsim)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,sp", WIRE, ids=WIRE_IDS)
def test_gpu_wire_and_vector(fmt, sp):
    _wire_and_vector(wrhip_lib(), fmt, sp)


@pytest.mark.gpu
def test_gpu_odd_vectors():
    _odd_vectors(wrhip_lib())


@pytest.mark.gpu
def test_gpu_bounds():
    _bounds(wrhip_lib())


@pytest.mark.gpu
def test_gpu_chroma_and_luma_only():
    _chroma_and_luma_only(wrhip_lib())


@pytest.mark.gpu
def test_gpu_still_key_mixing():
    _still_key_mixing(wrhip_lib())


@pytest.mark.gpu
def test_gpu_flip_rows():
    _flip_rows(wrhip_lib())


@pytest.mark.gpu
def test_gpu_device_sink():
    _device_sink(wrhip_lib())


@pytest.mark.gpu
def test_gpu_stream():
    _stream(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_parked():
    _parked(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_refusals_and_cost():
    _refusals_and_cost(wrhip_lib())
