"""Scaled YUV grabs (include/wrhip.h: WrhipGrabTextureYuvScaled): a texture rect scaled down by the scaled grab's chain and delivered
as the YUV grab's planes, at up to four sizes -- the lowest levels of the one chain -- from a single pass.  Expected bytes never come
from the code under test: the ORACLE runs the chain as BlitFramebuffer calls and every level is kept (tests/grab_yuv_scaled.py:
blit_levels), tests/grab_yuv.py's restatement turns level k into planes, and 0 bytes may differ.  Device destinations and host
buffers are filled with 0xA5 first and compared whole.  Each check runs on the host simulation and, under -m gpu, on the MI355X."""
import ctypes as C
import itertools
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
import frame_grabs as fg
import grab_tensor as gt
import grab_yuv as gy
import grab_yuv_scaled as gys
from grab_scaled import levels_of
from grab_yuv import I420, NV12, I444, FORMATS, SPACES, FLIP, GUARD
from test_grab_scaled import STREAM_SEEDS, W, H, TW, TH, _noise, _frame
from webrender_amd import glapi, glconst as G, device
from webrender_amd.renderer import Renderer
from webrender_amd.harness import render_streamed, render_streamed_yuv

# name: (rect, size of rendition 0, renditions)
CASES = {
    "L0_general": ((0, 0, 333, 201), (200, 121), 1),          # 64-px tiles cut on both axes, the clamp at an odd last row
    "L0_equal": ((3, 5, 61, 37), (61, 37), 1),                # the nearest copy: a YUV grab of the rect
    "L1_edge": ((233, 101, 100, 100), (30, 30), 2),           # taps at the texture's last column and row; 30 x 30 and 60 x 60
    "L2_ladder": ((0, 0, 333, 201), (60, 36), 3),             # three renditions from one launch, both LDS buffers
    "L3_even": ((0, 0, 333, 201), (37, 22), 4),               # 8-px tiles, odd width, flipped 4:2:0 inside tiles
    "L3_odd": ((0, 0, 333, 201), (37, 21), 4),                # flipped 4:2:0 of odd height: the extra launch, for rendition 0 only
    "L4": ((0, 0, 330, 170), (20, 10), 3),                    # renditions split over two launches
    "L8": ((0, 0, 333, 201), (1, 1), 2),                      # three launches; 1 x 1 and 2 x 2 images
    "thin": ((328, 0, 5, 201), (2, 80), 2),                   # a rect 5 pixels wide
}
LEVELS = {"L0_general": 0, "L0_equal": 0, "L1_edge": 1, "L2_ladder": 2, "L3_even": 3, "L3_odd": 3, "L4": 4, "L8": 8, "thin": 1}
TWO_SPACES = (2, 1)                                           # Rec709Narrow, Rec601Full: the clamp fires in a full range
WIN = ((0, 0, W, H), (64, 64), 3)                             # the window's ladder: 64, 128 and 256 squared; L = 2
_cache = {}


def _oracle_noise(ref):
    """The oracle's chain, every level kept, for every case on the noise texture: computed once per session, never modified"""
    if (ref, "noise") not in _cache:
        gl = glapi.GL(ref)
        r = Renderer(gl, 64, 64)
        d = r.device
        tex = d.create_texture(TW, TH, G.GL_RGBA8, render_target=True)
        d.upload_texture(tex, 0, 0, TW, TH, G.GL_BGRA, G.GL_UNSIGNED_BYTE, _noise())
        _cache[(ref, "noise")] = {name: gys.blit_levels(gl, d, tex, rect, size) for name, (rect, size, _) in CASES.items()}
        r.destroy()
    return _cache[(ref, "noise")]


def _oracle_frames(ref):
    """The oracle's chain 512 x 512 -> 64 x 64, every level kept, on its own render of the cfg2 frame and of every streamed frame"""
    if (ref, "frames") not in _cache:
        gl = glapi.GL(ref)
        r = Renderer(gl, W, H)
        window = device.Texture(0, W, H, G.GL_RGBA8, fbo=0)
        out = {}
        for key, frame in [("cfg2", _frame())] + [(sd, _frame(sd, 60)) for sd in STREAM_SEEDS]:
            r.render(frame)
            r.finish()
            out[key] = gys.blit_levels(gl, r.device, window, WIN[0], WIN[1])
        r.destroy()
        _cache[(ref, "frames")] = out
    return _cache[(ref, "frames")]


def _noise_session(lib):
    s = fg.Session(lib, 64, 64)
    tex = s.make(_noise(), G.GL_RGBA8)
    s.r.finish()
    return s, tex


def _fetch_host(gl, t, payload):
    """The ticket's payload through WrhipGrabResultGet into a buffer of guard bytes, compared whole: -> info dict, the planes' bytes"""
    buf = np.full(payload + 48, GUARD, np.uint8)
    r = glapi.WrhipGrabInfo()
    assert gl.WrhipGrabResultGet(t, C.byref(r), buf.ctypes.data, 0, 1) == 0
    assert (buf[payload:] == GUARD).all(), "bytes behind the payload were written"
    info = {"status": r.status, "format": r.format, "flags": r.flags, "rects": [tuple(r.rects[i]) for i in range(r.nrects)],
            "bytes": int(r.bytes), "scaled_w": r.scaled_w, "scaled_h": r.scaled_h, "levels": r.levels, "renditions": r.renditions}
    return info, buf[:payload]


def _one(s, tex, rect, size, n, levels, fmt, sp, flags=0, sink="host", what="", **geom):
    """One grab on a quiescent session, checked whole: `levels` are the oracle's.  The header's launches, no flush."""
    L = levels_of(rect[2], size[0])
    want = gys.planes(levels, n, fmt, sp, flags)
    flat = np.concatenate([p.reshape(-1) for r in want for p in r])
    d = gys.Ladder(s.gl, size, n, fmt, **geom) if sink == "device" else None
    a = s.stats()
    t = gys.grab(s, tex, rect, size, n, fmt, sp, flags, d)
    b = s.stats()
    assert b["kernel_launches"] == a["kernel_launches"] + gys.launches(L, size, fmt, flags) and b["flushes"] == a["flushes"], (what, a, b)
    if d is None:
        info, got = _fetch_host(s.gl, t, len(flat))
        gys.check_info(info, rect, size, L, n, flags, len(flat))
        assert int((got != flat).sum()) == 0, f"{what}: {int((got != flat).sum())} bytes of the payload differ"
    else:
        info, got = s.gl.grab_result(t)
        assert len(got) == 0
        gys.check_info(info, rect, size, L, n, flags, 0)
        d.check(want, what)
        d.free()


# ---------------------------------------------------------------------------- 1. the table against the oracle's chain

def _case(lib, ref, name):
    rect, size, n = CASES[name]
    levels = _oracle_noise(ref)[name]
    L = LEVELS[name]
    assert len(levels) == L + 1 == levels_of(rect[2], size[0]) + 1 and n <= min(L + 1, 4)
    assert all(levels[k].shape == (size[1] << k, size[0] << k, 4) for k in range(L + 1))
    s, tex = _noise_session(lib)
    for fmt, sp, flags, sink in itertools.product(FORMATS, TWO_SPACES, (0, FLIP), ("host", "device")):
        _one(s, tex.id, rect, size, n, levels, fmt, sp, flags, sink, what=f"{name} fmt {fmt} space {sp} flags {flags} {sink}")
    # the bytes that crossed: the header (word 0: the payload's bytes), then rendition after rendition
    t = gys.grab(s, tex.id, rect, size, n, NV12, 2)
    raw = s.gl.grab_payload(t)
    want = gys.expected(levels, n, NV12, 2)
    assert len(raw) == fg.HEADER + len(want) and int.from_bytes(raw[:4], "little") == len(want)
    assert np.array_equal(np.frombuffer(raw[fg.HEADER:], np.uint8), want)
    info, flat = s.gl.grab_result(t)
    assert np.array_equal(flat, want)
    rends = glapi.yuv_split_renditions(flat, size, n, NV12)
    assert [r[0].shape for r in rends] == [(size[1] << k, size[0] << k) for k in range(n)]
    assert s.gl.GetError() == 0
    s.close()


def _all_spaces(lib, ref):
    rect, size, n = CASES["L2_ladder"]
    levels = _oracle_noise(ref)["L2_ladder"]
    s, tex = _noise_session(lib)
    for k, sp in enumerate(SPACES):
        fmt, flags = FORMATS[k % 3], FLIP if k % 2 else 0
        _one(s, tex.id, rect, size, n, levels, fmt, sp, flags, "host", what=f"space {sp}")
        _one(s, tex.id, rect, size, n, levels, FORMATS[(k + 1) % 3], sp, flags ^ FLIP, "device", what=f"space {sp} device")
    assert s.gl.GetError() == 0
    s.close()


def _clamp(lib, ref):
    """Noise never reaches the clamp.  tests/test_grab_yuv.py's constructed texture does: its flat 2 x 2 blocks of pure blue and pure
    red survive the 2:1 top step to level 1, where a full range gives 256 before the clamp"""
    from test_grab_yuv import constructed
    rect, size, n = (0, 0, 64, 8), (16, 2), 2
    if (ref, "constructed") not in _cache:
        gl = glapi.GL(ref)
        r = Renderer(gl, 64, 64)
        tex = r.device.create_texture(64, 8, G.GL_RGBA8, render_target=True)
        r.device.upload_texture(tex, 0, 0, 64, 8, G.GL_BGRA, G.GL_UNSIGNED_BYTE, constructed())
        _cache[(ref, "constructed")] = gys.blit_levels(gl, r.device, tex, rect, size)
        r.destroy()
    levels = _cache[(ref, "constructed")]
    assert len(levels) == 2
    s = fg.Session(lib, 64, 64)
    tex = s.make(constructed(), G.GL_RGBA8)
    s.r.finish()
    for fmt, sp in itertools.product(FORMATS, (1, 3, 5)):
        if fmt == I444:
            assert gy.clamped(levels[1], fmt, sp)[1] > 0, (fmt, sp)
        for flags, sink in itertools.product((0, FLIP), ("host", "device")):
            _one(s, tex.id, rect, size, n, levels, fmt, sp, flags, sink, what=f"constructed fmt {fmt} space {sp} flags {flags} {sink}")
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 2. equivalence with the calls it restates

def _equivalence(lib, ref):
    s, tex = _noise_session(lib)
    for name, (rect, size, n) in CASES.items():
        fmt, sp, flags = FORMATS[len(name) % 3], 3, FLIP if len(name) % 2 else 0
        flat = s.gl.grab_result(gys.grab(s, tex.id, rect, size, n, fmt, sp, flags))[1]
        rends = glapi.yuv_split_renditions(flat, size, n, fmt)
        for k in range(n):
            sk = (size[0] << k, size[1] << k)
            if sk[0] > rect[2] or sk[1] > rect[3]:
                continue                                    # (the standalone call is not legal: it would scale up)
            # rendition k is the n = 1 grab of that size ...
            alone = s.gl.grab_result(gys.grab(s, tex.id, rect, sk, 1, fmt, sp, flags))[1]
            assert all(np.array_equal(a, b) for a, b in zip(rends[k], glapi.yuv_split(alone, sk[0], sk[1], fmt))), (name, k)
            # ... and the restatement on what WrhipGrabTextureScaled delivers at that size
            t = s.gl.grab_texture_scaled(tex.id, rect, sk)
            assert t >= 0
            px = s.gl.grab_result(t)[1]
            assert np.array_equal(px, _oracle_noise(ref)[name][k]), (name, k)
            assert all(np.array_equal(a, b) for a, b in zip(rends[k], gy.planes(px, fmt, sp, flags))), (name, k)
    # n = 1 at the rect's size is the YUV grab of the rect
    rect, size, _ = CASES["L0_equal"]
    for fmt, flags in itertools.product(FORMATS, (0, FLIP)):
        a = s.gl.grab_result(gys.grab(s, tex.id, rect, size, 1, fmt, 5, flags))[1]
        b = s.gl.grab_result(gy.grab(s, tex.id, rect, fmt, 5, flags))[1]
        assert np.array_equal(a, b) and np.array_equal(a, gy.expected(fg.crop(_noise(), rect), fmt, 5, flags)), (fmt, flags)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 3. device-sink geometry

def _geometry(lib, ref):
    s, tex = _noise_session(lib)
    for name in ("L2_ladder", "L3_odd"):
        rect, size, n = CASES[name]
        levels = _oracle_noise(ref)[name]
        for fmt in FORMATS:
            def st(fy, fc):
                out = []
                for k in range(n):
                    w, h = size[0] << k, size[1] << k
                    out.append(dict(y_stride=fy(w), c_stride=fc(gy.row_bytes(w, h, fmt)[1][1])))
                return out
            r16 = lambda v: (v + 15) // 16 * 16 + 16
            geoms = [dict(off=1), dict(off=3, gap=5), dict(off=16, gap=16), dict(gap=1),          # (off 1, 3: NV12 at an odd address)
                     dict(geoms=st(lambda w: w + 1, lambda c: c | 1)), dict(off=3, gap=7, geoms=st(lambda w: w + 13, lambda c: (c + 2) | 1)),
                     dict(geoms=st(r16, r16)), dict(off=16, gap=32, geoms=st(lambda w: r16(w) + 16, r16)),
                     dict(gap=3, geoms=st(lambda w: (w + 7) // 8 * 8, lambda c: (c + 7) // 8 * 8 + 4))]
            for k, g in enumerate(geoms):
                _one(s, tex.id, rect, size, n, levels, fmt, (k + fmt) % 6, FLIP if k % 2 else 0, "device", what=f"{name} fmt {fmt} geometry {k}", **g)
    # dst_bytes: Ladder passes exactly each extent (accepted above); a byte short in any rendition is rejected and writes nothing
    rect, size, n = CASES["L2_ladder"]
    n0, f0 = s.stats()["kernel_launches"], s.stats()["flushes"]
    for fmt, short in itertools.product(FORMATS, range(n)):
        d = gys.Ladder(s.gl, size, n, fmt, off=1, gap=2)
        assert s.gl.grab_texture_yuv_scaled(tex.id, rect, size, fmt, 0, 0, renditions=n, dsts=d.dsts(short=short), strides=d.strides()) == -1
        assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0
        assert d.untouched()
        d.free()
    assert s.stats()["kernel_launches"] == n0 and s.stats()["flushes"] == f0
    s.close()


# ---------------------------------------------------------------------------- 4. ordering

def _later_upload(lib, ref):
    """A grab to either sink, then an upload over the source: the grabs are unchanged"""
    rect, size, n = CASES["L4"]
    levels = _oracle_noise(ref)["L4"]
    s, tex = _noise_session(lib)
    d = gys.Ladder(s.gl, size, n, I420, off=1)
    th, td = gys.grab(s, tex.id, rect, size, n, NV12, 3), gys.grab(s, tex.id, rect, size, n, I420, 0, FLIP, d)
    s.upload(tex, 0, 0, fg.noise(TH, TW, G.GL_RGBA8, 12))
    s.r.finish()
    assert np.array_equal(s.gl.grab_result(th)[1], gys.expected(levels, n, NV12, 3))
    s.gl.grab_result(td)
    d.check(gys.planes(levels, n, I420, 0, FLIP), "device grab ahead of an upload")
    d.free()
    assert s.gl.GetError() == 0
    s.close()


def _rendered_frame(lib, ref):
    """The window behind its held-back launches, no Finish: both grabs are parked; a later write to the window is not seen"""
    rect, size, n = WIN
    levels = _oracle_frames(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    s.r.render(_frame())
    d = gys.Ladder(s.gl, size, n, NV12, gap=4)
    th = gys.grab(s, s.window, rect, size, n, I420, 2, FLIP)      # (submits what was recorded; the frame's raster launches stay held back)
    a = s.stats()
    td = gys.grab(s, s.window, rect, size, n, NV12, 5, 0, d)
    assert s.gl.grab_result(th, wait=False) is None and s.gl.grab_result(td, wait=False) is None          # parked
    assert s.stats()["kernel_launches"] == a["kernel_launches"]          # (nothing left: neither a grab nor what it is parked behind)
    s.upload(device.Texture(s.window, W, H, G.GL_RGBA8), 100, 60, fg.noise(70, 40, G.GL_RGBA8, 77))
    info, flat = s.gl.grab_result(th)
    want = gys.expected(levels, n, I420, 2, FLIP)
    gys.check_info(info, rect, size, 2, n, FLIP, len(want))
    assert int((flat != want).sum()) == 0
    gys.check_info(s.gl.grab_result(td)[0], rect, size, 2, n, 0, 0)
    d.check(gys.planes(levels, n, NV12, 5), "rendered frame, device")
    d.free()
    s.r.finish()
    assert s.gl.GetError() == 0
    s.close()


def _nine(s, levels, parked, sink):
    """Nine grabs of the window without a fetch: the ring holds the 8 newest tickets.  Host sink: the first is dead, the other eight
    are exact.  Device sink: all nine buffers are written."""
    rect, size, _ = WIN
    dests, tickets, wants = [], [], []
    for k in range(9):
        fmt, sp, flags, n = FORMATS[k % 3], k % 6, FLIP if k % 2 else 0, 1 + k % 3
        d = gys.Ladder(s.gl, size, n, fmt, off=k % 2) if sink == "device" else None
        tickets.append(gys.grab(s, s.window, rect, size, n, fmt, sp, flags, d))
        dests.append(d)
        wants.append(gys.planes(levels, n, fmt, sp, flags))
    assert len(set(tickets)) == 9
    out = glapi.WrhipGrabInfo()
    if parked:
        assert all(s.gl.WrhipGrabResultGet(t, C.byref(out), None, 0, 0) == 1 for t in tickets[1:])
    assert s.gl.WrhipGrabResultGet(tickets[0], C.byref(out), None, 0, 1) == -1
    with pytest.raises(KeyError):
        s.gl.grab_result(tickets[0])
    if parked:
        gt.send_held(s.gl)                              # the held-back launches go out, the grabs behind them
    for k in range(1, 9):
        info, flat = s.gl.grab_result(tickets[k])
        assert info["flags"] & gys.YUV and info["flags"] & gys.SCALED and info["renditions"] == 1 + k % 3
        if sink == "host":
            want = np.concatenate([p.reshape(-1) for r in wants[k] for p in r])
            assert int((flat != want).sum()) == 0, k
    for k, (d, want) in enumerate(zip(dests, wants)):
        if d is not None:
            d.check(want, f"grab {k}")
            d.free()


def _ring(lib, ref):
    levels = _oracle_frames(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    for sink in ("host", "device"):
        s.r.render(_frame())
        _nine(s, levels, True, sink)
        s.r.finish()
        _nine(s, levels, False, sink)
    assert s.gl.GetError() == 0
    s.close()


def _free_and_put(lib, ref):
    rect, size, n = WIN
    levels = _oracle_frames(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    gl = s.gl
    # WrhipDeviceFree of a buffer a parked grab writes: the grab is sent first (with what it is parked behind), and the call returns
    s.r.render(_frame())
    d = gys.Ladder(gl, size, n, I420)
    t = gys.grab(s, s.window, rect, size, n, I420, 1, 0, d)
    assert gl.grab_result(t, wait=False) is None
    d.free()
    assert gl.WrhipFlushHeld() == 0                     # nothing is held any more
    gys.check_info(gl.grab_result(t)[0], rect, size, 2, n, 0, 0)
    s.r.finish()
    # a put that reads a parked grab's destination sees the grab's bytes: the Y plane of rendition 1 (128 x 128) becomes an R8
    # texture -- the overlap rule holds for every rendition, not the first alone
    r8 = s.d.create_texture(128, 128, G.GL_R8, render_target=True)
    s.upload(r8, 0, 0, np.zeros((128, 128), np.uint8))
    s.r.finish()
    s.r.render(_frame())
    d = gys.Ladder(gl, size, n, I444, gap=16)
    t = gys.grab(s, s.window, rect, size, n, I444, 3, FLIP, d)
    assert gl.grab_result(t, wait=False) is None
    y1 = d.dsts()[1][0]
    assert gl.put_texture_tensor(r8.id, (0, 0, 128, 128), y1, 128 * 128, dtype=gt.U8, layout=gt.CHW, channels=1) == 0
    want = gys.planes(levels, n, I444, 3, FLIP)
    assert np.array_equal(s.d.read_texture(r8), want[1][0])
    gl.grab_result(t)
    d.check(want, "the grab a put read from")
    d.free()
    s.r.finish()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 5. streamed

def _stream(lib, ref):
    rect, size, n = WIN
    frames = lambda: [_frame(sd, 60) for sd in STREAM_SEEDS]
    _, plain = render_streamed(lib, frames())
    want = _oracle_frames(ref)
    for dev, fmt, sp in ((False, I420, 2), (True, NV12, 1)):
        rends, st, infos = render_streamed_yuv(lib, frames(), fmt, sp, device=dev, scale_to=size, renditions=n)
        assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
        assert st["setup_carried"] == plain["setup_carried"] and st["setup_carried"] >= len(STREAM_SEEDS) - 1, (st, plain)
        assert len(rends) == len(infos) == len(STREAM_SEEDS)
        bad = [sd for i, sd in enumerate(STREAM_SEEDS)
               if not all(np.array_equal(a, b) for got, exp in zip(rends[i], gys.planes(want[sd], n, fmt, sp)) for a, b in zip(got, exp))]
        assert not bad, f"frames whose renditions are not the restatement on the oracle's chain: {bad}"
        assert all(len(r) == n and len(r[k]) == (2 if fmt == NV12 else 3) for r in rends for k in range(n))
        payload = 0 if dev else len(gys.expected(want[STREAM_SEEDS[0]], n, fmt, sp))
        gys.check_info(infos[-1], rect, size, 2, n, 0, payload)


# ---------------------------------------------------------------------------- 6. the contract's rejections

def _contract(lib):
    s = fg.Session(lib, W, H)
    gl = s.gl
    s.r.render(_frame())
    s.r.finish()
    r8 = s.make(fg.noise(37, 61, G.GL_R8, 611), G.GL_R8)
    s.r.finish()
    assert gl.GetError() == 0
    win = s.window
    full = (0, 0, W, H)
    room = 1 << 18                                      # (64, 128 and 256 squared in I444 fit three times over)
    buf = gl.device_alloc(3 * room)
    gt.fill(gl, buf, 3 * room)
    n0, f0 = s.stats()["kernel_launches"], s.stats()["flushes"]
    i420 = lambda k: (64 << k) * (64 << k) * 3 // 2
    good = [(buf + k * room, i420(k)) for k in range(3)]

    def call(tex=win, rect=full, size=(64, 64), fmt=I420, sp=0, flags=0, n=3, dsts=good, strides=None):
        return gl.grab_texture_yuv_scaled(tex, rect, size, fmt, sp, flags, renditions=n, dsts=dsts, strides=strides)

    def raw(descs, n, rect=full, size=(64, 64)):
        """The call with descs built field by field: (format, space, flags, dst, dst_bytes, y_stride, c_stride) each"""
        arr = (glapi.WrhipYuvDesc * len(descs))()
        for d, v in zip(arr, descs):
            d.format, d.color_space, d.flags, d.dst, d.dst_bytes, d.y_stride, d.c_stride = v
        r4 = (C.c_int32 * 4)(*rect)
        return gl.WrhipGrabTextureYuvScaled(win, C.addressof(r4), size[0], size[1], C.addressof(arr), n)
    dev = lambda k, fmt=I420, sp=0, flags=0: (fmt, sp, flags, good[k][0], good[k][1], 0, 0)
    host = lambda fmt=I420, sp=0, flags=0: (fmt, sp, flags, None, 0, 0, 0)
    r4 = (C.c_int32 * 4)(*full)
    bad = [
        # what WrhipGrabTextureScaled rejects for tex, rect, out_w, out_h
        lambda: call(tex=9999), lambda: call(tex=r8.id, rect=(0, 0, 8, 8), size=(2, 2), n=1),      # unknown texture; not GL_RGBA8
        lambda: call(rect=(0, 0, 0, 4), size=(1, 1), n=1), lambda: call(rect=(0, 0, 4, 0), size=(1, 1), n=1),      # empty
        lambda: call(rect=(500, 0, 13, 1), size=(1, 1), n=1), lambda: call(rect=(0, -1, 4, 4), size=(2, 2), n=1),      # outside the texture
        lambda: call(size=(0, 64), n=1), lambda: call(size=(64, 0), n=1),                 # size below 1
        lambda: call(size=(W + 1, 64), n=1), lambda: call(size=(64, H + 1), n=1),         # size above the rect's
        lambda: call(size=(1, H), n=1, dsts=None),                                        # L = 8: level 8 would be 256 x 131072
        # what WrhipGrabTextureYuv rejects for a desc, in the first rendition and in a later one
        lambda: call(fmt=3), lambda: call(sp=6), lambda: call(sp=7),                      # unknown format; GbrIdentity and above
        lambda: call(flags=glapi.GRAB_SWAP_RB), lambda: call(flags=glapi.GRAB_DELTA), lambda: call(flags=gys.YUV), lambda: call(flags=gys.SCALED),
        lambda: call(dsts=None, strides=[(64, 0), (0, 0), (0, 0)]), lambda: call(dsts=None, strides=[(0, 0), (0, 0), (0, 128)]),      # host sink with a stride
        lambda: raw([host(), (I420, 0, 0, None, 1, 0, 0)], 2),                            # host sink with dst_bytes
        lambda: call(strides=[(63, 0), (0, 0), (0, 0)]), lambda: call(strides=[(0, 0), (127, 0), (0, 0)]),      # strides below the rendition's rows
        lambda: call(strides=[(0, 0), (0, 0), (0, 127)]), lambda: call(strides=[(0, 0), (-128, 0), (0, 0)]),
        lambda: call(fmt=NV12, strides=[(0, 0), (0, 127), (0, 0)]),
        lambda: call(strides=[(0, 0), ((1 << 40) + 1, 0), (0, 0)], dsts=[good[0], (good[1][0], 1 << 62), good[2]]),
        lambda: call(dsts=[(good[0][0], i420(0) - 1), good[1], good[2]]),                 # an extent that does not fit, per rendition
        lambda: call(dsts=[good[0], good[1], (good[2][0], i420(2) - 1)]),
        lambda: call(fmt=I444, dsts=[(buf, 64 * 64 * 3), (buf + room, 128 * 128 * 3 - 1)], n=2),
        # renditions outside 1 .. min(L + 1, 4); no descs
        lambda: call(n=0), lambda: call(n=-1), lambda: call(n=4, dsts=good + [(buf, 1 << 30)]), lambda: call(n=5, dsts=None),
        lambda: call(size=(256, 256), n=2, dsts=None),                                    # L = 0: one rendition
        lambda: call(rect=(0, 0, 2, 2), size=(1, 1), n=2, dsts=None),                     # L = 0 again: 2 <= 2 * 1
        lambda: call(size=(4, 4), n=5, dsts=None),                                        # L = 6: still no more than 4
        lambda: gl.WrhipGrabTextureYuvScaled(win, C.addressof(r4), 64, 64, None, 1),
        lambda: gl.WrhipGrabTextureYuvScaled(win, None, 64, 64, None, 1),
        # descs that disagree
        lambda: raw([dev(0), dev(1, fmt=NV12)], 2), lambda: raw([dev(0), dev(1), dev(2, sp=2)], 3), lambda: raw([dev(0, flags=FLIP), dev(1)], 2),
        lambda: raw([host(), dev(1)], 2), lambda: raw([dev(0), host()], 2),               # sinks of both kinds
        # device extents that overlap: the same address, one byte shared, one inside the other
        lambda: call(dsts=[good[0], (good[0][0], i420(1)), good[2]]),
        lambda: call(dsts=[good[0], (good[0][0] + i420(0) - 1, i420(1)), good[2]]),
        lambda: call(dsts=[(good[2][0] + 64, i420(0)), good[1], good[2]]),
    ]
    for k, c in enumerate(bad):
        assert c() == -1, k
        assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0, k
    gl.WrhipSetShard(0, 2)
    assert call() == -1 and gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    gl.WrhipSetShard(0, 1)
    gl.WrhipSetTargetRows(win, 0, 256)
    assert call() == -1 and gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    gl.WrhipSetTargetRows(win, 0, 0)
    # the other grab calls keep rejecting the ticket's flags
    assert gl.grab_texture(win, [(0, 0, 4, 4)], gys.YUV | gys.SCALED) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert gl.grab_texture_scaled(win, full, (64, 64), gys.YUV) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert gl.grab_texture_yuv(win, full, I420, 0, gys.SCALED) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert s.stats()["kernel_launches"] == n0 and s.stats()["flushes"] == f0
    assert (gl.device_read(buf, 3 * room) == GUARD).all()
    # good calls: renditions that touch without sharing a byte; strides given with exactly the bytes they need
    assert call(dsts=[(buf, i420(0)), (buf + i420(0), i420(1)), (buf + i420(0) + i420(1), i420(2))]) >= 0
    assert s.stats()["kernel_launches"] == n0 + 1 and gl.GetError() == 0
    assert call(n=1, strides=[(80, 40)], dsts=[(buf, 64 * 80 + 63 * 40 + 32)]) >= 0 and gl.GetError() == 0
    assert call(n=1, strides=[(80, 40)], dsts=[(buf, 64 * 80 + 63 * 40 + 32 - 1)]) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    # a scaled YUV ticket delivers tight: a dst_stride is rejected; the new field is 0 for any other grab
    t = call(dsts=None, n=2)
    payload = i420(0) + i420(1)
    hostbuf = np.full(payload, GUARD, np.uint8)
    out = glapi.WrhipGrabInfo()
    assert gl.WrhipGrabResultGet(t, C.byref(out), hostbuf.ctypes.data, 64, 1) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert (hostbuf == GUARD).all()
    assert gl.WrhipGrabResultGet(t, C.byref(out), hostbuf.ctypes.data, 0, 1) == 0 and out.bytes == fg.HEADER + payload and out.renditions == 2
    for other in (gl.grab_texture(win, (0, 0, 4, 4)), gl.grab_texture_scaled(win, full, (64, 64)), gl.grab_texture_yuv(win, (0, 0, 4, 4), I420, 0)):
        assert gl.grab_result(other)[0]["renditions"] == 0
    gl.device_free(buf)
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 7. CPU only: the kernel's budget

def test_grab_scale_yuv_kernel_has_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    assert "wr_grab_scale_yuv_kernel" in notes, sorted(notes)
    vgprs, scratch = notes["wr_grab_scale_yuv_kernel"]
    assert scratch == 0, (vgprs, scratch)


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name", list(CASES))
def test_hostsim_case(hostsim, oracle_gcc, name):
    _case(hostsim, oracle_gcc, name)


def test_hostsim_all_spaces(hostsim, oracle_gcc):
    _all_spaces(hostsim, oracle_gcc)


def test_hostsim_clamp(hostsim, oracle_gcc):
    _clamp(hostsim, oracle_gcc)


def test_hostsim_equivalence(hostsim, oracle_gcc):
    _equivalence(hostsim, oracle_gcc)


def test_hostsim_geometry(hostsim, oracle_gcc):
    _geometry(hostsim, oracle_gcc)


def test_hostsim_later_upload(hostsim, oracle_gcc):
    _later_upload(hostsim, oracle_gcc)


def test_hostsim_rendered_frame(hostsim, oracle_gcc):
    _rendered_frame(hostsim, oracle_gcc)


def test_hostsim_ring(hostsim, oracle_gcc):
    _ring(hostsim, oracle_gcc)


def test_hostsim_free_and_put(hostsim, oracle_gcc):
    _free_and_put(hostsim, oracle_gcc)


def test_hostsim_stream(hostsim, oracle_gcc):
    _stream(hostsim, oracle_gcc)


def test_hostsim_contract(hostsim):
    _contract(hostsim)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_case(name):
    _case(wrhip_lib(), _gpu_ref(), name)


@pytest.mark.gpu
def test_gpu_all_spaces():
    _all_spaces(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_clamp():
    _clamp(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_equivalence():
    _equivalence(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_geometry():
    _geometry(wrhip_lib(), _gpu_ref())


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
def test_gpu_free_and_put():
    _free_and_put(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_stream():
    _stream(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_contract():
    _gpu_ref()
    _contract(wrhip_lib())
