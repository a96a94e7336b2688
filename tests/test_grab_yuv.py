"""YUV grabs (include/wrhip.h: WrhipGrabTextureYuv): a rect of an RGBA8 texture converted on the device, in one launch, into 8-bit
I420, NV12 or I444 planes of one of six ranged colour spaces -- delivered through the grab ring to the host, or written into the
caller's device memory.  Expected planes are computed in numpy (tests/grab_yuv.py, the table typed in from the contract) from the
ORACLE's stored bytes -- its upload or render read back -- and compared byte for byte: 0 differences, no tolerance anywhere.  Device
destinations and host buffers are filled with 0xA5 first and compared whole.  Each check runs on the host simulation and, under
-m gpu, on the MI355X."""
import ctypes as C
import itertools
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
import frame_grabs as fg
import grab_tensor as gt
import grab_yuv as gy
from grab_yuv import I420, NV12, I444, FORMATS, SPACES, FLIP, GUARD
from test_grab_scaled import STREAM_SEEDS, W, H, _noise, _frame
from test_grab_tensor import _oracle_stored
from webrender_amd import glapi, glconst as G, device
from webrender_amd.renderer import Renderer
from webrender_amd.harness import render_streamed, render_streamed_yuv

RECTS = {
    "full": (0, 0, 333, 201),
    "inner": (3, 5, 61, 37),                 # odd origin, odd sizes
    "corner": (233, 101, 100, 100),          # the texture's last column and row
    "thin": (328, 0, 5, 201),
    "short": (1, 2, 64, 3),
    "one": (10, 10, 1, 1),
    "pair": (0, 0, 2, 1),
}
CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]
RT_RECT = (7, 9, 66, 37)                     # the round trip's: 66 x 37
_cache = {}


# ---------------------------------------------------------------------------- 1. table and formula: pure CPU, no library

def test_table_is_its_derivation():
    for sp in SPACES:
        assert gy.derived_table(sp) == gy.TABLE[sp], sp
        y, cb, cr = gy.TABLE[sp]
        assert sum(y) == (65536 if gy.full_range(sp) else 56284) and sum(cb) == 0 and sum(cr) == 0, sp


def _solid(rgb, h=2, w=2):
    px = np.zeros((h, w, 4), np.uint8)
    px[..., 2], px[..., 1], px[..., 0], px[..., 3] = rgb[0], rgb[1], rgb[2], 255
    return px


def test_greys_corners_and_flat_blocks():
    g = np.arange(256)
    greys = np.stack([g, g, g, 255 - g], axis=-1).astype(np.uint8)[None]          # (1, 256, 4); alpha is anything
    for sp in SPACES:
        want_y = g if gy.full_range(sp) else 16 + (g * 219 * 2 + 255) // 510          # y0 + round(g * 219 / 255)
        assert np.array_equal(gy.luma(greys, sp)[0], want_y), sp
        for k in (1, 2):
            assert (gy.chroma444_raw(greys, sp, k) == 128).all() and (gy.chroma420_raw(greys, sp, k) == 128).all(), sp
        top = 0
        for c in CORNERS:
            px = _solid(c)
            y = int(gy.luma(px, sp)[0, 0])
            raw = [int(gy.chroma444_raw(px, sp, k)[0, 0]) for k in (1, 2)]
            # a flat 2 x 2 block gives I444's chroma, before and after the clamp
            assert [int(gy.chroma420_raw(px, sp, k)[0, 0]) for k in (1, 2)] == raw, (sp, c)
            if gy.full_range(sp):
                assert 0 <= y <= 255 and all(1 <= v <= 256 for v in raw), (sp, c, y, raw)      # (the lower bound of the clamp is never reached)
            else:
                assert 16 <= y <= 235 and all(16 <= v <= 240 for v in raw), (sp, c, y, raw)
            top = max(top, *raw)
        assert top == (256 if gy.full_range(sp) else 240), (sp, top)
        if gy.full_range(sp):
            for c, k in (((0, 0, 255), 1), ((255, 0, 0), 2)):                    # pure blue: Cb, pure red: Cr
                assert int(gy.chroma444_raw(_solid(c), sp, k)[0, 0]) == 256
                assert gy.planes(_solid(c), I444, sp)[k][0, 0] == 255


def test_within_one_of_the_real_formula():
    """no sample is further than 1 from the float64 formula rounded half up: cube corners, greys and noise"""
    px = np.concatenate([_noise()[:64, :64].reshape(-1, 4), np.array([(b, g, r, 255) for r, g, b in CORNERS], np.uint8)]).reshape(1, -1, 4)
    rgb = px[0, :, [2, 1, 0]].astype(np.float64)
    for sp in SPACES:
        y, cb, cr = gy.real_rows(sp)
        got = gy.planes(px, I444, sp)
        for k, (row, off) in enumerate(((y, gy.y0_of(sp)), (cb, 128), (cr, 128))):
            real = np.clip(np.floor(row @ rgb + off + 0.5), 0, 255)
            assert np.abs(got[k][0].astype(np.int64) - real).max() <= 1, (sp, k)


# ---------------------------------------------------------------------------- helpers

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
            "bytes": int(r.bytes), "scaled_w": r.scaled_w, "scaled_h": r.scaled_h, "levels": r.levels}
    return info, buf[:payload]


def _one(s, tex, rect, px, fmt, sp, flags=0, sink="host", what="", **geom):
    """One grab on a quiescent session, checked whole: `px` are the stored bytes of the rect.  One launch, no flush."""
    want = gy.planes(px, fmt, sp, flags)
    flat = np.concatenate([p.reshape(-1) for p in want])
    d = gy.Dest(s.gl, rect[2], rect[3], fmt, **geom) if sink == "device" else None
    a = s.stats()
    t = gy.grab(s, tex, rect, fmt, sp, flags, d)
    b = s.stats()
    assert b["kernel_launches"] == a["kernel_launches"] + 1 and b["flushes"] == a["flushes"], (what, a, b)
    if d is None:
        info, got = _fetch_host(s.gl, t, len(flat))
        gy.check_info(info, rect, flags, len(flat))
        assert int((got != flat).sum()) == 0, f"{what}: {int((got != flat).sum())} bytes of the payload differ"
    else:
        info, got = s.gl.grab_result(t)
        assert len(got) == 0
        gy.check_info(info, rect, flags, 0)
        d.check(want, what)
        d.free()


# ---------------------------------------------------------------------------- 2. the matrix

def _matrix(lib, ref, name):
    rect = RECTS[name]
    px = fg.crop(_oracle_stored(ref)["rgba"], rect)
    s, tex = _noise_session(lib)
    for fmt, sp, flags, sink in itertools.product(FORMATS, SPACES, (0, FLIP), ("host", "device")):
        _one(s, tex.id, rect, px, fmt, sp, flags, sink, what=f"{name} fmt {fmt} space {sp} flags {flags} {sink}")
    # the bytes that crossed: the header (word 0: the payload's bytes), then the planes
    t = gy.grab(s, tex.id, rect, NV12, 2)
    raw = s.gl.grab_payload(t)
    want = gy.expected(px, NV12, 2)
    assert len(raw) == fg.HEADER + len(want) and int.from_bytes(raw[:4], "little") == len(want)
    assert np.array_equal(np.frombuffer(raw[fg.HEADER:], np.uint8), want)
    info, flat = s.gl.grab_result(t)
    assert np.array_equal(flat, want)
    y, c = glapi.yuv_split(flat, rect[2], rect[3], NV12)
    assert y.shape == (rect[3], rect[2]) and c.shape == ((rect[3] + 1) // 2, (rect[2] + 1) // 2, 2)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 3. a constructed texture

def constructed():
    """64 x 8: the cube corners as flat 2 x 2 blocks, the same corners as single pixels in a checkerboard -- mixed sums --, and
    columns of alpha 0 and 255 over equal colours"""
    rng = np.random.default_rng(97)
    px = rng.integers(0, 256, (8, 64, 4), dtype=np.uint8)
    for k, (r, g, b) in enumerate(CORNERS):
        px[0:2, 2 * k:2 * k + 2] = (b, g, r, 255)
    for y in (2, 3):
        for x in range(64):
            r, g, b = CORNERS[(x + 3 * y) % 8]
            px[y, x] = (b, g, r, 17 * x % 256)
    px[4:8, 32:64, :3] = px[4:8, 0:32, :3]
    px[4:8, 0:32, 3] = 0
    px[4:8, 32:64, 3] = 255
    return px


def _oracle_constructed(ref):
    if (ref, "constructed") not in _cache:
        gl = glapi.GL(ref)
        r = Renderer(gl, 64, 64)
        px = constructed()
        tex = r.device.create_texture(64, 8, G.GL_RGBA8, render_target=True)
        r.device.upload_texture(tex, 0, 0, 64, 8, G.GL_BGRA, G.GL_UNSIGNED_BYTE, px)
        _cache[(ref, "constructed")] = r.device.read_texture(tex).copy()
        assert np.array_equal(_cache[(ref, "constructed")], px)
        r.destroy()
    return _cache[(ref, "constructed")]


def _constructed(lib, ref):
    px = _oracle_constructed(ref)
    opaque = px.copy()
    opaque[..., 3] = 255
    s = fg.Session(lib, 64, 64)
    tex = s.make(constructed(), G.GL_RGBA8)
    s.r.finish()
    for fmt, sp in itertools.product(FORMATS, SPACES):
        want = gy.planes(px, fmt, sp)
        # alpha does not matter; the halves with alpha 0 and 255 over equal colours give equal samples
        assert all(np.array_equal(a, b) for a, b in zip(want, gy.planes(opaque, fmt, sp)))
        assert np.array_equal(want[0][4:8, 0:32], want[0][4:8, 32:64])
        if gy.full_range(sp):
            # (chroma cannot fall below 1, test_greys_corners_and_flat_blocks: the clamp is live at the top only)
            below, above = gy.clamped(px, fmt, sp)
            assert below == 0 and above > 0 and all((p == 255).any() for p in want[1:]), (fmt, sp, below, above)
        for flags, sink in itertools.product((0, FLIP), ("host", "device")):
            _one(s, tex.id, (0, 0, 64, 8), px, fmt, sp, flags, sink, what=f"constructed fmt {fmt} space {sp} flags {flags} {sink}")
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 4. device-sink geometry

def _geometry(lib, ref):
    s, tex = _noise_session(lib)
    stored = _oracle_stored(ref)["rgba"]
    for name in ("inner", "short", "thin", "corner"):
        rect = RECTS[name]
        px = fg.crop(stored, rect)
        w = rect[2]
        for fmt in FORMATS:
            crow = gy.row_bytes(w, rect[3], fmt)[1][1]
            y16, c16 = (w + 15) // 16 * 16 + 16, (crow + 15) // 16 * 16 + 16
            geoms = [dict(off=1), dict(off=3), dict(off=16), dict(y_stride=w + 1), dict(y_stride=w + 13), dict(c_stride=crow | 1),
                     dict(off=3, y_stride=w + 13, c_stride=(crow + 2) | 1), dict(y_stride=y16, c_stride=c16),
                     dict(off=16, y_stride=y16 + 16, c_stride=c16), dict(y_stride=(w + 7) // 8 * 8, c_stride=(crow + 7) // 8 * 8 + 4)]
            for k, g in enumerate(geoms):
                _one(s, tex.id, rect, px, fmt, (k + fmt) % 6, FLIP if k % 2 else 0, "device", what=f"{name} fmt {fmt} {g}", **g)
    # dst_bytes: Dest passes exactly the extent (accepted above); a byte short is rejected and writes nothing
    rect = RECTS["inner"]
    n0, f0 = s.stats()["kernel_launches"], s.stats()["flushes"]
    for fmt in FORMATS:
        d = gy.Dest(s.gl, rect[2], rect[3], fmt, off=1, y_stride=rect[2] + 3)
        assert s.gl.grab_texture_yuv(tex.id, rect, fmt, 0, 0, dst=d.dst, dst_bytes=d.dst_bytes - 1, strides=d.strides) == -1
        assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0
        assert d.untouched()
        d.free()
    assert s.stats()["kernel_launches"] == n0 and s.stats()["flushes"] == f0
    s.close()


# ---------------------------------------------------------------------------- 5. ordering

def _later_upload(lib, ref):
    """A grab, then an upload over the rect: the grab is unchanged"""
    rect = RECTS["inner"]
    px = fg.crop(_oracle_stored(ref)["rgba"], rect)
    s, tex = _noise_session(lib)
    d = gy.Dest(s.gl, rect[2], rect[3], I420)
    th, td = gy.grab(s, tex.id, rect, NV12, 3), gy.grab(s, tex.id, rect, I420, 0, FLIP, d)
    s.upload(tex, 0, 0, fg.noise(60, 80, G.GL_RGBA8, 78))
    assert np.array_equal(s.gl.grab_result(th)[1], gy.expected(px, NV12, 3))
    s.gl.grab_result(td)
    d.check(gy.planes(px, I420, 0, FLIP), "device grab ahead of an upload")
    d.free()
    assert s.gl.GetError() == 0
    s.close()


def _rendered_frame(lib, ref):
    """The window behind its held-back launches, no Finish: both grabs are parked; a later write to the window is not seen"""
    px = _oracle_stored(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    s.r.render(_frame())
    rect = (0, 0, W, H)
    d = gy.Dest(s.gl, W, H, NV12)
    th = gy.grab(s, s.window, rect, I420, 2)            # (submits what was recorded; the frame's raster launches stay held back)
    a = s.stats()
    td = gy.grab(s, s.window, rect, NV12, 5, 0, d)
    assert s.gl.grab_result(th, wait=False) is None and s.gl.grab_result(td, wait=False) is None          # parked
    assert s.stats()["kernel_launches"] == a["kernel_launches"]          # (nothing left: neither a grab nor what it is parked behind)
    s.upload(device.Texture(s.window, W, H, G.GL_RGBA8), 100, 60, fg.noise(70, 40, G.GL_RGBA8, 77))
    info, flat = s.gl.grab_result(th)
    want = gy.expected(px, I420, 2)
    gy.check_info(info, rect, 0, len(want))
    assert int((flat != want).sum()) == 0
    gy.check_info(s.gl.grab_result(td)[0], rect, 0, 0)
    d.check(gy.planes(px, NV12, 5), "rendered frame, device")
    d.free()
    s.r.finish()
    assert s.gl.GetError() == 0
    s.close()


def _nine(s, px, parked, sink):
    """Nine grabs of the window without a fetch: the ring holds the 8 newest tickets.  Host sink: the first is dead, the other eight
    are exact.  Device sink: all nine buffers are written."""
    dests, tickets, wants = [], [], []
    for k in range(9):
        fmt, sp, flags = FORMATS[k % 3], k % 6, FLIP if k % 2 else 0
        rect = (7 * k, 11 * k, 100 + k, 20 + k)
        d = gy.Dest(s.gl, rect[2], rect[3], fmt, off=k % 2) if sink == "device" else None
        tickets.append(gy.grab(s, s.window, rect, fmt, sp, flags, d))
        dests.append(d)
        wants.append(gy.planes(fg.crop(px, rect), fmt, sp, flags))
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
        assert info["flags"] & gy.YUV
        if sink == "host":
            want = np.concatenate([p.reshape(-1) for p in wants[k]])
            assert int((flat != want).sum()) == 0, k
    for k, (d, want) in enumerate(zip(dests, wants)):
        if d is not None:
            d.check(want, f"grab {k}")
            d.free()


def _ring(lib, ref):
    px = _oracle_stored(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    for sink in ("host", "device"):
        s.r.render(_frame())
        _nine(s, px, True, sink)
        s.r.finish()
        _nine(s, px, False, sink)
    assert s.gl.GetError() == 0
    s.close()


def _free_and_put(lib, ref):
    px = _oracle_stored(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    gl = s.gl
    # WrhipDeviceFree of a buffer a parked grab writes: the grab is sent first (with what it is parked behind), and the call returns
    s.r.render(_frame())
    rect = (5, 6, 64, 32)
    d = gy.Dest(gl, 64, 32, I420)
    t = gy.grab(s, s.window, rect, I420, 1, 0, d)
    assert gl.grab_result(t, wait=False) is None
    d.free()
    assert gl.WrhipFlushHeld() == 0                     # nothing is held any more
    gy.check_info(gl.grab_result(t)[0], rect, 0, 0)
    s.r.finish()
    # a put that reads a parked grab's destination sees the grab's bytes: the Y plane of an I444 grab becomes an R8 texture
    r8 = s.d.create_texture(64, 32, G.GL_R8, render_target=True)
    s.upload(r8, 0, 0, np.zeros((32, 64), np.uint8))
    s.r.finish()
    s.r.render(_frame())
    d = gy.Dest(gl, 64, 32, I444)
    t = gy.grab(s, s.window, rect, I444, 3, 0, d)
    assert gl.grab_result(t, wait=False) is None
    assert gl.put_texture_tensor(r8.id, (0, 0, 64, 32), d.dst, 64 * 32, dtype=gt.U8, layout=gt.CHW, channels=1) == 0
    want = gy.planes(fg.crop(px, rect), I444, 3)
    assert np.array_equal(s.d.read_texture(r8), want[0])
    gl.grab_result(t)
    d.check(want, "the grab a put read from")
    d.free()
    s.r.finish()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 6. streamed

def _oracle_renders(ref):
    """The oracle's render of every frame of the stream: computed once, never modified"""
    if (ref, "renders") not in _cache:
        gl = glapi.GL(ref)
        r = Renderer(gl, W, H)
        out = {}
        for sd in STREAM_SEEDS:
            r.render(_frame(sd, 60))
            r.finish()
            out[sd] = r.device.read_texture(device.Texture(0, W, H, G.GL_RGBA8, fbo=0)).copy()
        r.destroy()
        _cache[(ref, "renders")] = out
    return _cache[(ref, "renders")]


def _stream(lib, ref):
    frames = lambda: [_frame(sd, 60) for sd in STREAM_SEEDS]
    _, plain = render_streamed(lib, frames())
    want = _oracle_renders(ref)
    for dev, fmt, sp in ((False, I420, 2), (True, NV12, 1)):
        planes, st, infos = render_streamed_yuv(lib, frames(), fmt, sp, device=dev)
        assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
        assert st["setup_carried"] == plain["setup_carried"] and st["setup_carried"] >= len(STREAM_SEEDS) - 1, (st, plain)
        assert len(planes) == len(infos) == len(STREAM_SEEDS)
        bad = [sd for k, sd in enumerate(STREAM_SEEDS)
               if not all(np.array_equal(a, b) for a, b in zip(planes[k], gy.planes(want[sd], fmt, sp)))]
        assert not bad, f"frames whose planes are not the restatement on the oracle's render: {bad}"
        payload = 0 if dev else len(gy.expected(want[STREAM_SEEDS[0]], fmt, sp))
        gy.check_info(infos[-1], (0, 0, W, H), 0, payload)


# ---------------------------------------------------------------------------- 7. the round trip through CompositeYUV

def round_trip(gl, d, planes, w, h, sp):
    """Y, Cb, Cr planes uploaded as R8 textures, locked and drawn with CompositeYUV at 8 bits into an RGBA8 texture of w x h: its
    stored bytes.  (CompositeYUV takes three planes of ONE format -- the reference asserts it --, so NV12's pairs are split.)"""
    texs = []
    for p in planes:
        t = d.create_texture(p.shape[1], p.shape[0], G.GL_R8, render_target=True)
        d.upload_texture(t, 0, 0, p.shape[1], p.shape[0], G.GL_RED, G.GL_UNSIGNED_BYTE, np.ascontiguousarray(p))
        texs.append(t)
    dst = d.create_texture(w, h, G.GL_RGBA8, render_target=True)
    d.upload_texture(dst, 0, 0, w, h, G.GL_BGRA, G.GL_UNSIGNED_BYTE, np.zeros((h, w, 4), np.uint8))
    ld = gl.LockTexture(dst.id)
    locks = [gl.LockTexture(t.id) for t in texs]
    gl.CompositeYUV(ld, locks[0], locks[1], locks[2], sp, 8, 0, 0, w, h, 0, 0, w, h, 0, 0, 0, 0, w, h)
    for l in locks:
        gl.UnlockResource(l)
    gl.UnlockResource(ld)
    out = d.read_texture(dst).copy()
    for t in texs + [dst]:
        d.delete_texture(t)
    return out


def _as_three(planes, fmt):
    return [planes[0], planes[1][..., 0], planes[1][..., 1]] if fmt == NV12 else planes


def _oracle_round_trips(ref):
    if (ref, "rt") not in _cache:
        px = fg.crop(_oracle_stored(ref)["rgba"], RT_RECT)
        gl = glapi.GL(ref)
        r = Renderer(gl, 64, 64)
        _cache[(ref, "rt")] = {(fmt, sp): round_trip(gl, r.device, _as_three(gy.planes(px, fmt, sp), fmt), RT_RECT[2], RT_RECT[3], sp)
                               for fmt in (I420, NV12) for sp in SPACES}
        r.destroy()
    return _cache[(ref, "rt")]


def _round_trip(lib, ref):
    want = _oracle_round_trips(ref)
    s, tex = _noise_session(lib)
    w, h = RT_RECT[2:]
    for fmt in (I420, NV12):
        for sp in SPACES:
            info, flat = s.gl.grab_result(gy.grab(s, tex.id, RT_RECT, fmt, sp))
            got = round_trip(s.gl, s.d, _as_three(glapi.yuv_split(flat, w, h, fmt), fmt), w, h, sp)
            assert int((got != want[(fmt, sp)]).sum()) == 0, (fmt, sp)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 8. the contract's rejections

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
    size = 1 << 16                                      # (room for every call below, the strided good one included)
    buf = gl.device_alloc(size)
    gt.fill(gl, buf, size)
    n0, f0 = s.stats()["kernel_launches"], s.stats()["flushes"]

    def call(tex=win, rect=(0, 0, 64, 32), fmt=I420, sp=0, flags=0, dst=buf, dst_bytes=64 * 32 * 3 // 2, strides=(0, 0)):
        return gl.grab_texture_yuv(tex, rect, fmt, sp, flags, dst=dst, dst_bytes=dst_bytes, strides=strides)
    rect4 = (C.c_int32 * 4)(0, 0, 64, 32)
    bad = [
        lambda: call(tex=9999),                                               # unknown texture
        lambda: call(tex=f32.id, rect=(0, 0, 8, 8)), lambda: call(tex=r8.id, rect=(0, 0, 8, 8)),      # not GL_RGBA8
        lambda: call(rect=(0, 0, 0, 4)), lambda: call(rect=(0, 0, 4, 0)),     # empty
        lambda: call(rect=(500, 0, 13, 1)), lambda: call(rect=(0, -1, 4, 4)), lambda: call(rect=(0, 500, 4, 13)),      # outside the texture
        lambda: call(fmt=3), lambda: call(sp=6), lambda: call(sp=7),          # unknown format; GbrIdentity and above
        lambda: call(flags=glapi.GRAB_SWAP_RB), lambda: call(flags=glapi.GRAB_DELTA), lambda: call(flags=gy.YUV), lambda: call(flags=glapi.GRAB_TENSOR),
        lambda: gl.WrhipGrabTextureYuv(win, C.addressof(rect4), None),        # no desc
        lambda: call(dst=None, strides=(64, 0)), lambda: call(dst=None, strides=(0, 32)), lambda: call(dst=None, dst_bytes=1, strides=(0, 0)),      # host sink
        lambda: call(strides=(63, 0)), lambda: call(strides=(0, 31)), lambda: call(strides=(-64, 0)),      # strides below their rows
        lambda: call(fmt=NV12, strides=(0, 63)), lambda: call(fmt=I444, strides=(0, 63)),
        lambda: call(strides=((1 << 40) + 1, 0), dst_bytes=1 << 62), lambda: call(strides=(0, (1 << 40) + 1), dst_bytes=1 << 62),
        lambda: call(dst_bytes=64 * 32 * 3 // 2 - 1),                         # the extent does not fit
        lambda: call(fmt=I444, dst_bytes=64 * 32 * 3 - 1),
        lambda: call(strides=(80, 40), dst_bytes=32 * 80 + 31 * 40 + 32 - 1),
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
    # the other grab calls reject 512
    assert gl.grab_texture(win, [(0, 0, 4, 4)], gy.YUV) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert gl.grab_texture_scaled(win, (0, 0, W, H), (64, 64), gy.YUV) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert s.stats()["kernel_launches"] == n0 and s.stats()["flushes"] == f0
    assert (gl.device_read(buf, size) == GUARD).all()
    # one good call with strides given and exactly the bytes it needs; a YUV ticket delivers tight: a dst_stride is rejected
    assert call(strides=(80, 40), dst_bytes=32 * 80 + 31 * 40 + 32) >= 0
    assert s.stats()["kernel_launches"] == n0 + 1 and gl.GetError() == 0
    t = call(dst=None, dst_bytes=0)
    payload = 64 * 32 * 3 // 2
    host = np.full(payload, GUARD, np.uint8)
    out = glapi.WrhipGrabInfo()
    assert gl.WrhipGrabResultGet(t, C.byref(out), host.ctypes.data, 64, 1) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert (host == GUARD).all()
    assert gl.WrhipGrabResultGet(t, C.byref(out), host.ctypes.data, 0, 1) == 0 and out.bytes == fg.HEADER + payload
    gl.device_free(buf)
    assert gl.GetError() == 0
    s.close()


def test_yuv_kernel_has_no_scratch_and_no_lds(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    assert "wr_grab_yuv_kernel" in notes, sorted(notes)
    vgprs, scratch = notes["wr_grab_yuv_kernel"]
    assert scratch == 0 and vgprs <= 64, (vgprs, scratch)          # (64: a streaming kernel keeps 8 waves per SIMD)


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name", list(RECTS))
def test_hostsim_matrix(hostsim, oracle_gcc, name):
    _matrix(hostsim, oracle_gcc, name)


def test_hostsim_constructed(hostsim, oracle_gcc):
    _constructed(hostsim, oracle_gcc)


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


def test_hostsim_round_trip(hostsim, oracle_gcc):
    _round_trip(hostsim, oracle_gcc)


def test_hostsim_contract(hostsim):
    _contract(hostsim)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RECTS))
def test_gpu_matrix(name):
    _matrix(wrhip_lib(), _gpu_ref(), name)


@pytest.mark.gpu
def test_gpu_constructed():
    _constructed(wrhip_lib(), _gpu_ref())


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
def test_gpu_round_trip():
    _round_trip(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_contract():
    _gpu_ref()
    _contract(wrhip_lib())
