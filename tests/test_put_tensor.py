"""Tensor puts (include/wrhip.h: WrhipPutTextureTensor): a CHW / HWC tensor of U8, F16, BF16 or F32 elements in the caller's device
memory converted on the device into the stored bytes of a rect of an RGBA8, R8 or RG8 texture, in draw order, in one launch.
Truth is the ORACLE: the same call script runs on swgl with every put replaced by TexSubImage2D of the bytes a numpy restatement of
the contract gives (tests/put_tensor.py).  Textures are read back WHOLE and compared, so the bytes outside the rect are checked too:
0 differing bytes, no tolerance anywhere.  Each check runs on the host simulation and, under -m gpu, on the MI355X."""
import ctypes as C
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
import frame_grabs as fg
import frame_taps as ft
import grab_tensor as gt
import hazard_cases as hz
import put_tensor as pt
from put_tensor import U8, F16, BF16, F32, CHW, HWC, BGR, FLIP
from test_grab_tensor import RECTS, R8W, R8H, DTYPES, LAYOUTS, _oracle_stored
from test_grab_scaled import STREAM_SEEDS, W, H, _noise, _frame
from webrender_amd import glapi, glconst as G
from webrender_amd.harness import render_streamed_fed

RG8W, RG8H = 67, 5
FLAGS = (0, BGR, FLIP, BGR | FLIP)
_want = {}


def _both(lib, ref, key, script):
    """`script(backend)` -> {name: array} on libwrhip and -- once per session -- on the oracle: every array must be equal"""
    if (ref, key) not in _want:
        _want[(ref, key)] = script(ref)
    want, got = _want[(ref, key)], script(lib)
    assert list(want) == list(got) and len(want) >= 1
    bad = [f"{k}: {pt.differing(got[k], want[k])} bytes differ" for k in want if not np.array_equal(got[k], want[k])]
    assert not bad, f"{key}: {bad[:8]} ({len(bad)} of {len(want)})"
    return want


def _seed(*parts):
    return [sum(ord(ch) for ch in str(p)) for p in parts]


# ---------------------------------------------------------------------------- 1. the matrix

def _matrix_script(name):
    rect = RECTS[name]

    def script(lib):
        s = pt.Session(lib)
        tex = s.make(_noise(), G.GL_RGBA8)
        s.r.finish()
        out = {}
        for dtype in DTYPES:
            for layout in LAYOUTS:
                for ch in (3, 4):
                    rng = np.random.default_rng(_seed(name, dtype, layout, ch))
                    for flags in FLAGS:
                        t = pt.tensor(rng, rect[2], rect[3], dtype, layout, ch)
                        assert pt.covers_the_rule(t, dtype, layout)
                        what = f"{name} {dtype} {layout} {ch} {flags}"
                        s.put(tex, rect, t, dtype, layout, alpha=0x5A + flags % 7, flags=flags, what=what)
                        out[what] = s.read(tex)
        assert s.gl.GetError() == 0
        s.close()
        return out
    return script


def _matrix(lib, ref, name):
    _both(lib, ref, ("matrix", name), _matrix_script(name))


def _small_script(fmt, w, h, ch):
    def script(lib):
        s = pt.Session(lib)
        tex = s.make(fg.noise(h, w, G.GL_R8, 611) if fmt == G.GL_R8 else np.random.default_rng(612).integers(0, 256, (h, w, 2), dtype=np.uint8), fmt)
        s.r.finish()
        out = {}
        for rect in ((0, 0, w, h), (7, 1, w - 17, h - 2)):
            for dtype in DTYPES:
                for layout in LAYOUTS:
                    rng = np.random.default_rng(_seed(fmt, rect, dtype, layout))
                    for flags in FLAGS:
                        t = pt.tensor(rng, rect[2], rect[3], dtype, layout, ch)
                        what = f"{rect} {dtype} {layout} {flags}"
                        s.put(tex, rect, t, dtype, layout, flags=flags, what=what)
                        out[what] = s.read(tex)
        assert s.gl.GetError() == 0
        s.close()
        return out
    return script


def _r8(lib, ref):
    _both(lib, ref, "r8", _small_script(G.GL_R8, R8W, R8H, 1))


def _rg8(lib, ref):
    _both(lib, ref, "rg8", _small_script(G.GL_RG8, RG8W, RG8H, 2))


# ---------------------------------------------------------------------------- 2. every value

EPS = np.float32(2.0 ** -23)
FUSED_SCALE, FUSED_BIAS = np.float32(1.0) + np.float32(3.0) * EPS, np.float32(-2.0 ** 20)
# (scale, bias) for the single channel of an R8 put: as they are; subnormals brought into range; large values brought into range
HALF_SETTINGS = {F16: ((1.0, 0.0), (2.0 ** 22, 0.25), (2.0 ** -8, -1.5)), BF16: ((1.0, 0.0), (2.0 ** 126, 0.5), (2.0 ** -120, -2.0))}
F32_SETTINGS = ((1.0, 0.0), (float(FUSED_SCALE), float(FUSED_BIAS)), (2.0 ** 127, 0.25))


def _f32_bits():
    """128 x 64 float32 patterns: every tie k + 0.5 with the floats next to it, zeros, subnormals, infinities, NaNs quiet and
    signalling of both signs, 255 and its neighbours, 1e30, the multiples of 1 / 8 from 2^20 on (what FUSED_SCALE and FUSED_BIAS
    bring to ties a fused multiply-add rounds the other way), and seeded random bits"""
    ties = (np.arange(255, dtype=np.float32) + np.float32(0.5)).view(np.uint32)
    v255 = np.array([255.0], np.float32).view(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x7F800000, 0xFF800000,
                        0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC12345, 0x7F800001, 0xFF800001, 0x7FA00000, 0xFFA00000, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32)
    big = np.array([1e30, -1e30], np.float32).view(np.uint32)
    steps = (np.float32(2.0 ** 20) + np.arange(2048, dtype=np.float32) * np.float32(0.125)).view(np.uint32)
    fixed = np.concatenate([ties - 1, ties, ties + 1, v255 - 1, v255, v255 + 1, special, big, steps])
    rnd = np.random.default_rng(23).integers(0, 1 << 32, 128 * 64 - len(fixed), dtype=np.uint64).astype(np.uint32)
    return np.concatenate([fixed, rnd]).reshape(1, 64, 128)


def _values_script(lib):
    s = pt.Session(lib)
    out = {}
    big = s.make(np.zeros((256, 256), np.uint8), G.GL_R8)
    small = s.make(np.zeros((64, 128), np.uint8), G.GL_R8)
    s.r.finish()
    every = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    for dtype in (F16, BF16):
        for scale, bias in HALF_SETTINGS[dtype]:
            s.put(big, (0, 0, 256, 256), every, dtype, CHW, scale=[scale], bias=[bias], what=f"{dtype} {scale} {bias}")
            out[f"every {dtype} {scale} {bias}"] = s.read(big)
    for scale, bias in F32_SETTINGS:
        layout = HWC if scale == 1.0 else CHW
        bits = _f32_bits().reshape((1, 64, 128) if layout == CHW else (64, 128, 1))
        s.put(small, (0, 0, 128, 64), bits, F32, layout, scale=[scale], bias=[bias], what=f"f32 {scale} {bias}")
        out[f"f32 {scale} {bias}"] = s.read(small)
    assert s.gl.GetError() == 0
    s.close()
    return out


def _values(lib, ref):
    want = _both(lib, ref, "values", _values_script)
    # the expectation alone: it holds 0, 255, a tie rounded down and a tie rounded up ...
    bits = _f32_bits()
    with np.errstate(invalid="ignore"):
        y = pt.to_f32(bits, F32).astype(np.float64)[0]
    b = want["f32 1.0 0.0"]
    assert (b == 0).any() and (b == 255).any()
    assert b[y == 2.5].tolist() == [2] and b[y == 3.5].tolist() == [4] and b[y == 0.5].tolist() == [0]
    assert (b[np.isnan(y)] == 0).all() and np.isnan(y).sum() >= 10 and (b[y < 0] == 0).all() and (b[y >= 255] == 255).all()
    for dtype in (F16, BF16):
        for scale, bias in HALF_SETTINGS[dtype]:
            e = want[f"every {dtype} {scale} {bias}"]
            # (bfloat16 has 8 significant bits: above 128 it holds the even numbers only)
            assert (e == 0).any() and (e == 255).any() and len(np.unique(e)) >= (256 if dtype == F16 else 128), (dtype, scale)
    # ... and a fused multiply-add would have given other bytes: the product kept exact (float64 holds it), one rounding at the end
    with np.errstate(invalid="ignore", over="ignore"):
        x = pt.to_f32(bits, F32).astype(np.float64)[0]
        fused = pt.byte_of((x * np.float64(FUSED_SCALE) + np.float64(FUSED_BIAS)).astype(np.float32))
    assert int((fused != want[f"f32 {float(FUSED_SCALE)} {float(FUSED_BIAS)}"]).sum()) >= 64


# ---------------------------------------------------------------------------- 3. geometry

def _geometry_script(lib):
    s = pt.Session(lib)
    tex = s.make(_noise(), G.GL_RGBA8)
    r8 = s.make(fg.noise(R8H, R8W, G.GL_R8, 611), G.GL_R8)
    s.r.finish()
    out = {}
    # rects at odd x, narrower than one 16-byte piece, on the texture's last column and row
    rects = [(3, 5, 61, 37), (1, 2, 64, 3), (329, 7, 1, 11), (330, 190, 3, 11), (331, 0, 2, 201), (233, 101, 100, 100), (0, 200, 333, 1)]
    k = 0
    for rect in rects:
        w, h = rect[2], rect[3]
        for dtype in DTYPES:
            per16 = 16 // pt.ELEM[dtype]
            for layout, c in ((CHW, 3), (HWC, 4), (CHW, 4), (HWC, 3)):
                tight = w if layout == CHW else w * c
                odd = tight + 3 if layout == CHW else tight + 1
                wide = (tight + per16 - 1) // per16 * per16 + per16      # rows that stay 16-byte aligned, with padding behind them
                geoms = [dict(off=1), dict(off=3), dict(row=odd), dict(off=1, row=odd), dict(row=wide)]
                if layout == CHW:
                    geoms += [dict(plane=h * w + 5), dict(off=3, row=odd, plane=(h - 1) * odd + w), dict(row=wide, plane=h * wide + per16)]
                g = geoms[k % len(geoms)]                                  # (every geometry meets every format over the rects)
                k += 1
                for g in (g, geoms[(k * 5) % len(geoms)]):
                    rng = np.random.default_rng(_seed(rect, dtype, layout, c, sorted(g.items())))
                    t = pt.tensor(rng, w, h, dtype, layout, c)
                    what = f"{rect} {dtype} {layout} {c} {g}"
                    s.put(tex, rect, t, dtype, layout, alpha=17, flags=FLIP if k % 3 == 0 else 0, what=what, **g)
                    out[what] = s.read(tex)
    for g in (dict(off=1), dict(off=3, row=R8W + 3), dict(row=64 + 16)):
        for dtype in DTYPES:
            rect = (5, 3, 50, 30)
            t = pt.tensor(np.random.default_rng(_seed(dtype, sorted(g.items()))), 50, 30, dtype, CHW, 1)
            s.put(r8, rect, t, dtype, CHW, what=f"r8 {dtype} {g}", **g)
            out[f"r8 {dtype} {g}"] = s.read(r8)
    assert s.gl.GetError() == 0
    s.close()
    return out


def _geometry(lib, ref):
    _both(lib, ref, "geometry", _geometry_script)


# ---------------------------------------------------------------------------- 4. rejections, WrhipDeviceWrite

def _contract(lib):
    s = pt.Session(lib, W, H)
    gl = s.gl
    px = _noise()
    tex = s.make(px, G.GL_RGBA8)
    r8 = s.make(fg.noise(R8H, R8W, G.GL_R8, 611), G.GL_R8)
    rg8 = s.make(np.zeros((RG8H, RG8W, 2), np.uint8), G.GL_RG8)
    f32 = s.d.create_texture(8, 8, G.GL_RGBA32F)
    nostorage = gl.gen("GenTextures")
    host = np.zeros((8, 8, 4), np.uint8)
    backed = gl.gen("GenTextures")
    gl.SetTextureBuffer(backed, G.GL_RGBA8, 8, 8, 32, host.ctypes.data, 8, 8)
    locked = s.make(np.zeros((8, 8, 4), np.uint8), G.GL_RGBA8)
    s.r.finish()
    lock = gl.LockTexture(locked.id)
    assert lock and gl.GetError() == 0
    buf = gl.device_alloc(1 << 20)
    n0, f0, h0 = (s.stats()[k] for k in ("kernel_launches", "flushes", "h2d_bytes"))

    def call(tex=tex.id, rect=(0, 0, 64, 32), src=buf, src_bytes=1 << 20, **kw):
        return gl.put_texture_tensor(tex, rect, src, src_bytes, **kw)
    rect4 = (C.c_int32 * 4)(0, 0, 64, 32)
    bad = [
        lambda: call(tex=9999), lambda: call(tex=0), lambda: call(tex=nostorage, rect=(0, 0, 1, 1)),      # unknown texture, no storage
        lambda: call(tex=f32.id, rect=(0, 0, 8, 8), channels=4),              # a format other than RGBA8, R8, RG8
        lambda: call(tex=backed, rect=(0, 0, 8, 8)),                          # storage that is a caller's host buffer
        lambda: call(tex=locked.id, rect=(0, 0, 8, 8)),                       # a locked texture
        lambda: call(channels=1), lambda: call(channels=2), lambda: call(channels=5), lambda: call(channels=0),      # channels against the format
        lambda: call(tex=r8.id, rect=(0, 0, 8, 8), channels=3), lambda: call(tex=r8.id, rect=(0, 0, 8, 8), channels=2),
        lambda: call(tex=rg8.id, rect=(0, 0, 8, 4), channels=1), lambda: call(tex=rg8.id, rect=(0, 0, 8, 4), channels=3),
        lambda: call(rect=(0, 0, 0, 4)), lambda: call(rect=(0, 0, 4, 0)), lambda: call(rect=(0, 0, -4, 4)),       # empty
        lambda: call(rect=(330, 0, 4, 1)), lambda: call(rect=(0, -1, 4, 4)), lambda: call(rect=(0, 200, 4, 2)), lambda: call(rect=(-1, 0, 4, 4)),
        lambda: call(dtype=4), lambda: call(layout=2),
        lambda: call(flags=glapi.GRAB_SWAP_RB), lambda: call(flags=glapi.GRAB_DELTA), lambda: call(flags=glapi.GRAB_TENSOR), lambda: call(flags=512),
        lambda: gl.WrhipPutTextureTensor(tex.id, C.addressof(rect4), None),   # no desc
        lambda: call(src=0),                                                  # no source
        lambda: call(dtype=F16, src=buf + 1), lambda: call(dtype=F32, src=buf + 2),      # not aligned to its element
        lambda: call(strides=(63, 0)), lambda: call(strides=(64, 31 * 64 + 63)), lambda: call(strides=(-64, 0)),      # strides below their minimum
        lambda: call(layout=HWC, strides=(64 * 3 - 1, 0)),
        lambda: call(strides=((1 << 40) + 1, 0), src_bytes=1 << 62), lambda: call(strides=(64, (1 << 40) + 1), src_bytes=1 << 62),
        lambda: call(dtype=F32, src_bytes=3 * 32 * 64 * 4 - 1),               # the extent does not fit
        lambda: call(dtype=F32, strides=(100, 5000), src_bytes=(2 * 5000 + 31 * 100 + 64) * 4 - 1),
        lambda: call(alpha=256),
    ]
    for k, c in enumerate(bad):
        assert c() == -1, k
        assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0, k
    gl.WrhipSetShard(0, 2)
    assert call() == -1 and gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    gl.WrhipSetShard(0, 1)
    gl.WrhipSetTargetRows(tex.id, 0, 100)
    assert call() == -1 and gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    gl.WrhipSetTargetRows(tex.id, 0, 0)
    st = s.stats()
    assert (st["kernel_launches"], st["flushes"], st["h2d_bytes"]) == (n0, f0, h0)
    gl.UnlockResource(lock)
    assert np.array_equal(s.read(tex), px)
    # WrhipDeviceWrite: NULL pointers, an empty copy, h2d_bytes, and what it wrote
    data = np.random.default_rng(9).integers(0, 256, 4096, dtype=np.uint8)
    h1 = s.stats()["h2d_bytes"]
    assert gl.WrhipDeviceWrite(None, data.ctypes.data, 16) == -1 and gl.WrhipDeviceWrite(buf, None, 16) == -1
    assert gl.WrhipDeviceWrite(None, None, 0) == 0 and s.stats()["h2d_bytes"] == h1
    gl.device_write(buf + 16, data)
    assert s.stats()["h2d_bytes"] == h1 + 4096 and np.array_equal(gl.device_read(buf + 16, 4096), data)
    # one good call: exactly the bytes it needs, strides given
    n1 = s.stats()["kernel_launches"]
    assert call(dtype=F32, strides=(100, 5000), src_bytes=(2 * 5000 + 31 * 100 + 64) * 4) == 0
    assert s.stats()["kernel_launches"] == n1 + 1 and gl.GetError() == 0
    gl.device_free(buf)
    s.r.finish()
    assert gl.GetError() == 0
    s.close()


def _kernel_stats(lib):
    """WrhipGetKernelStats reports a put as kind 16 with the texture's format and the elements read plus the bytes written"""
    s = pt.Session(lib)
    gl = s.gl
    tex = s.make(_noise(), G.GL_RGBA8)
    s.r.finish()
    gl.WrhipSetProfiling(1)
    rect = RECTS["inner"]
    s.put(tex, rect, pt.tensor(np.random.default_rng(1), rect[2], rect[3], F16, CHW, 3), F16, CHW)
    ks = (glapi.WrhipKernelStat * 64)()
    n = gl.WrhipGetKernelStats(ks, 64)
    puts = [k for k in ks[:n] if k.kind == 16]
    gl.WrhipSetProfiling(0)
    assert len(puts) == 1 and puts[0].launches == 1 and puts[0].feat == 0, [(k.kind, k.launches) for k in ks[:n]]
    assert puts[0].algo_bytes == rect[2] * rect[3] * (3 * 2 + 4), puts[0].algo_bytes
    s.close()


# ---------------------------------------------------------------------------- 5. hazards: the two groups of tests/hazard_cases.py

def _script_put(s, ref, x, y, tens, dtype, layout, **kw):
    """A put into the texture of TextureRef `ref` on a hazard_cases.Script: TexSubImage2D of the restatement's bytes on the oracle"""
    h, w = (tens.shape[1:] if layout == CHW else tens.shape[:2])
    if not s.wrhip:
        s.upload(ref, x, y, pt.expected(tens, dtype, layout, ref.fmt, **kw))
        return
    src = pt.Src(s.gl, tens, dtype, layout)
    assert pt.put(s.gl, s.tex(ref).id, (x, y, w, h), src, **kw) == 0, s.gl.GetError()
    src.free()


def _patch(seed, w, h, dtype=F16, layout=CHW, ch=4):
    return pt.tensor(np.random.default_rng(seed), w, h, dtype, layout, ch), dtype, layout


def p1_sampled_then_put(s):
    f = hz.image_frame(nearest=False, render_target=True)
    s.begin(f)
    s.draw(hz.retarget(f.tile, "T0"))
    s.write()
    _script_put(s, f.atlas, 37, 21, *_patch(91, 123, 77))
    s.draw(hz.retarget(f.tile, "T1"))
    s.keep["atlas"] = f.atlas


def p2_target_then_put(s):
    """A put into a render target that has recorded draws, then a draw over it that loads its content"""
    a1 = hz.decoration_target(151)
    s.begin(hz.image_frame(seed=9, n=4, atlas=512), statics=False)
    s.draw(a1, keep=False)
    s.write()
    _script_put(s, a1.texture, 41, 33, *_patch(92, 131, 59, BF16, HWC, 3), alpha=200)
    a2 = hz.decoration_target(152)
    a2.texture, a2.clear_color = a1.texture, None
    s.draw(a2)


PENDING = {"p1_sampled_then_put": (p1_sampled_then_put, [("T0", "T1")]), "p2_target_then_put": (p2_target_then_put, [])}


def _run_pending(lib, name):
    s = hz.Script(lib)
    PENDING[name][0](s)
    return s.finish()


def _pending(lib, ref, name):
    if (ref, name) not in _want:
        _want[(ref, name)] = _run_pending(ref, name)
    want, got = _want[(ref, name)], _run_pending(lib, name)
    assert int(want["gl_error"]) == 0 and int(got["gl_error"]) == 0
    for before, after in PENDING[name][1]:
        assert not np.array_equal(want[before], want[after]), f"{name}: the oracle draws {before} and {after} alike"
    writes = got["flushes_at_write"]
    assert len(writes) >= 1 and (writes == got["flushes_first_draw"]).all(), f"{name}: flushed before the put ({got['flushes_first_draw']} -> {writes})"
    names = [k for k in want if k != "gl_error"]
    bad = [f"{k}: {pt.differing(got[k], want[k])} bytes differ" for k in names if not np.array_equal(got[k], want[k])]
    assert names and not bad, f"{name}: {bad}"


def _upload_orders_script(lib):
    """A queued, unflushed TexSubImage2D and a put that overlap, in both orders; a tap and a grab issued before a put"""
    s = pt.Session(lib)
    px = _noise()
    tex = s.make(px, G.GL_RGBA8)
    s.r.finish()
    out = {}
    patch = fg.noise(60, 90, G.GL_RGBA8, 5)
    t, dtype, layout = _patch(93, 100, 50, F32, HWC, 4)
    s.write(tex, 20, 30, patch)
    s.put(tex, (70, 50, 100, 50), t, dtype, layout, quiet=False)
    out["upload_put"] = s.read(tex)
    t, dtype, layout = _patch(94, 100, 50, U8, CHW, 3)
    s.put(tex, (10, 60, 100, 50), t, dtype, layout, alpha=9)
    s.write(tex, 20, 30, patch[::-1])
    out["put_upload"] = s.read(tex)
    if s.wrhip:
        # a tap and a grab before the put keep the old bytes; a tap after it sees the new ones
        old = out["put_upload"]
        tap0, grab0 = s.gl.tap_texture(tex.id), s.gl.grab_texture(tex.id)
        t, dtype, layout = _patch(95, 333, 201, BF16, CHW, 4)
        s.put(tex, (0, 0, 333, 201), t, dtype, layout)
        tap1 = s.gl.tap_texture(tex.id)
        new = pt.expected(t, dtype, layout, G.GL_RGBA8)
        assert not np.array_equal(old, new)
        assert tuple(s.gl.tap_result(tap0)["digest"]) == ft.digest(old) and tuple(s.gl.tap_result(tap1)["digest"]) == ft.digest(new)
        assert np.array_equal(s.gl.grab_result(grab0)[1], old)
        assert np.array_equal(s.read(tex), new)
    assert s.gl.GetError() == 0
    s.close()
    return out


def _upload_orders(lib, ref):
    _both(lib, ref, "upload_orders", _upload_orders_script)


def _held_frames():
    f = hz.image_frame(seed=17, n=16)

    def pre(k):
        rect = ((37, 21, 123, 77), (11, 90, 201, 55), (129, 3, 99, 141))[k - 1]
        t, dtype, layout = _patch(200 + k, rect[2], rect[3], (F16, U8, F32)[k - 1], (CHW, HWC, HWC)[k - 1], 4)
        return lambda s: _script_put(s, f.atlas, rect[0], rect[1], t, dtype, layout, flags=BGR if k == 2 else 0)
    return [(None, f)] + [(pre(k), f) for k in (1, 2, 3)]


def _held(lib, ref):
    """Streamed frames with WrhipFlushHeld, and puts into a texture the held-back launches read (hazard_cases' b1 with puts)"""
    if (ref, "held") not in _want:
        _want[(ref, "held")] = hz.Script(ref).stream(_held_frames())
    want, got = _want[(ref, "held")], hz.Script(lib).stream(_held_frames())
    assert int(want["gl_error"]) == 0 and int(got["gl_error"]) == 0
    n = 4
    for k in range(1, n):
        assert not np.array_equal(want["frame%d" % (k - 1)], want["frame%d" % k]), f"the oracle's frames {k - 1} and {k} are alike"
    assert got["held"].tolist() == [1] * n, got["held"].tolist()
    bad = [k for k in range(n) if tuple(int(v) for v in got["tap%d" % k]) != ft.digest(ft.window_stored(want["frame%d" % k]))]
    assert not bad, f"frames whose window is not the oracle's: {bad}"
    assert np.array_equal(got["window"], want["window"])


def _parked_source(lib, ref):
    """A put whose src is the destination of a PARKED tensor grab: the texture holds the grabbed frame, not the guard bytes"""
    px = _oracle_stored(ref)["cfg2"]
    s = pt.Session(lib, W, H)
    tex = s.make(np.zeros((H, W, 4), np.uint8), G.GL_RGBA8)
    s.r.finish()
    inv = np.full(4, np.float32(1.0) / np.float32(255.0), np.float32)
    zero = np.zeros(4, np.float32)
    s.r.render(_frame())
    d = gt.Dest(s.gl, (3, H, W), F16, CHW)
    t = gt.grab(s, s.window, (0, 0, W, H), d, scale=inv, bias=zero)
    assert s.gl.grab_result(t, wait=False) is None          # parked behind the held-back launches
    a = s.stats()
    assert s.gl.put_texture_tensor(tex.id, (0, 0, W, H), d.dst, d.dst_bytes, dtype=F16, layout=CHW, channels=3, scale=[255.0] * 4, alpha=77) == 0
    b = s.stats()
    assert b["h2d_bytes"] == a["h2d_bytes"] and b["d2h_bytes"] <= a["d2h_bytes"] + glapi.GRAB_HEADER
    assert s.gl.WrhipFlushHeld() == 0                       # what the grab was parked behind has left
    tensor = gt.expected(px, F16, CHW, 3, inv, zero)
    want = pt.expected(tensor, F16, CHW, G.GL_RGBA8, scale=[255.0] * 4, bias=zero, alpha=77)
    assert np.array_equal(want[:, :, :3], px[:, :, :3])     # (a byte survives the round trip through float16)
    got = s.read(tex)
    assert np.array_equal(got, want), f"{pt.differing(got, want)} bytes differ"
    d.free()
    s.r.finish()
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 6. the closed loop

def _loop_frame(seed):
    """hazard_cases.image_frame on a window-sized atlas, under its 16 small images one large one of the WHOLE atlas, scaled down a
    little: what is fed back stays in view frame after frame"""
    f = hz.image_frame(seed=seed, n=16, atlas=W)
    step = f.tile.alpha[0]
    addr = f.gpu_cache.push([[0.0, 0.0, float(W), float(H)], [0.0, 0.0, 0.0, 0.0]])
    spec = f.gpu_cache.push([[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [-1.0, -1.0, 0.0, 0.0]])
    task = f.add_render_task((0.0, 0.0, float(W), float(H)), 1.0, (0.0, 0.0))
    ph = f.add_prim_header((37.0, 21.0, 37.0 + 438.0, 21.0 + 470.0), (-hz.BIG, -hz.BIG, hz.BIG, hz.BIG), 1, spec, 0, task,
                           (4 | (1 << 16), 0, int(round(0.9 * 65535.0)), 0))
    row = np.array([f.brush_instance(ph, hz.CLIP_TASK_EMPTY, resource_address=addr)], dtype=np.int32)
    step.instances = np.concatenate([row, step.instances])
    return f


def _loop_frames():
    return [_loop_frame(sd) for sd in STREAM_SEEDS[:4]]


def _loop(lib, ref):
    first = hz.image_pixels(3, W)
    if (ref, "loop") not in _want:
        _want[(ref, "loop")] = render_streamed_fed(ref, _loop_frames(), "hz_atlas", initial=first)[0]
    want = _want[(ref, "loop")]
    assert len(want) == 4 and all(not np.array_equal(want[k], want[k + 1]) for k in range(3))
    got, st = render_streamed_fed(lib, _loop_frames(), "hz_atlas", initial=first)
    assert st["gl_error"] == 0, st
    bad = [k for k in range(4) if not np.array_equal(got[k], want[k])]
    assert not bad, f"presented frames that are not the oracle's: {bad}"
    # the fed texture's bytes never come from the host: the loop uploads what the same loop without the feedback uploads
    off_images, off = render_streamed_fed(lib, _loop_frames(), "hz_atlas", feed=False, initial=first)
    assert off["gl_error"] == 0 and st["h2d_bytes"] == off["h2d_bytes"], (st["h2d_bytes"], off["h2d_bytes"])
    assert st["h2d_bytes"] < off["h2d_bytes"] + W * H * 4      # (one fed texture uploaded once would show)
    assert np.array_equal(off_images[0], want[0]) and not np.array_equal(off_images[1], want[1])      # (the feedback is seen from frame 1 on)


# ---------------------------------------------------------------------------- CPU only: the two conversions

CONV_SRC = r'''
#include <stdio.h>
#include <stdint.h>
#include "wr_tensor_round.h"
int main(int argc, char** argv) {
  FILE* out = fopen(argv[1], "wb");
  for (uint32_t h = 0; h < 65536; h++) { const uint32_t u = wr_f16_bits_to_f32_bits((uint16_t)h); fwrite(&u, 4, 1, out); }
  FILE* in = fopen(argv[2], "rb");
  uint32_t u;
  while (fread(&u, 4, 1, in) == 1) { const uint8_t b = wr_f32_bits_to_byte(u); fwrite(&b, 1, 1, out); }
  fclose(in); fclose(out);
  return 0;
}
'''


def test_conversion_helpers(tmp_path):
    """webrender_amd/csrc/wr_tensor_round.h, the integer arithmetic the host simulation compiles: every float16 pattern widened, and
    float32 -> byte on the constructed patterns and a million random ones, against numpy"""
    import os
    import subprocess
    from conftest import ROOT
    u = np.concatenate([_f32_bits().ravel(), np.random.default_rng(6).integers(0, 1 << 32, 1000000, dtype=np.uint64).astype(np.uint32),
                        np.random.default_rng(7).uniform(-1, 256, 500000).astype(np.float32).view(np.uint32)])
    (tmp_path / "c.cpp").write_text(CONV_SRC)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "webrender_amd", "csrc"), str(tmp_path / "c.cpp"), "-o", str(tmp_path / "c")])
    u.tofile(tmp_path / "in.bin")
    subprocess.check_call([str(tmp_path / "c"), str(tmp_path / "out.bin"), str(tmp_path / "in.bin")])
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    wide, got = raw[:65536 * 4].view(np.uint32), raw[65536 * 4:]
    want = pt.to_f32(np.arange(65536, dtype=np.uint16), F16)
    nan = np.isnan(want)
    assert np.array_equal(wide[~nan], want.view(np.uint32)[~nan])
    assert np.isnan(wide.view(np.float32)[nan]).all() and np.array_equal(wide[nan] >> 31, want.view(np.uint32)[nan] >> 31)
    assert len(got) == len(u) and np.array_equal(got, pt.byte_of(u.view(np.float32)))


def test_put_kernel_has_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    assert "wr_put_tensor_kernel" in notes, sorted(notes)
    assert notes["wr_put_tensor_kernel"][1] == 0, notes["wr_put_tensor_kernel"]


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name", list(RECTS))
def test_hostsim_matrix(hostsim, oracle_gcc, name):
    _matrix(hostsim, oracle_gcc, name)


def test_hostsim_r8(hostsim, oracle_gcc):
    _r8(hostsim, oracle_gcc)


def test_hostsim_rg8(hostsim, oracle_gcc):
    _rg8(hostsim, oracle_gcc)


def test_hostsim_every_value(hostsim, oracle_gcc):
    _values(hostsim, oracle_gcc)


def test_hostsim_geometry(hostsim, oracle_gcc):
    _geometry(hostsim, oracle_gcc)


def test_hostsim_contract(hostsim):
    _contract(hostsim)


def test_hostsim_kernel_stats(hostsim):
    _kernel_stats(hostsim)


@pytest.mark.parametrize("name", list(PENDING))
def test_hostsim_put_meets_recorded_draws(hostsim, oracle_gcc, name):
    _pending(hostsim, oracle_gcc, name)


def test_hostsim_put_and_queued_uploads(hostsim, oracle_gcc):
    _upload_orders(hostsim, oracle_gcc)


def test_hostsim_put_meets_held_launches(hostsim, oracle_gcc):
    _held(hostsim, oracle_gcc)


def test_hostsim_put_from_parked_grab(hostsim, oracle_gcc):
    _parked_source(hostsim, oracle_gcc)


def test_hostsim_closed_loop(hostsim, oracle_gcc):
    _loop(hostsim, oracle_gcc)


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
def test_gpu_r8():
    _r8(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_rg8():
    _rg8(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_every_value():
    _values(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_geometry():
    _geometry(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_contract():
    _gpu_ref()
    _contract(wrhip_lib())


@pytest.mark.gpu
def test_gpu_kernel_stats():
    _gpu_ref()
    _kernel_stats(wrhip_lib())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PENDING))
def test_gpu_put_meets_recorded_draws(name):
    _pending(wrhip_lib(), _gpu_ref(), name)


@pytest.mark.gpu
def test_gpu_put_and_queued_uploads():
    _upload_orders(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_put_meets_held_launches():
    _held(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_put_from_parked_grab():
    _parked_source(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_closed_loop():
    _loop(wrhip_lib(), _gpu_ref())
