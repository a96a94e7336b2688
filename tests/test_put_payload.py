"""Payload puts (include/wrhip.h: WrhipPutTexturePayload): a delta, packed or scroll payload decoded on the device into a texture rect,
in draw order, in one launch or two.  Expected bytes never come from the code under test: they are the numpy arrays the test
uploaded, what the numpy decoders of tests/grab_scroll.py and tests/grab_packed.py make of a payload, or what WrhipGrabDecode (which
has its own tests) leaves in a numpy image.  Textures are pre-filled with noise, read back WHOLE and compared byte for byte, so a
byte written outside a cut block fails: 0 differing bytes, no tolerance anywhere.  Each check runs on the host simulation and, under
-m gpu, on the MI355X."""
import ctypes as C
import os
import shutil
import subprocess
import numpy as np
import pytest
from conftest import ROOT, wrhip_lib, oracle_ref
import frame_grabs as fg
import frame_taps as ft
import grab_packed as gp
import grab_scroll as gs
import hazard_cases as hz
import put_payload as pp
from put_payload import DELTA, PACKED, SCROLL
from webrender_amd import glapi, glconst as G
from webrender_amd.harness import render_streamed_mirrored

# name: (texture w, texture h, rect): a pixel; a block; a one-pixel cut block beside and below one; odd sizes of several blocks; rows
# that are not 16-byte aligned in a texture whose stride is no multiple of 16; aligned stores
SIZES = {"1x1": (1, 1, (0, 0, 1, 1)), "64x64": (64, 64, (0, 0, 64, 64)), "65x64": (65, 64, (0, 0, 65, 64)), "64x65": (64, 65, (0, 0, 64, 65)),
         "67x129": (67, 129, (0, 0, 67, 129)), "130x70@3,5": (141, 83, (3, 5, 130, 70)), "200x200@16,0": (256, 256, (16, 0, 200, 200))}
_want = {}


def _inset(tex_px, rect, px):
    out = tex_px.copy()
    out[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = px
    return out


def _same(got, want, what):
    assert np.array_equal(got, want), f"{what}: {pp.differing(got, want)} bytes differ"


# ---------------------------------------------------------------------------- 1. round trip

def _round_trip(lib, size, bpp, mode):
    tw, th, rect = SIZES[size]
    case = list(SIZES).index(size) * 2 + (bpp == 1)
    frames = pp.sequence(rect[2], rect[3], bpp, case)
    assert len(frames) == 6 and all(not np.array_equal(frames[k], frames[k + 1]) for k in range(5))
    s = pp.Session(lib)
    gl = s.gl
    a = s.make_px(pp.noise(tw, th, bpp, 1))
    want = pp.noise(tw, th, bpp, 2)
    b = s.make_px(want)
    s.r.finish()
    copied = launches = 0
    for k, f in enumerate(frames):
        flags = pp.MODES[mode][k % len(pp.MODES[mode])]
        s.upload(a, rect[0], rect[1], f)
        t = gl.grab_texture(a.id, rect, flags)
        assert t >= 0, gl.GetError()
        payload = gl.grab_payload(t)
        info = gl.grab_result(t, into=np.zeros(pp.shape(rect[2], rect[3], bpp), np.uint8))[0]
        copied += info["copied"]
        # (the numpy decoder on the payload: what the put has to reproduce is what was uploaded)
        if flags & glapi.GRAB_PACKED:
            img = np.ascontiguousarray(fg.crop(want, rect)).copy()
            gs.decode(payload, img)
            _same(img, f, f"{size} {mode} frame {k}: the numpy decoder")
        launches += s.put(b, rect, payload, flags, what=f"{size} {mode} frame {k}")
        want = _inset(want, rect, f)
        _same(s.read(b), want, f"{size} {bpp} {mode} frame {k}")
    assert launches >= 6
    # (the scrolled frames of the tall rects reach the put as COPY entries: tests/test_grab_scroll.py pins when a grab finds a scroll)
    assert copied > 0 or mode != "scroll" or rect[3] < 129, (size, mode, copied)
    assert gl.GetError() == 0
    s.close()
    return copied


# ---------------------------------------------------------------------------- 2. constructed payloads

def _constructed_cases(bpp):
    """-> [(name, rect size, before, payload, flags)]: payloads no grab emits but the format allows"""
    out = []
    rng = np.random.default_rng(40 + bpp)
    w, h = 150, 200
    before = pp.noise(w, h, bpp, 41)
    img = gp.mixed_content(h, w, bpp, 42)
    recs = fg.blocks_of(w, h)
    packed = [gp.encode_block(img, r) for r in recs]
    plain = [pp.encode_plain(img, r) for r in recs]
    out.append(("packed reversed", before, pp.payload_of(packed[::-1]), PACKED))
    out.append(("packed shuffled", before, pp.payload_of([packed[i] for i in rng.permutation(len(recs))]), PACKED))
    out.append(("plain shuffled", before, pp.payload_of([plain[i] for i in rng.permutation(len(recs))]), DELTA))
    out.append(("plain, a few, off the grid", before, pp.payload_of([pp.encode_plain(img, r) for r in ((3, 5, 64, 64), (67, 5, 30, 64), (3, 69, 64, 1), (149, 199, 1, 1))]), DELTA))
    # COPY columns with |dy| < 64, both signs: every block whose source lies inside the rect is a COPY, the rest is sent, shuffled
    for dy in (7, 63, -1, -37, 64, -64, 65):
        ent = [gs.encode_copy(r) if 0 <= r[1] + dy and r[1] + dy + r[3] <= h else gp.encode_block(img, r) for r in recs]
        out.append((f"copy columns dy {dy}", before, pp.payload_of([ent[i] for i in rng.permutation(len(ent))], dy), SCROLL))
    # a COPY whose source is another entry's RUNS block (the COPY sees the bytes from before the put); a COPY and a SOLID of one block
    runs = gp.block_with_n_starts(300, bpp, 5)
    e_runs = np.frombuffer(gp.encode_block(_inset(np.zeros(pp.shape(w, h, bpp), np.uint8), (0, 64, 64, 64), runs), (0, 64, 64, 64)), np.uint8).tobytes()
    assert int(np.frombuffer(e_runs, "<u4", 1, 8)[0]) >> 16 == gp.RUNS
    solid = np.array([64, 64, 64 | 64 << 8 | gp.SOLID << 16, 0x11223344 if bpp == 4 else 0x5A], "<u4").tobytes()
    out.append(("copy from a RUNS block", before, pp.payload_of([e_runs, gs.encode_copy((0, 0, 64, 64))], 64), SCROLL))
    out.append(("a COPY and a SOLID of one block", before, pp.payload_of([solid, gs.encode_copy((64, 64, 64, 64)), gs.encode_copy((64, 0, 64, 64))], 64), SCROLL))
    # RUNS: n = 2; a start at a bitmap word's last bit; the largest n that is still a RUNS entry
    for name, blk in (("n 2", gp.block_with_starts(64, 64, [0, 4095], bpp)), ("a start at column 63", gp.block_with_starts(64, 64, [0, 63, 64 * 17 + 63, 4095], bpp)),
                      ("the largest n", gp.block_with_n_starts(3964 if bpp == 4 else 3568, bpp, 6)),
                      ("a cut block 5 x 64", gp.block_with_starts(5, 64, [0, 4, 5, 9, 319], bpp)), ("a cut block 64 x 3", gp.block_with_starts(64, 3, [0, 63, 64, 191], bpp))):
        bh, bw = blk.shape[:2]
        e = gp.encode_block(_inset(np.zeros(pp.shape(w, h, bpp), np.uint8), (64, 64, bw, bh), blk), (64, 64, bw, bh))
        assert int(np.frombuffer(e, "<u4", 1, 8)[0]) >> 16 == gp.RUNS, name
        out.append((f"RUNS {name}", before, pp.payload_of([e]), PACKED))
    # RAW of a cut block: noise, zeros beyond the cut block in the body
    e = gp.encode_block(pp.noise(w, h, bpp, 43), (64, 128, 63, 64))
    assert int(np.frombuffer(e, "<u4", 1, 8)[0]) >> 16 == gp.RAW
    out.append(("RAW of a cut block", before, pp.payload_of([e]), PACKED))
    for flags in (DELTA, PACKED, SCROLL, SCROLL | glapi.GRAB_KEY):
        out.append((f"no entry, flags {flags}", before, pp.payload_of([]), flags))
    return out


def _constructed(lib, bpp):
    s = pp.Session(lib)
    gl = s.gl
    tw, th, origin = 173, 211, (19, 6)
    for k, (name, before, payload, flags) in enumerate(_constructed_cases(bpp)):
        h, w = before.shape[:2]
        rect = origin + (w, h) if k % 2 else (16, 0, w, h)      # (rows that no 16-byte store fits; rows that take them)
        tex_px = _inset(pp.noise(tw, th, bpp, 50 + k), rect, before)
        t = s.make_px(tex_px)
        s.r.finish()
        want = _inset(tex_px, rect, pp.decoded(gl, payload, flags, before))
        if flags & glapi.GRAB_PACKED and len(payload) > 16 and "of one block" not in name:      # (the numpy walk takes a record once)
            img = before.copy()
            gs.decode(payload, img)
            _same(fg.crop(want, rect), img, f"{name}: WrhipGrabDecode against the numpy decoder")
        s.put(t, rect, payload, flags, what=name)
        _same(s.read(t), want, f"{name} ({bpp})")
        s.d.delete_texture(t)
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 3. rejections

def _malformed(bpp):
    """-> [(name, payload, bytes or None, flags)] for a 150 x 200 rect: every case tools/grab_codec_check.cpp lists and the COPY rules"""
    w, h = 150, 200
    img = gp.mixed_content(h, w, bpp, 42)
    blk = gp.block_with_starts(10, 5, [2 * k for k in range(25)], bpp)
    e = gp.encode_block(_inset(img, (3, 2, 10, 5), blk), (3, 2, 10, 5))
    good = pp.payload_of([e])

    def rec(e, **kw):
        m = bytearray(e)
        for k, v in kw.items():
            at = {"x": 0, "y": 4, "whm": 8, "aux": 12}[k]
            m[at:at + 4] = np.array([v & 0xFFFFFFFF], "<u4").tobytes()
        return bytes(m)
    out = []
    for cut in (8, 16 + 12, 16 + 8 * 5 + bpp * 3 // 2 + 1):
        held = good[:16 + cut]
        out.append((f"truncated at {cut}: fewer bytes than the header says", held, None, PACKED))
        out.append((f"truncated at {cut}: the header says fewer than the entry needs", np.array([cut, 0, 0, 0], "<u4").tobytes() + held[16:], None, PACKED))
    out.append(("fewer bytes than a header", good, 15, PACKED))
    out.append(("more bytes than 16 plus header word 0", good + bytes(16), None, PACKED))
    out.append(("n larger than the popcount", pp.payload_of([rec(e, aux=26)]), None, PACKED))
    out.append(("n smaller than the popcount", pp.payload_of([rec(e, aux=24)]), None, PACKED))
    out.append(("an n that overflows the size", pp.payload_of([rec(e, aux=0xFFFFFFF0)]), None, PACKED))
    for wv, hv in ((0, 5), (10, 0), (65, 5), (10, 65)):
        for mode in (gp.RUNS, gp.SOLID, gp.RAW):
            out.append((f"w {wv} h {hv} mode {mode}", pp.payload_of([rec(e, whm=wv | hv << 8 | mode << 16) + bytes(16 + 64 * 64 * bpp - len(e))]), None, PACKED))
    out.append(("x + w beyond the rect", pp.payload_of([rec(e, x=141)]), None, PACKED))
    out.append(("y + h beyond the rect", pp.payload_of([rec(e, y=196)]), None, PACKED))
    out.append(("a negative x", pp.payload_of([rec(e, x=-2)]), None, PACKED))
    out.append(("a negative y", pp.payload_of([rec(e, y=-(1 << 31))]), None, PACKED))
    out.append(("mode 3 without SCROLL", pp.payload_of([rec(e, whm=10 | 5 << 8 | 3 << 16)]), None, PACKED))
    out.append(("mode 4", pp.payload_of([rec(e, whm=10 | 5 << 8 | 4 << 16)]), None, SCROLL))
    m = bytearray(e); m[16 + 8] &= 0xFE; m[16 + 8 + 1] |= 4
    out.append(("a bitmap bit at a column >= w", pp.payload_of([bytes(m)]), None, PACKED))
    m = bytearray(e); m[16] = (m[16] & 0xFE) | 2
    out.append(("a first pixel without a start bit", pp.payload_of([bytes(m)]), None, PACKED))
    out.append(("a good entry ahead of a bad one", pp.payload_of([e, rec(e, whm=10 | 5 << 8 | 3 << 16)]), None, PACKED))
    out.append(("a RAW entry without its body", pp.payload_of([rec(e, whm=10 | 5 << 8)]), None, PACKED))
    out.append(("a plain entry cut short", pp.payload_of([pp.encode_plain(img, (0, 0, 64, 64))[:-16]]), None, DELTA))
    out.append(("a dy in a payload that is no scroll grab's", pp.payload_of([e], 3), None, PACKED))
    # the COPY rules
    c00, c064 = gs.encode_copy((0, 0, 64, 64)), gs.encode_copy((0, 64, 64, 64))
    out.append(("COPY with dy 0", pp.payload_of([c00], 0), None, SCROLL))
    out.append(("dy 513", pp.payload_of([c00], 513), None, SCROLL))
    out.append(("dy -513", pp.payload_of([e], -513), None, SCROLL))
    out.append(("a COPY source above the rect", pp.payload_of([c00], -1), None, SCROLL))
    out.append(("a COPY source below the rect", pp.payload_of([gs.encode_copy((0, 192, 64, 8))], 1), None, SCROLL))
    out.append(("a COPY source beyond the rect by |dy| > h", pp.payload_of([c00], 300), None, SCROLL))
    out.append(("a block named by two COPY entries", pp.payload_of([c064, e, c064], 7), None, SCROLL))
    out.append(("a COPY block off the grid", pp.payload_of([gs.encode_copy((1, 0, 64, 64))], 7), None, SCROLL))
    out.append(("a COPY block that is not whole", pp.payload_of([gs.encode_copy((128, 0, 21, 64))], 7), None, SCROLL))
    out.append(("a COPY with an aux", pp.payload_of([rec(c00, aux=1)], 7), None, SCROLL))
    out.append(("a COPY entry in a plain payload", pp.payload_of([c00], 7), None, DELTA))
    # one payload the decoder takes and the put refuses: two entries that are no COPY and share a pixel
    out.append(("two entries of one block", pp.payload_of([e, e]), None, PACKED))
    out.append(("two plain entries sharing a pixel", pp.payload_of([pp.encode_plain(img, (3, 5, 64, 64)), pp.encode_plain(img, (66, 68, 10, 10))]), None, DELTA))
    return out, good


OWN = ("more bytes than 16 plus header word 0", "two entries of one block", "two plain entries sharing a pixel")


def _rejections(lib, bpp):
    s = pp.Session(lib)
    gl = s.gl
    fmt = pp.FMT[bpp]
    w, h = 150, 200
    px = pp.noise(w, h, bpp, 60)
    tex = s.make_px(px)
    other = s.make_px(pp.noise(64, 64, bpp, 61))
    rg8 = s.d.create_texture(8, 8, G.GL_RG8)
    f32 = s.d.create_texture(8, 8, G.GL_RGBA32F)
    nostorage = gl.gen("GenTextures")
    host = np.zeros((64, 64, 4), np.uint8)
    backed = gl.gen("GenTextures")
    gl.SetTextureBuffer(backed, G.GL_RGBA8, 64, 64, 256, host.ctypes.data, 64, 64)
    locked = s.make_px(np.zeros(pp.shape(64, 64, bpp), np.uint8))
    s.r.finish()
    lock = gl.LockTexture(locked.id)
    assert lock and gl.GetError() == 0
    # an upload is queued and stays queued: a refused put sends nothing ahead of itself
    patch = pp.noise(20, 10, bpp, 62)
    s.upload(other, 3, 3, patch)
    n0 = s.stats()
    bad, good = _malformed(bpp)
    rect = (0, 0, w, h)
    small = pp.payload_of([gp.encode_block(gp.mixed_content(64, 64, bpp, 1), (0, 0, 64, 64))])
    rect4 = (C.c_int32 * 4)(*rect)

    def refused(rc, what):
        assert rc == -1, what
        assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0, what
        st = s.stats()
        assert all(st[k] == n0[k] for k in ("kernel_launches", "h2d_bytes", "d2h_bytes", "flushes")), (what, n0, st)
    for name, payload, nbytes, flags in bad:
        if nbytes is None:
            rc = gl.put_texture_payload(tex.id, rect, payload, flags)
        else:
            src = (C.c_char * len(payload)).from_buffer_copy(payload)
            rc = gl.WrhipPutTexturePayload(tex.id, C.addressof(rect4), src, nbytes, flags)
        refused(rc, name)
        # (all but the put's own three are the decoder's refusals)
        if name not in OWN and nbytes is None:
            with pytest.raises(ValueError):
                gl.grab_decode(payload, fmt, flags, px.copy())
                pytest.fail(f"WrhipGrabDecode takes: {name}")
    args = [
        ("an unknown texture", lambda: gl.put_texture_payload(9999, rect, good, PACKED)), ("texture 0", lambda: gl.put_texture_payload(0, rect, good, PACKED)),
        ("no storage", lambda: gl.put_texture_payload(nostorage, (0, 0, 1, 1), pp.payload_of([]), PACKED)),
        ("GL_RG8", lambda: gl.put_texture_payload(rg8.id, (0, 0, 8, 8), pp.payload_of([]), PACKED)),
        ("GL_RGBA32F", lambda: gl.put_texture_payload(f32.id, (0, 0, 8, 8), pp.payload_of([]), PACKED)),
        ("SetTextureBuffer storage", lambda: gl.put_texture_payload(backed, (0, 0, 64, 64), small, PACKED)),
        ("a locked texture", lambda: gl.put_texture_payload(locked.id, (0, 0, 64, 64), small, PACKED)),
        ("an empty rect", lambda: gl.put_texture_payload(tex.id, (0, 0, 0, 4), pp.payload_of([]), PACKED)),
        ("an empty rect", lambda: gl.put_texture_payload(tex.id, (0, 0, 4, 0), pp.payload_of([]), PACKED)),
        ("a negative size", lambda: gl.put_texture_payload(tex.id, (0, 0, -4, 4), pp.payload_of([]), PACKED)),
        ("a rect beyond the right edge", lambda: gl.put_texture_payload(tex.id, (1, 0, w, h), good, PACKED)),
        ("a rect beyond the last row", lambda: gl.put_texture_payload(tex.id, (0, 1, w, h), good, PACKED)),
        ("a negative x", lambda: gl.put_texture_payload(tex.id, (-1, 0, w, h), good, PACKED)), ("a negative y", lambda: gl.put_texture_payload(tex.id, (0, -1, w, h), good, PACKED)),
        ("no rect", lambda: gl.WrhipPutTexturePayload(tex.id, None, C.create_string_buffer(good, len(good)), len(good), PACKED)),
        ("no payload", lambda: gl.put_texture_payload(tex.id, rect, None, PACKED)),
        ("no payload, bytes given", lambda: gl.WrhipPutTexturePayload(tex.id, C.addressof(rect4), None, 32, PACKED)),
        ("no DELTA", lambda: gl.put_texture_payload(tex.id, rect, good, glapi.GRAB_PACKED)), ("no flag", lambda: gl.put_texture_payload(tex.id, rect, pp.payload_of([]), 0)),
        ("SCROLL without PACKED", lambda: gl.put_texture_payload(tex.id, rect, pp.payload_of([]), DELTA | glapi.GRAB_SCROLL)),
        ("FLIP_ROWS", lambda: gl.put_texture_payload(tex.id, rect, good, PACKED | glapi.GRAB_FLIP_ROWS)), ("SWAP_RB", lambda: gl.put_texture_payload(tex.id, rect, good, PACKED | glapi.GRAB_SWAP_RB)),
        ("16", lambda: gl.put_texture_payload(tex.id, rect, good, PACKED | 16)), ("YUV", lambda: gl.put_texture_payload(tex.id, rect, good, PACKED | glapi.GRAB_YUV)),
        ("TENSOR", lambda: gl.put_texture_payload(tex.id, rect, good, PACKED | glapi.GRAB_TENSOR)), ("SCALED", lambda: gl.put_texture_payload(tex.id, rect, good, PACKED | glapi.GRAB_SCALED)),
        ("bit 31", lambda: gl.put_texture_payload(tex.id, rect, good, PACKED | 1 << 31)),
    ]
    for name, call in args:
        refused(call(), name)
    gl.WrhipSetShard(0, 2)
    refused(gl.put_texture_payload(tex.id, rect, good, PACKED), "sharding is on")
    gl.WrhipSetShard(0, 1)
    gl.WrhipSetTargetRows(tex.id, 0, 100)
    refused(gl.put_texture_payload(tex.id, rect, good, PACKED), "a target that holds a strip")
    gl.WrhipSetTargetRows(tex.id, 0, 0)
    gl.UnlockResource(lock)
    # the good payload is one: the queued upload leaves ahead of it (a launch of its own), the texture changes, the other one too
    a = s.stats()
    assert gl.put_texture_payload(tex.id, rect, good, PACKED | glapi.GRAB_KEY) == 0
    b = s.stats()
    assert b["kernel_launches"] == a["kernel_launches"] + 2 and b["d2h_bytes"] == a["d2h_bytes"], (a, b)
    _same(s.read(tex), _inset(px, rect, pp.decoded(gl, good, PACKED, px)), "the good payload")
    assert pp.differing(s.read(tex), px) > 0
    _same(s.read(other), _inset(pp.noise(64, 64, bpp, 61), (3, 3, 20, 10), patch), "the queued upload")
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 4. ordering

def _payload_for(ref_px, x, y, new):
    """A packed payload that turns the rect (x, y, new's size) into `new`, from every block of it"""
    h, w = new.shape[:2]
    return (x, y, w, h), pp.payload_of([gp.encode_block(new, r) for r in fg.blocks_of(w, h)])


def _script_put(s, ref, x, y, new):
    """A put into the texture of TextureRef `ref` on a hazard_cases.Script: TexSubImage2D of the bytes themselves on the oracle"""
    if not s.wrhip:
        s.upload(ref, x, y, new)
        return
    rect, payload = _payload_for(None, x, y, new)
    assert s.gl.put_texture_payload(s.tex(ref).id, rect, payload, PACKED) == 0, s.gl.GetError()


def _patch(seed, w, h):
    return hz.premultiplied_noise(np.random.default_rng(seed), h, w) if seed % 2 else gp.mixed_content(h, w, 4, seed)


def p1_sampled_then_put(s):
    f = hz.image_frame(nearest=False, render_target=True)
    s.begin(f)
    s.draw(hz.retarget(f.tile, "T0"))
    s.write()
    _script_put(s, f.atlas, 37, 21, _patch(91, 123, 77))
    s.draw(hz.retarget(f.tile, "T1"))
    s.keep["atlas"] = f.atlas


def p2_target_then_put(s):
    """A put into a render target that has recorded draws, then a draw over it that loads its content"""
    a1 = hz.decoration_target(151)
    s.begin(hz.image_frame(seed=9, n=4, atlas=512), statics=False)
    s.draw(a1, keep=False)
    s.write()
    _script_put(s, a1.texture, 41, 33, _patch(92, 131, 59))
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
    bad = [f"{k}: {pp.differing(got[k], want[k])} bytes differ" for k in names if not np.array_equal(got[k], want[k])]
    assert names and not bad, f"{name}: {bad}"


def _held_frames():
    f = hz.image_frame(seed=17, n=16)

    def pre(k):
        x, y, w, h = ((37, 21, 123, 77), (11, 90, 201, 55), (129, 3, 99, 141))[k - 1]
        return lambda s: _script_put(s, f.atlas, x, y, _patch(200 + k, w, h))
    return [(None, f)] + [(pre(k), f) for k in (1, 2, 3)]


def _held(lib, ref):
    """Streamed frames with WrhipFlushHeld, and puts into a texture the held-back launches read"""
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


def _after_put(lib):
    """A tap and a grab before a put keep the old bytes; a tap and a full grab after it see the new ones; a queued upload and a put
    that overlap land in call order; a delta grab after a put sends exactly the blocks the put changed"""
    s = pp.Session(lib)
    gl = s.gl
    w, h = 333, 201
    old = pp.noise(w, h, 4, 70)
    tex = s.make_px(old)
    s.r.finish()
    rect = (0, 0, w, h)
    key = gl.grab_texture(tex.id, rect, PACKED)           # (the retained copy: `old`)
    assert gl.grab_result(key, into=np.zeros_like(old))[0]["keyframe"] == 1
    new = old.copy()
    changed = [(64, 0, 64, 64), (256, 128, 64, 64), (320, 192, 13, 9)]
    for k, (x, y, bw, bh) in enumerate(changed):
        new[y:y + bh, x:x + bw] = gp.mixed_content(bh, bw, 4, 71 + k) if k else pp.noise(bw, bh, 4, 71)
    same = (0, 64, 64, 64)                                # (a block that is sent with the bytes it already has)
    payload = pp.payload_of([gp.encode_block(new, r) for r in changed + [same]])
    tap0, grab0 = gl.tap_texture(tex.id), gl.grab_texture(tex.id)
    s.put(tex, rect, payload, PACKED)
    tap1, grab1 = gl.tap_texture(tex.id), gl.grab_texture(tex.id)
    delta = gl.grab_texture(tex.id, rect, PACKED)
    assert tuple(gl.tap_result(tap0)["digest"]) == ft.digest(old) and tuple(gl.tap_result(tap1)["digest"]) == ft.digest(new)
    _same(gl.grab_result(grab0)[1], old, "a grab before the put")
    _same(gl.grab_result(grab1)[1], new, "a grab after the put")
    host = old.copy()
    info = gl.grab_result(delta, into=host)[0]
    assert info["keyframe"] == 0 and info["blocks"] == len(changed) and fg.sent_records(gl, delta, old.shape) == set(changed), info
    _same(host, new, "the delta grab's image")
    # a queued upload under a put, and a put under a queued upload
    patch = pp.noise(90, 60, 4, 75)
    s.upload(tex, 20, 30, patch)
    r2, p2 = _payload_for(None, 70, 50, gp.mixed_content(50, 100, 4, 76))
    s.put(tex, r2, p2, PACKED, quiet=False)
    want = _inset(_inset(new, (20, 30, 90, 60), patch), r2, gp.mixed_content(50, 100, 4, 76))
    _same(s.read(tex), want, "upload, then put")
    r3, p3 = _payload_for(None, 10, 60, pp.noise(100, 50, 4, 77))
    s.put(tex, r3, p3, PACKED)
    s.upload(tex, 20, 30, patch[::-1])
    want = _inset(_inset(want, r3, pp.noise(100, 50, 4, 77)), (20, 30, 90, 60), patch[::-1])
    _same(s.read(tex), want, "put, then upload")
    assert gl.GetError() == 0
    s.close()


def _untouched_in_stream(lib):
    """A put into a texture no frame touches, between streamed frames: every flush still rides in the launch held back before it"""
    from webrender_amd import scenes
    from webrender_amd.glapi import GL
    from webrender_amd.renderer import Renderer
    frames = [scenes.cfg2_overlapping_rects(width=256, height=256, n=60, seed=sd) for sd in (3, 4, 5, 6, 7, 8)]
    runs = {}
    for put in (False, True):
        gl = GL(lib)
        r = Renderer(gl, 256, 256)
        before = pp.noise(130, 70, 4, 80)
        side = r.device.create_texture(130, 70, G.GL_RGBA8, render_target=True)
        r.device.upload_texture(side, 0, 0, 130, 70, G.GL_BGRA, G.GL_UNSIGNED_BYTE, before)
        want = before
        for k, f in enumerate(frames):
            r.render(f)
            if put:
                new = gp.mixed_content(70, 130, 4, 81 + k)
                ent = [gs.encode_copy(rec) if rec[1] == 0 else gp.encode_block(new, rec) for rec in fg.blocks_of(130, 70)]
                payload = pp.payload_of(ent, 6)
                a = gl.stats()
                assert gl.put_texture_payload(side.id, (0, 0, 130, 70), payload, SCROLL) == 0
                b = gl.stats()
                assert b["flushes"] == a["flushes"] and b["kernel_launches"] == a["kernel_launches"] + 2, (a, b)
                want = pp.decoded(gl, payload, SCROLL, want)
        stats = gl.stats()
        r.finish()
        assert gl.GetError() == 0
        runs[put] = (stats, r.read_pixels().copy())
        _same(r.device.read_texture(side), want, "the side texture")
        r.destroy()
    assert runs[True][0]["setup_carried"] == runs[False][0]["setup_carried"] >= len(frames) - 1, (runs[True][0], runs[False][0])
    assert runs[True][0]["flushes"] == runs[False][0]["flushes"]
    _same(runs[True][1], runs[False][1], "the window")


# ---------------------------------------------------------------------------- 5. cost, kernel statistics

def _kernel_stats(lib, bpp):
    """Launches 0, 1 and 2 (pp.Session.put checks every put's), and WrhipGetKernelStats: kind 16, feat 1 the patch pass, feat 2 the
    COPY pass"""
    s = pp.Session(lib)
    gl = s.gl
    w, h = 130, 200
    px = pp.noise(w, h, bpp, 90)
    tex = s.make_px(px)
    s.r.finish()
    gl.WrhipSetProfiling(1)
    img = gp.mixed_content(h, w, bpp, 91)
    rect = (0, 0, w, h)
    recs = fg.blocks_of(w, h)
    copies = [gs.encode_copy(r) for r in recs if r[1] + 64 + r[3] <= h]
    sends = [gp.encode_block(img, r) for r in recs if r[1] + 64 + r[3] > h]
    assert s.put(tex, rect, pp.payload_of([]), PACKED) == 0
    assert s.put(tex, rect, pp.payload_of(sends), PACKED) == 1
    assert s.put(tex, rect, pp.payload_of(copies, 64), SCROLL) == 1
    assert s.put(tex, rect, pp.payload_of(sends + copies, 64), SCROLL) == 2
    ks = (glapi.WrhipKernelStat * 64)()
    n = gl.WrhipGetKernelStats(ks, 64)
    puts = {k.feat: k for k in ks[:n] if k.kind == 16}
    gl.WrhipSetProfiling(0)
    assert sorted(puts) == [1, 2] and puts[1].launches == 2 and puts[2].launches == 2, [(k.kind, k.feat, k.launches) for k in ks[:n]]
    assert puts[1].workgroups == 2 * len(sends) and puts[2].workgroups == 2 * 3      # (a workgroup per entry; one per block column)
    s.close()


# ---------------------------------------------------------------------------- 6. the harness loop

def _mirror_frames():
    from webrender_amd import scenes
    return [scenes.cfg2_overlapping_rects(width=256, height=256, n=40 + 5 * (k % 3), seed=30 + k // 2) for k in range(10)]


def _mirrored(lib, packed, scroll):
    px, st, windows, mirrors, crossed = render_streamed_mirrored(lib, _mirror_frames(), packed=packed, scroll=scroll)
    assert st["gl_error"] == 0 and len(windows) == len(mirrors) == len(crossed) == 10
    assert len({w.tobytes() for w in windows}) >= 5                       # (the frames differ; some repeat: a payload of no entry)
    bad = [k for k in range(10) if not np.array_equal(windows[k], mirrors[k])]
    assert not bad, f"frames after which the mirror is not the window: {bad}"
    _same(px, windows[-1], "the mirror after the last frame")
    if packed:
        assert sum(crossed) < 10 * 256 * 256 * 4 // 4, crossed            # (flat rects: packed payloads are a fraction of the pixels)


# ---------------------------------------------------------------------------- CPU only: the index builder; the code object

def test_index_builder_on_hostile_input(tmp_path):
    """tools/put_payload_check.cpp -- wr_grab_codec.h alone, its own main -- under AddressSanitizer and UBSan, as a process of its own"""
    cxx = shutil.which("g++")
    flags = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    trivial = tmp_path / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    if cxx is None or subprocess.run([cxx] + flags + [str(trivial), "-o", str(tmp_path / "trivial")], capture_output=True).returncode != 0:
        pytest.skip("no g++ that links with -fsanitize=address,undefined")
    exe = tmp_path / "put_payload_check"
    subprocess.run([cxx] + flags + ["-I", os.path.join(ROOT, "webrender_amd", "csrc"), os.path.join(ROOT, "tools", "put_payload_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "put_payload_check: ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_put_payload_kernels_have_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    for name in ("wr_put_copy_kernel", "wr_put_patch_kernel"):
        assert name in notes, sorted(notes)
        vgprs, scratch = notes[name]
        assert scratch == 0, (name, vgprs, scratch)


# ---------------------------------------------------------------------------- CPU: the host simulation

CASES = [(size, bpp, mode) for size in SIZES for bpp in (4, 1) for mode in pp.MODES]


@pytest.mark.parametrize("size,bpp,mode", CASES)
def test_hostsim_round_trip(hostsim, size, bpp, mode):
    _round_trip(hostsim, size, bpp, mode)


@pytest.mark.parametrize("bpp", (4, 1))
def test_hostsim_constructed_payloads(hostsim, bpp):
    _constructed(hostsim, bpp)


@pytest.mark.parametrize("bpp", (4, 1))
def test_hostsim_rejections(hostsim, bpp):
    _rejections(hostsim, bpp)


@pytest.mark.parametrize("name", list(PENDING))
def test_hostsim_put_meets_recorded_draws(hostsim, oracle_gcc, name):
    _pending(hostsim, oracle_gcc, name)


def test_hostsim_put_meets_held_launches(hostsim, oracle_gcc):
    _held(hostsim, oracle_gcc)


def test_hostsim_taps_grabs_uploads_around_a_put(hostsim):
    _after_put(hostsim)


def test_hostsim_put_on_untouched_texture_in_stream(hostsim):
    _untouched_in_stream(hostsim)


@pytest.mark.parametrize("bpp", (4, 1))
def test_hostsim_cost_and_kernel_stats(hostsim, bpp):
    _kernel_stats(hostsim, bpp)


@pytest.mark.parametrize("packed,scroll", ((False, False), (True, False), (True, True)))
def test_hostsim_mirrored_stream(hostsim, packed, scroll):
    _mirrored(hostsim, packed, scroll)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("size,bpp,mode", CASES)
def test_gpu_round_trip(size, bpp, mode):
    _round_trip(wrhip_lib(), size, bpp, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("bpp", (4, 1))
def test_gpu_constructed_payloads(bpp):
    _constructed(wrhip_lib(), bpp)


@pytest.mark.gpu
@pytest.mark.parametrize("bpp", (4, 1))
def test_gpu_rejections(bpp):
    _rejections(wrhip_lib(), bpp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PENDING))
def test_gpu_put_meets_recorded_draws(name):
    _pending(wrhip_lib(), _gpu_ref(), name)


@pytest.mark.gpu
def test_gpu_put_meets_held_launches():
    _held(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_taps_grabs_uploads_around_a_put():
    _after_put(wrhip_lib())


@pytest.mark.gpu
def test_gpu_put_on_untouched_texture_in_stream():
    _untouched_in_stream(wrhip_lib())


@pytest.mark.gpu
@pytest.mark.parametrize("bpp", (4, 1))
def test_gpu_cost_and_kernel_stats(bpp):
    _kernel_stats(wrhip_lib(), bpp)


@pytest.mark.gpu
@pytest.mark.parametrize("packed,scroll", ((False, False), (True, False), (True, True)))
def test_gpu_mirrored_stream(packed, scroll):
    _mirrored(wrhip_lib(), packed, scroll)
