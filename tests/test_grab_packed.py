"""Packed delta grabs (include/wrhip.h: WRHIP_GRAB_PACKED, WrhipGrabPayloadGet, WrhipGrabDecode): the blocks a delta grab sends,
written as SOLID / RUNS / RAW entries by wr_grab_pack_runs_kernel.  The bytes that crossed are compared entry for entry with a numpy
restatement of the format (tests/grab_packed.py) that shares nothing with the library's decoder; images are compared byte for byte
with the oracle's render or with bytes the test uploaded.  Each check runs on the host simulation and, under -m gpu, on the MI355X;
the budget and the hostile-input checks need neither."""
import os
import shutil
import subprocess
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref, ROOT
import frame_taps as ft
import frame_grabs as fg
import grab_packed as gp
import stream_cases
import test_frame_grabs as tfg
from webrender_amd import scenes, glapi, glconst as G, device
from webrender_amd.harness import render_streamed_grabbed

DELTA, KEY, PACKED, FLIP, SWAP = glapi.GRAB_DELTA, glapi.GRAB_KEY, glapi.GRAB_PACKED, glapi.GRAB_FLIP_ROWS, glapi.GRAB_SWAP_RB
DP = DELTA | PACKED


class Hosts:
    """Three host images of one rect, each kept up to date by one decoder: grab_result(into=), GL.grab_decode, the numpy helper's"""

    def __init__(self, like):
        self.lib, self.pure, self.numpy = (np.zeros_like(like) for _ in range(3))


def check_packed(gl, ticket, hosts, want, sent, keyframe, flags=DP, modes=None):
    """A packed delta ticket against the expected stored bytes `want` of its rect and the expected records `sent`: the payload's
    entries byte for byte, info, and the three decoders.  modes: a dict that counts the entries' modes.  -> info"""
    h, w = want.shape[:2]
    bpp = fg.bpp_of(want)
    fmt = G.GL_RGBA8 if bpp == 4 else G.GL_R8
    sent = set(sent)
    payload = gl.grab_payload(ticket)
    entries = gp.split(payload, bpp)
    assert set(entries) == sent, (sorted(entries), sorted(sent))
    for rec, (mode, e) in entries.items():
        expect = gp.encode_block(want, rec)
        assert e == expect, f"the entry of block {rec} (mode {mode}, {len(e)} bytes) is not the expected one (mode {np.frombuffer(expect, '<u4', 1, 8)[0] >> 16}, {len(expect)} bytes)"
        if modes is not None:
            modes[mode] = modes.get(mode, 0) + 1
    info, out = gl.grab_result(ticket, into=hosts.lib)
    assert out is hosts.lib
    assert info["status"] == 0 and info["format"] == fmt and info["flags"] == flags, info
    assert info["keyframe"] == (1 if keyframe else 0) and info["blocks_total"] == len(fg.blocks_of(w, h)), info
    assert info["blocks"] == len(sent) and tuple(info["damage"]) == fg.damage_of(sent), (info, sorted(sent))
    assert info["bytes"] == len(payload) == fg.HEADER + sum(len(e) for _, e in entries.values()) == gp.predicted_bytes(want, sent), info
    assert info["bytes"] <= fg.HEADER + len(sent) * fg.entry_bytes(bpp)
    assert gl.grab_decode(payload, fmt, flags, hosts.pure) == (fg.damage_of(sent), len(sent))
    assert gp.decode(payload, hosts.numpy) == len(sent)
    for name, img in (("grab_result", hosts.lib), ("grab_decode", hosts.pure), ("the numpy decoder", hosts.numpy)):
        assert np.array_equal(img, want), f"{name}: {int((img != want).sum())} bytes of the patched image differ"
    assert gl.grab_payload(ticket) == payload          # (fetched twice: the same bytes)
    return info


# ---------------------------------------------------------------------------- 1. the wire format, byte for byte

def _packed_steps(s, t, a, window, modes):
    """tests/test_frame_grabs.py's delta sequence (_delta_steps) with DELTA | PACKED on texture `t` whose stored bytes are `a`"""
    gl = s.gl
    h, w = a.shape[:2]
    fmt = G.GL_RGBA8 if a.ndim == 3 else G.GL_R8
    blocks = fg.blocks_of(w, h)
    hosts = Hosts(a)
    grab = lambda flags=DP, rect=None: gl.grab_texture(t.id, rect, flags)
    # A: a keyframe; A again: nothing
    check_packed(gl, grab(), hosts, a, blocks, True, modes=modes)
    info = check_packed(gl, grab(), hosts, a, [], False)
    assert info["bytes"] == fg.HEADER and tuple(info["damage"]) == (0, 0, 0, 0)
    # B: one change confined to one (edge) block
    one = blocks[-2] if len(blocks) > 1 else blocks[0]
    b = tfg._one_block_change(a, one)
    s.upload(t, one[0], one[1], ft.crop(b, one))
    check_packed(gl, grab(), hosts, b, [one], False, modes=modes)
    # C: pixels of block (0, 0) and of the last edge block
    c = b.copy()
    c[0, 0] = c[0, 0] ^ 0x80
    c[h - 1, w - 1] = c[h - 1, w - 1] ^ 0x02
    c[min(h - 1, 63), min(w - 1, 63)] = c[min(h - 1, 63), min(w - 1, 63)] ^ 0x10
    s.upload(t, 0, 0, c)
    sent = fg.changed_blocks(b, c)
    assert sent == {blocks[0], blocks[-1]}
    check_packed(gl, grab(), hosts, c, sent, False, modes=modes)
    # WRHIP_GRAB_KEY: a keyframe again, into fresh images
    hosts = Hosts(a)
    check_packed(gl, grab(DP | KEY), hosts, c, blocks, True, flags=DP | KEY)
    check_packed(gl, grab(), hosts, c, [], False)
    # another rect: a keyframe; the same rect again: nothing; the whole texture again: a keyframe
    if w > 8 and h > 8:
        rect = (3, 2, w - 5, h - 3)
        part = np.ascontiguousarray(ft.crop(c, rect))
        ph = Hosts(part)
        check_packed(gl, grab(rect=rect), ph, part, fg.blocks_of(rect[2], rect[3]), True, modes=modes)
        check_packed(gl, grab(rect=rect), ph, part, [], False)
        check_packed(gl, grab(), hosts, c, blocks, True)
    # new storage of another size: a keyframe
    nw, nh = w + 3, h + 1
    n = gp.mixed_content(nh, nw, fg.bpp_of(a), 900 + w)
    if window:
        s.d.init_default_framebuffer(nw, nh)
        t = device.Texture(gl.WrhipGetFramebufferTexture(0), nw, nh, fmt)
    else:
        gl.ActiveTexture(G.GL_TEXTURE0)
        gl.BindTexture(G.GL_TEXTURE_2D, t.id)
        gl.TexStorage2D(G.GL_TEXTURE_2D, 1, fmt, nw, nh)
        t = device.Texture(t.id, nw, nh, fmt)
    s.upload(t, 0, 0, n)
    hosts = Hosts(n)
    check_packed(gl, gl.grab_texture(t.id, None, DP), hosts, n, fg.blocks_of(nw, nh), True, modes=modes)
    check_packed(gl, gl.grab_texture(t.id, None, DP), hosts, n, [], False)
    assert gl.GetError() == 0


def _wire_format(lib):
    modes = {}
    for (w, h) in ((130, 67), (333, 201)):
        s = fg.Session(lib, w, h)
        a = gp.mixed_content(h, w, 4, w)
        win = device.Texture(s.window, w, h, G.GL_RGBA8)
        s.upload(win, 0, 0, a)
        _packed_steps(s, win, a, True, modes)
        s.close()
    assert all(modes.get(m, 0) > 0 for m in (gp.RAW, gp.SOLID, gp.RUNS)), modes
    modes = {}
    s = fg.Session(lib, 64, 64)
    for (w, h) in ((61, 37), (513, 513)):
        a = gp.mixed_content(h, w, 1, w)
        _packed_steps(s, s.make(a, G.GL_R8), a, False, modes)
    s.close()
    assert all(modes.get(m, 0) > 0 for m in (gp.RAW, gp.SOLID, gp.RUNS)), modes


# ---------------------------------------------------------------------------- 2. boundaries of the mode rule and of the scan

def _boundary_cases():
    """(name, image, {record: expected mode}): 64 x 64 textures of one block, and textures with cut blocks"""
    B = gp.BLOCK
    full = (0, 0, B, B)
    cases = []
    for bpp, ns in ((4, (1, 2, 3964, 3965)), (1, (1, 2, 3568, 3569))):
        for n in ns:
            want = gp.SOLID if n == 1 else gp.RAW if n in (3965, 3569) else gp.RUNS
            cases.append((f"bpp{bpp}-n{n}", gp.block_with_n_starts(n, bpp, seed=n), {full: want}))
        # run starts on wave, piece-group and row boundaries only
        cases.append((f"bpp{bpp}-edges", gp.block_with_starts(B, B, [0, 63, 64, 255, 256, 1023, 1024, 4095], bpp), {full: gp.RUNS}))
        # 66 x 67: a 2 x 64, a 64 x 3 and a 2 x 3 cut block; the 2 x 3 one once with the rows' first pixels equal to the last pixel
        # of the row above (a b / b c / c d: starts at 0, 1, 3, 5) and once with them different (a b / a b / a b: every pixel)
        for name, starts in (("wrap-equal", [0, 1, 3, 5]), ("wrap-differs", [0, 1, 2, 3, 4, 5])):
            img = fg.noise(67, 66, G.GL_RGBA8 if bpp == 4 else G.GL_R8, 66 + bpp)
            img[64:67, 64:66] = gp.block_with_starts(2, 3, starts, bpp, seed=5)
            if name == "wrap-differs":
                img[64:67, 64:66] = img[64:65, 64:66]
                assert len(np.unique(gp.values_of(img[64:65, 64:66]))) == 2
            assert int(gp.run_starts(img[64:67, 64:66])[1].sum()) == len(starts)
            cases.append((f"bpp{bpp}-2x3-{name}", img, {(64, 64, 2, 3): gp.RUNS}))
        # 127 x 127: cut blocks of 63 x 64, 64 x 63 and 63 x 63 noise pixels, all RAW: the bytes of a RAW body beyond the cut block
        if bpp == 4:
            img = fg.noise(127, 127, G.GL_RGBA8, 127)
            cases.append(("bpp4-cut-raw", img, {(64, 0, 63, 64): gp.RAW, (0, 64, 64, 63): gp.RAW, (64, 64, 63, 63): gp.RAW}))
        # 65 x 65: a 1 x 1 cut block (one pixel: SOLID), a 1 x 64 column of one value above it (SOLID) and a 64 x 1 row of 64 values
        img = fg.noise(65, 65, G.GL_RGBA8 if bpp == 4 else G.GL_R8, 65 + bpp)
        img[0:64, 64] = img[0, 64]
        img[64:65, 0:64] = gp.block_with_starts(64, 1, range(64), bpp, seed=9)
        cases.append((f"bpp{bpp}-1x1", img, {(64, 64, 1, 1): gp.SOLID, (64, 0, 1, 64): gp.SOLID, (0, 64, 64, 1): gp.RUNS}))
    return cases


def _boundaries(lib):
    s = fg.Session(lib, 64, 64)
    for name, img, expect in _boundary_cases():
        bpp = fg.bpp_of(img)
        t = s.make(img, G.GL_RGBA8 if bpp == 4 else G.GL_R8)
        h, w = img.shape[:2]
        ticket = s.gl.grab_texture(t.id, None, DP)
        entries = gp.split(s.gl.grab_payload(ticket), bpp)
        for rec, mode in expect.items():
            assert rec in entries and entries[rec][0] == mode, (name, rec, mode, {r: m for r, (m, _) in entries.items()})
        check_packed(s.gl, ticket, Hosts(img), img, fg.blocks_of(w, h), True)
        s.d.delete_texture(t)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 3. plain and packed delta grabs of one texture

def _mixing(lib):
    w, h = 130, 67
    s = fg.Session(lib, w, h)
    gl = s.gl
    a = gp.mixed_content(h, w, 4, 7)
    win = device.Texture(s.window, w, h, G.GL_RGBA8)
    s.upload(win, 0, 0, a)
    blocks = fg.blocks_of(w, h)
    host = np.zeros_like(a)
    hosts = Hosts(a)
    fg.check_delta(gl, gl.grab_texture(win.id, None, DELTA), host, a, blocks, keyframe=True)
    hosts.lib[...] = hosts.pure[...] = hosts.numpy[...] = a
    cur = a
    for k, flags in enumerate((DELTA, DP, DELTA, DP)):
        one = blocks[(2 * k + 1) % len(blocks)]
        nxt = tfg._one_block_change(cur, one)
        s.upload(win, one[0], one[1], ft.crop(nxt, one))
        t = gl.grab_texture(win.id, None, flags)
        if flags & PACKED:
            check_packed(gl, t, hosts, nxt, [one], False)
            host[...] = nxt
        else:
            fg.check_delta(gl, t, host, nxt, [one], keyframe=False)
            hosts.lib[...] = hosts.pure[...] = hosts.numpy[...] = nxt
        cur = nxt
    check_packed(gl, gl.grab_texture(win.id, None, DP | KEY), Hosts(a), cur, blocks, True, flags=DP | KEY)
    fg.check_delta(gl, gl.grab_texture(win.id, None, DELTA), host, cur, [], keyframe=False)
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 4. refusals; 5. one launch, nothing drained

def _refusals_and_one_launch(lib):
    s = fg.Session(lib, tfg.W, tfg.H)
    s.r.render(tfg._frame())
    s.r.finish()
    s.r.read_pixels()
    gl = s.gl
    assert gl.GetError() == 0
    one = [(0, 0, 4, 4)]
    n0 = s.stats()["kernel_launches"]
    for k, (rects, flags) in enumerate(((one, PACKED), (one, PACKED | FLIP), (one, PACKED | DELTA | SWAP), (one * 2, PACKED | DELTA), (one, 16), (one, 64),
                                        (one, PACKED | KEY), (one, PACKED | DELTA | FLIP), (one, PACKED | DELTA | 16))):
        assert gl.grab_texture(s.window, rects, flags) == -1, k
        assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0, k
    assert s.stats()["kernel_launches"] == n0
    for k, flags in enumerate((DP, DP, DP | KEY, DP)):
        a = s.stats()
        t = gl.grab_texture(s.window, None, flags)
        b = s.stats()
        assert t >= 0 and b["kernel_launches"] == a["kernel_launches"] + 1 and b["flushes"] == a["flushes"]
        # d2h_bytes grows once per ticket, at whichever getter comes first
        if k & 1:
            payload = gl.grab_payload(t)
            c = s.stats()
            info, _ = gl.grab_result(t)
        else:
            info, _ = gl.grab_result(t)
            c = s.stats()
            payload = gl.grab_payload(t)
        assert len(payload) == info["bytes"] and c["d2h_bytes"] == a["d2h_bytes"] + info["bytes"]
        assert info["keyframe"] == (1 if k in (0, 2) else 0) and info["blocks"] == (64 if k in (0, 2) else 0)
        gl.grab_result(t)
        gl.grab_payload(t)
        d = s.stats()
        assert d["d2h_bytes"] == c["d2h_bytes"] and d["kernel_launches"] == b["kernel_launches"] and d["flushes"] == a["flushes"]
    # the payload getter on a plain delta and on a full grab: the bytes of the slot, header first
    t = gl.grab_texture(s.window, (0, 0, 3, 2), 0)
    info, px = gl.grab_result(t)
    payload = gl.grab_payload(t)
    assert len(payload) == info["bytes"] == 16 + 24 and payload[16:] == px.tobytes() and int(np.frombuffer(payload, "<u4", 1)[0]) == 24
    n = glapi.u64(0)
    import ctypes as C
    buf = C.create_string_buffer(b"\xa5" * 32, 32)
    assert gl.WrhipGrabPayloadGet(t, buf, 20, C.byref(n), 0) == 0 and n.value == 40          # (a short buffer: its first bytes only)
    assert buf.raw[:20] == payload[:20] and buf.raw[20:] == b"\xa5" * 12
    assert gl.WrhipGrabPayloadGet(t + 1, None, 0, C.byref(n), 1) == -1 and gl.WrhipGrabPayloadGet(-3, None, 0, C.byref(n), 0) == -1
    with pytest.raises(KeyError):
        gl.grab_payload(t + 1)
    with pytest.raises(ValueError):
        gl.grab_decode(payload[:16] + b"\x01" * 24, G.GL_RGBA8, DP, np.zeros((2, 3, 4), np.uint8))
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 6. every frame of a stream

def _stream(lib, ref, name, seq, on_gpu):
    if seq is None:
        makes = [(("rects", sd), (lambda sd=sd: scenes.cfg2_overlapping_rects(n=60, seed=sd, **stream_cases.W))) for sd in tfg.RECT_SEEDS]
        carried = len(makes) - 1
    else:
        if on_gpu:
            seq = [i for i in seq if i not in stream_cases.DEVICE_INEXACT]
        makes = [(("menu", i), stream_cases.MENU[i]) for i in seq]
        carried = stream_cases.carriers_expected(seq)
    px, st, images, infos = render_streamed_grabbed(lib, [m() for _, m in makes], delta=True, packed=True)
    assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
    assert st["setup_carried"] >= carried, (st, carried)
    assert len(images) == len(infos) == len(makes)
    prev = None
    for k, ((key, make), img, info) in enumerate(zip(makes, images, infos)):
        want = ft.window_stored(tfg._ref_render(ref, key, make))
        assert np.array_equal(img, want), f"{name}: frame {k} ({key}) is not the oracle's render"
        sent = fg.blocks_of(want.shape[1], want.shape[0]) if k == 0 else fg.changed_blocks(prev, want)
        plain = fg.HEADER + len(sent) * fg.entry_bytes(4)
        assert info["status"] == 0 and info["keyframe"] == (1 if k == 0 else 0) and info["blocks_total"] == 64, info
        assert info["blocks"] == len(sent), (k, info)
        assert info["bytes"] == gp.predicted_bytes(want, sent), (k, info)
        assert info["bytes"] <= plain and (k > 0 or info["bytes"] < plain), (k, info, plain)
        prev = want
    assert np.array_equal(px, tfg._ref_render(ref, makes[-1][0], makes[-1][1]))


STREAMS = [tfg.SEQUENCES[0], ("rects", None)]


# ---------------------------------------------------------------------------- 7. parked behind the tail

def _parked(lib, ref):
    W, H = tfg.W, tfg.H
    want1 = ft.window_stored(tfg._ref_render(ref, "cfg2", tfg._frame))
    s = fg.Session(lib, W, H)
    s.r.render(tfg._frame())
    hosts = Hosts(want1)
    win = device.Texture(s.window, W, H, G.GL_RGBA8)
    t = s.gl.grab_texture(s.window, None, DP)
    patch = fg.noise(70, 40, G.GL_RGBA8, 77)
    s.upload(win, 100, 60, patch)                    # x 100..139, y 60..129: blocks (1..2, 0..2)
    t2 = s.gl.grab_texture(s.window, None, DP)
    check_packed(s.gl, t, hosts, want1, fg.blocks_of(W, H), True)
    want2 = want1.copy()
    want2[60:130, 100:140] = patch
    sent = fg.changed_blocks(want1, want2)
    assert len(sent) == 6
    check_packed(s.gl, t2, hosts, want2, sent, False)
    s.r.finish()
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 8. budget; 9. the decoder on hostile input (CPU only)

def test_packed_grab_kernel_has_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    for name in ("wr_grab_pack_runs_kernel", "wr_grab_pack_kernel", "wr_grab_push_kernel"):
        assert name in notes, sorted(notes)
        vgprs, scratch = notes[name]
        assert scratch == 0, (name, vgprs, scratch)


def test_decoder_on_hostile_input(tmp_path):
    """tools/grab_codec_check.cpp -- wr_grab_codec.h alone, its own main -- under AddressSanitizer and UBSan, as a process of its own"""
    cxx = shutil.which("g++")
    flags = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    trivial = tmp_path / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    if cxx is None or subprocess.run([cxx] + flags + [str(trivial), "-o", str(tmp_path / "trivial")], capture_output=True).returncode != 0:
        pytest.skip("no g++ that links with -fsanitize=address,undefined")
    exe = tmp_path / "grab_codec_check"
    subprocess.run([cxx] + flags + ["-I", os.path.join(ROOT, "webrender_amd", "csrc"), os.path.join(ROOT, "tools", "grab_codec_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "grab_codec_check: ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


# ---------------------------------------------------------------------------- CPU: the host simulation

def test_hostsim_wire_format(hostsim):
    _wire_format(hostsim)


def test_hostsim_boundaries(hostsim):
    _boundaries(hostsim)


def test_hostsim_mixing(hostsim):
    _mixing(hostsim)


def test_hostsim_refusals_and_one_launch(hostsim):
    _refusals_and_one_launch(hostsim)


@pytest.mark.parametrize("name,seq", STREAMS, ids=[n for n, _ in STREAMS])
def test_hostsim_packed_stream(hostsim, oracle_gcc, name, seq):
    _stream(hostsim, oracle_gcc, name, seq, on_gpu=False)


def test_hostsim_parked(hostsim, oracle_gcc):
    _parked(hostsim, oracle_gcc)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
def test_gpu_wire_format():
    _wire_format(wrhip_lib())


@pytest.mark.gpu
def test_gpu_boundaries():
    _boundaries(wrhip_lib())


@pytest.mark.gpu
def test_gpu_mixing():
    _mixing(wrhip_lib())


@pytest.mark.gpu
def test_gpu_refusals_and_one_launch():
    _refusals_and_one_launch(wrhip_lib())


@pytest.mark.gpu
@pytest.mark.parametrize("name,seq", STREAMS, ids=[n for n, _ in STREAMS])
def test_gpu_packed_stream(name, seq):
    _stream(wrhip_lib(), _gpu_ref(), name, seq, on_gpu=True)


@pytest.mark.gpu
def test_gpu_parked():
    _parked(wrhip_lib(), _gpu_ref())
