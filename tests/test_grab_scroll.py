"""Scroll grabs (include/wrhip.h: WRHIP_GRAB_SCROLL): a packed delta grab that finds the vertical scroll on the device and sends a
scrolled block as a 16-byte COPY entry.  The vector, the entries that crossed and the three decoders' images are compared with a
numpy restatement of the contract (tests/grab_scroll.py) that shares nothing with the library's kernels or codec.  Content is a tall
page of random bytes of which the texture shows a slice -- every segment is unique, so voting by hashes and the model's exact
equality agree -- or periodic / solid on purpose.  Each check runs on the host simulation and, under -m gpu, on the MI355X; the
decoder's hostile-input check and the kernels' budget need neither."""
import os
import shutil
import subprocess
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref, ROOT
import frame_taps as ft
import frame_grabs as fg
import grab_packed as gp
import grab_scroll as gs
import grab_tensor as gt
import stream_cases
import test_frame_grabs as tfg
from test_grab_packed import Hosts, check_packed
from webrender_amd import scenes, glapi, glconst as G, device
from webrender_amd.harness import render_streamed_grabbed

DELTA, KEY, PACKED, SCROLL, FLIP, SWAP = glapi.GRAB_DELTA, glapi.GRAB_KEY, glapi.GRAB_PACKED, glapi.GRAB_SCROLL, glapi.GRAB_FLIP_ROWS, glapi.GRAB_SWAP_RB
DP = DELTA | PACKED
DPS = DP | SCROLL


def check_scroll(gl, ticket, hosts, prev, want, flags=DPS, keyframe=False):
    """A scroll ticket against the retained bytes `prev` and the stored bytes `want` of its rect: the vector, the entries byte for
    byte, info, and the three decoders (`hosts` hold `prev`, or anything on a keyframe).  -> info, with "other": the non-COPY entries"""
    h, w = want.shape[:2]
    bpp = fg.bpp_of(want)
    fmt = G.GL_RGBA8 if bpp == 4 else G.GL_R8
    if keyframe:
        dy, expect = 0, {rec: gp.encode_block(want, rec) for rec in fg.blocks_of(w, h)}
    else:
        dy, expect = gs.expected_entries(prev, want)
    payload = gl.grab_payload(ticket)
    got_dy, entries = gs.split(payload, bpp)
    assert got_dy == dy, (got_dy, dy)
    assert set(entries) == set(expect), (sorted(entries), sorted(expect))
    for rec, (mode, e) in entries.items():
        assert e == expect[rec], f"the entry of block {rec} (mode {mode}, {len(e)} bytes) is not the expected one ({len(expect[rec])} bytes)"
    copied = sum(1 for mode, _ in entries.values() if mode == gs.COPY)
    sent = set(expect)
    info, out = gl.grab_result(ticket, into=hosts.lib)
    assert out is hosts.lib
    assert info["status"] == 0 and info["format"] == fmt and info["flags"] == flags, info
    assert info["keyframe"] == (1 if keyframe else 0) and info["blocks_total"] == len(fg.blocks_of(w, h)), info
    assert info["scroll_dy"] == dy and info["copied"] == copied and info["blocks"] == len(sent), (info, dy, copied, len(sent))
    assert tuple(info["damage"]) == fg.damage_of(sent), (info, sorted(sent))
    assert info["bytes"] == len(payload) == fg.HEADER + sum(len(e) for e in expect.values()), info
    assert gl.grab_decode(payload, fmt, flags, hosts.pure) == (fg.damage_of(sent), len(sent))
    assert gs.decode(payload, hosts.numpy) == (len(sent), copied)
    for name, img in (("grab_result", hosts.lib), ("grab_decode", hosts.pure), ("the numpy decoder", hosts.numpy)):
        assert np.array_equal(img, want), f"{name}: {int((img != want).sum())} bytes of the patched image differ"
    info["other"] = len(sent) - copied
    info["modes"] = {rec: mode for rec, (mode, _) in entries.items()}
    return info


class Scroller:
    """A texture that shows rows [at, at + h) of a tall page, grabbed with SCROLL into three host images"""

    def __init__(self, s, page, h, at, fmt=G.GL_RGBA8, tex=None, rect=None):
        self.s, self.page, self.h, self.at, self.rect = s, page, h, at, rect
        self.shown = np.ascontiguousarray(page[at:at + h])
        self.t = s.make(self.shown, fmt) if tex is None else tex
        if tex is not None:
            s.upload(tex, 0, 0, self.shown)
        self.prev = self.view()
        self.hosts = Hosts(self.prev)

    def view(self):
        return self.shown if self.rect is None else np.ascontiguousarray(ft.crop(self.shown, self.rect))

    def show(self, img):
        self.shown = np.ascontiguousarray(img)
        self.s.upload(self.t, 0, 0, self.shown)

    def scroll(self, dy):
        self.at += dy
        self.show(self.page[self.at:self.at + self.h])

    def grab(self, flags=DPS, keyframe=False):
        want = self.view()
        info = check_scroll(self.s.gl, self.s.gl.grab_texture(self.t.id, self.rect, flags), self.hosts, self.prev, want, flags, keyframe)
        self.prev = want
        return info

    def still(self):
        """a second grab of unchanged content: 16 bytes, no vector"""
        info = self.grab()
        assert info["bytes"] == fg.HEADER and info["scroll_dy"] == 0 and info["blocks"] == 0, info


# ---------------------------------------------------------------------------- 1. pure scrolls; 2. the bound

PURE = {1: (20, 4), 7: (20, 4), -3: (20, 4), -64: (20, 4), 64: (16, 8), 65: (16, 8), -130: (12, 12), 200: (8, 16), 330: (0, 24)}


def _pure_scrolls(lib):
    s = fg.Session(lib, 64, 64)
    w, h = 200, 331
    sc = Scroller(s, gs.page(h + 1000, w, 4, 1), h, 400)
    sc.grab(keyframe=True)
    sc.still()
    for dy, (copied, other) in PURE.items():
        sc.scroll(dy)
        info = sc.grab()
        assert info["scroll_dy"] == dy and (info["copied"], info["other"]) == (copied, other), (dy, info)
        sc.still()
    # R8, 131 x 200: the last column 3 pixels, the last block row 8 rows
    r8 = Scroller(s, gs.page(200 + 200, 131, 1, 2), 200, 100, fmt=G.GL_R8)
    r8.grab(keyframe=True)
    for dy in (7, -64):
        r8.scroll(dy)
        info = r8.grab()
        assert info["scroll_dy"] == dy and info["copied"] > 0, info
        r8.still()
    # rows that are no multiple of 16 bytes, a rect that starts at x = 3
    odd = Scroller(s, gs.page(140 + 60, 513, 4, 3), 140, 30, rect=(3, 2, 500, 130))
    odd.grab(keyframe=True)
    odd.scroll(7)
    info = odd.grab()
    assert info["scroll_dy"] == 7 and (info["copied"], info["other"]) == (8, 16), info
    odd.still()
    assert s.gl.GetError() == 0
    s.close()


def _the_bound(lib):
    s = fg.Session(lib, 64, 64)
    w, h = 96, 700
    sc = Scroller(s, gs.page(h + 1100, w, 4, 4), h, 550)
    sc.grab(keyframe=True)
    for dy, (want_dy, copied, other) in ((512, (512, 4, 18)), (-512, (-512, 6, 16)), (513, (0, 0, 22))):
        sc.scroll(550 - sc.at)               # (from the first slice each time)
        sc.grab()
        sc.scroll(dy)
        info = sc.grab()
        assert (info["scroll_dy"], info["copied"], info["other"]) == (want_dy, copied, other), (dy, info)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 3. fixed chrome; 4. ties and no vote

def _fixed_chrome(lib):
    s = fg.Session(lib, 64, 64)
    w, h = 200, 331
    page = gs.page(h + 200, w, 4, 5)
    chrome = gs.page(h, w, 4, 6)

    def shown(at):
        img = page[at:at + h].copy()
        img[:70] = chrome[:70]
        img[:, :70] = chrome[:, :70]
        return img
    sc = Scroller(s, page, h, 100)
    sc.show(shown(100))
    sc.prev = sc.view()
    sc.grab(keyframe=True)
    at = 100
    for dy, (same, copied, other) in ((5, (9, 6, 9)), (-37, (9, 8, 7))):
        at += dy
        sc.show(shown(at))
        info = sc.grab()
        assert info["scroll_dy"] == dy and (info["blocks_total"] - info["blocks"], info["copied"], info["other"]) == (same, copied, other), (dy, info)
    assert s.gl.GetError() == 0
    s.close()


def _ties_and_no_vote(lib):
    s = fg.Session(lib, 64, 64)
    w, h = 200, 331
    # an 8-row periodic page scrolled by 20: 4 and -4 have the most votes, the positive one wins
    period = gs.page(8, w, 4, 7)
    page = np.ascontiguousarray(np.tile(period, ((h + 64) // 8 + 1, 1, 1)))
    sc = Scroller(s, page, h, 0)
    sc.grab(keyframe=True)
    sc.scroll(20)
    v = gs.votes(sc.prev, sc.view())
    assert v[4] == v[-4] == max(v.values())
    info = sc.grab()
    assert info["scroll_dy"] == 4 and info["copied"] == 20, info
    # a solid page that changes colour: no segment is found anywhere else, and the entries are a packed delta grab's
    a, b = np.empty((h, w, 4), np.uint8), np.empty((h, w, 4), np.uint8)
    a[...] = (10, 20, 30, 255)
    b[...] = (11, 20, 30, 255)
    solid = Scroller(s, a, h, 0)
    plain = s.make(a, G.GL_RGBA8)
    solid.grab(keyframe=True)
    hosts = Hosts(a)
    check_packed(s.gl, s.gl.grab_texture(plain.id, None, DP), hosts, a, fg.blocks_of(w, h), True)
    solid.show(b)
    s.upload(plain, 0, 0, b)
    t = s.gl.grab_texture(plain.id, None, DP)
    info = solid.grab()
    assert info["scroll_dy"] == 0 and info["copied"] == 0 and info["blocks"] == 24, info
    check_packed(s.gl, t, hosts, b, fg.blocks_of(w, h), False)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 5. scroll plus change

def _scroll_plus_change(lib):
    s = fg.Session(lib, 64, 64)
    w, h = 200, 331
    sc = Scroller(s, gs.page(h + 400, w, 4, 8), h, 200)
    sc.grab(keyframe=True)
    # a scroll by 7 and a 10 x 10 patch rewritten inside the moved area: that block is sent, the rest is a pure scroll's
    img = sc.page[207:207 + h].copy()
    img[100:110, 80:90] = fg.noise(10, 10, G.GL_RGBA8, 9)
    sc.at = 207
    sc.show(img)
    info = sc.grab()
    assert info["scroll_dy"] == 7 and (info["copied"], info["other"]) == (19, 5) and info["modes"][(64, 64, 64, 64)] != gs.COPY, info
    # three scrolls in a row with no keyframe between them: a retained copy brought up to date too early, or not at all, shows
    sc.show(sc.page[207:207 + h])
    sc.grab()
    for dy in (7, -64, 65):
        sc.scroll(dy)
        info = sc.grab()
        assert info["scroll_dy"] == dy and info["keyframe"] == 0 and (info["copied"], info["other"]) == PURE[dy], (dy, info)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 6. scroll, packed and plain delta grabs of one texture

def _mixing(lib):
    s = fg.Session(lib, 64, 64)
    w, h = 200, 331
    gl = s.gl
    sc = Scroller(s, gs.page(h + 400, w, 4, 10), h, 200)
    host = np.zeros_like(sc.prev)
    blocks = fg.blocks_of(w, h)

    def sync(img):
        sc.hosts.lib[...] = sc.hosts.pure[...] = sc.hosts.numpy[...] = host[...] = img
    fg.check_delta(gl, gl.grab_texture(sc.t.id, None, DELTA), host, sc.prev, blocks, keyframe=True)      # the one keyframe
    sync(sc.prev)
    for k, (flags, dy) in enumerate(((DPS, 7), (DP, 3), (DPS, -64), (DELTA, 1), (DPS, 0), (DPS, 65), (DP, 0), (DPS | KEY, 5), (DPS, -5), (DELTA, 0))):
        if dy:
            sc.scroll(dy)
        else:
            one = blocks[(3 * k + 1) % len(blocks)]
            sc.show(tfg._one_block_change(sc.shown, one))
        want = sc.view()
        if flags & SCROLL:
            info = sc.grab(flags, keyframe=bool(flags & KEY))
            assert info["scroll_dy"] == (0 if flags & KEY else dy), (k, info)
        elif flags & PACKED:
            check_packed(gl, gl.grab_texture(sc.t.id, None, flags), sc.hosts, want, fg.changed_blocks(sc.prev, want), False)
        else:
            fg.check_delta(gl, gl.grab_texture(sc.t.id, None, flags), host, want, fg.changed_blocks(sc.prev, want), keyframe=False)
        sc.prev = want
        sync(want)
    # another rect: a keyframe; the first rect again: a keyframe too
    rect = (3, 2, w - 5, h - 3)
    part = np.ascontiguousarray(ft.crop(sc.shown, rect))
    ph = Hosts(part)
    check_scroll(gl, gl.grab_texture(sc.t.id, rect, DPS), ph, part, part, keyframe=True)
    check_scroll(gl, gl.grab_texture(sc.t.id, rect, DPS), ph, part, part)
    sc.grab(keyframe=True)
    sc.still()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 7. refusals and cost

def _refusals_and_cost(lib):
    s = fg.Session(lib, tfg.W, tfg.H)
    s.r.render(tfg._frame())
    s.r.finish()
    s.r.read_pixels()
    gl = s.gl
    assert gl.GetError() == 0
    assert glapi.GRAB_SCROLL == 1024 and glapi.GRAB_SCROLL_MAX == 512 and 1 <= glapi.GRAB_SCROLL_LAUNCHES <= 4
    one = [(0, 0, 4, 4)]
    rect = (0, 0, 64, 64)
    n0 = s.stats()["kernel_launches"]
    for k, (rects, flags) in enumerate(((one, SCROLL), (one, SCROLL | DELTA), (one, SCROLL | PACKED), (one, SCROLL | KEY), (one, SCROLL | DELTA | KEY),
                                        (one, DPS | FLIP), (one, DPS | SWAP), (one * 2, DPS), (one, DPS | 16), (one, DPS | 64), (one, DPS | 128), (one, DPS | 512),
                                        (one, 16), (one, 64), (one, 128), (one, 512))):
        assert gl.grab_texture(s.window, rects, flags) == -1, k
        assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0, k
    assert gl.grab_texture_scaled(s.window, rect, (32, 32), SCROLL) == -1
    assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    buf = gl.device_alloc(64 * 64 * 3 * 4)
    assert gl.grab_texture_tensor(s.window, rect, buf, 64 * 64 * 3 * 4, flags=SCROLL) == -1
    assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    assert gl.grab_texture_yuv(s.window, rect, glapi.YUV_I420, glapi.YUV_REC709_NARROW, flags=SCROLL) == -1
    assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    assert gl.grab_texture_yuv_delta(s.window, rect, glapi.YUV_I420, glapi.YUV_REC709_NARROW, key=SCROLL) == -1
    assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    assert gl.grab_texture_yuv_delta(s.window, rect, glapi.YUV_I420, glapi.YUV_REC709_NARROW, flags=SCROLL) == -1
    assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    assert gl.grab_texture_yuv_scaled(s.window, rect, (32, 32), glapi.YUV_I420, glapi.YUV_REC709_NARROW, flags=SCROLL) == -1
    assert gl.GetError() == G.GL_INVALID_VALUE and gl.GetError() == 0
    assert s.stats()["kernel_launches"] == n0
    gl.device_free(buf)
    # a keyframe is the packed grab's one launch; any other scroll grab is GRAB_SCROLL_LAUNCHES; nothing is flushed or drained
    for k, flags in enumerate((DPS, DPS, DPS | KEY, DPS)):
        a = s.stats()
        t = gl.grab_texture(s.window, None, flags)
        b = s.stats()
        key = k in (0, 2)
        assert t >= 0 and b["kernel_launches"] == a["kernel_launches"] + (1 if key else glapi.GRAB_SCROLL_LAUNCHES) and b["flushes"] == a["flushes"], (k, a, b)
        info, _ = gl.grab_result(t)
        assert info["flags"] == flags and info["keyframe"] == (1 if key else 0) and info["blocks"] == (64 if key else 0), info
        assert info["scroll_dy"] == 0 and info["copied"] == 0 and info["bytes"] == len(gl.grab_payload(t)), info
    # the other grabs report no vector
    for flags in (0, DELTA, DP):
        info, _ = gl.grab_result(gl.grab_texture(s.window, None, flags))
        assert info["scroll_dy"] == 0 and info["copied"] == 0, info
    # the pure decoder from Python on malformed payloads: ValueError, `into` as it was
    rec = lambda x, y, w, h, mode, aux=0: np.array([x, y, w | h << 8 | mode << 16, aux], "<u4").tobytes()
    head = lambda n, dy: np.array([n, dy & 0xFFFFFFFF, 0, 0], "<u4").tobytes()
    copy = rec(0, 0, 64, 64, gs.COPY)
    bad = [(head(16, 0) + copy, DPS), (head(16, 513) + rec(0, 0, 64, 64, gp.SOLID, 5), DPS), (head(16, -513) + rec(0, 0, 64, 64, gp.SOLID, 5), DPS),
           (head(16, 137) + copy, DPS), (head(16, -1) + copy, DPS), (head(16, 3) + rec(0, 0, 64, 64, gs.COPY, 1), DPS),
           (head(16, 3) + copy, DP), (head(16, 3) + rec(0, 0, 64, 64, gp.SOLID, 5), DP), (head(16, 3) + copy, DELTA | SCROLL), ((head(16, 3) + copy)[:24], DPS)]
    for k, (payload, flags) in enumerate(bad):
        into = fg.noise(200, 130, G.GL_RGBA8, 20 + k)
        keep = into.copy()
        with pytest.raises(ValueError):
            gl.grab_decode(payload, G.GL_RGBA8, flags, into)
        assert np.array_equal(into, keep), k
    into = fg.noise(200, 130, G.GL_RGBA8, 40)
    keep = into.copy()
    assert gl.grab_decode(head(16, 3) + copy, G.GL_RGBA8, DPS, into) == ((0, 0, 64, 64), 1)
    assert np.array_equal(into[:64, :64], keep[3:67, :64]) and np.array_equal(into[64:], keep[64:]) and np.array_equal(into[:, 64:], keep[:, 64:])
    assert gl.GetError() == 0
    s.close()


def _stream(lib, ref):
    """tests/test_frame_grabs.py's streamed rect frames with a scroll grab per frame: nothing is drained, every image is the oracle's"""
    makes = [(("rects", sd), (lambda sd=sd: scenes.cfg2_overlapping_rects(n=60, seed=sd, **stream_cases.W))) for sd in tfg.RECT_SEEDS]
    px, st, images, infos = render_streamed_grabbed(lib, [m() for _, m in makes], delta=True, packed=True, scroll=True)
    assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
    assert st["setup_carried"] >= len(makes) - 1, st
    assert len(images) == len(infos) == len(makes)
    for k, ((key, make), img, info) in enumerate(zip(makes, images, infos)):
        want = ft.window_stored(tfg._ref_render(ref, key, make))
        assert np.array_equal(img, want), f"frame {k} ({key}) is not the oracle's render"
        assert info["status"] == 0 and info["flags"] == DPS and info["keyframe"] == (1 if k == 0 else 0), info
    assert np.array_equal(px, tfg._ref_render(ref, makes[-1][0], makes[-1][1]))


# ---------------------------------------------------------------------------- 8. ordering

def _parked(lib, ref):
    W, H = tfg.W, tfg.H
    want1 = ft.window_stored(tfg._ref_render(ref, "cfg2", tfg._frame))
    s = fg.Session(lib, W, H)
    gl = s.gl
    win = device.Texture(s.window, W, H, G.GL_RGBA8)
    # a scroll grab parked behind held-back raster launches; a later upload -- the window scrolled by 9 -- does not change its result
    s.r.render(tfg._frame())
    hosts = Hosts(want1)
    t = gl.grab_texture(s.window, None, DPS)
    want2 = want1.copy()
    want2[:H - 9] = want1[9:]
    s.upload(win, 0, 0, want2)
    t2 = gl.grab_texture(s.window, None, DPS)
    check_scroll(gl, t, hosts, want1, want1, keyframe=True)
    info = check_scroll(gl, t2, hosts, want1, want2)
    assert info["scroll_dy"] == 9 and info["copied"] > 0, info
    s.r.finish()
    # nine tickets against the ring of 8, parked: the first is dropped with its ticket -- it would have brought the retained copy
    # up to date --, so the second sends every block in its place
    s.upload(win, 0, 0, want1)
    s.r.render(tfg._frame())
    tickets = [gl.grab_texture(s.window, None, DPS) for _ in range(9)]
    assert len(set(tickets)) == 9
    with pytest.raises(KeyError):
        gl.grab_result(tickets[0])
    gt.send_held(gl)
    hosts = Hosts(want1)
    check_scroll(gl, tickets[1], hosts, want1, want1, keyframe=True)
    for t in tickets[2:]:
        info = check_scroll(gl, t, hosts, want1, want1)
        assert info["bytes"] == fg.HEADER, info
    want3 = want1.copy()
    want3[12:] = want1[:H - 12]
    s.upload(win, 0, 0, want3)
    info = check_scroll(gl, gl.grab_texture(s.window, None, DPS), hosts, want1, want3)
    assert info["scroll_dy"] == -12 and info["copied"] > 0, info
    s.r.finish()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 9. the decoder, stand-alone; 10. budget (CPU only)

def test_scroll_decoder_on_hostile_input(tmp_path):
    """tools/grab_scroll_check.cpp -- wr_grab_codec.h alone, its own main -- under AddressSanitizer and UBSan, as a process of its own"""
    cxx = shutil.which("g++")
    flags = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    trivial = tmp_path / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    if cxx is None or subprocess.run([cxx] + flags + [str(trivial), "-o", str(tmp_path / "trivial")], capture_output=True).returncode != 0:
        pytest.skip("no g++ that links with -fsanitize=address,undefined")
    exe = tmp_path / "grab_scroll_check"
    subprocess.run([cxx] + flags + ["-I", os.path.join(ROOT, "webrender_amd", "csrc"), os.path.join(ROOT, "tools", "grab_scroll_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "grab_scroll_check: ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_scroll_grab_kernels_have_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    for name in ("wr_grab_scroll_probe_kernel", "wr_grab_scroll_vote_kernel", "wr_grab_scroll_pack_kernel", "wr_grab_scroll_update_kernel"):
        assert name in notes, sorted(notes)
        vgprs, scratch = notes[name]
        assert scratch == 0, (name, vgprs, scratch)


# ---------------------------------------------------------------------------- CPU: the host simulation

def test_hostsim_pure_scrolls(hostsim):
    _pure_scrolls(hostsim)


def test_hostsim_the_bound(hostsim):
    _the_bound(hostsim)


def test_hostsim_fixed_chrome(hostsim):
    _fixed_chrome(hostsim)


def test_hostsim_ties_and_no_vote(hostsim):
    _ties_and_no_vote(hostsim)


def test_hostsim_scroll_plus_change(hostsim):
    _scroll_plus_change(hostsim)


def test_hostsim_mixing(hostsim):
    _mixing(hostsim)


def test_hostsim_refusals_and_cost(hostsim):
    _refusals_and_cost(hostsim)


def test_hostsim_scroll_stream(hostsim, oracle_gcc):
    _stream(hostsim, oracle_gcc)


def test_hostsim_parked(hostsim, oracle_gcc):
    _parked(hostsim, oracle_gcc)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
def test_gpu_pure_scrolls():
    _pure_scrolls(wrhip_lib())


@pytest.mark.gpu
def test_gpu_the_bound():
    _the_bound(wrhip_lib())


@pytest.mark.gpu
def test_gpu_fixed_chrome():
    _fixed_chrome(wrhip_lib())


@pytest.mark.gpu
def test_gpu_ties_and_no_vote():
    _ties_and_no_vote(wrhip_lib())


@pytest.mark.gpu
def test_gpu_scroll_plus_change():
    _scroll_plus_change(wrhip_lib())


@pytest.mark.gpu
def test_gpu_mixing():
    _mixing(wrhip_lib())


@pytest.mark.gpu
def test_gpu_refusals_and_cost():
    _refusals_and_cost(wrhip_lib())


@pytest.mark.gpu
def test_gpu_scroll_stream():
    _stream(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_parked():
    _parked(wrhip_lib(), _gpu_ref())
