"""Texture taps (include/wrhip.h: WrhipTapTexture / WrhipTapResultGet): a digest of a texture rect and, against an expected
texture, wrench's difference histogram, taken on the device in stream order -- behind held-back raster launches too -- and
delivered through a ring of tickets.  Every comparison is an exact integer equality against the numpy restatement in
tests/frame_taps.py.  Each check runs on the host simulation and, under -m gpu, on the MI355X."""
import ctypes as C
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
import frame_taps as ft
import stream_cases
import tile_size_cases
from webrender_amd import scenes, glapi, glconst as G
from webrender_amd.harness import render_direct, render_streamed_tapped
from webrender_amd.renderer import Renderer

RESULT_BYTES = C.sizeof(glapi.WrhipTapResult)
W = H = 512
# the rects of the digest test, in a 512 x 512 RGBA8 window and a 513 x 513 R8 mask atlas (R8 rows of 516 bytes: every second
# row starts 4 bytes past a 16-byte boundary)
RECTS = [None, (0, 0, 1, 1), "last", (3, 5, 61, 37), (1, 2, 333, 201), (507, 0, 5, "h"), (0, 77, "w", 1)]
ATLAS = 513


def _frame():
    return scenes.cfg2_overlapping_rects(n=200, seed=44, encoding="brush", width=W, height=H)


def _mask_frame():
    return scenes.box_shadow_masks(n=5, atlas=ATLAS, seed=49, pin_corner=True)


def _rect(r, w, h):
    if r is None:
        return (0, 0, w, h)
    if r == "last":
        return (w - 1, h - 1, 1, 1)
    return tuple(w if v == "w" else h if v == "h" else v for v in r)


_refs = {}


def _ref_render(ref, key, make):
    """The oracle's render of a frame, computed once per session and backend"""
    if (ref, key) not in _refs:
        out, _ = render_direct(ref, make())
        _refs[(ref, key)] = out
    return _refs[(ref, key)]


class Session:
    """One context: frames rendered through the Python mirror, taps, readbacks"""

    def __init__(self, lib, w=W, h=H):
        self.gl = glapi.GL(lib)
        self.r = Renderer(self.gl, w, h)
        self.d = self.r.device
        self.window = self.gl.WrhipGetFramebufferTexture(0)

    def tex(self, name):
        return self.r.textures[name]

    def make(self, px, fmt, render_target=True):
        """A texture holding the stored bytes `px` ((h, w, 4) BGRA or (h, w) R8)"""
        h, w = px.shape[:2]
        t = self.d.create_texture(w, h, fmt, render_target=render_target)
        self.d.upload_texture(t, 0, 0, w, h, G.GL_RED if fmt == G.GL_R8 else G.GL_BGRA, G.GL_UNSIGNED_BYTE, np.ascontiguousarray(px))
        return t

    def window_stored(self):
        return ft.window_stored(self.r.read_pixels())

    def launches(self):
        return self.gl.stats()["kernel_launches"]

    def close(self):
        self.r.destroy()


def _noise(h, w, fmt, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if fmt == G.GL_R8 else (h, w, 4), dtype=np.uint8)


# ---------------------------------------------------------------------------- 0. row order

def _row_orientation(lib):
    s = Session(lib)
    s.r.render(_frame())
    top = s.gl.tap_texture(s.window, (0, 0, W, H // 2))
    s.r.finish()
    got = s.gl.tap_result(top)
    px = s.window_stored()
    s.close()
    assert not np.array_equal(px[:H // 2], px[H // 2:][::-1]) and not np.array_equal(px[:H // 2], px[H // 2:])
    assert tuple(got["digest"]) == ft.digest(px[:H // 2])
    assert tuple(got["digest"]) != ft.digest(px[H // 2:]) and tuple(got["digest"]) != ft.digest(px[::-1][:H // 2])


# ---------------------------------------------------------------------------- 1. the digest is the specified function

def _digest_is_specified(lib):
    # RGBA8: the window (tapped behind its held-back launches) and two picture tiles of odd sizes; R8: a mask atlas, and two
    # textures of the same odd sizes
    s = Session(lib)
    s.r.render(_frame())
    taps = [(s.gl.tap_texture(s.window, None if r is None else _rect(r, W, H)), _rect(r, W, H)) for r in RECTS]
    s.r.finish()
    assert s.gl.GetError() == 0
    px = s.window_stored()
    for t, rect in taps:
        ft.check_digest(s.gl.tap_result(t), ft.crop(px, rect), G.GL_RGBA8)
    # teeth: two pixels swapped, one byte off by one
    whole = ft.digest(px)
    sw = px.copy()
    sw[10, 20], sw[300, 400] = px[300, 400], px[10, 20]
    assert not np.array_equal(px[10, 20], px[300, 400]) and ft.digest(sw) != whole
    assert ft.digest(sw)[0] != whole[0] and ft.digest(sw)[1] != whole[1]
    one = px.copy()
    one[511, 511, 2] = (int(one[511, 511, 2]) + 1) & 255
    assert ft.digest(one)[0] != whole[0] and ft.digest(one)[1] != whole[1]
    s.close()

    for tile in ((61, 37), (130, 64)):
        frame = tile_size_cases.build_tile_frame(tile, "rects_brush")
        s = Session(lib, frame.width, frame.height)
        s.r.render(frame)
        names = [tg.texture.name for tg in tile_size_cases.picture_tiles(frame)][:2]
        taps = [(s.gl.tap_texture(s.tex(n).id), n) for n in names]
        s.r.finish()
        for t, n in taps:
            stored = s.d.read_texture(s.tex(n))
            assert stored.shape[:2] == (tile[1], tile[0])
            ft.check_digest(s.gl.tap_result(t), stored, G.GL_RGBA8)
        s.close()

    frame = _mask_frame()
    s = Session(lib, frame.width, frame.height)
    s.r.render(frame)
    mask = s.tex("box_shadow_masks")
    taps = [(s.gl.tap_texture(mask.id, None if r is None else _rect(r, ATLAS, ATLAS)), _rect(r, ATLAS, ATLAS)) for r in RECTS]
    small = [(s.make(_noise(th, tw, G.GL_R8, 7 + tw), G.GL_R8), _noise(th, tw, G.GL_R8, 7 + tw)) for tw, th in ((61, 37), (130, 64))]
    taps_small = [s.gl.tap_texture(t.id) for t, _ in small]
    s.r.finish()
    px = s.d.read_texture(mask)
    assert len(np.unique(px)) > 16          # (a mask with shadow ramps in it, not a cleared atlas)
    for t, rect in taps:
        ft.check_digest(s.gl.tap_result(t), ft.crop(px, rect), G.GL_R8)
    for t, (tex, want) in zip(taps_small, small):
        assert np.array_equal(s.d.read_texture(tex), want)
        ft.check_digest(s.gl.tap_result(t), want, G.GL_R8)
    s.close()


# ---------------------------------------------------------------------------- 2. the comparison is wrench's

def _perturb(stored, rng):
    """~40 known pixels of a copy changed by known amounts; -> the copy"""
    out = stored.copy()
    h, w = stored.shape[:2]
    rgba = stored.ndim == 3
    spots = {(0, 0), (h - 1, w - 1)}
    while len(spots) < 40:
        spots.add((int(rng.integers(0, h)), int(rng.integers(0, w))))

    def bump(y, x, c, by):
        if rgba:
            out[y, x, c] = np.clip(int(out[y, x, c]) + (by if int(out[y, x, c]) + by <= 255 and int(out[y, x, c]) + by >= 0 else -by), 0, 255)
        else:
            out[y, x] = np.clip(int(out[y, x]) + (by if 0 <= int(out[y, x]) + by <= 255 else -by), 0, 255)
    for i, (y, x) in enumerate(sorted(spots)):
        kind = i % 4
        if kind == 0:
            bump(y, x, 0, 1)                        # +1 on B only
        elif kind == 1:
            bump(y, x, 3, -3)                       # -3 on alpha only
        elif kind == 2:                             # 255 on one channel where it holds 0 or 255 (alpha, a cleared mask), >= 128 elsewhere
            if rgba:
                out[y, x, 3] = 0 if stored[y, x, 3] >= 128 else 255
            else:
                out[y, x] = 0 if stored[y, x] >= 128 else 255
        else:                                       # two channels by different amounts
            bump(y, x, 2, 7)
            if rgba:
                bump(y, x, 0, 19)
    return out


def _compare_case(s, tex_id, rect, got_stored, want_stored, fmt, seed):
    """Tap `rect` of `tex_id` against `want_stored` (the oracle's bytes of that rect) unperturbed and perturbed"""
    w, h = rect[2], rect[3]
    assert want_stored.shape[:2] == (h, w)
    pert = _perturb(want_stored, np.random.default_rng(seed))
    assert ft.histogram(want_stored, pert)[2] >= 38
    e0, e1 = s.make(want_stored, fmt), s.make(pert, fmt)
    t0, t1 = s.gl.tap_texture(tex_id, rect, e0.id), s.gl.tap_texture(tex_id, rect, e1.id)
    assert t0 >= 0 and t1 >= 0
    r0, r1 = s.gl.tap_result(t0), s.gl.tap_result(t1)
    assert r0["hist"][0] == w * h and r0["max_diff"] == 0 and r0["differing"] == 0, "the backend's frame is not the oracle's"
    hist, mx, n = ft.histogram(ft.crop(got_stored, rect), pert)
    assert (r1["hist"], r1["max_diff"], r1["differing"]) == (hist, mx, n)
    assert n >= 38 and hist[1] > 0 and hist[3] > 0 and mx >= 128
    assert tuple(r1["digest"]) == ft.digest(ft.crop(got_stored, rect)) == tuple(r0["digest"])
    assert (r1["width"], r1["height"], r1["format"]) == (w, h, fmt)


def _comparison_is_wrenchs(lib, ref):
    want = ft.window_stored(_ref_render(ref, "cfg2", _frame))
    s = Session(lib)
    s.r.render(_frame())
    s.r.finish()
    got = s.window_stored()
    _compare_case(s, s.window, (0, 0, W, H), got, want, G.GL_RGBA8, 1)
    sub = (3, 5, 61, 37)
    _compare_case(s, s.window, sub, got, ft.crop(want, sub).copy(), G.GL_RGBA8, 2)
    # refusals: -1, GL_INVALID_VALUE, nothing launched
    e_rgba, e_r8, e_small = s.make(want, G.GL_RGBA8), s.make(_noise(H, W, G.GL_R8, 3), G.GL_R8), s.make(want[:100, :100], G.GL_RGBA8)
    s.r.finish()
    assert s.gl.GetError() == 0
    n0 = s.launches()
    bad = [
        lambda: s.gl.tap_texture(s.window, (0, 0, W, H), e_r8.id),            # another format
        lambda: s.gl.tap_texture(s.window, (0, 0, 101, 100), e_small.id),     # expected too small
        lambda: s.gl.tap_texture(s.window, (500, 0, 13, 1)),                  # outside the texture
        lambda: s.gl.tap_texture(s.window, (0, -1, 4, 4)),
        lambda: s.gl.tap_texture(s.window, (0, 0, 0, 4)),
        lambda: s.gl.tap_texture(9999, (0, 0, 1, 1)),                         # unknown texture
        lambda: s.gl.tap_texture(s.window, (0, 0, 4, 4), 9999),
    ]
    for call in bad:
        assert call() == -1
        assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0
    s.gl.WrhipSetShard(0, 2)
    assert s.gl.tap_texture(s.window, (0, 0, W, H), e_rgba.id) == -1
    assert s.gl.GetError() == G.GL_INVALID_VALUE
    s.gl.WrhipSetShard(0, 1)
    s.gl.WrhipSetTargetRows(s.window, 0, 256)
    assert s.gl.tap_texture(s.window, (0, 0, 4, 4)) == -1
    assert s.gl.GetError() == G.GL_INVALID_VALUE
    s.gl.WrhipSetTargetRows(s.window, 0, 0)
    assert s.launches() == n0
    assert s.gl.tap_texture(s.window, (0, 0, 100, 100), e_small.id) >= 0 and s.launches() == n0 + 1
    s.close()

    # R8: the mask atlas, whole and a sub-rect at an odd origin against a smaller expected texture
    ref_out = _ref_render(ref, "masks", _mask_frame)
    want = ref_out["box_shadow_masks"]
    frame = _mask_frame()
    s = Session(lib, frame.width, frame.height)
    s.r.render(frame)
    s.r.finish()
    mask = s.tex("box_shadow_masks")
    got = s.d.read_texture(mask)
    _compare_case(s, mask.id, (0, 0, ATLAS, ATLAS), got, want, G.GL_R8, 4)
    # (the last task is pinned to the atlas's corner: this rect has shadow ramps in it)
    sub = (ATLAS - 61 - 2, ATLAS - 37 - 4, 61, 37)
    assert len(np.unique(ft.crop(want, sub))) > 4
    _compare_case(s, mask.id, sub, got, ft.crop(want, sub).copy(), G.GL_R8, 5)
    s.close()


# ---------------------------------------------------------------------------- 3. one launch, nothing drained

def _one_launch(lib):
    s = Session(lib)
    s.r.render(_frame())
    s.r.finish()
    s.r.read_pixels()
    a = s.gl.stats()
    t = s.gl.tap_texture(s.window)
    b = s.gl.stats()
    assert b["kernel_launches"] == a["kernel_launches"] + 1
    assert b["flushes"] == a["flushes"]
    assert s.gl.tap_result(t)["status"] == 0
    c = s.gl.stats()
    assert c["d2h_bytes"] == a["d2h_bytes"] + RESULT_BYTES
    assert c["kernel_launches"] == b["kernel_launches"] and c["flushes"] == a["flushes"]
    s.close()


# ---------------------------------------------------------------------------- 4. every frame of a stream

# four fixed sequences of 6-10 menu frames, and cfg2 rects that differ in colours and seed only: every flush of that one, carried
# and carrying, is the rect-only fused launch
SEQUENCES = [("menu%d" % i, seq) for i, seq in enumerate(stream_cases.random_sequences(seed=515, count=4, lo=6, hi=10))]
RECT_SEEDS = (40, 71, 72, 73, 74, 75)


def _stream(lib, ref, name, seq, on_gpu):
    if seq is None:
        makes = [(("rects", sd), (lambda sd=sd: scenes.cfg2_overlapping_rects(n=60, seed=sd, **stream_cases.W))) for sd in RECT_SEEDS]
        carried = len(makes) - 1
    else:
        assert set(seq) <= set(stream_cases.menu_ok())
        if on_gpu:
            seq = [i for i in seq if i not in stream_cases.DEVICE_INEXACT]
        makes = [(("menu", i), stream_cases.MENU[i]) for i in seq]
        carried = stream_cases.carriers_expected(seq)
    px, st, taps = render_streamed_tapped(lib, [m() for _, m in makes])
    assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
    assert st["setup_carried"] >= carried, (st, carried)          # (a tap that drained the held-back launches would lose these)
    assert len(taps) == len(makes)
    bad = []
    for k, ((key, make), res) in enumerate(zip(makes, taps)):
        want = ft.window_stored(_ref_render(ref, key, make))
        assert (res["status"], res["width"], res["height"], res["format"]) == (0, want.shape[1], want.shape[0], G.GL_RGBA8)
        if tuple(res["digest"]) != ft.digest(want):
            bad.append((k, key))
    assert not bad, f"{name}: frames whose digest is not the oracle's: {bad}"
    assert np.array_equal(px, _ref_render(ref, makes[-1][0], makes[-1][1]))


# ---------------------------------------------------------------------------- 5. lifetime and tickets

def _lifetime_and_tickets(lib):
    f1, f2 = _frame(), scenes.cfg2_overlapping_rects(n=150, seed=45, encoding="brush", width=W, height=H)
    want1 = ft.window_stored(render_direct(lib, _frame())[0])
    # the window is tapped, then cleared and drawn again with no Finish in between
    s = Session(lib)
    s.r.render(f1)
    t = s.gl.tap_texture(s.window)
    early = s.gl.tap_result(t, wait=False)          # (never KeyError: None, or the result)
    s.r.render(f2)
    s.r.finish()
    res = s.gl.tap_result(t)
    assert early is None or early == res
    ft.check_digest(res, want1, G.GL_RGBA8)
    assert ft.digest(s.window_stored()) != ft.digest(want1)
    # a picture tile is tapped behind the held-back launches that draw it, then deleted
    s.r.render(f1)
    name = tile_size_cases.picture_tiles(f1)[0].texture.name
    tile = s.r.textures.pop(name)
    t = s.gl.tap_texture(tile.id)
    s.d.delete_texture(tile)
    s.r.finish()
    res_tile = s.gl.tap_result(t)
    s.close()
    f1.readback = [tile_size_cases.picture_tiles(f1)[0].texture]
    ft.check_digest(res_tile, render_direct(lib, f1)[0][name], G.GL_RGBA8)

    # a texture is tapped and deleted on an idle context; a ticket polled at once; more taps than the ring holds
    s = Session(lib, 64, 64)
    s.r.finish()
    px = _noise(37, 61, G.GL_RGBA8, 11)
    tex = s.make(px, G.GL_RGBA8)
    t = s.gl.tap_texture(tex.id)
    polled = s.gl.tap_result(t, wait=False)
    s.d.delete_texture(tex)
    other = s.make(_noise(37, 61, G.GL_RGBA8, 12), G.GL_RGBA8)      # (takes the freed storage over)
    s.r.finish()
    res = s.gl.tap_result(t)
    assert polled is None or polled == res
    ft.check_digest(res, px, G.GL_RGBA8)
    out = glapi.WrhipTapResult()
    assert s.gl.WrhipTapResultGet(t, C.byref(out), 0) == 0 and s.gl.WrhipTapResultGet(t, C.byref(out), 1) == 0
    assert s.gl.WrhipTapResultGet(-5, C.byref(out), 1) == -1 and s.gl.WrhipTapResultGet(-5, C.byref(out), 0) == -1
    assert s.gl.WrhipTapResultGet(t + 1, C.byref(out), 1) == -1         # (never handed out)
    srcs = [_noise(5, 9, G.GL_R8, 100 + k) for k in range(4)]
    texs = [s.make(p, G.GL_R8) for p in srcs]
    n = 64 + 6
    tickets = [s.gl.tap_texture(texs[k % 4].id) for k in range(n)]
    assert len(set(tickets)) == n and min(tickets) >= 0
    for k in range(n - 64):
        assert s.gl.WrhipTapResultGet(tickets[k], C.byref(out), 1) == -1
        with pytest.raises(KeyError):
            s.gl.tap_result(tickets[k])
    for k in (n - 64, n - 33, n - 2, n - 1):
        ft.check_digest(s.gl.tap_result(tickets[k]), srcs[k % 4], G.GL_R8)
    s.d.delete_texture(other)
    s.close()


# ---------------------------------------------------------------------------- CPU: the host simulation

def test_hostsim_row_orientation(hostsim, oracle_gcc):
    _row_orientation(hostsim)


def test_hostsim_digest_is_the_specified_function(hostsim, oracle_gcc):
    _digest_is_specified(hostsim)


def test_hostsim_comparison_is_wrenchs(hostsim, oracle_gcc):
    _comparison_is_wrenchs(hostsim, oracle_gcc)


def test_hostsim_one_launch_nothing_drained(hostsim, oracle_gcc):
    _one_launch(hostsim)


@pytest.mark.parametrize("name,seq", SEQUENCES + [("rects", None)], ids=[n for n, _ in SEQUENCES] + ["rects"])
def test_hostsim_every_frame_of_a_stream(hostsim, oracle_gcc, name, seq):
    _stream(hostsim, oracle_gcc, name, seq, on_gpu=False)


def test_hostsim_lifetime_and_tickets(hostsim, oracle_gcc):
    _lifetime_and_tickets(hostsim)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
def test_gpu_row_orientation():
    _gpu_ref()
    _row_orientation(wrhip_lib())


@pytest.mark.gpu
def test_gpu_digest_is_the_specified_function():
    _gpu_ref()
    _digest_is_specified(wrhip_lib())


@pytest.mark.gpu
def test_gpu_comparison_is_wrenchs():
    _comparison_is_wrenchs(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_one_launch_nothing_drained():
    _gpu_ref()
    _one_launch(wrhip_lib())


@pytest.mark.gpu
@pytest.mark.parametrize("name,seq", SEQUENCES + [("rects", None)], ids=[n for n, _ in SEQUENCES] + ["rects"])
def test_gpu_every_frame_of_a_stream(name, seq):
    _stream(wrhip_lib(), _gpu_ref(), name, seq, on_gpu=True)


@pytest.mark.gpu
def test_gpu_lifetime_and_tickets():
    _gpu_ref()
    _lifetime_and_tickets(wrhip_lib())
