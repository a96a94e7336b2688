"""Texture grabs (include/wrhip.h: WrhipGrabTexture / WrhipGrabResultGet): the pixels of texture rects, or the 64 x 64 blocks of a
rect that changed since its previous grab, packed on the device in stream order -- behind held-back raster launches too -- and
delivered through a ring of 8 tickets.  Every comparison is byte for byte against the oracle's render or against bytes the test
uploaded, never against libwrhip's own readback.  Each check runs on the host simulation and, under -m gpu, on the MI355X."""
import ctypes as C
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
import frame_taps as ft
import frame_grabs as fg
import stream_cases
import tile_size_cases
from webrender_amd import scenes, glapi, glconst as G, device
from webrender_amd.harness import render_direct, render_streamed_grabbed

W = H = 512
ATLAS = 513
RECTS = [None, (0, 0, 1, 1), "last", (3, 5, 61, 37), (1, 2, 333, 201), ("w-5", 0, 5, "h"), (0, 77, "w", 1)]
FLIP, SWAP, DELTA, KEY = glapi.GRAB_FLIP_ROWS, glapi.GRAB_SWAP_RB, glapi.GRAB_DELTA, glapi.GRAB_KEY


def _frame():
    return scenes.cfg2_overlapping_rects(n=200, seed=44, encoding="brush", width=W, height=H)


def _mask_frame():
    return scenes.box_shadow_masks(n=5, atlas=ATLAS, seed=49, pin_corner=True)


def _rect(r, w, h):
    if r is None:
        return (0, 0, w, h)
    if r == "last":
        return (w - 1, h - 1, 1, 1)
    return tuple(w if v == "w" else h if v == "h" else w - 5 if v == "w-5" else v for v in r)


def _rects_in(w, h):
    """RECTS as far as they lie inside a w x h texture (the row of RECTS at y = 77: at h // 2 in a lower one)"""
    out = []
    for r in RECTS:
        x, y, rw, rh = _rect(r, w, h)
        if rh == 1 and rw == w and y >= h:
            y = h // 2
        if x >= 0 and y >= 0 and x + rw <= w and y + rh <= h:
            out.append((x, y, rw, rh))
    return out


_refs = {}


def _ref_render(ref, key, make):
    """The oracle's render of a frame, computed once per session and backend; never modified"""
    if (ref, key) not in _refs:
        out, _ = render_direct(ref, make())
        _refs[(ref, key)] = out
    return _refs[(ref, key)]


def _raw_get(gl, ticket, shape, stride):
    """WrhipGrabResultGet into rows of `stride` bytes: -> (the rows' pixels, the padding behind them)"""
    h, row = shape[0], int(np.prod(shape[1:]))
    buf = np.full((h, stride), 0xA5, np.uint8)
    info = glapi.WrhipGrabInfo()
    assert gl.WrhipGrabResultGet(ticket, C.byref(info), buf.ctypes.data, stride, 1) == 0
    return buf[:, :row].reshape(shape), buf[:, row:]


# ---------------------------------------------------------------------------- 1. full grabs are the stored bytes

def _check_texture(s, tex_id, want, flip_rect):
    """Every grab of the full-mode test on one texture whose stored bytes are `want`; the tickets are fetched by the caller's
    order of business: here, at once (a fetch waits for its own ticket only)"""
    gl = s.gl
    h, w = want.shape[:2]
    rgba = want.ndim == 3
    rects = _rects_in(w, h)
    fmt = G.GL_RGBA8 if rgba else G.GL_R8
    singles = [(gl.grab_texture(tex_id, None if r == (0, 0, w, h) else r), r) for r in rects]
    all_at_once = gl.grab_texture(tex_id, rects)
    assert len(singles) + 1 <= 8          # (the ring: nothing fetched yet is overwritten)
    for t, r in singles:
        info, px = gl.grab_result(t)
        assert (info["status"], info["format"], info["rects"], info["flags"]) == (0, fmt, [r], 0), info
        assert info["bytes"] == fg.HEADER + r[2] * r[3] * (4 if rgba else 1)
        assert np.array_equal(px, ft.crop(want, r)), r
    info, parts = gl.grab_result(all_at_once)
    assert info["rects"] == rects and len(parts) == len(rects) > 1
    for px, r in zip(parts, rects):
        assert np.array_equal(px, ft.crop(want, r)), r
    flags = [FLIP, SWAP, FLIP | SWAP] if rgba else [FLIP]
    flagged = [(gl.grab_texture(tex_id, flip_rect, f), f) for f in flags]
    for t, f in flagged:
        info, px = gl.grab_result(t)
        plain = ft.crop(want, flip_rect)
        assert info["flags"] == f and np.array_equal(px, fg.flagged(plain, f)), f
        assert not np.array_equal(px, plain)              # (the flag did something to this rect)
    # rows at a stride larger than tight, and tight by 0: the same bytes, the padding untouched
    t = gl.grab_texture(tex_id, flip_rect)
    tight = flip_rect[2] * (4 if rgba else 1)
    shape = ft.crop(want, flip_rect).shape
    px, pad = _raw_get(gl, t, shape, tight + 24)
    assert np.array_equal(px, ft.crop(want, flip_rect)) and (pad == 0xA5).all()
    px0, _ = _raw_get(gl, t, shape, tight)
    buf = np.full(shape, 0xA5, np.uint8)
    info = glapi.WrhipGrabInfo()
    assert gl.WrhipGrabResultGet(t, C.byref(info), buf.ctypes.data, 0, 1) == 0
    assert np.array_equal(buf, px0) and np.array_equal(buf, ft.crop(want, flip_rect))


def _full_grabs(lib, ref):
    # the window, grabbed before the Finish: behind its held-back launches
    want = ft.window_stored(_ref_render(ref, "cfg2", _frame))
    assert not np.array_equal(want[:H // 2], want[H // 2:]) and not np.array_equal(want[:H // 2], want[H // 2:][::-1])
    s = fg.Session(lib, W, H)
    s.r.render(_frame())
    _check_texture(s, s.window, want, (3, 5, 61, 37))
    # sixteen rects in one grab, two of them overlapping
    rng = np.random.default_rng(5)
    rects = [(int(x), int(y), int(rw), int(rh)) for x, y, rw, rh in
             zip(rng.integers(0, 300, 14), rng.integers(0, 300, 14), rng.integers(1, 200, 14), rng.integers(1, 200, 14))]
    rects += [(100, 100, 64, 64), (130, 90, 65, 33)]
    t = s.gl.grab_texture(s.window, rects)
    s.r.finish()
    assert s.gl.GetError() == 0
    info, parts = s.gl.grab_result(t)
    assert info["rects"] == rects and len(parts) == 16
    for px, r in zip(parts, rects):
        assert np.array_equal(px, ft.crop(want, r)), r
    s.close()

    # the R8 mask atlas (rows of 516 bytes), drawn; noise textures of both formats, uploaded
    want = _ref_render(ref, "masks", _mask_frame)["box_shadow_masks"]
    assert want.shape == (ATLAS, ATLAS) and len(np.unique(want)) > 16
    assert not np.array_equal(want[:256], want[257:]) and not np.array_equal(want[:256], want[257:][::-1])
    frame = _mask_frame()
    s = fg.Session(lib, frame.width, frame.height)
    s.r.render(frame)
    _check_texture(s, s.tex("box_shadow_masks").id, want, (3, 5, 61, 37))
    s.r.finish()
    for (tw, th) in ((61, 37), (333, 201)):
        for fmt in (G.GL_RGBA8, G.GL_R8):
            px = fg.noise(th, tw, fmt, tw + (1 if fmt == G.GL_R8 else 0))
            _check_texture(s, s.make(px, fmt).id, px, (3, 5, 33, 21))
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 2. one launch, nothing drained

def _one_launch(lib):
    s = fg.Session(lib, W, H)
    s.r.render(_frame())
    s.r.finish()
    s.r.read_pixels()
    r8 = s.make(fg.noise(37, 61, G.GL_R8, 3), G.GL_R8)
    s.r.finish()
    assert s.gl.GetError() == 0
    for flags in (0, DELTA, DELTA):
        a = s.stats()
        t = s.gl.grab_texture(s.window, None, flags)
        b = s.stats()
        # (kernel_launches counts the pack; the transport -- wr_grab_push_kernel or a plain copy, on the library's second
        # stream -- is not a launch of the frame's stream and is not counted)
        assert b["kernel_launches"] == a["kernel_launches"] + 1
        assert b["flushes"] == a["flushes"]
        info, _ = s.gl.grab_result(t)
        c = s.stats()
        assert c["d2h_bytes"] == a["d2h_bytes"] + info["bytes"]
        assert c["kernel_launches"] == b["kernel_launches"] and c["flushes"] == a["flushes"]
        s.gl.grab_result(t)
        assert s.stats()["d2h_bytes"] == c["d2h_bytes"]          # (a second fetch carries nothing)
    n0 = s.stats()["kernel_launches"]
    one = [(0, 0, 4, 4)]
    bad = [
        lambda: s.gl.grab_texture(s.window, (500, 0, 13, 1)),                     # outside the texture
        lambda: s.gl.grab_texture(s.window, (0, -1, 4, 4)),
        lambda: s.gl.grab_texture(s.window, [(0, 0, 4, 4), (0, 510, 4, 3)]),
        lambda: s.gl.grab_texture(s.window, (0, 0, 0, 4)),                        # empty
        lambda: s.gl.grab_texture(s.window, (0, 0, 4, 0)),
        lambda: s.gl.grab_texture(s.window, []),                                  # 0 rects
        lambda: s.gl.grab_texture(s.window, one * 17),                            # 17 rects
        lambda: s.gl.grab_texture(s.window, one * 2, DELTA),
        lambda: s.gl.grab_texture(s.window, one, DELTA | FLIP),
        lambda: s.gl.grab_texture(s.window, one, DELTA | SWAP),
        lambda: s.gl.grab_texture(r8.id, one, SWAP),                              # SWAP_RB on R8
        lambda: s.gl.grab_texture(9999, one),                                     # unknown texture
        lambda: s.gl.grab_texture(s.window, one, 16),                             # unknown flag
    ]
    for k, call in enumerate(bad):
        assert call() == -1, k
        assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0, k
    s.gl.WrhipSetShard(0, 2)
    assert s.gl.grab_texture(s.window, one) == -1
    assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0
    s.gl.WrhipSetShard(0, 1)
    s.gl.WrhipSetTargetRows(s.window, 0, 256)
    assert s.gl.grab_texture(s.window, one) == -1
    assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0
    s.gl.WrhipSetTargetRows(s.window, 0, 0)
    assert s.stats()["kernel_launches"] == n0
    assert s.gl.grab_texture(s.window, one * 16) >= 0 and s.stats()["kernel_launches"] == n0 + 1
    s.close()


# ---------------------------------------------------------------------------- 3. every frame of a stream

SEQUENCES = [("menu%d" % i, seq) for i, seq in enumerate(stream_cases.random_sequences(seed=515, count=4, lo=6, hi=10))]
RECT_SEEDS = (40, 71, 72, 73, 74, 75)


def _stream(lib, ref, name, seq, on_gpu, delta=False):
    if seq is None:
        makes = [(("rects", sd), (lambda sd=sd: scenes.cfg2_overlapping_rects(n=60, seed=sd, **stream_cases.W))) for sd in RECT_SEEDS]
        carried = len(makes) - 1
    else:
        assert set(seq) <= set(stream_cases.menu_ok())
        if on_gpu:
            seq = [i for i in seq if i not in stream_cases.DEVICE_INEXACT]
        makes = [(("menu", i), stream_cases.MENU[i]) for i in seq]
        carried = stream_cases.carriers_expected(seq)
    px, st, images, infos = render_streamed_grabbed(lib, [m() for _, m in makes], delta=delta)
    assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
    assert st["setup_carried"] >= carried, (st, carried)          # (a grab that drained the held-back launches would lose these)
    assert len(images) == len(infos) == len(makes)
    bad = []
    for k, ((key, make), img, info) in enumerate(zip(makes, images, infos)):
        want = ft.window_stored(_ref_render(ref, key, make))
        assert info["status"] == 0 and info["format"] == G.GL_RGBA8 and info["rects"] == [(0, 0, want.shape[1], want.shape[0])]
        if delta:
            assert info["keyframe"] == (1 if k == 0 else 0) and info["blocks_total"] == 64
            assert info["bytes"] == fg.HEADER + info["blocks"] * fg.entry_bytes(4)
            if k > 0:
                prev = ft.window_stored(_ref_render(ref, makes[k - 1][0], makes[k - 1][1]))
                assert info["blocks"] == len(fg.changed_blocks(prev, want)), (k, info)
        if not np.array_equal(img, want):
            bad.append((k, key))
    assert not bad, f"{name}: frames whose grab is not the oracle's render: {bad}"
    assert np.array_equal(px, _ref_render(ref, makes[-1][0], makes[-1][1]))


# ---------------------------------------------------------------------------- 4. delta grabs

def _one_block_change(a, block):
    """A copy of `a` with a few bytes inside `block` changed"""
    x, y, w, h = block
    b = a.copy()
    b[y + h - 1, x + w - 1] = b[y + h - 1, x + w - 1] ^ 0x40
    b[y, x] = b[y, x] ^ 1
    return b


def _delta_steps(s, t, a, window):
    """The delta sequence of one texture `t` (a device.Texture) whose stored bytes are `a`"""
    gl = s.gl
    h, w = a.shape[:2]
    fmt = G.GL_RGBA8 if a.ndim == 3 else G.GL_R8
    blocks = fg.blocks_of(w, h)
    host = np.zeros_like(a)
    grab = lambda flags=DELTA, rect=None: gl.grab_texture(t.id, rect, flags)
    # A: a keyframe; A again: nothing
    fg.check_delta(gl, grab(), host, a, blocks, keyframe=True)
    info = fg.check_delta(gl, grab(), host, a, [], keyframe=False)
    assert info["bytes"] <= fg.HEADER and tuple(info["damage"]) == (0, 0, 0, 0)
    # B: one change confined to one block (the last but one where there is one: an edge block)
    one = blocks[-2] if len(blocks) > 1 else blocks[0]
    b = _one_block_change(a, one)
    s.upload(t, one[0], one[1], ft.crop(b, one))
    info = fg.check_delta(gl, grab(), host, b, [one], keyframe=False)
    assert info["blocks"] == 1 and tuple(info["damage"]) == one
    # C: pixels of block (0, 0) and of the last edge block
    c = b.copy()
    c[0, 0] = c[0, 0] ^ 0x80
    c[h - 1, w - 1] = c[h - 1, w - 1] ^ 0x02
    c[min(h - 1, 63), min(w - 1, 63)] = c[min(h - 1, 63), min(w - 1, 63)] ^ 0x10
    s.upload(t, 0, 0, c)
    sent = fg.changed_blocks(b, c)
    assert sent == {blocks[0], blocks[-1]}
    fg.check_delta(gl, grab(), host, c, sent, keyframe=False)
    # WRHIP_GRAB_KEY: a keyframe again, into a fresh image
    host = np.zeros_like(a)
    fg.check_delta(gl, grab(DELTA | KEY), host, c, blocks, keyframe=True)
    fg.check_delta(gl, grab(), host, c, [], keyframe=False)
    # another rect: a keyframe; the same rect again: nothing; the whole texture again: a keyframe
    if w > 8 and h > 8:
        rect = (3, 2, w - 5, h - 3)
        part = np.zeros_like(ft.crop(c, rect))
        fg.check_delta(gl, grab(rect=rect), part, np.ascontiguousarray(ft.crop(c, rect)), fg.blocks_of(rect[2], rect[3]), keyframe=True)
        fg.check_delta(gl, grab(rect=rect), part, np.ascontiguousarray(ft.crop(c, rect)), [], keyframe=False)
        fg.check_delta(gl, grab(), host, c, blocks, keyframe=True)
    # new storage of another size: a keyframe
    nw, nh = w + 3, h + 1
    n = fg.noise(nh, nw, fmt, 900 + w)
    if window:
        s.d.init_default_framebuffer(nw, nh)
        t = device.Texture(gl.WrhipGetFramebufferTexture(0), nw, nh, fmt)
    else:
        gl.ActiveTexture(G.GL_TEXTURE0)
        gl.BindTexture(G.GL_TEXTURE_2D, t.id)
        gl.TexStorage2D(G.GL_TEXTURE_2D, 1, fmt, nw, nh)
        t = device.Texture(t.id, nw, nh, fmt)
    s.upload(t, 0, 0, n)
    host = np.zeros_like(n)
    fg.check_delta(gl, gl.grab_texture(t.id, None, DELTA), host, n, fg.blocks_of(nw, nh), keyframe=True)
    fg.check_delta(gl, gl.grab_texture(t.id, None, DELTA), host, n, [], keyframe=False)
    assert gl.GetError() == 0


def _delta_grabs(lib):
    # windows of 130 x 67 (3 x 2 blocks, a 2-pixel-wide and a 3-row-high edge block, rows of 520 bytes) and 333 x 201
    for (w, h) in ((130, 67), (333, 201)):
        s = fg.Session(lib, w, h)
        a = fg.noise(h, w, G.GL_RGBA8, w)
        win = device.Texture(s.window, w, h, G.GL_RGBA8)
        s.upload(win, 0, 0, a)
        _delta_steps(s, win, a, window=True)
        s.close()
    # R8: smaller than one block, and 513 x 513 (rows of 516 bytes, 81 blocks)
    s = fg.Session(lib, 64, 64)
    for (w, h) in ((61, 37), (513, 513)):
        a = fg.noise(h, w, G.GL_R8, w)
        _delta_steps(s, s.make(a, G.GL_R8), a, window=False)
    s.close()


# ---------------------------------------------------------------------------- 5. lifetime and tickets

def _lifetime_and_tickets(lib, ref):
    f1, f2 = _frame(), scenes.cfg2_overlapping_rects(n=150, seed=45, encoding="brush", width=W, height=H)
    want1 = ft.window_stored(_ref_render(ref, "cfg2", _frame))
    # the window is grabbed, then cleared and drawn again with no Finish in between
    s = fg.Session(lib, W, H)
    s.r.render(f1)
    t = s.gl.grab_texture(s.window)
    early = s.gl.grab_result(t, wait=False)          # (never KeyError: None, or the result)
    s.r.render(f2)
    s.r.finish()
    info, px = s.gl.grab_result(t)
    assert early is None or (early[0] == info and np.array_equal(early[1], px))
    assert np.array_equal(px, want1)
    info2, px2 = s.gl.grab_result(t)                 # a result fetched twice is identical
    assert info2 == info and np.array_equal(px2, px)
    # a picture tile is grabbed behind the held-back launches that draw it, then deleted
    f1.readback = [tile_size_cases.picture_tiles(f1)[0].texture]
    name = f1.readback[0].name
    want_tile = _ref_render(ref, "cfg2_tile", lambda: f1)[name]
    s.r.render(f1)
    tile = s.r.textures.pop(name)
    t = s.gl.grab_texture(tile.id)
    s.d.delete_texture(tile)
    s.r.finish()
    assert np.array_equal(s.gl.grab_result(t)[1], want_tile)
    # a delta grab parked behind the tail, then a TexSubImage2D into the texture: the grab delivers what was there before the
    # write, and the next one sends exactly the written blocks
    s.r.render(f1)
    host = np.zeros_like(want1)
    win = device.Texture(s.window, W, H, G.GL_RGBA8)
    t = s.gl.grab_texture(s.window, None, DELTA)
    patch = fg.noise(70, 40, G.GL_RGBA8, 77)
    s.upload(win, 100, 60, patch)                    # x 100..139, y 60..129: blocks (1..2, 0..2)
    t2 = s.gl.grab_texture(s.window, None, DELTA)
    fg.check_delta(s.gl, t, host, want1, fg.blocks_of(W, H), keyframe=True)
    want2 = want1.copy()
    want2[60:130, 100:140] = patch
    sent = fg.changed_blocks(want1, want2)
    assert len(sent) == 6
    fg.check_delta(s.gl, t2, host, want2, sent, keyframe=False)
    s.r.finish()
    assert s.gl.GetError() == 0
    s.close()

    # a texture is grabbed and deleted on an idle context, its storage taken over by another upload before the result is
    # fetched; a ticket polled at once; more grabs than the ring holds
    s = fg.Session(lib, 64, 64)
    s.r.finish()
    px = fg.noise(37, 61, G.GL_RGBA8, 11)
    tex = s.make(px, G.GL_RGBA8)
    t = s.gl.grab_texture(tex.id)
    polled = s.gl.grab_result(t, wait=False)
    s.d.delete_texture(tex)
    other = s.make(fg.noise(37, 61, G.GL_RGBA8, 12), G.GL_RGBA8)      # (takes the freed storage over)
    s.r.finish()
    info, got = s.gl.grab_result(t)
    assert polled is None or (polled[0] == info and np.array_equal(polled[1], got))
    assert np.array_equal(got, px)
    out = glapi.WrhipGrabInfo()
    assert s.gl.WrhipGrabResultGet(t, C.byref(out), None, 0, 0) == 0 and s.gl.WrhipGrabResultGet(t, C.byref(out), None, 0, 1) == 0
    assert s.gl.WrhipGrabResultGet(-5, C.byref(out), None, 0, 1) == -1 and s.gl.WrhipGrabResultGet(-5, C.byref(out), None, 0, 0) == -1
    assert s.gl.WrhipGrabResultGet(t + 1, C.byref(out), None, 0, 1) == -1         # (never handed out)
    srcs = [fg.noise(5 + k, 9 + 16 * k, G.GL_R8, 100 + k) for k in range(4)]
    texs = [s.make(p, G.GL_R8) for p in srcs]
    n = 8 + 3
    tickets = [s.gl.grab_texture(texs[k % 4].id) for k in range(n)]
    assert len(set(tickets)) == n and min(tickets) >= 0
    for k in range(3, n):
        s.gl.grab_result(tickets[k], wait=False)      # (polling a live ticket never raises)
    for k in range(3):
        assert s.gl.WrhipGrabResultGet(tickets[k], C.byref(out), None, 0, 1) == -1
        with pytest.raises(KeyError):
            s.gl.grab_result(tickets[k])
    for k in range(3, n):
        assert np.array_equal(s.gl.grab_result(tickets[k])[1], srcs[k % 4]), k
    s.d.delete_texture(other)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 6. budget (CPU only)

def test_grab_kernels_have_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    for name in ("wr_grab_pack_kernel", "wr_grab_push_kernel"):      # (the pack kernel is one kernel for both modes)
        assert name in notes, sorted(notes)
        vgprs, scratch = notes[name]
        assert scratch == 0, (name, vgprs, scratch)


# ---------------------------------------------------------------------------- CPU: the host simulation

def test_hostsim_full_grabs_are_the_stored_bytes(hostsim, oracle_gcc):
    _full_grabs(hostsim, oracle_gcc)


def test_hostsim_one_launch_nothing_drained(hostsim, oracle_gcc):
    _one_launch(hostsim)


@pytest.mark.parametrize("name,seq", SEQUENCES + [("rects", None)], ids=[n for n, _ in SEQUENCES] + ["rects"])
def test_hostsim_every_frame_of_a_stream(hostsim, oracle_gcc, name, seq):
    _stream(hostsim, oracle_gcc, name, seq, on_gpu=False)


def test_hostsim_delta_grabs(hostsim, oracle_gcc):
    _delta_grabs(hostsim)


@pytest.mark.parametrize("name,seq", [SEQUENCES[0], ("rects", None)], ids=[SEQUENCES[0][0], "rects"])
def test_hostsim_delta_stream(hostsim, oracle_gcc, name, seq):
    _stream(hostsim, oracle_gcc, name, seq, on_gpu=False, delta=True)


def test_hostsim_lifetime_and_tickets(hostsim, oracle_gcc):
    _lifetime_and_tickets(hostsim, oracle_gcc)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
def test_gpu_full_grabs_are_the_stored_bytes():
    _full_grabs(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_one_launch_nothing_drained():
    _gpu_ref()
    _one_launch(wrhip_lib())


@pytest.mark.gpu
@pytest.mark.parametrize("name,seq", SEQUENCES + [("rects", None)], ids=[n for n, _ in SEQUENCES] + ["rects"])
def test_gpu_every_frame_of_a_stream(name, seq):
    _stream(wrhip_lib(), _gpu_ref(), name, seq, on_gpu=True)


@pytest.mark.gpu
def test_gpu_delta_grabs():
    _gpu_ref()
    _delta_grabs(wrhip_lib())


@pytest.mark.gpu
@pytest.mark.parametrize("name,seq", [SEQUENCES[0], ("rects", None)], ids=[SEQUENCES[0][0], "rects"])
def test_gpu_delta_stream(name, seq):
    _stream(wrhip_lib(), _gpu_ref(), name, seq, on_gpu=True, delta=True)


@pytest.mark.gpu
def test_gpu_lifetime_and_tickets():
    _lifetime_and_tickets(wrhip_lib(), _gpu_ref())
