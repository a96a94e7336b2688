"""Scaled grabs (include/wrhip.h: WrhipGrabTextureScaled): a texture rect scaled down as the reference's screenshot grabber scales
it -- a GL_LINEAR blit to level L, then L exact 2:1 blits -- in one pass on the device, delivered through the grab ring.  The
expected bytes always come from the ORACLE running that chain of BlitFramebuffer calls (tests/grab_scaled.py: blit_chain), and 0
bytes may differ.  Each check runs on the host simulation and, under -m gpu, on the MI355X."""
import ctypes as C
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
import frame_grabs as fg
import grab_scaled as gsc
from webrender_amd import scenes, glapi, glconst as G, device
from webrender_amd.renderer import Renderer
from webrender_amd.harness import render_streamed_grabbed, screenshot_size

W = H = 512
TW, TH = 333, 201
FLIP, SWAP, SCALED = glapi.GRAB_FLIP_ROWS, glapi.GRAB_SWAP_RB, glapi.GRAB_SCALED
# name: (rect, size, L)
CASES = {
    "L0_general": ((0, 0, 333, 201), (200, 121), 0),          # a single general-ratio tap
    "L0_tall": ((0, 0, 100, 90), (50, 20), 0),                # height ratio above 2: rows skipped by the top step
    "L0_equal": ((3, 5, 61, 37), (61, 37), 0),                # a nearest copy: equals a full grab
    "L0_one_axis": ((3, 5, 61, 37), (61, 20), 0),             # one axis equal: still linear
    "L1": ((1, 2, 331, 199), (100, 60), 1),                   # rect off origin: edge taps read texels outside the rect
    "L2": ((0, 0, 333, 201), (60, 36), 2),
    "L3": ((0, 0, 333, 201), (37, 21), 3),                    # top level 296 x 168: tiles cut on both axes, rows of 148 bytes
    "L4": ((0, 0, 330, 170), (20, 10), 4),                    # the second launch, through scratch
    "L8": ((0, 0, 333, 201), (1, 1), 8),                      # three launches
    "edge": ((233, 101, 100, 100), (30, 30), 1),              # the texture's last column and row
    "edge_thin": ((328, 0, 5, 201), (2, 80), 1),              # a rect 5 pixels wide
}
STREAM_SEEDS = (40, 71, 72, 73, 74, 75, 76, 77, 78, 79)


def _noise():
    return fg.noise(TH, TW, G.GL_RGBA8, 3331)


def _frame(seed=44, n=200):
    return scenes.cfg2_overlapping_rects(n=n, seed=seed, encoding="brush", width=W, height=H)


_want = {}


def _oracle_noise(ref):
    """The oracle's chain for every case on the noise texture: computed once per session, never modified"""
    if (ref, "noise") not in _want:
        gl = glapi.GL(ref)
        r = Renderer(gl, 64, 64)
        d = r.device
        tex = d.create_texture(TW, TH, G.GL_RGBA8, render_target=True)
        d.upload_texture(tex, 0, 0, TW, TH, G.GL_BGRA, G.GL_UNSIGNED_BYTE, _noise())
        _want[(ref, "noise")] = {name: gsc.blit_chain(gl, d, tex, rect, size) for name, (rect, size, _) in CASES.items()}
        r.destroy()
    return _want[(ref, "noise")]


def _oracle_frames(ref):
    """The oracle's chain 512 x 512 -> 64 x 64 on its own render of the cfg2 frame and of every frame of the stream"""
    if (ref, "frames") not in _want:
        gl = glapi.GL(ref)
        r = Renderer(gl, W, H)
        window = device.Texture(0, W, H, G.GL_RGBA8, fbo=0)
        out = {}
        for key, frame in [("cfg2", _frame())] + [(sd, _frame(sd, 60)) for sd in STREAM_SEEDS]:
            r.render(frame)
            r.finish()
            out[key] = gsc.blit_chain(gl, r.device, window, (0, 0, W, H), (64, 64))
        r.destroy()
        _want[(ref, "frames")] = out
    return _want[(ref, "frames")]


def _grab(gl, tex, rect, size, flags=0):
    t = gl.grab_texture_scaled(tex, rect, size, flags)
    assert t >= 0, (t, gl.GetError())
    return t


# ---------------------------------------------------------------------------- 1. every case against the oracle's chain

def _case(lib, ref, name):
    rect, size, L = CASES[name]
    want = _oracle_noise(ref)[name]
    assert want.shape == (size[1], size[0], 4) and gsc.levels_of(rect[2], size[0]) == L
    s = fg.Session(lib, 64, 64)
    px = _noise()
    tex = s.make(px, G.GL_RGBA8)
    s.r.finish()
    a = s.stats()
    t = _grab(s.gl, tex.id, rect, size)
    b = s.stats()
    assert b["kernel_launches"] == a["kernel_launches"] + 1 + L // 4 and b["flushes"] == a["flushes"]
    info, got = s.gl.grab_result(t)
    assert (info["status"], info["format"], info["flags"], info["rects"]) == (0, G.GL_RGBA8, SCALED, [rect]), info
    assert (info["scaled_w"], info["scaled_h"], info["levels"]) == (size[0], size[1], L), info
    assert info["bytes"] == fg.HEADER + size[0] * size[1] * 4
    assert got.shape == want.shape
    assert int((got != want).sum()) == 0, f"{name}: {int((got != want).sum())} bytes differ from the oracle's chain"
    if name == "L0_equal":
        assert np.array_equal(got, s.gl.grab_result(s.gl.grab_texture(tex.id, rect))[1]) and np.array_equal(got, fg.crop(px, rect))
    c = s.stats()
    assert c["d2h_bytes"] == a["d2h_bytes"] + info["bytes"] + (info["bytes"] if name == "L0_equal" else 0)
    # the bytes that crossed: the header (word 0: the payload's bytes), then the same pixels
    raw = s.gl.grab_payload(t)
    assert len(raw) == info["bytes"] and int.from_bytes(raw[:4], "little") == want.size
    assert np.array_equal(np.frombuffer(raw[fg.HEADER:], np.uint8).reshape(want.shape), want)
    assert s.gl.GetError() == 0
    s.close()


def _blit_path_agrees(lib, ref):
    """libwrhip's own BlitFramebuffer chain (wr_blit_kernel) gives the oracle's bytes too: new kernel, old kernel and swgl are one"""
    s = fg.Session(lib, 64, 64)
    tex = s.make(_noise(), G.GL_RGBA8)
    for name, (rect, size, _) in CASES.items():
        got = gsc.blit_chain(s.gl, s.d, tex, rect, size)
        assert np.array_equal(got, _oracle_noise(ref)[name]), name
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 2. flags and strided delivery

def _flags_and_stride(lib, ref):
    rect, size, _ = CASES["L3"]
    want = _oracle_noise(ref)["L3"]
    s = fg.Session(lib, 64, 64)
    tex = s.make(_noise(), G.GL_RGBA8)
    tickets = [(_grab(s.gl, tex.id, rect, size, f), f) for f in (FLIP, SWAP, FLIP | SWAP)]
    for t, f in tickets:
        info, got = s.gl.grab_result(t)
        assert info["flags"] == (f | SCALED)
        assert np.array_equal(got, fg.flagged(want, f)), f
        assert not np.array_equal(got, want)
    t = _grab(s.gl, tex.id, rect, size)
    tight = size[0] * 4
    buf = np.full((size[1], tight + 12), 0xA5, np.uint8)
    info = glapi.WrhipGrabInfo()
    assert s.gl.WrhipGrabResultGet(t, C.byref(info), buf.ctypes.data, tight + 12, 1) == 0
    assert np.array_equal(buf[:, :tight].reshape(want.shape), want) and (buf[:, tight:] == 0xA5).all()
    assert s.gl.GetError() == 0
    assert s.gl.WrhipGrabResultGet(t, C.byref(info), buf.ctypes.data, tight - 4, 1) == -1
    assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 3. stream order

def _rendered_frame(lib, ref):
    """The window behind its held-back launches, no Finish; then a write to it that the result does not see"""
    want = _oracle_frames(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    s.r.render(_frame())
    t = _grab(s.gl, s.window, None, (64, 64))
    s.upload(device.Texture(s.window, W, H, G.GL_RGBA8), 100, 60, fg.noise(70, 40, G.GL_RGBA8, 77))
    info, got = s.gl.grab_result(t)
    assert info["levels"] == 2 and info["rects"] == [(0, 0, W, H)]
    assert int((got != want).sum()) == 0
    s.r.finish()
    assert s.gl.GetError() == 0
    s.close()


def _stream(lib, ref):
    frames = [_frame(sd, 60) for sd in STREAM_SEEDS]
    px, st, images, infos = render_streamed_grabbed(lib, frames, scale_to=(64, 64))
    assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
    assert st["setup_carried"] >= len(frames) - 1, st          # (a grab that drained the held-back launches would lose these)
    assert len(images) == len(infos) == len(frames)
    want = _oracle_frames(ref)
    bad = [sd for sd, img in zip(STREAM_SEEDS, images) if img.shape != (64, 64, 4) or not np.array_equal(img, want[sd])]
    assert not bad, f"frames whose scaled grab is not the oracle's chain on its render: {bad}"
    assert len({want[sd].tobytes() for sd in STREAM_SEEDS}) == len(STREAM_SEEDS)      # (the frames differ)


def _lifetime_and_tickets(lib, ref):
    rect, size, _ = CASES["L4"]
    want = _oracle_noise(ref)["L4"]
    s = fg.Session(lib, 64, 64)
    s.r.finish()
    tex = s.make(_noise(), G.GL_RGBA8)
    # a write to the texture after the grab call does not change the result
    t = _grab(s.gl, tex.id, rect, size)
    s.upload(tex, 0, 0, fg.noise(TH, TW, G.GL_RGBA8, 12))
    s.r.finish()
    assert np.array_equal(s.gl.grab_result(t)[1], want)
    # nine scaled grabs without a fetch: the ring holds the 8 newest
    s.upload(tex, 0, 0, _noise())
    tickets = [_grab(s.gl, tex.id, *CASES[name][:2]) for name in ("L3", "L4", "L8", "L1", "L2", "edge", "L0_tall", "L3", "L4")]
    assert len(set(tickets)) == 9
    out = glapi.WrhipGrabInfo()
    assert s.gl.WrhipGrabResultGet(tickets[0], C.byref(out), None, 0, 1) == -1
    with pytest.raises(KeyError):
        s.gl.grab_result(tickets[0])
    for t, name in zip(tickets[1:], ("L4", "L8", "L1", "L2", "edge", "L0_tall", "L3", "L4")):
        assert np.array_equal(s.gl.grab_result(t)[1], _oracle_noise(ref)[name]), name
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 4. the contract's rejections

def _contract(lib):
    s = fg.Session(lib, W, H)
    s.r.render(_frame())
    s.r.finish()
    r8 = s.make(fg.noise(37, 61, G.GL_R8, 3), G.GL_R8)
    s.r.finish()
    assert s.gl.GetError() == 0
    n0 = s.stats()["kernel_launches"]
    f0 = s.stats()["flushes"]
    full = (0, 0, W, H)
    bad = [
        lambda: s.gl.grab_texture_scaled(9999, (0, 0, 4, 4), (2, 2)),             # unknown texture
        lambda: s.gl.grab_texture_scaled(r8.id, (0, 0, 4, 4), (2, 2)),            # not GL_RGBA8
        lambda: s.gl.grab_texture_scaled(s.window, (0, 0, 0, 4), (1, 1)),         # empty
        lambda: s.gl.grab_texture_scaled(s.window, (0, 0, 4, 0), (1, 1)),
        lambda: s.gl.grab_texture_scaled(s.window, (500, 0, 13, 1), (1, 1)),      # outside the texture
        lambda: s.gl.grab_texture_scaled(s.window, (0, -1, 4, 4), (2, 2)),
        lambda: s.gl.grab_texture_scaled(s.window, full, (0, 64)),                # size below 1
        lambda: s.gl.grab_texture_scaled(s.window, full, (64, 0)),
        lambda: s.gl.grab_texture_scaled(s.window, full, (W + 1, 64)),            # size above the rect's
        lambda: s.gl.grab_texture_scaled(s.window, full, (64, H + 1)),
        lambda: s.gl.grab_texture_scaled(s.window, full, (1, H)),                 # L = 8: level 8 would be 256 x 131072
        lambda: s.gl.grab_texture_scaled(s.window, full, (64, 64), glapi.GRAB_DELTA),
        lambda: s.gl.grab_texture_scaled(s.window, full, (64, 64), 16),
        lambda: s.gl.grab_texture_scaled(s.window, full, (64, 64), SCALED),
        lambda: s.gl.grab_texture(s.window, [(0, 0, 4, 4)], SCALED),              # WrhipGrabTexture keeps rejecting 64
    ]
    for k, call in enumerate(bad):
        assert call() == -1, k
        assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0, k
    s.gl.WrhipSetShard(0, 2)
    assert s.gl.grab_texture_scaled(s.window, full, (64, 64)) == -1
    assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0
    s.gl.WrhipSetShard(0, 1)
    s.gl.WrhipSetTargetRows(s.window, 0, 256)
    assert s.gl.grab_texture_scaled(s.window, full, (64, 64)) == -1
    assert s.gl.GetError() == G.GL_INVALID_VALUE and s.gl.GetError() == 0
    s.gl.WrhipSetTargetRows(s.window, 0, 0)
    assert s.stats()["kernel_launches"] == n0 and s.stats()["flushes"] == f0
    assert s.gl.grab_texture_scaled(s.window, full, (64, 64)) >= 0 and s.stats()["kernel_launches"] == n0 + 1
    # the three new fields are 0 for any other grab
    info, _ = s.gl.grab_result(s.gl.grab_texture(s.window, (0, 0, 4, 4)))
    assert (info["scaled_w"], info["scaled_h"], info["levels"], info["flags"]) == (0, 0, 0, 0)
    s.close()


# ---------------------------------------------------------------------------- 5. CPU only: the size rule, the kernel's budget

def test_screenshot_size():
    # scale = min(bw / w, bh / h) in f32; each dimension times it, rounded half away from zero (screen_capture.rs:121-124)
    assert screenshot_size((3840, 2160), (350, 350)) == (350, 197)        # 2160 * 0.091145836 = 196.875
    assert screenshot_size((1920, 1080), (350, 350)) == (350, 197)
    assert screenshot_size((1000, 2000), (350, 350)) == (175, 350)
    assert screenshot_size((512, 512), (64, 64)) == (64, 64)
    assert screenshot_size((100, 100), (350, 350)) == (350, 350)          # (the rule itself scales up too)
    assert screenshot_size((4, 3), (2, 2)) == (2, 2)                      # a tie: 3 * 0.5 = 1.5 rounds away from zero
    assert screenshot_size((8, 5), (4, 4)) == (4, 3)                      # 2.5 -> 3
    assert screenshot_size((8, 1), (4, 4)) == (4, 1)                      # 0.5 -> 1


def test_grab_scale_kernel_has_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    assert "wr_grab_scale_kernel" in notes, sorted(notes)
    vgprs, scratch = notes["wr_grab_scale_kernel"]
    assert scratch == 0, (vgprs, scratch)


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name", list(CASES))
def test_hostsim_case(hostsim, oracle_gcc, name):
    _case(hostsim, oracle_gcc, name)


def test_hostsim_blit_path_agrees(hostsim, oracle_gcc):
    _blit_path_agrees(hostsim, oracle_gcc)


def test_hostsim_flags_and_stride(hostsim, oracle_gcc):
    _flags_and_stride(hostsim, oracle_gcc)


def test_hostsim_rendered_frame(hostsim, oracle_gcc):
    _rendered_frame(hostsim, oracle_gcc)


def test_hostsim_stream(hostsim, oracle_gcc):
    _stream(hostsim, oracle_gcc)


def test_hostsim_lifetime_and_tickets(hostsim, oracle_gcc):
    _lifetime_and_tickets(hostsim, oracle_gcc)


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
def test_gpu_blit_path_agrees():
    _blit_path_agrees(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_flags_and_stride():
    _flags_and_stride(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_rendered_frame():
    _rendered_frame(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_stream():
    _stream(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_lifetime_and_tickets():
    _lifetime_and_tickets(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_contract():
    _gpu_ref()
    _contract(wrhip_lib())
