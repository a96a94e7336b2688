"""Tensor grabs (include/wrhip.h: WrhipGrabTextureTensor): a texture rect -- as stored, or scaled down by the scaled grab's chain --
converted on the device into a normalised CHW / HWC tensor of U8, F16, BF16 or F32 elements in the caller's device memory; only a
16-byte ticket crosses to the host.  Expected tensors are computed in numpy (tests/grab_tensor.py) from the ORACLE's bytes -- its
upload or render read back, or its chain of BlitFramebuffer calls (tests/grab_scaled.py) -- and are compared as raw bits: 0
differing elements, no tolerance anywhere.  Destinations are filled with a guard byte first and read back whole, so every byte
outside the contract's elements is checked too.  Each check runs on the host simulation and, under -m gpu, on the MI355X."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from conftest import ROOT, wrhip_lib, oracle_ref
import frame_grabs as fg
import grab_tensor as gt
from grab_tensor import U8, F16, BF16, F32, CHW, HWC, BGR, FLIP
from test_grab_scaled import CASES, STREAM_SEEDS, W, H, _noise, _frame, _oracle_noise, _oracle_frames
from webrender_amd import glapi, glconst as G, device
from webrender_amd.renderer import Renderer
from webrender_amd.harness import render_streamed_tensors

RECTS = {
    "full": (0, 0, 333, 201),
    "inner": (3, 5, 61, 37),
    "corner": (233, 101, 100, 100),          # the texture's last column and row
    "thin": (328, 0, 5, 201),                # narrower than any group
    "short": (1, 2, 64, 3),
}
R8W, R8H = 61, 37                            # R8 rows of 61 bytes: odd
SCALED_NAMES = ("L0_general", "L1", "L3", "L4", "L8", "edge_thin")
DTYPES, LAYOUTS = (U8, F16, BF16, F32), (CHW, HWC)

_want = {}


def _r8_noise():
    return fg.noise(R8H, R8W, G.GL_R8, 611)


def _oracle_stored(ref):
    """The oracle's own stored bytes: the two noise textures uploaded and read back, its render of the cfg2 frame"""
    if ref not in _want:
        gl = glapi.GL(ref)
        r = Renderer(gl, W, H)
        d = r.device
        out = {}
        for key, px, fmt, up in (("rgba", _noise(), G.GL_RGBA8, G.GL_BGRA), ("r8", _r8_noise(), G.GL_R8, G.GL_RED)):
            tex = d.create_texture(px.shape[1], px.shape[0], fmt, render_target=True)
            d.upload_texture(tex, 0, 0, px.shape[1], px.shape[0], up, G.GL_UNSIGNED_BYTE, px)
            out[key] = d.read_texture(tex).copy()
            assert np.array_equal(out[key], px)
        r.render(_frame())
        r.finish()
        out["cfg2"] = d.read_texture(device.Texture(0, W, H, G.GL_RGBA8, fbo=0)).copy()
        r.destroy()
        _want[ref] = out
    return _want[ref]


def _one(s, tex, fmt, rect, px, dtype, layout, channels, flags=0, size=None, scaled=None, launches=1, scale=gt.SCALE, bias=gt.BIAS,
         off=0, row=0, plane=0, what=""):
    """One grab on a quiescent session into a guarded destination, checked whole: `px` are the stored bytes the contract names"""
    h, w = px.shape[:2]
    d = gt.Dest(s.gl, gt.shape_of(w, h, layout, channels), dtype, layout, off, row, plane)
    a = s.stats()
    t = gt.grab(s, tex, rect, d, size=size, scale=scale, bias=bias, flags=flags)
    b = s.stats()
    assert b["kernel_launches"] == a["kernel_launches"] + launches and b["flushes"] == a["flushes"], (what, a, b)
    info, pixels = s.gl.grab_result(t)
    assert pixels is None
    gt.check_info(info, rect, flags, fmt, scaled)
    d.check(gt.expected(px, dtype, layout, channels, scale, bias, flags), what)
    assert s.stats()["d2h_bytes"] >= b["d2h_bytes"] + glapi.GRAB_HEADER
    d.free()


def _noise_session(lib):
    s = fg.Session(lib, 64, 64)
    tex = s.make(_noise(), G.GL_RGBA8)
    s.r.finish()
    return s, tex


# ---------------------------------------------------------------------------- 1. the unscaled matrix

def _matrix(lib, ref, name):
    rect = RECTS[name]
    px = fg.crop(_oracle_stored(ref)["rgba"], rect)
    s, tex = _noise_session(lib)
    for dtype in DTYPES:
        for layout in LAYOUTS:
            for channels in (3, 4):
                for flags in (0, BGR, FLIP, BGR | FLIP):
                    _one(s, tex.id, G.GL_RGBA8, rect, px, dtype, layout, channels, flags, what=f"{name} {dtype} {layout} {channels} {flags}")
    assert s.gl.GetError() == 0
    s.close()


def _f16_edges(lib, ref):
    """scale 2^-20: bytes under 64 give f16 subnormals; scale 300: 255 * 300 > 65504 overflows to infinity"""
    rect = RECTS["full"]
    px = fg.crop(_oracle_stored(ref)["rgba"], rect)
    s, tex = _noise_session(lib)
    zero = np.zeros(4, np.float32)
    for scale, mask, hit in ((2.0 ** -20, 0x7C00, 0x0000), (300.0, 0x7FFF, 0x7C00)):
        sc = np.full(4, scale, np.float32)
        want = gt.expected(px, F16, CHW, 3, sc, zero)
        assert ((want & mask) == hit).any() and (want != 0).any()          # (subnormals: exponent 0; infinities: 0x7C00)
        if hit == 0:
            assert (((want & 0x7C00) == 0) & ((want & 0x3FF) != 0)).any()
        _one(s, tex.id, G.GL_RGBA8, rect, px, F16, CHW, 3, scale=sc, bias=zero, what=f"scale {scale}")
        _one(s, tex.id, G.GL_RGBA8, rect, px, F16, HWC, 4, flags=FLIP, scale=sc, bias=zero, what=f"scale {scale}")
    s.close()


# ---------------------------------------------------------------------------- 2. alignment and guard bytes

def _alignment(lib, ref):
    s, tex = _noise_session(lib)
    stored = _oracle_stored(ref)["rgba"]
    for name in ("inner", "short", "thin"):
        rect = RECTS[name]
        px = fg.crop(stored, rect)
        h, w = px.shape[:2]
        for dtype in DTYPES:
            per16 = 16 // gt.ELEM[dtype]
            for layout, c in ((CHW, 3), (HWC, 3), (HWC, 4)):
                tight = w if layout == CHW else w * c
                odd = w + 3 if layout == CHW else w * c + 1
                wide = (tight + per16 - 1) // per16 * per16 + per16           # rows that stay 16-byte aligned, with padding behind them
                geoms = [dict(), dict(off=1), dict(row=odd), dict(off=1, row=odd), dict(row=wide)]
                if layout == CHW:
                    geoms += [dict(plane=h * w + 5), dict(row=odd, plane=h * odd + 5), dict(off=1, row=odd, plane=(h - 1) * odd + w),
                              dict(row=wide, plane=h * wide + per16), dict(row=wide, plane=h * wide + 5)]
                for g in geoms:
                    _one(s, tex.id, G.GL_RGBA8, rect, px, dtype, layout, c, what=f"{name} {dtype} {layout} {c} {g}", **g)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 3. R8

def _r8(lib, ref):
    stored = _oracle_stored(ref)["r8"]
    s = fg.Session(lib, 64, 64)
    tex = s.make(_r8_noise(), G.GL_R8)
    s.r.finish()
    for rect in ((0, 0, R8W, R8H), (7, 3, 50, 30)):
        px = fg.crop(stored, rect)
        for dtype in DTYPES:
            for layout in LAYOUTS:
                for flags in (0, FLIP):
                    _one(s, tex.id, G.GL_R8, rect, px, dtype, layout, 1, flags, what=f"r8 {rect} {dtype} {layout} {flags}")
        _one(s, tex.id, G.GL_R8, rect, px, F32, CHW, 1, off=1, row=rect[2] + 3, what="r8 strided")
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 4. scaled

def _scaled(lib, ref, name):
    rect, size, L = CASES[name]
    px = _oracle_noise(ref)[name]                       # the oracle's chain: (size[1], size[0], 4) stored bytes
    assert px.shape == (size[1], size[0], 4)
    s, tex = _noise_session(lib)
    kw = dict(size=size, scaled=(size[0], size[1], L), launches=1 + L // 4)
    _one(s, tex.id, G.GL_RGBA8, rect, px, F32, CHW, 3, what=f"{name} f32", **kw)
    _one(s, tex.id, G.GL_RGBA8, rect, px, BF16, HWC, 4, what=f"{name} bf16", **kw)
    _one(s, tex.id, G.GL_RGBA8, rect, px, F16, CHW, 4, FLIP | BGR, what=f"{name} f16 flipped", **kw)
    _one(s, tex.id, G.GL_RGBA8, rect, px, U8, CHW, 3, off=1, row=size[0] + 3, what=f"{name} u8 strided", **kw)
    # U8 / HWC / 4 / BGR is the scaled grab's payload, byte for byte
    d = gt.Dest(s.gl, (size[1], size[0], 4), U8, HWC)
    a = s.stats()
    t = gt.grab(s, tex.id, rect, d, size=size, flags=BGR)
    assert s.stats()["kernel_launches"] == a["kernel_launches"] + 1 + L // 4
    s.gl.grab_result(t)
    raw = s.gl.grab_payload(s.gl.grab_texture_scaled(tex.id, rect, size))
    assert len(raw) == fg.HEADER + size[0] * size[1] * 4
    got = d.read()
    assert got[:d.extent].tobytes() == raw[fg.HEADER:] and (got[d.extent:] == gt.GUARD).all()
    d.free()
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 5. stream order

def _rendered_frame(lib, ref):
    """The window behind its held-back launches, no Finish: the grab is parked; a later write to the window is not seen"""
    px = _oracle_frames(ref)["cfg2"]
    s = fg.Session(lib, W, H)
    s.r.render(_frame())
    d = gt.Dest(s.gl, (3, 64, 64), F32, CHW)
    t = gt.grab(s, s.window, (0, 0, W, H), d, size=(64, 64))
    assert s.gl.grab_result(t, wait=False) is None          # parked: it waits for the held-back launches, and does not make them
    s.upload(device.Texture(s.window, W, H, G.GL_RGBA8), 100, 60, fg.noise(70, 40, G.GL_RGBA8, 77))
    info, _ = s.gl.grab_result(t)
    gt.check_info(info, (0, 0, W, H), 0, G.GL_RGBA8, (64, 64, 2))
    d.check(gt.expected(px, F32, CHW, 3), "rendered frame")
    d.free()
    s.r.finish()
    assert s.gl.GetError() == 0
    s.close()


def _stream(lib, ref):
    frames = [_frame(sd, 60) for sd in STREAM_SEEDS]
    batch, st, infos = render_streamed_tensors(lib, frames, (64, 64), F16, CHW, 3, gt.SCALE, gt.BIAS)
    assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
    assert st["setup_carried"] >= len(frames) - 1, st          # (a grab that drained the held-back launches would lose these)
    assert batch.shape == (len(frames), 3, 64, 64) and batch.dtype == np.float16
    want = _oracle_frames(ref)
    bad = [sd for k, sd in enumerate(STREAM_SEEDS) if not np.array_equal(batch[k].view(np.uint16), gt.expected(want[sd], F16, CHW, 3))]
    assert not bad, f"slots that are not the oracle's chain on their frame's render: {bad}"
    assert len(infos) == len(frames) and infos[-1] is not None
    gt.check_info(infos[-1], (0, 0, W, H), 0, G.GL_RGBA8, (64, 64, 2))


# ---------------------------------------------------------------------------- 6. the ring: the write outlives the ticket

def _nine(s, px, parked):
    """Nine tensor grabs of the window into nine buffers without a fetch: the ring holds the 8 newest tickets, every buffer is written"""
    dests, tickets, wants = [], [], []
    for k in range(9):
        dtype, layout, c = DTYPES[k % 4], LAYOUTS[k % 2], 3 + k % 2
        if k % 3 == 2:
            rect, size, src = (0, 0, W, H), (64, 64), None
        else:
            rect = (7 * k, 11 * k, 100 + k, 20 + k)
            size, src = None, fg.crop(px["cfg2"], rect)
        src = px["chain"] if src is None else src
        d = gt.Dest(s.gl, gt.shape_of(src.shape[1], src.shape[0], layout, c), dtype, layout, off=k % 2)
        tickets.append(gt.grab(s, s.window, rect, d, size=size, flags=BGR if k % 4 == 3 else 0))
        dests.append(d)
        wants.append(gt.expected(src, dtype, layout, c, flags=BGR if k % 4 == 3 else 0))
    assert len(set(tickets)) == 9
    out = glapi.WrhipGrabInfo()
    if parked:
        assert all(s.gl.WrhipGrabResultGet(t, C.byref(out), None, 0, 0) == 1 for t in tickets[1:])
    assert s.gl.WrhipGrabResultGet(tickets[0], C.byref(out), None, 0, 1) == -1
    with pytest.raises(KeyError):
        s.gl.grab_result(tickets[0])
    if parked:
        gt.send_held(s.gl)                              # the held-back launches go out, the nine grabs behind them
    for t in tickets[1:]:
        assert s.gl.grab_result(t)[0]["flags"] & gt.TENSOR
    for k, (d, want) in enumerate(zip(dests, wants)):
        d.check(want, f"grab {k}")
        d.free()


def _ring(lib, ref):
    px = dict(_oracle_stored(ref), chain=_oracle_frames(ref)["cfg2"])
    s = fg.Session(lib, W, H)
    s.r.render(_frame())
    _nine(s, px, True)
    s.r.finish()
    _nine(s, px, False)
    assert s.gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 7. the contract's rejections, device memory

def _contract(lib):
    s = fg.Session(lib, W, H)
    gl = s.gl
    s.r.render(_frame())
    s.r.finish()
    r8 = s.make(_r8_noise(), G.GL_R8)
    f32 = s.d.create_texture(8, 8, G.GL_RGBA32F)
    s.r.finish()
    assert gl.GetError() == 0
    full, win = (0, 0, W, H), s.window
    buf = gl.device_alloc(1 << 20)
    n0, f0 = s.stats()["kernel_launches"], s.stats()["flushes"]

    def call(tex=win, rect=(0, 0, 64, 32), dst=buf, dst_bytes=1 << 20, **kw):
        return gl.grab_texture_tensor(tex, rect, dst, dst_bytes, **kw)
    rect4 = (C.c_int32 * 4)(0, 0, 64, 32)
    bad = [
        lambda: call(tex=9999),                                               # unknown texture
        lambda: call(tex=f32.id, rect=(0, 0, 8, 8)),                          # neither GL_RGBA8 nor GL_R8
        lambda: call(channels=1), lambda: call(channels=2), lambda: call(channels=5),      # channels against the format
        lambda: call(tex=r8.id, rect=(0, 0, 8, 8), channels=3),
        lambda: call(rect=(0, 0, 0, 4)), lambda: call(rect=(0, 0, 4, 0)),     # empty
        lambda: call(rect=(500, 0, 13, 1)), lambda: call(rect=(0, -1, 4, 4)),      # outside the texture
        lambda: call(rect=full, size=(0, 64)), lambda: call(rect=full, size=(64, 0)),      # size below 1
        lambda: call(rect=full, size=(W + 1, 64)), lambda: call(rect=full, size=(64, H + 1)),      # size above the rect's
        lambda: call(tex=r8.id, rect=(0, 0, 8, 8), size=(4, 4), channels=1),       # scaling an R8 texture
        lambda: call(rect=full, size=(1, H)),                                 # L = 8: level 8 would be 256 x 131072
        lambda: call(dtype=4), lambda: call(layout=2),
        lambda: call(flags=glapi.GRAB_SWAP_RB), lambda: call(flags=glapi.GRAB_DELTA), lambda: call(flags=gt.TENSOR), lambda: call(flags=512),
        lambda: gl.WrhipGrabTextureTensor(win, C.addressof(rect4), None),      # no desc
        lambda: call(dst=0),                                                  # no destination
        lambda: call(strides=(63, 0)), lambda: call(strides=(64, 31 * 64 + 63)), lambda: call(strides=(-64, 0)),      # strides below their minimum
        lambda: call(layout=HWC, strides=(64 * 3 - 1, 0)),
        lambda: call(dtype=F32, dst_bytes=3 * 32 * 64 * 4 - 1),               # the extent does not fit
        lambda: call(dtype=F32, strides=(100, 5000), dst_bytes=(2 * 5000 + 31 * 100 + 64) * 4 - 1),
        lambda: call(dtype=F16, dst=buf + 1),                                 # not aligned to its element
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
    # the other grab calls keep rejecting 128
    assert gl.grab_texture(win, [(0, 0, 4, 4)], gt.TENSOR) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert gl.grab_texture_scaled(win, full, (64, 64), gt.TENSOR) == -1 and gl.GetError() == G.GL_INVALID_VALUE
    assert s.stats()["kernel_launches"] == n0 and s.stats()["flushes"] == f0
    # one good call: exactly the bytes it needs, strides given
    assert call(dtype=F32, strides=(100, 5000), dst_bytes=(2 * 5000 + 31 * 100 + 64) * 4) >= 0
    assert s.stats()["kernel_launches"] == n0 + 1 and gl.GetError() == 0
    # WrhipDeviceAlloc(0): a valid allocation of no usable bytes -- not NULL, its own address, freed like any other
    z0, z1 = gl.device_alloc(0), gl.device_alloc(0)
    assert z0 and z1 and z0 != z1 and z0 % 16 == 0 and gl.GetError() == 0
    gl.device_free(z0)
    gl.device_free(z1)
    gl.device_free(0)                                   # (NULL: nothing happens)
    gl.device_free(buf)
    # WrhipDeviceFree of a buffer a parked grab writes: the grab is sent first (with what it is parked behind), and the call returns
    s.r.render(_frame())
    d = gt.Dest(gl, (3, 32, 64), F32, CHW)
    t = gt.grab(s, win, (0, 0, 64, 32), d)
    assert gl.grab_result(t, wait=False) is None
    d.free()
    assert gl.WrhipFlushHeld() == 0                     # nothing is held any more
    info, _ = gl.grab_result(t)
    gt.check_info(info, (0, 0, 64, 32), 0, G.GL_RGBA8)
    s.r.finish()
    assert gl.GetError() == 0
    s.close()


# ---------------------------------------------------------------------------- 8. CPU only: the kernels' budget, the two roundings

def test_tensor_kernels_have_no_scratch(tmp_path):
    from test_kernel_budget import lib_kernels
    notes = lib_kernels(tmp_path)
    for name in ("wr_grab_tensor_kernel", "wr_grab_scale_tensor_kernel"):
        assert name in notes, sorted(notes)
        vgprs, scratch = notes[name]
        assert scratch == 0, (name, vgprs, scratch)


ROUND_SRC = r'''
#include <stdio.h>
#include <stdint.h>
#include "wr_tensor_round.h"
int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
  uint32_t u;
  while (fread(&u, 4, 1, in) == 1) { const uint16_t r[2] = {wr_f32_to_f16_bits(u), wr_f32_to_bf16_bits(u)}; fwrite(r, 2, 2, out); }
  fclose(in); fclose(out);
  return 0;
}
'''


def test_rounding_helpers(tmp_path):
    """webrender_amd/csrc/wr_tensor_round.h, the integer arithmetic both builds compile, against numpy on two million float32
    patterns: every f16 boundary case by hand, and random bits"""
    rng = np.random.default_rng(5)
    edge = np.array([0x00000000, 0x80000000, 0x33000000, 0x33000001, 0x32FFFFFF, 0x33800000, 0x33C00000, 0x387FC000, 0x387FE000, 0x387FF000,
                     0x38800000, 0x38801000, 0x38803000, 0x477FE000, 0x477FEFFF, 0x477FF000, 0x477FF001, 0x47800000, 0x7F7FFFFF,
                     0x7F800000, 0xFF800000, 0x3F800000, 0x3F801000, 0x3F803000, 0x3F80FFFF, 0x3F808000, 0x3F818000, 0x7F7F8000], np.uint32)
    sub = (rng.integers(0x33000000, 0x38800000, 500000, dtype=np.uint32)) | (rng.integers(0, 2, 500000, dtype=np.uint32) << 31)
    u = np.concatenate([edge, sub, rng.integers(0, 1 << 32, 1500000, dtype=np.uint64).astype(np.uint32)])
    x = u.view(np.float32)
    (tmp_path / "r.cpp").write_text(ROUND_SRC)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "webrender_amd", "csrc"), str(tmp_path / "r.cpp"), "-o", str(tmp_path / "r")])
    u.tofile(tmp_path / "in.bin")
    subprocess.check_call([str(tmp_path / "r"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.uint16).reshape(-1, 2)
    finite = np.isfinite(x) | np.isinf(x)
    with np.errstate(over="ignore"):
        want16 = x.astype(np.float16).view(np.uint16)
    assert int((got[finite, 0] != want16[finite]).sum()) == 0
    assert int((got[finite, 1] != gt.bf16_bits(x)[finite]).sum()) == 0
    nan = ~finite                                                             # a NaN stays one, of the same sign
    assert ((got[nan, 0] & 0x7FFF) > 0x7C00).all() and ((got[nan, 1] & 0x7FFF) > 0x7F80).all()
    assert np.array_equal(got[nan, 0] >> 15, (u[nan] >> 31).astype(np.uint16))


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name", list(RECTS))
def test_hostsim_matrix(hostsim, oracle_gcc, name):
    _matrix(hostsim, oracle_gcc, name)


def test_hostsim_f16_edges(hostsim, oracle_gcc):
    _f16_edges(hostsim, oracle_gcc)


def test_hostsim_alignment(hostsim, oracle_gcc):
    _alignment(hostsim, oracle_gcc)


def test_hostsim_r8(hostsim, oracle_gcc):
    _r8(hostsim, oracle_gcc)


@pytest.mark.parametrize("name", SCALED_NAMES)
def test_hostsim_scaled(hostsim, oracle_gcc, name):
    _scaled(hostsim, oracle_gcc, name)


def test_hostsim_rendered_frame(hostsim, oracle_gcc):
    _rendered_frame(hostsim, oracle_gcc)


def test_hostsim_stream(hostsim, oracle_gcc):
    _stream(hostsim, oracle_gcc)


def test_hostsim_ring(hostsim, oracle_gcc):
    _ring(hostsim, oracle_gcc)


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
def test_gpu_f16_edges():
    _f16_edges(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_alignment():
    _alignment(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_r8():
    _r8(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCALED_NAMES)
def test_gpu_scaled(name):
    _scaled(wrhip_lib(), _gpu_ref(), name)


@pytest.mark.gpu
def test_gpu_rendered_frame():
    _rendered_frame(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_stream():
    _stream(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_ring():
    _ring(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_contract():
    _gpu_ref()
    _contract(wrhip_lib())


@pytest.mark.gpu
def test_gpu_torch_consumes_on_the_draw_stream():
    """torch as the consumer: a WrhipDeviceAlloc'd buffer viewed through dist.DeviceArray, work enqueued on the library's draw stream
    behind a tensor grab that WrhipFlushHeld sent -- the ticket is never fetched"""
    import torch
    from webrender_amd.dist import DeviceArray
    px = _oracle_frames(_gpu_ref())["cfg2"]
    s = fg.Session(wrhip_lib(), W, H)
    stream = torch.cuda.ExternalStream(int(s.gl.WrhipGetStream()))
    # the ImageNet normalisation, and v - 128: whole numbers that F32 and BF16 both hold exactly and whose sums over a plane stay
    # below 2^24, so that the sum is the same float in whatever order the device adds
    one, mid = np.ones(4, np.float32), np.full(4, -128, np.float32)
    for dtype, tdt in ((F32, torch.float32), (BF16, torch.bfloat16)):
        for scale, bias in ((gt.SCALE, gt.BIAS), (one, mid)):
            want = gt.expected(px, dtype, CHW, 3, scale, bias)
            s.r.render(_frame())
            d = gt.Dest(s.gl, (3, 64, 64), dtype, CHW)
            gt.grab(s, s.window, (0, 0, W, H), d, size=(64, 64), scale=scale, bias=bias)
            gt.send_held(s.gl)                              # the held-back launches go out, the parked grab behind them
            raw = torch.as_tensor(DeviceArray(d.dst, d.dst_bytes), device="cuda")
            with torch.cuda.stream(stream):
                t = raw.view(tdt).view(3, 64, 64)
                sums = t.float().sum(dim=(1, 2)).cpu()
                whole = t.cpu()
            stream.synchronize()
            if dtype == F32:
                wf = want.view(np.float32)
                assert np.array_equal(whole.numpy().view(np.uint32), want)
            else:
                wf = (want.astype(np.uint32) << 16).view(np.float32)
                assert np.array_equal(whole.view(torch.int16).numpy().view(np.uint16), want)
            if scale is one:
                assert np.array_equal(wf, np.rint(wf)) and np.abs(wf).sum(axis=(1, 2)).max() < 2 ** 24
                assert np.array_equal(sums.numpy(), wf.sum(axis=(1, 2), dtype=np.float64).astype(np.float32))
            d.free()
    s.r.finish()
    assert s.gl.GetError() == 0
    s.close()
