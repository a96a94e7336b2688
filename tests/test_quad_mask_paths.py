"""The two outputs of build_mask_tasks (render_target.rs:1200-1440) that used to be reported instead of drawn.

Image masks: ps_quad_textured with QF_IS_MASK and a texture segment (CSS mask-image; :1258-1331), drawn under the multiply blend --
axis-aligned, tiled, rotated, under projective transforms (also cut by the near plane), under a scissor, behind depth runs and
flattened depth rows, in bins, in the thin pass and with the row tables off; RGBA8 and R8 mask textures.  swgl has no span shader
for the combination: every pixel is main() -- the clamped texture() sample, times v_color, .rrrr.

Rounded-rect masks (ps_quad_mask, both keys) whose clip transform is projective (:1339-1359): vClipLocalPos.w varies over the prim
and is divided out per pixel.  A prim that is itself under a projective transform AND has such a clip stays reported.

0 differing bytes: the host simulation against the reference's generated program here, libwrhip on the MI355X (-m gpu) against the
same oracle.  On the commit before this file every parity case fails with GL_INVALID_OPERATION and the masks missing."""
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
from webrender_amd import scenes
from webrender_amd.harness import render_direct, render_streamed_tapped

W = H = 512          # one 1024x512 tile cut by the window: bins, tile rows and the thin pass all still occur


def _im(**kw):
    kw.setdefault("n", 32)
    return scenes.image_masks(width=W, height=H, **kw)


CASES = [
    ("axis_linear", lambda: _im(seed=601)),
    ("axis_nearest", lambda: _im(seed=602, nearest=True)),
    ("tiled", lambda: _im(seed=603, tiled=True)),
    ("rotated", lambda: _im(seed=604, rotate=True)),
    ("rotated_nearest", lambda: _im(seed=605, rotate=True, nearest=True)),
    ("rotated_tiled", lambda: _im(seed=606, rotate=True, tiled=True, n=24)),
    ("perspective", lambda: _im(seed=607, rotate=True, perspective=True)),
    ("perspective_near_plane", lambda: _im(seed=608, rotate=True, perspective="clip")),
    # (a scissor that cuts the prims -- and the 64-px bins -- at odd pixels)
    ("scissored", lambda: _im(seed=609, scissor=True)),
    ("scissored_rotated", lambda: _im(seed=610, scissor=True, rotate=True)),
    # (opaque rects ahead of the masked prims: the rows behind them are cut into depth runs, each restarting the interpolants)
    ("occluded", lambda: scenes.add_occluders(_im(seed=611), n=30, zmax=40, seed=43)),
    ("rotated_occluded", lambda: scenes.add_occluders(_im(seed=612, rotate=True), n=30, zmax=40, seed=44)),
    # (a perspective prim ahead on the same rows: flattened depth rows)
    ("perspective_occluded", lambda: scenes.add_occluders(_im(seed=613, rotate=True, perspective=True), n=30, zmax=40, seed=45)),
    # (R8 mask textures: texture() of an R8 sampler is (r, 0, 0, 1) -- the oracle draws them, so they are drawn)
    # (anti-aliased mask edges -- not what the batcher emits, but the route every anti-aliased textured quad takes)
    ("aa_edges", lambda: _im(seed=616, mask_edge_flags=15)),
    ("aa_edges_rotated_tiled", lambda: _im(seed=617, mask_edge_flags=15, rotate=True, tiled=True)),
    ("r8_linear", lambda: _im(seed=614, r8=True)),
    ("r8_rotated_nearest_tiled", lambda: _im(seed=615, r8=True, rotate=True, nearest=True, tiled=True)),
]


# ---- ps_quad_mask under projective clip transforms
def _qm(**kw):
    kw.setdefault("n", 40)
    return scenes.quad_masks(width=W, height=H, clip_projective=True, **kw)


def _projective_clips(frame):
    """-> [(fast, clip-out)] of the mask instances whose clip transform is not the identity"""
    out = []
    for t in frame.passes[0]:
        for s in t.alpha:
            if s.desc != "MASK" or int(s.instances[0][4]) == 0:
                continue
            fast = "FAST_PATH" in s.shader
            mode = float(frame.gpu_buffer_f.data[int(s.instances[0][5]) + (2 if fast else 3)][0])
            out.append((fast, mode == 1.0))
    return out


ONLY = [i for i in range(40) if i % 3]          # the prims whose clip transform is projective

CLIP_CASES = [
    ("clip_projective", lambda: _qm(seed=651)),
    ("clip_projective_rotated", lambda: _qm(seed=652, rotate=True)),
    ("clip_projective_only", lambda: _qm(seed=653, only=ONLY)),
    ("clip_projective_only_rotated", lambda: _qm(seed=654, only=ONLY, rotate=True)),
    ("clip_projective_occluded", lambda: scenes.add_occluders(_qm(seed=655, rotate=True), n=30, zmax=40, seed=46)),
]
CASES += CLIP_CASES

# a few large masks and many small ones: also with the row kernel, the thin pass and the quad row tables off
KNOBBED = [
    ("large", lambda: _im(seed=621, n=4, size=(260, 500), rotate=True)),
    ("small", lambda: _im(seed=622, n=160, size=(12, 56), rotate=True)),
    ("clip_large", lambda: _qm(seed=661, n=4, size=(260, 500), rotate=True)),
    ("clip_small", lambda: _qm(seed=662, n=160, size=(12, 56), rotate=True)),
]
KNOBS = [None, "WRHIP_NO_TILE_ROWS", "WRHIP_NO_THIN", "WRHIP_NO_QTAB"]


def _check(got, st, want):
    assert st["gl_error"] == 0
    assert (want != 255).any()
    d = got != want
    assert not d.any(), f"{int(d.sum())} differing bytes"


# ---------------------------------------------------------------------------- CPU: what the scenes show (the oracle alone)

def _frac(a, b):
    return float((a != b).any(axis=2).mean())


@pytest.fixture(scope="module")
def oracle_masks(oracle_gcc):
    want, _ = render_direct(oracle_gcc, _im(seed=601))
    return want


def test_oracle_masks_change_the_frame(oracle_gcc, oracle_masks):
    bare, _ = render_direct(oracle_gcc, _im(seed=601, masks=False))
    assert _frac(oracle_masks, bare) > 0.10


def _r_everywhere(pix):       # (B, G, R, A bytes)
    pix[..., 0] = pix[..., 1] = pix[..., 3] = pix[..., 2]
    return pix


def _a_over_r(pix):
    pix[..., 2] = pix[..., 3]
    return pix


def test_oracle_masks_read_the_red_channel_alone(oracle_gcc, oracle_masks):
    grey, _ = render_direct(oracle_gcc, _im(seed=601, atlas_edit=_r_everywhere))
    assert not (oracle_masks != grey).any()
    moved, _ = render_direct(oracle_gcc, _im(seed=601, atlas_edit=_a_over_r))
    assert _frac(oracle_masks, moved) > 0.05


def test_mask_atlas_has_independent_channels_and_a_corner_image():
    pix, srcs = scenes.mask_image_atlas(np.random.default_rng(5))
    assert srcs[-1][2:] == (pix.shape[1], pix.shape[0])
    assert all(20 <= s[2] - s[0] <= 64 and 20 <= s[3] - s[1] <= 64 for s in srcs)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (pix[..., a] != pix[..., b]).mean() > 0.9


def test_scissored_steps_cut_bins_off_their_edges():
    frame = _im(seed=609, scissor=True)
    sc = [s.scissor for t in frame.passes[0] for s in t.alpha if s.scissor is not None]
    assert len(sc) >= 8
    assert all(x % 64 and y % 64 and (x + w) % 64 and (y + h) % 64 for (x, y, w, h) in sc)
    assert all(s.scissor is None for t in _im(seed=601).passes[0] for s in t.alpha)


def test_projective_clip_cases_cover_both_keys_and_clip_out():
    for name, make in CLIP_CASES:
        clips = _projective_clips(make())
        assert sum(1 for f, _ in clips if f) >= 4, name
        assert sum(1 for f, _ in clips if not f) >= 4, name
        assert sum(1 for _, out in clips if out) >= 4, name
    assert not _projective_clips(scenes.quad_masks(width=W, height=H, n=40, seed=651))


def test_oracle_projective_clips_change_the_frame(oracle_gcc):
    want, _ = render_direct(oracle_gcc, _qm(seed=651))
    flat, _ = render_direct(oracle_gcc, scenes.quad_masks(width=W, height=H, n=40, seed=651))
    assert _frac(want, flat) > 0.01


def _reported(lib, frame, capfd):
    from webrender_amd import glapi, glconst as G
    from webrender_amd.renderer import Renderer
    gl = glapi.GL(lib)
    r = Renderer(gl, frame.width, frame.height)
    r.render(frame)
    r.finish()
    assert gl.GetError() == G.GL_INVALID_OPERATION
    assert gl.GetError() == 0
    assert "perspective" in capfd.readouterr().err
    px = r.read_pixels()
    r.destroy()
    assert (px != 255).any()          # the rest of the frame is drawn


def test_hostsim_projective_prim_under_projective_clip_is_reported(hostsim, capfd):
    _reported(hostsim, _qm(seed=656, rotate=True, perspective=True), capfd)


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_hostsim_image_masks_match_oracle(hostsim, oracle_gcc, name, make):
    want, _ = render_direct(oracle_gcc, make())
    got, st = render_direct(hostsim, make())
    _check(got, st, want)


@pytest.mark.parametrize("knob", KNOBS, ids=[k or "default" for k in KNOBS])
@pytest.mark.parametrize("name,make", KNOBBED, ids=[c[0] for c in KNOBBED])
def test_hostsim_image_masks_every_route(hostsim, oracle_gcc, name, make, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    want, _ = render_direct(oracle_gcc, make())
    got, st = render_direct(hostsim, make())
    _check(got, st, want)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_gpu_image_masks_match_oracle(name, make):
    want, _ = render_direct(_gpu_ref(), make())
    got, st = render_direct(wrhip_lib(), make())
    _check(got, st, want)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS + ["WRHIP_NO_FUSE_THIN"], ids=[k or "default" for k in KNOBS + ["WRHIP_NO_FUSE_THIN"]])
@pytest.mark.parametrize("name,make", KNOBBED, ids=[c[0] for c in KNOBBED])
def test_gpu_image_masks_every_route(name, make, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    want, _ = render_direct(_gpu_ref(), make())
    got, st = render_direct(wrhip_lib(), make())
    _check(got, st, want)


@pytest.mark.gpu
def test_gpu_projective_prim_under_projective_clip_is_reported(capfd):
    _reported(wrhip_lib(), _qm(seed=656, rotate=True, perspective=True), capfd)


def _streamed(lib, ref, carried):
    """Three different frames back to back with nothing between them that drains the held-back launches (the next frame's setup runs
    inside this frame's raster launch); each is compared where it was drawn with the oracle's frame, through the texture taps."""
    import frame_taps as ft
    makes = [lambda: _im(seed=631), lambda: _im(seed=632, tiled=True, nearest=True), lambda: _im(seed=633, rotate=True, perspective=True)]
    wants = [render_direct(ref, mk())[0] for mk in makes]
    px, st, taps = render_streamed_tapped(lib, [mk() for mk in makes])
    assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
    # (every flush after the first is carried by the launch the flush before held back: anything that drained between frames loses these)
    assert st["setup_carried"] >= carried, st
    assert len(taps) == len(makes)
    for k, (want, tap) in enumerate(zip(wants, taps)):
        assert (want != 255).any()
        stored = ft.window_stored(want)
        assert (tap["status"], tap["width"], tap["height"]) == (0, stored.shape[1], stored.shape[0]), k
        assert tuple(tap["digest"]) == ft.digest(stored), f"frame {k}: not the oracle's digest"
    assert not (px != wants[-1]).any()


def test_hostsim_image_masks_streamed(hostsim, oracle_gcc):
    _streamed(hostsim, oracle_gcc, 2)


@pytest.mark.gpu
def test_gpu_image_masks_streamed():
    _streamed(wrhip_lib(), _gpu_ref(), 2)
