"""Interleaved 4:2:2 video (YUV_FORMAT_INTERLEAVED: one YUY2 / GL_RGB_RAW_422_APPLE texture on sColor0) through brush_yuv_image and
composite ... YUV: blendYUV's one-sampler overload with textureLinearPlanarYUY2 for a linear sampler, main() with textureLinearYUY2 /
texelFetchYUY2 for the tails and for a nearest one -- axis-aligned, rotated, skewed, anti-aliased, masked, under perspective, behind
occluders, under the TEXTURE_RECT keys, on every route of the tile pass.  0 differing bytes: the host simulation against the
reference's generated program here, libwrhip on the MI355X (-m gpu) against the same oracle.  Video cut by the near plane stays
reported (GL_INVALID_OPERATION at Finish), and the frames of the other layouts are the ones they were."""
import hashlib
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
from webrender_amd import scenes, glconst as G
from webrender_amd.frame import Frame, TextureRef, Target, Step, CompositeTile
from webrender_amd.harness import render_direct


def _grid(**kw):
    kw.setdefault("width", 512)
    kw.setdefault("height", 512)
    kw.setdefault("n", 40)
    return scenes.yuv_grid(formats="interleaved", **kw)


CASES = [
    ("axis_aligned", lambda: _grid(seed=601)),
    ("axis_aligned_nearest", lambda: _grid(seed=602, nearest=True)),
    ("rotated", lambda: _grid(seed=603, rotate=True)),
    ("rotated_nearest", lambda: _grid(seed=604, rotate=True, nearest=True)),
    ("perspective", lambda: _grid(seed=605, perspective=True)),
    ("perspective_mixed_occluded", lambda: scenes.add_occluders(_grid(seed=606, perspective="mixed"), zmax=160, seed=43)),
    ("rotated_masked", lambda: _grid(seed=607, rotate=True, masked=True)),
    ("force_aa", lambda: _grid(seed=608, force_aa=True)),
    ("rect_axis_aligned", lambda: scenes.texture_rect(_grid(seed=609))),
    ("rect_rotated", lambda: scenes.texture_rect(_grid(seed=610, rotate=True))),
    ("composites", lambda: scenes.yuv_composites(width=512, height=512, formats="interleaved")),
    ("composites_nearest", lambda: scenes.yuv_composites(width=512, height=512, formats="interleaved", nearest=True)),
    ("composites_rect", lambda: scenes.texture_rect(scenes.yuv_composites(width=512, height=512, formats="interleaved"))),
]

# a few large videos (tile rows) and many small ones (bins): also with the row kernel, the thin pass and the row tables off
KNOBBED = [
    ("large", lambda: _grid(rotate=True, perspective="mixed", seed=611, n=6)),
    ("small", lambda: _grid(rotate=True, perspective="mixed", seed=612, n=160)),
]
KNOBS = [None, "WRHIP_NO_TILE_ROWS", "WRHIP_NO_THIN", "WRHIP_NO_QTAB"]


def edge_frame(nearest=False):
    """The sampler's edges on two tiny textures (8 x 4 and 16 x 6): uv rects from x = 0 and from an odd x, to the last column and one
    short of it, drawn 1:1, 3.7 x up, 0.5 x down and 0.37 px off the pixel grid -- the i.x >= 0 fraction mask left of the first texel
    centre, both selectors, the width - 3 saturation of both fractions at the right edge, the last chunk of the last row."""
    rng = np.random.default_rng(77)
    frame = Frame(256, 256, (1.0, 1.0, 1.0, 1.0))
    filt = G.GL_NEAREST if nearest else G.GL_LINEAR
    texs = []
    for (w, h) in ((8, 4), (16, 6)):
        t = scenes.yuy2_texture(f"yuy2_{w}x{h}", rng.integers(0, 256, size=(h, w), dtype=np.uint8), rng.integers(0, 256, size=(h, w // 2), dtype=np.uint8),
                                rng.integers(0, 256, size=(h, w // 2), dtype=np.uint8), filt)
        frame.static_textures.append(t)
        texs.append((t, w, h))
    tex = TextureRef("edge_tile", 256, 256, G.GL_RGBA8, G.GL_LINEAR, render_target=True, with_depth=True)
    target = Target(tex, "picture_tile", clear_color=(1.0, 1.0, 1.0, 1.0), clear_depth=True)
    task = frame.add_render_task((0.0, 0.0, 256.0, 256.0), 1.0, (0.0, 0.0))
    big = (-scenes.BIG, -scenes.BIG, scenes.BIG, scenes.BIG)
    z = 0
    for ti, (t, w, h) in enumerate(texs):
        opaque, alpha = [], []
        uvs = [(0, 0, w, h), (1, 0, w, h), (0, 0, w - 1, h), (1, 1, w - 1, h - 1), (3, 0, w, h)]
        y = 4.0 + 126.0 * ti
        for ui, uv in enumerate(uvs):
            src = frame.gpu_cache.push([[float(v) for v in uv], [0.0, 0.0, 0.0, 0.0]])
            uw, uh = uv[2] - uv[0], uv[3] - uv[1]
            x = 4.0
            for si, (sc, off) in enumerate(((1.0, 0.0), (3.7, 0.0), (0.5, 0.0), (1.0, 0.37), (3.7, 0.37))):
                z += 1
                spec = frame.gpu_cache.push([[8.0, float(z % 7), float(scenes.YUV_FORMAT_INTERLEAVED), 0.0]])
                rect = (x + off, y + off, x + off + uw * sc, y + off + uh * sc)
                ph = frame.add_prim_header(rect, big, z, spec, 0, task, (src, 0, 0, 0))
                (opaque if (ui + si) % 2 == 0 else alpha).append(frame.brush_instance(ph, scenes.CLIP_TASK_EMPTY))
                x += float(np.ceil(uw * sc)) + 3.0
            y += float(np.ceil(uh * 3.7)) + 2.0
        target.opaque.append(Step("brush_yuv_image TEXTURE_2D,YUV", "PRIM_INSTANCES", np.array(opaque[::-1], dtype=np.int32), None, "opaque", textures={0: t}))
        target.alpha.append(Step("brush_yuv_image ALPHA_PASS,TEXTURE_2D,YUV", "PRIM_INSTANCES", np.array(alpha, dtype=np.int32), "PremultipliedAlpha", "alpha",
                                 textures={0: t}))
    frame.composite_tiles.append(CompositeTile(tex, (0.0, 0.0, 256.0, 256.0), (0.0, 0.0, 256.0, 256.0), opaque=True))
    frame.passes.append([target])
    return frame


def _check(got, st, want):
    assert st["gl_error"] == 0
    assert (want != 255).any()
    d = got != want
    assert not d.any(), f"{int(d.sum())} differing bytes"


def _reported(lib, frame, capfd):
    from webrender_amd import glapi
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


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_hostsim_interleaved_video_matches_oracle(hostsim, oracle_gcc, name, make):
    want, _ = render_direct(oracle_gcc, make())
    got, st = render_direct(hostsim, make())
    _check(got, st, want)


@pytest.mark.parametrize("nearest", [False, True], ids=["linear", "nearest"])
def test_hostsim_interleaved_sampler_edges(hostsim, oracle_gcc, nearest):
    want, _ = render_direct(oracle_gcc, edge_frame(nearest))
    got, st = render_direct(hostsim, edge_frame(nearest))
    _check(got, st, want)


@pytest.mark.parametrize("knob", KNOBS, ids=[k or "default" for k in KNOBS])
@pytest.mark.parametrize("name,make", KNOBBED, ids=[c[0] for c in KNOBBED])
def test_hostsim_interleaved_video_every_route(hostsim, oracle_gcc, name, make, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    want, _ = render_direct(oracle_gcc, make())
    got, st = render_direct(hostsim, make())
    _check(got, st, want)


def test_hostsim_near_plane_interleaved_video_is_reported(hostsim, capfd):
    _reported(hostsim, _grid(n=24, seed=613, perspective="clip"), capfd)


# ---------------------------------------------------------------------------- the scene builders

def test_interleaved_atlas_layout():
    """One GL_RGB_RAW_422_APPLE texture of 2 bytes per pixel, uploaded as GL_RGB_422_APPLE / GL_UNSIGNED_SHORT_8_8_REV_APPLE; brush
    blocks [8, colour space, 4, 0]; one image source per video, some from an odd column, one to the texture's last column and row"""
    frame = _grid(seed=601)
    (t,) = frame.static_textures
    assert (t.fmt, t.upload_format, t.upload_type) == (G.GL_RGB_RAW_422_APPLE, G.GL_RGB_422_APPLE, G.GL_UNSIGNED_SHORT_8_8_REV_APPLE)
    assert t.pixels.dtype == np.uint8 and t.pixels.shape == (t.h, t.w, 2)
    cache = frame.gpu_cache.texture_data(1).reshape(-1, 4)
    hi = frame.prim_headers_i.texture_data(1).reshape(-1, 4)
    specs, sources = set(), set()
    for targets in frame.passes:
        for target in targets:
            for step in list(target.opaque) + list(target.alpha):
                assert set(step.textures) - {9} == {0}
                for inst in np.asarray(step.instances).reshape(-1, 4):
                    h0, h1 = hi[2 * inst[0]], hi[2 * inst[0] + 1]
                    specs.add(int(h0[1]))
                    sources.add(int(h1[0]))
    for a in specs:
        assert cache[a][0] == 8.0 and cache[a][2] == 4.0 and cache[a][3] == 0.0
    rects = [tuple(int(v) for v in cache[a]) for a in sources]
    assert sum(r[0] % 2 == 1 for r in rects) >= 2
    assert any(r[2] == t.w and r[3] == t.h for r in rects)


def _frame_digest(frame):
    h = hashlib.sha256()
    for targets in frame.passes:
        for target in targets:
            for step in list(target.opaque) + list(target.alpha) + list(target.steps):
                h.update(step.shader.encode())
                h.update(np.ascontiguousarray(step.instances).tobytes())
    for t in frame.static_textures:
        h.update(f"{t.name} {t.w} {t.h} {t.fmt}".encode())
        h.update(np.ascontiguousarray(t.pixels).tobytes())
    for store in (frame.gpu_cache, frame.prim_headers_f, frame.prim_headers_i, frame.transforms, frame.render_tasks):
        h.update(np.ascontiguousarray(store.texture_data(1)).tobytes())
    return h.hexdigest()


# SHA-256 of _frame_digest's bytes -- every step's program key and instance bytes, the static textures, the data textures -- taken
# from the commit before `formats="interleaved"` existed: the new argument changes no random draw and no address of these frames
UNCHANGED = [
    ("default", lambda: scenes.yuv_grid(), "2238a32482b7e6adbf5c0b0135cb3628cb61c28f06229178b837e6a9bf28d5d9"),
    ("rotated_hdr", lambda: scenes.yuv_grid(rotate=True, hdr=True), "6cd530ce016fb26e7b2ce04b0164e57344c8b866e3ba62b4b293a0522013bd77"),
    ("composites", lambda: scenes.yuv_composites(), "2603f022e708acb6c5ccff8e1a553dee0dfc0b390c8944cbc85952a75cdf839d"),
]


@pytest.mark.parametrize("name,make,digest", UNCHANGED, ids=[c[0] for c in UNCHANGED])
def test_other_layouts_frames_unchanged(name, make, digest):
    assert _frame_digest(make()) == digest


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_gpu_interleaved_video_matches_oracle(name, make):
    want, _ = render_direct(_gpu_ref(), make())
    got, st = render_direct(wrhip_lib(), make())
    _check(got, st, want)


@pytest.mark.gpu
@pytest.mark.parametrize("nearest", [False, True], ids=["linear", "nearest"])
def test_gpu_interleaved_sampler_edges(nearest):
    want, _ = render_direct(_gpu_ref(), edge_frame(nearest))
    got, st = render_direct(wrhip_lib(), edge_frame(nearest))
    _check(got, st, want)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS + ["WRHIP_NO_FUSE_THIN"], ids=[k or "default" for k in KNOBS + ["WRHIP_NO_FUSE_THIN"]])
@pytest.mark.parametrize("name,make", KNOBBED, ids=[c[0] for c in KNOBBED])
def test_gpu_interleaved_video_every_route(name, make, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    want, _ = render_direct(_gpu_ref(), make())
    got, st = render_direct(wrhip_lib(), make())
    _check(got, st, want)


@pytest.mark.gpu
def test_gpu_near_plane_interleaved_video_is_reported(capfd):
    _reported(wrhip_lib(), _grid(n=24, seed=613, perspective="clip"), capfd)
