"""brush_yuv_image under rotations, skews and projective transforms: the general-quad path (WR_PK_TEX_QUAD with a WR_PK_YUV base)
for both program keys, both texture types and every plane layout that is drawn -- three R8 planes, NV12, three 10-bit R16 planes,
P010 -- with swgl_antiAlias edges, clip masks, depth runs and flattened depth rows.  0 differing bytes: the host simulation against
the reference's generated program here, libwrhip on the MI355X (-m gpu) against the same oracle.  Video cut by the near plane and
a planar video whose chroma varyings differ under a projective transform stay reported (GL_INVALID_OPERATION at Finish)."""
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
from webrender_amd import scenes
from webrender_amd.harness import render_direct

# the four plane layouts: yuv_grid(hdr, formats)
LAYOUTS = {"planar": (False, "planar"), "nv12": (False, "semi"), "planar10": (True, "planar"), "p010": (True, "semi")}


def _grid(layout, **kw):
    hdr, fmts = LAYOUTS[layout]
    return scenes.yuv_grid(hdr=hdr, formats=fmts, **kw)


CASES = [(f"rotated_{lay}", (lambda lay=lay, i=i: _grid(lay, rotate=True, seed=410 + i, n=40))) for i, lay in enumerate(LAYOUTS)]
# (nearest samplers: the 8-bit layouts -- 16-bit planes take the linear path only, axis-aligned or not)
CASES += [(f"rotated_{lay}_nearest", (lambda lay=lay, i=i: _grid(lay, rotate=True, nearest=True, seed=420 + i, n=40))) for i, lay in enumerate(LAYOUTS) if i < 2]
CASES += [("perspective_nv12_nearest", lambda: _grid("nv12", perspective=True, nearest=True, seed=425, n=40))]
CASES += [(f"perspective_{lay}", (lambda lay=lay, i=i: _grid(lay, perspective=True, seed=430 + i, n=40))) for i, lay in enumerate(LAYOUTS)]
CASES += [
    ("rotated_masked", lambda: scenes.yuv_grid(rotate=True, masked=True, seed=441, n=40)),
    ("perspective_masked", lambda: scenes.yuv_grid(perspective=True, masked=True, seed=442, n=40, hdr=True)),
    ("rotated_occluded", lambda: scenes.add_occluders(scenes.yuv_grid(rotate=True, seed=443, n=50), zmax=160, seed=41)),
    # (a perspective prim ahead on the same rows: the rows behind it are flattened depth rows)
    ("perspective_occluded", lambda: scenes.add_occluders(scenes.yuv_grid(perspective="mixed", seed=444, n=50), zmax=160, seed=42)),
    ("force_aa", lambda: scenes.yuv_grid(force_aa=True, seed=445, n=40)),
    ("force_aa_masked_10bit", lambda: scenes.yuv_grid(force_aa=True, masked=True, hdr=True, seed=446, n=40)),
    ("rect_rotated", lambda: scenes.texture_rect(scenes.yuv_grid(rotate=True, seed=451, n=40))),
    ("rect_rotated_nv12", lambda: scenes.texture_rect(scenes.yuv_grid(rotate=True, planar=False, seed=452, n=40))),
    ("rect_rotated_10bit", lambda: scenes.texture_rect(scenes.yuv_grid(rotate=True, hdr=True, seed=453, n=40))),
    ("rect_perspective", lambda: scenes.texture_rect(scenes.yuv_grid(perspective=True, seed=454, n=40))),
    ("rect_force_aa_masked", lambda: scenes.texture_rect(scenes.yuv_grid(force_aa=True, masked=True, seed=455, n=40))),
    ("rect_sheared_rows", lambda: scenes.texture_rect(sheared_videos())),
]

# a few large videos (tile rows) and many small ones (bins): also with the row kernel and the thin pass off
KNOBBED = [
    ("large", lambda: scenes.yuv_grid(rotate=True, perspective="mixed", seed=461, n=6)),
    ("small", lambda: scenes.yuv_grid(rotate=True, perspective="mixed", seed=462, n=160)),
]
KNOBS = [None, "WRHIP_NO_TILE_ROWS", "WRHIP_NO_THIN", "WRHIP_NO_QTAB"]


def sheared_videos(width=512, height=512, seed=457):
    """Planar videos under a horizontal shear (x' = x + s y): every row of such a prim steps its planes along x only, so the rows meet
    blendYUV's CompositeYUV-backed condition of the rect overload (swgl_ext.h:1199-1240) -- and rotated ones beside them, which do not."""
    rng = np.random.default_rng(seed)
    frame = scenes.yuv_grid(width=width, height=height, n=12, seed=seed, formats="planar", rotate=True)
    hi = frame.prim_headers_i.data
    for r in range(0, hi.shape[0], 4):
        s = float(rng.uniform(-0.5, 0.5))
        m = np.eye(4)
        m[0, 1] = s
        m[0, 3] = -s * 256.0
        hi[r, 2] = frame.add_transform(m.T.astype(np.float32), np.linalg.inv(m).T.astype(np.float32), axis_aligned=False)
    return frame


def _check(got, st, want):
    assert st["gl_error"] == 0
    assert (want != 255).any()
    d = got != want
    assert not d.any(), f"{int(d.sum())} differing bytes"


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_hostsim_video_transforms_match_oracle(hostsim, oracle_gcc, name, make):
    want, _ = render_direct(oracle_gcc, make())
    got, st = render_direct(hostsim, make())
    _check(got, st, want)


@pytest.mark.parametrize("knob", KNOBS, ids=[k or "default" for k in KNOBS])
@pytest.mark.parametrize("name,make", KNOBBED, ids=[c[0] for c in KNOBBED])
def test_hostsim_video_transforms_every_route(hostsim, oracle_gcc, name, make, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    want, _ = render_direct(oracle_gcc, make())
    got, st = render_direct(hostsim, make())
    _check(got, st, want)


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


def planar_split_chroma(seed=471):
    """Planar videos under projective transforms whose V plane is sampled from another rect than the U plane"""
    frame = scenes.yuv_grid(width=512, height=512, n=16, seed=seed, formats="planar", perspective=True)
    rv = frame.gpu_cache.push([[2, 2, 60, 40], [0.0, 0.0, 0.0, 0.0]])
    hi = frame.prim_headers_i.data
    hi[1::2, 2] = rv                  # (user data row of every header: the third word is vUv_V's image source)
    return frame


def test_hostsim_near_plane_video_is_reported(hostsim, capfd):
    _reported(hostsim, scenes.yuv_grid(width=512, height=512, n=24, seed=472, perspective="clip"), capfd)


def test_hostsim_planar_split_chroma_perspective_is_reported(hostsim, capfd):
    _reported(hostsim, planar_split_chroma(), capfd)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_gpu_video_transforms_match_oracle(name, make):
    want, _ = render_direct(_gpu_ref(), make())
    got, st = render_direct(wrhip_lib(), make())
    _check(got, st, want)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS + ["WRHIP_NO_FUSE_THIN"], ids=[k or "default" for k in KNOBS + ["WRHIP_NO_FUSE_THIN"]])
@pytest.mark.parametrize("name,make", KNOBBED, ids=[c[0] for c in KNOBBED])
def test_gpu_video_transforms_every_route(name, make, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    want, _ = render_direct(_gpu_ref(), make())
    got, st = render_direct(wrhip_lib(), make())
    _check(got, st, want)


@pytest.mark.gpu
def test_gpu_video_transforms_4k():
    want, _ = render_direct(_gpu_ref(), scenes.make_workload("video-transforms"))
    got, st = render_direct(wrhip_lib(), scenes.make_workload("video-transforms"))
    _check(got, st, want)


@pytest.mark.gpu
def test_gpu_near_plane_video_is_reported(capfd):
    _reported(wrhip_lib(), scenes.yuv_grid(width=512, height=512, n=24, seed=472, perspective="clip"), capfd)


@pytest.mark.gpu
def test_gpu_planar_split_chroma_perspective_is_reported(capfd):
    _reported(wrhip_lib(), planar_split_chroma(), capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rotate", "perspective"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gpu_video_transforms_sweep(layout, mode):
    """20 fixed seeds per layout and transform kind, small frames"""
    ref = _gpu_ref()
    bad = []
    for seed in range(500, 520):
        mk = lambda: _grid(layout, width=512, height=512, n=14, seed=seed, **{mode: True})
        want, _ = render_direct(ref, mk())
        got, st = render_direct(wrhip_lib(), mk())
        if st["gl_error"] != 0 or (got != want).any():
            bad.append((seed, st["gl_error"], int((got != want).sum())))
    assert not bad, bad
