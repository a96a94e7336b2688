"""The legacy clip masks (cs_clip_rectangle, both keys, and cs_clip_box_shadow) whose clip or prim spatial node is not the identity.

Rotations and skews: vLocalPos steps along a row in x AND y -- the span rasterisers with both local steps non-zero.  They were drawn
before this file (libwrhip took the same path as for the identity) but nothing showed it.

Projective nodes: vLocalPos.w is a varying.  Both span shaders begin with `if (swgl_interpStep(vLocalPos).w != 0.0) return;`, so the
decision is a ROW's: a row along which w does not move runs the span rasteriser with its own w ("rows": w varies with y alone), a row
at w <= 0 is solid 0, and every other row runs main() on every chunk -- the position divided per lane, the AA range from lanes 0 / 1
of the chunk, 0 where w <= 0 ("behind": part of the mask lies at or behind the camera plane).

0 differing bytes: the host simulation against the reference's generated program here, libwrhip on the MI355X (-m gpu) against the
same oracle -- through the mask-row kernel, through the bins (WRHIP_NO_MASK_ROWS), streamed behind held-back launches, and sampled by
a picture tile.  On the commit before this file every projective / rows / behind case fails with GL_INVALID_OPERATION and the masks
missing."""
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
import frame_taps as ft
from webrender_amd import scenes, glapi, glconst as G
from webrender_amd.frame import TRANSFORM_NON_AXIS_ALIGNED
from webrender_amd.harness import render_direct
from webrender_amd.renderer import Renderer

ATLAS, N = 512, 12
KINDS = ("affine", "projective", "rows", "behind")
FAMILIES = {"clip": (scenes.clip_masks, "clip_masks", 31), "box": (scenes.box_shadow_masks, "box_shadow_masks", 41)}


def _scene(family, how=None, kind=None, **kw):
    make, _, seed = FAMILIES[family]
    kw.setdefault("n", N)
    kw.setdefault("atlas", ATLAS)
    kw.setdefault("seed", seed)
    if how is not None:
        kw[how + "_transform"] = kind
    return make(**kw)


def _case(family, how, kind, **kw):
    tag = "-".join(f"{k}{v}" for k, v in kw.items())
    return (f"{family}-{how}-{kind}" + (f"-{tag}" if tag else ""), family, dict(how=how, kind=kind, **kw))


# every kind as clip transform and as prim transform; clip_masks holds both programs of cs_clip_rectangle, and at n = 12 its second,
# multiplied step
PLAIN = [_case(f, how, kind) for f in FAMILIES for how in ("clip", "prim") for kind in KINDS]
MIXED = [_case(f, how, "mix") for f in FAMILIES for how in ("clip", "prim")]
# device pixel scale 2; and either side of the four-pixels-per-lane switch, with a task on the last column and row
OTHER = [_case("clip", "clip", "projective", dps=2.0), _case("box", "prim", "projective", dps=2.0),
         _case("clip", "clip", "projective", n=8, atlas=331, seed=34, pin_corner=True),
         _case("box", "prim", "rows", n=3, atlas=331, seed=49, pin_corner=True),
         _case("clip", "prim", "mix", n=8, atlas=513, seed=34, pin_corner=True),
         _case("box", "clip", "projective", n=5, atlas=513, seed=49, pin_corner=True)]
CASES = PLAIN + MIXED + OTHER
# ... and through the bins
BINNED = [c for c in CASES if c[2]["kind"] in ("projective", "mix")]

# Row shapes: tasks 1-3 pixels wide (no span part: every pixel is the tail), widths of 4 k + 1 .. 4 k + 3, tasks wider than 256 pixels
# (a lane of the row kernel holds more than one pixel of a row, and more than one chunk), tasks one row high; fifteen tasks, so that
# every kind of "mix" (k mod 5) meets a clip-out instance (k mod 3 == 2)
SHAPES = [(1, 37), (2, 41), (3, 29), (5, 33), (6, 30), (7, 31), (9, 1), (300, 21), (13, 1), (1, 1), (261, 2), (23, 17), (3, 1), (330, 5), (34, 9)]
SHAPED = [(f"{prog}-{how}", prog, how) for prog in ("fast", "general", "box") for how in ("clip", "prim")]


def _shaped(prog, how):
    kw = {how + "_transform": "mix", "task_sizes": SHAPES, "n": len(SHAPES), "atlas": ATLAS}
    if prog == "box":
        return scenes.box_shadow_masks(seed=43, **kw)
    return scenes.clip_masks(seed=33, program=prog, **kw)


def _tile_scene(kind="mix"):
    return scenes.masked_rects(width=512, height=512, n=40, seed=14, atlas=512, fractional=True, clip_transform=kind)


def _name(frame):
    return frame.readback[0].name


def _check(got, st, want, name):
    assert st["gl_error"] == 0
    assert (want[name] != 255).any()
    d = got[name] != want[name]
    assert not d.any(), f"{int(d.sum())} differing bytes"


_refs = {}


def _want(ref, key, make):
    """The oracle's render of a frame, once per session"""
    if (ref, key) not in _refs:
        _refs[(ref, key)] = render_direct(ref, make())[0]
    return _refs[(ref, key)]


def _parity(lib, ref, name, family, kw):
    frame = _scene(family, **kw)
    got, st = render_direct(lib, frame)
    _check(got, st, _want(ref, name, lambda: _scene(family, **kw)), _name(frame))


def _parity_shaped(lib, ref, prog, how):
    frame = _shaped(prog, how)
    got, st = render_direct(lib, frame)
    _check(got, st, _want(ref, ("shaped", prog, how), lambda: _shaped(prog, how)), _name(frame))


def _parity_tile(lib, ref):
    want = _want(ref, "tile", _tile_scene)
    got, st = render_direct(lib, _tile_scene())
    assert st["gl_error"] == 0
    assert not (got != want).any(), f"{int((got != want).sum())} differing bytes"


# ---------------------------------------------------------------------------- CPU: what the scenes hold (no library but the oracle)

def _instances(frame):
    """-> [(corner positions in device pixels (4, 2), dps, clip node, prim node)] of the frame's legacy clip instances"""
    out = []
    for tgt in frame.passes[0]:
        for s in tgt.steps:
            for inst in s.instances:
                ox, oy = float(inst["origins"][2]), float(inst["origins"][3])
                a = inst["area"]
                pts = np.array([(ox + a[0], oy + a[1]), (ox + a[2], oy + a[1]), (ox + a[0], oy + a[3]), (ox + a[2], oy + a[3])], np.float64)
                out.append((pts, float(inst["dps"]), int(inst["tids"][0]), int(inst["tids"][1])))
    return out


def _node(frame, tid):
    b = frame.transforms.data[(tid & ~TRANSFORM_NON_AXIS_ALIGNED) * 8:][:8].astype(np.float64)
    return b[:4].T, b[4:].T         # m, inv_m


def _corner_w(frame, pts, dps, ctid, ptid):
    """vLocalPos.w at the four corners (TL, TR, BL, BR) of a task: clip_shared.glsl:43-78 for the planar nodes of these scenes (no z)"""
    m, _ = _node(frame, ptid)
    _, inv = _node(frame, ctid)
    assert m[2, 3] == 0 and inv[3, 2] == 0 and inv[2, 3] == 0
    w = []
    for (dx, dy) in pts:
        pos = m @ np.array([dx / dps, dy / dps, 0.0, 1.0])
        p = inv @ np.array([pos[0] / pos[3], pos[1] / pos[3], 0.0, 1.0])
        w.append(p[3] * pos[3])
    return np.array(w)


def test_scenes_without_the_arguments_hold_no_node():
    for family in FAMILIES:
        assert all(c == 0 and p == 0 for _, _, c, p in _instances(_scene(family)))
        f = _scene(family)
        assert f.transforms.len == 8          # the identity alone


@pytest.mark.parametrize("how", ["clip", "prim"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_scenes_hold_the_kinds_they_name(family, how):
    def ws(kind):
        f = _scene(family, how, kind)
        insts = _instances(f)
        assert all((c if how == "clip" else p) & TRANSFORM_NON_AXIS_ALIGNED for _, _, c, p in insts)
        assert all((p if how == "clip" else c) == 0 for _, _, c, p in insts)
        return f, insts, [_corner_w(f, *i) for i in insts]

    _, _, w = ws("affine")
    assert all(np.all(np.abs(x - 1.0) < 1e-6) for x in w)
    # rows: w equal within each vertex pair (exactly: the w row of the node has no x term), unequal between the pairs
    f, insts, w = ws("rows")
    for (_, _, c, p) in insts:
        m, inv = _node(f, p if how == "prim" else c)
        assert (m if how == "prim" else inv)[3, 0] == 0.0
    assert all(x[0] == x[1] and x[2] == x[3] and abs(x[0] - x[2]) > 0.02 and x.min() > 0 for x in w)
    # projective: w differs along x, and stays positive over the task
    _, _, w = ws("projective")
    assert sum(1 for x in w if abs(x[0] - x[1]) > 0.02 and abs(x[2] - x[3]) > 0.02) >= len(w) // 2
    assert all(x.min() > 0 for x in w)
    # behind: a corner at w <= 0 and one at w > 0
    _, _, w = ws("behind")
    assert sum(1 for x in w if x.min() <= 0 < x.max()) >= 3
    # mix: every kind, and the identity
    f, insts, w = _mix(family, how)
    assert any(c == 0 and p == 0 for _, _, c, p in insts)
    assert any(x.min() <= 0 < x.max() for x in w) and any(x[0] == x[1] and x[0] != x[2] for x in w) and any(x[0] != x[1] and x.min() > 0 for x in w)


def _mix(family, how):
    f = _scene(family, how, "mix")
    insts = _instances(f)
    return f, insts, [_corner_w(f, *i) for i in insts]


def test_mixed_clip_scene_has_the_multiplied_step():
    f = _scene("clip", "clip", "mix")
    steps = f.passes[0][0].steps
    assert [s.blend for s in steps] == [None, None, "Multiply"]
    assert {s.shader for s in steps} == {"cs_clip_rectangle FAST_PATH", "cs_clip_rectangle"}


def test_shaped_scenes_hold_the_row_shapes_and_a_clip_out_of_every_kind():
    for _, prog, how in SHAPED:
        f = _shaped(prog, how)
        first = f.passes[0][0].steps[0]
        if prog != "box":
            assert first.shader == ("cs_clip_rectangle FAST_PATH" if prog == "fast" else "cs_clip_rectangle")
        sizes = [(int(i["area"][2]), int(i["area"][3])) for i in first.instances]
        assert sizes == SHAPES
        assert {1, 2, 3} <= {w for w, _ in sizes} and {1, 2, 3} <= {w % 4 for w, _ in sizes if w > 4}
        assert any(w > 256 for w, _ in sizes) and any(h == 1 for _, h in sizes)
        out_kinds = {k % 5 for k, i in enumerate(first.instances) if float(i["mode"]) == 1.0}
        assert out_kinds == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("name,family,kw", [c for c in PLAIN if c[2]["kind"] != "affine"], ids=[c[0] for c in PLAIN if c[2]["kind"] != "affine"])
def test_oracle_nodes_change_the_masks(oracle_gcc, name, family, kw):
    """more than 2 % of the mask bytes differ from the untransformed twin's (the smallest measured: 4.3 %)"""
    tex = FAMILIES[family][1]
    want = _want(oracle_gcc, name, lambda: _scene(family, **kw))[tex]
    flat = _want(oracle_gcc, family, lambda: _scene(family))[tex]
    assert float((want != flat).mean()) > 0.02


def test_oracle_tile_scene_samples_the_masks(oracle_gcc):
    want = _want(oracle_gcc, "tile", _tile_scene)
    flat = _want(oracle_gcc, "tile-flat", lambda: _tile_scene(None))
    assert float((want != flat).any(axis=2).mean()) > 0.02


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name,family,kw", CASES, ids=[c[0] for c in CASES])
def test_hostsim_matches_oracle(hostsim, oracle_gcc, name, family, kw):
    _parity(hostsim, oracle_gcc, name, family, kw)


@pytest.mark.parametrize("name,family,kw", BINNED, ids=[c[0] for c in BINNED])
def test_hostsim_matches_oracle_in_the_bins(hostsim, oracle_gcc, name, family, kw, monkeypatch):
    monkeypatch.setenv("WRHIP_NO_MASK_ROWS", "1")
    _parity(hostsim, oracle_gcc, name, family, kw)


@pytest.mark.parametrize("knob", [None, "WRHIP_NO_MASK_ROWS"], ids=["rows", "bins"])
@pytest.mark.parametrize("name,prog,how", SHAPED, ids=[c[0] for c in SHAPED])
def test_hostsim_row_shapes(hostsim, oracle_gcc, name, prog, how, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    _parity_shaped(hostsim, oracle_gcc, prog, how)


@pytest.mark.parametrize("knob", [None, "WRHIP_NO_TILE_ROWS"], ids=["default", "WRHIP_NO_TILE_ROWS"])
def test_hostsim_picture_tile_samples_the_masks(hostsim, oracle_gcc, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    _parity_tile(hostsim, oracle_gcc)


# Streamed: three different frames back to back with nothing between them that drains the held-back launches (the mask-row store and
# the held-back launches are shared between the frames); each frame's mask texture is tapped behind it -- a digest taken on the device,
# in stream order -- and compared with the oracle's.
STREAM = [("clip", dict(how="clip", kind="projective", seed=35)), ("box", dict(how="prim", kind="projective", seed=45)),
          ("clip", dict(how="prim", kind="affine", seed=36))]


def _streamed(lib, ref):
    frames = [_scene(f, **kw) for f, kw in STREAM]
    wants = [_want(ref, ("stream", k), lambda f=f, kw=kw: _scene(f, **kw)) for k, (f, kw) in enumerate(STREAM)]
    gl = glapi.GL(lib)
    r = Renderer(gl, frames[0].width, frames[0].height)
    tickets = []
    for f in frames:
        r.render(f)
        tickets.append(gl.tap_texture(r.textures[_name(f)].id))
    r.finish()
    assert gl.GetError() == 0
    assert all(t >= 0 for t in tickets), tickets
    taps = [gl.tap_result(t) for t in tickets]
    st = gl.stats()
    last = r.device.read_texture(r.textures[_name(frames[-1])])
    r.destroy()
    assert st["carrier_lost"] == 0, st
    for k, (f, want, tap) in enumerate(zip(frames, wants, taps)):
        stored = want[_name(f)]
        assert (stored != 255).any()
        assert (tap["status"], tap["width"], tap["height"], tap["format"]) == (0, ATLAS, ATLAS, G.GL_R8), (k, tap)
        assert tuple(tap["digest"]) == ft.digest(stored), f"frame {k}: not the oracle's digest"
    assert not (last != wants[-1][_name(frames[-1])]).any()


def test_hostsim_streamed(hostsim, oracle_gcc):
    _streamed(hostsim, oracle_gcc)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,family,kw", CASES, ids=[c[0] for c in CASES])
def test_gpu_matches_oracle(name, family, kw):
    _parity(wrhip_lib(), _gpu_ref(), name, family, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name,family,kw", BINNED, ids=[c[0] for c in BINNED])
def test_gpu_matches_oracle_in_the_bins(name, family, kw, monkeypatch):
    monkeypatch.setenv("WRHIP_NO_MASK_ROWS", "1")
    _parity(wrhip_lib(), _gpu_ref(), name, family, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", [None, "WRHIP_NO_MASK_ROWS"], ids=["rows", "bins"])
@pytest.mark.parametrize("name,prog,how", SHAPED, ids=[c[0] for c in SHAPED])
def test_gpu_row_shapes(name, prog, how, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    _parity_shaped(wrhip_lib(), _gpu_ref(), prog, how)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", [None, "WRHIP_NO_TILE_ROWS"], ids=["default", "WRHIP_NO_TILE_ROWS"])
def test_gpu_picture_tile_samples_the_masks(knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    _parity_tile(wrhip_lib(), _gpu_ref())


@pytest.mark.gpu
def test_gpu_streamed():
    _streamed(wrhip_lib(), _gpu_ref())
