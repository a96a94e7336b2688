"""Partial tile updates (tests/test_partial_updates.py): frames that redraw only the dirty rect of only the invalidated picture-cache
tiles, as WebRender's picture cache does on the common frame -- a Clear(colour | depth) scissored to the dirty rect, the batches
scissored to dirty & valid (Renderer.draw_picture_cache_target over Target.dirty_rect), and last frame's pixels everywhere else.

libwrhip folds only a leading full-target clear into the bins' initial value.  A partial update therefore runs as: the depth clear
(widened to the whole invalidated depth buffer) leading, the colour clear kept as an ordered prim, the target's kept colour loaded from
memory (WrTargetDesc::load_color) and scissored depth-tested draws over it -- in every raster kernel's own way.

A sequence (Seq) is four frames in one Renderer, built on hazard_cases.Script.  Frame 0 draws every tile in full.  A later frame has
ANOTHER display list everywhere (other seed: prims moved and recoloured outside the dirty rects too) but lists only the dirty tiles in
its last pass, each with a dirty rect, and composites all tiles: a backend that ignores the scissor, clears the whole tile or starts
from the clear colour gets other bytes outside the rect.  Seq.fulls[k] is frame k as a full redraw: what the oracle renders from scratch
to show that the partial result is not simply that frame.

P6 (group-A style, one Finish) puts a clear in the MIDDLE of a target: full clear, opaque depth writers, a Clear over part of them that
is not preceded by an InvalidateFramebuffer (so it stays partial for depth too), then depth-tested images / gradients behind the
writers' z."""
import copy
import numpy as np
from webrender_amd import glconst as G, scenes
from webrender_amd.device import ortho
from webrender_amd.frame import Target, Step, TextureRef
import hazard_cases as hz

FULL = "full"
CLEARS = ((1.0, 1.0, 1.0, 1.0), (0.875, 0.9375, 1.0, 1.0), (1.0, 0.9375, 0.8125, 1.0), (0.9375, 1.0, 0.875, 1.0))      # the tiles' clear colour, per frame

# tile size -> (valid height of the bottom row of tiles in the 2 x 2 windows, dirty rects a, b, c, one pixel, one row)
#   a  inside one bin at odd coordinates             b  across a bin corner (an edge where the tile has no corner), no multiple of 4
#   c  touching the last column and the last row
SIZES = {
    (128, 128): (72, (5, 7, 43, 30), (37, 51, 99, 77), (99, 109, 128, 128), (70, 33, 71, 34), (0, 41, 128, 42)),     # stride % 16 == 0, four whole bins
    (66, 65): (35, (5, 7, 43, 30), (37, 51, 65, 65), (37, 46, 66, 65), (65, 64, 66, 65), (0, 64, 66, 65)),           # bins cut by 2 px and 1 px
    (61, 37): (23, (5, 7, 43, 30), (37, 21, 59, 35), (32, 18, 61, 37), (30, 17, 31, 18), (0, 19, 61, 20)),           # less than one bin: scalar loads
    (130, 64): (36, (5, 7, 43, 30), (37, 21, 99, 51), (101, 45, 130, 64), (129, 33, 130, 34), (0, 41, 130, 42)),     # a last bin of two columns
}


def valid_rects(frame):
    """Tile name -> its valid rect in tile pixels (as Renderer.render derives it from the composite)"""
    out = {}
    for t in frame.composite_tiles:
        r, c = t.rect, t.clip_rect
        out[t.texture.name] = (int(max(c[0], r[0]) - r[0]), int(max(c[1], r[1]) - r[1]), int(min(c[2], r[2]) - r[0]), int(min(c[3], r[3]) - r[1]))
    return out


def partial(full, dirty, k):
    """Frame `full` with only the tiles of `dirty` ({name: rect | FULL}) in its last pass, each with its dirty rect"""
    f = copy.copy(full)
    tiles = []
    for target in full.passes[-1]:
        target.clear_color = CLEARS[k % len(CLEARS)]
        if target.texture.name in dirty:
            t = copy.copy(target)
            rect = dirty[target.texture.name]
            t.dirty_rect = None if rect == FULL else rect
            tiles.append(t)
    f.passes = list(full.passes[:-1]) + [tiles]
    return f


class Seq:
    def __init__(self, fulls, plan, prepare=None):
        """fulls: frame k as a full redraw; plan: per frame k >= 1 {tile name: dirty rect | FULL} (FULL: redrawn whole, no dirty rect)"""
        self.fulls, self.plan = fulls, [None] + list(plan)
        self.w, self.h = fulls[0].width, fulls[0].height
        self.tiles = [t.texture for t in fulls[0].passes[-1]]
        self.valid = valid_rects(fulls[0])
        self.atlases = []           # (TextureRef of an off-screen target that lives across the frames, per frame k >= 1 the rects redrawn)
        for name in self.valid:
            assert all(valid_rects(f)[name] == self.valid[name] for f in fulls)
        self.frames = [partial(fulls[0], {t.name: FULL for t in self.tiles}, 0)] + [partial(fulls[k], self.plan[k], k) for k in range(1, len(fulls))]
        if prepare:
            prepare(self)

    def task_rect(self, name, rect):
        """dirty & valid, None when empty"""
        v = self.valid[name]
        r = v if rect == FULL else (max(rect[0], v[0]), max(rect[1], v[1]), min(rect[2], v[2]), min(rect[3], v[3]))
        return r if r[2] > r[0] and r[3] > r[1] else None


def two_by_two(tw, th):
    """Window size, and the plan of a window of 2 x 2 tiles of tw x th whose bottom row the window cuts: every dirty rect of the issue"""
    vh, a, b, c, pixel, row = SIZES[(tw, th)]
    e = (0, 0, tw, vh)                            # equal to the valid rect of a cut tile: the clear is not scissored
    f = (3, vh + 2, min(40, tw), th)              # wholly outside the valid rect: nothing is drawn
    g = (11, vh - 9, tw - 7, th)                  # across the valid rect's edge: the batches are cut to dirty & valid
    plan = [{"tile_0_0": a, "tile_1_0": b, "tile_0_1": e, "tile_1_1": f},
            {"tile_0_0": c, "tile_1_0": pixel, "tile_0_1": (0, vh // 2, tw, vh // 2 + 1), "tile_1_1": g},
            {"tile_0_0": row, "tile_1_0": a, "tile_1_1": b if b[3] <= vh else a}]
    return (2 * tw, th + vh), plan


def block_plan(tw, th, names, valid):
    """The same for four tiles `names` = (whole, whole, cut, cut) of a larger window: valid rect of the cut ones `valid`"""
    _, a, b, c, pixel, row = SIZES[(tw, th)]
    vw, vh = valid[2], valid[3]
    if vw < tw:
        f, g, line = (vw + 2, 3, tw, min(40, th)), (vw - 9, 11, tw, th - 7), (vw // 2, 0, vw // 2 + 1, th)
    else:
        f, g, line = (3, vh + 2, min(40, tw), th), (11, vh - 9, tw - 7, th), (0, vh // 2, tw, vh // 2 + 1)
    return [{names[0]: a, names[1]: b, names[2]: tuple(valid), names[3]: f},
            {names[0]: c, names[1]: pixel, names[2]: line, names[3]: g},
            {names[0]: row, names[1]: a, names[3]: a}]


# ---------------------------------------------------------------------------- P1, P4: rects

def rect_frame(w, h, tw, th, n, seed, encoding):
    """cfg2_overlapping_rects in small, two rects in five opaque (drawn front to back, depth-written), the others translucent"""
    rng, rects = scenes.random_rects(n, w, h, 6, max(tw, th), seed, fractional=False)
    rgb = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    alpha = np.round(rng.uniform(0.25, 0.75, size=n) * 255).astype(np.uint8)
    opaque = (np.arange(n) % 5) < 2
    alpha[opaque] = 255
    with scenes.tile_size(tw, th):
        return scenes.build_rect_frame(w, h, rects, scenes.premultiply(np.concatenate([rgb, alpha[:, None]], axis=1)), opaque, encoding)


def p1_rects(tw, th, encoding):
    (w, h), plan = two_by_two(tw, th)
    return Seq([rect_frame(w, h, tw, th, 40, 700 + k, encoding) for k in range(4)], plan)


def p4_some_tiles():
    """2 x 2 tiles of 128 x 128: frame 1 redraws one tile in part and one in full and leaves two alone, frame 2 redraws all of them
    (the window's composites can be forwarded again), frame 3 one in part"""
    tw = th = 128
    (w, h), _ = two_by_two(tw, th)
    plan = [{"tile_0_0": SIZES[(tw, th)][2], "tile_1_1": FULL},
            {n: FULL for n in ("tile_0_0", "tile_1_0", "tile_0_1", "tile_1_1")},
            {"tile_1_0": SIZES[(tw, th)][1]}]
    return Seq([rect_frame(w, h, tw, th, 40, 740 + k, "brush" if k & 1 else "quad") for k in range(4)], plan)


# ---------------------------------------------------------------------------- P2, P3: the builders of scenes.py on four tiles of a window

def block(build, tw, th, ty0, seeds, move=False, **kw):
    """Frames of `build` in a window of 512 // tw x 512 // th tiles of tw x th (the builders of scenes.py lay their prims out for
    windows of about that size) whose right column is cut to just over half its width; only the 2 x 2 tiles of the last two columns
    and of rows ty0, ty0 + 1 are drawn and composited.  move: the frames share a seed (a builder whose static textures depend
    on it) and differ in where the prims are: frame k's local rects are shifted by 7k px"""
    nx, ny = 512 // tw, 512 // th
    w, h = nx * tw - (tw // 2 - 8), ny * th
    keep = lambda tx, ty: tx in (nx - 2, nx - 1) and ty in (ty0, ty0 + 1)
    fulls = []
    for k, seed in enumerate(seeds):
        with scenes.tile_size(tw, th):
            f = build(width=w, height=h, seed=seed, tile_filter=keep, **kw)
        if move and k:
            n = f.prim_headers_f.len // 2
            f.prim_headers_f.data[0:2 * n:2] += np.float32(7.0 * k) * np.array([1.0, -1.0, 1.0, -1.0], np.float32)
        fulls.append(f)
    names = ("tile_%d_%d" % (nx - 2, ty0), "tile_%d_%d" % (nx - 2, ty0 + 1), "tile_%d_%d" % (nx - 1, ty0), "tile_%d_%d" % (nx - 1, ty0 + 1))
    return fulls, names


def step_scissor(seq, k, name, rect):
    """Splits the first alpha step of tile `name` of frame k in three; the middle one is drawn under a Step.scissor of its own, `rect`
    (x0, y0, x1, y1, inside the tile's dirty & valid rect): the steps after it are scissored to the dirty rect again"""
    t = next(t for t in seq.frames[k].passes[-1] if t.texture.name == name)
    st = t.alpha[0]
    n = len(st.instances)
    assert n >= 3
    parts = []
    for i, sl in enumerate((slice(0, n // 3), slice(n // 3, 2 * n // 3), slice(2 * n // 3, n))):
        s2 = copy.copy(st)
        s2.instances = st.instances[sl]
        if i == 1:
            s2.scissor = (rect[0], rect[1], rect[2] - rect[0], rect[3] - rect[1])
        parts.append(s2)
    t.alpha = parts + list(t.alpha[1:])


def _seq_of(fulls, names, tw, th, prepare=None):
    valid = valid_rects(fulls[0])
    return Seq(fulls, block_plan(tw, th, names, valid[names[2]]), prepare)


def p2_images(tw, th):
    """The tiles under the builder's band of opaque-pass images, with opaque rects ahead of the opaque pass and nearer than everything: the
    depth-tested images are cut into depth runs.  The atlas and the images keep their seed (block(move=True)); the occluders do not"""
    def build(seed, **kw):
        f = scenes.image_grid(seed=51, **kw)
        with scenes.tile_size(tw, th):
            return scenes.add_occluders(f, n=60, seed=900 + seed, zmax=1 << 20, wmin=6, wmax=70, first=lambda tx, ty: True)
    fulls, names = block(build, tw, th, 0 if th > 65 else 1, (1, 2, 3, 4), move=True, n=60)
    return _seq_of(fulls, names, tw, th)


def p2_text(tw, th):
    fulls, names = block(scenes.cfg3_text, tw, th, 1, (3, 4, 5, 6), lines=32, glyphs_per_line=40, run_len=8)
    return _seq_of(fulls, names, tw, th)


def p2_masked(tw, th):
    def cut(seq):
        # frame 1, the first whole tile (dirty rect a): the middle third of its prims under a scissor that cuts a's right and bottom
        a = SIZES[(tw, th)][1]
        step_scissor(seq, 1, names[0], (a[0] + 9, a[1] + 5, a[2], a[3]))
    fulls, names = block(scenes.masked_rects, tw, th, 1, (12, 13, 14, 15), n=150, atlas=512)
    return _seq_of(fulls, names, tw, th, cut)


def p3_gradients(tw, th):
    """A few large gradients per tile (what tile_rows_eligible accepts), under the builder's band of opaque-pass gradients"""
    fulls, names = block(scenes.gradient_grid, tw, th, 1 if th > 65 else 3, (61, 62, 63, 64), n=60, fractional=True)
    return _seq_of(fulls, names, tw, th)


SEQS = {}
for _tw, _th in SIZES:
    for _enc in ("quad", "brush"):
        SEQS["p1_rects_%s_%dx%d" % (_enc, _tw, _th)] = (p1_rects, (_tw, _th, _enc))
for _tw, _th in ((128, 128), (66, 65)):
    SEQS["p2_images_%dx%d" % (_tw, _th)] = (p2_images, (_tw, _th))
    SEQS["p2_text_%dx%d" % (_tw, _th)] = (p2_text, (_tw, _th))
    SEQS["p2_masked_%dx%d" % (_tw, _th)] = (p2_masked, (_tw, _th))
    SEQS["p3_gradients_%dx%d" % (_tw, _th)] = (p3_gradients, (_tw, _th))
SEQS["p4_some_tiles"] = (p4_some_tiles, ())


# ---------------------------------------------------------------------------- P5: off-screen atlases with per-task clears

def _task_targets(tex, kind, step, picks, values):
    """One Target per picked instance of `step`: a Clear scissored to the instance's task rect (draw_alpha_target's per-task clears,
    zero and one in turn), then the instance -> (targets, task rects)"""
    targets, rects = [], []
    for j, i in enumerate(picks):
        inst = step.instances[i:i + 1]
        if step.desc == "CLIP_RECT":
            x, y = float(inst["origins"][0][0]), float(inst["origins"][0][1])
            w, h = float(inst["area"][0][2]), float(inst["area"][0][3])
        else:
            x, y, w, h = step.task_rects[i]
        x0, y0, x1, y1 = max(0, int(x)), max(0, int(y)), min(tex.w, int(x + w)), min(tex.h, int(y + h))
        v = values[j % len(values)]
        t = Target(tex, kind, clear_color=(v, v, v, v), clear_rect=(x0, y0, x1 - x0, y1 - y0))
        s2 = copy.copy(step)
        s2.instances = inst
        t.steps.append(s2)
        targets.append(t)
        rects.append((x0, y0, x1, y1))
    return targets, rects


def p5_masks(atlas):
    """masked_rects whose R8 clip-mask atlas is drawn by a pass of its own (cs_clip_rectangle: the mask-rows kernel) and lives across
    the frames: a later frame clears and redraws every other clip task only (under clip transforms of another kind, so with another
    mask), and its tiles, which sample redrawn and kept tasks side by side, in part"""
    tw = th = 128
    (w, h), plan = two_by_two(tw, th)
    kinds = ("affine", "rows", "projective", "affine")
    fulls = []
    for k, kind in enumerate(kinds):
        with scenes.tile_size(tw, th):
            f = scenes.masked_rects(width=w, height=h, n=40, seed=12, atlas=atlas, clip_transform=kind)
        if k:
            n = f.prim_headers_f.len // 2
            f.prim_headers_f.data[0:2 * n:2] += np.float32(7.0 * k) * np.array([1.0, -1.0, 1.0, -1.0], np.float32)
        fulls.append(f)
    q = Seq(fulls, plan)
    tex = fulls[0].passes[0][0].texture
    q.atlases = [(tex, [None])]
    for k in range(1, len(fulls)):
        targets, rects = [], []
        for step in fulls[k].passes[0][0].steps:
            t, r = _task_targets(tex, "alpha", step, range(k & 1, len(step.instances), 2), (0.0, 1.0))
            targets += t
            rects += r
        q.frames[k].passes = [targets] + q.frames[k].passes[1:]
        q.atlases[0][1].append(rects)
    return q


def p5_blur(atlas):
    """An RGBA8 blur chain (cs_blur vertical, then horizontal: the span-rows kernel) of nine tasks in atlas-sized targets that live
    across the frames, and one 256 x 256 tile of images that sample the horizontal target on a 64-texel grid.  A later frame clears
    and redraws every other task of both targets, with another deviation, and the tile in part"""
    W = 256
    sigmas = (2.5, 1.5, 3.5, 2.0)
    fulls = []
    for k, sg in enumerate(sigmas):
        f = scenes.blur_chain(fmt="rgba8", content=(83, 83), sigma=sg, atlas=atlas, n_tasks=9, seed=4, window=(W, W))
        t_h = f.passes[-1][0].texture
        rng = np.random.default_rng(520 + k)
        tex = TextureRef("tile_0_0", W, W, G.GL_RGBA8, G.GL_LINEAR, render_target=True, with_depth=True)
        target = Target(tex, "picture_tile", clear_color=(1.0, 1.0, 1.0, 1.0), clear_depth=True)
        task = f.add_render_task((0.0, 0.0, float(W), float(W)), 1.0, (0.0, 0.0))
        inst = []
        for i in range(20):
            cx, cy = int(rng.integers(0, 4)), int(rng.integers(0, 4))
            sw, sh = int(rng.integers(30, 62)) | 1, int(rng.integers(30, 62)) | 1
            addr = f.gpu_cache.push([[cx * 64 + 1, cy * 64 + 1, cx * 64 + 1 + sw, cy * 64 + 1 + sh], [0.0, 0.0, 0.0, 0.0]])
            sc = (1.0, 1.0, float(rng.uniform(1.3, 2.0)), 0.5)[i % 4]
            pw, ph_ = sw * sc, sh * sc
            px, py = float(rng.uniform(0, W - pw)), float(rng.uniform(0, W - ph_))
            if i % 4 == 0:
                px, py = float(int(px)), float(int(py))
            spec = f.gpu_cache.push([[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [-1.0, -1.0, 0.0, 0.0]])
            ph = f.add_prim_header((px, py, px + pw, py + ph_), (-hz.BIG, -hz.BIG, hz.BIG, hz.BIG), i + 1, spec, 0, task,
                                   (4 | (1 << 16), 0, 65535 if i % 3 else int(rng.integers(20000, 60000)), 0))
            inst.append(f.brush_instance(ph, hz.CLIP_TASK_EMPTY, resource_address=addr))
        target.alpha.append(Step("brush_image ALPHA_PASS,TEXTURE_2D", "PRIM_INSTANCES", np.array(inst, dtype=np.int32), "PremultipliedAlpha", "alpha",
                                 textures={0: t_h}))
        f.passes.append([target])
        f.composite_tiles.append(hz.CompositeTile(tex, (0.0, 0.0, float(W), float(W)), None, opaque=True))
        fulls.append(f)
    _, a, b, c, _, _ = SIZES[(128, 128)]
    q = Seq(fulls, [{"tile_0_0": (a[0], a[1], a[2] + 100, a[3] + 90)}, {"tile_0_0": (b[0], b[1], b[2] + 64, b[3] + 64)}, {"tile_0_0": (c[0] + 28, c[1] + 28, 256, 256)}])
    q.atlases = []
    for p in (-3, -2):
        tex = fulls[0].passes[p][0].texture
        per_frame = [None]
        for k in range(1, len(fulls)):
            step = fulls[k].passes[p][0].steps[0]
            step.task_rects = [tuple(float(v) for v in fulls[k].render_tasks.data[2 * int(i["a"][0])]) for i in step.instances]
            step.task_rects = [(r[0], r[1], r[2] - r[0], r[3] - r[1]) for r in step.task_rects]
            targets, rects = _task_targets(tex, "color", step, range(k & 1, len(step.instances), 2), (0.0,))
            q.frames[k].passes[p] = targets
            per_frame.append(rects)
        q.atlases.append((tex, per_frame))
    return q


for _atlas in (331, 512):
    SEQS["p5_masks_%d" % _atlas] = (p5_masks, (_atlas,))
    SEQS["p5_blur_%d" % _atlas] = (p5_blur, (_atlas,))

_built = {}


def seq(name):
    if name not in _built:
        fn, args = SEQS[name]
        _built[name] = fn(*args)
    return _built[name]


def run(backend_path, name):
    """Streams sequence `name` on the backend: hazard_cases.Script.stream's results with every tile read back after the last frame
    ("tile/<name>"), the oracle's tiles after every frame ("frame<k>/<name>") and libwrhip's statistics after every frame ("stats<k>")"""
    q = seq(name)
    s = hz.Script(backend_path, q.w, q.h)
    return s.stream([(None, f) for f in q.frames], tiles=q.tiles + [a[0] for a in q.atlases])


def run_scratch(backend_path, name, k):
    """Frame k of the sequence as a full redraw in a context of its own (with the first frame's static textures, as the sequence has
    them): {tile name: stored bytes}"""
    q = seq(name)
    s = hz.Script(backend_path, q.w, q.h)
    for ref in q.fulls[0].static_textures:
        s.r.resolve(ref)
    for target in q.fulls[k].passes[-1]:
        target.clear_color = CLEARS[k % len(CLEARS)]
    s.r.render(q.fulls[k])
    s.gl.Finish()
    assert int(s.gl.GetError()) == 0
    out = {ref.name: s.d.read_texture(s.tex(ref)).copy() for ref in q.tiles}
    s.r.destroy()
    return out


# ---------------------------------------------------------------------------- P6: a clear in the middle of a target

P6_SIZE = 256
# x0, y0, x1, y1 of the mid-target clear: across the bins' corners, odd columns.  Its rows are multiples of 32 because the oracle is
# only defined there: swgl delays a full clear row by row (32 rows to a word of Texture::cleared_rows), and the scissored clear that
# follows forces the delayed one with the scissor's columns left out on EVERY row of the words its rows touch (gl.cc force_clear) --
# rows outside the scissor in those words that nothing has drawn to yet keep uninitialised memory there.
P6_RECT = (37, 32, 171, 160)
P6_COLOR = (0.25, 0.5, 0.125, 0.75)


def p6_frame(family):
    """One 256 x 256 tile of the builder's opaque-pass band (depth-tested and -written images / gradients) and alpha pass, with 40
    opaque rects nearer than all of it ahead of the opaque pass"""
    build = {"images": lambda **kw: scenes.image_grid(n=60, seed=51, **kw), "gradients": lambda **kw: scenes.gradient_grid(n=24, seed=61, **kw)}[family]
    with scenes.tile_size(P6_SIZE, P6_SIZE):
        f = build(width=512, height=512, tile_filter=lambda tx, ty: (tx, ty) == (0, 0))
        scenes.add_occluders(f, n=40, seed=931, zmax=1 << 20, wmin=10, wmax=90, first=lambda tx, ty: True)
    tile = f.passes[-1][0]
    assert len(tile.opaque) >= 2 and tile.opaque[0].shader == "brush_solid" and tile.alpha
    return f, tile


def p6(s, family, variant):
    """variant: "none" (no clear in the middle: the control), "partial" (Clear(COLOR | DEPTH) scissored to P6_RECT), "full_depth"
    (Clear(DEPTH) of the whole target), "clear_tex" (ClearTexSubImage of P6_RECT of the colour texture: the depth stays),
    "continuation" (partial, then a ReadPixels of the target, which flushes it with its depth live)"""
    f, tile = p6_frame(family)
    s.begin(f)
    r, d, gl = s.r, s.d, s.gl
    tex = s.tex(tile.texture)
    d.bind_draw_target(tex.fbo_with_depth, tex.width, tex.height)
    projection = ortho(0.0, tex.width, 0.0, tex.height)
    d.enable_depth_write()
    d.set_blend(False)
    d.clear_target((1.0, 1.0, 1.0, 1.0), 1.0, None)
    d.enable_depth(G.GL_LEQUAL)
    r._draw_step(tile.opaque[0], projection)                # the depth writers
    s.flushes_first_draw = s._flushes()
    x0, y0, x1, y1 = P6_RECT
    s.write()
    if variant in ("partial", "continuation"):
        d.clear_target(P6_COLOR, 1.0, (x0, y0, x1 - x0, y1 - y0))
    elif variant == "full_depth":
        d.clear_target(None, 1.0, None)
    elif variant == "clear_tex":
        gl.ClearTexSubImage(tex.id, 0, x0, y0, 0, x1 - x0, y1 - y0, 1, G.GL_RGBA, G.GL_FLOAT, np.array(P6_COLOR, np.float32))
    else:
        assert variant == "none"
    if variant == "continuation":
        s.out["mid"] = d.read_texture(tex).copy()
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, tex.fbo_with_depth)
    for step in tile.opaque[1:]:                            # depth-tested and -written, behind the writers
        r._draw_step(step, projection)
    d.disable_depth_write()
    d.set_blend(True)
    prev = None
    for step in tile.alpha:                                 # depth-tested
        if step.blend != prev:
            d.set_blend_mode(step.blend)
            prev = step.blend
        r._draw_step(step, projection)
    d.set_blend(False)
    d.disable_depth()
    d.invalidate_depth_target()
    s.keep["tile"] = tile.texture


P6_CASES = [(fam, var) for fam in ("images", "gradients") for var in ("partial", "full_depth", "clear_tex", "continuation")]


def run_p6(backend_path, family, variant):
    s = hz.Script(backend_path)
    p6(s, family, variant)
    return s.finish()
