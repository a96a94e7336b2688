"""Writes to textures that recorded or held-back draws still read (tests/test_write_hazards.py).

libwrhip records draws per target and flushes them later, and holds the last raster level of a flush back until the next flush
(Context::Tail).  A write that comes from outside the draw stream -- an upload, a copy, a blit, a clear, a deletion, new storage -- or
a second draw into a target that was sampled must therefore not overtake the draws that read the old contents, and must be seen by the
draws that follow.  swgl executes every call at once, so the oracle's results are the truth for any call order.

run(backend_path, case) runs the identical call script on either backend and returns everything observable as numpy arrays.

Group A ("pending"): one frame's data, two or more targets of their own, nothing between the draws and the write that would flush --
no readback, blit to a keeper, query or tap, and the per-frame GpuBuffer textures are deleted only at the end.  Every step's result
lands in a target of its own; all are read after the one Finish.  On libwrhip the script also notes WrhipStats::flushes when its first
draw has been recorded and immediately before every write under test: equal values mean the write met recorded, unflushed draws.

Group B ("held"): frames streamed through Renderer.render with the window tapped after each of them (a tap flushes but leaves the
held-back launches held) and WrhipFlushHeld called once per frame, which reports whether they are.  The oracle's window is read after
every frame instead.  The uploads between the frames are issued by the case, not by Renderer.resolve.

Textures are at most 512 texels a side except where an existing builder fixes them (yuv_grid's 1024 x 1024 plane atlases, filter_grid's
1024 x 1024 picture atlas); the existing builders' bytes are left alone."""
import copy
import numpy as np
from webrender_amd import glconst as G, scenes
from webrender_amd.glapi import GL
from webrender_amd.renderer import Renderer
from webrender_amd.frame import Frame, TextureRef, Target, Step, CompositeTile, CLIP_TASK_EMPTY, TEX_W

W = H = 512
BIG = scenes.BIG
F32 = (G.GL_RGBA, G.GL_FLOAT)


# ---------------------------------------------------------------------------- the script runner

class Script:
    """One context and a window (512 x 512 unless told otherwise) on one backend"""

    def __init__(self, backend_path, w=W, h=H):
        self.gl = GL(backend_path)
        self.w, self.h = w, h
        self.r = Renderer(self.gl, w, h)
        self.d = self.r.device
        self.wrhip = self.gl.is_wrhip
        self.keep = {}                  # result name -> TextureRef of a target read after the Finish
        self.gb = []
        self.flushes_first_draw = None
        self.flushes_at_write = []
        self.out = {}

    def _flushes(self):
        return int(self.gl.stats()["flushes"]) if self.wrhip else 0

    # -- group A
    def begin(self, frame, statics=True):
        """What Renderer.render does ahead of a frame's passes; the GpuBuffer textures live until finish()"""
        r, d = self.r, self.d
        if statics:
            for ref in frame.static_textures:
                r.resolve(ref)
        d.disable_depth_write()
        d.set_blend(False)
        r.bind_frame_data(frame)
        self.gb = [r._create_gpu_buffer_texture("sGpuBufferF", frame.gpu_buffer_f, G.GL_RGBA32F, G.GL_RGBA, G.GL_FLOAT),
                   r._create_gpu_buffer_texture("sGpuBufferI", frame.gpu_buffer_i, G.GL_RGBA32I, G.GL_RGBA_INTEGER, G.GL_INT)]

    def draw(self, target, keep=True, valid_rect=None):
        """A picture tile's dirty rect goes with the target (Target.dirty_rect); valid_rect: what the compositor shows of the tile"""
        if target.kind == "picture_tile":
            self.r.draw_picture_cache_target(target, valid_rect)
        else:
            self.r.draw_offscreen_target(target)
        if self.flushes_first_draw is None:
            self.flushes_first_draw = self._flushes()
        if keep:
            self.keep[target.texture.name] = target.texture

    def write(self):
        """Called immediately before a write under test"""
        self.flushes_at_write.append(self._flushes())

    def tex(self, ref):
        return self.r.resolve(ref)

    def upload(self, ref, x, y, px):
        """TexSubImage2D of `px` at (x, y) of the texture of `ref`, in the format `ref` uploads"""
        fmt = ref.upload_format or (G.GL_RED if ref.fmt == G.GL_R8 else G.GL_BGRA)
        px = np.ascontiguousarray(px)
        self.d.upload_texture(self.tex(ref), x, y, px.shape[1], px.shape[0], fmt, ref.upload_type or G.GL_UNSIGNED_BYTE, px)

    def blit(self, src, dst, s, dd, filt=G.GL_NEAREST):
        gl = self.gl
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, self.tex(src).fbo)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, self.tex(dst).fbo)
        gl.BlitFramebuffer(s[0], s[1], s[2], s[3], dd[0], dd[1], dd[2], dd[3], G.GL_COLOR_BUFFER_BIT, filt)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, 0)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)

    def finish(self):
        self.gl.Finish()
        out = self.out
        out["gl_error"] = np.array(int(self.gl.GetError()))
        for name, ref in self.keep.items():
            out[name] = self.d.read_texture(self.tex(ref)).copy()
        if self.wrhip and self.flushes_first_draw is not None:
            out["flushes_first_draw"] = np.array(self.flushes_first_draw)
            out["flushes_at_write"] = np.array(self.flushes_at_write)
        for t in self.gb:
            self.d.delete_texture(t)
        self.r.destroy()
        return out

    # -- group B
    def stream(self, frames, probe="after_frame", tiles=()):
        """frames: [(pre, frame)]: `pre(script)` issues the writes that come before the frame (None: none).  probe: where
        WrhipFlushHeld is called, once per frame -- "after_frame", or "end_frame": ahead of the deletion of the frame's GpuBuffer
        textures at the end of Renderer.render, for frames whose held-back launches read those (the deletion is then the write).
        tiles: TextureRefs of targets that live across the frames -- all are read back after the last frame ("tile/<name>"), the
        oracle's after every frame as well ("frame<k>/<name>"); libwrhip's WrhipStats are noted after every frame ("stats<k>": a frame's
        held-back launches are not in them yet) and after the Finish ("stats_end")"""
        gl, r = self.gl, self.r
        window = gl.WrhipGetFramebufferTexture(0) if self.wrhip else 0
        tickets, held = [], []
        if self.wrhip and probe == "end_frame":
            delete = self.d.delete_texture

            def probing_delete(tex):
                if len(held) == r.frame_count:      # (the first deletion of this frame)
                    held.append(int(gl.WrhipFlushHeld()))
                delete(tex)
            self.d.delete_texture = probing_delete
        for k, (pre, frame) in enumerate(frames):
            if pre is not None:
                pre(self)
            r.render(frame)
            if self.wrhip:
                tickets.append(gl.tap_texture(window))
                if probe == "after_frame":
                    held.append(int(gl.WrhipFlushHeld()))
                if tiles:
                    self.out["stats%d" % k] = dict(gl.stats())
            else:
                self.out["frame%d" % k] = r.read_pixels().copy()
                for ref in tiles:
                    self.out["frame%d/%s" % (k, ref.name)] = self.d.read_texture(self.tex(ref)).copy()
        gl.Finish()
        self.out["gl_error"] = np.array(int(gl.GetError()))
        if self.wrhip:
            assert all(t >= 0 for t in tickets), tickets
            for k, t in enumerate(tickets):
                res = gl.tap_result(t)
                assert (res["status"], res["width"], res["height"], res["format"]) == (0, self.w, self.h, G.GL_RGBA8), res
                self.out["tap%d" % k] = np.array(res["digest"], dtype=np.uint64)
            self.out["held"] = np.array(held)
            if tiles:
                self.out["stats_end"] = dict(gl.stats())
        self.out["window"] = r.read_pixels().copy()
        for ref in tiles:
            self.out["tile/" + ref.name] = self.d.read_texture(self.tex(ref)).copy()
        r.destroy()
        return self.out


# ---------------------------------------------------------------------------- frames

def retarget(target, name, swap=None, clear="keep"):
    """A copy of `target` that draws the same steps into a texture of its own called `name`; swap: {TextureRef name: TextureRef} --
    the steps sample the replacement instead; clear: another clear colour (None: no clear)"""
    t = copy.copy(target)
    src = target.texture
    t.texture = TextureRef(name, src.w, src.h, src.fmt, src.filter, render_target=True, with_depth=src.with_depth)
    if clear != "keep":
        t.clear_color = clear
    if swap:
        def sw(step):
            s2 = copy.copy(step)
            s2.textures = {k: (swap.get(v.name, v) if v is not None else None) for k, v in step.textures.items()}
            return s2
        t.opaque, t.alpha, t.steps = [sw(x) for x in target.opaque], [sw(x) for x in target.alpha], [sw(x) for x in target.steps]
    return t


def premultiplied_noise(rng, h, w):
    px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    px[..., :3] = (px[..., :3].astype(np.uint16) * px[..., 3:4] // 255).astype(np.uint8)
    return px


def image_pixels(seed, size):
    """A premultiplied BGRA picture with structure at every scale: ramps under noise, a quarter of it opaque"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, size=(size, size, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:size, 0:size]
    px[..., 0] = (xx * 255 // (size - 1)).astype(np.uint8)
    px[..., 1] = (yy * 255 // (size - 1)).astype(np.uint8)
    px[..., 3] = np.where((xx // 64 + yy // 64) % 4 == 0, 255, px[..., 3])
    px[..., :3] = (px[..., :3].astype(np.uint16) * px[..., 3:4] // 255).astype(np.uint8)
    return px


def image_frame(seed=7, n=20, atlas=256, nearest=False, render_target=False):
    """image_grid in small: `n` alpha-pass brush_image prims in one 512 x 512 tile ("tile"), from sub-images of odd sizes on a 64-texel
    grid of an atlas x atlas RGBA8 texture ("hz_atlas": frame.atlas) -- 1:1 at whole and fractional positions, scaled up and down"""
    rng = np.random.default_rng(seed)
    frame = Frame(W, H, (1.0, 1.0, 1.0, 1.0))
    t_atlas = TextureRef("hz_atlas", atlas, atlas, G.GL_RGBA8, G.GL_NEAREST if nearest else G.GL_LINEAR, render_target=render_target,
                         pixels=image_pixels(seed, atlas), upload_format=G.GL_BGRA)
    frame.static_textures.append(t_atlas)
    cells = atlas // 64
    srcs = []
    for cy in range(cells):
        for cx in range(cells):
            w, h = int(rng.integers(30, 62)) | 1, int(rng.integers(30, 62)) | 1
            x, y = cx * 64 + 1, cy * 64 + 1
            srcs.append((w, h, frame.gpu_cache.push([[x, y, x + w, y + h], [0.0, 0.0, 0.0, 0.0]])))
    tex = TextureRef("tile", W, H, G.GL_RGBA8, G.GL_LINEAR, render_target=True, with_depth=True)
    target = Target(tex, "picture_tile", clear_color=(1.0, 1.0, 1.0, 1.0), clear_depth=True)
    task = frame.add_render_task((0.0, 0.0, float(W), float(H)), 1.0, (0.0, 0.0))
    inst = []
    for k in range(n):
        sw, sh, addr = srcs[k % len(srcs)]
        mode = k % 4
        sc = (1.0, 1.0, float(rng.uniform(1.3, 3.0)), 0.5)[mode]
        w, h = sw * sc, sh * sc
        px, py = float(rng.uniform(0, W - w)), float(rng.uniform(0, H - h))
        if mode == 0:
            px, py = float(int(px)), float(int(py))
        opacity = 1.0 if k % 3 else float(rng.uniform(0.3, 0.9))
        spec = frame.gpu_cache.push([[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [-1.0, -1.0, 0.0, 0.0]])
        ph = frame.add_prim_header((px, py, px + w, py + h), (-BIG, -BIG, BIG, BIG), k + 1, spec, 0, task,
                                   (4 | (1 << 16), 0, int(round(opacity * 65535.0)), 0))
        inst.append(frame.brush_instance(ph, CLIP_TASK_EMPTY, resource_address=addr))
    target.alpha.append(Step("brush_image ALPHA_PASS,TEXTURE_2D", "PRIM_INSTANCES", np.array(inst, dtype=np.int32), "PremultipliedAlpha", "alpha",
                             textures={0: t_atlas}))
    frame.passes.append([target])
    frame.composite_tiles.append(CompositeTile(tex, (0.0, 0.0, float(W), float(H)), None, opaque=True))
    frame.atlas, frame.tile = t_atlas, target
    return frame


_glyphs = {}
GLYPH_SIZES = (13, 18, 24)


def glyph_atlases():
    """The cells of three sizes of scenes.build_glyph_atlas / build_glyph_atlas_lcd packed again into 512 x 512 atlases:
    (R8 pixels, {(size, ch): (uv rect, offset, advance)}, BGRA pixels, {(size, ch): (uv rect, offset)})"""
    if not _glyphs:
        def pack(big, table, shape):
            px, out = np.zeros(shape, np.uint8), {}
            x = y = 1
            shelf = 0
            for key in sorted(k for k in table if k[0] in GLYPH_SIZES):
                x0, y0, x1, y1 = (int(v) for v in table[key][0])
                w, h = x1 - x0, y1 - y0
                if x + w + 1 > shape[1]:
                    x, y, shelf = 1, y + shelf + 1, 0
                assert y + h + 1 <= shape[0]
                px[y:y + h, x:x + w] = big[y0:y1, x0:x1]
                out[key] = ((float(x), float(y), float(x + w), float(y + h)),) + tuple(table[key][1:])
                x += w + 1
                shelf = max(shelf, h)
            return px, out
        a, t = pack(*scenes.build_glyph_atlas(), (512, 512))
        al, tl = pack(*scenes.build_glyph_atlas_lcd(), (512, 512, 4))
        _glyphs["v"] = (a, t, al, tl)
    return _glyphs["v"]


def text_frame(seed=3, lines=6, per_line=18, run_len=6, modes=(0,)):
    """cfg3_text in small: runs of ps_text_run glyphs in one 512 x 512 tile from the 512 x 512 atlases of glyph_atlases() ("hz_glyphs_r8":
    frame.atlas, colour mode 0; "hz_glyphs_bgra8": frame.atlas_bgra, the other modes, cycled per run).  frame.used: the (bgra, (size,
    ch)) cells its runs sample."""
    rng = np.random.default_rng(seed)
    a, table, al, table_l = glyph_atlases()
    frame = Frame(W, H, (1.0, 1.0, 1.0, 1.0))
    frame.atlas = TextureRef("hz_glyphs_r8", 512, 512, G.GL_R8, G.GL_LINEAR, pixels=a, upload_format=G.GL_RED)
    frame.atlas_bgra = TextureRef("hz_glyphs_bgra8", 512, 512, G.GL_RGBA8, G.GL_LINEAR, pixels=al, upload_format=G.GL_BGRA)
    frame.static_textures += [frame.atlas] + ([frame.atlas_bgra] if any(modes) else [])
    res = {k: frame.add_glyph_resource(v[0], v[1], 1.0) for k, v in table.items()}
    res_l = {k: frame.add_glyph_resource(v[0], v[1], 1.0) for k, v in table_l.items()} if any(modes) else {}
    tex = TextureRef("tile", W, H, G.GL_RGBA8, G.GL_LINEAR, render_target=True, with_depth=True)
    target = Target(tex, "picture_tile", clear_color=(1.0, 1.0, 1.0, 1.0), clear_depth=True)
    task = frame.add_render_task((0.0, 0.0, float(W), float(H)), 1.0, (0.0, 0.0))
    inst, inst_bgra, used, z = [], [], set(), 1
    pitch = H / lines
    for li in range(lines):
        size = int(rng.choice(GLYPH_SIZES))
        pen = float(rng.uniform(0.0, 30.0))
        base_y = float(size + li * pitch + rng.uniform(0.0, 1.0))
        chars = [int(c) if (size, int(c)) in table and (size, int(c)) in table_l else 65 for c in rng.integers(33, 127, size=per_line)]
        for r0 in range(0, per_line, run_len):
            run = chars[r0:r0 + run_len]
            pts, x = [], 0.0
            for c in run:
                pts.append((x, 0.0))
                x += table[(size, c)][2]
            rgba = np.array([[rng.integers(0, 96), rng.integers(0, 96), rng.integers(0, 96), rng.integers(160, 256)]], np.uint8)
            addr = frame.add_text_run(scenes.premultiply(rgba)[0], pts)
            ph = frame.add_prim_header((pen, base_y, 0.0, 0.0), (-BIG, -BIG, BIG, BIG), z, addr, 0, task, (65535, 0, 0, 0))
            mode = modes[(z - 1) % len(modes)]
            for gi, c in enumerate(run):
                (inst_bgra if mode else inst).append(Frame.glyph_instance(ph, gi, (res_l if mode else res)[(size, c)], color_mode=mode))
                used.add((bool(mode), (size, c)))
            pen += x
            z += 1
    if inst:
        target.alpha.append(Step("ps_text_run ALPHA_PASS,TEXTURE_2D", "PRIM_INSTANCES", np.array(inst, dtype=np.int32), "PremultipliedAlpha", "alpha",
                                 textures={0: frame.atlas}))
    if inst_bgra:
        target.alpha.append(Step("ps_text_run ALPHA_PASS,TEXTURE_2D", "PRIM_INSTANCES", np.array(inst_bgra, dtype=np.int32), "PremultipliedAlpha",
                                 "alpha", textures={0: frame.atlas_bgra}))
    frame.passes.append([target])
    frame.composite_tiles.append(CompositeTile(tex, (0.0, 0.0, float(W), float(H)), None, opaque=True))
    frame.tile, frame.used = target, used
    return frame


def one_tile(build, **kw):
    """A builder of scenes.py at 512 x 512 with one 512 x 512 picture tile: (frame, its tile target)"""
    with scenes.tile_size(W, H):
        frame = build(width=W, height=H, **kw)
    assert len(frame.passes[-1]) == 1
    return frame, frame.passes[-1][0]


def mask_target(seed, clear=(1.0, 1.0, 1.0, 1.0)):
    """An R8 512 x 512 alpha target of rounded-rect clip masks (the instances carry all their data)"""
    t = scenes.clip_masks(n=14, atlas=512, seed=seed).passes[0][0]
    t.clear_color = clear
    return t


def decoration_target(seed, clear=(0.0, 0.0, 0.0, 0.0)):
    """An RGBA8 512 x 512 texture-cache target of two-stop gradients and line decorations (likewise)"""
    t = scenes.cache_decorations(n_lines=14, n_grads=24, n_lgrads=0, atlas=512, seed=seed).passes[0][0]
    t.clear_color = clear
    return t


# ---------------------------------------------------------------------------- group A

def a1_image_atlas(s, nearest, overlap=False):
    f = image_frame(nearest=nearest)
    s.begin(f)
    s.draw(retarget(f.tile, "T0"))
    s.write()
    # rows that are no multiple of 16 bytes at an odd origin: some sub-images whole, some in part, some not at all
    s.upload(f.atlas, 37, 21, premultiplied_noise(np.random.default_rng(91), 77, 123))
    if overlap:
        # two more patches, the second overlapping the first and both the one above: the last write wins
        s.upload(f.atlas, 90, 60, premultiplied_noise(np.random.default_rng(92), 61, 75))
        s.upload(f.atlas, 101, 83, premultiplied_noise(np.random.default_rng(93), 45, 37))
    s.draw(retarget(f.tile, "T1"))


def a2_glyph_atlas(s):
    f = text_frame(seed=5)
    s.begin(f)
    s.draw(retarget(f.tile, "T0"))
    s.write()
    # a few glyph cells replaced by other glyphs' coverage, upside down
    a, table = glyph_atlases()[:2]
    cells = sorted(table[k][0] for on_bgra, k in f.used if not on_bgra)[::3]
    assert len(cells) >= 4
    for (x0, y0, x1, y1) in cells:
        s.upload(f.atlas, int(x0), int(y0), a[int(y0):int(y1), int(x0):int(x1)][::-1, ::-1])
    s.draw(retarget(f.tile, "T1"))


def _brush_rects():
    return one_tile(scenes.cfg2_overlapping_rects, n=30, seed=48, encoding="brush")


def a3a_gpu_cache_row(s):
    f, tile = _brush_rects()
    s.begin(f)
    s.draw(retarget(tile, "T0"))
    s.write()
    # part of one row of the GPU cache: the colour blocks of some of the prims both targets draw
    rng = np.random.default_rng(94)
    x0, n = 3, 17
    assert f.gpu_cache.len > x0 + n
    cols = scenes.premultiply(np.concatenate([rng.integers(0, 256, size=(n, 3)), rng.integers(90, 256, size=(n, 1))], axis=1).astype(np.uint8))
    s.d.upload_texture(s.r.data_tex["sGpuCache"][0], x0, 0, n, 1, *F32, np.ascontiguousarray(cols, dtype=np.float32))
    s.draw(retarget(tile, "T1"))


def _whole(s, sampler, data):
    tex, rows = s.r.data_tex[sampler]
    assert data.shape == (rows, TEX_W, 4)
    s.d.upload_texture(tex, 0, 0, TEX_W, rows, *F32, np.ascontiguousarray(data))


def _moved_headers(f):
    hf = f.prim_headers_f.texture_data().copy()
    n = f.prim_headers_f.len // 2
    flat = hf.reshape(-1, 4)
    flat[0:2 * n:2] += np.float32(11.0) * np.array([1.0, -1.0, 1.0, -1.0], np.float32)      # the local rects move; the clip rects stay
    return hf


def a3b_whole_reupload(s):
    f, tile = _brush_rects()
    s.begin(f)                      # (the data textures are uploaded whole in the batch the draws below are recorded in)
    s.draw(retarget(tile, "T0"))
    s.write()
    _whole(s, "sPrimitiveHeadersF", _moved_headers(f))
    cache = f.gpu_cache.texture_data(20).copy()
    cache[0, :f.gpu_cache.len] = cache[0, :f.gpu_cache.len][:, [2, 0, 1, 3]]
    _whole(s, "sGpuCache", cache)
    s.draw(retarget(tile, "T1"))


def a3c_whole_then_row(s):
    f, tile = _brush_rects()
    s.begin(f)
    s.draw(retarget(tile, "T0"))
    s.write()
    # whole, then part of a row of the same texture with nothing drawn in between: the row lands on top
    cache = f.gpu_cache.texture_data(20).copy()
    cache[0, :f.gpu_cache.len] = cache[0, :f.gpu_cache.len][:, [1, 2, 0, 3]]
    _whole(s, "sGpuCache", cache)
    x0, n = 5, 13
    s.d.upload_texture(s.r.data_tex["sGpuCache"][0], x0, 0, n, 1, *F32, np.ascontiguousarray(f.gpu_cache.texture_data(20)[0, x0:x0 + n]))
    s.draw(retarget(tile, "T1"))


def _a4(s, frame, tile, a_ref_name, make_a, cleared):
    """A -> B samples A -> A drawn again -> C samples A"""
    a1 = make_a(1)
    swap = {a_ref_name: a1.texture}
    s.begin(frame, statics=False)
    s.draw(a1, keep=False)
    s.draw(retarget(tile, "B", swap))
    a2 = make_a(2)
    a2.texture = a1.texture
    if not cleared:
        a2.clear_color = None           # A's kept content is loaded and drawn over
    s.write()
    s.draw(a2)
    s.draw(retarget(tile, "C", swap))
    s.keep["A"] = s.keep.pop(a1.texture.name)


def a4_r8(s, cleared):
    f, tile = one_tile(scenes.masked_rects, n=30, seed=14, atlas=512)
    _a4(s, f, tile, "clip_mask_atlas", lambda v: mask_target(30 + v), cleared)


def a4_rgba8(s, cleared):
    f = image_frame(seed=9, n=24, atlas=512)
    _a4(s, f, f.tile, "hz_atlas", lambda v: decoration_target(150 + v), cleared)


def a5_copy_dest(s, how):
    f = image_frame(seed=11, render_target=True)
    src = TextureRef("hz_src", 200, 160, G.GL_RGBA8, G.GL_LINEAR, render_target=True, pixels=premultiplied_noise(np.random.default_rng(95), 160, 200),
                     upload_format=G.GL_BGRA)
    f.static_textures.append(src)
    s.begin(f)
    x = f.atlas
    if how == "pending_source":
        src = decoration_target(153).texture        # (created and its storage allocated before the first draw is recorded)
        s.tex(src)
    s.draw(retarget(f.tile, "T0"))
    if how == "pending_source":
        # the source of the copy is a target with recorded, unflushed draws
        s.draw(decoration_target(153), keep=False)
    s.write()
    if how == "blit" or how == "pending_source":
        s.blit(src, x, (3, 5, 3 + 123, 5 + 77), (37, 21, 37 + 123, 21 + 77))
    elif how == "blit_linear":
        s.blit(src, x, (0, 0, 200, 160), (37, 21, 37 + 131, 21 + 97), G.GL_LINEAR)
    elif how == "copy":
        s.gl.CopyImageSubData(s.tex(src).id, G.GL_TEXTURE_2D, 0, 3, 5, 0, s.tex(x).id, G.GL_TEXTURE_2D, 0, 37, 21, 0, 123, 77, 1)
    else:
        col = np.array([0.25, 0.5, 0.125, 0.75], np.float32)
        s.gl.ClearTexSubImage(s.tex(x).id, 0, 37, 21, 0, 123, 77, 1, G.GL_RGBA, G.GL_FLOAT, col)
    s.draw(retarget(f.tile, "T1"))


def a6_storage_recycled(s, how):
    f = image_frame(seed=13)
    s.begin(f)
    s.draw(retarget(f.tile, "T0"))
    s.write()
    if how == "deleted":
        # X is deleted; Y, of its size and format, takes its storage from the pool and is uploaded at once
        s.d.delete_texture(s.r.textures.pop(f.atlas.name))
        y = TextureRef("hz_atlas_y", f.atlas.w, f.atlas.h, G.GL_RGBA8, G.GL_LINEAR, pixels=image_pixels(14, f.atlas.w), upload_format=G.GL_BGRA)
    else:
        # X is kept and gets new storage of another size
        xt = s.tex(f.atlas)
        s.gl.ActiveTexture(G.GL_TEXTURE0)
        s.gl.BindTexture(G.GL_TEXTURE_2D, xt.id)
        s.gl.TexStorage2D(G.GL_TEXTURE_2D, 1, G.GL_RGBA8, 300, 300)
        xt.width = xt.height = 300
        # ... and a texture of X's old size and format, which takes the storage X gave up, is uploaded at once, ahead of X itself
        s.tex(TextureRef("hz_atlas_z", f.atlas.w, f.atlas.h, G.GL_RGBA8, G.GL_LINEAR, pixels=image_pixels(15, f.atlas.w), upload_format=G.GL_BGRA))
        y = TextureRef(f.atlas.name, 300, 300, G.GL_RGBA8, G.GL_LINEAR, upload_format=G.GL_BGRA)
        s.upload(y, 0, 0, image_pixels(14, 300))
    s.tex(y)
    s.draw(retarget(f.tile, "T1", {f.atlas.name: y}))


# ---------------------------------------------------------------------------- group B

def b1_texture_cache():
    f = image_frame(seed=17, n=16)

    def pre(k):
        rect = ((37, 21, 123, 77), (11, 90, 201, 55), (129, 3, 99, 141))[k - 1]
        return lambda s: s.upload(f.atlas, rect[0], rect[1], premultiplied_noise(np.random.default_rng(200 + k), rect[3], rect[2]))
    return [(None, f)] + [(pre(k), f) for k in (1, 2, 3)]


def b2_glyph_cache():
    a, table, al, table_l = glyph_atlases()
    frames = [text_frame(seed=20 + k, modes=(0, 1, 2, 3)) for k in range(4)]
    have = set(frames[0].used)

    def only(px, tab, keys):
        out = np.zeros_like(px)
        for k in keys:
            x0, y0, x1, y1 = (int(v) for v in tab[k][0])
            out[y0:y1, x0:x1] = px[y0:y1, x0:x1]
        return out
    # the cache starts with the cells the first frame uses; every later frame brings the cells it is the first to use
    r8_0, bgra_0 = only(a, table, [k for b, k in have if not b]), only(al, table_l, [k for b, k in have if b])
    for f in frames:
        f.atlas.pixels, f.atlas_bgra.pixels = r8_0, bgra_0

    def pre(f):
        def go(s):
            new = sorted(f.used - have)
            assert len(new) >= 4
            for on_bgra, k in new:
                px, tab, ref = (al, table_l, f.atlas_bgra) if on_bgra else (a, table, f.atlas)
                x0, y0, x1, y1 = (int(v) for v in tab[k][0])
                s.upload(ref, x0, y0, px[y0:y1, x0:x1])
            have.update(new)
        return go
    return [(None, frames[0])] + [(pre(f), f) for f in frames[1:]]


def _video(frame):
    """Four versions of a video frame's plane textures: the planes are uploaded whole with new samples before every frame but the first"""
    def pre(k):
        def go(s):
            for i, ref in enumerate(frame.static_textures):
                rng = np.random.default_rng([300 + k, i])
                noise = rng.integers(0, 64, size=ref.pixels.shape).astype(ref.pixels.dtype)
                if ref.name.startswith("p010"):
                    noise = noise << 6            # (P010 keeps its samples in the high ten bits)
                s.upload(ref, 0, 0, ref.pixels ^ noise)
        return go
    return [(None, frame)] + [(pre(k), frame) for k in (1, 2, 3)]


def b3_video(kind):
    if kind == "composites":
        return _video(scenes.yuv_composites(width=W, height=H))
    if kind == "composites_yuy2":
        return _video(scenes.yuv_composites(width=W, height=H, formats="interleaved"))
    kw = {"8bit": {}, "10bit": {"hdr": True}, "yuy2": {"formats": "interleaved"}}[kind]
    return _video(one_tile(scenes.yuv_grid, n=12, **kw)[0])


def b4_filter_tables():
    # component-transfer tables live in the GPU cache and are read by the raster stage; they reach the texture through the dirty-row
    # uploads of Renderer._update_gpu_cache (the first frame's upload is whole)
    return [(None, one_tile(scenes.filter_grid, n=16, seed=71 + k, ops=[scenes.FILTER_COMPONENT_TRANSFER])[0]) for k in range(4)]


def b4_gradient_stops():
    # more than 256 gradients in one draw: the stops are read in sGpuBufferF where the frame builder put them
    frames = [one_tile(scenes.gradient_grid, n=280, seed=61 + k)[0] for k in range(3)]
    for f in frames:
        assert max(len(st.instances) for st in f.passes[-1][0].alpha) > 256
    return [(None, f) for f in frames]


def _b5(frame, tile, a_ref_name, make_a, patch):
    frames = []
    a_ref = make_a(0).texture
    for k in range(3):
        f = copy.copy(frame)
        a = make_a(k)
        a.texture = a_ref
        if patch and k:
            a.clear_color = None
        t = retarget(tile, "tile", {a_ref_name: a_ref})
        f.passes = [[a], [t]]
        f.static_textures = []
        f.composite_tiles = [CompositeTile(t.texture, (0.0, 0.0, float(W), float(H)), None, opaque=True)]
        pre = None
        if patch and k:
            # the redraw's first operation is an upload into the target, and what the target kept is drawn over
            pre = (lambda k: lambda s: s.upload(a_ref, 41, 33 + 50 * k, premultiplied_noise(np.random.default_rng(400 + k), 59, 131)))(k)
        frames.append((pre, f))
    return frames


def b5_target_redrawn(fmt):
    if fmt == "r8":
        f, tile = one_tile(scenes.masked_rects, n=30, seed=14, atlas=512)
        return _b5(f, tile, "clip_mask_atlas", lambda k: mask_target(40 + k), False)
    f = image_frame(seed=9, n=24, atlas=512)
    return _b5(f, f.tile, "hz_atlas", lambda k: decoration_target(160 + k), True)


# ---------------------------------------------------------------------------- the cases

class Case:
    def __init__(self, group, fn, differ=(), args=(), probe="after_frame"):
        self.group, self.fn, self.args, self.probe = group, fn, args, probe
        self.differ = list(differ)      # group A: (result before the write, result after it) -- they must differ in the oracle's run


T01 = [("T0", "T1")]
CASES = {
    "a1_image_atlas_linear": Case("A", a1_image_atlas, T01, (False,)),
    "a1_image_atlas_nearest": Case("A", a1_image_atlas, T01, (True,)),
    "a1_overlapping_patches": Case("A", a1_image_atlas, T01, (False, True)),
    "a2_glyph_atlas": Case("A", a2_glyph_atlas, T01),
    "a3a_gpu_cache_row": Case("A", a3a_gpu_cache_row, T01),
    "a3b_whole_reupload": Case("A", a3b_whole_reupload, T01),
    "a3c_whole_then_row": Case("A", a3c_whole_then_row, T01),
    "a4_r8_cleared": Case("A", a4_r8, [("B", "C")], (True,)),
    "a4_r8_kept": Case("A", a4_r8, [("B", "C")], (False,)),
    "a4_rgba8_cleared": Case("A", a4_rgba8, [("B", "C")], (True,)),
    "a4_rgba8_kept": Case("A", a4_rgba8, [("B", "C")], (False,)),
    "a5_blit": Case("A", a5_copy_dest, T01, ("blit",)),
    "a5_blit_linear": Case("A", a5_copy_dest, T01, ("blit_linear",)),
    "a5_copy": Case("A", a5_copy_dest, T01, ("copy",)),
    "a5_clear": Case("A", a5_copy_dest, T01, ("clear",)),
    "a5_pending_source": Case("A", a5_copy_dest, T01, ("pending_source",)),
    "a6_deleted": Case("A", a6_storage_recycled, T01, ("deleted",)),
    "a6_new_storage": Case("A", a6_storage_recycled, T01, ("new_storage",)),
    "b1_texture_cache": Case("B", b1_texture_cache),
    "b2_glyph_cache": Case("B", b2_glyph_cache),
    "b3_video_8bit": Case("B", b3_video, args=("8bit",)),
    "b3_video_10bit": Case("B", b3_video, args=("10bit",)),
    "b3_video_yuy2": Case("B", b3_video, args=("yuy2",)),
    "b3_video_composites": Case("B", b3_video, args=("composites",)),
    "b3_video_composites_yuy2": Case("B", b3_video, args=("composites_yuy2",)),
    "b4_filter_tables": Case("B", b4_filter_tables),
    "b4_gradient_stops": Case("B", b4_gradient_stops, probe="end_frame"),
    "b5_target_redrawn_r8": Case("B", b5_target_redrawn, args=("r8",)),
    "b5_target_redrawn_rgba8": Case("B", b5_target_redrawn, args=("rgba8",)),
}


def run(backend_path, case):
    """Runs case `case` (a key of CASES) on the backend library at `backend_path`; returns its results by name.
    Group A: "gl_error", every kept target's stored bytes, and on libwrhip "flushes_first_draw" / "flushes_at_write".
    Group B: "gl_error", the final "window", and per frame k the oracle's "frame<k>" (its window) or libwrhip's "tap<k>" (the two digest
    words of a tap of the window) with "held" (what WrhipFlushHeld returned after each frame)."""
    c = CASES[case]
    s = Script(backend_path)
    if c.group == "A":
        c.fn(s, *c.args)
        return s.finish()
    return s.stream(c.fn(*c.args), c.probe)
