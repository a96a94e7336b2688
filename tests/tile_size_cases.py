"""Cases of tests/test_target_sizes.py: the shader families drawn into picture-cache tiles whose size is no multiple of the
raster's 64-px bin (scenes.tile_size), and the off-screen families at atlas sizes whose rows are no multiple of 16 bytes or
sit at the row kernels' switch from one to four pixels per lane.

Tile sizes (the smallest at which each path can go wrong):
  61x37     smaller than one bin both ways; width = 1 (mod 4): RGBA8 stride 244, the scalar load / store path; strips of a wave
            wholly below the target
  66x65     a second bin column 2 px wide, a second bin row 1 px high
  130x64    width = 2 (mod 4), stride 520; exactly one bin row
  333x201   width = 1 (mod 4), stride 1332; several bins; odd depth row length
  260x96    width = 0 (mod 4) but no multiple of 64, stride 1040: the vector path, with lanes wholly outside
  1024x32, 32x1024   WebRender's scrollbar tile shapes: half a bin in one direction

The window is a little over two tiles each way and no multiple of the tile: tile origins then sit at x = 1, 2, 3 (mod 4)
for the forwarded composite's per-pixel branch, and the last tiles are clipped by the window.  Its height is odd; its width is
odd for every other family and a multiple of 4 for the rest (window_for).  A family whose builder needs
room to place its content (image_grid, gradient_grid: their size ranges assume a few hundred pixels) gets at least ROOMY."""
import numpy as np
from webrender_amd import scenes

TILES = [(61, 37), (66, 65), (130, 64), (333, 201), (260, 96), (1024, 32), (32, 1024)]
ROOMY = (643, 515)


def window_for(tw, th, roomy=False, aligned=False, min_h=0):
    """aligned: a width that is a multiple of 4 -- RGBA8 rows of a multiple of 16 bytes, where the forwarded composite may store
    four pixels at once and has to look at the tile's x origin -- instead of an odd one (scalar stores throughout)"""
    w, h = 2 * tw + tw // 3 + 1, max((2 * th + th // 3 + 1) | 1, min_h)
    if roomy:
        w, h = max(w, ROOMY[0]), max(h, ROOMY[1])
    w = (w + 3) & ~3 if aligned else w | 1
    if w % tw == 0:
        w += 4
    assert w % tw and h % th
    return w, h


def _text(w, h, s, n):
    return scenes.cfg3_text(width=w, height=h, lines=max(3, h // 9), glyphs_per_line=max(8, w // 6), run_len=6, seed=s)


def _images(w, h, s, n):
    f = scenes.image_grid(width=w, height=h, n=n, seed=s)
    f = scenes.add_occluders(f, n=24, seed=s + 1, zmax=80, wmin=12, wmax=200)
    return scenes.add_slivers(f, pitch=12, y1=min(240, h))


# name -> (builder(width, height, seed, n), seed, n, needs a roomy window).  `n` is the prim count in a window of up to ROOMY's
# area and grows with the window's (the scrollbar tiles' windows are long): the tiles' last columns and rows are single
# pixel lines, and enough prims have to cross them (test_target_sizes asserts that they do, on the oracle's output)
FAMILIES = {
    "rects_quad": (lambda w, h, s, n: scenes.cfg2_overlapping_rects(width=w, height=h, n=n, seed=s, fractional=True, encoding="quad"), 5, 40, False),
    "rects_brush": (lambda w, h, s, n: scenes.cfg2_overlapping_rects(width=w, height=h, n=n, seed=s, fractional=True, encoding="brush"), 6, 40, False),
    # (an anti-aliasing request takes a draw off the rect-only kernel variant, the cell raster with it: the pixel walk's edge code)
    "rects_quad_aa": (lambda w, h, s, n: scenes.cfg2_overlapping_rects(width=w, height=h, n=n, seed=s, fractional=True, encoding="quad", aa_edges=15), 7, 40, False),
    "rects_brush_aa": (lambda w, h, s, n: scenes.cfg2_overlapping_rects(width=w, height=h, n=n, seed=s, fractional=True, encoding="brush", aa_edges=15), 8, 40, False),
    "images_occluded_slivers": (_images, 52, 90, True),
    "rotated_rects": (lambda w, h, s, n: scenes.rotated_rects(width=w, height=h, n=n, seed=s), 96, 40, False),
    "perspective_images": (lambda w, h, s, n: scenes.rotated_images(width=w, height=h, n=n, seed=s, perspective=True), 106, 80, False),
    "gradient_grid": (lambda w, h, s, n: scenes.gradient_grid(width=w, height=h, n=n, seed=s), 62, 60, True),
    "text": (_text, 4, 0, False),
    "masked_rects_frac": (lambda w, h, s, n: scenes.masked_rects(width=w, height=h, n=n, seed=s, fractional=True), 13, 60, False),
    "quad_masks_rotated": (lambda w, h, s, n: scenes.quad_masks(width=w, height=h, n=n, seed=s, rotate=True), 84, 50, False),
    "blend_modes": (lambda w, h, s, n: scenes.blend_modes(width=w, height=h, per_state=n, seed=s), 112, 4, False),
    "yuv_grid": (lambda w, h, s, n: scenes.yuv_grid(width=w, height=h, n=n, seed=s), 302, 40, True),
    # (tests/test_gpu_sweep.py ONE_LSB has this family: the device's sqrt / division in the non-separable modes)
    "mix_grid_perspective": (lambda w, h, s, n: scenes.mix_blend_grid(width=w, height=h, n=n, seed=s, perspective=True), 216, 40, True),
}
# gradient_grid and yuv_grid keep the top 200 rows for their opaque prims, which end above y = 196: with 201-row tiles the first
# tile row's last row (y = 200) stays clear whatever the seed, so these two get a window of four tile rows and a bit
MIN_HEIGHT = {((333, 201), "gradient_grid"): 871, ((333, 201), "yuv_grid"): 871}
RECT_FAMILIES = ("rects_quad", "rects_brush")
# the rect and image families once more under each of these: the ragged edge in the plain bin walk as well as in the cell raster,
# in the bins as well as in the tile-rows kernel, and in stores without forwarding
KNOBS = ("WRHIP_NO_CELLS", "WRHIP_NO_TILE_ROWS", "WRHIP_NO_FORWARD")
KNOB_FAMILIES = RECT_FAMILIES + ("images_occluded_slivers",)


def tile_cases():
    """[(id, tile, family, env knob or None)]"""
    out = []
    for tile in TILES:
        for fam in FAMILIES:
            out.append((f"{tile[0]}x{tile[1]}-{fam}", tile, fam, None))
        for fam in KNOB_FAMILIES:
            for knob in KNOBS:
                out.append((f"{tile[0]}x{tile[1]}-{fam}-{knob[6:].lower()}", tile, fam, knob))
    return out


def picture_tiles(frame):
    return [tg for p in frame.passes for tg in p if tg.kind == "picture_tile"]


def build_tile_frame(tile, fam):
    """The family's frame in tiles of `tile`, with every tile texture in Frame.readback: the pixels a composite clips away are
    compared too, and a wrong store shows in the tile it happened in."""
    make, seed, n, roomy = FAMILIES[fam]
    # (every other family, the first of the rect families among them, under a window whose width is a multiple of 4)
    w, h = window_for(*tile, roomy=roomy, aligned=list(FAMILIES).index(fam) % 2 == 0, min_h=MIN_HEIGHT.get((tuple(tile), fam), 0))
    n *= max(1, -(-w * h // (ROOMY[0] * ROOMY[1])))
    with scenes.tile_size(*tile):
        frame = make(w, h, seed, n)
    tiles = picture_tiles(frame)
    assert tiles and all((tg.texture.w, tg.texture.h) == tuple(tile) for tg in tiles)
    frame.readback = list(frame.readback) + [tg.texture for tg in tiles]
    return frame


def clear_bytes(frame):
    """{tile texture name: the BGRA8 bytes its clear leaves (the rounding every backend applies to a clear colour: +0.5, truncate)}"""
    out = {}
    for tg in picture_tiles(frame):
        r, g, b, a = [int(np.float32(c) * np.float32(255.0) + np.float32(0.5)) for c in tg.clear_color]
        out[tg.texture.name] = np.array([b, g, r, a], np.uint8)
    return out


def coverage(frame, pixels):
    """Fractions of the tiles whose last column / last row / whole area differ from their clear colour somewhere in `pixels`
    ({texture name: BGRA8 array}, the oracle's): a case in which they are small would not show a wrong edge."""
    clear = clear_bytes(frame)
    col = row = anyw = 0
    for name, c in clear.items():
        d = (pixels[name] != c).any(axis=2)
        col += bool(d[:, -1].any())
        row += bool(d[-1, :].any())
        anyw += bool(d.any())
    n = len(clear)
    return col / n, row / n, anyw / n


# ---- off-screen targets ---------------------------------------------------------------------------------------------------
# 331: R8 stride 332, RGBA8 stride 1324; 513 / 515: the first widths at four pixels per lane in the row kernels
# (WR_SPAN_PPL), with a 1-px and a 3-px last lane; 512: the last width at one pixel per lane.
ATLASES = (331, 513, 515)
ATLASES_ROWS = (331, 512, 513, 515)      # clip_masks and blur_chain, the families the row kernels take


def _blur(fmt, atlas):
    # a column of tasks against the atlas's right edge, the last one against its bottom edge
    cw, ch, n = 61, 47, 3
    return scenes.blur_chain(fmt=fmt, content=(cw, ch), sigma=[2.5, 0.8, 4.0], atlas=atlas, n_tasks=n, seed=6,
                             origin=(atlas - cw, atlas - ch - (n - 1) * (ch + 3)), pattern="noise")


def offscreen_cases():
    """[(id, builder() -> frame with .readback, names of the read-back targets that must reach the last column and row)]"""
    out = []
    for a in ATLASES_ROWS:
        out.append((f"blur_r8-{a}", lambda a=a: _blur("r8", a), ("blur_v", "blur_h")))
        out.append((f"blur_rgba8-{a}", lambda a=a: _blur("rgba8", a), ("blur_v", "blur_h")))
        out.append((f"clip_masks-{a}", lambda a=a: scenes.clip_masks(n=8, atlas=a, seed=34, pin_corner=True), ("clip_masks",)))
    for a in ATLASES:
        out.append((f"box_shadow_masks-{a}", lambda a=a: scenes.box_shadow_masks(n=3 if a < 512 else 5, atlas=a, seed=49, pin_corner=True), ("box_shadow_masks",)))
        out.append((f"border_solid-{a}", lambda a=a: scenes.border_solid(n=12, seed=134, atlas=a, pin_corner=True), ("border_cache",)))
        out.append((f"border_segments-{a}", lambda a=a: scenes.border_segments(n=20, seed=143, atlas=a, pin_corner=True), ("border_cache",)))
        out.append((f"cache_decorations-{a}", lambda a=a: scenes.cache_decorations(n_lines=20, n_grads=10, n_lgrads=10, n_rgrads=6, n_cgrads=6, seed=154, atlas=a,
                                                                                   pin_corner=True), ("decoration_cache",)))
        out.append((f"texture_cache_copies-{a}", lambda a=a: scenes.texture_cache_copies(n=30, seed=194, src_size=a, dst_size=a + 184, pin_corner=True),
                    ("copy_dst_rgba", "copy_dst_r8", "copy_dst2_rgba", "copy_dst2_r8")))
    return out


def touches_edges(px, background):
    """Does this read-back target differ from `background` somewhere in its last column, and somewhere in its last row?"""
    d = px != background
    if d.ndim == 3:
        d = d.any(axis=2)
    return bool(d[:, -1].any()), bool(d[-1, :].any())
