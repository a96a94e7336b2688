"""Transform classes the scene builders never draw (test infrastructure, not collected by pytest): `retransform(frame, cls)` rewrites
the transform blocks -- or the render tasks' device pixel scale -- of an already built frame in place, so that the parity scenes
are also rasterised mirrored (determinant < 0), under exact quarter / half turns and axis flips (matrices of 0 and +-1), under
scales other than 1, smaller than a pixel, larger than the target, beyond 32-bit integers, under singular transforms, and at
device pixel scales of 1.5 and 0.77.  webrender_amd/scenes.py is untouched: every golden digest of the existing scenes holds.

Transform k is rows 8k .. 8k+3 (m.T) and 8k+4 .. 8k+7 (inv(m).T) of frame.transforms.data; k = 0 is the identity and stays.
An affine m is taken apart into its linear part A and the fixed point c of the builders' "rotation about the prim's own centre"
((A - I) c = -t), and T(c) . L . T(-c) is stored with its float64 inverse cast to float32; L depends on k, so one scene carries
every member of a class.

`reedge(frame)` (the `*_edges` classes) also gives every transformed prim a subset of its anti-aliased edges: the builders always ask
for all four, and then no mirror shows which screen edge an `aa_edges` bit belongs to.

Tile assignment stays that of the unrewritten scene: a prim that a rewritten transform moves or grows into a tile it was not
listed for is not drawn there, and one that leaves its tiles is clipped away.  Both backends receive the same instance lists, so
parity is unaffected -- the scenes are no longer what a display list would produce, the comparison is what it was."""
import numpy as np
from webrender_amd import scenes

_T = np.array
# the exact maps: entries of 0 and +-1 (a random angle never lands on them; cos(pi / 2) in float64 is 6e-17, not 0)
EXACT = [("flip x", _T([[-1.0, 0.0], [0.0, 1.0]])), ("flip y", _T([[1.0, 0.0], [0.0, -1.0]])), ("half turn", _T([[-1.0, 0.0], [0.0, -1.0]])),
         ("quarter turn", _T([[0.0, -1.0], [1.0, 0.0]])), ("quarter turn back", _T([[0.0, 1.0], [-1.0, 0.0]])),
         ("transpose", _T([[0.0, 1.0], [1.0, 0.0]]))]
AFFINE_SCALES = [(0.37, 1.9), (2.3, 0.6), (-0.37, 1.9), (0.5, -0.5)]
# affine: eight members by k % 8 -- the builder's own map mirrored, the six exact maps, the builder's map scaled (the four scales in turn, by k // 8)
AFFINE = ["A.diag(-1, 1)"] + [n for n, _ in EXACT] + ["A.diag(s)"]
# degenerate: twelve members by k % 12, the four groups interleaved so that neighbours in the cycle draw where a member draws nothing
DEGENERATE = [("tiny", (0.004, 0.004)), ("large", (300.0, 300.0)), ("beyond int", (1e8, 1e8)), ("singular", (0.0, 1.0)),
              ("tiny", (0.02, 1.0)), ("large", (1000.0, 0.5)), ("beyond int", (3e9, 0.5)), ("singular", (1.0, 0.0)),
              ("tiny", (1.0, 0.003)), ("large", (1e4, 1e4)), ("beyond int", (3e7, 3e7)), ("singular", (1e-30, 1.0))]
CLASSES = ("affine", "degenerate", "screen_mirror", "dps1.5", "dps0.77", "affine_edges", "screen_mirror_edges")
MIXED = ("affine", "degenerate", "affine_edges")


def member(cls, k):
    """what transform k of a frame rewritten with a mixed class is: 'k % len(cycle): description'"""
    if cls.startswith("affine"):
        s = f" s = {AFFINE_SCALES[(k // 8) % 4]}" if k % 8 == 7 else ""
        e = f", aa edges {edge_subset(k):#x}" if cls == "affine_edges" else ""
        return f"member {k % 8}: {AFFINE[k % 8]}{s}{e}"
    group, s = DEGENERATE[k % 12]
    return f"member {k % 12}: {group}, A.diag{s}"


def _linear(cls, k, a):
    if cls == "affine":
        j = k % 8
        if j == 0:
            return a @ np.diag([-1.0, 1.0])
        if j <= 6:
            return EXACT[j - 1][1]
        return a @ np.diag(AFFINE_SCALES[(k // 8) % 4])
    return a @ np.diag(DEGENERATE[k % 12][1])


def edge_subset(k):
    """the anti-aliased edges (1 .. 14: never none, never all four) of the prims under transform k: five different subsets for
    every member of the affine cycle among the first forty transforms"""
    return (5 * (k // 8) + 3 * (k % 8)) % 14 + 1


def reedge(frame):
    """Every builder asks for all four anti-aliased edges (edge flags 15) on a transformed prim, so which screen edge an `aa_edges`
    bit lands on never shows.  Rewrites the flags of such brush_* and ps_quad_* instances to edge_subset(transform index); returns
    the number of instances rewritten."""
    hi, bi = frame.prim_headers_i.data, frame.gpu_buffer_i.data
    done = 0
    for targets in frame.passes:
        for tg in targets:
            for step in list(tg.opaque) + list(tg.alpha) + list(tg.steps):
                quad = step.shader.startswith("ps_quad")
                if step.desc != "PRIM_INSTANCES" or not (quad or step.shader.startswith("brush_")):
                    continue
                shift = 16 if quad else 28
                inst = step.instances
                for r in range(len(inst)):
                    k = (int(bi[inst[r, 0], 0]) if quad else int(hi[2 * inst[r, 0], 2])) & 0x3FFFFF
                    word = int(np.uint32(inst[r, 2]))
                    if k == 0 or (word >> shift) & 15 != 15:
                        continue
                    word = (word & ~(15 << shift)) | (edge_subset(k) << shift)
                    inst[r, 2] = np.int32(np.uint32(word))
                    done += 1
    return done


def _store(d, k, m):
    with np.errstate(all="ignore"):
        try:
            inv = np.linalg.inv(m)
        except np.linalg.LinAlgError:
            inv = np.zeros((4, 4))
        d[8 * k:8 * k + 4] = m.T.astype(np.float32)
        d[8 * k + 4:8 * k + 8] = inv.T.astype(np.float32)


def retransform(frame, cls):
    """Rewrite `frame` in place for `cls` (one of CLASSES); returns the number of transforms / render tasks rewritten."""
    assert cls in CLASSES, cls
    done = 0
    if cls.endswith("_edges"):
        return retransform(frame, cls[:-6]) if reedge(frame) else 0
    if cls.startswith("dps"):
        rt = frame.render_tasks.data
        for k in range(frame.render_tasks.len // 2):
            if rt[2 * k + 1, 0] == 1.0:
                rt[2 * k + 1, 0] = float(cls[3:])
                done += 1
        return done
    d = frame.transforms.data
    for k in range(1, frame.transforms.len // 8):
        m = d[8 * k:8 * k + 4].T.astype(np.float64)
        if cls == "screen_mirror":      # the whole scene mirrored on screen: S . m, S = T(width) . diag(-1, 1) -- projective transforms as well
            s = np.eye(4)
            s[0, 0], s[0, 3] = -1.0, float(frame.width)
            _store(d, k, s @ m)
            done += 1
            continue
        if not np.array_equal(m[2:], np.eye(4)[2:]) or m[0, 2] or m[1, 2]:      # (projective, or not a 2-D map: left alone)
            continue
        a, t = m[:2, :2], m[:2, 3]
        try:
            c = np.linalg.solve(a - np.eye(2), -t)
        except np.linalg.LinAlgError:
            continue
        lin = _linear(cls, k, a)
        m2 = np.eye(4)
        m2[:2, :2] = lin
        m2[:2, 3] = c - lin @ c
        _store(d, k, m2)
        done += 1
    return done


def prim_boxes(frame):
    """[(transform index k, (x0, y0, x1, y1) in window pixels, y down)] of the picture tiles' prims under a transform k > 0, in draw
    order per tile: the local rect's corners through the stored matrix.  A box that is not finite covers the window.  (Picture
    tasks at device pixel scale 1 whose content origin is the tile's place in the window -- what every builder here makes.)"""
    out = []
    hf, hi = frame.prim_headers_f.data, frame.prim_headers_i.data
    bf, bi = frame.gpu_buffer_f.data, frame.gpu_buffer_i.data
    tr = frame.transforms.data
    for targets in frame.passes:
        for tg in targets:
            if tg.kind != "picture_tile":
                continue
            for step in list(tg.opaque) + list(tg.alpha):
                if step.desc != "PRIM_INSTANCES":
                    continue
                for inst in np.asarray(step.instances).reshape(-1, 4):
                    if step.shader.startswith("ps_quad"):
                        k, rect = int(bi[inst[0], 0]), bf[inst[1]]
                    else:
                        k, rect = int(hi[2 * inst[0], 2]), hf[2 * inst[0]]
                    k &= 0x3FFFFF
                    if k == 0 or 8 * k + 4 > len(tr):
                        continue
                    m = tr[8 * k:8 * k + 4].T.astype(np.float64)
                    x0, y0, x1, y1 = [float(v) for v in rect]
                    with np.errstate(all="ignore"):
                        p = m @ np.array([[x0, x1, x1, x0], [y0, y0, y1, y1], [0.0] * 4, [1.0] * 4])
                        q = p[:2] / p[3]
                    if np.isfinite(q).all() and (p[3] > 0).all():
                        box = (q[0].min(), q[1].min(), q[0].max(), q[1].max())
                    else:
                        box = (0.0, 0.0, float(frame.width), float(frame.height))
                    out.append((k, box))
    return out


def first_member_at(frame, cls, diff):
    """`diff`: bool [H, W] of differing pixels as read_pixels returns them (bottom row first).  The member of the first prim
    whose bounding box (grown by a pixel) holds one, or None."""
    ys, xs = np.nonzero(diff)
    if not len(ys):
        return None
    ys = diff.shape[0] - 1 - ys
    for k, (x0, y0, x1, y1) in prim_boxes(frame):
        if ((xs >= x0 - 1) & (xs <= x1 + 1) & (ys >= y0 - 1) & (ys <= y1 + 1)).any():
            return f"transform {k}, {member(cls, k)}"
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# (name, make, classes): the rotated builders at the small sizes of the parity cases, one scene per family
_EXACT_OPS = [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]
_TEXT = dict(width=1024, height=512, lines=20, glyphs_per_line=60, run_len=12)
_ROT = ("affine", "degenerate", "dps1.5", "dps0.77")
CASES = [
    ("rects", lambda: scenes.rotated_rects(n=40), _ROT),
    ("rects_quad", lambda: scenes.rotated_rects(n=40, encoding="quad"), _ROT),
    ("rects_depth_writers", lambda: scenes.rotated_rects(n=40, opaque_frac=0.5, seed=96), _ROT),
    ("images", lambda: scenes.rotated_images(n=40), _ROT),
    ("images_quad", lambda: scenes.rotated_images(n=40, encoding="quad"), _ROT),
    ("images_repeat", lambda: scenes.rotated_images(n=24, repeat=True), _ROT),
    ("images_masked", lambda: scenes.rotated_images(n=40, masked=True), _ROT),
    ("images_repeat_dual", lambda: scenes.rotated_images(n=40, repeat=True, dual=True, seed=105), _ROT),
    ("gradients", lambda: scenes.gradient_grid(rotate=True, n=40, seed=66), _ROT),
    ("filters", lambda: scenes.filter_grid(rotate=True, n=44, seed=76, ops=_EXACT_OPS), _ROT),
    ("opacity", lambda: scenes.filter_grid(rotate=True, n=40, shader="opacity", seed=78), _ROT),
    ("quad_masks", lambda: scenes.quad_masks(rotate=True, n=40, seed=86), _ROT),
    ("masked_rects", lambda: scenes.masked_rects(rotate=True, force_aa=True, fractional=True, n=80, seed=14), _ROT),
    ("image_masks", lambda: scenes.image_masks(rotate=True, n=40), _ROT),
    ("quad_gradients", lambda: scenes.quad_gradients(rotate=True, n=24, seed=182), _ROT),
    ("mix_blend", lambda: scenes.mix_blend_grid(rotate=True, n=40, seed=208), _ROT),
    ("yuv", lambda: scenes.yuv_grid(rotate=True, n=40, seed=410), _ROT),
    ("split_composites", lambda: scenes.split_composites(n=40), _ROT),
    ("text", lambda: scenes.cfg3_text(rotate=True, **_TEXT), _ROT),
]
# ... and the projective variants of the same builders that sit in parity_cases.ROTATED, mirrored on screen: reversed winding
# through draw_perspective and, where prims reach the camera plane, clip_side
PROJECTIVE = ("perspective_rects", "perspective_rects_quad", "near_clipped_rects", "near_clipped_depth_writers", "perspective_images",
              "near_clipped_images_quad", "near_clipped_images_repeat", "perspective_filters_exact", "perspective_opacity",
              "perspective_gradients", "perspective_quad_masks", "perspective_masked_rects", "perspective_quad_gradients",
              "perspective_text")


def _cases():
    from parity_cases import ROTATED
    rotated = dict(ROTATED)
    return CASES + [(n, rotated[n], ("screen_mirror",)) for n in PROJECTIVE]


# the same with a subset of the anti-aliased edges per prim (reedge): the families whose prims ask for swgl_antiAlias in the alpha pass
EDGES = ("rects", "rects_quad", "masked_rects", "images", "images_quad", "gradients", "quad_masks")
EDGES_PROJECTIVE = ("perspective_rects_quad", "near_clipped_rects", "near_clipped_images_quad")


def _all():
    cases = _cases()
    out = [(f"{name}-{cls}", name, make, cls) for name, make, classes in cases for cls in classes]
    by_name = {name: make for name, make, _ in cases}
    out += [(f"{name}-affine_edges", name, by_name[name], "affine_edges") for name in EDGES]
    out += [(f"{name}-screen_mirror_edges", name, by_name[name], "screen_mirror_edges") for name in EDGES_PROJECTIVE]
    return out


ALL = _all()
# the one family whose float functions come from the device's math library there (sqrt / division of the non-separable modes,
# tests/test_gpu_parity.py::test_hip_mix_blend_matches_oracle): <= 1 LSB on <= 1e-4 of the bytes on the device, and only there
DEVICE_ONE_LSB = ("mix_blend",)
