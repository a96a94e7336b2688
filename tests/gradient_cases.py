"""Case tables for the gradient shaders -- brush_linear_gradient (both passes), cs_fast_linear_gradient, cs_linear_gradient,
cs_radial_gradient, cs_conic_gradient, ps_quad_radial_gradient, ps_quad_conic_gradient -- over constructed stop tables and geometry,
and the builders that pack a family's cases into frames (tests/test_gradient_sweep.py compares the backends;
tests/golden/make_gradient_sweep.py records the oracle's digests).

Every table is a pure function of SEED.  A case is a small dict: one prim (or one cache task) in a cell of its own -- its size,
the fraction of a pixel its origin sits at, its stop table and where that lies in the 1024-wide buffer, the family's geometry
parameters --, `classes` (labels computed from the parameters alone, counted below at import) and `tag` (one line a failure
message prints).  Cases are packed many to a frame, 2 px apart; a differing pixel is mapped back to its cell.

Frames.  The cs_* tasks go on shelves of a 1024-wide cache target that is read back.  Brush and quad prims go in disjoint cells
of 1024 x 512 picture tiles, in three frames per family: "dense" (more prims per tile than wr_tile_rows_kernel takes, 128: the
bin raster), "rows" (few prims per tile, the long spans among them: brush_linear_gradient tiles take the row kernel there and are
drawn a second time through the bins; the quad pattern shaders are never eligible for the row kernel, their "rows" frame is one
more bin-raster frame) and "slivers" (behind opaque slivers, scenes.add_slivers: the span shader restarts inside the span).

What the cases stay inside: colours in [0, 1] and finite; no transforms (tests/test_transform_classes.py).  Raw tables keep
alpha at exactly 1 with a zero step, so a premultiplied colour never exceeds its alpha.

On the device cs_conic_gradient alone is not compared at 0 bytes (its angle is the device's atan2f): see
CONIC_DIFF_SHARE for the measured share of bytes that differ by 1, and device_runs() for the tables it leaves to the host side."""
import hashlib
import math
import zlib
import numpy as np
from webrender_amd import glconst as G
from webrender_amd import scenes as S
from webrender_amd.frame import Frame, Target, Step, TextureRef, CompositeTile, CLIP_TASK_EMPTY, TEX_W

SEED = 0x6AD5EED
MIN_PER_CLASS = 8
NOOP_CAP = 0.20          # share of a family's cases whose cell may hold a single colour on the oracle
GAP = 2
TILE_W, TILE_H = 1024, 512
ROWS_MAX_PER_TILE = 100      # "rows" frames: well under the 128 prims a tile-rows target may hold
DENSE_MIN_PER_TILE = 129     # "dense" frames: above it
SLIVER_PITCH = 40            # 26 slivers per tile row: inside what the depth-run tables hold (pitch 9 overflows them: parity_cases.TILE_ROWS)
FAMILIES = ("brush_linear_gradient", "cs_fast_linear_gradient", "cs_linear_gradient", "cs_radial_gradient", "cs_conic_gradient",
            "ps_quad_radial_gradient", "ps_quad_conic_gradient")
CS = ("cs_fast_linear_gradient", "cs_linear_gradient", "cs_radial_gradient", "cs_conic_gradient")
# cs_conic_gradient on the device: bytes that may differ from the oracle by 1 (never more), as a share of the bytes of the compared
# cells.  MEASURED on the MI355X against the oracle (tests/test_gradient_sweep.py prints it); allowed: twice the measured share
# (the margin tests/test_clang_budget.py's CLANG_BUDGET gives a family).
CONIC_DIFF_SHARE = 2 * 6 / 524416      # measured: 6 of the 524416 bytes of the 164 compared cells (1.14e-05), each by 1

f32 = np.float32
WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9)
LONG_WIDTHS = (260, 516, 1020)
ORIGINS = (0.0, 0.41, 0.5)
BREAKS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)
EVENS = (3, 9, 17, 33, 65, 129)
PLACES = ("col0", "col764", "straddle", "last_row")


# ---- stop tables ---------------------------------------------------------------------------------------------------------------
def _trng(name, variant):
    return np.random.default_rng([SEED, 7, zlib.crc32(name.encode()), variant])


def _cols(rng, n, variant):
    """n straight-alpha colours; variant 0: alpha 1 everywhere (usable in the opaque pass), else mixed"""
    return [tuple(float(v) for v in rng.uniform(0.0, 1.0, size=3)) + ((1.0,) if variant == 0 else (float(rng.choice([1.0, 0.7, 0.35])),))
            for _ in range(n)]


def _raw_break(k, variant, rng):
    """130 x (start, step) written directly: two linear pieces over entries 1 .. k and k + 1 .. 128 whose steps differ.
    variant 0: entries 0 and 129 are the constant ends a built table has (merge bits 0, k and 128 are clear);
    variant 1: entry 0 carries the first piece's step and entry 129 the second's, so bit k is the ONLY clear bit."""
    t = np.zeros((130, 2, 4), np.float64)
    for ch in range(3):
        while True:
            v0, vj, v1 = (float(v) for v in rng.uniform(0.1, 0.9, size=3))
            sa = (vj - v0) / k
            sb = (v1 - vj) / (128 - k) if k < 128 else -sa / 2
            if abs(sa - sb) > 1e-4:
                break
        for i in range(1, 129):
            t[i, 0, ch] = v0 + sa * (i - 1) if i <= k else vj + sb * (i - k - 1)
            t[i, 1, ch] = sa if i <= k else sb
        t[0, 0, ch], t[129, 0, ch] = v0, v1
        if variant:
            t[0, 1, ch] = sa
            t[129, 0, ch], t[129, 1, ch] = v1 - sb, sb
    t[:, 0, 3] = 1.0
    return t.astype(f32).reshape(-1, 4)


def make_table(name, variant):
    """the (260, 4) float32 table of class `name`"""
    rng = _trng(name, variant)
    lut = S.build_gradient_lut
    if name == "two_stop":
        c = _cols(rng, 2, variant)
        return lut([(0.0, c[0]), (1.0, c[1])])
    if name.startswith("even_"):
        n = int(name.split("_")[1])
        offs = [i / (n - 1) for i in range(n)]
        if name.endswith("_hard"):
            offs[n // 2 + 1] = offs[n // 2]
        return lut(list(zip(offs, _cols(rng, n, variant))))
    if name.startswith("break_at_"):
        return _raw_break(int(name.split("_")[2]), variant, rng)
    if name == "hard_at_0":
        c = _cols(rng, 3, variant)
        return lut([(0.0, c[0]), (0.0, c[1]), (1.0, c[2])])
    if name == "hard_at_1":
        c = _cols(rng, 3, variant)
        return lut([(0.0, c[0]), (1.0, c[1]), (1.0, c[2])])
    if name == "hard_on_entry":
        c, k = _cols(rng, 4, variant), (40, 64)[variant]
        return lut([(0.0, c[0]), (k / 128.0, c[1]), (k / 128.0, c[2]), (1.0, c[3])])
    if name == "two_in_one_entry":
        c, o = _cols(rng, 4, variant), (0.5, 0.25)[variant]
        return lut([(0.0, c[0]), (o + 0.0005, c[1]), (o + 0.0025, c[2]), (1.0, c[3])])
    if name == "constant_builder":
        c = _cols(rng, 1, variant)[0]
        return lut([(0.0, c), (1.0, c)])
    if name == "constant_raw":
        a = (1.0, 0.6)[variant]
        t = np.zeros((130, 2, 4), f32)
        t[:, 0, :3] = [float(v) * a for v in rng.uniform(0.0, 1.0, size=3)]
        t[:, 0, 3] = a
        return t.reshape(-1, 4)
    if name == "alpha0_stops":
        c = _cols(rng, 5, 0)
        for i in ((1, 3), (0, 2, 4))[variant]:
            c[i] = c[i][:3] + (0.0,)
        return lut([(i / 4.0, c[i]) for i in range(5)])
    if name == "reversed":
        c = _cols(rng, 4, variant)
        return lut([(0.0, c[0]), (0.3, c[1]), (0.55, c[2]), (1.0, c[3])], reverse=True)
    raise KeyError(name)


HARD_TABLES = ("hard_at_0", "hard_at_1", "hard_on_entry", "even_9_hard") + tuple(f"break_at_{k}" for k in BREAKS)
TABLE_CLASSES = (("two_stop",) + tuple(f"even_{n}" for n in EVENS) + tuple(f"break_at_{k}" for k in BREAKS) +
                 ("hard_at_0", "hard_at_1", "hard_on_entry", "two_in_one_entry", "constant_builder", "constant_raw", "alpha0_stops", "reversed"))
FIXED_TABLES = ("two_stop", "even_9_hard", "break_at_32", "even_129")
_tables = {}


def table(name, variant):
    if (name, variant) not in _tables:
        t = make_table(name, variant)
        assert t.shape == (260, 4) and t.dtype == f32 and np.isfinite(t).all()
        e = t.reshape(130, 2, 4)
        # (inside [0, 1] up to the few ulp the builder's running sums drift by, as GradientGpuBlockBuilder's do)
        assert min(e[:, 0].min(), (e[:, 0] + e[:, 1]).min()) >= -1e-5 and max(e[:, 0].max(), (e[:, 0] + e[:, 1]).max()) <= 1.0 + 1e-5, name
        _tables[(name, variant)] = t
    return _tables[(name, variant)]


def table_opaque(name, variant):
    return variant == 0 or name.startswith("break_at_")


def merge_bits(t):
    """bit j: entries j and j + 1 of the table carry the same step (GradientStops::can_merge)"""
    e = t.reshape(130, 2, 4)
    return [bool((e[j, 1].view(np.uint32) == e[j + 1, 1].view(np.uint32)).all()) for j in range(129)]


# what the table classes promise, checked where it can be: the break sits exactly there, and no two entries of even_129 merge
for _k in BREAKS:
    _m = merge_bits(make_table(f"break_at_{_k}", 1))
    assert [j for j in range(129) if not _m[j]] == [_k], _k
    _m = merge_bits(make_table(f"break_at_{_k}", 0))
    assert sorted(set([j for j in range(129) if not _m[j]])) == sorted({0, _k, 128}), _k
assert not any(merge_bits(make_table("even_129", 0))) and not any(merge_bits(make_table("even_129", 1)))
assert all(merge_bits(make_table("constant_raw", 0)))


class Tables:
    """the stop tables of one frame in its sGpuBufferF store: one copy per (name, variant, place)"""

    def __init__(self, store):
        self.store, self.addr, self.late = store, {}, {}

    def _skip_to(self, col):
        s = self.store
        cur = s.len % TEX_W
        s.len += (col - cur) if cur <= col else (TEX_W - cur + col)

    def get(self, name, variant, place):
        """the table's address (any place but "last_row": later())"""
        key = (name, variant, place)
        if key not in self.addr:
            s, t = self.store, table(name, variant)
            if place == "any":
                self.addr[key] = s.push(t)
            else:
                self._skip_to({"col0": 0, "col764": 764, "straddle": 766}[place])
                a = s.len
                s.len += 260                              # (straddle: runs on into the next row, which is thereby allocated)
                while s.len > len(s.data):
                    s.data = np.concatenate([s.data, np.zeros_like(s.data)])
                s.data[a:a + 260] = t
                self.addr[key] = a
        return self.addr[key]

    def later(self, name, variant, fix):
        """place "last_row": the address is not known yet -- `fix(address)` is called from finish()"""
        self.late.setdefault((name, variant), []).append(fix)

    def of(self, case, fix):
        if case["place"] == "last_row":
            self.later(*case["table"], fix)
            return 0
        return self.get(*case["table"], case["place"])

    def finish(self):
        """after everything else has been pushed: the last_row tables, at the start of a fresh row that is then the buffer's last"""
        if self.late:
            assert len(self.late) * 260 <= TEX_W
            self._skip_to(0)
            for (name, variant), fixes in self.late.items():
                a = self.store.push(table(name, variant))
                for fix in fixes:
                    fix(a)
            assert (self.store.len - 1) // TEX_W == a // TEX_W == self.store.rows() - 1


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def _first_pixel(fx):
    """the first pixel a prim covers whose origin sits at fraction fx of a pixel: a centre exactly on the left / top edge is outside"""
    return 0 if fx < 0.5 else 1


def _first_centre(fx):
    """local x of the first covered pixel centre"""
    return _first_pixel(fx) + 0.5 - fx


def _first_centre_y(c):
    """(cache targets are drawn bottom-up: whether a centre exactly on a task's top edge is inside depends on the rounding of the
    flipped edge -- at origin .5 the labels place the first row as the picture tiles have it, half a pixel at most from where it is)"""
    return _first_centre(c["fx"])


def _table_classes(c):
    if c["table"] is None:
        return []
    name = c["table"][0]
    k = [name]
    if name.startswith("break_at_"): k.append("break_at_k")
    if name.startswith("even_") and not name.endswith("_hard"): k.append("even_N")
    if c["place"] != "any": k.append("place_" + c["place"])
    return k


def _common_classes(c):
    k = _table_classes(c)
    k.append(f"w{c['w']}")
    if c["w"] in LONG_WIDTHS: k.append("long_span")
    k.append("x" + {0.0: ".0", 0.41: ".41", 0.5: ".5"}[c["fx"]])
    k.append({"dense": "bins", "rows": "few_prims", "slivers": "depth_runs", "atlas": "atlas"}[c["frame"]])
    g = c["g"]
    if "extend" in g: k.append("repeat" if g["extend"] else "clamp")
    if c["w"] < 4: k.append("span_lt_4")
    elif c["w"] % 4: k.append(f"tail_{c['w'] % 4}")
    return k


def _lin_offset(c, x, y):
    (sx, sy), (ex, ey) = c["g"]["start"], c["g"]["end"]
    dx, dy = ex - sx, ey - sy
    return ((x - sx) * dx + (y - sy) * dy) / (dx * dx + dy * dy)


def linear_classes(c):
    g = c["g"]
    (sx, sy), (ex, ey) = g["start"], g["end"]
    dx, dy = ex - sx, ey - sy
    k = _common_classes(c)
    if g.get("pass"): k.append(g["pass"] + "_pass")
    st = g.get("stretch")
    if st:
        tx, ty = st[0] != c["w"], st[1] != c["h"]
        k += ["tile_repeat", "tile_" + ("xy" if tx and ty else "x" if tx else "y"), "stretch_" + g["stretch_name"]]
    if dx == 0 and dy == 0:
        return tuple(k + ["delta_nonfinite"])
    k.append("delta_pos" if dx > 0 else "delta_neg" if dx < 0 else "delta_zero")
    length = math.hypot(dx, dy)
    if dy == 0 and abs(dx) == 512: k.append("one_entry_per_chunk")
    if length >= 1e5: k.append("tiny_delta")
    if length <= 0.25: k.append("huge_delta")
    if st:
        return tuple(k)
    x0, y0 = _first_centre(c["fx"]), _first_centre_y(c)
    x1, y1 = x0 + c["w"] - 1, y0 + c["h"] - 1
    corners = [_lin_offset(c, x, y) for x in (x0, x1) for y in (y0, y1)]
    lo, hi = min(corners), max(corners)
    if not g["extend"]:
        if hi < 0: k.append("below_0")
        if lo >= 1: k.append("above_1")
    run = 0.0
    for y in (y0, y1):
        a, b = _lin_offset(c, x0, y), _lin_offset(c, x1, y)
        if min(a, b) < 0 < max(a, b): k.append("cross_0")
        if min(a, b) < 1 < max(a, b): k.append("cross_1")
        if a != b:      # pixels of the row whose offset lies in [0, 1): one merged range under a two-stop table
            ta, tb = sorted((x0 + (0 - a) * (x1 - x0) / (b - a), x0 + (1 - a) * (x1 - x0) / (b - a)))
            run = max(run, min(tb, x1 + 1) - max(ta, x0))
    if g["extend"] and min(abs(lo), abs(hi)) > 40: k.append("far_repeat")
    if c["table"] and c["table"][0] == "two_stop" and not g["extend"]:
        if run > 4 * 64: k.append("seg_ge_1")
        if run > 4 * 128: k.append("seg_ge_2")
    return tuple(dict.fromkeys(k))


def radial_classes(c):
    g = c["g"]
    k = _common_classes(c)
    cx, cy = g["center"]
    x0, y0 = _first_centre(c["fx"]), _first_centre_y(c)
    x1, y1 = x0 + c["w"] - 1, y0 + c["h"] - 1
    in_rows = y0 <= cy <= y1
    if x0 <= cx <= x1 and in_rows: k.append("centre_inside")
    if cx < x0: k.append("centre_left")
    if cx > x1: k.append("centre_right")
    if c["fx"] == 0.0 and cx % 1 == 0.5 and cy % 1 == 0.5 and x0 <= cx <= x1 and in_rows: k.append("centre_on_pixel_centre")
    if c["fx"] == 0.0 and cx % 1 == 0.0 and cy % 1 == 0.0: k.append("centre_on_pixel_corner")
    r0, r1 = g["r0"], g["r1"]
    if r0 == 0: k.append("r0_zero")
    if r0 == r1: k.append("r0_eq_r1")
    if r0 > r1: k.append("r0_gt_r1")
    if r1 - r0 == 0.5: k.append("range_half_px")
    if r1 - r0 == 1e4: k.append("range_1e4")
    if 0 < r0 < r1 and x0 <= cx - r0 and cx + r0 <= x1 and in_rows: k.append("inner_disc_inside_span")
    k.append(f"ratio_{g['ratio']:g}")
    if c["family"] in CS: k.append(f"scale_{g['scale']:g}")
    return tuple(dict.fromkeys(k))


def conic_classes(c):
    g = c["g"]
    k = _common_classes(c)
    cx, cy = g["center"]
    x0, y0 = _first_centre(c["fx"]), _first_centre_y(c)
    x1, y1 = x0 + c["w"] - 1, y0 + c["h"] - 1
    inside = x0 <= cx <= x1 and y0 <= cy <= y1
    if c["fx"] == 0.0 and inside and cx % 1 == 0.5 and cy % 1 == 0.5: k.append("centre_on_pixel_centre")
    if c["fx"] == 0.0 and inside and cx % 1 == 0.0 and cy % 1 == 0.0: k.append("centre_on_pixel_corner")
    if not (x0 - 0.5 <= cx <= x1 + 0.5 and y0 - 0.5 <= cy <= y1 + 0.5): k.append("centre_outside")
    k.append("angle_" + g["angle_name"])
    s0, s1 = g["s0"], g["s1"]
    k.append("offsets_0_1" if (s0, s1) == (0.0, 1.0) else "offsets_equal" if s0 == s1 else "offsets_reversed" if s0 > s1 else
             "offsets_quarter" if (s0, s1) == (0.25, 0.75) else "offsets_other")
    return tuple(dict.fromkeys(k))


def fast_classes(c):
    g = c["g"]
    k = _common_classes(c)
    k.append("axis_y" if g["axis"] else "axis_x")
    k.append(g["colours"])
    return tuple(k)


def _fmt(v):
    if isinstance(v, (tuple, list)):
        return "(" + ",".join(_fmt(x) for x in v) + ")"
    return f"{v:g}" if isinstance(v, float) else str(v)


class _Family:
    def __init__(self, family, classes_of):
        self.family, self.classes_of, self.cases = family, classes_of, []
        self.cs = family in CS

    def add(self, frame, w, h, fx, tab, place, g):
        c = {"family": self.family, "index": len(self.cases), "frame": "atlas" if self.cs else frame, "w": int(w), "h": int(h), "fx": float(fx),
             "table": tab, "place": place, "g": g}
        c["classes"] = self.classes_of(c)
        tname = "-" if tab is None else f"{tab[0]}/{tab[1]}" + ("" if place == "any" else "@" + place)
        c["tag"] = (f"{self.family}[{c['index']}] {c['frame']} {w}x{h}+{fx:g} table {tname} " +
                    " ".join(f"{k}={_fmt(v)}" for k, v in g.items()) + " " + "/".join(c["classes"]))
        self.cases.append(c)
        return c

    def crossed(self, fixed, variants, long_variants=None):
        """`fixed`: the four fixed geometries; `variants`: [(a, b)] geometry dicts (with "w", "h", "fx") per geometry class.
        Every table class under the fixed geometries (bins); the placements under two fixed tables; every geometry class under the
        four fixed tables, variant a in the dense frame and b in the few-prims one; the fixed geometries under the fixed tables
        behind slivers."""
        def put(frame, geo, tab, place="any"):
            g = {k: v for k, v in geo.items() if k not in ("w", "h", "fx")}
            if "pass" in g:
                g["pass"] = "opaque" if (table_opaque(*tab) and len(self.cases) % 2 == 0) else "alpha"
            return self.add(frame, geo["w"], geo["h"], geo["fx"], tab, place, g)
        for name in TABLE_CLASSES:
            for v in (0, 1):
                for geo in fixed:
                    put("dense", geo, (name, v))
        for place in PLACES:
            for name in FIXED_TABLES[:2]:
                for geo in fixed:
                    put("dense", geo, (name, 0), place)
        for a, b in variants:
            for name in FIXED_TABLES:
                put("dense", a, (name, 0))
                put("rows", b, (name, 1))
        for geo in long_variants or []:
            for v in (0, 1):
                put("rows", geo, ("two_stop", v))
        if not self.cs:
            for name in FIXED_TABLES:
                for geo in fixed:
                    put("slivers", geo, (name, 0))


def _geo(w, h, fx, **g):
    return dict(w=w, h=h, fx=fx, **g)


def _linear_family(family):
    brush = family == "brush_linear_gradient"
    F = _Family(family, linear_classes)
    extra = {"pass": "?"} if brush else {}

    def L(w, h, fx, start, end, extend, **kw):
        return _geo(w, h, fx, start=(float(start[0]), float(start[1])), end=(float(end[0]), float(end[1])), extend=extend, **extra, **kw)
    fixed = [L(64, 6, 0.0, (0, 0), (64, 0), 0), L(64, 6, 0.41, (48, 5), (16, 1), 0), L(64, 6, 0.5, (3, 0), (27, 10), 1),
             L(61, 6, 0.0, (-20, -4), (90, 9), 0)]
    V = []
    # span widths: a diagonal line across the cell (a 1-px column still changes from row to row), both directions, origins in turn
    for i, w in enumerate(WIDTHS):
        V.append((L(w, 5, ORIGINS[i % 3], (-1.5, -1.0), (w + 2.0, 8.0), 0), L(w, 5, ORIGINS[(i + 1) % 3], (w + 2.0, 8.0), (-1.5, -1.0), i % 2)))
    # delta
    V += [(L(64, 6, 0.0, (5, 0), (50, 0), 0), L(64, 6, 0.41, (0, 2), (40, 8), 1)),
          (L(64, 6, 0.41, (50, 0), (5, 0), 0), L(64, 6, 0.5, (40, 8), (0, 2), 1)),
          (L(64, 6, 0.0, (0, 0), (0, 6), 0), L(64, 6, 0.41, (0, 1), (0, 4), 1)),
          (L(64, 6, 0.0, (32, 3), (32, 3), 0), L(64, 6, 0.5, (0, 0), (0, 0), 1)),
          (L(64, 6, 0.41, (-100, 0), (412, 0), 0), L(64, 6, 0.0, (300, 0), (-212, 0), 1)),
          (L(64, 6, 0.0, (-5e4, 0), (5e4, 0), 0), L(64, 6, 0.41, (0, 0), (1e5, 0), 1)),
          (L(64, 6, 0.0, (20, 0), (20.25, 0), 0), L(64, 6, 0.41, (10.1, 0), (10.35, 0), 1))]
    # offsets
    V += [(L(64, 6, 0.0, (80, 0), (150, 0), 0), L(64, 6, 0.41, (-10, 0), (-40, 0), 0)),
          (L(64, 6, 0.41, (-40, 0), (-10, 0), 0), L(64, 6, 0.0, (150, 0), (80, 0), 0)),
          (L(64, 6, 0.0, (30.3, 0), (200, 0), 0), L(64, 6, 0.5, (20, 0), (-100, 3), 0)),
          (L(64, 6, 0.5, (-100, 0), (37.7, 0), 0), L(64, 6, 0.0, (150, 0), (21, 0), 0)),
          (L(64, 6, 0.0, (-1000, 0), (-980, 0), 1), L(64, 6, 0.41, (-16000, 0), (-15984, 0), 1))]
    if brush:
        # tile repeat: the line lies inside one stretch tile; 100-px prims, so that every stretch size puts a tile boundary inside the span
        w, h = 100, 10
        for sname, sx_, sy_ in (("4", 4.0, 4.0), ("7.5", 7.5, 7.5), ("64", 64.0, 64.0), ("rect/2.5", w / 2.5, h / 2.5)):
            for axis in ("x", "y", "xy"):
                st = (sx_ if "x" in axis else float(w), sy_ if "y" in axis else float(h))
                mk = lambda fx, ext, rev: L(w, h, fx, *(((0.9 * st[0], 0.6 * st[1]), (0.1 * st[0], 0.0)) if rev else ((0.1 * st[0], 0.0), (0.9 * st[0], 0.6 * st[1]))),
                                            ext, stretch=st, stretch_name=sname)
                V.append((mk(0.0, 0, False), mk(0.41, 1, True)))
    long = []
    for w in LONG_WIDTHS:
        long += [L(w, 3, 0.0, (0, 0), (w, 0), 0), L(w, 3, 0.41, (w, 0), (0, 0), 0), L(w, 3, 0.5, (-10, 0), (w + 10, 3), 0), L(w, 3, 0.0, (w + 5, 2), (-5, 0), 0)]
    F.crossed(fixed, V, long)
    return F.cases


def _radial_family(family):
    cs = family in CS
    F = _Family(family, radial_classes)

    def R(w, h, fx, center, r0, r1, extend, ratio=1.0, scale=1.0):
        return _geo(w, h, fx, center=(float(center[0]), float(center[1])), r0=float(r0), r1=float(r1), ratio=float(ratio), extend=extend, scale=float(scale))
    fixed = [R(64, 12, 0.0, (32, 6), 0, 30, 0), R(64, 12, 0.41, (20.3, 4.7), 5, 25, 1), R(64, 12, 0.5, (-10, 6), 8, 90, 0), R(61, 12, 0.0, (80, -20), 10, 60, 1)]
    V = []
    for i, w in enumerate(WIDTHS):
        V.append((R(w, 5, ORIGINS[i % 3], (w / 2 + 0.3, 2.2), 1, w / 2 + 3, 0), R(w, 5, ORIGINS[(i + 1) % 3], (w / 2 - 0.2, 1.7), 0.5, w / 2 + 2, 1)))
    # centre
    V += [(R(64, 12, 0.0, (31.7, 5.2), 4, 28, 0), R(64, 12, 0.41, (12.2, 8.9), 4, 28, 1)),
          (R(64, 12, 0.0, (-15, 6.5), 4, 60, 0), R(64, 12, 0.5, (-3.3, 2), 4, 40, 1)),
          (R(64, 12, 0.41, (79, 6.5), 4, 60, 0), R(64, 12, 0.0, (66.6, 11), 4, 40, 1)),
          (R(64, 12, 0.0, (20.5, 6.5), 0, 20, 0), R(64, 12, 0.0, (0.5, 0.5), 0, 50, 1)),
          (R(64, 12, 0.0, (20, 6), 0, 20, 0), R(64, 12, 0.0, (33, 3), 2, 30, 1))]
    # radii
    V += [(R(64, 12, 0.41, (30.3, 6.2), 0, 25, 0), R(64, 12, 0.5, (30.3, 6.2), 0, 40, 1)),
          (R(64, 12, 0.0, (30.3, 6.2), 10, 26, 0), R(64, 12, 0.41, (30.3, 6.2), 5, 12, 1)),
          (R(64, 12, 0.0, (30.3, 6.2), 10, 10.5, 0), R(64, 12, 0.41, (30.3, 6.2), 7, 7.5, 1)),
          (R(64, 12, 0.0, (30.3, 6.2), 0, 1e4, 0), R(64, 12, 0.41, (10.3, 6.2), 0, 1e4, 1)),
          (R(64, 12, 0.0, (30.3, 6.2), 10, 10, 0), R(64, 12, 0.41, (30.3, 6.2), 4, 4, 1)),
          (R(64, 12, 0.0, (30.3, 6.2), 25, 5, 0), R(64, 12, 0.41, (30.3, 6.2), 30, 12, 1))]
    # ratio_xy, task scale
    for ratio in (0.25, 4.0):
        V.append((R(64, 12, 0.0, (30.3, 6.2), 3, 27, 0, ratio=ratio), R(64, 12, 0.41, (22.3, 3.2), 3, 27, 1, ratio=ratio)))
    if cs:
        for scale in (0.5, 2.0):
            V.append((R(64, 12, 0.0, (30.3, 6.2), 3, 27, 0, scale=scale), R(64, 12, 0.41, (22.3, 3.2), 3, 27, 1, scale=scale)))
    long = []
    for w in LONG_WIDTHS:
        long += [R(w, 3, 0.0, (w * 0.3, 1.5), 0, w * 0.8, 0), R(w, 3, 0.41, (-50, 1.2), 10, w + 60, 0), R(w, 3, 0.5, (w + 30, 4), 20, w + 40, 0),
                 R(w, 3, 0.0, (w // 2 + 0.5, 1.5), 0, w * 0.6, 0)]
    F.crossed(fixed, V, long)
    return F.cases


ANGLES = (("0", 0.0), ("pi/2", math.pi / 2), ("pi", math.pi), ("2pi", 2 * math.pi), ("-1", -1.0), ("7", 7.0))


def _conic_family(family):
    F = _Family(family, conic_classes)

    def Cn(w, h, fx, center, angle, s0, s1, extend, scale=1.0):
        an = next((n for n, v in ANGLES if v == angle), f"{angle:g}")
        return _geo(w, h, fx, center=(float(center[0]), float(center[1])), angle=float(angle), angle_name=an, s0=float(s0), s1=float(s1), extend=extend, scale=float(scale))
    fixed = [Cn(64, 12, 0.0, (32, 6), 0.0, 0, 1, 0), Cn(64, 12, 0.41, (20.3, 4.7), 1.0, 0.25, 0.75, 1), Cn(64, 12, 0.5, (-10, 6), math.pi / 2, 0, 1, 0),
             Cn(61, 12, 0.0, (40, 20), -1.0, 0.1, 0.9, 1)]
    V = [(Cn(64, 12, 0.0, (20.5, 6.5), 0.3, 0, 1, 0), Cn(64, 12, 0.0, (40.5, 3.5), 2.0, 0, 1, 1)),
         (Cn(64, 12, 0.0, (20, 6), 0.3, 0, 1, 0), Cn(64, 12, 0.0, (41, 3), 2.0, 0.1, 0.9, 1)),
         (Cn(64, 12, 0.41, (-15, 20), 0.3, 0, 1, 0), Cn(64, 12, 0.5, (90, -8), 2.0, 0, 1, 1))]
    for _, a in ANGLES:
        V.append((Cn(64, 12, 0.0, (30.3, 6.2), a, 0, 1, 0), Cn(64, 12, 0.41, (12.3, 3.2), a, 0.1, 0.9, 1)))
    for s0, s1 in ((0.0, 1.0), (0.25, 0.75), (0.5, 0.5), (0.75, 0.25)):
        V.append((Cn(64, 12, 0.0, (30.3, 6.2), 0.7, s0, s1, 0), Cn(64, 12, 0.41, (12.3, 3.2), 4.0, s0, s1, 1)))
    F.crossed(fixed, V)
    return F.cases


def _fast_family(family):
    F = _Family(family, fast_classes)
    rng = np.random.default_rng([SEED, 8])

    def colours(kind):
        c0, c1 = ([float(v) for v in rng.uniform(0, 1, size=4)] for _ in range(2))
        if kind == "constant": c1 = list(c0)
        if kind == "alpha0_stops": c1[3] = 0.0
        return kind, tuple(c0[:3] + [c0[3]]), tuple(c1[:3] + [c1[3]])

    def add(w, h, fx, axis, kind):
        kname, c0, c1 = colours(kind)
        F.add("atlas", w, h, fx, None, "any", dict(axis=axis, colours=kname, c0=tuple(round(v, 4) for v in c0), c1=tuple(round(v, 4) for v in c1)))
    for w in WIDTHS:
        for j in range(8):
            add(w, 5, ORIGINS[j % 3], j % 2, "two_stop")
    for kind in ("constant", "alpha0_stops"):
        for j in range(8):
            add((64, 61)[j % 2], 6, ORIGINS[j % 3], (j // 2) % 2, kind)
    for w in LONG_WIDTHS:
        for j in range(8):
            add(w, 3, ORIGINS[j % 3], j % 2, "two_stop")
    return F.cases


GENERATORS = {"brush_linear_gradient": _linear_family, "cs_fast_linear_gradient": _fast_family, "cs_linear_gradient": _linear_family,
              "cs_radial_gradient": _radial_family, "cs_conic_gradient": _conic_family, "ps_quad_radial_gradient": _radial_family,
              "ps_quad_conic_gradient": _conic_family}
CASES = {f: GENERATORS[f](f) for f in FAMILIES}

_WIDTH_REQ = tuple(f"w{w}" for w in WIDTHS + LONG_WIDTHS) + ("x.0", "x.41", "x.5", "long_span", "span_lt_4", "tail_1", "tail_2", "tail_3")
_TABLE_REQ = TABLE_CLASSES + ("even_9_hard", "break_at_k", "even_N") + tuple("place_" + p for p in PLACES)
_LIN_REQ = _WIDTH_REQ + _TABLE_REQ + ("delta_pos", "delta_neg", "delta_zero", "delta_nonfinite", "one_entry_per_chunk", "tiny_delta", "huge_delta",
                                      "below_0", "above_1", "cross_0", "cross_1", "far_repeat", "clamp", "repeat", "seg_ge_1", "seg_ge_2")
_RAD_REQ = _WIDTH_REQ + _TABLE_REQ + ("centre_inside", "centre_left", "centre_right", "centre_on_pixel_centre", "centre_on_pixel_corner", "r0_zero",
                                      "inner_disc_inside_span", "range_half_px", "range_1e4", "r0_eq_r1", "r0_gt_r1", "ratio_0.25", "ratio_1", "ratio_4",
                                      "clamp", "repeat")
_CON_REQ = _TABLE_REQ + ("centre_on_pixel_centre", "centre_on_pixel_corner", "centre_outside", "offsets_0_1", "offsets_quarter", "offsets_equal",
                         "offsets_reversed", "clamp", "repeat") + tuple("angle_" + n for n, _ in ANGLES)
_PICTURE_REQ = ("bins", "few_prims", "depth_runs")
REQUIRED = {
    "brush_linear_gradient": _LIN_REQ + _PICTURE_REQ + ("opaque_pass", "alpha_pass", "tile_repeat", "tile_x", "tile_y", "tile_xy", "stretch_4", "stretch_7.5",
                                                        "stretch_64", "stretch_rect/2.5"),
    "cs_fast_linear_gradient": _WIDTH_REQ + ("axis_x", "axis_y", "two_stop", "constant", "alpha0_stops"),
    "cs_linear_gradient": _LIN_REQ,
    "cs_radial_gradient": _RAD_REQ + ("scale_0.5", "scale_1", "scale_2"),
    "cs_conic_gradient": _CON_REQ,
    "ps_quad_radial_gradient": _RAD_REQ + _PICTURE_REQ,
    "ps_quad_conic_gradient": _CON_REQ + _PICTURE_REQ,
}


def class_counts(family):
    n = {}
    for c in CASES[family]:
        for k in c["classes"]:
            n[k] = n.get(k, 0) + 1
    return n


# coverage is a condition of the tables, not an accident of the seed
for _f in FAMILIES:
    _n = class_counts(_f)
    _short = {k: _n.get(k, 0) for k in REQUIRED[_f] if _n.get(k, 0) < MIN_PER_CLASS}
    assert not _short, f"gradient_cases: {_f} classes below {MIN_PER_CLASS} cases: {_short}"


def device_exact(case):
    """Is the case compared at 0 bytes on the device?  All but cs_conic_gradient (the device's atan2f: 1 LSB); its tables with a
    jump in them run on the host side only -- an angle 1 ulp off picks the entry on the other side of the jump."""
    return case["family"] != "cs_conic_gradient"


def device_runs(case):
    return case["family"] != "cs_conic_gradient" or case["table"][0] not in HARD_TABLES


# ---- packing -------------------------------------------------------------------------------------------------------------------
def _cell_size(c):
    e = 1 if c["fx"] else 0
    return c["w"] + e, c["h"] + e


def _pack(cases, band_h, max_per_band):
    """shelves, 2 px apart, inside bands of band_h rows (picture tiles; None: one unbounded band) -> {index: (x, y)}, height used"""
    pos = {}
    x, y, shelf, band, n_band = GAP, GAP, 0, 0, 0
    for c in cases:
        cw, ch = _cell_size(c)
        if x + cw + GAP > TILE_W:
            x, y, shelf = GAP, y + shelf + GAP, 0
        if band_h is not None and (y + ch + GAP > (band + 1) * band_h or n_band >= max_per_band):
            band += 1
            x, y, shelf, n_band = GAP, band * band_h + GAP, 0, 0
        pos[c["index"]] = (x, y)
        x += cw + GAP
        shelf = max(shelf, ch)
        n_band += 1
    return pos, y + shelf + GAP


def _pack_slivers(cases):
    """cells on an 80-px grid, each with one sliver (x = 3 + 40 n, 2 px wide) 33 px inside it: a depth run that ends and one that
    starts in the middle of a chunk"""
    pos = {}
    for i, c in enumerate(cases):
        x = 80 * (i % 12) + 10
        assert any(x + 8 <= 3 + SLIVER_PITCH * n and 3 + SLIVER_PITCH * n + 2 <= x + c["w"] - 8 for n in range(TILE_W // SLIVER_PITCH)), c["tag"]
        pos[c["index"]] = (x, GAP + 16 * (i // 12))
    return pos, GAP + 16 * ((len(cases) + 11) // 12)


FRAMES = {}          # family -> [frame name]
for _f in FAMILIES:
    _cs = CASES[_f]
    _names = ["atlas"] if _f in CS else ["dense", "rows", "slivers"]
    FRAMES[_f] = _names
    for _name in _names:
        _sel = [c for c in _cs if c["frame"] == _name]
        assert _sel, (_f, _name)
        if _name == "atlas":
            _pos, _h = _pack(_sel, None, None)
        elif _name == "slivers":
            _pos, _h = _pack_slivers(_sel)
        else:
            _pos, _h = _pack(_sel, TILE_H, ROWS_MAX_PER_TILE if _name == "rows" else 1 << 30)
        for c in _sel:
            cw, ch = _cell_size(c)
            x, y = _pos[c["index"]]
            c["cell"] = (x, y, x + cw, y + ch)
            assert x + cw <= TILE_W and (_name == "atlas" or y // TILE_H == (y + ch - 1) // TILE_H)
        for c in _sel:
            c["frame_height"] = _h


def frame_height(family, name):
    h = next(c["frame_height"] for c in CASES[family] if c["frame"] == name)
    return h if name == "atlas" else ((h + TILE_H - 1) // TILE_H) * TILE_H


def frame_cases(family, name):
    return [c for c in CASES[family] if c["frame"] == name]


def _prim_rect(c):
    x, y = c["cell"][0] + c["fx"], c["cell"][1] + c["fx"]
    return (x, y, x + c["w"], y + c["h"])


# ---- frame builders ----------------------------------------------------------------------------------------------------------------
def _atlas_frame(family, device):
    cases = [c for c in frame_cases(family, "atlas") if not device or device_runs(c)]
    height = frame_height(family, "atlas")
    frame = Frame(TILE_W, height, (1.0, 1.0, 1.0, 1.0))
    tex = TextureRef("gradient_atlas", TILE_W, height, G.GL_RGBA8, G.GL_LINEAR, render_target=True)
    tgt = Target(tex, "texture_cache", clear_color=(0.0, 0.0, 0.0, 0.0))
    tabs = Tables(frame.gpu_buffer_f)
    inst = []
    for c in cases:
        g, rect = c["g"], _prim_rect(c)
        if family == "cs_fast_linear_gradient":
            e = np.zeros(1, S.FASTGRAD_DTYPE)
            e["c0"][0] = [g["c0"][0] * g["c0"][3], g["c0"][1] * g["c0"][3], g["c0"][2] * g["c0"][3], g["c0"][3]]
            e["c1"][0] = [g["c1"][0] * g["c1"][3], g["c1"][1] * g["c1"][3], g["c1"][2] * g["c1"][3], g["c1"][3]]
            e["axis"][0] = float(g["axis"])
        elif family == "cs_linear_gradient":
            e = np.zeros(1, S.LGRAD_DTYPE)
            e["start"][0], e["end"][0], e["scale"][0] = g["start"], g["end"], (1.0, 1.0)
        else:
            e = np.zeros(1, S.RGRAD_DTYPE)
            s = g["scale"]
            e["center"][0], e["scale"][0] = (g["center"][0] * s, g["center"][1] * s), (s, s)
            if family == "cs_radial_gradient":
                e["r0"][0], e["r1"][0], e["ratio"][0] = g["r0"] * s, g["r1"] * s, g["ratio"]
            else:
                e["r0"][0], e["r1"][0], e["ratio"][0] = g["s0"], g["s1"], g["angle"]
        e["task"][0] = rect
        if c["table"] is not None:
            e["extend"][0] = g["extend"]
            e["addr"][0] = tabs.of(c, lambda a, e=e: e["addr"].__setitem__(0, a))
        inst.append(e)
    tabs.finish()
    desc = {"cs_fast_linear_gradient": "FAST_LINEAR_GRADIENT", "cs_linear_gradient": "LINEAR_GRADIENT", "cs_radial_gradient": "RADIAL_GRADIENT",
            "cs_conic_gradient": "CONIC_GRADIENT"}[family]
    tgt.steps.append(Step(family, desc, np.concatenate(inst), None, "none"))
    frame.passes.append([tgt])
    frame.readback = [tex]
    return frame


_FILL = dict(w=4, h=4, fx=0.0, table=("two_stop", 0), place="any")


def _picture_frame(family, name):
    cases = frame_cases(family, name)
    height = frame_height(family, name)
    frame = Frame(TILE_W, height, (1.0, 1.0, 1.0, 1.0))
    tabs = Tables(frame.gpu_buffer_f)
    brush = family == "brush_linear_gradient"
    big = (-S.BIG, -S.BIG, S.BIG, S.BIG)
    targets = []
    for ty in range(height // TILE_H):
        oy = ty * TILE_H
        tex = TextureRef(f"tile_0_{ty}", TILE_W, TILE_H, G.GL_RGBA8, G.GL_LINEAR, render_target=True, with_depth=True)
        target = Target(tex, "picture_tile", clear_color=(1.0, 1.0, 1.0, 1.0), clear_depth=True)
        task = frame.add_render_task((0.0, 0.0, float(TILE_W), float(TILE_H)), 1.0, (0.0, float(oy)))
        mine = [c for c in cases if c["cell"][1] // TILE_H == ty]
        if brush and name == "dense" and len(mine) < DENSE_MIN_PER_TILE:
            # filler prims (no cases) along the tile's bottom edge: the tile has to stay above what the row kernel takes
            y = oy + TILE_H - 6
            assert all(c["cell"][3] + GAP <= y for c in mine)
            mine = mine + [dict(_FILL, family=family, cell=(GAP + 6 * i, y, GAP + 6 * i + 4, y + 4),
                                g=dict(start=(0.0, 0.0), end=(4.0, 2.0), extend=0, **{"pass": "alpha"})) for i in range(DENSE_MIN_PER_TILE - len(mine))]
        op, al = [], []
        for zi, c in enumerate(mine):
            g, rect = c["g"], _prim_rect(c)
            if brush:
                st = g.get("stretch") or (float(c["w"]), float(c["h"]))
                spec = frame.gpu_cache.push([[g["start"][0], g["start"][1], g["end"][0], g["end"][1]], [float(g["extend"]), st[0], st[1], 0.0]])
                slot = []
                lut = tabs.of(c, lambda a, slot=slot: frame.prim_headers_i.data.__setitem__((2 * slot[0] + 1, 0), a))
                ph = frame.add_prim_header(rect, big, zi + 1, spec, 0, task, (lut, 0, 0, 0))
                slot.append(ph)
                (op if g["pass"] == "opaque" else al).append(frame.brush_instance(ph, CLIP_TASK_EMPTY))
            else:
                repeat = float(g["extend"])
                if family == "ps_quad_radial_gradient":
                    blocks = [[g["center"][0], g["center"][1], 1.0, 1.0], [g["r0"], g["r1"], g["ratio"], repeat]]
                else:
                    blocks = [[g["center"][0], g["center"][1], 1.0, 1.0], [g["s0"], g["s1"], g["angle"], repeat]]
                params = frame.gpu_buffer_f.push(blocks)
                slot = []
                lut = tabs.of(c, lambda a, slot=slot: frame.gpu_buffer_i.data.__setitem__((slot[0], 3), a))
                q = frame.quad_instance(rect, big, (1.0, 1.0, 1.0, 1.0), zi + 1, task, pattern_input=(params, lut))
                slot.append(q[0])
                target.alpha.append(Step(family, "PRIM_INSTANCES", np.array([q], dtype=np.int32), "PremultipliedAlpha", "alpha", textures={}))
        if op:
            target.opaque.append(Step("brush_linear_gradient", "PRIM_INSTANCES", np.array(op[::-1], dtype=np.int32), None, "opaque"))
        if al:
            target.alpha.append(Step("brush_linear_gradient ALPHA_PASS", "PRIM_INSTANCES", np.array(al, dtype=np.int32), "PremultipliedAlpha", "alpha"))
        targets.append(target)
        rect = (0.0, float(oy), float(TILE_W), float(oy + TILE_H))
        frame.composite_tiles.append(CompositeTile(tex, rect, rect, opaque=True))
        frame.readback.append(tex)
    frame.passes.append(targets)
    tabs.finish()
    if name == "slivers":
        S.add_slivers(frame, pitch=SLIVER_PITCH, width=2, y0=0, y1=height)
    return frame


def make_frame(family, name, device=False):
    """the frame `name` of the family; device=True: what the device draws of it (device_runs), every cell where it was"""
    return _atlas_frame(family, device) if name == "atlas" else _picture_frame(family, name)


def image(result, family, name):
    """the frame's readback as one (height, 1024, 4) array of stored bytes: the cache target, or the picture tiles one below the other"""
    if name == "atlas":
        return result["gradient_atlas"]
    return np.concatenate([result[f"tile_0_{ty}"] for ty in range(frame_height(family, name) // TILE_H)])


def cell_of(img, case):
    x0, y0, x1, y1 = case["cell"]
    return img[y0:y1, x0:x1]


def drawn(img, case):
    """the pixels of the case's cell that hold something other than the target's clear colour, as rows of 4 bytes"""
    px = cell_of(img, case).reshape(-1, 4)
    clear = np.array([0, 0, 0, 0] if case["frame"] == "atlas" else [255, 255, 255, 255], np.uint8)
    return px[(px != clear).any(axis=1)]


def digest(px):
    return hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest()[:24]


def outside_cells(family, name, shape):
    """mask of the frame's pixels that belong to no case's cell"""
    m = np.ones(shape[:2], bool)
    for c in frame_cases(family, name):
        x0, y0, x1, y1 = c["cell"]
        m[y0:y1, x0:x1] = False
    return m
