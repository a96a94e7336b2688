"""Case tables for the immediate pixel calls of the ABI -- BlitFramebuffer, Composite, CompositeYUV, ClearTexSubImage /
ClearTexImage / ClearColorRect, TexSubImage2D and ReadPixels -- and the driver that runs one case on a backend
(tests/test_pixel_calls.py compares the backends; tests/golden/make_pixel_calls.py records the oracle's digests).

Every table is a pure function of SEED.  A case is a small dict: the call's parameters, `classes` (labels computed from the
parameters alone: what the call has to exercise, counted below at import) and `tag` (one line a failure message prints in full).
Texture contents come from the case's own rng (content_rng), so a case can be run alone.

What the cases stay inside, because the oracle is built without its asserts and an illegal call is undefined there:
BlitFramebuffer never swaps X; Composite runs between RGBA8 textures, CompositeYUV between three planes of one format (R8 at
depth 8, R16 above) with equal chroma planes; clear rects overlap and upload rects lie inside their texture; request sizes are
positive."""
import ctypes as C
import hashlib
import numpy as np
from webrender_amd import glconst as G

SEED = 0x51C3A11
SIDES = (1, 2, 3, 4, 5, 7, 8, 13, 16, 31, 33, 64, 67)
FAMILIES = ("blit", "composite", "composite_yuv", "clear", "upload")
MIN_PER_CLASS = 12
NOOP_CAP = 0.20          # share of a family's cases the call may leave the destination unchanged in (measured on the oracle)

# bytes per texel -> (internal format, data format, data type, numpy dtype, channels)
FORMATS = {
    1: (G.GL_R8, G.GL_RED, G.GL_UNSIGNED_BYTE, np.uint8, 1),
    2: (G.GL_RG8, G.GL_RG, G.GL_UNSIGNED_BYTE, np.uint8, 2),
    4: (G.GL_RGBA8, G.GL_BGRA, G.GL_UNSIGNED_BYTE, np.uint8, 4),
    "r16": (G.GL_R16, G.GL_RED, G.GL_UNSIGNED_SHORT, np.uint16, 1),
}
CROSS_PAIRS = ((1, 2), (1, 4), (2, 1), (2, 4), (4, 1), (4, 2))
NEAREST, LINEAR = G.GL_NEAREST, G.GL_LINEAR


def _side(rng, lo=1, hi=67):
    return int(rng.choice([s for s in SIDES if lo <= s <= hi]))


def _span(rng, n, out):
    """[a, b) with a < b that overlaps [0, n) and reaches at most `out` outside it"""
    a = int(rng.integers(-out, n))
    b = int(rng.integers(max(a, 0) + 1, n + out + 1))
    return a, b


def _inter(a, b):
    return (max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3]))


def _empty(r):
    return r[2] <= r[0] or r[3] <= r[1]


def _fmt_rect(r):
    return "(" + ",".join(str(int(v)) for v in r) + ")"


# ---- blit -----------------------------------------------------------------------------------------------------------------
# src / dst: (x0, y0, x1, y1) as handed to BlitFramebuffer: y0 > y1 is a Y flip on that side

def blit_linear_path(c):
    """does the call take linear_blit?  (composite.h:473-476, from the parameters)"""
    sw_, sh_ = c["src"][2] - c["src"][0], abs(c["src"][3] - c["src"][1])
    dw_, dh_ = c["dst"][2] - c["dst"][0], abs(c["dst"][3] - c["dst"][1])
    return c["filter"] == LINEAR and c["sbpp"] == c["dbpp"] and c["sw"] >= 2 and (sw_, sh_) != (dw_, dh_)


def blit_classes(c):
    s, d = c["src"], c["dst"]
    sy0, sy1 = min(s[1], s[3]), max(s[1], s[3])
    dy0, dy1 = min(d[1], d[3]), max(d[1], d[3])
    lin = blit_linear_path(c)
    k = [f"bpp{c['sbpp']}to{c['dbpp']}"]
    if lin and c["sbpp"] == 2:
        k.append("rg8_linear_scaled")
    if lin and (d[0] < 0 or dy0 < 0) and d[2] > 0 and dy1 > 0:
        k.append("linear_neg_dst")
    if not lin:
        if s[0] < 0: k.append("nearest_src_left")
        if sy0 < 0: k.append("nearest_src_top")
        if s[2] > c["sw"]: k.append("nearest_src_right")
        if sy1 > c["sh"]: k.append("nearest_src_bottom")
    if c["sw"] == 1 and c["filter"] == LINEAR:
        k.append("src_w1_linear")
    if s[3] < s[1] or d[3] < d[1]:
        k.append("flip_y")
    return tuple(k)


def _tdiv(a, b):
    return abs(a) // b if a >= 0 else -(abs(a) // b)


def blit_bounds(c):
    """the destination bounds of the call RELATIVE to its (flip-normalised) request, by the reference's rules (composite.h:166-195,
    362-366, 456-478): request & texture; for linear_blit & the ABSOLUTE request, which BlitFramebuffer hands it as the clip rect;
    for scale_blit & the source texture's bounds scaled to the destination rounding inward"""
    s, d = list(c["src"]), list(c["dst"])
    if s[3] < s[1]:
        s[1], s[3], d[1], d[3] = s[3], s[1], d[3], d[1]
    inv = d[3] < d[1]
    if inv:
        d[1], d[3] = d[3], d[1]
    sw_, sh_, dw_, dh_ = s[2] - s[0], s[3] - s[1], d[2] - d[0], d[3] - d[1]
    b = _inter((0, 0, dw_, dh_), (-d[0], -d[1], c["dw"] - d[0], c["dh"] - d[1]))
    if blit_linear_path(c):
        return _inter(b, d)
    k = [-s[0], -s[1], c["sw"] - s[0], c["sh"] - s[1]]
    if inv:
        k[1], k[3] = sh_ - k[3], sh_ - k[1]
    return _inter(b, (_tdiv(k[0] * dw_ + sw_ - 1, sw_), _tdiv(k[1] * dh_ + sh_ - 1, sh_), _tdiv(k[2] * dw_, sw_), _tdiv(k[3] * dh_, sh_)))


BLIT_KINDS = ("any", "any", "copy", "rg8_linear_scaled", "linear_neg_dst", "nearest_src_left", "nearest_src_top",
              "nearest_src_right", "nearest_src_bottom", "src_w1_linear", "cross", "any")
BLIT_REQUIRED = tuple(f"bpp{a}to{b}" for a in (1, 2, 4) for b in (1, 2, 4)) + (
    "rg8_linear_scaled", "linear_neg_dst", "nearest_src_left", "nearest_src_top", "nearest_src_right", "nearest_src_bottom", "src_w1_linear")


def _blit_candidate(rng, kind, cross):
    c = {}
    if kind in ("rg8_linear_scaled",):
        c["sbpp"] = c["dbpp"] = 2
    elif kind in ("copy", "linear_neg_dst"):
        c["sbpp"] = c["dbpp"] = int(rng.choice([1, 2, 4]))
    elif kind == "cross" or rng.random() >= 0.6:
        c["sbpp"], c["dbpp"] = cross
    else:
        c["sbpp"] = c["dbpp"] = int(rng.choice([1, 2, 4]))
    c["sw"], c["sh"], c["dw"], c["dh"] = _side(rng), _side(rng), _side(rng), _side(rng)
    if kind == "src_w1_linear":
        c["sw"] = 1
    if kind in ("rg8_linear_scaled", "linear_neg_dst"):
        c["sw"] = _side(rng, 2)
    c["filter"] = LINEAR if kind in ("rg8_linear_scaled", "linear_neg_dst", "src_w1_linear") else NEAREST if kind.startswith("nearest") or kind == "copy" else int(rng.choice([NEAREST, LINEAR]))
    so = 3 if (kind.startswith("nearest") or rng.random() < 0.3) else 0
    do = 5 if rng.random() < 0.3 else 0
    sx0, sx1 = _span(rng, c["sw"], so)
    sy0, sy1 = _span(rng, c["sh"], so)
    if kind == "nearest_src_left": sx0 = -int(rng.integers(1, 4))
    if kind == "nearest_src_top": sy0 = -int(rng.integers(1, 4))
    if kind == "nearest_src_right": sx1 = c["sw"] + int(rng.integers(1, 4))
    if kind == "nearest_src_bottom": sy1 = c["sh"] + int(rng.integers(1, 4))
    dx0, dx1 = _span(rng, c["dw"], do)
    dy0, dy1 = _span(rng, c["dh"], do)
    if kind == "copy" or (kind == "any" and rng.random() < 0.15):       # equal sizes: the copy path (or its flipped / converting forms)
        dx0 = int(rng.integers(max(-5, 1 - (sx1 - sx0)), c["dw"])); dx1 = dx0 + (sx1 - sx0)
        dy0 = int(rng.integers(max(-5, 1 - (sy1 - sy0)), c["dh"])); dy1 = dy0 + (sy1 - sy0)
    if kind == "linear_neg_dst":
        if rng.random() < 0.6: dx0 = -int(rng.integers(1, 6))
        else: dy0 = -int(rng.integers(1, 6))
        if rng.random() < 0.3: dx0, dy0 = -int(rng.integers(1, 6)), -int(rng.integers(1, 6))
    c["src"], c["dst"] = [sx0, sy0, sx1, sy1], [dx0, dy0, dx1, dy1]
    if blit_linear_path(c) and rng.random() < 0.8:
        # (linear_blit is handed the ABSOLUTE request as its clip: a request that starts beyond its own size draws nothing --
        # most linear cases start near the origin)
        w_, h_ = dx1 - dx0, dy1 - dy0
        nx = dx0 if dx0 < 0 else int(rng.integers(-2, max(1, w_ // 3) + 1))
        ny = dy0 if dy0 < 0 else int(rng.integers(-2, max(1, h_ // 3) + 1))
        if nx + w_ > 0 and ny + h_ > 0:
            c["dst"] = [nx, ny, nx + w_, ny + h_]
    flip = rng.random()
    if 0.5 <= flip < 0.67 or flip >= 0.84:
        c["src"][1], c["src"][3] = c["src"][3], c["src"][1]
    if flip >= 0.67:
        c["dst"][1], c["dst"][3] = c["dst"][3], c["dst"][1]
    return c


def blit_cases(n=408):
    rng = np.random.default_rng([SEED, 1])
    out, ncross = [], 0
    for i in range(n):
        kind = BLIT_KINDS[i % len(BLIT_KINDS)]
        while True:
            c = _blit_candidate(rng, kind, CROSS_PAIRS[ncross % 6])
            # (a call whose bounds come out empty draws nothing: one in eight of those is kept)
            if (kind in ("any", "copy", "cross") or kind in blit_classes(c)) and (not _empty(blit_bounds(c)) or rng.random() < 0.125):
                break
        if c["sbpp"] != c["dbpp"]:
            ncross += 1
        c["classes"] = blit_classes(c)
        c["tag"] = (f"blit[{i}] {c['sbpp']}B {c['sw']}x{c['sh']} -> {c['dbpp']}B {c['dw']}x{c['dh']} src{_fmt_rect(c['src'])} dst{_fmt_rect(c['dst'])} "
                    f"{'LINEAR' if c['filter'] == LINEAR else 'NEAREST'} {'/'.join(c['classes'])}")
        out.append(c)
    return out


# ---- composite / composite_yuv: requests and clips ---------------------------------------------------------------------------
# src / dst / clip: (x, y, w, h) as handed to Composite / CompositeYUV

def visible(c):
    """the destination bounds of a Composite / CompositeYUV call RELATIVE to its request: request & texture & clip"""
    x, y, w, h = c["dst"]
    b = _inter((0, 0, w, h), (-x, -y, c["dw"] - x, c["dh"] - y))
    cl = c["clip"]
    return _inter(b, (cl[0] - x, cl[1] - y, cl[0] - x + cl[2], cl[1] - y + cl[3]))


def clip_mid_chunk(c):
    """the clip's left edge cuts into the request, at column 1 .. 3 of one of the request's 4-pixel chunks"""
    b = visible(c)
    return (not _empty(b)) and b[0] == c["clip"][0] - c["dst"][0] and b[0] % 4 != 0


def _request(rng, n, out, lo=1):
    a, b = _span(rng, n, out)
    while b - a < lo:
        a, b = _span(rng, n, out)
    return a, b - a


def _clip_for(rng, c, mode):
    """mode: "request", "mid" (starts mid-chunk inside the request), "random" (intersects the request 4 times out of 5)"""
    x, y, w, h = c["dst"]
    if mode == "request":
        return [x, y, w, h]
    vis = _inter((x, y, x + w, y + h), (0, 0, c["dw"], c["dh"]))
    if mode == "mid" and vis[2] - vis[0] >= 2:
        for _ in range(64):
            cx = int(rng.integers(vis[0] + 1, vis[2]))
            if (cx - x) % 4 != 0:
                cy = int(rng.integers(vis[1], vis[3]))
                return [cx, cy, int(rng.integers(1, vis[2] - cx + 4)), int(rng.integers(1, vis[3] - cy + 4))]
    if rng.random() < 0.8 and not _empty(vis):
        cx, cy = int(rng.integers(vis[0] - 2, vis[2])), int(rng.integers(vis[1] - 2, vis[3]))
        return [cx, cy, int(rng.integers(max(1, vis[0] + 1 - cx), vis[2] - cx + 3)), int(rng.integers(max(1, vis[1] + 1 - cy), vis[3] - cy + 3))]
    return [int(rng.integers(-4, c["dw"] + 4)), int(rng.integers(-4, c["dh"] + 4)), int(rng.integers(1, 20)), int(rng.integers(1, 20))]


def composite_classes(c):
    k = [("opaque" if c["opaque"] else "blend") + ("_linear" if c["filter"] == LINEAR else "_nearest") + ("_flipx" if c["flip_x"] else "_noflipx")]
    if clip_mid_chunk(c): k.append("clip_mid_chunk")
    if c["flip_y"]: k.append("flip_y")
    if (c["src"][2], c["src"][3]) != (c["dst"][2], c["dst"][3]): k.append("scaled")
    if c["clip"] != c["dst"]: k.append("clipped")
    return tuple(k)


COMPOSITE_REQUIRED = tuple(f"{o}_{f}_{x}" for o in ("opaque", "blend") for f in ("nearest", "linear") for x in ("flipx", "noflipx")) + ("clip_mid_chunk",)


def composite_cases(n=304):
    rng = np.random.default_rng([SEED, 2])
    out = []
    for i in range(n):
        c = {"opaque": i & 1, "filter": LINEAR if i & 2 else NEAREST, "flip_x": (i >> 2) & 1, "flip_y": int(rng.random() < 0.35)}
        c["sw"], c["sh"], c["dw"], c["dh"] = _side(rng, 2 if rng.random() < 0.9 else 1), _side(rng), _side(rng), _side(rng)
        so, do = (3 if rng.random() < 0.3 else 0), (5 if rng.random() < 0.3 else 0)
        sx, sw_ = _request(rng, c["sw"], so); sy, sh_ = _request(rng, c["sh"], so)
        dx, dw_ = _request(rng, c["dw"], do); dy, dh_ = _request(rng, c["dh"], do)
        if rng.random() < (0.15 if c["filter"] == LINEAR else 0.4):       # equal sizes
            dw_, dh_ = sw_, sh_
            dx = int(rng.integers(max(-5, 1 - dw_), c["dw"])); dy = int(rng.integers(max(-5, 1 - dh_), c["dh"]))
        c["src"], c["dst"] = [sx, sy, sw_, sh_], [dx, dy, dw_, dh_]
        c["clip"] = _clip_for(rng, c, "mid" if i % 5 == 4 else "request" if rng.random() < 0.45 else "random")
        c["classes"] = composite_classes(c)
        c["tag"] = (f"composite[{i}] {c['sw']}x{c['sh']} -> {c['dw']}x{c['dh']} src{_fmt_rect(c['src'])} dst{_fmt_rect(c['dst'])} clip{_fmt_rect(c['clip'])} "
                    f"{'LINEAR' if c['filter'] == LINEAR else 'NEAREST'} flip({c['flip_x']},{c['flip_y']}) {'/'.join(c['classes'])}")
        out.append(c)
    return out


# ---- composite_yuv ---------------------------------------------------------------------------------------------------------
CHROMA_MODES = ("420", "422", "444", "quarter")


def chroma_size(mode, w, h):
    return {"420": ((w + 1) // 2, (h + 1) // 2), "422": ((w + 1) // 2, h), "444": (w, h), "quarter": (max(1, w // 4), h)}[mode]


def yuv_classes(c):
    cw, _ = chroma_size(c["chroma"], c["sw"], c["sh"])
    b = visible(c)
    span = 0 if _empty(b) else b[2] - b[0]
    k = [f"space{c['space']}", f"depth{c['depth']}", "chroma_" + c["chroma"]]
    if c["sw"] == 1 or cw == 1: k.append("plane_w1")
    if 2 <= c["sw"] <= 4: k.append("luma_w2_4")
    if c["flip_x"]: k.append("flip_x")
    if c["flip_y"]: k.append("flip_y")
    if c["dst"][2] < c["src"][2]: k.append("downscale")
    if c["depth"] == 8 and c["chroma"] == "420" and not c["flip_x"] and c["dst"][2] >= c["src"][2] and span >= 12 and c["sw"] >= 16:
        k.append("fast_window")
        if span % 4: k.append("fast_window_span_not4")
        if clip_mid_chunk(c): k.append("fast_window_clip_mid")
    if c["sw"] % 2 or c["sh"] % 2: k.append("odd_luma")
    return tuple(k)


YUV_KINDS = ("plane_w1", "plane_w1", "luma_w2_4", "fast_window", "fast_window_span_not4", "fast_window_clip_mid", "flip_x", "downscale",
             "chroma_444", "chroma_quarter", "depth10", "depth12", "depth16", "any", "any", "chroma_422")
YUV_REQUIRED = ("plane_w1", "luma_w2_4", "fast_window", "fast_window_span_not4", "fast_window_clip_mid", "flip_x", "downscale", "chroma_444",
                "chroma_quarter", "depth10", "depth12", "depth16") + tuple(f"space{s}" for s in range(7))


def _yuv_candidate(rng, kind, space):
    c = {"space": space}
    fast = kind.startswith("fast_window")
    c["depth"] = 8 if fast else int(kind[5:]) if kind.startswith("depth") else int(rng.choice([8, 8, 8, 10, 12, 16]))
    c["chroma"] = "420" if fast else kind[7:] if kind.startswith("chroma_") else str(rng.choice(CHROMA_MODES))
    c["sw"], c["sh"], c["dw"], c["dh"] = _side(rng), _side(rng), _side(rng), _side(rng)
    if kind == "plane_w1":
        c["sw"] = int(rng.choice([1, 1, 2, 3, 4, 5, 7]))
        if c["sw"] > 2: c["chroma"] = "quarter"
        elif c["sw"] == 2: c["chroma"] = str(rng.choice(["420", "422", "quarter"]))
    if kind == "luma_w2_4": c["sw"] = int(rng.choice([2, 3, 4]))
    c["flip_x"] = 1 if kind == "flip_x" else 0 if fast else int(rng.random() < 0.25)
    c["flip_y"] = int(rng.random() < 0.3)
    if fast:
        c["sw"], c["dw"] = _side(rng, 16), _side(rng, 13)
        sx = int(rng.integers(0, 3)); sw_ = int(rng.integers(12, c["sw"] - sx + 1))
        sy, sh_ = _request(rng, c["sh"], 0)
        dw_ = int(rng.integers(sw_, max(sw_, min(3 * sw_, c["dw"] + 4)) + 1)); dx = int(rng.integers(-3, max(-2, c["dw"] - dw_ + 3)))
        dy, dh_ = _request(rng, c["dh"], 5 if rng.random() < 0.3 else 0)
    else:
        so, do = (3 if rng.random() < 0.3 else 0), (5 if rng.random() < 0.3 else 0)
        sx, sw_ = _request(rng, c["sw"], so); sy, sh_ = _request(rng, c["sh"], so)
        dx, dw_ = _request(rng, c["dw"], do); dy, dh_ = _request(rng, c["dh"], do)
        if rng.random() < 0.25:       # 1:1
            dw_, dh_ = sw_, sh_
            dx = int(rng.integers(max(-5, 1 - dw_), c["dw"])); dy = int(rng.integers(max(-5, 1 - dh_), c["dh"]))
    c["src"], c["dst"] = [sx, sy, sw_, sh_], [dx, dy, dw_, dh_]
    c["clip"] = _clip_for(rng, c, "mid" if kind == "fast_window_clip_mid" or rng.random() < 0.15 else "request" if rng.random() < 0.5 else "random")
    return c


def composite_yuv_cases(n=400):
    rng = np.random.default_rng([SEED, 3])
    out = []
    for i in range(n):
        kind = YUV_KINDS[i % len(YUV_KINDS)]
        while True:
            c = _yuv_candidate(rng, kind, i % 7)
            if kind == "any" or kind in yuv_classes(c):
                break
        c["classes"] = yuv_classes(c)
        cw, ch = chroma_size(c["chroma"], c["sw"], c["sh"])
        c["tag"] = (f"composite_yuv[{i}] depth {c['depth']} space {c['space']} luma {c['sw']}x{c['sh']} chroma {cw}x{ch} -> {c['dw']}x{c['dh']} src{_fmt_rect(c['src'])} "
                    f"dst{_fmt_rect(c['dst'])} clip{_fmt_rect(c['clip'])} flip({c['flip_x']},{c['flip_y']}) {'/'.join(c['classes'])}")
        out.append(c)
    return out


# ---- clear -----------------------------------------------------------------------------------------------------------------
CLEAR_OPS = ("ClearTexSubImage", "ClearTexImage", "ClearColorRect")
CLEAR_REQUIRED = tuple(f"{op}_bpp{b}" for op in CLEAR_OPS for b in (1, 2, 4))


def clear_cases(n=207):
    rng = np.random.default_rng([SEED, 4])
    out = []
    for i in range(n):
        c = {"op": CLEAR_OPS[i % 3], "bpp": (1, 2, 4)[(i // 3) % 3], "w": _side(rng), "h": _side(rng)}
        c["data_type"] = "float" if c["op"] == "ClearColorRect" or rng.random() < 0.5 else "ubyte"
        c["data_format"] = "RGBA" if c["op"] == "ClearColorRect" else str(rng.choice(["RED", "RG", "RGBA"]))
        if c["data_type"] == "float":
            c["color"] = [float(np.float32(v)) for v in rng.choice([0.0, 1.0, 0.5, 0.25, 1.0 / 3.0, 0.999, 0.002] + list(rng.random(4)), 4)]
        else:
            c["color"] = [int(v) for v in rng.integers(0, 256, 4)]
        rect_kind = "whole" if c["op"] == "ClearTexImage" else str(rng.choice(["partial", "partial", "whole", "outside"]))
        if rect_kind == "whole":
            c["rect"] = [0, 0, c["w"], c["h"]]
        else:
            o = 4 if rect_kind == "outside" else 0
            x, w_ = _request(rng, c["w"], o); y, h_ = _request(rng, c["h"], o)
            c["rect"] = [x, y, w_, h_]
        c["classes"] = (f"{c['op']}_bpp{c['bpp']}", rect_kind, c["data_type"], c["data_format"])
        c["tag"] = f"clear[{i}] {c['op']} {c['bpp']}B {c['w']}x{c['h']} rect{_fmt_rect(c['rect'])} {c['data_format']}/{c['data_type']} {c['color']} {rect_kind}"
        out.append(c)
    return out


# ---- upload / readback -----------------------------------------------------------------------------------------------------
UPLOAD_KINDS = ("r8", "rg8", "bgra", "rgba", "r16")
UPLOAD_REQUIRED = UPLOAD_KINDS + ("pbo", "row_length", "read_outside", "read_rgba")


def upload_cases(n=200):
    rng = np.random.default_rng([SEED, 5])
    out = []
    for i in range(n):
        kind = UPLOAD_KINDS[i % 5]
        c = {"kind": kind, "w": _side(rng), "h": _side(rng)}
        x0, x1 = _span(rng, c["w"], 0); y0, y1 = _span(rng, c["h"], 0)
        c["rect"] = [x0, y0, x1 - x0, y1 - y0]
        c["row_extra"] = int(rng.choice([0, 0, 1, 3, 5]))
        c["pbo_offset"] = int(rng.choice([-1, -1, 0, 4, 12, 64]))          # -1: client memory
        o = 3 if rng.random() < 0.5 else 0
        while True:          # (nine readbacks in ten see some of what was uploaded)
            rx, rw = _request(rng, c["w"], o); ry, rh = _request(rng, c["h"], o)
            if not _empty(_inter((rx, ry, rx + rw, ry + rh), (x0, y0, x1, y1))) or rng.random() < 0.03:
                break
        c["read"] = [rx, ry, rw, rh]
        c["read_rgba"] = int(kind in ("bgra", "rgba") and rng.random() < 0.5)
        k = [kind]
        if c["pbo_offset"] >= 0: k.append("pbo")
        if c["row_extra"]: k.append("row_length")
        if rx < 0 or ry < 0 or rx + rw > c["w"] or ry + rh > c["h"]: k.append("read_outside")
        if c["read_rgba"]: k.append("read_rgba")
        c["classes"] = tuple(k)
        c["tag"] = (f"upload[{i}] {kind} {c['w']}x{c['h']} rect{_fmt_rect(c['rect'])} row_length+{c['row_extra']} "
                    f"{'client' if c['pbo_offset'] < 0 else 'pbo@%d' % c['pbo_offset']} read{_fmt_rect(c['read'])}{' as RGBA' if c['read_rgba'] else ''}")
        out.append(c)
    return out


GENERATORS = {"blit": blit_cases, "composite": composite_cases, "composite_yuv": composite_yuv_cases, "clear": clear_cases, "upload": upload_cases}
REQUIRED = {"blit": BLIT_REQUIRED, "composite": COMPOSITE_REQUIRED, "composite_yuv": YUV_REQUIRED, "clear": CLEAR_REQUIRED, "upload": UPLOAD_REQUIRED}
CASES = {}
for _f in FAMILIES:
    CASES[_f] = GENERATORS[_f]()
    for _i, _c in enumerate(CASES[_f]):
        _c["family"], _c["index"] = _f, _i


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
    assert not _short, f"pixel_call_cases: {_f} classes below {MIN_PER_CLASS} cases: {_short}"


# ---- the driver --------------------------------------------------------------------------------------------------------------
def content_rng(case):
    return np.random.default_rng([SEED, 99, FAMILIES.index(case["family"]), case["index"]])


def _texels(rng, key, w, h, premultiplied=False, bits=8):
    _, _, _, dtype, ch = FORMATS[key]
    px = rng.integers(0, 1 << bits, size=(h, w, ch), dtype=np.uint16 if bits > 8 else np.uint8).astype(dtype)
    if premultiplied:          # stored B, G, R, A with colour <= alpha
        a = px[..., 3:4].astype(np.uint16)
        px[..., :3] = ((px[..., :3].astype(np.uint16) * a + 127) // 255).astype(np.uint8)
    return px


def _make(gl, device, key, px):
    """a texture holding exactly `px` (every texel uploaded: fresh storage is undefined, and swgl keeps whole-texture clears pending)"""
    fmt, dfmt, dty, _, _ = FORMATS[key]
    h, w = px.shape[:2]
    t = device.create_texture(w, h, fmt, render_target=True)
    device.upload_texture(t, 0, 0, w, h, dfmt, dty, np.ascontiguousarray(px))
    t.key = key
    return t


def _read(gl, t, rect=None, as_rgba=False, fill=0):
    """ReadPixels of `rect` (all of the texture) in the texture's own format -> the bytes of the caller's buffer"""
    _, dfmt, dty, dtype, ch = FORMATS[t.key]
    x, y, w, h = rect or (0, 0, t.width, t.height)
    out = np.full((h, w, ch * np.dtype(dtype).itemsize), fill, np.uint8)
    gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, t.fbo)
    gl.ReadPixels(x, y, w, h, G.GL_RGBA if as_rgba else dfmt, dty, out)
    gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)
    return out.reshape(-1)


def _resource_bytes(gl, lock, bpp=4):
    w_, h_, s_ = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    p = gl.GetResourceBuffer(lock, w_, h_, s_)
    return np.concatenate([np.frombuffer(C.string_at(p + y * s_.value, w_.value * bpp), np.uint8) for y in range(h_.value)])


def _run_blit(gl, device, c, rng, call):
    s = _make(gl, device, c["sbpp"], _texels(rng, c["sbpp"], c["sw"], c["sh"]))
    d = _make(gl, device, c["dbpp"], _texels(rng, c["dbpp"], c["dw"], c["dh"]))
    if call:
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, s.fbo)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, d.fbo)
        gl.BlitFramebuffer(*c["src"], *c["dst"], G.GL_COLOR_BUFFER_BIT, c["filter"])
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, 0)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)
    return _read(gl, d), (s, d)


def _run_composite(gl, device, c, rng, call):
    s = _make(gl, device, 4, _texels(rng, 4, c["sw"], c["sh"], premultiplied=True))
    d = _make(gl, device, 4, _texels(rng, 4, c["dw"], c["dh"], premultiplied=True))
    ld, ls = gl.LockTexture(d.id), gl.LockTexture(s.id)
    if call:
        gl.Composite(ld, ls, *c["src"], *c["dst"], c["opaque"], c["flip_x"], c["flip_y"], c["filter"], *c["clip"])
    view = _resource_bytes(gl, ld)
    gl.UnlockResource(ls); gl.UnlockResource(ld)
    return np.concatenate([view, _read(gl, d)]), (s, d)


def _run_composite_yuv(gl, device, c, rng, call):
    key, bits = (1, 8) if c["depth"] == 8 else ("r16", c["depth"])
    cw, ch = chroma_size(c["chroma"], c["sw"], c["sh"])
    planes = [_make(gl, device, key, _texels(rng, key, w, h, bits=bits)) for (w, h) in ((c["sw"], c["sh"]), (cw, ch), (cw, ch))]
    d = _make(gl, device, 4, _texels(rng, 4, c["dw"], c["dh"]))
    ld = gl.LockTexture(d.id)
    locks = [gl.LockTexture(t.id) for t in planes]
    if call:
        gl.CompositeYUV(ld, locks[0], locks[1], locks[2], c["space"], c["depth"], *c["src"], *c["dst"], c["flip_x"], c["flip_y"], *c["clip"])
    for l in locks:
        gl.UnlockResource(l)
    view = _resource_bytes(gl, ld)
    gl.UnlockResource(ld)
    return np.concatenate([view, _read(gl, d)]), planes + [d]


def _run_clear(gl, device, c, rng, call):
    t = _make(gl, device, c["bpp"], _texels(rng, c["bpp"], c["w"], c["h"]))
    if call:
        data = (C.c_float * 4)(*c["color"]) if c["data_type"] == "float" else (C.c_uint8 * 4)(*c["color"])
        fmt = {"RED": G.GL_RED, "RG": G.GL_RG, "RGBA": G.GL_RGBA}[c["data_format"]]
        ty = G.GL_FLOAT if c["data_type"] == "float" else G.GL_UNSIGNED_BYTE
        x, y, w, h = c["rect"]
        if c["op"] == "ClearTexSubImage":
            gl.ClearTexSubImage(t.id, 0, x, y, 0, w, h, 1, fmt, ty, data)
        elif c["op"] == "ClearTexImage":
            gl.ClearTexImage(t.id, 0, fmt, ty, data)
        else:
            gl.ClearColorRect(t.fbo, x, y, w, h, *c["color"])
    return _read(gl, t), (t,)


def _run_upload(gl, device, c, rng, call):
    key = {"r8": 1, "rg8": 2, "bgra": 4, "rgba": 4, "r16": "r16"}[c["kind"]]
    _, dfmt, dty, dtype, ch = FORMATS[key]
    t = _make(gl, device, key, _texels(rng, key, c["w"], c["h"], bits=16 if key == "r16" else 8))
    x, y, w, h = c["rect"]
    rows = rng.integers(0, 1 << (16 if key == "r16" else 8), size=(h, w + c["row_extra"], ch), dtype=np.uint16).astype(dtype)
    if call:
        gl.ActiveTexture(G.GL_TEXTURE0); gl.BindTexture(G.GL_TEXTURE_2D, t.id)
        gl.PixelStorei(G.GL_UNPACK_ROW_LENGTH, w + c["row_extra"] if c["row_extra"] else 0)
        fmt = G.GL_RGBA if c["kind"] == "rgba" else dfmt
        if c["pbo_offset"] >= 0:
            pbo = gl.gen("GenBuffers")
            gl.BindBuffer(G.GL_PIXEL_UNPACK_BUFFER, pbo)
            gl.BufferData(G.GL_PIXEL_UNPACK_BUFFER, rows.nbytes + c["pbo_offset"], None, G.GL_STREAM_DRAW)
            gl.BufferSubData(G.GL_PIXEL_UNPACK_BUFFER, c["pbo_offset"], rows.nbytes, rows)
            gl.TexSubImage2D(G.GL_TEXTURE_2D, 0, x, y, w, h, fmt, dty, c["pbo_offset"])
            gl.BindBuffer(G.GL_PIXEL_UNPACK_BUFFER, 0)
            gl.DeleteBuffer(pbo)
        else:
            gl.TexSubImage2D(G.GL_TEXTURE_2D, 0, x, y, w, h, fmt, dty, rows)
        gl.PixelStorei(G.GL_UNPACK_ROW_LENGTH, 0)
    return _read(gl, t, c["read"], as_rgba=bool(c["read_rgba"]), fill=77), (t,)


_RUN = {"blit": _run_blit, "composite": _run_composite, "composite_yuv": _run_composite_yuv, "clear": _run_clear, "upload": _run_upload}
TWO_VIEWS = ("composite", "composite_yuv")          # results: GetResourceBuffer's bytes, then ReadPixels' -- both have to agree


def run_case(gl, device, case, call=True):
    """Create the case's textures, upload every texel of each, make the one call and return the destination's stored bytes
    (call=False: everything but the call -- what the destination held before it)."""
    res, texs = _RUN[case["family"]](gl, device, case, content_rng(case), call)
    for t in texs:
        device.delete_texture(t)
    return res


def digest(res):
    return hashlib.sha256(np.ascontiguousarray(res).tobytes()).hexdigest()


def run_family(lib_path, family, call=True):
    """every case of `family` on one context of the backend at `lib_path` -> the list of results"""
    from webrender_amd.glapi import GL
    from webrender_amd.device import Device
    gl = GL(lib_path)
    device = Device(gl)
    try:
        return [run_case(gl, device, c, call) for c in CASES[family]]
    finally:
        device.destroy()
