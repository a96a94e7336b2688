#!/usr/bin/env python3
"""Generates tests/golden/reftest_png.npz and reftest_png.json from the reference's own reftest manifests
(wrench/reftests/*/reftest.list): for each pinned manifest line the EXPECTED IMAGE (decoded RGBA8, first row = top of the window), the
display list's values (parsed numbers and names, no yaml text) and the fuzz the line resolves to on platform "swgl" -- input data and
recorded results of the reference, not code.  The tests (tests/test_reftest_png.py) read only the two fixtures.

    python3 tests/golden/make_reftest_pngs.py [reference root]        (in a container that has the reference tree)

How wrench resolves a line's fuzz (wrench/src/reftest.rs:345-532, ReftestManifest::new), restated in resolve_fuzz():
  * tokens are read left to right; `fuzzy(max, num)` pushes one range (and asserts the list was empty); `fuzzy-if(cond, max, num)` does
    nothing when the condition is false and otherwise CLEARS the list before pushing its range -- so `fuzzy(1,1) fuzzy-if(platform(swgl),4,27)`
    is (4, 27) alone on swgl;
  * `fuzzy-range(<=m1, n1, <=m2, *n2, ...)` pushes one range per pair; the `<=` and `*` prefixes are stripped and mean nothing to wrench
    (`*` is Gecko's "this count is not an upper bound worth tightening" marker); `fuzzy-range-if(cond, ...)` clears first like fuzzy-if;
  * a bare condition token such as `platform(linux,mac)` or `skip_on(android)` that is false ends the line (the test is not run): under
    swgl the platform string is "swgl" (reftest.rs:593-607), so `platform(linux,mac)` lines do not apply;
  * no range at all -> one range (allow_max_difference, allow_num_differences) = (0, 0) by default: exact; several ranges are sorted by
    max difference, and range j bounds the number of pixels whose difference is > range j-1's max and <= its own (reftest.rs:121-210).
"""
import json
import os
import re
import sys
import numpy as np
import yaml
from PIL import Image

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
PLATFORM = "swgl"

# (directory, yaml) of the pinned lines; the manifest line is looked up, not restated
LINES = [("clip", "clip-mode"), ("clip", "clip-ellipse"), ("aa", "rounded-rects"), ("border", "overlapping"), ("gradient", "linear"),
         ("gradient", "linear-reverse"), ("boxshadow", "inset-no-blur-radius"), ("image", "segments")]


def parse_function(tok):
    m = re.match(r"([\w-]+)\((.*)\)$", tok)
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def has(arg):
    """ReftestEnvironment::has (reftest.rs:580-591): the platform string or the build mode (no version under swgl)"""
    return arg in (PLATFORM, "release")


def condition(tok):
    """ReftestEnvironment::parse_condition (reftest.rs:646-678): True / False, None = not a condition"""
    if "(" not in tok:
        return None
    name, args = parse_function(tok)
    if name == "platform":
        return PLATFORM in args
    if name == "skip_on":                                     # skipped only if the environment has EVERY listed condition
        return not all(has(a) for a in args)
    if name == "env":
        return all(has(a) for a in args)
    return None


def split_if(tok):
    """`name-if(cond(...),a,b,...)` -> (cond, "a,b,...")"""
    return re.match(r"[\w-]+\((.*?\)),(.*)\)$", tok).groups()


def resolve_fuzz(tokens):
    fuzz, paths, op = [], [], None
    for tok in tokens:
        if tok in ("==", "!="):
            op = tok
        elif tok.startswith(("fuzzy-range(", "fuzzy-range-if(")):
            inner = tok[tok.index("(") + 1:-1]
            if tok.startswith("fuzzy-range-if("):
                cond, inner = split_if(tok)
                if not condition(cond):
                    continue
                fuzz.clear()
            args = [a.strip() for a in inner.split(",")]
            for k in range(len(args) // 2):
                fuzz.append([int(args[2 * k].removeprefix("<=")), int(args[2 * k + 1].removeprefix("*"))])
        elif tok.startswith(("fuzzy(", "fuzzy-if(")):
            inner = tok[tok.index("(") + 1:-1]
            if tok.startswith("fuzzy-if("):
                cond, inner = split_if(tok)
                if not condition(cond):
                    continue
                fuzz.clear()
            assert not fuzz                                   # (wrench asserts the same: "consider fuzzy-range instead")
            fuzz.append([int(v) for v in inner.split(",")])
        else:
            c = condition(tok)
            if c is None:
                paths.append(tok)
            elif not c:
                return None
    if not fuzz:
        fuzz = [[0, 0]]
    return op, paths, sorted(fuzz)


def find_line(directory, name):
    """the FIRST line of the directory's manifest that applies on swgl and compares <name>.yaml with a PNG"""
    for raw in open(os.path.join(REF, "wrench", "reftests", directory, "reftest.list")):
        s = raw.split("#")[0].strip()
        if not s or s.startswith("include"):
            continue
        r = resolve_fuzz(s.split())
        if r and r[0] == "==" and r[1][0] == name + ".yaml" and r[1][-1].endswith(".png"):
            return s, r[1][-1], r[2]
    raise KeyError((directory, name))


def nums(v):
    if isinstance(v, (list, tuple)):
        return [float(x) for x in v]
    return [float(x) for x in str(v).replace(",", " ").split()]


def radii(v):
    """yaml_helper.rs:454-501 as_border_radius -> [[w, h]] for top-left, top-right, bottom-left, bottom-right"""
    comp = lambda c: [float(c), float(c)] if isinstance(c, (int, float)) else nums(c)
    if v is None:
        return [[0.0, 0.0]] * 4
    if isinstance(v, (int, float)):
        return [[float(v), float(v)]] * 4
    if isinstance(v, dict):
        return [comp(v[k]) for k in ("top-left", "top-right", "bottom-left", "bottom-right")]
    if len(v) == 2:
        return [nums(v)] * 4
    assert len(v) == 4
    return [comp(c) for c in v]


def color(v):
    """yaml_helper.rs:55-95 string_to_color / as_colorf: a name, or 3 / 4 numbers (alpha 0..1) -> [r, g, b, a] in 0..255 / 0..1"""
    if isinstance(v, str) and not re.match(r"^[\d. ]+$", v):
        return v
    c = nums(v)
    return c + [1.0] if len(c) == 3 else c


def flatten(items, origin, clips, out):
    """the display list as a flat list of prims: stacking-context offsets folded into `origin`, `clip` / `clip-chain` items resolved
    into the complex clips each prim is under (yaml_frame_reader.rs: handle_clip, handle_clip_chain, `clip-chain:` on an item)"""
    for it in items:
        t = it.get("type")
        if t is None:
            t = "image" if "image" in it else "gradient" if "gradient" in it else "rect" if "rect" in it else None
        if t == "stacking-context":
            b = nums(it.get("bounds", [0, 0, 0, 0]))
            assert not any(k in it for k in ("transform", "filters", "mix-blend-mode", "perspective"))
            flatten(it["items"], [origin[0] + b[0], origin[1] + b[1]], clips, out)
        elif t == "clip":
            assert "items" not in it
            clips[it["id"]] = [{"rect": nums(c["rect"]), "radii": radii(c.get("radius")), "mode": c.get("clip-mode", "clip"), "origin": list(origin)}
                               for c in it.get("complex", [])]
        elif t == "clip-chain":
            clips[it["id"]] = [c for i in it["clips"] for c in clips[i]]
        else:
            chain = it.get("clip-chain")
            ids = chain if isinstance(chain, list) else [] if chain is None else [chain]
            d = {"type": t, "origin": list(origin), "bounds": nums(it["bounds"]), "clips": [c for i in ids for c in clips[i]]}
            if t == "rect":
                d["color"] = color(it["color"])
            elif t == "gradient":
                st = it["stops"]
                d.update(start=nums(it["start"]), end=nums(it["end"]), repeat=bool(it.get("repeat", False)),
                         stops=[[float(st[k]), color(st[k + 1])] for k in range(0, len(st), 2)])
            elif t == "box-shadow":
                d.update({"color": color(it["color"]), "offset": nums(it.get("offset", [0, 0])), "blur-radius": float(it.get("blur-radius", 0)),
                          "spread-radius": float(it.get("spread-radius", 0)), "clip-mode": it.get("clip-mode", "outset"),
                          "border-radius": radii(it.get("border-radius"))})
            elif t == "image":
                fn, args = parse_function(it["image"].replace(" ", ""))
                assert fn == "checkerboard"                   # yaml_frame_reader.rs:180-250: (border, tile size, tiles) or (border, tw, th, nx, ny)
                d["generator"] = {"name": fn, "args": [int(a) for a in args]}
            else:
                raise NotImplementedError(t)
            out.append(d)
    return out


def main():
    meta, pix = {}, {}
    for directory, name in LINES:
        line, png, fuzz = find_line(directory, name)
        key = f"{directory}/{name}"
        img = np.asarray(Image.open(os.path.join(REF, "wrench", "reftests", directory, png)).convert("RGBA"))
        doc = yaml.safe_load(open(os.path.join(REF, "wrench", "reftests", directory, name + ".yaml")))
        pix[key] = np.ascontiguousarray(img, dtype=np.uint8)
        meta[key] = {"directory": directory, "yaml": name + ".yaml", "image": png, "size": [int(img.shape[1]), int(img.shape[0])],
                     "fuzz": fuzz, "items": flatten(doc["root"]["items"], [0.0, 0.0], {}, [])}
    doc = {"source": "wrench/reftests/*/reftest.list of servo/webrender: expected images, display-list values, fuzz on platform swgl",
           "window": window_size(), "lines": meta}
    with open(os.path.join(HERE, "reftest_png.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "reftest_png.npz"), **pix)
    print("wrote", len(pix), "lines,", os.path.getsize(os.path.join(HERE, "reftest_png.npz")), "bytes of pixels")


def window_size():
    """wrench's default window, which `wrench reftest` runs in (wrench/src/main.rs: `.unwrap_or(DeviceIntSize::new(w, h))`)"""
    src = open(os.path.join(REF, "wrench", "src", "main.rs")).read()
    m = re.search(r"\.unwrap_or\(DeviceIntSize::new\((\d+), (\d+)\)\)", src)
    return [int(m.group(1)), int(m.group(2))]


if __name__ == "__main__":
    main()
