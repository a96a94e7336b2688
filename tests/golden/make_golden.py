"""Generates tests/golden/digests.json from the reference-built oracle
(oracle/_ref/libswgl_ref_gcc.so, i.e. the reference's own swgl compiled from
/root/reference).  Run in the authoring container: `python tests/golden/make_golden.py`.
The digests travel to the GPU box, where /root/reference does not exist."""
import hashlib
import json
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from webrender_amd import scenes
from webrender_amd.harness import render_direct
sys.path.insert(0, os.path.join(ROOT, "tests"))
from parity_cases import OCCLUDED, OCCLUDED_GOLDEN, BLEND, BLEND_GOLDEN, ROTATED, ROTATED_GOLDEN

LIB = os.path.join(ROOT, "oracle", "_ref", "libswgl_ref_gcc.so")


def digest(px):
    return hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest()


def round3_digests():
    """brush_mix_blend, brush_image DUAL_SOURCE_BLENDING (window pixels)"""
    from parity_cases import MIX_BLEND, DUAL_SOURCE
    out = {}
    for name, scene, kw in MIX_BLEND:
        out[name] = digest(render_direct(LIB, getattr(scenes, scene)(**kw))[0])
    for name, kw in DUAL_SOURCE:
        out[name] = digest(render_direct(LIB, scenes.image_grid(**kw))[0])
    from parity_cases import SPLIT, SPLIT_GOLDEN
    for name, make in SPLIT:             # ps_split_composite
        if name in SPLIT_GOLDEN:
            out[name] = digest(render_direct(LIB, make())[0])
    from parity_cases import GLYPH_TRANSFORM
    for name, make in GLYPH_TRANSFORM[:3]:      # ps_text_run GLYPH_TRANSFORM (hold with the same PIL glyph bitmaps only: golden_applies)
        out[name] = digest(render_direct(LIB, make())[0])
    from parity_cases import AA_SCAN, aa_scan_frame
    for name, enc, n, flagged, _plain in AA_SCAN:      # one AA request at the boundaries of the recording's scan
        out[name] = digest(render_direct(LIB, aa_scan_frame(enc, n, flagged))[0])
    for name, make in ROTATED:
        if (name.startswith("near_clipped") or name in ("perspective_filters_exact", "perspective_opacity", "perspective_gradients", "perspective_quad_gradients", "perspective_images_repeat", "perspective_quad_masks", "rotated_text", "perspective_text")) and name in ROTATED_GOLDEN:
            out[name] = digest(render_direct(LIB, make())[0])
    return out


def main():
    out = {}
    out["cfg1"] = digest(render_direct(LIB, scenes.cfg1_solid_colors())[0])
    out["simple_batching"] = digest(render_direct(LIB, scenes.simple_batching())[0])
    out["cfg2_small"] = digest(render_direct(LIB, scenes.cfg2_overlapping_rects(width=1024, height=1024, n=200, seed=7))[0])
    out["cfg2_small_frac"] = digest(render_direct(LIB, scenes.cfg2_overlapping_rects(width=1024, height=1024, n=200, seed=7, fractional=True))[0])
    out["cfg2_4k_quad"] = digest(render_direct(LIB, scenes.cfg2_overlapping_rects())[0])
    out["cfg2_4k_brush"] = digest(render_direct(LIB, scenes.cfg2_overlapping_rects(encoding="brush"))[0])
    out["cfg5_8k"] = digest(render_direct(LIB, scenes.cfg5_many_rects())[0])
    out["cfg5_small"] = digest(render_direct(LIB, scenes.cfg5_many_rects(width=2048, height=1024, n=5000))[0])
    # text: digests are only meaningful with the very same PIL/FreeType glyph
    # bitmaps, so the atlas digest is recorded next to them
    out["glyph_atlas"] = digest(scenes.build_glyph_atlas()[0])
    out["cfg3_small"] = digest(render_direct(LIB, scenes.cfg3_text(width=1024, height=512, lines=20, glyphs_per_line=60, run_len=12))[0])
    out["cfg3_small_zoom"] = digest(render_direct(LIB, scenes.cfg3_text(width=1024, height=512, lines=20, glyphs_per_line=60, run_len=12, glyph_zoom=1.25))[0])
    out["cfg3_4k"] = digest(render_direct(LIB, scenes.cfg3_text())[0])
    out["clip_masks"] = digest(render_direct(LIB, scenes.clip_masks())[0]["clip_masks"])
    out["clip_masks_dps"] = digest(render_direct(LIB, scenes.clip_masks(dps=1.5, seed=32))[0]["clip_masks"])
    out["box_shadow_masks"] = digest(render_direct(LIB, scenes.box_shadow_masks())[0]["box_shadow_masks"])
    out["box_shadow_masks_dps"] = digest(render_direct(LIB, scenes.box_shadow_masks(dps=1.5, seed=42))[0]["box_shadow_masks"])
    out["cfg4_small"] = digest(render_direct(LIB, scenes.cfg4_box_shadow(width=1024, height=1024))[0]["window"])
    out["cfg4_4k_dps2"] = digest(render_direct(LIB, scenes.cfg4_box_shadow(dps=2.0))[0]["window"])
    out["image_grid"] = digest(render_direct(LIB, scenes.image_grid())[0])
    out["gradient_grid"] = digest(render_direct(LIB, scenes.gradient_grid())[0])
    out["filter_grid"] = digest(render_direct(LIB, scenes.filter_grid())[0])
    out["quad_masks"] = digest(render_direct(LIB, scenes.quad_masks())[0])
    out["rotated_rects"] = digest(render_direct(LIB, scenes.rotated_rects())[0])
    out["rotated_images"] = digest(render_direct(LIB, scenes.rotated_images())[0])
    out["rotated_images_repeat"] = digest(render_direct(LIB, scenes.rotated_images(repeat=True))[0])
    out["rotated_images_quad"] = digest(render_direct(LIB, scenes.rotated_images(encoding="quad"))[0])
    out["opacity_grid"] = digest(render_direct(LIB, scenes.filter_grid(shader="opacity"))[0])
    out["image_repeat"] = digest(render_direct(LIB, scenes.image_repeat())[0])
    out["image_repeat_nearest"] = digest(render_direct(LIB, scenes.image_repeat(nearest=True))[0])
    out["filter_grid_exact"] = digest(render_direct(LIB, scenes.filter_grid(ops=[0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]))[0])
    out["aa_rects_brush"] = digest(render_direct(LIB, scenes.cfg2_overlapping_rects(width=1024, height=1024, n=120, seed=7, fractional=True, encoding="brush", aa_edges=15))[0])
    out["aa_rects_quad"] = digest(render_direct(LIB, scenes.cfg2_overlapping_rects(width=1024, height=1024, n=120, seed=7, fractional=True, encoding="quad", aa_edges=15))[0])
    out["scaled_composites"] = digest(render_direct(LIB, scenes.scaled_composites())[0])
    out["masked_rects"] = digest(render_direct(LIB, scenes.masked_rects())[0])
    out["masked_rects_frac"] = digest(render_direct(LIB, scenes.masked_rects(fractional=True))[0])
    for name, make in OCCLUDED + BLEND + ROTATED:
        if name in OCCLUDED_GOLDEN + BLEND_GOLDEN + ROTATED_GOLDEN:
            out[name] = digest(render_direct(LIB, make())[0])
    from parity_cases import BORDERS, BORDER_SEGMENTS
    for name, kw in BORDERS:
        out[name] = digest(render_direct(LIB, scenes.border_solid(**kw))[0]["border_cache"])
    from parity_cases import DECORATIONS
    for name, kw in DECORATIONS:
        out[name] = digest(render_direct(LIB, scenes.cache_decorations(**kw))[0]["decoration_cache"])
    for name, kw in BORDER_SEGMENTS:
        out[name] = digest(render_direct(LIB, scenes.border_segments(**kw))[0]["border_cache"])
    for name, kw in (("blur_r8", dict(fmt="r8")), ("blur_rgba8", dict(fmt="rgba8")),
                     ("blur_r8_sigmas", dict(fmt="r8", content=(40, 30), sigma=[0.8, 1.7, 3.2, 4.0], n_tasks=12, origin=(0, 0))),
                     ("blur_rgba8_tiny", dict(fmt="rgba8", content=(5, 3), sigma=1.2, n_tasks=9, origin=(1, 1), atlas=64)),
                     ("blur_r8_scaled", dict(fmt="r8", scale_steps=2, content=(166, 140), sigma=2.5)),
                     ("blur_rgba8_scaled", dict(fmt="rgba8", scale_steps=2, content=(150, 97), sigma=3.0))):
        out[name] = digest(render_direct(LIB, scenes.blur_chain(**kw))[0]["blur_h"])
    out.update(round3_digests())
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "digests.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--round3":
    # (only the entries added in round 3: the full set takes minutes of 4K / 8K oracle renders)
    path = os.path.join(ROOT, "tests", "golden", "digests.json")
    cur = json.load(open(path))
    cur.update(round3_digests())
    json.dump(cur, open(path, "w"), indent=1, sort_keys=True)
    sys.exit(0)
if __name__ == "__main__":
    main()


def abi_surface_golden():
    """tests/golden/abi_surface.json: digests of everything tests/abi_surface.py observes on the oracle."""
    import abi_surface
    d = abi_surface.digest_of(abi_surface.run(LIB))
    for k in abi_surface.BACKEND_SPECIFIC:
        d.pop(k, None)
    json.dump(d, open(os.path.join(ROOT, "tests", "golden", "abi_surface.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--round3":
    # (only the entries added in round 3: the full set takes minutes of 4K / 8K oracle renders)
    path = os.path.join(ROOT, "tests", "golden", "digests.json")
    cur = json.load(open(path))
    cur.update(round3_digests())
    json.dump(cur, open(path, "w"), indent=1, sort_keys=True)
    sys.exit(0)
if __name__ == "__main__":
    abi_surface_golden()
