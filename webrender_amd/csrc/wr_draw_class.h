// The class of a draw, decided when it is recorded: which programs form which family, which sampler slots the RASTER stage reads, and
// the WR_DF_SIMPLE / WR_DF_XFORM / WR_DF_QUADS bits that build_launches(), plan_target(), tile_rows_eligible() and span_rows_eligible()
// -- and through them the kernel variant of every launch -- depend on.  Plain C++: no HIP, no library state, only wrhip_types.h is
// needed.  Everything is constexpr and the cases at the end state today's behaviour, so a wrong edit fails both builds.
//
// A new shader key is entered in SHADERS[] (wrhip.hip), in shader_feat() and in the predicates below -- nowhere else on the record path.
#ifndef WR_DRAW_CLASS_H
#define WR_DRAW_CLASS_H
#include "wrhip_types.h"

// ---- program families ------------------------------------------------------------------------------------------------------------
constexpr bool is_text_run(int sh) { return sh == WR_SH_PS_TEXT_RUN || sh == WR_SH_PS_TEXT_RUN_DUAL || sh == WR_SH_PS_TEXT_RUN_GT || sh == WR_SH_PS_TEXT_RUN_DUAL_GT; }
constexpr bool is_clip_mask(int sh) { return sh == WR_SH_CS_CLIP_RECT || sh == WR_SH_CS_CLIP_RECT_FAST || sh == WR_SH_CS_CLIP_BOX_SHADOW; }
constexpr bool is_brush_solid(int sh) { return sh == WR_SH_BRUSH_SOLID || sh == WR_SH_BRUSH_SOLID_ALPHA; }
constexpr bool is_quad_prog(int sh) {
  return sh == WR_SH_PS_QUAD_TEXTURED || sh == WR_SH_PS_QUAD_MASK || sh == WR_SH_PS_QUAD_MASK_FAST || sh == WR_SH_PS_QUAD_RADIAL_GRADIENT || sh == WR_SH_PS_QUAD_CONIC_GRADIENT;
}
constexpr bool is_gradient_prog(int sh) {
  return sh == WR_SH_BRUSH_LINEAR_GRADIENT || sh == WR_SH_BRUSH_LINEAR_GRADIENT_ALPHA || sh == WR_SH_PS_QUAD_RADIAL_GRADIENT || sh == WR_SH_PS_QUAD_CONIC_GRADIENT ||
         sh == WR_SH_CS_LINEAR_GRADIENT || sh == WR_SH_CS_RADIAL_GRADIENT || sh == WR_SH_CS_CONIC_GRADIENT;
}
// The prim families (WR_FEAT_*) a draw of this program can hold unless the host has verified it plain (WR_DF_SIMPLE: none).  A clip
// mask that the rows kernel evaluates asks for WR_FEAT_BLUR instead: build_launches() knows which do.
constexpr int shader_feat(int sh) {
  if (sh == WR_SH_PS_CLEAR || sh == WR_SH_CLEAR_OP) return 0;
  if (is_text_run(sh)) return WR_FEAT_R8TEX | WR_FEAT_TEX | WR_FEAT_GENERIC;
  if (is_brush_solid(sh)) return WR_FEAT_R8TEX | WR_FEAT_GENERIC;      // masked / odd blend
  if (sh == WR_SH_CS_BLUR_ALPHA || sh == WR_SH_CS_BLUR_COLOR) return WR_FEAT_BLUR;
  if (is_clip_mask(sh)) return WR_FEAT_CLIP;
  if (is_gradient_prog(sh)) return WR_FEAT_SHADE | WR_FEAT_GENERIC;
  switch (sh) {
    case WR_SH_BRUSH_BLEND: case WR_SH_BRUSH_BLEND_ALPHA: case WR_SH_BRUSH_MIX_BLEND: case WR_SH_BRUSH_MIX_BLEND_ALPHA:
    case WR_SH_CS_SVG_FILTER: case WR_SH_CS_SVG_FILTER_NODE: case WR_SH_BRUSH_YUV: case WR_SH_BRUSH_YUV_ALPHA: case WR_SH_COMPOSITE_YUV:
    case WR_SH_PS_QUAD_MASK: case WR_SH_PS_QUAD_MASK_FAST:
    case WR_SH_CS_BORDER_SOLID: case WR_SH_CS_BORDER_SEGMENT: case WR_SH_CS_FAST_LINEAR_GRADIENT: case WR_SH_CS_LINE_DECORATION:
    case WR_SH_BRUSH_IMAGE_REPEAT: case WR_SH_BRUSH_IMAGE_REPEAT_ALPHA: case WR_SH_BRUSH_IMAGE_REPEAT_DUAL:
      return WR_FEAT_SHADE | WR_FEAT_GENERIC;
    default: return WR_FEAT_TEX | WR_FEAT_GENERIC;
  }
}
// Image-like brushes whose prims may sit on a general quad or ask for swgl_antiAlias: those need the WR_PK_TEX_QUAD path (WR_FEAT_SHADE
// launches).  WR_SH_BRUSH_IMAGE_DUAL is absent on purpose: its prims are drawn axis-aligned and without AA, whatever their ids and
// instances say; the ANTIALIASING,REPETITION twin of the dual-source key (..._REPEAT_DUAL) is on the general-quad path and is listed.
constexpr bool is_aa_image_brush(int sh) {
  return sh == WR_SH_BRUSH_IMAGE || sh == WR_SH_BRUSH_IMAGE_ALPHA || sh == WR_SH_BRUSH_OPACITY || sh == WR_SH_BRUSH_OPACITY_ALPHA ||
         sh == WR_SH_BRUSH_IMAGE_REPEAT || sh == WR_SH_BRUSH_IMAGE_REPEAT_ALPHA || sh == WR_SH_BRUSH_IMAGE_REPEAT_DUAL ||
         sh == WR_SH_BRUSH_LINEAR_GRADIENT || sh == WR_SH_BRUSH_LINEAR_GRADIENT_ALPHA || sh == WR_SH_BRUSH_BLEND || sh == WR_SH_BRUSH_BLEND_ALPHA ||
         sh == WR_SH_BRUSH_MIX_BLEND || sh == WR_SH_BRUSH_MIX_BLEND_ALPHA || sh == WR_SH_BRUSH_YUV || sh == WR_SH_BRUSH_YUV_ALPHA;
}
// Quad programs on the textured-quad path: all of is_quad_prog() except a ps_quad_textured draw whose sColor0 is the 1x1 dummy
// (`color0_wide`: width >= 2 -- a Rectangle prim samples nothing and is classed like a solid).
constexpr bool is_textured_quad(int sh, bool color0_wide) { return sh == WR_SH_PS_QUAD_TEXTURED ? color0_wide : is_quad_prog(sh); }
// Programs that write the second colour of GL_ONE, GL_ONE_MINUS_SRC1_COLOR themselves: every prim of the dual-source text programs
// replaces the key with swgl_blendSubpixelText / swgl_blendDropShadow in its vertex stage, the image programs' main() writes it.
constexpr bool writes_second_colour(int sh) {
  return sh == WR_SH_PS_TEXT_RUN_DUAL || sh == WR_SH_PS_TEXT_RUN_DUAL_GT || sh == WR_SH_BRUSH_IMAGE_DUAL || sh == WR_SH_BRUSH_IMAGE_REPEAT_DUAL;
}
// Programs whose main() reads component-transfer tables from the GPU cache (so the RASTER stage reads sGpuCache).
constexpr bool reads_transfer_tables(int sh) {
  return sh == WR_SH_BRUSH_BLEND || sh == WR_SH_BRUSH_BLEND_ALPHA || sh == WR_SH_CS_SVG_FILTER || sh == WR_SH_CS_SVG_FILTER_NODE;
}
// The sampler slots the RASTER stage of a draw reads; the data textures -- every other slot -- are consumed by the setup stage of the
// same flush.  The colour and mask samplers always; the filter tables; the gradient stops where the frame builder put them (the span
// shaders and main() of every gradient program read them), unless the setup stage copies them into the flush's pool for this draw
// (`gtab`: WR_DF_GTAB).
constexpr unsigned raster_read_mask(int kind, bool gtab) {
  return (1u << WR_S_COLOR0) | (1u << WR_S_COLOR1) | (1u << WR_S_COLOR2) | (1u << WR_S_CLIP_MASK) |
         (reads_transfer_tables(kind) ? 1u << WR_S_GPU_CACHE : 0u) | (is_gradient_prog(kind) && !gtab ? 1u << WR_S_GPU_BUFFER_F : 0u);
}

// ---- the class of one draw -------------------------------------------------------------------------------------------------------
// What the classification depends on, and nothing else.
struct DrawFacts {
  int kind = WR_SH_NONE;            // WrShader
  int blend = WR_BLEND_NONE;        // the draw's blend key (WR_BLEND_NONE with GL_BLEND off)
  bool rgba8 = false;               // the colour target is RGBA8 (the general-quad path exists there only)
  bool mask_wide = false;           // sClipMask is bound to a texture of width >= 2 (not the 1x1 dummy)
  bool color0_wide = false;         // sColor0 likewise
  // Does the RGBA32I texture on the unit of sPrimitiveHeadersI / sGpuBufferI hold a transform id that is not axis-aligned
  // (Texture::complex_ids_headers / complex_ids_gpubuf)?  The unit's 2-D binding, whatever the program's sampler set; no texture: clean.
  bool complex_headers = false, complex_gpubuf = false;
  bool third_word = false;          // the instances carry aData.z: attr_off[0] >= 0 && attr_bytes[0] >= 12 && inst_stride >= 12
};
// Whether a draw's instance bytes have to be asked for a swgl_antiAlias request (any_aa_request), and in which encoding.
enum WrAaScan { WR_AA_SCAN_NONE = 0, WR_AA_SCAN_BRUSH, WR_AA_SCAN_QUAD };

// draws that can only produce solid prims with a blend the inline raster paths know (WrFeat) -- before the instances have their say
constexpr bool simple_candidate(const DrawFacts& f) {
  const bool plain_blend = f.blend == WR_BLEND_NONE || f.blend == WR_BLEND_PREMULT;
  const bool maskable = f.blend != WR_BLEND_NONE && f.mask_wide;
  if (is_brush_solid(f.kind)) return plain_blend && !maskable && !f.complex_headers;
  if (f.kind == WR_SH_PS_QUAD_TEXTURED) return plain_blend && !f.color0_wide && !f.complex_gpubuf;
  return false;
}
// textured prims on rotated quads or with swgl_antiAlias need the WR_PK_TEX_QUAD path; so do masked solids.  (Glyph quads under a
// rotation -- local raster space -- ride on the same path, see aa_scan().)
constexpr bool quad_path_candidate(const DrawFacts& f) {
  const bool solid_masked = is_brush_solid(f.kind) && f.blend != WR_BLEND_NONE && f.mask_wide;
  return f.rgba8 && (is_aa_image_brush(f.kind) || is_textured_quad(f.kind, f.color0_wide) || solid_masked || is_text_run(f.kind));
}
// where the transform ids of the prims on the quad path live: the GPU buffer for textured quads, the prim headers otherwise
constexpr bool quad_path_ids_complex(const DrawFacts& f) { return is_textured_quad(f.kind, f.color0_wide) ? f.complex_gpubuf : f.complex_headers; }

// swgl_antiAlias only matters with blending on, and the bytes are only worth reading where the answer can change the class: a draw
// that would otherwise be SIMPLE, or one on the quad path whose transform ids are clean.  The two cases exclude each other (a SIMPLE
// solid has no mask, a SIMPLE ps_quad_textured a narrow sColor0), so a draw is scanned at most once.  Never a text run: the program
// never asks for swgl_antiAlias and a glyph instance's third word is not a brush's flags -- the transform ids alone decide.
constexpr WrAaScan aa_scan(const DrawFacts& f) {
  if (f.blend == WR_BLEND_NONE || !f.third_word) return WR_AA_SCAN_NONE;
  if (simple_candidate(f)) return f.kind == WR_SH_PS_QUAD_TEXTURED ? WR_AA_SCAN_QUAD : WR_AA_SCAN_BRUSH;
  if (quad_path_candidate(f) && !is_text_run(f.kind) && !quad_path_ids_complex(f)) return is_textured_quad(f.kind, f.color0_wide) ? WR_AA_SCAN_QUAD : WR_AA_SCAN_BRUSH;
  return WR_AA_SCAN_NONE;
}
// The WR_DF_SIMPLE | WR_DF_XFORM | WR_DF_QUADS bits.  `aa_request`: the scan's answer (ignored where aa_scan() asks for none).
constexpr int draw_class_flags(const DrawFacts& f, bool aa_request) {
  const bool aa = aa_request && aa_scan(f) != WR_AA_SCAN_NONE;
  int flags = 0;
  if (simple_candidate(f) && !aa) flags |= WR_DF_SIMPLE;
  // can a prim of this draw sit under a rotation or a projective transform?  (brushes / text: transform ids in the prim headers; quads:
  // in the GPU buffer.)  A split polygon's vertices are any convex quad, whatever the transform (ps_split_composite.glsl:85-87).
  if ((is_quad_prog(f.kind) ? f.complex_gpubuf : f.complex_headers) || f.kind == WR_SH_PS_SPLIT_COMPOSITE) flags |= WR_DF_XFORM;
  if (quad_path_candidate(f) && (quad_path_ids_complex(f) || aa)) flags |= WR_DF_QUADS;
  if (f.kind == WR_SH_PS_SPLIT_COMPOSITE && f.rgba8) flags |= WR_DF_QUADS;
  return flags;
}

// ---- today's behaviour, case by case (checked by the host pass of either build) --------------------------------------------------
#ifndef __HIP_DEVICE_COMPILE__
namespace wr_draw_class_cases {
// kind, blend, RGBA8 target, wide mask, wide sColor0, complex header ids, complex GPU-buffer ids; the third word is there
constexpr DrawFacts facts(int kind, int blend, bool rgba8 = true, bool mask = false, bool color0 = false, bool ch = false, bool cg = false) {
  DrawFacts f; f.kind = kind; f.blend = blend; f.rgba8 = rgba8; f.mask_wide = mask; f.color0_wide = color0; f.complex_headers = ch; f.complex_gpubuf = cg; f.third_word = true;
  return f;
}
constexpr bool every_kind(bool (*holds)(int)) { for (int k = 0; k < WR_SH_COUNT; k++) if (!holds(k)) return false; return true; }
// every combination of the boolean facts under the blend keys the classification tells apart (NONE, PREMULT, any other), for one
// program or for all of them
constexpr bool every_facts_of(int kind, bool (*holds)(const DrawFacts&)) {
  const int blends[] = {WR_BLEND_NONE, WR_BLEND_PREMULT, WR_BLEND_DUAL_SRC};
  for (int b : blends) for (int m = 0; m < 32; m++) if (!holds(facts(kind, b, m & 1, m & 2, m & 4, m & 8, m & 16))) return false;
  return true;
}
constexpr bool every_facts(bool (*holds)(const DrawFacts&)) { for (int k = 0; k < WR_SH_COUNT; k++) if (!every_facts_of(k, holds)) return false; return true; }
// brush_solid
constexpr DrawFacts solid = facts(WR_SH_BRUSH_SOLID_ALPHA, WR_BLEND_PREMULT);
static_assert(aa_scan(solid) == WR_AA_SCAN_BRUSH && draw_class_flags(solid, false) == WR_DF_SIMPLE, "a plain solid without an AA request is SIMPLE alone");
static_assert(draw_class_flags(solid, true) == 0, "a plain solid with an AA request is neither SIMPLE nor QUADS");
constexpr DrawFacts solid_masked = facts(WR_SH_BRUSH_SOLID_ALPHA, WR_BLEND_PREMULT, true, true);
static_assert(aa_scan(solid_masked) == WR_AA_SCAN_BRUSH && draw_class_flags(solid_masked, true) == WR_DF_QUADS && draw_class_flags(solid_masked, false) == 0,
              "a masked solid on RGBA8 is never SIMPLE and takes the quad path with an AA request");
static_assert(aa_scan(facts(WR_SH_BRUSH_SOLID, WR_BLEND_NONE, true, true)) == WR_AA_SCAN_NONE && draw_class_flags(facts(WR_SH_BRUSH_SOLID, WR_BLEND_NONE, true, true), true) == WR_DF_SIMPLE,
              "a mask does not matter to an unblended solid");
static_assert(draw_class_flags(facts(WR_SH_BRUSH_SOLID_ALPHA, WR_BLEND_ALPHA), false) == 0, "a solid under another blend key is not SIMPLE");
static_assert(aa_scan(facts(WR_SH_BRUSH_SOLID, WR_BLEND_PREMULT, true, false, false, true)) == WR_AA_SCAN_NONE &&
              draw_class_flags(facts(WR_SH_BRUSH_SOLID, WR_BLEND_PREMULT, true, false, false, true), false) == WR_DF_XFORM, "unclean header ids: XFORM, not SIMPLE, no scan");
// ps_quad_textured
constexpr DrawFacts rect_quad = facts(WR_SH_PS_QUAD_TEXTURED, WR_BLEND_PREMULT);
static_assert(aa_scan(rect_quad) == WR_AA_SCAN_QUAD && draw_class_flags(rect_quad, false) == WR_DF_SIMPLE && draw_class_flags(rect_quad, true) == 0,
              "ps_quad_textured with a narrow sColor0 is classed like a solid, with the quad scan");
constexpr DrawFacts image_quad = facts(WR_SH_PS_QUAD_TEXTURED, WR_BLEND_PREMULT, true, false, true);
static_assert(aa_scan(image_quad) == WR_AA_SCAN_QUAD && draw_class_flags(image_quad, false) == 0 && draw_class_flags(image_quad, true) == WR_DF_QUADS,
              "ps_quad_textured with a wide sColor0 is on the textured-quad path");
static_assert(draw_class_flags(facts(WR_SH_PS_QUAD_TEXTURED, WR_BLEND_PREMULT, true, false, true, true, false), false) == 0 &&
              draw_class_flags(facts(WR_SH_PS_QUAD_TEXTURED, WR_BLEND_PREMULT, true, false, true, false, true), false) == (WR_DF_XFORM | WR_DF_QUADS),
              "a textured quad takes its ids from the GPU buffer");
// brush_image
constexpr DrawFacts image = facts(WR_SH_BRUSH_IMAGE_ALPHA, WR_BLEND_PREMULT);
static_assert(aa_scan(image) == WR_AA_SCAN_BRUSH && draw_class_flags(image, true) == WR_DF_QUADS && draw_class_flags(image, false) == 0, "brush_image on RGBA8: QUADS under blend with AA");
constexpr DrawFacts image_rotated = facts(WR_SH_BRUSH_IMAGE_ALPHA, WR_BLEND_PREMULT, true, false, true, true);
static_assert(aa_scan(image_rotated) == WR_AA_SCAN_NONE && draw_class_flags(image_rotated, false) == (WR_DF_XFORM | WR_DF_QUADS), "brush_image: QUADS from unclean header ids without any scan");
static_assert(every_facts_of(WR_SH_BRUSH_IMAGE_DUAL, [](const DrawFacts& f) { return !(draw_class_flags(f, true) & WR_DF_QUADS) && aa_scan(f) == WR_AA_SCAN_NONE; }) &&
              draw_class_flags(facts(WR_SH_BRUSH_IMAGE_REPEAT_DUAL, WR_BLEND_DUAL_SRC), true) == WR_DF_QUADS,
              "BRUSH_IMAGE_DUAL never gives QUADS and is never scanned; its REPETITION twin does and is");
// a text run
constexpr DrawFacts text_rotated = facts(WR_SH_PS_TEXT_RUN, WR_BLEND_PREMULT, true, false, true, true);
static_assert(draw_class_flags(text_rotated, false) == (WR_DF_XFORM | WR_DF_QUADS) && draw_class_flags(facts(WR_SH_PS_TEXT_RUN, WR_BLEND_PREMULT, true, false, true), true) == 0,
              "a text run gives QUADS from the transform ids alone");
static_assert(every_facts([](const DrawFacts& f) { return !is_text_run(f.kind) || aa_scan(f) == WR_AA_SCAN_NONE; }), "a text run requests no scan");
// ps_split_composite
static_assert(every_facts_of(WR_SH_PS_SPLIT_COMPOSITE, [](const DrawFacts& f) { return draw_class_flags(f, true) == (WR_DF_XFORM | (f.rgba8 ? WR_DF_QUADS : 0)); }),
              "ps_split_composite gives XFORM always, and QUADS only on RGBA8");
// whatever the program
static_assert(every_facts([](const DrawFacts& f) { return f.rgba8 || !(draw_class_flags(f, true) & WR_DF_QUADS); }), "an R8 target never gives QUADS");
static_assert(every_facts([](const DrawFacts& f) { DrawFacts g = f; g.third_word = false; return (f.blend != WR_BLEND_NONE || aa_scan(f) == WR_AA_SCAN_NONE) && aa_scan(g) == WR_AA_SCAN_NONE; }),
              "blend NONE never scans, nor do instances without the third word");
static_assert(every_facts([](const DrawFacts& f) { return aa_scan(f) == WR_AA_SCAN_NONE || (draw_class_flags(f, true) & (WR_DF_SIMPLE | WR_DF_QUADS)) != (draw_class_flags(f, false) & (WR_DF_SIMPLE | WR_DF_QUADS)); }),
              "the bytes are scanned only where the answer changes the class");
static_assert(every_facts([](const DrawFacts& f) { return aa_scan(f) != WR_AA_SCAN_NONE || draw_class_flags(f, true) == draw_class_flags(f, false); }), "without a scan the answer does not enter");
static_assert(every_facts([](const DrawFacts& f) {
                return !!(draw_class_flags(f, false) & WR_DF_XFORM) == ((is_quad_prog(f.kind) ? f.complex_gpubuf : f.complex_headers) || f.kind == WR_SH_PS_SPLIT_COMPOSITE);
              }) && is_quad_prog(WR_SH_PS_QUAD_TEXTURED) && is_quad_prog(WR_SH_PS_QUAD_MASK) && is_quad_prog(WR_SH_PS_QUAD_MASK_FAST) && is_quad_prog(WR_SH_PS_QUAD_RADIAL_GRADIENT) &&
              is_quad_prog(WR_SH_PS_QUAD_CONIC_GRADIENT) && every_kind([](int k) { return !is_quad_prog(k) || k == WR_SH_PS_QUAD_TEXTURED || k == WR_SH_PS_QUAD_MASK || k == WR_SH_PS_QUAD_MASK_FAST || k == WR_SH_PS_QUAD_RADIAL_GRADIENT || k == WR_SH_PS_QUAD_CONIC_GRADIENT; }),
              "XFORM takes its ids from the GPU buffer for the five quad programs and from the headers for every other program");
// the raster stage's reads
static_assert(raster_read_mask(WR_SH_BRUSH_IMAGE, false) == ((1u << WR_S_COLOR0) | (1u << WR_S_COLOR1) | (1u << WR_S_COLOR2) | (1u << WR_S_CLIP_MASK)), "colour and mask samplers");
static_assert((raster_read_mask(WR_SH_BRUSH_BLEND, false) & raster_read_mask(WR_SH_CS_SVG_FILTER_NODE, true) & (1u << WR_S_GPU_CACHE)) != 0, "component-transfer tables");
static_assert((raster_read_mask(WR_SH_CS_RADIAL_GRADIENT, false) & ~raster_read_mask(WR_SH_CS_RADIAL_GRADIENT, true)) == (1u << WR_S_GPU_BUFFER_F),
              "gradient stops are read in place unless a table copy is promised");
}  // namespace wr_draw_class_cases
#endif
#endif
