// wrhip_k_pixels.h -- part of the gfx950 kernels of libwrhip: included by wrhip_kernels.h, in its order, and by nothing else.
// Per-pixel and per-row evaluators the raster stages share: blits, texture filters, gradients, filters, mix-blend, blur, clip masks, box shadows.
#pragma once

// Scatter queued texture uploads from the staging mirror to their textures.
// 8 workgroups per segment; 16-byte lanes where the rows allow it.
// `parts` workgroups per segment (the host sizes it for the largest segment of the batch: one per 64 KB, 8 .. 256)
// (the body: also run by the first workgroups of a flush's setup-carrying launch -- WrSetupArgs::up_*, "fused scatter" --, which takes the
// scatter off the frame's critical path: the setup stage reads whole-texture uploads of data textures straight from the staging mirror)
WR_DEVICE void wr_upload_body(const WrUploadSeg* __restrict__ segs, int n_segs, int parts, int bid) {
  const int si = bid / parts, part = bid % parts;
  if (si >= n_segs) return;
  const WrUploadSeg sg = segs[si];
  const size_t total = (size_t)sg.row_bytes * sg.rows;
  const bool vec = ((sg.row_bytes & 15) == 0) && ((sg.dst_stride & 15) == 0) && (((uintptr_t)sg.src & 15) == 0) && (((uintptr_t)sg.dst & 15) == 0);
  if (vec) {
    const size_t n16 = total >> 4, per_row = sg.row_bytes >> 4;
    for (size_t i = (size_t)part * blockDim.x + threadIdx.x; i < n16; i += (size_t)parts * blockDim.x) {
      size_t r = i / per_row, c = i - r * per_row;
      ((uint4*)((uint8_t*)sg.dst + r * sg.dst_stride))[c] = ((const uint4*)sg.src)[i];
    }
  } else {
    for (size_t i = (size_t)part * blockDim.x + threadIdx.x; i < total; i += (size_t)parts * blockDim.x) {
      size_t r = i / sg.row_bytes, c = i - r * sg.row_bytes;
      ((uint8_t*)sg.dst)[r * sg.dst_stride + c] = sg.src[i];
    }
  }
}
#ifndef WR_INST_ONLY      /* (not a template: defined by wrhip.hip alone, not by the instantiation units wrhip_inst.hip) */
__global__ void wr_upload_kernel(const WrUploadSeg* __restrict__ segs, int n_segs, int parts) {
  wr_upload_body(segs, n_segs, parts, (int)blockIdx.x);
}
#endif

// linear_blit's walk over the source (composite.h:342-418): srcUV = quantize(srcReq.origin (+ size when flipped) + srcDUV *
// (dstBounds.origin + 0.5)), stepped by srcDUV * 128 per pixel (init_interp lanes, then one add of 4 * srcDU per 4-pixel chunk)
// and per row.  wr_blit_walk_u(i) / wr_blit_walk_v(j): the coordinates, in 1/128 texel, of column i / row j of the dest bounds.
struct WrBlitWalk { float u0, v0, du, dv; };
WR_DEVICE WrBlitWalk wr_blit_walk(int srx0, int sry0, int srw, int srh, int drw, int drh, int bx0, int by0, int invert_x, int invert_y) {
  float u0 = float(srx0), v0 = float(sry0);
  float du = float(srw) / float(drw), dv = float(srh) / float(drh);
  if (invert_x) { u0 += float(srw); du = -du; }
  if (invert_y) { v0 += float(srh); dv = -dv; }
  u0 += du * (float(bx0) + 0.5f); v0 += dv * (float(by0) + 0.5f);
  u0 = u0 * 128.0f + (0.5f - 0.5f * 128.0f); v0 = v0 * 128.0f + (0.5f - 0.5f * 128.0f);
  du *= 128.0f; dv *= 128.0f;
  return WrBlitWalk{u0, v0, du, dv};
}
WR_DEVICE float wr_blit_walk_u(const WrBlitWalk& w, int i) {
  float lu = w.u0;
  for (int k = 0; k < (i & 3); k++) lu = lu + w.du;
  return wr_accum(lu, 4.0f * w.du, i >> 2);
}
WR_DEVICE float wr_blit_walk_v(const WrBlitWalk& w, int j) { return wr_accum(w.v0, w.dv, j); }

// BlitFramebuffer with scaling / flipping / format conversion (composite.h:62-283, 285-418); one thread per dest pixel.
#ifndef WR_INST_ONLY     /* (not a template: defined by wrhip.hip alone, not by the instantiation units wrhip_inst.hip) */
__global__ void wr_blit_kernel(WrBlitArgs a) {
  const int bw = a.bx1 - a.bx0, bh = a.by1 - a.by0;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)bw * bh) return;
  const int i = int(idx % bw), j = int(idx / bw);
  const int X = a.bx0 + i, Y = a.by0 + j;
  uint8_t* dp = (uint8_t*)a.dst + (size_t)(a.dry0 + Y) * a.dst_stride + (size_t)(a.drx0 + X) * a.dbpp;
  if (!a.linear) {
    // scale_row's stepping: the source column of dest column X is floor(srcWidth * X / dstWidth), rows likewise
    const int sx = a.srx0 + int((long long)a.srw * X / a.drw);
    const int syr = int((long long)a.srh * Y / a.drh);
    const int sy = a.invert_y ? a.sry0 + a.srh - 1 - syr : a.sry0 + syr;
    const uint8_t* sp = (const uint8_t*)a.src + (size_t)sy * a.src_stride + (size_t)sx * a.sbpp;
    if (a.composite && a.sbpp == 4 && a.dbpp == 4) {       // copy_row / scale_row<true>: src + dst - muldiv255(dst, alphas(src))
      uint32_t sv, dv;
      __builtin_memcpy(&sv, sp, 4); __builtin_memcpy(&dv, dp, 4);
      const uint32_t o = wr_blend_rgba8(WR_BLEND_PREMULT, dv, wr_unpack(sv), nullptr);
      __builtin_memcpy(dp, &o, 4);
      return;
    }
    if (a.sbpp == a.dbpp) { for (int k = 0; k < a.dbpp; k++) dp[k] = sp[k]; return; }
    // convert_pixel (composite.h:5-70)
    uint32_t v = 0;
    if (a.sbpp == 4) __builtin_memcpy(&v, sp, 4); else if (a.sbpp == 2) { uint16_t h; __builtin_memcpy(&h, sp, 2); v = h; } else v = sp[0];
    if (a.dbpp == 4) {
      const uint32_t o = a.sbpp == 1 ? ((v << 16) | 0xFF000000u) : (((v & 0x00FFu) << 16) | (v & 0xFF00u) | 0xFF000000u);
      __builtin_memcpy(dp, &o, 4);
    } else if (a.dbpp == 1) {
      dp[0] = a.sbpp == 4 ? uint8_t((v >> 16) & 0xFF) : uint8_t(v & 0xFF);
    } else {
      const uint16_t o = a.sbpp == 4 ? uint16_t(((v >> 16) & 0x00FF) | (v & 0xFF00)) : uint16_t(v);
      __builtin_memcpy(dp, &o, 2);
    }
    return;
  }
  const WrBlitWalk bw_ = wr_blit_walk(a.srx0, a.sry0, a.srw, a.srh, a.drw, a.drh, a.bx0, a.by0, a.invert_x, a.invert_y);
  const float lu = wr_blit_walk_u(bw_, i);
  const float lv = wr_blit_walk_v(bw_, j);
  WrTexDesc t;
  t.ptr = a.src; t.width = a.sw; t.height = a.sh; t.stride = a.sbpp == 4 ? a.src_stride / 4 : (a.sbpp == 2 ? a.src_stride / 2 : a.src_stride);
  t.format = a.sbpp == 4 ? WR_FMT_RGBA8 : (a.sbpp == 2 ? WR_FMT_RG8 : WR_FMT_R8); t.linear = 1; t.sw = float(a.sw); t.sh = float(a.sh);
  if (a.sbpp == 4) {
    const WrWide w = wr_sample_linear_rgba8(t, int(lu), int(lv));
    uint32_t o = wr_pack(w);
    if (a.composite) {                                       // linear_row_blit<true>
      uint32_t dv_;
      __builtin_memcpy(&dv_, dp, 4);
      o = wr_blend_rgba8(WR_BLEND_PREMULT, dv_, w, nullptr);
    }
    __builtin_memcpy(dp, &o, 4);
  } else if (a.sbpp == 2) {                                  // linear_row_blit(uint16_t*): textureLinearPackedRG8 -- the NV12 chroma plane's filter
    int v[4];
    wr_bilinear<2>(t, int(lu), int(lv), v);
    const uint16_t o = uint16_t(wr_pack1(uint32_t(v[0]) & 0xFFFF) | (wr_pack1(uint32_t(v[1]) & 0xFFFF) << 8));
    __builtin_memcpy(dp, &o, 2);
  } else {
    dp[0] = (uint8_t)wr_pack1(uint32_t(wr_sample_linear_r8(t, int(lu), int(lv))) & 0xFFFF);
  }
}
// ClearTexSubImage of an RG8 texture (clear_buffer<uint16_t>, gl.cc:2161-2188): `value` into the w x h texels from (x0, y0) on, which the
// host has cut to the texture; one thread per texel.
__global__ void wr_clear_rg8_kernel(uint8_t* dst, int stride, int x0, int y0, int w, int h, uint16_t value) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)w * h) return;
  const int i = int(idx % w), j = int(idx / w);
  __builtin_memcpy(dst + (size_t)(y0 + j) * stride + (size_t)(x0 + i) * 2, &value, 2);
}
#endif

// WrhipTapTexture (include/wrhip.h): two order-free 64-bit sums over the pixels of a texture rect -- pixel i = r * w + c of the rect
// with stored value v contributes mix(((u64)i << 32 | v) + C_j), mix = the splitmix64 finaliser -- and, against an expected
// texture, the histogram of per-pixel differences (the largest absolute channel difference: wrench's reftest measure).
// A read-only stream: a 256-thread workgroup per run of rows (WrTapArgs::rows_per_wg), 16-byte loads from the first 16-byte
// boundary of a row on where the expected row is aligned there too, single pixels before it, behind the last whole piece and
// wherever the two rows' alignments differ.  The sums stay in registers (a wave reduction, the four waves' sums added in LDS, then
// one 64-bit atomic per workgroup and word); differences are counted in an LDS histogram (equal pixels, the usual case, in a register instead) that leaves with one
// atomic per bin in use.  Integer sums commute: the result does not depend on the order the workgroups run in.
WR_DEVICE unsigned long long wr_tap_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
struct WrTapAcc { unsigned long long d0, d1; unsigned n0; };
WR_DEVICE uint32_t wr_tap_absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
// pixel `i` of the rect: value v, expected e (== v when nothing is expected); hist: the workgroup's 256 bins
WR_DEVICE void wr_tap_px(WrTapAcc& A, unsigned* hist, unsigned long long i, uint32_t v, uint32_t e) {
  const unsigned long long k = (i << 32) | v;
  A.d0 += wr_tap_mix(k + 0x9E3779B97F4A7C15ull);
  A.d1 += wr_tap_mix(k + 0xD1B54A32D192ED03ull);
  if (v == e) { A.n0++; return; }
  uint32_t d = wr_tap_absdiff(v & 0xFF, e & 0xFF);       // (R8 values have no more than this byte)
  d = (uint32_t)wr_imax((int)d, (int)wr_tap_absdiff((v >> 8) & 0xFF, (e >> 8) & 0xFF));
  d = (uint32_t)wr_imax((int)d, (int)wr_tap_absdiff((v >> 16) & 0xFF, (e >> 16) & 0xFF));
  d = (uint32_t)wr_imax((int)d, (int)wr_tap_absdiff(v >> 24, e >> 24));
  atomicAdd(&hist[d], 1u);
}
WR_DEVICE uint32_t wr_tap_load(const uint8_t* p, int bpp) {
  if (bpp == 1) return p[0];
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
// row r of the rect, thread t of nt
WR_DEVICE void wr_tap_row(const WrTapArgs& a, int r, int t, int nt, WrTapAcc& A, unsigned* hist) {
  const uint8_t* ps = a.src + (size_t)r * a.src_stride;
  const uint8_t* pe = a.exp ? a.exp + (size_t)r * a.exp_stride : nullptr;
  const unsigned long long i0 = (unsigned long long)r * (unsigned)a.w;
  const int bpp = a.bpp, ppv = 16 / bpp;
  // [0, head) single pixels, [head, tail0) 16-byte pieces, [tail0, w) single pixels
  int head = a.w;
  if (((uintptr_t)ps & (uintptr_t)(bpp - 1)) == 0) {
    const int h16 = (int)(((16 - ((uintptr_t)ps & 15)) & 15) / bpp);
    if (h16 < a.w && (!pe || (((uintptr_t)pe + (size_t)h16 * bpp) & 15) == 0)) head = h16;
  }
  const int nvec = (a.w - head) / ppv, tail0 = head + nvec * ppv;
  for (int c = t; c < nvec; c += nt) {
    const int p = head + c * ppv;
    const wr_u4 sv = wr_load16(ps + (size_t)p * bpp);
    const wr_u4 ev = pe ? wr_load16(pe + (size_t)p * bpp) : sv;
    const uint32_t sw[4] = {sv.x, sv.y, sv.z, sv.w}, ew[4] = {ev.x, ev.y, ev.z, ev.w};
    if (bpp == 4) {
#pragma unroll
      for (int k = 0; k < 4; k++) wr_tap_px(A, hist, i0 + (unsigned)(p + k), sw[k], ew[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++) wr_tap_px(A, hist, i0 + (unsigned)(p + k), (sw[k >> 2] >> (8 * (k & 3))) & 0xFF, (ew[k >> 2] >> (8 * (k & 3))) & 0xFF);
    }
  }
  const int nscalar = head + (a.w - tail0);
  for (int q = t; q < nscalar; q += nt) {
    const int p = q < head ? q : tail0 + (q - head);
    const uint32_t v = wr_tap_load(ps + (size_t)p * bpp, bpp);
    wr_tap_px(A, hist, i0 + (unsigned)p, v, pe ? wr_tap_load(pe + (size_t)p * bpp, bpp) : v);
  }
}
#ifndef WR_INST_ONLY      /* (not a template: defined by wrhip.hip alone, not by the instantiation units wrhip_inst.hip) */
__global__ void __launch_bounds__(256) wr_tap_kernel(WrTapArgs a) {
  const int r0 = (int)blockIdx.x * a.rows_per_wg, r1 = wr_imin(a.h, r0 + a.rows_per_wg);
  WrTapAcc A = {0ull, 0ull, 0u};
#ifdef WRHIP_HOSTSIM
  // (threads run one after the other: each adds what it saw straight to the slot)
  for (int r = r0; r < r1; r++) wr_tap_row(a, r, (int)threadIdx.x, (int)blockDim.x, A, a.hist);
  atomicAdd(&a.digest[0], A.d0); atomicAdd(&a.digest[1], A.d1);
  atomicAdd(&a.hist[0], A.n0);
#else
  __shared__ unsigned lh[256];
  __shared__ unsigned long long ld[2];
  lh[threadIdx.x] = 0u;
  if (threadIdx.x < 2) ld[threadIdx.x] = 0ull;
  __syncthreads();
  for (int r = r0; r < r1; r++) wr_tap_row(a, r, (int)threadIdx.x, 256, A, lh);
  for (int o = 32; o > 0; o >>= 1) {
    A.d0 += __shfl_down(A.d0, o);
    A.d1 += __shfl_down(A.d1, o);
    A.n0 += __shfl_down(A.n0, o);
  }
  // (the waves' sums meet in LDS: atomics on ONE address run one after the other chip-wide, 11-13 ns each -- at one per wave
  // and word the 17 k of a 4K window took 220 us against 29 us this way)
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&ld[0], A.d0); atomicAdd(&ld[1], A.d1);
    if (A.n0) atomicAdd(&lh[0], A.n0);
  }
  __syncthreads();
  if (threadIdx.x < 2) atomicAdd(&a.digest[threadIdx.x], ld[threadIdx.x]);
  const unsigned n = lh[threadIdx.x];
  if (n) atomicAdd(&a.hist[threadIdx.x], n);
#endif
}
#endif

// WrhipGrabTexture (include/wrhip.h): the pixels themselves, packed into the ticket's device slot (layout: WrGrabArgs).
// Full mode is the tap kernel's walk with a store behind every load: a 256-thread workgroup per run of rows of the rects laid end
// to end, 16-byte loads and stores from the source row's first 16-byte boundary on where the (tight) destination row is aligned
// there too, single pixels before it, behind the last whole piece and wherever the two disagree.  Rows are flipped and R and B
// exchanged on the way.
// Delta mode gives every 64 x 64 block of the rect a workgroup: a thread holds the block's 16-byte pieces it is responsible for in
// registers (four for RGBA8, one for R8; pieces count from the block's left edge, so that the retained copy and the slot entry --
// both the library's own, both 16-byte aligned there -- take whole stores whatever the texture's alignment is), compares them with
// the retained copy, and the block leaves -- record, pixels, retained copy -- only if a lane of it saw a difference: a ballot per
// wave, one LDS word per workgroup.  Its entry is the next free one (one atomic per CHANGED block on the slot's byte count), or its
// own index on a keyframe, where nothing is compared and nothing is counted.
WR_DEVICE void wr_grab_st16(void* p, const wr_u4& v) {
#ifdef WRHIP_HOSTSIM
  __builtin_memcpy(p, &v, 16);
#else
  typedef uint32_t wr_gu4 __attribute__((ext_vector_type(4)));
  *(__attribute__((address_space(1))) wr_gu4*)p = wr_gu4{v.x, v.y, v.z, v.w};
#endif
}
WR_DEVICE void wr_grab_st4(void* p, uint32_t v) {
#ifdef WRHIP_HOSTSIM
  __builtin_memcpy(p, &v, 4);
#else
  *(__attribute__((address_space(1))) uint32_t*)p = v;
#endif
}
WR_DEVICE uint32_t wr_grab_swap(uint32_t v) { return (v & 0xFF00FF00u) | ((v & 0xFFu) << 16) | ((v >> 16) & 0xFFu); }
// row g of the rects' rows laid end to end, thread t of nt
WR_DEVICE void wr_grab_row(const WrGrabArgs& a, int g, int t, int nt) {
  const int bpp = a.bpp, ppv = 16 / bpp;
  size_t off = 0;
  int i = 0, r = g;
  for (; i < a.nrects - 1 && r >= a.rects[i][3]; i++) { r -= a.rects[i][3]; off += (size_t)a.rects[i][2] * a.rects[i][3] * bpp; }
  const int w = a.rects[i][2], h = a.rects[i][3];
  const uint8_t* ps = a.tex + (size_t)(a.rects[i][1] + r) * a.tex_stride + (size_t)a.rects[i][0] * bpp;
  uint8_t* pd = a.slot + WR_GRAB_HEADER + off + (size_t)(a.flip ? h - 1 - r : r) * w * bpp;
  // [0, head) single pixels, [head, tail0) 16-byte pieces, [tail0, w) single pixels
  int head = w;
  const int h16 = (int)(((16 - ((uintptr_t)ps & 15)) & 15) / bpp);
  if (h16 < w && (((uintptr_t)pd + (size_t)h16 * bpp) & 15) == 0) head = h16;
  const int nvec = (w - head) / ppv, tail0 = head + nvec * ppv;
  for (int c = t; c < nvec; c += nt) {
    const int p = head + c * ppv;
    wr_u4 v = wr_load16(ps + (size_t)p * bpp);
    if (a.swap_rb) { v.x = wr_grab_swap(v.x); v.y = wr_grab_swap(v.y); v.z = wr_grab_swap(v.z); v.w = wr_grab_swap(v.w); }
    wr_grab_st16(pd + (size_t)p * bpp, v);
  }
  const int nscalar = head + (w - tail0);
  for (int q = t; q < nscalar; q += nt) {
    const int p = q < head ? q : tail0 + (q - head);
    if (bpp == 4) {
      const uint32_t v = wr_load4(ps + (size_t)p * 4);
      wr_grab_st4(pd + (size_t)p * 4, a.swap_rb ? wr_grab_swap(v) : v);
    } else {
      pd[p] = ps[p];
    }
  }
}
// delta: the geometry of block b, and piece `piece` of it (row-major, 64 * bpp / 16 pieces per block row)
struct WrGrabBlock { const uint8_t* ps; uint8_t* pk; int x0, y0, bw, bh; };
WR_DEVICE WrGrabBlock wr_grab_block(const WrGrabArgs& a, int b) {
  WrGrabBlock B;
  B.x0 = (b % a.bx) * WR_GRAB_BLOCK; B.y0 = (b / a.bx) * WR_GRAB_BLOCK;
  B.bw = wr_imin(WR_GRAB_BLOCK, a.rects[0][2] - B.x0); B.bh = wr_imin(WR_GRAB_BLOCK, a.rects[0][3] - B.y0);
  B.ps = a.tex + (size_t)(a.rects[0][1] + B.y0) * a.tex_stride + (size_t)(a.rects[0][0] + B.x0) * a.bpp;
  B.pk = a.keep + (size_t)B.y0 * a.keep_stride + (size_t)B.x0 * a.bpp;
  return B;
}
// -> the piece's pixels inside the block (0: none of it is), `v`: their bytes, zero beyond them; r, o: its row and byte offset in it
WR_DEVICE int wr_grab_piece(const WrGrabArgs& a, const WrGrabBlock& B, int piece, wr_u4& v, int& r, int& o) {
  const int bpp = a.bpp, ppv = 16 / bpp, ppr = WR_GRAB_BLOCK / ppv;
  r = piece / ppr;
  const int px0 = (piece % ppr) * ppv;
  o = px0 * bpp;
  const int n = r < B.bh ? wr_imax(0, wr_imin(ppv, B.bw - px0)) : 0;
  if (n == 0) return 0;
  const uint8_t* p = B.ps + (size_t)r * a.tex_stride + o;
  if (n == ppv && ((uintptr_t)p & 15) == 0) { v = wr_load16(p); return n; }
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (bpp == 4) {
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < n) w[k] = wr_load4(p + 4 * k);
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) if (k < n) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
  }
  v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
  return n;
}
WR_DEVICE bool wr_grab_differs(const wr_u4& v, const wr_u4& e) { return ((v.x ^ e.x) | (v.y ^ e.y) | (v.z ^ e.z) | (v.w ^ e.w)) != 0u; }
// the entry's record and where its pixels start
WR_DEVICE uint8_t* wr_grab_entry(const WrGrabArgs& a, const WrGrabBlock& B, unsigned index, bool write_record) {
  uint8_t* e = a.slot + WR_GRAB_HEADER + (size_t)index * WR_GRAB_ENTRY(a.bpp);
  if (write_record) wr_grab_st16(e, wr_u4{(uint32_t)B.x0, (uint32_t)B.y0, (uint32_t)B.bw, (uint32_t)B.bh});
  return e + 16;
}
#ifndef WR_INST_ONLY
__global__ void __launch_bounds__(256) wr_grab_pack_kernel(WrGrabArgs a) {
  const int t = (int)threadIdx.x;
  // (what the host knows of the slot's byte count is written here: everything in full mode and on a keyframe)
  if ((!a.delta || a.keyframe) && blockIdx.x == 0 && t == 0) wr_grab_st16(a.slot, wr_u4{a.payload, 0u, 0u, 0u});
  if (!a.delta) {
    int rows = 0;
    for (int i = 0; i < a.nrects; i++) rows += a.rects[i][3];
    const int g0 = (int)blockIdx.x * a.rows_per_wg, g1 = wr_imin(rows, g0 + a.rows_per_wg);
    for (int g = g0; g < g1; g++) wr_grab_row(a, g, t, (int)blockDim.x);
    return;
  }
  const int b = (int)blockIdx.x;
  const WrGrabBlock B = wr_grab_block(a, b);
  const int pieces = WR_GRAB_BLOCK * WR_GRAB_BLOCK * a.bpp / 16, pitch = WR_GRAB_BLOCK * a.bpp;
  const unsigned entry_bytes = (unsigned)WR_GRAB_ENTRY(a.bpp);
#ifdef WRHIP_HOSTSIM
  // (threads run one after the other: the first walks the block twice)
  if (t != 0) return;
  bool diff = a.keyframe != 0;
  wr_u4 v; int r, o;
  for (int piece = 0; piece < pieces && !diff; piece++)
    if (wr_grab_piece(a, B, piece, v, r, o)) diff = wr_grab_differs(v, wr_load16(B.pk + (size_t)r * a.keep_stride + o));
  if (!diff) return;
  const unsigned index = a.keyframe ? (unsigned)b : atomicAdd((unsigned*)a.slot, entry_bytes) / entry_bytes;
  uint8_t* px = wr_grab_entry(a, B, index, true);
  for (int piece = 0; piece < pieces; piece++)
    if (wr_grab_piece(a, B, piece, v, r, o)) { wr_grab_st16(px + (size_t)r * pitch + o, v); wr_grab_st16(B.pk + (size_t)r * a.keep_stride + o, v); }
#else
  __shared__ unsigned lw[2];           // [0]: a lane saw a difference; [1]: the entry the block takes
  wr_u4 v[4];
  int n[4], r[4], o[4];
  bool diff = false;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    n[k] = 0;
    const int piece = k * 256 + t;
    if (piece >= pieces) continue;
    n[k] = wr_grab_piece(a, B, piece, v[k], r[k], o[k]);
    if (n[k] && !a.keyframe) diff = diff || wr_grab_differs(v[k], wr_load16(B.pk + (size_t)r[k] * a.keep_stride + o[k]));
  }
  unsigned index = (unsigned)b;
  if (!a.keyframe) {
    if (t == 0) lw[0] = 0u;
    __syncthreads();
    if (__ballot(diff) != 0ull && (t & 63) == 0) lw[0] = 1u;
    __syncthreads();
    if (lw[0] == 0u) return;
    if (t == 0) lw[1] = atomicAdd((unsigned*)a.slot, entry_bytes) / entry_bytes;
    __syncthreads();
    index = lw[1];
  }
  uint8_t* px = wr_grab_entry(a, B, index, t == 0);
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (n[k]) { wr_grab_st16(px + (size_t)r[k] * pitch + o[k], v[k]); wr_grab_st16(B.pk + (size_t)r[k] * a.keep_stride + o[k], v[k]); }
#endif
}
// WRHIP_GRAB_PACKED: the delta path with every sent block written as a packed entry (wr_grab_codec.h; the contract is in
// include/wrhip.h).  Geometry, piece ownership and the compare with the retained copy are wr_grab_pack_kernel's.  A block that is
// sent is staged in LDS at the pitch of a plain entry, zeros beyond the cut block, and then looked at in raster order: thread t has
// the 16 pixels of row t / 4 from column 16 * (t & 3) on, so that the predecessor of its first pixel -- the pixel to the left, or the
// last valid one of the row above -- is one LDS read.  The run starts a thread found are 16 bits of the row's bitmap word and a
// count; the counts are scanned across the wave by lane shifts and across the four waves through four LDS words, which gives n and
// where each thread's values go among the n.  n decides the mode and the entry's size, ONE returning atomic on the slot's byte count
// takes the entry (keyframes too: entries differ in size, so entry i is not block i), and what leaves for the slot leaves as
// 16-byte stores: a RUNS body is put together in a second LDS buffer and copied out, a RAW body is the registers the pieces were
// loaded into.  32 KB of LDS per workgroup.
#ifndef WRHIP_HOSTSIM
typedef uint32_t wr_lu4 __attribute__((ext_vector_type(4)));
typedef uint16_t __attribute__((may_alias)) wr_u16a;
template <int BPP> WR_DEVICE uint32_t wr_grab_staged(const wr_lu4* stage, int r, int c) {
  return BPP == 4 ? ((const uint32_t*)stage)[r * WR_GRAB_BLOCK + c] : (uint32_t)((const uint8_t*)stage)[r * WR_GRAB_BLOCK + c];
}
// (KEEP false: the retained copy is left as it is -- the scroll grab's pack launch, whose other workgroups are reading it)
template <int BPP, bool KEEP = true> WR_DEVICE void wr_grab_pack_runs(const WrGrabArgs& a, const WrGrabBlock& B, int t, wr_lu4* stage, wr_lu4* outb, unsigned* lw) {
  constexpr int NP = BPP == 4 ? 4 : 1;          // 16-byte pieces of the block per thread
  wr_u4 v[NP];
  int n[NP], r[NP], o[NP];
  bool diff = false;
#pragma unroll
  for (int k = 0; k < NP; k++) {
    const int piece = k * 256 + t;
    v[k] = wr_u4{0u, 0u, 0u, 0u};
    n[k] = wr_grab_piece(a, B, piece, v[k], r[k], o[k]);
    if (n[k] && !a.keyframe) diff = diff || wr_grab_differs(v[k], wr_load16(B.pk + (size_t)r[k] * a.keep_stride + o[k]));
    stage[piece] = wr_lu4{v[k].x, v[k].y, v[k].z, v[k].w};
  }
  // lw[0]: the block is sent; lw[1..4]: the waves' run starts; lw[5]: the entry's offset in the payload
  if (t == 0) lw[0] = a.keyframe ? 1u : 0u;
  __syncthreads();
  if (__ballot(diff) != 0ull && (t & 63) == 0) lw[0] = 1u;
  __syncthreads();
  if (lw[0] == 0u) return;
  if (KEEP) {
#pragma unroll
    for (int k = 0; k < NP; k++)
      if (n[k]) wr_grab_st16(B.pk + (size_t)r[k] * a.keep_stride + o[k], v[k]);
  }
  // this thread's 16 pixels in raster order, and which of them start a run
  const int row = t >> 2, c0 = (t & 3) * 16;
  uint32_t px[16];
  if (BPP == 4) {
#pragma unroll
    for (int q = 0; q < 4; q++) { const wr_lu4 w = stage[4 * t + q]; px[4 * q] = w.x; px[4 * q + 1] = w.y; px[4 * q + 2] = w.z; px[4 * q + 3] = w.w; }
  } else {
    const wr_lu4 w = stage[t];
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 16; j++) px[j] = (ww[j >> 2] >> (8 * (j & 3))) & 0xFFu;
  }
  uint32_t prev = 0u;
  if (c0 > 0) prev = wr_grab_staged<BPP>(stage, row, c0 - 1);
  else if (row > 0) prev = wr_grab_staged<BPP>(stage, row - 1, B.bw - 1);
  bool has_prev = t != 0;
  unsigned m = 0u;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const bool valid = row < B.bh && c0 + j < B.bw;
    if (valid && (!has_prev || px[j] != prev)) m |= 1u << j;
    prev = px[j]; has_prev = true;
  }
  const unsigned cnt = (unsigned)__popc(m);
  const int lane = t & 63, wave = t >> 6;
  unsigned inc = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const unsigned u = __shfl_up(inc, d); if (lane >= d) inc += u; }
  if (lane == 63) lw[1 + wave] = inc;
  __syncthreads();
  unsigned before = 0u, total = 0u;
#pragma unroll
  for (int w = 0; w < 4; w++) { const unsigned s = lw[1 + w]; if (w < wave) before += s; total += s; }
  // the mode (include/wrhip.h): one run start is SOLID; RUNS if that is smaller than RAW
  const unsigned raw = (unsigned)WR_GRAB_ENTRY(BPP);
  const unsigned body = (8u * (unsigned)B.bh + total * BPP + 15u) & ~15u;
  const unsigned mode = total == 1u ? 1u : (16u + body < raw ? 2u : 0u);
  const unsigned size = mode == 1u ? 16u : mode == 2u ? 16u + body : raw;
  if (t == 0) lw[5] = atomicAdd((unsigned*)a.slot, size);
  if (mode == 2u) {
    uint8_t* ob = (uint8_t*)outb;
    if (row < B.bh) ((wr_u16a*)ob)[4 * row + (t & 3)] = (uint16_t)m;
    unsigned at = 8u * (unsigned)B.bh + (before + inc - cnt) * BPP;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (!((m >> j) & 1u)) continue;
      if (BPP == 4) *(uint32_t*)(ob + at) = px[j]; else ob[at] = (uint8_t)px[j];
      at += BPP;
    }
    const unsigned end = 8u * (unsigned)B.bh + total * BPP;
    if (t < 16 && end + (unsigned)t < body) ob[end + t] = 0;
  }
  __syncthreads();
  uint8_t* e = a.slot + WR_GRAB_HEADER + lw[5];
  if (t == 0) wr_grab_st16(e, wr_u4{(uint32_t)B.x0, (uint32_t)B.y0, (uint32_t)B.bw | (uint32_t)B.bh << 8 | mode << 16, mode == 1u ? px[0] : mode == 2u ? total : 0u});
  if (mode == 2u) {
    for (unsigned p = (unsigned)t; p < body / 16u; p += 256u) { const wr_lu4 w = outb[p]; wr_grab_st16(e + 16 + 16 * (size_t)p, wr_u4{w.x, w.y, w.z, w.w}); }
  } else if (mode == 0u) {
#pragma unroll
    for (int k = 0; k < NP; k++) wr_grab_st16(e + 16 + 16 * (size_t)(k * 256 + t), v[k]);
  }
}
#endif
__global__ void __launch_bounds__(256) wr_grab_pack_runs_kernel(WrGrabArgs a) {
  const int t = (int)threadIdx.x;
  const WrGrabBlock B = wr_grab_block(a, (int)blockIdx.x);
#ifdef WRHIP_HOSTSIM
  // (threads run one after the other: the first does it all, through the serial encoder of wr_grab_codec.h)
  if (t != 0) return;
  const int pieces = WR_GRAB_BLOCK * WR_GRAB_BLOCK * a.bpp / 16;
  bool diff = a.keyframe != 0;
  wr_u4 v; int r, o;
  for (int piece = 0; piece < pieces && !diff; piece++)
    if (wr_grab_piece(a, B, piece, v, r, o)) diff = wr_grab_differs(v, wr_load16(B.pk + (size_t)r * a.keep_stride + o));
  if (!diff) return;
  uint8_t entry[WR_GRAB_ENTRY(4)];
  const unsigned size = (unsigned)wr_gc_encode_block(B.ps, (size_t)a.tex_stride, B.x0, B.y0, B.bw, B.bh, a.bpp, entry);
  __builtin_memcpy(a.slot + WR_GRAB_HEADER + atomicAdd((unsigned*)a.slot, size), entry, size);
  for (int piece = 0; piece < pieces; piece++)
    if (wr_grab_piece(a, B, piece, v, r, o)) wr_grab_st16(B.pk + (size_t)r * a.keep_stride + o, v);
#else
  __shared__ wr_lu4 stage[1024], outb[1024];
  __shared__ unsigned lw[8];
  if (a.bpp == 4) wr_grab_pack_runs<4>(a, B, t, stage, outb, lw);
  else wr_grab_pack_runs<1>(a, B, t, stage, outb, lw);
#endif
}
// WrhipPutTexturePayload (include/wrhip.h; WrPutPayloadArgs): the pack kernels the other way -- a delta, packed or scroll payload in
// the staging mirror becomes the bytes of its blocks in a texture rect.  The host has checked every entry and left an index
// (wr_grab_codec.h, wr_gc_put_index), so no workgroup walks the payload and nothing read here decides an address unchecked.  Both
// kernels keep wr_grab_pack_runs' ownership: thread t of 256 has the 16 pixels of block row t / 4 from column 16 * (t & 3) on, as
// pieces of 16 bytes (four for RGBA8, one for R8).  A piece that lies whole inside the cut block and whose TEXTURE address is a
// multiple of 16 is one 16-byte load or store; any other piece goes pixel by pixel, and only its pixels inside the cut block are
// touched.  (The rect's origin is arbitrary: with rect.x = 3 no RGBA8 piece is aligned.)
//   copy    wr_put_copy_kernel, a workgroup per block COLUMN that has COPY entries.  COPY sources overlap their own block, other
//           COPY blocks and blocks that the patch pass writes, so a workgroup per block cannot be in place; columns share no byte.
//           The workgroup walks its column in the in-place order (ascending y for dy > 0, descending for dy < 0).  Per block: all
//           source pieces into registers, a barrier, the stores.  One barrier is enough: in that order a block's stores lie wholly
//           on the side of every LATER block's source that the scroll came from, and a later block's stores follow the barrier that
//           follows every earlier load.  No snapshot, no scratch memory, no LDS.
//   patch   wr_put_patch_kernel, a workgroup per entry that is no COPY.  SOLID: the record's value.  RAW and plain entries: the
//           body's pieces, which are 16-byte aligned in the mirror.  RUNS: the bitmap words and the values go to LDS as 16-byte
//           pieces; a thread's 16 bits of its row's word give its count of run starts, the counts are scanned as the encoder scans
//           them (lane shifts in a wave, four LDS words across the waves), and pixel j's value is values[starts before the thread +
//           popcount(bits up to j) - 1].  16.5 KB of LDS.
// Nothing is atomic, nothing spills (tests/test_put_payload.py reads the code object).
WR_DEVICE wr_u4 wr_put_ld_piece(const uint8_t* p, int n, int bpp) {
  if (n == 16 / bpp && ((uintptr_t)p & 15) == 0) return wr_load16(p);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (bpp == 4) {
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < n) w[k] = wr_load4(p + 4 * k);
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) if (k < n) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
  }
  return wr_u4{w[0], w[1], w[2], w[3]};
}
WR_DEVICE void wr_put_st_piece(uint8_t* p, const wr_u4& v, int n, int bpp) {
  if (n == 16 / bpp && ((uintptr_t)p & 15) == 0) { wr_grab_st16(p, v); return; }
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  if (bpp == 4) {
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < n) wr_grab_st4(p + 4 * k, w[k]);
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) if (k < n) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  }
}
// the pixels of piece k of thread t's 16 that lie inside a cut block of w x h
template <int BPP> WR_DEVICE int wr_put_piece_n(int t, int k, int w, int h) {
  constexpr int PPV = 16 / BPP;
  return (t >> 2) < h ? wr_imax(0, wr_imin(PPV, w - ((t & 3) * 16 + k * PPV))) : 0;
}
#ifndef WRHIP_HOSTSIM
template <int BPP> WR_DEVICE void wr_put_copy_column(const WrPutPayloadArgs& a, int t) {
  constexpr int NP = BPP == 4 ? 4 : 1;
  const uint32_t* starts = a.index + a.n_patch;
  const uint32_t* blocks = starts + a.n_cols + 1;
  const uint32_t b0 = starts[blockIdx.x], b1 = starts[blockIdx.x + 1];
  const int row = t >> 2, c0 = (t & 3) * 16;
  for (uint32_t b = b0; b < b1; b++) {
    const uint32_t word = blocks[b];
    const int x = (int)(word & 0xFFFFu) * WR_GRAB_BLOCK, y = (int)(word >> 16) * WR_GRAB_BLOCK;
    const int w = wr_imin(WR_GRAB_BLOCK, a.rw - x), h = wr_imin(WR_GRAB_BLOCK, a.rh - y);
    uint8_t* d = a.tex + (size_t)(a.ry + y + row) * a.tex_stride + (size_t)(a.rx + x + c0) * BPP;
    const uint8_t* s = d + (long long)a.dy * a.tex_stride;
    wr_u4 v[NP];
    int n[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) {
      n[k] = wr_put_piece_n<BPP>(t, k, w, h);
      v[k] = wr_u4{0u, 0u, 0u, 0u};
      if (n[k]) v[k] = wr_put_ld_piece(s + 16 * k, n[k], BPP);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NP; k++) if (n[k]) wr_put_st_piece(d + 16 * k, v[k], n[k], BPP);
  }
}
template <int BPP> WR_DEVICE void wr_put_patch_entry(const WrPutPayloadArgs& a, int t, wr_lu4* body, unsigned* lw) {
  constexpr int NP = BPP == 4 ? 4 : 1;
  const uint8_t* e = a.payload + a.index[blockIdx.x];
  const wr_u4 rec = wr_load16(e);
  const int x = (int)rec.x, y = (int)rec.y;
  int w = (int)rec.z, h = (int)rec.w;
  unsigned mode = 0u, aux = 0u;
  if (a.packed) { w = (int)(rec.z & 0xFFu); h = (int)((rec.z >> 8) & 0xFFu); mode = rec.z >> 16; aux = rec.w; }
  const int row = t >> 2, c0 = (t & 3) * 16;
  uint8_t* d = a.tex + (size_t)(a.ry + y + row) * a.tex_stride + (size_t)(a.rx + x + c0) * BPP;
  wr_u4 v[NP];
  int n[NP];
#pragma unroll
  for (int k = 0; k < NP; k++) { n[k] = wr_put_piece_n<BPP>(t, k, w, h); v[k] = wr_u4{0u, 0u, 0u, 0u}; }
  if (mode == 0u) {
    // (a body row is 64 pixels: thread t's 16 are pieces NP * t ... of the body)
#pragma unroll
    for (int k = 0; k < NP; k++) if (n[k]) v[k] = wr_load16(e + 16 + 16 * (size_t)(NP * t + k));
  } else if (mode == 1u) {
    const uint32_t f = BPP == 4 ? aux : (aux & 0xFFu) * 0x01010101u;
#pragma unroll
    for (int k = 0; k < NP; k++) v[k] = wr_u4{f, f, f, f};
  } else {
    const unsigned pieces = (8u * (unsigned)h + aux * BPP + 15u) / 16u;
    for (unsigned p = (unsigned)t; p < pieces; p += 256u) { const wr_u4 q = wr_load16(e + 16 + 16 * (size_t)p); body[p] = wr_lu4{q.x, q.y, q.z, q.w}; }
    __syncthreads();
    unsigned m16 = 0u;
    if (row < h) m16 = (((const uint32_t*)body)[2 * row + (c0 >> 5)] >> (c0 & 31)) & 0xFFFFu;
    const unsigned cnt = (unsigned)__popc(m16);
    const int lane = t & 63, wave = t >> 6;
    unsigned inc = cnt;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const unsigned u = __shfl_up(inc, s); if (lane >= s) inc += u; }
    if (lane == 63) lw[wave] = inc;
    __syncthreads();
    unsigned before = 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) if (q < wave) before += lw[q];
    const unsigned base = before + inc - cnt;
    const uint8_t* values = (const uint8_t*)body + 8 * h;
    uint32_t px[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      px[j] = 0u;
      if (row < h && c0 + j < w) {
        const unsigned i = base + (unsigned)__popc(m16 & ((2u << j) - 1u)) - 1u;
        px[j] = BPP == 4 ? ((const uint32_t*)values)[i] : (uint32_t)values[i];
      }
    }
    if (BPP == 4) {
#pragma unroll
      for (int k = 0; k < NP; k++) v[k] = wr_u4{px[4 * k], px[4 * k + 1], px[4 * k + 2], px[4 * k + 3]};
    } else {
      uint32_t ww[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 16; j++) ww[j >> 2] |= px[j] << (8 * (j & 3));
      v[0] = wr_u4{ww[0], ww[1], ww[2], ww[3]};
    }
  }
#pragma unroll
  for (int k = 0; k < NP; k++) if (n[k]) wr_put_st_piece(d + 16 * k, v[k], n[k], BPP);
}
#endif
__global__ void __launch_bounds__(256) wr_put_copy_kernel(WrPutPayloadArgs a) {
  const int t = (int)threadIdx.x;
#ifdef WRHIP_HOSTSIM
  // (threads run one after the other: the first applies the column's blocks through the serial decoder of wr_grab_codec.h)
  if (t != 0) return;
  const uint32_t* starts = a.index + a.n_patch;
  const uint32_t* blocks = starts + a.n_cols + 1;
  uint8_t* rect = a.tex + (size_t)a.ry * a.tex_stride + (size_t)a.rx * a.bpp;
  for (uint32_t b = starts[blockIdx.x]; b < starts[blockIdx.x + 1]; b++) {
    const int x = (int)(blocks[b] & 0xFFFFu) * WR_GRAB_BLOCK, y = (int)(blocks[b] >> 16) * WR_GRAB_BLOCK;
    wr_gc_copy(WrGrabCopy{x, y, wr_imin(WR_GRAB_BLOCK, a.rw - x), wr_imin(WR_GRAB_BLOCK, a.rh - y)}, a.dy, a.bpp, rect, (size_t)a.tex_stride);
  }
#else
  if (a.bpp == 4) wr_put_copy_column<4>(a, t);
  else wr_put_copy_column<1>(a, t);
#endif
}
__global__ void __launch_bounds__(256) wr_put_patch_kernel(WrPutPayloadArgs a) {
  const int t = (int)threadIdx.x;
#ifdef WRHIP_HOSTSIM
  // (threads run one after the other: the first patches the entry through the serial decoder of wr_grab_codec.h)
  if (t != 0) return;
  const uint32_t off = a.index[blockIdx.x];
  WrGrabEntry E;
  wr_gc_entry(a.payload + off, (size_t)WR_GC_HEADER + a.count - off, a.bpp, a.packed != 0, a.rw, a.rh, &E, true);
  wr_gc_patch(a.payload + off, E, a.bpp, a.tex + (size_t)a.ry * a.tex_stride + (size_t)a.rx * a.bpp, (size_t)a.tex_stride);
#else
  __shared__ wr_lu4 body[1056];        // a RUNS body at its largest: 64 bitmap words and 4096 RGBA8 values
  __shared__ unsigned lw[4];
  if (a.bpp == 4) wr_put_patch_entry<4>(a, t, body, lw);
  else wr_put_patch_entry<1>(a, t, body, lw);
#endif
}
// WrhipGrabTextureScaled (include/wrhip.h; the launch: WrGrabScaleArgs): a workgroup per 64 x 64 tile of the launch's top level.
//   coords  (modes 0, 1) the source coordinate of each of the tile's columns and rows, once, into LDS: the blit kernel's own walk
//           (wr_blit_walk_u / _v -- wr_accum is not cheap) in mode 0, scale_blit's integer stepping in mode 1
//   fill    the tile's pixels: thread t has pixels t, t + 256, ... in row-major order, so a wave fills a row of 64 words -- one
//           linear_blit tap of the texture each (wr_sample_linear_rgba8: clamped at the TEXTURE's edges, plain global loads), a
//           copied texel, or the 2 x 2 texels of the level above under the 2:1 rule (wr_bilerp_half_rgba8)
//   halve   `steps` times, a barrier in between: level k of the tile (pitch 64 >> k words) alternates between the buffers `a`
//           and `b`; a thread reads the 2 x 2 texels of an output as two 8-byte words.  Pitch 64: the 32 lanes of a half-wave read
//           one whole 256-byte bank row each time -- no conflicts; the two smaller levels (a quarter and a sixteenth of the
//           work) have rows 2 j and 2 j + 2 of the level on the same banks: 2- and 4-way.
//   store   what is left, (64 >> steps) pixels square, cut to the level: 16-byte stores for every 4 pixels of a row that start
//           on a 16-byte boundary of the destination, single pixels otherwise; the last launch of a grab flips the rows and
//           exchanges R and B here and writes the slot's header.
// Each phase is a function of the thread's number.  The device runs them with barriers between; the host simulation, whose
// threads run one after the other, has thread 0 run each phase for every thread number in turn.
struct WrGrabScaleTile { uint32_t a[WR_SCALE_TILE * WR_SCALE_TILE]; uint32_t b[WR_SCALE_TILE * WR_SCALE_TILE / 4]; int qx[WR_SCALE_TILE], qy[WR_SCALE_TILE]; };
struct WrGrabScaleGeom { int x0, y0, cw, ch; };      // the workgroup's tile of the top level: origin, size cut to the level
WR_DEVICE WrGrabScaleGeom wr_grab_scale_geom(const WrGrabScaleArgs& a, int b) {
  WrGrabScaleGeom g;
  g.x0 = (b % a.tiles_x) * WR_SCALE_TILE; g.y0 = (b / a.tiles_x) * WR_SCALE_TILE;
  g.cw = wr_imin(WR_SCALE_TILE, a.tw - g.x0); g.ch = wr_imin(WR_SCALE_TILE, a.th - g.y0);
  return g;
}
WR_DEVICE void wr_grab_scale_coords(const WrGrabScaleArgs& a, const WrGrabScaleGeom& g, WrGrabScaleTile& T, int t) {
  if (a.mode == 2 || t >= 2 * WR_SCALE_TILE) return;
  const bool row = t >= WR_SCALE_TILE;
  const int k = row ? t - WR_SCALE_TILE : t;
  if (k >= (row ? g.ch : g.cw)) return;
  if (a.mode == 1) {
    // scale_row's stepping (wr_blit_kernel): the source column of dest column X is floor(srcWidth * X / dstWidth), rows likewise
    if (row) T.qy[k] = a.ry + int((long long)a.rh * (g.y0 + k) / a.th);
    else T.qx[k] = a.rx + int((long long)a.rw * (g.x0 + k) / a.tw);
    return;
  }
  const WrBlitWalk w = wr_blit_walk(a.rx, a.ry, a.rw, a.rh, a.tw, a.th, 0, 0, 0, 0);
  if (row) T.qy[k] = int(wr_blit_walk_v(w, g.y0 + k));
  else T.qx[k] = int(wr_blit_walk_u(w, g.x0 + k));
}
WR_DEVICE void wr_grab_scale_fill(const WrGrabScaleArgs& a, const WrGrabScaleGeom& g, WrGrabScaleTile& T, int t) {
  WrTexDesc d;
  d.ptr = a.src; d.width = a.sw; d.height = a.sh; d.stride = a.src_stride / 4;
  d.format = WR_FMT_RGBA8; d.linear = 1; d.sw = float(a.sw); d.sh = float(a.sh);
  for (int p = t; p < WR_SCALE_TILE * WR_SCALE_TILE; p += 256) {
    const int c = p % WR_SCALE_TILE, r = p / WR_SCALE_TILE;
    if (c >= g.cw || r >= g.ch) continue;
    uint32_t v;
    if (a.mode == 0) {
      v = wr_pack(wr_sample_linear_rgba8(d, T.qx[c], T.qy[r]));
    } else if (a.mode == 1) {
      v = wr_load4(a.src + (size_t)T.qy[r] * a.src_stride + (size_t)T.qx[c] * 4);
    } else {
      const uint8_t* s = a.src + (size_t)(2 * (g.y0 + r)) * a.src_stride + (size_t)(2 * (g.x0 + c)) * 4;
      v = wr_pack(wr_bilerp_half_rgba8(wr_load4(s), wr_load4(s + 4), wr_load4(s + a.src_stride), wr_load4(s + a.src_stride + 4)));
    }
    T.a[p] = v;
  }
}
// level k + 1 of the tile (pitch `pitch` / 2, cw / 2 x ch / 2 pixels) from level k
WR_DEVICE void wr_grab_scale_halve(const uint32_t* src, uint32_t* dst, int pitch, int cw, int ch, int t) {
  const int hp = pitch / 2;
  for (int p = t; p < hp * hp; p += 256) {
    const int i = p % hp, j = p / hp;
    if (i >= cw / 2 || j >= ch / 2) continue;
    uint32_t r0[2], r1[2];
    __builtin_memcpy(r0, __builtin_assume_aligned(src + (2 * j) * pitch + 2 * i, 8), 8);
    __builtin_memcpy(r1, __builtin_assume_aligned(src + (2 * j + 1) * pitch + 2 * i, 8), 8);
    dst[p] = wr_pack(wr_bilerp_half_rgba8(r0[0], r0[1], r1[0], r1[1]));
  }
}
// the tile's last level (pitch `pitch`, ow x oh pixels) to its place in the launch's output level
WR_DEVICE void wr_grab_scale_store(const WrGrabScaleArgs& a, const WrGrabScaleGeom& g, const uint32_t* src, int pitch, int t) {
  const int lw = a.tw >> a.steps, lh = a.th >> a.steps;            // the output level
  const int ox = g.x0 >> a.steps, oy = g.y0 >> a.steps, ow = g.cw >> a.steps, oh = g.ch >> a.steps;
  for (int p = t; p < ow * oh; p += 256) {
    const int c = p % ow, r = p / ow;
    const int dr = a.last && a.flip ? lh - 1 - (oy + r) : oy + r;
    const size_t at = (size_t)dr * lw + (size_t)(ox + c);          // in pixels; `dst` is 16-byte aligned
    const int c4 = c - (int)(at & 3);                              // where the 16-byte piece this pixel lies in starts in the tile's row
    const bool whole = c4 >= 0 && c4 + 4 <= ow;
    if (whole && c != c4) continue;                                // (stored by the piece's first pixel)
    const uint32_t* s = src + r * pitch + c;
    if (whole) {
      wr_u4 v{s[0], s[1], s[2], s[3]};
      if (a.last && a.swap_rb) { v.x = wr_grab_swap(v.x); v.y = wr_grab_swap(v.y); v.z = wr_grab_swap(v.z); v.w = wr_grab_swap(v.w); }
      wr_grab_st16(a.dst + 4 * at, v);
    } else {
      wr_grab_st4(a.dst + 4 * at, a.last && a.swap_rb ? wr_grab_swap(s[0]) : s[0]);
    }
  }
}
#ifdef WRHIP_HOSTSIM
#define WR_SCALE_PHASE(call) for (int t = 0; t < 256; t++) { call; }
#else
#define WR_SCALE_PHASE(call) { call; } __syncthreads();
#endif
__global__ void __launch_bounds__(256) wr_grab_scale_kernel(WrGrabScaleArgs a) {
  const WrGrabScaleGeom g = wr_grab_scale_geom(a, (int)blockIdx.x);
#ifdef WRHIP_HOSTSIM
  if (threadIdx.x != 0) return;
  WrGrabScaleTile T;
#else
  __shared__ WrGrabScaleTile T;
  const int t = (int)threadIdx.x;
#endif
  WR_SCALE_PHASE(wr_grab_scale_coords(a, g, T, t))
  WR_SCALE_PHASE(wr_grab_scale_fill(a, g, T, t))
  uint32_t* from = T.a;
  uint32_t* to = T.b;
  for (int k = 0; k < a.steps; k++) {
    WR_SCALE_PHASE(wr_grab_scale_halve(from, to, WR_SCALE_TILE >> k, g.cw >> k, g.ch >> k, t))
    uint32_t* const was = from; from = to; to = was;
  }
  WR_SCALE_PHASE(wr_grab_scale_store(a, g, from, WR_SCALE_TILE >> a.steps, t);
                 if (a.last && blockIdx.x == 0 && t == 0) wr_grab_st16(a.slot, wr_u4{a.payload, 0u, 0u, 0u}))
}

// WrhipGrabTextureTensor (include/wrhip.h; WrTensorOut): the pixels of a grab stored as tensor elements in the caller's memory.
// The pack kernel writes the bytes it reads; this writes 1 x (U8, 3 channels) to 4 x (F32, 4 channels) of them, so the work is cut
// along the DESTINATION: a thread owns a group of G = 16 / element size consecutive pixels of one output row (4 for F32, 8 for F16
// and BF16, 16 for U8) and stores 16 bytes per plane (CHW) or `channels` x 16 contiguous bytes (HWC).  That holds where dst and the
// byte strides are multiples of 16 (WrTensorOut::vec): groups count from the row's start, the row's last w % G pixels leave as
// single elements, a thread per pixel.  Any other geometry takes single elements throughout.  The formats and channel counts are
// template parameters, so that a group's pixels and words stay in registers under constant indices; the kernels branch on them once.
#include "wr_tensor_round.h"
constexpr int wr_tensor_elem(int dt) { return dt == WR_TENSOR_U8 ? 1 : dt == WR_TENSOR_F32 ? 4 : 2; }
// the bits of output channel c of the pixel whose stored word is px
template <int DT> WR_DEVICE uint32_t wr_tensor_bits(const WrTensorOut& o, uint32_t px, int c) {
  const uint32_t v = (px >> o.shift[c]) & 0xFFu;
  if (DT == WR_TENSOR_U8) return v;
  const float x = (float)v * o.scale[c] + o.bias[c];      // (two roundings: the build does not contract them)
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  if (DT == WR_TENSOR_F32) return u;
#ifdef WRHIP_HOSTSIM
  return DT == WR_TENSOR_F16 ? wr_f32_to_f16_bits(u) : wr_f32_to_bf16_bits(u);
#else
  // (the device's own converts round as wr_tensor_round.h does -- nearest even, f16 subnormals kept, overflow to infinity; the tests
  // compare them with numpy bit for bit.  As integer arithmetic the f16 rounding made the F16 grab of a 4K window VALU-bound)
  uint16_t h;
  if (DT == WR_TENSOR_F16) { const _Float16 f = (_Float16)x; __builtin_memcpy(&h, &f, 2); }
  else { const __bf16 f = (__bf16)x; __builtin_memcpy(&h, &f, 2); }
  return h;
#endif
}
// one pixel, element by element
template <int DT> WR_DEVICE void wr_tensor_put_pixel(const WrTensorOut& o, int y, int x, uint32_t px) {
  constexpr int E = wr_tensor_elem(DT);
#pragma unroll
  for (int c = 0; c < 4; c++) {
    if (c < o.channels) {
      const long long e = o.hwc ? (long long)y * o.row_stride + (long long)x * o.channels + c : c * o.plane_stride + (long long)y * o.row_stride + x;
      const uint32_t b = wr_tensor_bits<DT>(o, px, c);
      uint8_t* p = o.dst + e * E;
      if (E == 1) *p = (uint8_t)b;
      else if (E == 2) *(uint16_t*)p = (uint16_t)b;
      else *(uint32_t*)p = b;
    }
  }
}
// the group of G pixels px[0 .. G) that starts at x0, a multiple of G, of output row y (WrTensorOut::vec)
template <int DT, int CH> WR_DEVICE void wr_tensor_put_group(const WrTensorOut& o, int y, int x0, const uint32_t* px) {
  constexpr int E = wr_tensor_elem(DT), G = 16 / E;
#pragma unroll
  for (int k = 0; k < CH; k++) {
    // HWC: the k-th 16 bytes of the group's G * CH elements, pixel after pixel; CHW: plane k
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < G; i++) {
      const int j = k * G + i;
      const uint32_t b = o.hwc ? wr_tensor_bits<DT>(o, px[j / CH], j % CH) : wr_tensor_bits<DT>(o, px[i], k);
      w[i * E / 4] |= b << (8 * (i * E % 4));
    }
    const long long e = o.hwc ? (long long)y * o.row_stride + (long long)x0 * CH + k * G : k * o.plane_stride + (long long)y * o.row_stride + x0;
    wr_grab_st16(o.dst + e * E, wr_u4{w[0], w[1], w[2], w[3]});
  }
}
template <int DT> WR_DEVICE void wr_tensor_put_group_ch(const WrTensorOut& o, int y, int x0, const uint32_t* px) {
  if (o.channels == 4) wr_tensor_put_group<DT, 4>(o, y, x0, px);
  else if (o.channels == 3) wr_tensor_put_group<DT, 3>(o, y, x0, px);
  else wr_tensor_put_group<DT, 1>(o, y, x0, px);
}
// output rows [r0, r1) of the unscaled grab, thread t of nt: a row's whole groups, then its single pixels, the rows laid end to end.
// Source pixels are 4-byte loads -- coalesced across the wave whatever the rect's x is --, 16-byte ones where the group's are aligned.
template <int DT> WR_DEVICE void wr_grab_tensor_rows(const WrGrabTensorArgs& a, int r0, int r1, int t, int nt) {
  constexpr int G = 16 / wr_tensor_elem(DT);
  const WrTensorOut& o = a.o;
  const int w = o.ow, ng = o.vec ? w / G : 0, per_row = ng + (w - ng * G);
  const int items = (r1 - r0) * per_row;
  for (int it = t; it < items; it += nt) {
    const int y = r0 + it / per_row, i = it % per_row;
    const uint8_t* ps = a.tex + (size_t)(a.ry + (o.flip ? o.oh - 1 - y : y)) * a.tex_stride + (size_t)a.rx * a.bpp;
    if (i < ng) {
      uint32_t px[G];
      const uint8_t* p = ps + (size_t)i * G * a.bpp;
      if (a.bpp != 4) {
#pragma unroll
        for (int k = 0; k < G; k++) px[k] = p[k];
      } else if (((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int q = 0; q < G / 4; q++) { const wr_u4 v = wr_load16(p + 16 * q); px[4 * q] = v.x; px[4 * q + 1] = v.y; px[4 * q + 2] = v.z; px[4 * q + 3] = v.w; }
      } else {
#pragma unroll
        for (int k = 0; k < G; k++) px[k] = wr_load4(p + 4 * k);
      }
      wr_tensor_put_group_ch<DT>(o, y, i * G, px);
    } else {
      const int x = ng * G + (i - ng);
      wr_tensor_put_pixel<DT>(o, y, x, a.bpp == 4 ? wr_load4(ps + (size_t)x * 4) : (uint32_t)ps[x]);
    }
  }
}
__global__ void __launch_bounds__(256) wr_grab_tensor_kernel(WrGrabTensorArgs a) {
  const int t = (int)threadIdx.x;
  // (the ticket's header: an empty payload)
  if (a.slot && blockIdx.x == 0 && t == 0) wr_grab_st16(a.slot, wr_u4{0u, 0u, 0u, 0u});
  const int r0 = (int)blockIdx.x * a.rows_per_wg, r1 = wr_imin(a.o.oh, r0 + a.rows_per_wg);
  if (a.o.dtype == WR_TENSOR_F32) wr_grab_tensor_rows<WR_TENSOR_F32>(a, r0, r1, t, (int)blockDim.x);
  else if (a.o.dtype == WR_TENSOR_F16) wr_grab_tensor_rows<WR_TENSOR_F16>(a, r0, r1, t, (int)blockDim.x);
  else if (a.o.dtype == WR_TENSOR_BF16) wr_grab_tensor_rows<WR_TENSOR_BF16>(a, r0, r1, t, (int)blockDim.x);
  else wr_grab_tensor_rows<WR_TENSOR_U8>(a, r0, r1, t, (int)blockDim.x);
}

// WrhipPutTextureTensor (include/wrhip.h; WrTensorIn): wr_grab_tensor_kernel the other way -- tensor elements in the caller's memory
// become the stored bytes of a texture rect.  The work is again cut along the DESTINATION, which now is the texture: an item is one
// 16-byte piece of the texture's storage in one row -- P = 4 RGBA8 pixels, 8 RG8, 16 R8.  A piece that lies whole inside the rect's
// row leaves as one 16-byte store; the pieces a row starts and ends in leave pixel by pixel.  A texture row need not be a multiple
// of 16 bytes (333 RGBA8 pixels: the phase moves by a pixel every row), so where the pieces lie is taken from each row's ADDRESS.
// The elements behind a whole piece are P consecutive ones of each plane (CHW) or P * channels consecutive ones (HWC): such a run is
// fetched with the widest loads that divide it -- 16 bytes, or 8 or 4 where it is shorter (4 RGBA8 pixels are 8 bytes of an F16
// plane) -- if WrTensorIn::vec holds and the run's own address is aligned to them, with single-element loads otherwise.  Formats and
// channel counts are template parameters, so that a piece's elements and bytes stay in registers under constant indices.
WR_DEVICE void wr_put_load8(const void* p, uint32_t* w) {
#ifdef WRHIP_HOSTSIM
  __builtin_memcpy(w, p, 8);
#else
  typedef uint32_t wr_gu2 __attribute__((ext_vector_type(2)));
  const wr_gu2 v = *(const __attribute__((address_space(1))) wr_gu2*)p;
  w[0] = v.x; w[1] = v.y;
#endif
}
// the loads a run of `bytes` is cut into (every run is a multiple of 4 bytes: P * E is 4 at least)
constexpr int wr_put_chunk(int bytes) { return bytes % 16 == 0 ? 16 : bytes % 8 == 0 ? 8 : 4; }
// the bits of the one element of E bytes at p
template <int E> WR_DEVICE uint32_t wr_put_load_elem(const uint8_t* p) {
  if (E == 1) return *p;
  if (E == 2) { uint16_t h; __builtin_memcpy(&h, p, 2); return h; }
  uint32_t u; __builtin_memcpy(&u, p, 4); return u;
}
// the bits of N consecutive elements from p on -> el[0 .. N); N * E is a multiple of 4
template <int DT, int N> WR_DEVICE void wr_put_load_run(const uint8_t* p, bool vec, uint32_t* el) {
  constexpr int E = wr_tensor_elem(DT), BYTES = N * E, A = wr_put_chunk(BYTES);
  if (vec && ((uintptr_t)p & (uintptr_t)(A - 1)) == 0) {
    uint32_t w[BYTES / 4];
#pragma unroll
    for (int k = 0; k < BYTES / A; k++) {
      if (A == 16) { const wr_u4 v = wr_load16(p + 16 * k); w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
      else if (A == 8) wr_put_load8(p + 8 * k, w + 2 * k);
      else w[k] = wr_load4(p + 4 * k);
    }
#pragma unroll
    for (int j = 0; j < N; j++) el[j] = E == 4 ? w[j] : E == 2 ? (w[j / 2] >> (16 * (j % 2))) & 0xFFFFu : (w[j / 4] >> (8 * (j % 4))) & 0xFFu;
  } else {
#pragma unroll
    for (int j = 0; j < N; j++) el[j] = wr_put_load_elem<E>(p + E * j);
  }
}
// the stored byte of the element of input channel c whose bits are b
template <int DT> WR_DEVICE uint32_t wr_put_byte(const WrTensorIn& in, uint32_t b, int c) {
  if (DT == WR_TENSOR_U8) return b;
#ifdef WRHIP_HOSTSIM
  const float x = wr_bits_f(DT == WR_TENSOR_F32 ? b : DT == WR_TENSOR_F16 ? wr_f16_bits_to_f32_bits((uint16_t)b) : b << 16);
  const float y = x * in.scale[c] + in.bias[c];           // (two roundings: the build does not contract them)
  return wr_f32_bits_to_byte(wr_float_bits(y));
#else
  // (the device's own converts: v_cvt_f32_f16 is exact, subnormals included; round-to-nearest-even is the conversion's mode.  The
  // tests compare them with numpy on every f16 and bf16 pattern)
  float x;
  if (DT == WR_TENSOR_F16) { const uint16_t h = (uint16_t)b; _Float16 f; __builtin_memcpy(&f, &h, 2); x = (float)f; }
  else x = wr_bits_f(DT == WR_TENSOR_F32 ? b : b << 16);
  const float y = x * in.scale[c] + in.bias[c];
  return y >= 255.0f ? 255u : y >= 0.0f ? (uint32_t)__builtin_rintf(y) : 0u;      // (a NaN fails both comparisons)
#endif
}
// a pixel's stored word from the bytes v[c] of its input channels
template <int CH, int BPP> WR_DEVICE uint32_t wr_put_pack(const WrTensorIn& in, const uint32_t* v) {
  if (BPP == 1) return v[0];
  if (BPP == 2) return v[0] | (v[1] << 8);
  return (in.bgr ? v[0] : v[2]) | (v[1] << 8) | ((in.bgr ? v[2] : v[0]) << 16) | ((CH == 4 ? v[3] : in.alpha) << 24);
}
// one pixel, element by element: x of tensor row ty -> the BPP bytes at d
template <int DT, int CH, int BPP> WR_DEVICE void wr_put_pixel(const WrTensorIn& in, int ty, int x, uint8_t* d) {
  constexpr int E = wr_tensor_elem(DT);
  uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int c = 0; c < CH; c++) {
    const long long e = in.hwc ? (long long)ty * in.row_stride + (long long)x * CH + c : c * in.plane_stride + (long long)ty * in.row_stride + x;
    v[c] = wr_put_byte<DT>(in, wr_put_load_elem<E>(in.src + e * E), c);
  }
  const uint32_t px = wr_put_pack<CH, BPP>(in, v);
  if (BPP == 1) *d = (uint8_t)px;
  else if (BPP == 2) { const uint16_t h = (uint16_t)px; __builtin_memcpy(d, &h, 2); }
  else wr_grab_st4(d, px);
}
// a whole piece: the P pixels from x0 on of tensor row ty -> the 16 aligned bytes at d
template <int DT, int CH, int BPP> WR_DEVICE void wr_put_piece(const WrTensorIn& in, int ty, int x0, uint8_t* d) {
  constexpr int E = wr_tensor_elem(DT), P = 16 / BPP;
  uint32_t v[P][4];
  if (in.hwc) {
    uint32_t el[P * CH];
    wr_put_load_run<DT, P * CH>(in.src + ((long long)ty * in.row_stride + (long long)x0 * CH) * E, in.vec != 0, el);
#pragma unroll
    for (int i = 0; i < P; i++)
#pragma unroll
      for (int c = 0; c < CH; c++) v[i][c] = wr_put_byte<DT>(in, el[i * CH + c], c);
  } else {
#pragma unroll
    for (int c = 0; c < CH; c++) {
      uint32_t el[P];
      wr_put_load_run<DT, P>(in.src + (c * in.plane_stride + (long long)ty * in.row_stride + x0) * E, in.vec != 0, el);
#pragma unroll
      for (int i = 0; i < P; i++) v[i][c] = wr_put_byte<DT>(in, el[i], c);
    }
  }
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < P; i++) w[i * BPP / 4] |= wr_put_pack<CH, BPP>(in, v[i]) << (8 * (i * BPP % 4));
  wr_grab_st16(d, wr_u4{w[0], w[1], w[2], w[3]});
}
// rect rows [r0, r1), thread t of nt: the rows' items laid end to end, a.slots of them per row -- the last of a row may lie behind it
template <int DT, int CH, int BPP> WR_DEVICE void wr_put_tensor_rows(const WrPutTensorArgs& a, int r0, int r1, int t, int nt) {
  constexpr int P = 16 / BPP;
  const int items = (r1 - r0) * a.slots;
  for (int it = t; it < items; it += nt) {
    const int y = r0 + it / a.slots, s = it % a.slots;
    uint8_t* const row = a.tex + (size_t)(a.ry + y) * a.tex_stride + (size_t)a.rx * BPP;      // the first byte of the rect's row
    const int x0 = s * P - (int)((uintptr_t)row & 15) / BPP;      // the piece's first pixel, counted from the rect's left edge
    if (x0 >= a.w) continue;
    const int ty = a.in.flip ? a.h - 1 - y : y;
    if (x0 >= 0 && x0 + P <= a.w) {
      wr_put_piece<DT, CH, BPP>(a.in, ty, x0, row + (ptrdiff_t)x0 * BPP);
    } else {
      const int xa = wr_imax(x0, 0), xb = wr_imin(x0 + P, a.w);
      for (int x = xa; x < xb; x++) wr_put_pixel<DT, CH, BPP>(a.in, ty, x, row + (size_t)x * BPP);
    }
  }
}
template <int DT> WR_DEVICE void wr_put_tensor_rows_fmt(const WrPutTensorArgs& a, int r0, int r1, int t, int nt) {
  if (a.bpp == 4 && a.in.channels == 4) wr_put_tensor_rows<DT, 4, 4>(a, r0, r1, t, nt);
  else if (a.bpp == 4) wr_put_tensor_rows<DT, 3, 4>(a, r0, r1, t, nt);
  else if (a.bpp == 2) wr_put_tensor_rows<DT, 2, 2>(a, r0, r1, t, nt);
  else wr_put_tensor_rows<DT, 1, 1>(a, r0, r1, t, nt);
}
__global__ void __launch_bounds__(256) wr_put_tensor_kernel(WrPutTensorArgs a) {
  const int t = (int)threadIdx.x;
  const int r0 = (int)blockIdx.x * a.rows_per_wg, r1 = wr_imin(a.h, r0 + a.rows_per_wg);
  if (a.in.dtype == WR_TENSOR_F32) wr_put_tensor_rows_fmt<WR_TENSOR_F32>(a, r0, r1, t, (int)blockDim.x);
  else if (a.in.dtype == WR_TENSOR_F16) wr_put_tensor_rows_fmt<WR_TENSOR_F16>(a, r0, r1, t, (int)blockDim.x);
  else if (a.in.dtype == WR_TENSOR_BF16) wr_put_tensor_rows_fmt<WR_TENSOR_BF16>(a, r0, r1, t, (int)blockDim.x);
  else wr_put_tensor_rows_fmt<WR_TENSOR_U8>(a, r0, r1, t, (int)blockDim.x);
}
// The scaled grab's last launch with a converting store: the tile's last level (wr_grab_scale_store's geometry) leaves as elements --
// a thread per group of the OUTPUT row's grid that lies whole inside the tile's row, single pixels otherwise (a tile's row is
// (64 >> steps) pixels at most: 8 after three halvings, shorter than U8's group).
template <int DT> WR_DEVICE void wr_grab_scale_store_tensor(const WrGrabScaleArgs& a, const WrTensorOut& o, const WrGrabScaleGeom& g, const uint32_t* src, int pitch, int t) {
  constexpr int G = 16 / wr_tensor_elem(DT);
  const int ox = g.x0 >> a.steps, oy = g.y0 >> a.steps, ow = g.cw >> a.steps, oh = g.ch >> a.steps;
  for (int p = t; p < ow * oh; p += 256) {
    const int c = p % ow, r = p / ow;
    const int y = o.flip ? o.oh - 1 - (oy + r) : oy + r, x = ox + c;
    const int c0 = c - x % G;                                      // where the group this pixel lies in starts in the tile's row
    const bool whole = o.vec && c0 >= 0 && c0 + G <= ow;
    if (whole && c != c0) continue;                                // (stored by the group's first pixel)
    const uint32_t* s = src + r * pitch + c;
    if (whole) {
      uint32_t px[G];
#pragma unroll
      for (int k = 0; k < G; k++) px[k] = s[k];
      wr_tensor_put_group_ch<DT>(o, y, x, px);
    } else {
      wr_tensor_put_pixel<DT>(o, y, x, s[0]);
    }
  }
}
WR_DEVICE void wr_grab_scale_store_tensor_any(const WrGrabScaleArgs& a, const WrTensorOut& o, const WrGrabScaleGeom& g, const uint32_t* src, int pitch, int t) {
  if (o.dtype == WR_TENSOR_F32) wr_grab_scale_store_tensor<WR_TENSOR_F32>(a, o, g, src, pitch, t);
  else if (o.dtype == WR_TENSOR_F16) wr_grab_scale_store_tensor<WR_TENSOR_F16>(a, o, g, src, pitch, t);
  else if (o.dtype == WR_TENSOR_BF16) wr_grab_scale_store_tensor<WR_TENSOR_BF16>(a, o, g, src, pitch, t);
  else wr_grab_scale_store_tensor<WR_TENSOR_U8>(a, o, g, src, pitch, t);
}
__global__ void __launch_bounds__(256) wr_grab_scale_tensor_kernel(WrGrabScaleTensorArgs b) {
  const WrGrabScaleArgs& a = b.s;
  const WrGrabScaleGeom g = wr_grab_scale_geom(a, (int)blockIdx.x);
#ifdef WRHIP_HOSTSIM
  if (threadIdx.x != 0) return;
  WrGrabScaleTile T;
#else
  __shared__ WrGrabScaleTile T;
  const int t = (int)threadIdx.x;
#endif
  WR_SCALE_PHASE(wr_grab_scale_coords(a, g, T, t))
  WR_SCALE_PHASE(wr_grab_scale_fill(a, g, T, t))
  uint32_t* from = T.a;
  uint32_t* to = T.b;
  for (int k = 0; k < a.steps; k++) {
    WR_SCALE_PHASE(wr_grab_scale_halve(from, to, WR_SCALE_TILE >> k, g.cw >> k, g.ch >> k, t))
    uint32_t* const was = from; from = to; to = was;
  }
  WR_SCALE_PHASE(wr_grab_scale_store_tensor_any(a, b.o, g, from, WR_SCALE_TILE >> a.steps, t);
                 if (a.slot && blockIdx.x == 0 && t == 0) wr_grab_st16(a.slot, wr_u4{0u, 0u, 0u, 0u}))
}
// (WR_SCALE_PHASE stays defined for wr_grab_scale_yuv_kernel, behind the YUV grab's helpers)
// WrhipGrabTextureYuv (include/wrhip.h; WrGrabYuvArgs): the rect's stored B, G, R bytes as 8-bit Y, Cb and Cr planes for a video
// encoder -- the inverse of the video wr_composite_yuv_kernel draws.  A streaming converter bound by its read, 4 bytes per pixel
// against 1.5 or 3 written, so the work is cut along the SOURCE rows: a unit is two image rows (4:2:0: a chroma sample never needs
// another unit's pixels) or one (I444), an item is eight pixels of it -- two 16-byte loads per row where the address allows -- which
// are 8 bytes of a Y row, 4 of an I420 chroma row, 8 of an NV12 or I444 one.  Which eight pixels is decided per destination row from
// that row's ADDRESS, so that a piece lying whole inside its row leaves as one aligned 8- or 4-byte store and only the row's head and
// tail leave as bytes: odd widths and tight strides move the phase from row to row and from plane to plane.  Where the phases agree
// -- every stride a multiple of 8 -- the rows of a unit are loaded once; a row whose phase differs fetches its own window (WrYuvRow).
// The format is a template parameter; the colour space is nine coefficients and y0 in the arguments; the sink is base pointers.
WR_DEVICE void wr_yuv_st8(void* p, uint32_t lo, uint32_t hi) {
#ifdef WRHIP_HOSTSIM
  const uint32_t v[2] = {lo, hi};
  __builtin_memcpy(p, v, 8);
#else
  typedef uint32_t wr_gu2 __attribute__((ext_vector_type(2)));
  *(__attribute__((address_space(1))) wr_gu2*)p = wr_gu2{lo, hi};
#endif
}
// eight pixels of one source row: columns x0 .. x0 + 7, each held to the rect's [0, w) -- the clamp of a 4:2:0 block at the right edge
struct WrYuvRow { const uint8_t* row; int x0; uint32_t px[8]; };
WR_DEVICE void wr_yuv_fetch(WrYuvRow& R, int x0, int w) {
  if (R.x0 == x0) return;
  R.x0 = x0;
  if (x0 >= 0 && x0 + 8 <= w) {
    const uint8_t* p = R.row + (size_t)x0 * 4;
    if (((uintptr_t)p & 15) == 0) {
      const wr_u4 u = wr_load16(p), v = wr_load16(p + 16);
      R.px[0] = u.x; R.px[1] = u.y; R.px[2] = u.z; R.px[3] = u.w; R.px[4] = v.x; R.px[5] = v.y; R.px[6] = v.z; R.px[7] = v.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) R.px[k] = wr_load4(p + 4 * k);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) R.px[k] = wr_load4(R.row + (size_t)wr_iclamp(x0 + k, 0, w - 1) * 4);
  }
}
WR_DEVICE uint32_t wr_yuv_luma(const WrGrabYuvArgs& a, uint32_t px) {
  const int r = (int)((px >> 16) & 0xFFu), g = (int)((px >> 8) & 0xFFu), b = (int)(px & 0xFFu);
  return (uint32_t)((a.cy[0] * r + a.cy[1] * g + a.cy[2] * b + (a.y0 << 16) + 0x8000) >> 16);
}
// a chroma sample of the row `c` from channel sums over 1 << (SH - 16) pixels (SH 16: one pixel, 18: a 2 x 2 block)
// (the clamp comes BEFORE the shift -- the same value.  Shift, clamp and the OR of an NV12 pair are what the compiler turns into
// gfx950's v_ashr_pk_u8_i32, whose result it then ORs into a 32-bit word as if its upper half were zero: it is not)
template <int SH> WR_DEVICE uint32_t wr_yuv_chroma(const int32_t* c, int r, int g, int b) {
  return (uint32_t)wr_iclamp(c[0] * r + c[1] * g + c[2] * b + (128 << SH) + (1 << (SH - 1)), 0, (256 << SH) - 1) >> SH;
}
// the block sums of 4:2:0 sample k of a window: columns 2k, 2k + 1 of both rows
WR_DEVICE uint32_t wr_yuv_chroma420(const int32_t* c, const WrYuvRow& A, const WrYuvRow& B, int k) {
  const uint32_t p0 = A.px[2 * k], p1 = A.px[2 * k + 1], p2 = B.px[2 * k], p3 = B.px[2 * k + 1];
  // (R and B of the four pixels add up side by side in one word: 4 * 255 stays inside 16 bits)
  const uint32_t rb = (p0 & 0xFF00FFu) + (p1 & 0xFF00FFu) + (p2 & 0xFF00FFu) + (p3 & 0xFF00FFu);
  const uint32_t g = ((p0 >> 8) & 0xFFu) + ((p1 >> 8) & 0xFFu) + ((p2 >> 8) & 0xFFu) + ((p3 >> 8) & 0xFFu);
  return wr_yuv_chroma<18>(c, (int)(rb >> 16), (int)g, (int)(rb & 0xFFFFu));
}
// samples v[0 .. N) of a destination row of n samples of BYTES bytes at d, from sample i0 on: one aligned store of the N * BYTES (8
// or 4) bytes where all of them lie inside the row, bytes otherwise.  v[k] holds the sample's BYTES bytes.
template <int N, int BYTES> WR_DEVICE void wr_yuv_put(uint8_t* d, int i0, int n, const uint32_t* v) {
  uint8_t* const p = d + (ptrdiff_t)i0 * BYTES;
  if (i0 >= 0 && i0 + N <= n && ((uintptr_t)p & (uintptr_t)(N * BYTES - 1)) == 0) {
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < N; k++) w[k * BYTES / 4] |= v[k] << (8 * (k * BYTES % 4));
    if (N * BYTES == 8) wr_yuv_st8(p, w[0], w[1]);
    else wr_grab_st4(p, w[0]);
    return;
  }
#pragma unroll
  for (int k = 0; k < N; k++) {
    if (i0 + k >= 0 && i0 + k < n) {
      p[k * BYTES] = (uint8_t)v[k];
      if (BYTES == 2) p[k * BYTES + 1] = (uint8_t)(v[k] >> 8);
    }
  }
}
// the first sample of piece s of a row at d: pieces of N samples of BYTES bytes count from the aligned address at or below d
template <int N, int BYTES> WR_DEVICE int wr_yuv_first(const uint8_t* d, int s) {
  return s * N - (int)((uintptr_t)d & (uintptr_t)(N * BYTES - 1)) / BYTES;
}
// piece s of the Y row at d, or of an I444 chroma row (`c`: its coefficients; null: luma), from the source row R
WR_DEVICE void wr_yuv_row_piece(const WrGrabYuvArgs& a, WrYuvRow& R, uint8_t* d, int s, const int32_t* c) {
  const int i0 = wr_yuv_first<8, 1>(d, s);
  if (i0 >= a.w || i0 + 8 <= 0) return;
  wr_yuv_fetch(R, i0, a.w);
  uint32_t v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint32_t px = R.px[k];
    v[k] = c ? wr_yuv_chroma<16>(c, (int)((px >> 16) & 0xFFu), (int)((px >> 8) & 0xFFu), (int)(px & 0xFFu)) : wr_yuv_luma(a, px);
  }
  wr_yuv_put<8, 1>(d, i0, a.w, v);
}
// row units [u0, u1), thread t of nt: the units' items laid end to end, a.slots of them per unit
template <int FMT> WR_DEVICE void wr_grab_yuv_units(const WrGrabYuvArgs& a, int u0, int u1, int t, int nt) {
  const int items = (u1 - u0) * a.slots, cw = (a.w + 1) >> 1;
  for (int it = t; it < items; it += nt) {
    const int u = u0 + it / a.slots, s = it % a.slots;
    const int ra = FMT == WR_YUV_I444 ? u : 2 * u, rb = wr_imin(ra + 1, a.h - 1);
    WrYuvRow A, B;
    A.row = a.tex + (size_t)(a.ry + (a.flip ? a.h - 1 - ra : ra)) * a.tex_stride + (size_t)a.rx * 4;
    B.row = a.tex + (size_t)(a.ry + (a.flip ? a.h - 1 - rb : rb)) * a.tex_stride + (size_t)a.rx * 4;
    A.x0 = B.x0 = -0x40000000;      // (nothing fetched yet)
    wr_yuv_row_piece(a, A, a.y + ra * a.y_stride, s, nullptr);
    if (FMT == WR_YUV_I444) {
      wr_yuv_row_piece(a, A, a.cb + ra * a.c_stride, s, a.ccb);
      wr_yuv_row_piece(a, A, a.cr + ra * a.c_stride, s, a.ccr);
      continue;
    }
    if (ra + 1 < a.h) wr_yuv_row_piece(a, B, a.y + (ra + 1) * a.y_stride, s, nullptr);
    if (FMT == WR_YUV_NV12) {
      // (pairs: a row that starts at an odd address has no aligned piece of whole pairs -- it leaves as bytes)
      uint8_t* const d = a.cb + u * a.c_stride;
      const int i0 = wr_yuv_first<4, 2>(d, s);
      if (i0 >= cw || i0 + 4 <= 0) continue;
      wr_yuv_fetch(A, 2 * i0, a.w); wr_yuv_fetch(B, 2 * i0, a.w);
      uint32_t v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = wr_yuv_chroma420(a.ccb, A, B, k) | (wr_yuv_chroma420(a.ccr, A, B, k) << 8);
      wr_yuv_put<4, 2>(d, i0, cw, v);
    } else {
#pragma unroll
      for (int plane = 0; plane < 2; plane++) {
        uint8_t* const d = (plane ? a.cr : a.cb) + u * a.c_stride;
        const int i0 = wr_yuv_first<4, 1>(d, s);
        if (i0 >= cw || i0 + 4 <= 0) continue;
        wr_yuv_fetch(A, 2 * i0, a.w); wr_yuv_fetch(B, 2 * i0, a.w);
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = wr_yuv_chroma420(plane ? a.ccr : a.ccb, A, B, k);
        wr_yuv_put<4, 1>(d, i0, cw, v);
      }
    }
  }
}
__global__ void __launch_bounds__(256) wr_grab_yuv_kernel(WrGrabYuvArgs a) {
  const int t = (int)threadIdx.x;
  // (the ticket's header: the planes' bytes behind it, or an empty payload)
  if (a.slot && blockIdx.x == 0 && t == 0) wr_grab_st16(a.slot, wr_u4{a.payload, 0u, 0u, 0u});
  const int units = a.format == WR_YUV_I444 ? a.h : (a.h + 1) >> 1;
  const int u0 = (int)blockIdx.x * a.units_per_wg, u1 = wr_imin(units, u0 + a.units_per_wg);
  if (a.format == WR_YUV_I420) wr_grab_yuv_units<WR_YUV_I420>(a, u0, u1, t, (int)blockDim.x);
  else if (a.format == WR_YUV_NV12) wr_grab_yuv_units<WR_YUV_NV12>(a, u0, u1, t, (int)blockDim.x);
  else wr_grab_yuv_units<WR_YUV_I444>(a, u0, u1, t, (int)blockDim.x);
}
// WrhipGrabTextureYuvScaled (include/wrhip.h; WrGrabScaleYuvArgs): the scaled grab's launch -- its coordinates, fill and halving
// phases, called as they are -- with a store phase that turns levels of the tile's pyramid into samples while they are in LDS.  A
// launch holds levels top .. top - steps, each exactly once in the grab, so rendition k leaves from the launch that holds level k:
// the renditions of a ladder come out of the one pass over the source.  Level top - j of the tile is (64 >> j) pixels on a side
// at an origin that is a multiple of that: the 2 x 2 chroma blocks of the unflipped level never leave the tile, nor do those of a
// flipped level of even height (rows 2m + 1, 2m); only the clamp at an odd last column or row is left, and it is the tile's own
// last column or row.  (The flipped 4:2:0 level of odd height pairs rows 2m, 2m - 1: the host routes it through
// wr_grab_yuv_kernel.)  The work is cut as wr_grab_yuv_units cuts it: a unit is two level rows (4:2:0) or one (I444), an item the
// 8-byte piece of the Y row it touches -- which eight pixels is decided per destination row from that row's ADDRESS at the tile's
// first column, so a piece lying whole inside the tile's part of the row leaves as one aligned store and the rest as bytes.  A
// level is converted in the phase that reads it for the next halving: behind the barrier that completes it, ahead of the one
// after which its buffer is written again.
// eight pixels of one row of the tile's level: columns c0 .. c0 + 7 of the tile, each held to [0, ow)
WR_DEVICE void wr_yuv_fetch_tile(WrYuvRow& R, const uint32_t* row, int c0, int ow) {
  if (R.x0 == c0) return;
  R.x0 = c0;
#pragma unroll
  for (int k = 0; k < 8; k++) R.px[k] = row[wr_iclamp(c0 + k, 0, ow - 1)];
}
// piece s of the tile's part -- samples [0, ow) at d -- of a Y row, or of an I444 chroma row (`c`: its coefficients; null: luma)
WR_DEVICE void wr_yuv_tile_piece(const WrGrabYuvArgs& a, WrYuvRow& R, const uint32_t* row, uint8_t* d, int ow, int s, const int32_t* c) {
  const int i0 = wr_yuv_first<8, 1>(d, s);
  if (i0 >= ow || i0 + 8 <= 0) return;
  wr_yuv_fetch_tile(R, row, i0, ow);
  uint32_t v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint32_t px = R.px[k];
    v[k] = c ? wr_yuv_chroma<16>(c, (int)((px >> 16) & 0xFFu), (int)((px >> 8) & 0xFFu), (int)(px & 0xFFu)) : wr_yuv_luma(a, px);
  }
  wr_yuv_put<8, 1>(d, i0, ow, v);
}
// the tile's level after j halvings (pitch 64 >> j) into the planes L
template <int FMT> WR_DEVICE void wr_grab_scale_store_yuv(const WrGrabScaleYuvArgs& b, const WrYuvLevel& L, const WrGrabScaleGeom& g, const uint32_t* src, int j, int t) {
  const WrGrabYuvArgs& a = b.g;
  const int pitch = WR_SCALE_TILE >> j, lh = b.s.th >> j;
  const int ox = g.x0 >> j, oy = g.y0 >> j, ow = g.cw >> j, oh = g.ch >> j;
  const int units = FMT == WR_YUV_I444 ? oh : (oh + 1) >> 1, slots = (ow + 7) / 8 + 1, cow = (ow + 1) >> 1;
  for (int it = t; it < units * slots; it += 256) {
    const int u = it / slots, s = it % slots;
    // the unit's rows in the tile, in the level, and in the image
    const int ta = FMT == WR_YUV_I444 ? u : 2 * u, tb = wr_imin(ta + 1, oh - 1);
    const int ia = a.flip ? lh - 1 - (oy + ta) : oy + ta, ib = a.flip ? lh - 1 - (oy + tb) : oy + tb;
    WrYuvRow A, B;
    A.row = B.row = nullptr;
    A.x0 = B.x0 = -0x40000000;      // (nothing fetched yet)
    const uint32_t* const rowa = src + ta * pitch;
    const uint32_t* const rowb = src + tb * pitch;
    wr_yuv_tile_piece(a, A, rowa, L.y + ia * L.y_stride + ox, ow, s, nullptr);
    if (FMT == WR_YUV_I444) {
      wr_yuv_tile_piece(a, A, rowa, L.cb + ia * L.c_stride + ox, ow, s, a.ccb);
      wr_yuv_tile_piece(a, A, rowa, L.cr + ia * L.c_stride + ox, ow, s, a.ccr);
      continue;
    }
    if (tb != ta) wr_yuv_tile_piece(a, B, rowb, L.y + ib * L.y_stride + ox, ow, s, nullptr);
    const int cr = wr_imin(ia, ib) >> 1;      // (the block's row of the image: rows 2 cr and 2 cr + 1, whichever of them the tile's row ta is)
    if (FMT == WR_YUV_NV12) {
      uint8_t* const d = L.cb + cr * L.c_stride + ox;      // (ox is even: ox / 2 pairs)
      const int i0 = wr_yuv_first<4, 2>(d, s);
      if (i0 >= cow || i0 + 4 <= 0) continue;
      wr_yuv_fetch_tile(A, rowa, 2 * i0, ow); wr_yuv_fetch_tile(B, rowb, 2 * i0, ow);
      uint32_t v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = wr_yuv_chroma420(a.ccb, A, B, k) | (wr_yuv_chroma420(a.ccr, A, B, k) << 8);
      wr_yuv_put<4, 2>(d, i0, cow, v);
    } else {
#pragma unroll
      for (int plane = 0; plane < 2; plane++) {
        uint8_t* const d = (plane ? L.cr : L.cb) + cr * L.c_stride + (ox >> 1);
        const int i0 = wr_yuv_first<4, 1>(d, s);
        if (i0 >= cow || i0 + 4 <= 0) continue;
        wr_yuv_fetch_tile(A, rowa, 2 * i0, ow); wr_yuv_fetch_tile(B, rowb, 2 * i0, ow);
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = wr_yuv_chroma420(plane ? a.ccr : a.ccb, A, B, k);
        wr_yuv_put<4, 1>(d, i0, cow, v);
      }
    }
  }
}
WR_DEVICE void wr_grab_scale_store_yuv_any(const WrGrabScaleYuvArgs& b, const WrGrabScaleGeom& g, const uint32_t* src, int j, int t) {
  const WrYuvLevel& L = b.lv[j];
  if (!L.y) return;
  if (b.g.format == WR_YUV_I420) wr_grab_scale_store_yuv<WR_YUV_I420>(b, L, g, src, j, t);
  else if (b.g.format == WR_YUV_NV12) wr_grab_scale_store_yuv<WR_YUV_NV12>(b, L, g, src, j, t);
  else wr_grab_scale_store_yuv<WR_YUV_I444>(b, L, g, src, j, t);
}
__global__ void __launch_bounds__(256) wr_grab_scale_yuv_kernel(WrGrabScaleYuvArgs b) {
  const WrGrabScaleArgs& a = b.s;
  const WrGrabScaleGeom g = wr_grab_scale_geom(a, (int)blockIdx.x);
#ifdef WRHIP_HOSTSIM
  if (threadIdx.x != 0) return;
  WrGrabScaleTile T;
#else
  __shared__ WrGrabScaleTile T;
  const int t = (int)threadIdx.x;
#endif
  WR_SCALE_PHASE(wr_grab_scale_coords(a, g, T, t))
  WR_SCALE_PHASE(wr_grab_scale_fill(a, g, T, t))
  uint32_t* from = T.a;
  uint32_t* to = T.b;
  for (int k = 0; k < a.steps; k++) {
    WR_SCALE_PHASE(wr_grab_scale_store_yuv_any(b, g, from, k, t);
                   wr_grab_scale_halve(from, to, WR_SCALE_TILE >> k, g.cw >> k, g.ch >> k, t))
    uint32_t* const was = from; from = to; to = was;
  }
  WR_SCALE_PHASE(wr_grab_scale_store_yuv_any(b, g, from, a.steps, t);
                 if (b.rgba) wr_grab_scale_store(a, g, from, WR_SCALE_TILE >> a.steps, t);
                 if (a.slot && blockIdx.x == 0 && t == 0) wr_grab_st16(a.slot, wr_u4{a.payload, 0u, 0u, 0u}))
}
#undef WR_SCALE_PHASE
// WrhipGrabTextureYuvDelta (include/wrhip.h; WrGrabYuvDeltaArgs): the YUV grab's samples, block by block, and only the blocks whose
// samples differ from the retained planes.  A workgroup per 64 x 64 block of the image (after the flip), as wr_grab_pack_kernel has
// it; the YUV grab's item -- eight pixels of a row pair, or of one row of I444 -- tiles the block: 32 row pairs of 8 items are one
// item per thread in 4:2:0, 64 rows of 8 are two per thread in I444.  A thread fetches its pixels (wr_yuv_fetch: clamped to the
// rect, so an edge block's 2 x 2 sums are the full grab's), converts them in registers into six words -- 4:2:0: Y of the upper row,
// Y of the lower row, then Cb | Cr words (I420) or two words of pairs (NV12); I444: Y, Cb, Cr of its row -- with the bytes beyond the
// image zero, and compares them with the retained planes' 8 + 8 + 4 + 4 bytes (I444: 8 + 8 + 8).  The vote, the entry and the
// keyframe are the pack kernel's: a ballot per wave, one LDS word, one returning atomic per SENT block on the slot's byte count,
// entry i = block i on a keyframe.  What is sent goes to its entry (host sink) or through wr_yuv_put into the caller's planes
// (device sink, the entry then being the record alone), and to the retained planes.  Entry and retained rows are multiples of 8
// bytes: those stores are whole aligned words.
WR_DEVICE void wr_yuv_ld8(const void* p, uint32_t& lo, uint32_t& hi) {
#ifdef WRHIP_HOSTSIM
  uint32_t v[2];
  __builtin_memcpy(v, p, 8);
  lo = v[0]; hi = v[1];
#else
  typedef uint32_t wr_gu2 __attribute__((ext_vector_type(2)));
  const wr_gu2 v = *(const __attribute__((address_space(1))) wr_gu2*)p;
  lo = v.x; hi = v.y;
#endif
}
// a block's samples in one of the library's own homes, seen from the block's origin: the retained planes, or an entry's body
struct WrYuvdHome { uint8_t* y; uint8_t* c0; uint8_t* c1; int ys, cs; };
template <int FMT> WR_DEVICE WrYuvdHome wr_yuvd_keep(const WrGrabYuvDeltaArgs& d, int x0, int y0) {
  WrYuvdHome K;
  K.ys = d.keep_ys; K.cs = d.keep_cs;
  K.y = d.keep_y + (size_t)y0 * K.ys + x0;
  const size_t c = FMT == WR_YUV_I444 ? (size_t)y0 * K.cs + x0 : (size_t)(y0 >> 1) * K.cs + (FMT == WR_YUV_NV12 ? x0 : x0 >> 1);
  K.c0 = d.keep_cb + c; K.c1 = d.keep_cr + c;
  return K;
}
template <int FMT> WR_DEVICE WrYuvdHome wr_yuvd_body(uint8_t* e) {
  constexpr int B = WR_GRAB_BLOCK;
  WrYuvdHome E;
  E.ys = B; E.cs = FMT == WR_YUV_I420 ? B / 2 : B;
  E.y = e; E.c0 = e + B * B; E.c1 = E.c0 + (FMT == WR_YUV_I444 ? B * B : B * B / 4);
  return E;
}
// item j of the block at (x0, y0): -> false if none of it lies inside the image; w: its six words
template <int FMT> WR_DEVICE bool wr_yuvd_convert(const WrGrabYuvArgs& a, int x0, int y0, int j, uint32_t (&w)[6]) {
  const int cx = x0 + 8 * (j & 7), ra = y0 + (FMT == WR_YUV_I444 ? j >> 3 : 2 * (j >> 3));
  if (cx >= a.w || ra >= a.h) return false;
  const int n = wr_imin(8, a.w - cx);
  WrYuvRow A;
  A.row = a.tex + (size_t)(a.ry + (a.flip ? a.h - 1 - ra : ra)) * a.tex_stride + (size_t)a.rx * 4;
  A.x0 = -0x40000000;      // (nothing fetched yet)
  wr_yuv_fetch(A, cx, a.w);
#pragma unroll
  for (int k = 0; k < 6; k++) w[k] = 0u;
  if (FMT == WR_YUV_I444) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (k >= n) continue;
      const uint32_t px = A.px[k];
      const int r = (int)((px >> 16) & 0xFFu), g = (int)((px >> 8) & 0xFFu), b = (int)(px & 0xFFu);
      w[k >> 2] |= wr_yuv_luma(a, px) << (8 * (k & 3));
      w[2 + (k >> 2)] |= wr_yuv_chroma<16>(a.ccb, r, g, b) << (8 * (k & 3));
      w[4 + (k >> 2)] |= wr_yuv_chroma<16>(a.ccr, r, g, b) << (8 * (k & 3));
    }
    return true;
  }
  const int rb = wr_imin(ra + 1, a.h - 1);
  WrYuvRow B;
  B.row = a.tex + (size_t)(a.ry + (a.flip ? a.h - 1 - rb : rb)) * a.tex_stride + (size_t)a.rx * 4;
  B.x0 = -0x40000000;
  wr_yuv_fetch(B, cx, a.w);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (k >= n) continue;
    w[k >> 2] |= wr_yuv_luma(a, A.px[k]) << (8 * (k & 3));
    if (ra + 1 < a.h) w[2 + (k >> 2)] |= wr_yuv_luma(a, B.px[k]) << (8 * (k & 3));
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (2 * k >= n) continue;
    const uint32_t cb = wr_yuv_chroma420(a.ccb, A, B, k), cr = wr_yuv_chroma420(a.ccr, A, B, k);
    if (FMT == WR_YUV_NV12) w[4 + (k >> 1)] |= (cb | (cr << 8)) << (16 * (k & 1));
    else { w[4] |= cb << (8 * k); w[5] |= cr << (8 * k); }
  }
  return true;
}
// where item j's words lie in a home: Y (two rows in 4:2:0), chroma
template <int FMT> WR_DEVICE bool wr_yuvd_differs(const WrYuvdHome& K, int j, const uint32_t (&w)[6]) {
  const int i = j & 7, r = j >> 3;
  uint32_t e[6];
  if (FMT == WR_YUV_I444) {
    wr_yuv_ld8(K.y + (size_t)r * K.ys + 8 * i, e[0], e[1]);
    wr_yuv_ld8(K.c0 + (size_t)r * K.cs + 8 * i, e[2], e[3]);
    wr_yuv_ld8(K.c1 + (size_t)r * K.cs + 8 * i, e[4], e[5]);
  } else {
    wr_yuv_ld8(K.y + (size_t)(2 * r) * K.ys + 8 * i, e[0], e[1]);
    wr_yuv_ld8(K.y + (size_t)(2 * r + 1) * K.ys + 8 * i, e[2], e[3]);
    if (FMT == WR_YUV_NV12) wr_yuv_ld8(K.c0 + (size_t)r * K.cs + 8 * i, e[4], e[5]);
    else { e[4] = wr_load4(K.c0 + (size_t)r * K.cs + 4 * i); e[5] = wr_load4(K.c1 + (size_t)r * K.cs + 4 * i); }
  }
  return ((w[0] ^ e[0]) | (w[1] ^ e[1]) | (w[2] ^ e[2]) | (w[3] ^ e[3]) | (w[4] ^ e[4]) | (w[5] ^ e[5])) != 0u;
}
template <int FMT> WR_DEVICE void wr_yuvd_store(const WrYuvdHome& H, int j, const uint32_t (&w)[6]) {
  const int i = j & 7, r = j >> 3;
  if (FMT == WR_YUV_I444) {
    wr_yuv_st8(H.y + (size_t)r * H.ys + 8 * i, w[0], w[1]);
    wr_yuv_st8(H.c0 + (size_t)r * H.cs + 8 * i, w[2], w[3]);
    wr_yuv_st8(H.c1 + (size_t)r * H.cs + 8 * i, w[4], w[5]);
  } else {
    wr_yuv_st8(H.y + (size_t)(2 * r) * H.ys + 8 * i, w[0], w[1]);
    wr_yuv_st8(H.y + (size_t)(2 * r + 1) * H.ys + 8 * i, w[2], w[3]);
    if (FMT == WR_YUV_NV12) wr_yuv_st8(H.c0 + (size_t)r * H.cs + 8 * i, w[4], w[5]);
    else { wr_grab_st4(H.c0 + (size_t)r * H.cs + 4 * i, w[4]); wr_grab_st4(H.c1 + (size_t)r * H.cs + 4 * i, w[5]); }
  }
}
// the eight bytes of two words as samples for wr_yuv_put: eight of a byte, or four pairs
template <int BYTES> WR_DEVICE void wr_yuvd_samples(uint32_t lo, uint32_t hi, uint32_t (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 8 / BYTES; k++) v[k] = ((k < 4 / BYTES ? lo : hi) >> (8 * BYTES * (k % (4 / BYTES)))) & (BYTES == 2 ? 0xFFFFu : 0xFFu);
}
// item j into the caller's planes (device sink): the YUV grab's addresses, its rows cut by wr_yuv_put
template <int FMT> WR_DEVICE void wr_yuvd_put(const WrGrabYuvArgs& a, int x0, int y0, int j, const uint32_t (&w)[6]) {
  const int cx = x0 + 8 * (j & 7), ra = y0 + (FMT == WR_YUV_I444 ? j >> 3 : 2 * (j >> 3)), cw = (a.w + 1) >> 1;
  uint32_t v[8];
  wr_yuvd_samples<1>(w[0], w[1], v);
  wr_yuv_put<8, 1>(a.y + ra * a.y_stride, cx, a.w, v);
  if (FMT == WR_YUV_I444) {
    wr_yuvd_samples<1>(w[2], w[3], v);
    wr_yuv_put<8, 1>(a.cb + ra * a.c_stride, cx, a.w, v);
    wr_yuvd_samples<1>(w[4], w[5], v);
    wr_yuv_put<8, 1>(a.cr + ra * a.c_stride, cx, a.w, v);
    return;
  }
  if (ra + 1 < a.h) {
    wr_yuvd_samples<1>(w[2], w[3], v);
    wr_yuv_put<8, 1>(a.y + (ra + 1) * a.y_stride, cx, a.w, v);
  }
  if (FMT == WR_YUV_NV12) {
    wr_yuvd_samples<2>(w[4], w[5], v);
    wr_yuv_put<4, 2>(a.cb + (ra >> 1) * a.c_stride, cx >> 1, cw, v);
  } else {
    wr_yuvd_samples<1>(w[4], w[5], v);
    wr_yuv_put<4, 1>(a.cb + (ra >> 1) * a.c_stride, cx >> 1, cw, v);
    wr_yuv_put<4, 1>(a.cr + (ra >> 1) * a.c_stride, cx >> 1, cw, v + 4);
  }
}
// lw: the vote's two LDS words (wr_grab_pack_kernel's); unused by the host simulation
template <int FMT> WR_DEVICE void wr_grab_yuv_delta_block(const WrGrabYuvDeltaArgs& d, unsigned* lw) {
  constexpr int ITEMS = FMT == WR_YUV_I444 ? 2 : 1;      // per thread
  const WrGrabYuvArgs& a = d.g;
  const int t = (int)threadIdx.x, b = (int)blockIdx.x;
  const int x0 = (b % d.bx) * WR_GRAB_BLOCK, y0 = (b / d.bx) * WR_GRAB_BLOCK;
  const unsigned entry_bytes = d.device ? 16u : (unsigned)WR_YUVD_ENTRY(FMT);
  const wr_u4 record = {(uint32_t)x0, (uint32_t)y0, (uint32_t)wr_imin(WR_GRAB_BLOCK, a.w - x0), (uint32_t)wr_imin(WR_GRAB_BLOCK, a.h - y0)};
  const WrYuvdHome K = wr_yuvd_keep<FMT>(d, x0, y0);
  uint8_t* e = nullptr;                // the block's entry, once it has one
#ifdef WRHIP_HOSTSIM
  // (threads run one after the other: the first walks the block twice)
  (void)lw;
  if (t != 0) return;
  bool diff = d.keyframe != 0;
  uint32_t w[6];
  for (int j = 0; j < 256 * ITEMS && !diff; j++)
    if (wr_yuvd_convert<FMT>(a, x0, y0, j, w)) diff = wr_yuvd_differs<FMT>(K, j, w);
  if (!diff) return;
  if (a.slot) {
    const unsigned index = d.keyframe ? (unsigned)b : atomicAdd((unsigned*)a.slot, entry_bytes) / entry_bytes;
    e = a.slot + WR_GRAB_HEADER + (size_t)index * entry_bytes;
    wr_grab_st16(e, record);
  }
  const WrYuvdHome E = wr_yuvd_body<FMT>(e ? e + 16 : nullptr);
  for (int j = 0; j < 256 * ITEMS; j++) {
    if (!wr_yuvd_convert<FMT>(a, x0, y0, j, w)) continue;
    if (d.device) wr_yuvd_put<FMT>(a, x0, y0, j, w);
    else if (e) wr_yuvd_store<FMT>(E, j, w);
    wr_yuvd_store<FMT>(K, j, w);
  }
#else
  uint32_t w[ITEMS][6];
  bool on[ITEMS], diff = false;
#pragma unroll
  for (int k = 0; k < ITEMS; k++) {
    on[k] = wr_yuvd_convert<FMT>(a, x0, y0, k * 256 + t, w[k]);
    if (on[k] && !d.keyframe) diff = diff || wr_yuvd_differs<FMT>(K, k * 256 + t, w[k]);
  }
  unsigned index = (unsigned)b;
  if (!d.keyframe) {
    if (t == 0) lw[0] = 0u;
    __syncthreads();
    if (__ballot(diff) != 0ull && (t & 63) == 0) lw[0] = 1u;
    __syncthreads();
    if (lw[0] == 0u) return;
    if (t == 0) lw[1] = a.slot ? atomicAdd((unsigned*)a.slot, entry_bytes) / entry_bytes : 0u;
    __syncthreads();
    index = lw[1];
  }
  if (a.slot) {
    e = a.slot + WR_GRAB_HEADER + (size_t)index * entry_bytes;
    if (t == 0) wr_grab_st16(e, record);
  }
  const WrYuvdHome E = wr_yuvd_body<FMT>(e ? e + 16 : nullptr);
#pragma unroll
  for (int k = 0; k < ITEMS; k++) {
    if (!on[k]) continue;
    if (d.device) wr_yuvd_put<FMT>(a, x0, y0, k * 256 + t, w[k]);
    else if (e) wr_yuvd_store<FMT>(E, k * 256 + t, w[k]);
    wr_yuvd_store<FMT>(K, k * 256 + t, w[k]);
  }
#endif
}
__global__ void __launch_bounds__(256) wr_grab_yuv_delta_kernel(WrGrabYuvDeltaArgs d) {
  // (what the host knows of the slot's byte count is written here: a keyframe's)
  if (d.keyframe && d.g.slot && blockIdx.x == 0 && threadIdx.x == 0) wr_grab_st16(d.g.slot, wr_u4{d.g.payload, 0u, 0u, 0u});
#ifdef WRHIP_HOSTSIM
  unsigned* const lw = nullptr;
#else
  __shared__ unsigned lw[2];           // [0]: a lane saw a difference; [1]: the entry the block takes
#endif
  if (d.g.format == WR_YUV_I420) wr_grab_yuv_delta_block<WR_YUV_I420>(d, lw);
  else if (d.g.format == WR_YUV_NV12) wr_grab_yuv_delta_block<WR_YUV_NV12>(d, lw);
  else wr_grab_yuv_delta_block<WR_YUV_I444>(d, lw);
}
// The slot's header and as many bytes as its count word says, device slot -> pinned host slot, 16 bytes per store.  A small grid on
// the grab stream: the link, not the chip, bounds it, and the raster launches of the following frames keep the CUs.
__global__ void __launch_bounds__(256) wr_grab_push_kernel(WrGrabPushArgs a) {
  const uint32_t payload = wr_load4(a.src);
  unsigned long long n16 = ((unsigned long long)WR_GRAB_HEADER + payload + 15ull) >> 4;
  if (n16 > (unsigned long long)(a.capacity >> 4)) n16 = a.capacity >> 4;
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * step < n16; i += 4 * step) {
    const wr_u4 v0 = wr_load16(a.src + 16 * i), v1 = wr_load16(a.src + 16 * (i + step));
    const wr_u4 v2 = wr_load16(a.src + 16 * (i + 2 * step)), v3 = wr_load16(a.src + 16 * (i + 3 * step));
    wr_grab_st16(a.dst + 16 * i, v0); wr_grab_st16(a.dst + 16 * (i + step), v1);
    wr_grab_st16(a.dst + 16 * (i + 2 * step), v2); wr_grab_st16(a.dst + 16 * (i + 3 * step), v3);
  }
  for (; i < n16; i += step) wr_grab_st16(a.dst + 16 * i, wr_load16(a.src + 16 * i));
}
// WRHIP_GRAB_SCROLL (include/wrhip.h; WrGrabScrollArgs): a packed delta grab that first finds the one vertical scroll most of the
// changed content made, and writes a block that equals the retained copy `scroll_dy` rows away as a 16-byte COPY record.  Four
// launches on the draw stream, a workgroup per block in all but the vote; geometry and piece ownership are wr_grab_pack_kernel's.
//   probe   compares the block with the retained copy at its own place (-> the block's mask of differing rows) and hashes every
//           segment -- a block row -- of the texture and of the retained copy: the sum of its pieces' hashes (a multiply-xor fold of
//           the 16 bytes with the piece's place in the row), added up over the 16 (RGBA8) or 4 (R8) lanes that share the row.  The
//           retained copy is hashed here, every grab: nothing but the copy itself lives from one grab to the next.
//   vote    all pairs of one block column: a workgroup takes WR_SCROLL_VOTE_ROWS rows of the column against 256 candidates, a
//           candidate per lane -- the row's hash is a broadcast, the retained rows' hashes are consecutive LDS words -- and walks
//           the differing rows alone; a workgroup whose rows do not differ leaves at once.  6 KB of LDS.
//   pack    every workgroup of a changed block reduces the votes to scroll_dy (1025 words; block 0 stores it into header word 1),
//           compares the block EXACTLY with the retained copy scroll_dy rows away and takes a COPY record, or packs the block as
//           wr_grab_pack_runs_kernel does.  It does not write the retained copy: other workgroups are reading it.
//   update  the changed blocks, texture -> retained copy.
// Equality is decided by hashes in the vote only.
WR_DEVICE unsigned long long wr_scroll_piece_hash(const wr_u4& v, int pos) {
  const unsigned long long a = (unsigned long long)v.x | (unsigned long long)v.y << 32, b = (unsigned long long)v.z | (unsigned long long)v.w << 32;
  const unsigned long long k = (unsigned long long)(pos + 1);
  unsigned long long h = (a ^ (k * 0x9E3779B97F4A7C15ull)) * 0xFF51AFD7ED558CCDull;
  h ^= h >> 32;
  h += (b ^ (k * 0xC2B2AE3D27D4EB4Full)) * 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 29;
  return h * 0x9FB21C651E98DF25ull;
}
// the rule of the vote as one number: most votes, then the smaller |dy|, then the positive dy; 0: no vote
WR_DEVICE unsigned long long wr_scroll_key(unsigned votes, int dy) {
  const int ad = dy < 0 ? -dy : dy;
  return votes ? ((unsigned long long)votes << 11 | (unsigned long long)(WR_GRAB_SCROLL_MAX - ad) << 1 | (dy > 0 ? 1ull : 0ull)) : 0ull;
}
WR_DEVICE int wr_scroll_key_dy(unsigned long long key) {
  if (key == 0ull) return 0;
  const int ad = WR_GRAB_SCROLL_MAX - (int)((key >> 1) & 1023ull);
  return (key & 1ull) ? ad : -ad;
}
WR_DEVICE const uint8_t* wr_scroll_kept(const WrGrabArgs& a, const WrGrabBlock& B, int r, int o) {
  return B.pk + (ptrdiff_t)r * (ptrdiff_t)a.keep_stride + o;      // (r may be negative: a row above the block)
}
__global__ void __launch_bounds__(256) wr_grab_scroll_probe_kernel(WrGrabScrollArgs s) {
  const WrGrabArgs& a = s.g;
  const int t = (int)threadIdx.x, b = (int)blockIdx.x;
  const WrGrabBlock B = wr_grab_block(a, b);
  const size_t seg0 = (size_t)(b % a.bx) * (size_t)a.rects[0][3] + (size_t)B.y0;
  unsigned long long* hc = s.hash_cur + seg0;
  unsigned long long* hp = s.hash_prev + seg0;
  const int ppr = WR_GRAB_BLOCK * a.bpp / 16;
#ifdef WRHIP_HOSTSIM
  if (t != 0) return;
  if (b == 0) for (int i = 0; i < 2 * WR_GRAB_SCROLL_MAX + 1; i++) s.votes[i] = 0u;
  unsigned long long mask = 0ull;
  for (int row = 0; row < B.bh; row++) {
    unsigned long long c = 0ull, p = 0ull;
    bool diff = false;
    for (int q = 0; q < ppr; q++) {
      wr_u4 v; int r, o;
      if (!wr_grab_piece(a, B, row * ppr + q, v, r, o)) continue;
      const wr_u4 e = wr_load16(wr_scroll_kept(a, B, r, o));
      c += wr_scroll_piece_hash(v, q); p += wr_scroll_piece_hash(e, q);
      diff = diff || wr_grab_differs(v, e);
    }
    hc[row] = c; hp[row] = p;
    if (diff) mask |= 1ull << row;
  }
  s.rowdiff[b] = mask;
#else
  __shared__ unsigned lm[2];           // the mask of differing rows
  if (b == 0) for (int i = t; i < 2 * WR_GRAB_SCROLL_MAX + 1; i += 256) s.votes[i] = 0u;
  if (t < 2) lm[t] = 0u;
  __syncthreads();
  const int pieces = WR_GRAB_BLOCK * ppr;
  for (int k = 0; k < 4; k++) {
    const int piece = k * 256 + t;
    if (piece >= pieces) break;        // (uniform: 1024 pieces or 256)
    wr_u4 v; int r, o;
    unsigned long long c = 0ull, p = 0ull;
    bool diff = false;
    if (wr_grab_piece(a, B, piece, v, r, o)) {
      const wr_u4 e = wr_load16(wr_scroll_kept(a, B, r, o));
      c = wr_scroll_piece_hash(v, piece % ppr); p = wr_scroll_piece_hash(e, piece % ppr);
      diff = wr_grab_differs(v, e);
    }
    for (int m = 1; m < ppr; m <<= 1) { c += __shfl_xor(c, m); p += __shfl_xor(p, m); }
    const unsigned long long bal = __ballot(diff);
    const int lane = t & 63;
    if ((lane & (ppr - 1)) == 0 && r < B.bh) {
      hc[r] = c; hp[r] = p;
      if ((bal >> lane) & ((1ull << ppr) - 1ull)) atomicOr(&lm[r >> 5], 1u << (r & 31));
    }
  }
  __syncthreads();
  if (t == 0) s.rowdiff[b] = (unsigned long long)lm[0] | (unsigned long long)lm[1] << 32;
#endif
}
__global__ void __launch_bounds__(256) wr_grab_scroll_vote_kernel(WrGrabScrollArgs s) {
  const WrGrabArgs& a = s.g;
  const int t = (int)threadIdx.x, h = a.rects[0][3], D = s.dmax;
  int id = (int)blockIdx.x;
  const int chunk = id % s.dy_chunks; id /= s.dy_chunks;
  const int tile = id % s.row_tiles, c = id / s.row_tiles;
  const int r0 = tile * WR_SCROLL_VOTE_ROWS, d0 = -D + chunk * 256;
  const unsigned long long* hc = s.hash_cur + (size_t)c * (size_t)h;
  const unsigned long long* hp = s.hash_prev + (size_t)c * (size_t)h;
#ifdef WRHIP_HOSTSIM
  if (t != 0) return;
  for (int dy = d0; dy < d0 + 256 && dy <= D; dy++) {
    if (dy == 0) continue;
    unsigned n = 0u;
    for (int r = r0; r < r0 + WR_SCROLL_VOTE_ROWS && r < h; r++) {
      const bool differs = (s.rowdiff[(size_t)(r / WR_GRAB_BLOCK) * a.bx + c] >> (r % WR_GRAB_BLOCK)) & 1ull;
      if (differs && r + dy >= 0 && r + dy < h && hc[r] == hp[r + dy]) n++;
    }
    if (n) atomicAdd(&s.votes[dy + WR_GRAB_SCROLL_MAX], n);
  }
#else
  __shared__ unsigned long long lc[WR_SCROLL_VOTE_ROWS], lp[WR_SCROLL_VOTE_ROWS + 256], lmask[WR_SCROLL_VOTE_ROWS / WR_GRAB_BLOCK];
  if (t < WR_SCROLL_VOTE_ROWS / WR_GRAB_BLOCK) {
    const int q = r0 / WR_GRAB_BLOCK + t;
    lmask[t] = q < a.by ? s.rowdiff[(size_t)q * a.bx + c] : 0ull;
  }
  __syncthreads();
  unsigned long long any = 0ull;
  for (int q = 0; q < WR_SCROLL_VOTE_ROWS / WR_GRAB_BLOCK; q++) any |= lmask[q];
  if (any == 0ull) return;
  for (int i = t; i < WR_SCROLL_VOTE_ROWS; i += 256) lc[i] = r0 + i < h ? hc[r0 + i] : 0ull;
  for (int i = t; i < WR_SCROLL_VOTE_ROWS + 255; i += 256) {
    const int rr = r0 + d0 + i;
    lp[i] = rr >= 0 && rr < h ? hp[rr] : 0ull;
  }
  __syncthreads();
  const int dy = d0 + t;
  unsigned n = 0u;
  for (int q = 0; q < WR_SCROLL_VOTE_ROWS / WR_GRAB_BLOCK; q++) {
    unsigned long long m = lmask[q];
    while (m) {
      const int i = q * WR_GRAB_BLOCK + __builtin_ctzll(m);
      m &= m - 1ull;
      const int rr = r0 + i + dy;
      if (rr >= 0 && rr < h && lc[i] == lp[i + t]) n++;
    }
  }
  if (n && dy != 0 && dy <= D) atomicAdd(&s.votes[dy + WR_GRAB_SCROLL_MAX], n);
#endif
}
__global__ void __launch_bounds__(256) wr_grab_scroll_pack_kernel(WrGrabScrollArgs s) {
  const WrGrabArgs& a = s.g;
  const int t = (int)threadIdx.x, b = (int)blockIdx.x;
  const unsigned long long mask = s.rowdiff[b];
  if (mask == 0ull && b != 0) return;
  const int pieces = WR_GRAB_BLOCK * WR_GRAB_BLOCK * a.bpp / 16;
#ifdef WRHIP_HOSTSIM
  // (threads run one after the other: the first does it all)
  if (t != 0) return;
  unsigned long long key = 0ull;
  for (int i = 0; i < 2 * WR_GRAB_SCROLL_MAX + 1; i++) { const unsigned long long k = wr_scroll_key(s.votes[i], i - WR_GRAB_SCROLL_MAX); key = k > key ? k : key; }
  const int dy = wr_scroll_key_dy(key);
  if (b == 0) wr_grab_st4(a.slot + 4, (uint32_t)dy);
  if (mask == 0ull) return;
  const WrGrabBlock B = wr_grab_block(a, b);
  bool copy = dy != 0 && B.y0 + dy >= 0 && B.y0 + dy + B.bh <= a.rects[0][3];
  for (int piece = 0; piece < pieces && copy; piece++) {
    wr_u4 v; int r, o;
    if (wr_grab_piece(a, B, piece, v, r, o)) copy = !wr_grab_differs(v, wr_load16(wr_scroll_kept(a, B, r + dy, o)));
  }
  uint8_t entry[WR_GRAB_ENTRY(4)];
  const unsigned size = copy ? (unsigned)wr_gc_encode_copy(B.x0, B.y0, B.bw, B.bh, entry)
                             : (unsigned)wr_gc_encode_block(B.ps, (size_t)a.tex_stride, B.x0, B.y0, B.bw, B.bh, a.bpp, entry);
  __builtin_memcpy(a.slot + WR_GRAB_HEADER + atomicAdd((unsigned*)a.slot, size), entry, size);
#else
  __shared__ wr_lu4 stage[1024], outb[1024];
  __shared__ unsigned lw[8];           // [0..5]: wr_grab_pack_runs'; [6]: the block is no copy
  __shared__ unsigned long long lk[4];
  unsigned long long key = 0ull;
  for (int i = t; i < 2 * WR_GRAB_SCROLL_MAX + 1; i += 256) { const unsigned long long k = wr_scroll_key(s.votes[i], i - WR_GRAB_SCROLL_MAX); key = k > key ? k : key; }
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long k = __shfl_xor(key, o); key = k > key ? k : key; }
  if ((t & 63) == 0) lk[t >> 6] = key;
  if (t == 0) lw[6] = 0u;
  __syncthreads();
  for (int w = 0; w < 4; w++) key = lk[w] > key ? lk[w] : key;
  const int dy = wr_scroll_key_dy(key);
  if (b == 0 && t == 0) wr_grab_st4(a.slot + 4, (uint32_t)dy);
  if (mask == 0ull) return;
  const WrGrabBlock B = wr_grab_block(a, b);
  if (dy != 0 && B.y0 + dy >= 0 && B.y0 + dy + B.bh <= a.rects[0][3]) {
    bool diff = false;
    for (int k = 0; k < 4; k++) {
      const int piece = k * 256 + t;
      if (piece >= pieces) break;
      wr_u4 v; int r, o;
      if (wr_grab_piece(a, B, piece, v, r, o)) diff = diff || wr_grab_differs(v, wr_load16(wr_scroll_kept(a, B, r + dy, o)));
    }
    if (__ballot(diff) != 0ull && (t & 63) == 0) lw[6] = 1u;
    __syncthreads();
    if (lw[6] == 0u) {
      if (t == 0) wr_grab_st16(a.slot + WR_GRAB_HEADER + atomicAdd((unsigned*)a.slot, 16u), wr_u4{(uint32_t)B.x0, (uint32_t)B.y0, (uint32_t)B.bw | (uint32_t)B.bh << 8 | 3u << 16, 0u});
      return;
    }
  }
  if (a.bpp == 4) wr_grab_pack_runs<4, false>(a, B, t, stage, outb, lw);
  else wr_grab_pack_runs<1, false>(a, B, t, stage, outb, lw);
#endif
}
__global__ void __launch_bounds__(256) wr_grab_scroll_update_kernel(WrGrabScrollArgs s) {
  const WrGrabArgs& a = s.g;
  const int t = (int)threadIdx.x, b = (int)blockIdx.x;
  if (s.rowdiff[b] == 0ull) return;
  const WrGrabBlock B = wr_grab_block(a, b);
  const int pieces = WR_GRAB_BLOCK * WR_GRAB_BLOCK * a.bpp / 16;
#ifdef WRHIP_HOSTSIM
  if (t != 0) return;
  for (int piece = 0; piece < pieces; piece++) {
#else
  for (int piece = t; piece < pieces; piece += 256) {
#endif
    wr_u4 v; int r, o;
    if (wr_grab_piece(a, B, piece, v, r, o)) wr_grab_st16(B.pk + (size_t)r * a.keep_stride + o, v);
  }
}
// WrhipGrabTextureYuvDelta with WRHIP_GRAB_DELTA | WRHIP_GRAB_SCROLL (include/wrhip.h; WrGrabYuvScrollArgs): the delta YUV grab that first finds the one
// vertical scroll most of the changed LUMA made, and sends a block whose samples -- every plane -- equal the retained planes
// scroll_dy rows away as a 16-byte COPY record.  Three launches on the draw stream; blocks, items and their six words are
// wr_grab_yuv_delta_kernel's.
//   probe   converts the block once and writes its samples into the SECOND set of planes (next_*), whole.  It compares them with the
//           retained planes at their own place -- luma rows into the block's row mask, any plane into `changed` -- and hashes every
//           luma segment of both: a thread's eight bytes of a row through wr_scroll_piece_hash, added up over the eight lanes that
//           share the row.  A keyframe is this launch alone: it compares nothing and writes entry i = block i.
//   vote    wr_grab_scroll_vote_kernel, as it is: it sees hashes, row masks and the image's height.  It votes for odd vectors too.
//   pack    every workgroup of a changed block reduces the votes to scroll_dy -- odd candidates passed over in 4:2:0, where no chroma
//           sample survives them; block 0 stores it into header word 1 --, compares the block's samples in next_* EXACTLY with the
//           retained planes scroll_dy luma rows away (chroma: scroll_dy / 2 rows in 4:2:0) and takes a COPY record or a SAMPLES
//           entry with ONE returning atomic on the slot's byte count.  Device sink: a COPY block's samples go from the RETAINED
//           planes into the caller's, a SAMPLES block's from next_*.  Neither set of planes is written by this launch.
// The host then exchanges the two sets: no update launch.
template <int FMT> WR_DEVICE WrYuvdHome wr_yuvs_home(uint8_t* y, uint8_t* cb, uint8_t* cr, int ys, int cs, int x0, int y0) {
  WrYuvdHome K;
  K.ys = ys; K.cs = cs;
  K.y = y + (size_t)y0 * ys + x0;
  const size_t c = FMT == WR_YUV_I444 ? (size_t)y0 * cs + x0 : (size_t)(y0 >> 1) * cs + (FMT == WR_YUV_NV12 ? x0 : x0 >> 1);
  K.c0 = cb + c; K.c1 = cr + c;
  return K;
}
// item j's six words as a home holds them (wr_yuvd_store's places)
template <int FMT> WR_DEVICE void wr_yuvs_load(const WrYuvdHome& K, int j, uint32_t (&e)[6]) {
  const int i = j & 7, r = j >> 3;
  if (FMT == WR_YUV_I444) {
    wr_yuv_ld8(K.y + (size_t)r * K.ys + 8 * i, e[0], e[1]);
    wr_yuv_ld8(K.c0 + (size_t)r * K.cs + 8 * i, e[2], e[3]);
    wr_yuv_ld8(K.c1 + (size_t)r * K.cs + 8 * i, e[4], e[5]);
  } else {
    wr_yuv_ld8(K.y + (size_t)(2 * r) * K.ys + 8 * i, e[0], e[1]);
    wr_yuv_ld8(K.y + (size_t)(2 * r + 1) * K.ys + 8 * i, e[2], e[3]);
    if (FMT == WR_YUV_NV12) wr_yuv_ld8(K.c0 + (size_t)r * K.cs + 8 * i, e[4], e[5]);
    else { e[4] = wr_load4(K.c0 + (size_t)r * K.cs + 4 * i); e[5] = wr_load4(K.c1 + (size_t)r * K.cs + 4 * i); }
  }
}
// -> item j of the block at (x0, y0) has samples inside the image (wr_yuvd_convert's rule); second: so has its lower luma row (4:2:0)
template <int FMT> WR_DEVICE bool wr_yuvs_on(const WrGrabYuvArgs& a, int x0, int y0, int j, bool& second) {
  const int cx = x0 + 8 * (j & 7), ra = y0 + (FMT == WR_YUV_I444 ? j >> 3 : 2 * (j >> 3));
  second = FMT != WR_YUV_I444 && ra + 1 < a.h;
  return cx < a.w && ra < a.h;
}
// the words that are luma: of the item's row, and of its lower row (4:2:0)
WR_DEVICE bool wr_yuvs_luma_differs(const uint32_t (&w)[6], const uint32_t (&e)[6], int k) { return ((w[2 * k] ^ e[2 * k]) | (w[2 * k + 1] ^ e[2 * k + 1])) != 0u; }
// any sample of the item; a lower luma row outside the image is not one
template <int FMT> WR_DEVICE bool wr_yuvs_differs(const uint32_t (&w)[6], const uint32_t (&e)[6], bool second) {
  uint32_t x = (w[0] ^ e[0]) | (w[1] ^ e[1]) | (w[4] ^ e[4]) | (w[5] ^ e[5]);
  if (FMT == WR_YUV_I444 || second) x |= (w[2] ^ e[2]) | (w[3] ^ e[3]);
  return x != 0u;
}
WR_DEVICE unsigned long long wr_yuvs_hash(uint32_t lo, uint32_t hi, int pos) { return wr_scroll_piece_hash(wr_u4{lo, hi, 0u, 0u}, pos); }
WR_DEVICE wr_u4 wr_yuvs_record(int x0, int y0, int bw, int bh, unsigned mode) { return wr_u4{(uint32_t)x0, (uint32_t)y0, (uint32_t)bw | (uint32_t)bh << 8 | mode << 16, 0u}; }
// lm: three LDS words -- the mask of differing luma rows, and "a sample differs"; unused by the host simulation
template <int FMT> WR_DEVICE void wr_grab_yuv_scroll_probe_block(const WrGrabYuvScrollArgs& s, unsigned* lm) {
  constexpr int ITEMS = FMT == WR_YUV_I444 ? 2 : 1;      // per thread
  const WrGrabYuvDeltaArgs& d = s.d;
  const WrGrabYuvArgs& a = d.g;
  const int t = (int)threadIdx.x, b = (int)blockIdx.x;
  const int x0 = (b % d.bx) * WR_GRAB_BLOCK, y0 = (b / d.bx) * WR_GRAB_BLOCK;
  const int bw = wr_imin(WR_GRAB_BLOCK, a.w - x0), bh = wr_imin(WR_GRAB_BLOCK, a.h - y0);
  const WrYuvdHome N = wr_yuvs_home<FMT>(s.next_y, s.next_cb, s.next_cr, d.keep_ys, d.keep_cs, x0, y0);
  if (d.keyframe) {
    // (entry i is block i; nothing is compared)
    const unsigned entry_bytes = d.device ? 16u : (unsigned)WR_YUVD_ENTRY(FMT);
    uint8_t* const e = a.slot ? a.slot + WR_GRAB_HEADER + (size_t)b * entry_bytes : nullptr;
    if (e && t == 0) wr_grab_st16(e, wr_yuvs_record(x0, y0, bw, bh, 0u));
    const WrYuvdHome E = wr_yuvd_body<FMT>(e ? e + 16 : nullptr);
#ifdef WRHIP_HOSTSIM
    (void)lm;
    if (t != 0) return;
    for (int j = 0; j < 256 * ITEMS; j++) {
#else
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
      const int j = k * 256 + t;
#endif
      uint32_t w[6];
      if (!wr_yuvd_convert<FMT>(a, x0, y0, j, w)) continue;
      if (d.device) wr_yuvd_put<FMT>(a, x0, y0, j, w);
      else if (e) wr_yuvd_store<FMT>(E, j, w);
      wr_yuvd_store<FMT>(N, j, w);
    }
    return;
  }
  const WrYuvdHome K = wr_yuvs_home<FMT>(d.keep_y, d.keep_cb, d.keep_cr, d.keep_ys, d.keep_cs, x0, y0);
  const size_t seg0 = (size_t)(b % d.bx) * (size_t)a.h + (size_t)y0;
  unsigned long long* hc = s.hash_cur + seg0;
  unsigned long long* hp = s.hash_prev + seg0;
#ifdef WRHIP_HOSTSIM
  if (t != 0) return;
  if (b == 0) for (int i = 0; i < 2 * WR_GRAB_SCROLL_MAX + 1; i++) s.votes[i] = 0u;
  for (int r = 0; r < bh; r++) hc[r] = hp[r] = 0ull;
  unsigned long long mask = 0ull;
  bool changed = false;
  for (int j = 0; j < 256 * ITEMS; j++) {
    uint32_t w[6], e[6];
    bool second;
    if (!wr_yuvd_convert<FMT>(a, x0, y0, j, w)) continue;
    wr_yuvs_on<FMT>(a, x0, y0, j, second);
    wr_yuvs_load<FMT>(K, j, e);
    wr_yuvd_store<FMT>(N, j, w);
    const int i = j & 7, row = FMT == WR_YUV_I444 ? j >> 3 : 2 * (j >> 3);
    hc[row] += wr_yuvs_hash(w[0], w[1], i); hp[row] += wr_yuvs_hash(e[0], e[1], i);
    if (wr_yuvs_luma_differs(w, e, 0)) mask |= 1ull << row;
    if (second) {
      hc[row + 1] += wr_yuvs_hash(w[2], w[3], i); hp[row + 1] += wr_yuvs_hash(e[2], e[3], i);
      if (wr_yuvs_luma_differs(w, e, 1)) mask |= 1ull << (row + 1);
    }
    changed = changed || wr_yuvs_differs<FMT>(w, e, second);
  }
  s.rowdiff[b] = mask;
  s.changed[b] = changed ? 1u : 0u;
#else
  if (b == 0) for (int i = t; i < 2 * WR_GRAB_SCROLL_MAX + 1; i += 256) s.votes[i] = 0u;
  if (t < 3) lm[t] = 0u;
  __syncthreads();
  const int lane = t & 63;
#pragma unroll
  for (int k = 0; k < ITEMS; k++) {
    const int j = k * 256 + t, i = j & 7, row = FMT == WR_YUV_I444 ? j >> 3 : 2 * (j >> 3);
    uint32_t w[6], e[6];
    bool second = false;
    unsigned long long c0 = 0ull, p0 = 0ull, c1 = 0ull, p1 = 0ull;
    bool dl0 = false, dl1 = false, any = false;
    if (wr_yuvd_convert<FMT>(a, x0, y0, j, w)) {
      wr_yuvs_on<FMT>(a, x0, y0, j, second);
      wr_yuvs_load<FMT>(K, j, e);
      wr_yuvd_store<FMT>(N, j, w);
      c0 = wr_yuvs_hash(w[0], w[1], i); p0 = wr_yuvs_hash(e[0], e[1], i);
      dl0 = wr_yuvs_luma_differs(w, e, 0);
      if (second) {
        c1 = wr_yuvs_hash(w[2], w[3], i); p1 = wr_yuvs_hash(e[2], e[3], i);
        dl1 = wr_yuvs_luma_differs(w, e, 1);
      }
      any = wr_yuvs_differs<FMT>(w, e, second);
    }
    // (the eight lanes of a row, or of a row pair, are neighbours)
    for (int m = 1; m < 8; m <<= 1) {
      c0 += __shfl_xor(c0, m); p0 += __shfl_xor(p0, m);
      if (FMT != WR_YUV_I444) { c1 += __shfl_xor(c1, m); p1 += __shfl_xor(p1, m); }
    }
    const unsigned long long bal0 = __ballot(dl0), bal1 = __ballot(dl1), bala = __ballot(any);
    if ((lane & 7) == 0) {
      if (row < bh) {
        hc[row] = c0; hp[row] = p0;
        if ((bal0 >> lane) & 0xFFull) atomicOr(&lm[row >> 5], 1u << (row & 31));
      }
      if (FMT != WR_YUV_I444 && row + 1 < bh) {
        hc[row + 1] = c1; hp[row + 1] = p1;
        if ((bal1 >> lane) & 0xFFull) atomicOr(&lm[(row + 1) >> 5], 1u << ((row + 1) & 31));
      }
    }
    if (bala != 0ull && lane == 0) lm[2] = 1u;
  }
  __syncthreads();
  if (t == 0) { s.rowdiff[b] = (unsigned long long)lm[0] | (unsigned long long)lm[1] << 32; s.changed[b] = lm[2]; }
#endif
}
__global__ void __launch_bounds__(256) wr_grab_yuv_scroll_probe_kernel(WrGrabYuvScrollArgs s) {
  // (a keyframe's byte count is known on the host and written here, with a vector of 0)
  if (s.d.keyframe && s.d.g.slot && blockIdx.x == 0 && threadIdx.x == 0) wr_grab_st16(s.d.g.slot, wr_u4{s.d.g.payload, 0u, 0u, 0u});
#ifdef WRHIP_HOSTSIM
  unsigned* const lm = nullptr;
#else
  __shared__ unsigned lm[3];
#endif
  if (s.d.g.format == WR_YUV_I420) wr_grab_yuv_scroll_probe_block<WR_YUV_I420>(s, lm);
  else if (s.d.g.format == WR_YUV_NV12) wr_grab_yuv_scroll_probe_block<WR_YUV_NV12>(s, lm);
  else wr_grab_yuv_scroll_probe_block<WR_YUV_I444>(s, lm);
}
// lw: two LDS words -- [0]: a lane found the block to be no copy (cleared by the caller, behind a barrier); [1]: the entry's offset
template <int FMT> WR_DEVICE void wr_grab_yuv_scroll_pack_block(const WrGrabYuvScrollArgs& s, int dy, unsigned* lw) {
  constexpr int ITEMS = FMT == WR_YUV_I444 ? 2 : 1;      // per thread
  const WrGrabYuvDeltaArgs& d = s.d;
  const WrGrabYuvArgs& a = d.g;
  const int t = (int)threadIdx.x, b = (int)blockIdx.x;
  const int x0 = (b % d.bx) * WR_GRAB_BLOCK, y0 = (b / d.bx) * WR_GRAB_BLOCK;
  const int bw = wr_imin(WR_GRAB_BLOCK, a.w - x0), bh = wr_imin(WR_GRAB_BLOCK, a.h - y0);
  const WrYuvdHome N = wr_yuvs_home<FMT>(s.next_y, s.next_cb, s.next_cr, d.keep_ys, d.keep_cs, x0, y0);
  // (the block's source in the retained planes: its rows inside the image, or the block is no copy.  dy is even in 4:2:0)
  bool copy = dy != 0 && y0 + dy >= 0 && y0 + dy + bh <= a.h;
  const WrYuvdHome S = wr_yuvs_home<FMT>(d.keep_y, d.keep_cb, d.keep_cr, d.keep_ys, d.keep_cs, x0, copy ? y0 + dy : y0);
#ifdef WRHIP_HOSTSIM
  (void)lw;
  for (int j = 0; j < 256 * ITEMS && copy; j++) {
    uint32_t w[6], e[6];
    bool second;
    if (!wr_yuvs_on<FMT>(a, x0, y0, j, second)) continue;
    wr_yuvs_load<FMT>(N, j, w); wr_yuvs_load<FMT>(S, j, e);
    copy = !wr_yuvs_differs<FMT>(w, e, second);
  }
  const unsigned size = copy || d.device ? 16u : (unsigned)WR_YUVD_ENTRY(FMT);
  uint8_t* e = nullptr;
  if (a.slot) {
    e = a.slot + WR_GRAB_HEADER + atomicAdd((unsigned*)a.slot, size);
    uint8_t rec[16];
    wr_gc_yuv_encode_record(x0, y0, bw, bh, copy ? WR_GC_COPY : WR_GC_RAW, rec);
    __builtin_memcpy(e, rec, 16);
  }
  if (copy && !d.device) return;
  const WrYuvdHome E = wr_yuvd_body<FMT>(e ? e + 16 : nullptr);
  for (int j = 0; j < 256 * ITEMS; j++) {
    uint32_t w[6];
    bool second;
    if (!wr_yuvs_on<FMT>(a, x0, y0, j, second)) continue;
    wr_yuvs_load<FMT>(copy ? S : N, j, w);
    if (d.device) wr_yuvd_put<FMT>(a, x0, y0, j, w);
    else if (e) wr_yuvd_store<FMT>(E, j, w);
  }
#else
  uint32_t w[ITEMS][6];
  bool on[ITEMS], second[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; k++) {
    on[k] = wr_yuvs_on<FMT>(a, x0, y0, k * 256 + t, second[k]);
    if (on[k]) wr_yuvs_load<FMT>(N, k * 256 + t, w[k]);
  }
  if (copy) {
    bool diff = false;
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
      if (!on[k]) continue;
      uint32_t e[6];
      wr_yuvs_load<FMT>(S, k * 256 + t, e);
      diff = diff || wr_yuvs_differs<FMT>(w[k], e, second[k]);
    }
    if (__ballot(diff) != 0ull && (t & 63) == 0) lw[0] = 1u;
    __syncthreads();
    copy = lw[0] == 0u;
  }
  const unsigned size = copy || d.device ? 16u : (unsigned)WR_YUVD_ENTRY(FMT);
  uint8_t* e = nullptr;
  if (a.slot) {
    if (t == 0) lw[1] = atomicAdd((unsigned*)a.slot, size);
    __syncthreads();
    e = a.slot + WR_GRAB_HEADER + lw[1];
    if (t == 0) wr_grab_st16(e, wr_yuvs_record(x0, y0, bw, bh, copy ? 3u : 0u));
  }
  if (copy) {
    // (device sink: the samples come from the library's retained planes, whatever the caller's hold)
    if (!d.device) return;
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
      if (!on[k]) continue;
      uint32_t r[6];
      wr_yuvs_load<FMT>(S, k * 256 + t, r);
      wr_yuvd_put<FMT>(a, x0, y0, k * 256 + t, r);
    }
    return;
  }
  const WrYuvdHome E = wr_yuvd_body<FMT>(e ? e + 16 : nullptr);
#pragma unroll
  for (int k = 0; k < ITEMS; k++) {
    if (!on[k]) continue;
    if (d.device) wr_yuvd_put<FMT>(a, x0, y0, k * 256 + t, w[k]);
    else if (e) wr_yuvd_store<FMT>(E, k * 256 + t, w[k]);
  }
#endif
}
__global__ void __launch_bounds__(256) wr_grab_yuv_scroll_pack_kernel(WrGrabYuvScrollArgs s) {
  const WrGrabYuvArgs& a = s.d.g;
  const int t = (int)threadIdx.x, b = (int)blockIdx.x;
  const unsigned changed = s.changed[b];
  if (changed == 0u && b != 0) return;
  // the votes reduced to the vector (wr_scroll_key's rule); 4:2:0: even candidates alone
  const bool even = a.format != WR_YUV_I444;
  unsigned long long key = 0ull;
#ifdef WRHIP_HOSTSIM
  // (threads run one after the other: the first does it all)
  if (t != 0) return;
  unsigned* const lw = nullptr;
  for (int i = 0; i < 2 * WR_GRAB_SCROLL_MAX + 1; i++) {
    if (even && (i & 1)) continue;      // (WR_GRAB_SCROLL_MAX is even: i and dy have the same parity)
    const unsigned long long k = wr_scroll_key(s.votes[i], i - WR_GRAB_SCROLL_MAX);
    key = k > key ? k : key;
  }
#else
  __shared__ unsigned lw[2];
  __shared__ unsigned long long lk[4];
  for (int i = t; i < 2 * WR_GRAB_SCROLL_MAX + 1; i += 256) {
    if (even && (i & 1)) continue;      // (WR_GRAB_SCROLL_MAX is even: i and dy have the same parity)
    const unsigned long long k = wr_scroll_key(s.votes[i], i - WR_GRAB_SCROLL_MAX);
    key = k > key ? k : key;
  }
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long k = __shfl_xor(key, o); key = k > key ? k : key; }
  if ((t & 63) == 0) lk[t >> 6] = key;
  if (t == 0) lw[0] = 0u;
  __syncthreads();
  for (int w = 0; w < 4; w++) key = lk[w] > key ? lk[w] : key;
#endif
  const int dy = wr_scroll_key_dy(key);
  if (b == 0 && t == 0 && a.slot) wr_grab_st4(a.slot + 4, (uint32_t)dy);
  if (changed == 0u) return;
  if (a.format == WR_YUV_I420) wr_grab_yuv_scroll_pack_block<WR_YUV_I420>(s, dy, lw);
  else if (a.format == WR_YUV_NV12) wr_grab_yuv_scroll_pack_block<WR_YUV_NV12>(s, dy, lw);
  else wr_grab_yuv_scroll_pack_block<WR_YUV_I444>(s, dy, lw);
}
#endif

// A solid colour on a general quad, one row at a time: the row's span from the edge instances of its run (aa_span / aa_edge /
// aa_dist, rasterize.h:480-562) -- the two edge sums are what costs (Edge::nextRow, one add per row: wr_accum), so they are
// evaluated once per lane-row and shared by the row's pixels.
// (a lane's rows are 4 apart: the next row's sums are the previous row's plus four more adds when both rows lie in the same
// run of the walk -- `prev`, with prev.ok -- instead of the whole sum from the run's first row again)
struct WrQuadRowS { int ok, s0, s1, la1; float lstart, lend, rstart, rend; float xl, xr; int si, y; };
__device__ __noinline__ WrQuadRowS wr_quad_row_setup(const WrQuadRec* Qp, int y, float pxl, float pxr, int psi, int py_) {
  const WrQuadRec& Q = *Qp;
  WrQuadRowS R;
  R.ok = 0; R.s0 = R.s1 = R.la1 = 0; R.lstart = R.rstart = 256.0f; R.lend = R.rend = 0.0f;
  R.xl = R.xr = 0.0f; R.si = -1; R.y = y;
  int si = -1;
  for (int i = 0; i < Q.nseg; i++) if (y >= Q.seg[i].row_a && y < Q.seg[i].row_b) si = i;
  if (si < 0) return R;
  const WrQuadSeg& S = Q.seg[si];
  float xl, xr;
  if (si == psi && y > py_ && y - py_ <= 8) {
    xl = pxl; xr = pxr;
    for (int i = py_; i < y; i++) { xl = xl + S.ls; xr = xr + S.rs; }
  } else {
    wr_quad_row_x(Q, S, y, xl, xr);   // Edge::nextRow, one add per row
  }
  R.xl = xl; R.xr = xr; R.si = si;
  R.ok = 1;
  if (!Q.aa) {
    R.s0 = int(floorf(wr_clamp(xl, S.b0, S.b1) + 0.5f)); R.s1 = int(floorf(wr_clamp(xr, S.b0, S.b1) + 0.5f));
    return R;
  }
  // aa_edge: masked edges use the row's x intercepts rounded out, the others the rounded x
  const float radl = 0.5f * fabsf(S.ls), radr = 0.5f * fabsf(S.rs);
  R.s0 = S.lmask ? int(floorf(wr_clamp(xl - radl, S.b0, S.b1))) : int(floorf(wr_clamp(xl, S.b0, S.b1) + 0.5f));
  R.la1 = S.lmask ? int(ceilf(wr_clamp(xl + radl, S.b0, S.b1))) : int(floorf(wr_clamp(xl, S.b0, S.b1) + 0.5f));
  R.s1 = S.rmask ? int(ceilf(wr_clamp(xr + radr, S.b0, S.b1))) : int(floorf(wr_clamp(xr, S.b0, S.b1) + 0.5f));
  // aa_dist
  if (S.lmask) { const float dx = (-1.0f * 256.0f) * (1.0f / sqrtf(1.0f + S.ls * S.ls)); R.lstart = 128.0f + dx * (xl - 0.5f); R.lend = -dx; }
  if (S.rmask) { const float dx = (1.0f * 256.0f) * (1.0f / sqrtf(1.0f + S.rs * S.rs)); R.rstart = 128.0f + dx * (xr - 0.5f); R.rend = -dx; }
  return R;
}
// One pixel of that row: its coverage (DO_AA, blend.h:433-446), the blend.  Returns the new pixel in the low word and
// 1 << 32 when the pixel is inside the row's span.
__device__ __noinline__ unsigned long long wr_quad_row_pixel_rgba8(WrQuadRowS R, int aa, const WrDrawDesc* D, int blend, uint32_t c0, uint32_t c1,
                                                                    int x, uint32_t dstp_, const WrRuns* runs = nullptr) {
  const unsigned long long dstp = dstp_;
  const unsigned long long HIT = 1ull << 32;
  if (!R.ok || x < R.s0 || x >= R.s1) return dstp;
  WrWide src; src.bg = c0; src.ra = c1;
  if (!aa) return HIT | wr_blend_rgba8(blend, dstp_, src, D);
  // the 4-pixel chunks DO_AA sees start at the span start -- with depth runs, at the start of the run holding x
  int cs = R.s0;
  if (runs) { const int k = wr_find_run(runs, x); if (k >= 0) cs = wr_run_s(runs, k); }
  const int n = x - cs, lane = n & 3, base = cs + (n & ~3);
  const float off = float(4 * (base - R.la1));
  const float dl = (R.lstart + float(R.la1 + lane) * R.lend) + (R.lend / 4.0f) * off;
  const float dr = (R.rstart + float(R.la1 + lane) * R.rend) + (R.rend / 4.0f) * off;
  const uint32_t cov = uint32_t(int(wr_clamp(wr_min(dl, dr), 0.0f, 256.0f) * 1.0f + 0.5f)) & 0xFFFF;
  src.bg = ((((c0 & 0xFFFF) * cov) & 0xFFFF) >> 8) | (((((c0 >> 16) * cov) & 0xFFFF) >> 8) << 16);
  src.ra = ((((c1 & 0xFFFF) * cov) & 0xFFFF) >> 8) | (((((c1 >> 16) * cov) & 0xFFFF) >> 8) << 16);
  return HIT | wr_blend_rgba8(blend, dstp_, src, D);
}

// The edge values of one row of a general quad -- x, the two interpolants and, under perspective, z and 1/w of the run's left
// and right edge: Edge::nextRow, one add per row, i.e. a row-by-row sum (wr_accum) per value.  They are what a pixel of such
// a prim costs, and they only depend on the row: a lane keeps the last row it evaluated (its four pixels of a row share it),
// and its next row, four rows down in the same run, continues the sums with four adds each.
struct WrQuadRowCache { int y, si; float xl, xr, lu, lv, ru, rv, wl, wr, zl, zr; };
WR_DEVICE void wr_quad_row_edges(const WrQuadRec& Q, int si, int y, WrQuadRowCache* C, WrQuadRowCache& L) {
  if (C && C->si == si && C->y == y) { L = *C; return; }
  const WrQuadSeg& S = Q.seg[si];
  if (const float* e = Q.rowtab_stride >= 6 ? wr_quad_rowtab_entry(Q, y) : nullptr) {
    // the row's edge values as the setup stage summed them (wr_quad_build_rowtab)
    L.xl = e[0]; L.xr = e[1]; L.lu = e[2]; L.lv = e[3]; L.ru = e[4]; L.rv = e[5];
    L.wl = L.wr = L.zl = L.zr = 0.0f;
    if (Q.rowtab_stride >= 10) { L.wl = e[6]; L.wr = e[7]; L.zl = e[8]; L.zr = e[9]; }
    L.y = y; L.si = si;
    if (C) *C = L;
    return;
  }
  // (the z / w slots are in use: perspective, or a second varying -- brush_mix_blend, brush_yuv_image, ps_quad_mask's vClipLocalPos.w)
  const bool zw = Q.pad || Q.base_kind == WR_PK_MIX_BLEND || Q.base_kind == WR_PK_YUV || (Q.base_kind == WR_PK_QUAD_MASK && Q.clip.proj != 0);
  const int dy = C ? y - C->y : 0;
  if (C && C->si == si && dy > 0 && dy <= 8) {
    L = *C;
    for (int i = 0; i < dy; i++) {
      L.xl = L.xl + S.ls; L.xr = L.xr + S.rs;
      L.lu = L.lu + S.luvs[0]; L.lv = L.lv + S.luvs[1]; L.ru = L.ru + S.ruvs[0]; L.rv = L.rv + S.ruvs[1];
      if (zw) {
        L.wl = L.wl + Q.persp.lws[si]; L.wr = L.wr + Q.persp.rws[si];
        L.zl = L.zl + Q.persp.lzs[si]; L.zr = L.zr + Q.persp.rzs[si];
      }
    }
  } else {
    L.xl = wr_accum(S.lx, S.ls, y - S.lrow); L.xr = wr_accum(S.rx, S.rs, y - S.rrow);
    L.lu = wr_accum(S.luv[0], S.luvs[0], y - S.lrow); L.lv = wr_accum(S.luv[1], S.luvs[1], y - S.lrow);
    L.ru = wr_accum(S.ruv[0], S.ruvs[0], y - S.rrow); L.rv = wr_accum(S.ruv[1], S.ruvs[1], y - S.rrow);
    L.wl = L.wr = L.zl = L.zr = 0.0f;
    if (zw) {
      L.wl = wr_accum(Q.persp.lw[si], Q.persp.lws[si], y - S.lrow); L.wr = wr_accum(Q.persp.rw[si], Q.persp.rws[si], y - S.rrow);
      L.zl = wr_accum(Q.persp.lz[si], Q.persp.lzs[si], y - S.lrow); L.zr = wr_accum(Q.persp.rz[si], Q.persp.rzs[si], y - S.rrow);
    }
  }
  L.y = y; L.si = si;
  if (C) *C = L;
}

// The packed depth of one pixel of a perspective quad (draw_perspective_spans, rasterize.h:1236-1258 + packDepth :345): the
// row's edges give z at the span's ends (Point3D edges, stepped once per row), stepZW = (right.zw - left.zw) / (right.x -
// left.x), gl_FragCoord.z = init_interp(z at the span start's pixel centre, step) -- three sequential adds -- and every
// 4-pixel chunk, drawn or skipped, adds 4 * step (step_perspective, program.h:145-148) -- in a program that has varyings;
// one without (WrQuadRec::pad == 1) runs its chunks through the plain run / skip, which leave gl_FragCoord.z alone.
__device__ __noinline__ uint32_t wr_persp_depth(const WrQuadRec* Qp, int x, int y, WrQuadRowCache* cache = nullptr) {
  const WrQuadRec& Q = *Qp;
  int si = -1;
  for (int i = 0; i < Q.nseg; i++) if (y >= Q.seg[i].row_a && y < Q.seg[i].row_b) si = i;
  if (si < 0) return 0xFFFFFFFFu;
  const WrQuadSeg& S = Q.seg[si];
  WrQuadRowCache E;
  wr_quad_row_edges(Q, si, y, cache, E);
  const float xl = E.xl, xr = E.xr;
  int s0;
  if (!Q.aa) s0 = int(floorf(wr_clamp(xl, S.b0, S.b1) + 0.5f));
  else s0 = S.lmask ? int(floorf(wr_clamp(xl - 0.5f * fabsf(S.ls), S.b0, S.b1))) : int(floorf(wr_clamp(xl, S.b0, S.b1) + 0.5f));
  const float zl = E.zl, zr = E.zr;
  float stepScale = 1.0f / (xr - xl);
  if (!wr_isfinite(stepScale)) stepScale = 0.0f;
  const float stepZ = (zr - zl) * stepScale;
  const float z0 = zl + stepZ * ((float(s0) + 0.5f) - xl);
  const int k = x - s0;
  if (k < 0) return 0xFFFFFFFFu;
  float zi = z0;
  for (int i = 0; i < (k & 3); i++) zi = zi + stepZ;
  const float zc = Q.pad == 2 ? wr_accum(zi, stepZ * 4.0f, k >> 2) : zi;
  return uint32_t(int(zc * 16777215.0f));
}

// One pixel of an anti-aliased solid quad (DO_AA, blend.h:433-446): src = muldiv256(src, coverage)
// ahead of the blend.  Out of line: its float math must not cost the textured kernels registers.
__device__ __noinline__ uint32_t wr_aa_pixel_rgba8(const WrAARec* Ap, const WrDrawDesc* D, int blend, uint32_t c0, uint32_t c1,
                                                    int n, int x0, uint32_t dstp) {
  const WrAARec& A = *Ap;
  const int lane = n & 3, base = x0 + (n & ~3);
  const float off = float(4 * (base - A.laa_end));
  const float dl = (A.lstart + float(A.laa_end + lane) * A.lend) + (A.lend / 4.0f) * off;
  const float dr = (A.rstart + float(A.laa_end + lane) * A.rend) + (A.rend / 4.0f) * off;
  const uint32_t cov = uint32_t(int(wr_clamp(wr_min(dl, dr), 0.0f, 256.0f) * 1.0f + 0.5f)) & 0xFFFF;
  WrWide src;
  src.bg = ((((c0 & 0xFFFF) * cov) & 0xFFFF) >> 8) | (((((c0 >> 16) * cov) & 0xFFFF) >> 8) << 16);
  src.ra = ((((c1 & 0xFFFF) * cov) & 0xFFFF) >> 8) | (((((c1 >> 16) * cov) & 0xFFFF) >> 8) << 16);
  return wr_blend_rgba8(blend, dstp, src, D);
}

// MASK_ blend keys (blend.h:458-460): src = muldiv255(src, expand_mask(clip mask texel)); the mask is
// sampled 1:1 at (x, y) - swgl_ClipMaskOffset (get_clip_mask, blend.h:357-360)
WR_DEVICE WrWide wr_mask_src(const WrPrim& P, const WrDrawDesc* D, int x, int y, WrWide src) {
  if (!(P.flags & WR_PF_MASKED)) return src;
  const WrTexDesc& mt = D->tex[WR_S_CLIP_MASK];
  const uint32_t m = ((const uint8_t*)mt.ptr)[(size_t)(y - P.mask_off[1]) * mt.stride + (x - P.mask_off[0])];
  const uint32_t mm = m | (m << 16);
  WrWide r;
  r.bg = wr_muldiv255_2(src.bg, mm); r.ra = wr_muldiv255_2(src.ra, mm);
  return r;
}

// brush_image ... DUAL_SOURCE_BLENDING under GL_ONE, GL_ONE_MINUS_SRC1_COLOR (blend.h:496-511): main() writes the colour
// v_color * texel and a second one, texel * swizzle.x + texel.aaaa * swizzle.y; dst' = src + dst - dst x second (under a clip
// mask both terms are scaled by it).  `tx`: the texel main() sampled, (r, g, b, a) floats.
WR_DEVICE uint32_t wr_dual_blend(const WrPrim& P, const WrDrawDesc* D, int x, int y, uint32_t dstp, const float (&tx)[4], uint32_t cov, bool aa) {
  const float sx = P.dual_swz, sy = P.dual == 2 ? -P.dual_swz : 0.0f;
  uint32_t pc[2], ps[2];
  wr_pack_color(wf4{P.fcolor[0] * tx[0], P.fcolor[1] * tx[1], P.fcolor[2] * tx[2], P.fcolor[3] * tx[3]}, pc);
  wr_pack_color(wf4{tx[0] * sx + tx[3] * sy, tx[1] * sx + tx[3] * sy, tx[2] * sx + tx[3] * sy, tx[3] * sx + tx[3] * sy}, ps);
  WrWide s2; s2.bg = pc[0]; s2.ra = pc[1];
  const WrWide dst = wr_unpack(dstp);
  WrWide second; second.bg = wr_muldiv255_2(ps[0], dst.bg); second.ra = wr_muldiv255_2(ps[1], dst.ra);    // applyColor(dst, secondary)
  // (anti-aliased prims of the REPETITION key, blend.h:513-530: AA_BLEND_KEY scales source AND secondary colour by the coverage,
  // AA_MASK_BLEND_KEY scales the mask by it)
  if (P.flags & WR_PF_MASKED) {
    const WrTexDesc& mt = D->tex[WR_S_CLIP_MASK];
    uint32_t m = ((const uint8_t*)mt.ptr)[(size_t)(y - P.mask_off[1]) * mt.stride + (x - P.mask_off[0])];
    if (aa) m = ((m * cov) & 0xFFFFu) >> 8;
    const uint32_t mm = m | (m << 16);
    s2.bg = wr_muldiv255_2(s2.bg, mm); s2.ra = wr_muldiv255_2(s2.ra, mm);
    second.bg = wr_muldiv255_2(second.bg, mm); second.ra = wr_muldiv255_2(second.ra, mm);
  } else if (aa) {
    auto sc = [&](uint32_t c) { return ((((c & 0xFFFFu) * cov) & 0xFFFFu) >> 8) | (((((c >> 16) * cov) & 0xFFFFu) >> 8) << 16); };
    s2.bg = sc(s2.bg); s2.ra = sc(s2.ra); second.bg = sc(second.bg); second.ra = sc(second.ra);
  }
  WrWide res;
  res.bg = wr_sub2(wr_add2(s2.bg, dst.bg), second.bg);
  res.ra = wr_sub2(wr_add2(s2.ra, dst.ra), second.ra);
  return wr_pack(res);
}
// Generic (slow-path) pixel: any prim kind / blend key, one pixel at a time.
// Kept out of line so the fast paths below stay small and the 16 pixels of a
// lane stay in registers.
WR_DEVICE void wr_texture_rgba_f(const WrTexDesc& t, float cu, float cv, float (&c)[4]);
__device__ __noinline__ uint32_t wr_generic_pixel_rgba8(const WrPrim* Pp, const WrDrawDesc* D, int x, int y, uint32_t dstp, const WrRuns* runs = nullptr) {
  const WrPrim& P = *Pp;
  WrWide src;
  if (P.kind == WR_PK_SOLID) {
    src.bg = P.color[0]; src.ra = P.color[1];
  } else if (P.kind == WR_PK_SOLID_MASKED) {
    // applyColor(expand_mask(mask), colour) (swgl_ext.h:11-23); mask texel 1:1 at (x,y) - offset
    const WrTexDesc& mt = D->tex[WR_S_CLIP_MASK];
    const uint32_t m = ((const uint8_t*)mt.ptr)[(size_t)(y - P.mask_off[1]) * mt.stride + (x - P.mask_off[0])];
    WrWide mm; mm.bg = mm.ra = m | (m << 16);
    src = wr_apply_color(mm, P.color);
  } else if (P.dual && P.kind == WR_PK_TEX_FS && P.blend == WR_BLEND_DUAL_SRC) {
    // brush_image ALPHA_PASS,DUAL_SOURCE_BLENDING under GL_ONE, GL_ONE_MINUS_SRC1_COLOR (wr_dual_blend)
    const WrTexDesc& t = D->tex[P.tex_slot];
    const WrTexRow r = wr_tex_row(P, t, y, runs, x);
    float cu, cv;
    wr_tex_tail_uv(P, r, x - r.x0, cu, cv);
    float tx[4];
    wr_texture_rgba_f(t, cu, cv, tx);
    return wr_dual_blend(P, D, x, y, dstp, tx);
  } else {
    src = wr_mask_src(P, D, x, y, wr_tex_pixel(P, D->tex[P.tex_slot], x, y, runs));
  }
  return wr_blend_rgba8(P.blend, dstp, src, D, P.color);
}

struct WrGrad4 { WrWide v[4]; };
__device__ __noinline__ WrGrad4 wr_gradient_row4(const WrPrim* Pp, const WrGradRec* Gp, const WrDrawDesc* D, int x, int y, const WrRuns* runs);
__device__ __noinline__ WrWide wr_filter_pixel(const WrPrim* Pp, const WrFilterRec* Fp, const WrDrawDesc* D, int x, int y, const WrRuns* runs);
__device__ __noinline__ WrWide wr_filter_eval(const WrPrim* Pp, const WrFilterRec* Fp, const WrDrawDesc* D, float cu, float cv);
__device__ __noinline__ WrWide wr_gradient_main(const WrGradRec* Gp, const WrDrawDesc* D, float lu, float lv);
__device__ __noinline__ WrWide wr_quad_mask_pixel(const WrPrim* Pp, const WrClipRec* Cp, const WrDrawDesc* D, int x, int y, const WrRuns* runs, const float* wrow);
__device__ __noinline__ WrWide wr_yuv_pixel(const WrPrim* Pp, const WrYuvRec* Yp, const WrDrawDesc* D, int x, int y, const WrRuns* runs, const float* row);
WR_DEVICE void wr_yuv_main_sample(const WrTexDesc& t, int pl, float cu, float cv, float (&fs)[3]);
WR_DEVICE WrWide wr_yuv_main_rgb(const WrYuvRec& Y, const float (&fs)[3], bool clamp01);
__device__ __noinline__ WrWide wr_mix_blend_pixel(const WrPrim* Pp, const WrMixRec* Mp, const WrDrawDesc* D, int x, int y, const WrRuns* runs);
__device__ __noinline__ WrWide wr_mix_blend_main(const WrMixRec* Mp, const WrDrawDesc* D, float bu, float bv, float su, float sv);
__device__ __noinline__ WrWide wr_svg_filter_pixel(const WrPrim* Pp, const WrSvgRec* Sp, const WrDrawDesc* D, int x, int y, const WrRuns* runs);
WR_DEVICE float wr_r8_texture(const WrTexDesc& t, float u, float v);
WR_DEVICE WrWide wr_quad_mask_eval(const WrClipRec& C, float f0x, float f0y, float f1x, float f1y, float qx, float qy);
// One pixel of a textured prim on a general quad and / or with swgl_antiAlias (WR_PK_TEX_QUAD): this row's span and the
// pixel's coverage as in wr_quad_pixel_rgba8, the edge interpolants stepped row by row (Edge::nextRow), then the base
// kind's span shader / main() evaluation of pixel x - span.start, DO_AA ahead of the clip mask (blend.h:452-460).
__device__ __noinline__ unsigned long long wr_quad_tex_pixel_rgba8(const WrPrim* Pp, const WrQuadRec* Qp, const WrDrawDesc* D, int x, int y,
                                                                    uint32_t dstp_, const WrRuns* runs = nullptr, WrQuadRowCache* cache = nullptr) {
  const WrQuadRec& Q = *Qp;
  const unsigned long long dstp = dstp_;
  const unsigned long long HIT = 1ull << 32;
  int si = -1;
  for (int i = 0; i < Q.nseg; i++) if (y >= Q.seg[i].row_a && y < Q.seg[i].row_b) si = i;
  if (si < 0) return dstp;
  const WrQuadSeg& S = Q.seg[si];
  WrQuadRowCache E;
  wr_quad_row_edges(Q, si, y, cache, E);
  const float xl = E.xl, xr = E.xr;
  int s0, s1;
  uint32_t cov = 256;
  bool aa_skip = false;
  if (!Q.aa) {
    s0 = int(floorf(wr_clamp(xl, S.b0, S.b1) + 0.5f)); s1 = int(floorf(wr_clamp(xr, S.b0, S.b1) + 0.5f));
    // (the prim's box holds every span of the walk, so this changes nothing -- except under gl_ClipDistance, whose cut the
    // setup stage folded into the box: span.intersect(clip_distance_range), rasterize.h:953-955)
    s0 = wr_imax(s0, Pp->x0); s1 = wr_imin(s1, Pp->x1);
    if (x < s0 || x >= s1) return dstp;
  } else {
    const float radl = 0.5f * fabsf(S.ls), radr = 0.5f * fabsf(S.rs);
    const int la0 = S.lmask ? int(floorf(wr_clamp(xl - radl, S.b0, S.b1))) : int(floorf(wr_clamp(xl, S.b0, S.b1) + 0.5f));
    const int la1 = S.lmask ? int(ceilf(wr_clamp(xl + radl, S.b0, S.b1))) : int(floorf(wr_clamp(xl, S.b0, S.b1) + 0.5f));
    const int ra1 = S.rmask ? int(ceilf(wr_clamp(xr + radr, S.b0, S.b1))) : int(floorf(wr_clamp(xr, S.b0, S.b1) + 0.5f));
    if (x < la0 || x >= ra1) return dstp;
    float lstart = 256.0f, lend = 0.0f, rstart = 256.0f, rend = 0.0f;
    if (S.lmask) { const float dx = (-1.0f * 256.0f) * (1.0f / sqrtf(1.0f + S.ls * S.ls)); lstart = 128.0f + dx * (xl - 0.5f); lend = -dx; }
    if (S.rmask) { const float dx = (1.0f * 256.0f) * (1.0f / sqrtf(1.0f + S.rs * S.rs)); rstart = 128.0f + dx * (xr - 0.5f); rend = -dx; }
    int cs = la0;
    if (runs) { const int k = wr_find_run(runs, x); if (k >= 0) cs = wr_run_s(runs, k); }
    const int n = x - cs, lane = n & 3, base = cs + (n & ~3);
    const float off = float(4 * (base - la1));
    const float dl = (lstart + float(la1 + lane) * lend) + (lend / 4.0f) * off;
    const float dr = (rstart + float(la1 + lane) * rend) + (rend / 4.0f) * off;
    cov = uint32_t(int(wr_clamp(wr_min(dl, dr), 0.0f, 256.0f) * 1.0f + 0.5f)) & 0xFFFF;
    // chunks inside the opaque interior skip DO_AA altogether (aa_span's swgl_OpaqueStart / swgl_OpaqueSize, rasterize.h:545-546;
    // blend.h:433-436) -- not the same as multiplying by 256 when a main() output lane exceeds 255 (brush_blend, amount > 1)
    const int ra0 = S.rmask ? int(floorf(wr_clamp(xr - radr, S.b0, S.b1))) : int(floorf(wr_clamp(xr, S.b0, S.b1) + 0.5f));
    aa_skip = (unsigned)(base - la1) < (unsigned)wr_imax(ra0 - la1 - 3, 0);
    s0 = la0; s1 = ra1;
  }
  const bool flat = runs && runs->n < 0;      // a flattened depth row (WrTargetDesc::flat_rows): the whole span, chunk by chunk through main()
  if (runs && !flat) {        // the span the shader sees is the depth run holding x
    const int k = wr_find_run(runs, x);
    if (k >= 0) { s0 = wr_run_s(runs, k); s1 = wr_run_e(runs, k); } else runs = nullptr;
  }
  WrPrim Pl = *Pp;
  Pl.kind = (int16_t)Q.base_kind;
  const WrTexDesc& t = D->tex[Pl.tex_slot];
  const float Lu = E.lu, Lv = E.lv, Ru = E.ru, Rv = E.rv;
  if (Q.base_kind == WR_PK_SOLID_MASKED) {
    // flat colour under swgl_clipMask: the whole chunks of the span go through commit_masked_solid_span (colour x mask, then DO_AA
    // inside blend_span with the mask key overridden, swgl_ext.h:11-23), the < 4 leftover pixels through main() + blend_pixels
    // (DO_AA, then the mask: blend.h:452-460)
    // (perspective: no span shader, every chunk through main())
    const int len = s1 - s0, spanlen = (len >= 4 && !Q.pad && !flat) ? (len & ~3) : 0;
    WrWide src; src.bg = Pl.color[0]; src.ra = Pl.color[1];
    const bool in_span = x - s0 < spanlen;
    if (in_span) {
      const WrTexDesc& mt = D->tex[WR_S_CLIP_MASK];
      const uint32_t m = ((const uint8_t*)mt.ptr)[(size_t)(y - Pl.mask_off[1]) * mt.stride + (x - Pl.mask_off[0])];
      WrWide mm; mm.bg = mm.ra = m | (m << 16);
      src = wr_apply_color(mm, Pl.color);
    }
    if (Q.aa && !aa_skip) {
      const uint32_t c0 = src.bg, c1 = src.ra;
      src.bg = ((((c0 & 0xFFFF) * cov) & 0xFFFF) >> 8) | (((((c0 >> 16) * cov) & 0xFFFF) >> 8) << 16);
      src.ra = ((((c1 & 0xFFFF) * cov) & 0xFFFF) >> 8) | (((((c1 >> 16) * cov) & 0xFFFF) >> 8) << 16);
    }
    if (!in_span) src = wr_mask_src(Pl, D, x, y, src);
    return HIT | wr_blend_rgba8(Pl.blend, dstp_, src, D);
  }
  WrWide src;
  if (Q.pad) {
    // draw_perspective_spans (rasterize.h:1236-1258) + read_perspective_inputs / step_perspective_inputs (glsl-to-cxx
    // lib.rs:660-741): no span shader, every chunk runs main() with v_uv0 = (uv / w interpolated along the span) * (1 /
    // gl_FragCoord.w); both are init_interp lanes at the span start that every chunk, drawn or skipped, advances by 4 steps
    const float wl = E.wl, wr = E.wr;
    float stepScale = 1.0f / (xr - xl);
    if (!wr_isfinite(stepScale)) stepScale = 0.0f;
    const float su = (Ru - Lu) * stepScale, sv = (Rv - Lv) * stepScale, sw = (wr - wl) * stepScale;
    const float start = (float(s0) + 0.5f) - xl;
    const int k = x - s0;
    // the (uv / w, 1 / w) interpolants of lane kk of the span: init_interp lane, then a step of 4 per chunk
    auto lane_at = [&](int kk, float& pu_, float& pv_, float& fw_) {
      pu_ = Lu + su * start; pv_ = Lv + sv * start; fw_ = wl + sw * start;
      for (int i = 0; i < (kk & 3); i++) { pu_ = pu_ + su; pv_ = pv_ + sv; fw_ = fw_ + sw; }
      pu_ = wr_accum(pu_, (su * 4.0f) * 1.0f, kk >> 2); pv_ = wr_accum(pv_, (sv * 4.0f) * 1.0f, kk >> 2);
      fw_ = wr_accum(fw_, sw * 4.0f, kk >> 2);
    };
    if (Q.base_kind == WR_PK_QUAD_MASK) {
      // ps_quad_mask: vClipLocalPos = (xy, 0, 1) / w interpolated, times w per lane; clip_local_pos = .xy / .w of the pixel and of
      // lanes 0 / 1 of its chunk (fwidth).  The varying's w is 1 at the vertices (checked by the setup stage), so its
      // interpolant is the edges' 1 / w itself.
      float px_[3], py_[3];
      const int ks[3] = {k & ~3, (k & ~3) + 1, k};
      for (int j = 0; j < 3; j++) {
        float a_, b_, c_;
        lane_at(ks[j], a_, b_, c_);
        const float wq_ = 1.0f / c_;
        const float vx = a_ * wq_, vy = b_ * wq_, vw = c_ * wq_;
        px_[j] = vx / vw; py_[j] = vy / vw;
      }
      src = wr_quad_mask_eval(Q.clip, px_[0], py_[0], px_[1], py_[1], px_[2], py_[2]);
    } else if (Q.base_kind == WR_PK_MIX_BLEND) {
      // brush_mix_blend: v_backdrop_uv as it is, v_src_uv * mix(gl_FragCoord.w, 1.0, v_perspective.x) -- both varyings interpolated / w
      // along the span (the second one's edge values on this row: sums of its own, WrPerspRec::l2u ..), each clamped to its bounds
      float pu, pv, fw;
      lane_at(k, pu, pv, fw);
      const float wq = 1.0f / fw;
      float bu = pu * wq, bv = pv * wq;
      const float L2u = wr_accum(Q.persp.l2u[si], Q.persp.l2us[si], y - S.lrow), L2v = wr_accum(Q.persp.l2v[si], Q.persp.l2vs[si], y - S.lrow);
      const float R2u = wr_accum(Q.persp.r2u[si], Q.persp.r2us[si], y - S.rrow), R2v = wr_accum(Q.persp.r2v[si], Q.persp.r2vs[si], y - S.rrow);
      const float su2 = (R2u - L2u) * stepScale, sv2 = (R2v - L2v) * stepScale;
      float qu = L2u + su2 * start, qv = L2v + sv2 * start;
      for (int i = 0; i < (k & 3); i++) { qu = qu + su2; qv = qv + sv2; }
      qu = wr_accum(qu, (su2 * 4.0f) * 1.0f, k >> 2); qv = wr_accum(qv, (sv2 * 4.0f) * 1.0f, k >> 2);
      const float pd = (1.0f - fw) * Q.persp.div + fw;
      float su_ = (qu * wq) * pd, sv_ = (qv * wq) * pd;
      bu = wr_clamp(bu, Pl.uv_bounds[0], Pl.uv_bounds[2]); bv = wr_clamp(bv, Pl.uv_bounds[1], Pl.uv_bounds[3]);
      su_ = wr_clamp(su_, Q.mix.s_bounds[0], Q.mix.s_bounds[2]); sv_ = wr_clamp(sv_, Q.mix.s_bounds[1], Q.mix.s_bounds[3]);
      src = wr_mix_blend_main(&Q.mix, D, bu, bv, su_, sv_);
    } else if (Q.base_kind == WR_PK_YUV) {
      // brush_yuv_image: main() on every pixel (sample_yuv in float), vUv_Y and vUv_U each interpolated / w along the span and times
      // 1 / gl_FragCoord.w, each clamped to its own bounds; vUv_V is vUv_U (wr_yuv_persp_ok), sampled from its own plane
      float pu, pv, fw;
      lane_at(k, pu, pv, fw);
      const float wq = 1.0f / fw;
      const float* e = Q.rowtab_stride >= 14 ? wr_quad_rowtab_entry(Q, y) : nullptr;
      const float L2u = e ? e[10] : wr_accum(Q.persp.l2u[si], Q.persp.l2us[si], y - S.lrow), L2v = e ? e[11] : wr_accum(Q.persp.l2v[si], Q.persp.l2vs[si], y - S.lrow);
      const float R2u = e ? e[12] : wr_accum(Q.persp.r2u[si], Q.persp.r2us[si], y - S.rrow), R2v = e ? e[13] : wr_accum(Q.persp.r2v[si], Q.persp.r2vs[si], y - S.rrow);
      const float su2 = (R2u - L2u) * stepScale, sv2 = (R2v - L2v) * stepScale;
      float qu = L2u + su2 * start, qv = L2v + sv2 * start;
      for (int i = 0; i < (k & 3); i++) { qu = qu + su2; qv = qv + sv2; }
      qu = wr_accum(qu, (su2 * 4.0f) * 1.0f, k >> 2); qv = wr_accum(qv, (sv2 * 4.0f) * 1.0f, k >> 2);
      const WrYuvRec& Y = Q.yuv;
      const float cu = qu * wq, cv = qv * wq;
      float fs[3] = {0.f, 0.f, 0.f};
      wr_yuv_main_sample(t, 0, wr_clamp(pu * wq, Pl.uv_bounds[0], Pl.uv_bounds[2]), wr_clamp(pv * wq, Pl.uv_bounds[1], Pl.uv_bounds[3]), fs);
      if (Y.format != 4) wr_yuv_main_sample(D->tex[WR_S_COLOR1], 1, wr_clamp(cu, Y.u_bounds[0], Y.u_bounds[2]), wr_clamp(cv, Y.u_bounds[1], Y.u_bounds[3]), fs);      // (interleaved: sColor0 alone)
      if (Y.format == 3) wr_yuv_main_sample(D->tex[WR_S_COLOR2], 2, wr_clamp(cu, Y.v_bounds[0], Y.v_bounds[2]), wr_clamp(cv, Y.v_bounds[1], Y.v_bounds[3]), fs);
      src = wr_yuv_main_rgb(Y, fs, (Pl.flags & WR_PF_TAIL_MODULATE) != 0);
    } else {
    float pu, pv, fw;
    lane_at(k, pu, pv, fw);
    const float wq = 1.0f / fw;
    float cu = pu * wq, cv = pv * wq;
    if (Q.persp.div >= 0.0f) {       // brush_image: v_uv * mix(gl_FragCoord.w, 1.0, perspective_interpolate)
      const float pd = (1.0f - fw) * Q.persp.div + fw;
      cu = cu * pd; cv = cv * pd;
    }
    cu = cu + Pl.uv_add[0]; cv = cv + Pl.uv_add[1];
    if (Pl.flags & WR_PF_TAIL_CLAMP) { cu = wr_clamp(cu, Pl.uv_bounds[0], Pl.uv_bounds[2]); cv = wr_clamp(cv, Pl.uv_bounds[1], Pl.uv_bounds[3]); }
    // the program's main() with its varying at this pixel
    if (Q.base_kind == WR_PK_TEX_REPEAT && Pl.dual && Pl.blend == WR_BLEND_DUAL_SRC) {
      // (the dual-source REPETITION key under a projective transform: the repeated uv of wr_repeat_dual_pixel from the
      // perspective-correct v_uv, both colours and the coverage into the blend)
      const WrRepeatRec& R = Q.rep;
      const float usx = R.uv_repeat[2] - R.uv_repeat[0], usy = R.uv_repeat[3] - R.uv_repeat[1];
      const float du = wr_max(cu, 0.0f), dv = wr_max(cv, 0.0f);
      float ru = (du - floorf(du)) * usx + R.uv_repeat[0], rv = (dv - floorf(dv)) * usy + R.uv_repeat[1];
      if (du >= R.tile_repeat[0]) ru = R.uv_repeat[2];
      if (dv >= R.tile_repeat[1]) rv = R.uv_repeat[3];
      ru = wr_clamp(ru, Pl.uv_bounds[0], Pl.uv_bounds[2]); rv = wr_clamp(rv, Pl.uv_bounds[1], Pl.uv_bounds[3]);
      float tx[4];
      wr_texture_rgba_f(t, ru, rv, tx);
      return HIT | wr_dual_blend(Pl, D, x, y, dstp_, tx, cov, Q.aa && !aa_skip);
    }
    if (Q.base_kind == WR_PK_TEX_REPEAT) src = wr_repeat_main(Pl, Q.rep, t, cu, cv);
    else if (Q.base_kind == WR_PK_FILTER) src = wr_filter_eval(&Pl, &Q.filt, D, cu, cv);
    else if (Q.base_kind == WR_PK_GRADIENT) src = wr_gradient_main(&Q.grad, D, cu, cv);
    else src = wr_tex_tail_texel(Pl, t, cu, cv);
    }
  } else if (Q.base_kind == WR_PK_MIX_BLEND) {
    // brush_mix_blend on a rotated / skewed (or anti-aliased) quad: this row as a one-row axis-aligned prim, both varyings -- the
    // backdrop's uv from the walk's uv edges, the source's from its z / w slots
    Pl.uvL0[0] = Lu; Pl.uvL0[1] = Lv; Pl.uvR0[0] = Ru; Pl.uvR0[1] = Rv;
    Pl.uvLs[0] = Pl.uvLs[1] = Pl.uvRs[0] = Pl.uvRs[1] = 0.0f;
    Pl.xl = xl; Pl.xr = xr; Pl.x0 = s0; Pl.x1 = s1; Pl.y0 = y; Pl.y1 = y + 1; Pl.rows_linear = 1;
    WrMixRec M2 = Q.mix;
    M2.sL0[0] = E.zl; M2.sL0[1] = E.wl; M2.sR0[0] = E.zr; M2.sR0[1] = E.wr;
    M2.sLs[0] = M2.sLs[1] = M2.sRs[0] = M2.sRs[1] = 0.0f;
    src = wr_mix_blend_pixel(&Pl, &M2, D, x, y, runs);
  } else if (Q.base_kind == WR_PK_GRADIENT || Q.base_kind == WR_PK_FILTER || Q.base_kind == WR_PK_QUAD_MASK || Q.base_kind == WR_PK_YUV) {
    // shader replays that take their interpolants from the prim: hand them this row as a one-row axis-aligned prim (the span
    // [s0, s1), the edges' x and interpolants on this row, no row stepping left to do)
    Pl.uvL0[0] = Lu; Pl.uvL0[1] = Lv; Pl.uvR0[0] = Ru; Pl.uvR0[1] = Rv;
    Pl.uvLs[0] = Pl.uvLs[1] = Pl.uvRs[0] = Pl.uvRs[1] = 0.0f;
    Pl.xl = xl; Pl.xr = xr; Pl.x0 = s0; Pl.x1 = s1; Pl.y0 = y; Pl.y1 = y + 1; Pl.rows_linear = 1;
    if (Q.base_kind == WR_PK_YUV) {
      // brush_yuv_image: the chroma varyings' edge values on this row too -- vUv_U from the walk's second-varying slots, vUv_V from its z / w
      float ch[8];
      const float* e = Q.rowtab_stride >= 14 ? wr_quad_rowtab_entry(Q, y) : nullptr;
      ch[0] = e ? e[10] : wr_accum(Q.persp.l2u[si], Q.persp.l2us[si], y - S.lrow); ch[1] = e ? e[11] : wr_accum(Q.persp.l2v[si], Q.persp.l2vs[si], y - S.lrow);
      ch[2] = e ? e[12] : wr_accum(Q.persp.r2u[si], Q.persp.r2us[si], y - S.rrow); ch[3] = e ? e[13] : wr_accum(Q.persp.r2v[si], Q.persp.r2vs[si], y - S.rrow);
      ch[4] = E.zl; ch[5] = E.wl; ch[6] = E.zr; ch[7] = E.wr;
      src = wr_yuv_pixel(&Pl, &Q.yuv, D, x, y, runs, ch);
    }
    else if (Q.base_kind == WR_PK_GRADIENT) src = wr_gradient_row4(&Pl, &Q.grad, D, x, y, runs).v[0];
    else if (Q.base_kind == WR_PK_FILTER) src = wr_filter_pixel(&Pl, &Q.filt, D, x, y, runs);
    else {
      // (a projective clip transform: vClipLocalPos.w of the two edges on this row, from the walk's z slots)
      const float wrow[2] = {E.zl, E.zr};
      src = wr_quad_mask_pixel(&Pl, &Q.clip, D, x, y, runs, Q.clip.proj ? wrow : nullptr);
    }
  } else if (Q.base_kind == WR_PK_TEX_REPEAT && Pl.dual && Pl.blend == WR_BLEND_DUAL_SRC) {
    // the dual-source REPETITION key on an anti-aliased (or rotated) prim: no span shader under this key, every pixel runs main() --
    // the repeated uv of wr_repeat_dual_pixel from this row's edge interpolants -- and the blend takes both colours and the coverage
    const WrTexRow r = wr_tex_row_span(Pl, t, Lu, Lv, Ru, Rv, xl, xr, s0, s1 - s0, runs, x, true);
    const WrRepeatRec& R = Q.rep;
    const int n = x - r.x0, lane = n & 3, m = n >> 2;
    float lu = wr_pick4(r.lu, lane), lv = wr_pick4(r.lv, lane);
    lu = wr_accum(lu, (r.su * 4.0f) * 1.0f, m); lv = wr_accum(lv, (r.sv * 4.0f) * 1.0f, m);
    const float usx = R.uv_repeat[2] - R.uv_repeat[0], usy = R.uv_repeat[3] - R.uv_repeat[1];
    const float cu = wr_max(lu, 0.0f), cv = wr_max(lv, 0.0f);
    float ru = (cu - floorf(cu)) * usx + R.uv_repeat[0], rv = (cv - floorf(cv)) * usy + R.uv_repeat[1];
    if (cu >= R.tile_repeat[0]) ru = R.uv_repeat[2];
    if (cv >= R.tile_repeat[1]) rv = R.uv_repeat[3];
    ru = wr_clamp(ru, Pl.uv_bounds[0], Pl.uv_bounds[2]); rv = wr_clamp(rv, Pl.uv_bounds[1], Pl.uv_bounds[3]);
    float tx[4];
    wr_texture_rgba_f(t, ru, rv, tx);
    return HIT | wr_dual_blend(Pl, D, x, y, dstp_, tx, cov, Q.aa && !aa_skip);
  } else {
    const WrTexRow r = wr_tex_row_span(Pl, t, Lu, Lv, Ru, Rv, xl, xr, s0, s1 - s0, runs, x, Q.base_kind == WR_PK_TEX_REPEAT && Q.rep.no_span != 0);
    src = Q.base_kind == WR_PK_TEX_REPEAT ? wr_repeat_pixel_row(Pl, Q.rep, t, r, x - r.x0) : wr_tex_pixel_row(Pl, t, r, x - r.x0);
  }
  if (Q.aa && !aa_skip) {
    const uint32_t c0 = src.bg, c1 = src.ra;
    src.bg = ((((c0 & 0xFFFF) * cov) & 0xFFFF) >> 8) | (((((c0 >> 16) * cov) & 0xFFFF) >> 8) << 16);
    src.ra = ((((c1 & 0xFFFF) * cov) & 0xFFFF) >> 8) | (((((c1 >> 16) * cov) & 0xFFFF) >> 8) << 16);
  }
  src = wr_mask_src(Pl, D, x, y, src);
  return HIT | wr_blend_rgba8(Pl.blend, dstp_, src, D, Pl.color);
}

// red channel of a textured prim's fragment value (R8 targets)
__device__ __noinline__ uint32_t wr_tex_pixel_r(const WrPrim* Pp, const WrDrawDesc* D, int x, int y) {
  return wr_tex_pixel(*Pp, D->tex[Pp->tex_slot], x, y).ra & 0xFFFF;
}

// ---------------------------------------------------------------------------
// brush_linear_gradient: the 4 pixels x .. x+3 of row y (WideRGBA8 sources, b,g | r,a as u16 pairs).
//   span part   commitLinearGradient (swgl_ext.h:1390-1578) walks the row from the span start:
//               [run of whole chunks inside one merged table range, colour stepped in 0..0xFF00
//               fixed point] [one per-sample table lookup chunk] ...  A pixel's value depends on
//               the run it falls in, so the walk is replayed up to the chunk(s) holding x .. x+3.
//   the rest    fragment shader: sample_gradient(dot(fract(v_pos), v_scale_dir) - v_start_offset)
//               (brush_linear_gradient.glsl:66-83, gradient.glsl:42-61), also for every pixel when
//               the table fails swgl_validateGradient or the per-chunk delta is not finite.
WR_DEVICE bool wr_stops_merge(const float* stops, int a, int b) {   // GradientStops::can_merge
  const float* sa = stops + 8 * a + 4; const float* sb = stops + 8 * b + 4;
  return sa[0] == sb[0] && sa[1] == sb[1] && sa[2] == sb[2] && sa[3] == sb[3];
}
WR_DEVICE float wr_fract(float v) { return v - floorf(v); }
WR_DEVICE uint32_t wr_u16_round1(float v) { return uint32_t(int(v * 1.0f + 0.5f)) & 0xFFFF; }   // CONVERT(round_pixel(v, 1), U16)

// sampleGradient, one lane (swgl_ext.h:1349-1373): zyxw swizzle, round_pixel, packRGBA8 (wrapping)
WR_DEVICE WrWide wr_sample_gradient(const float* stops, float entry) {
  const int index = int(entry);
  const float offset = entry - float(index);
  const float* st = stops + 8 * index;
  wf4 c = {st[0] + st[4] * offset, st[1] + st[5] * offset, st[2] + st[6] * offset, st[3] + st[7] * offset};
  uint32_t pc[2];
  wr_pack_color(c, pc);
  WrWide w; w.bg = pc[0]; w.ra = pc[1];
  return w;
}

// `runs`: the row's depth runs; only pixel x is evaluated then (out.v[0]), inside the run that holds it.
__device__ __noinline__ WrGrad4 wr_gradient_row4(const WrPrim* Pp, const WrGradRec* Gp, const WrDrawDesc* D, int x, int y, const WrRuns* runs = nullptr) {
  const WrPrim& P = *Pp;
  const WrGradRec& G = *Gp;
  WrGrad4 out;
#pragma unroll
  for (int i = 0; i < 4; i++) { out.v[i].bg = 0; out.v[i].ra = 0; }
  // interpolants of v_pos at the span start (rasterize.h:1003-1017), as wr_tex_row
  const int k = y - P.y0;
  const bool lin = P.rows_linear != 0;
  const float Lu = wr_row_interp(P.uvL0[0], P.uvLs[0], k, lin), Lv = wr_row_interp(P.uvL0[1], P.uvLs[1], k, lin);
  const float Ru = wr_row_interp(P.uvR0[0], P.uvRs[0], k, lin), Rv = wr_row_interp(P.uvR0[1], P.uvRs[1], k, lin);
  float stepScale = 1.0f / (P.xr - P.xl);
  if (!wr_isfinite(stepScale)) stepScale = 0.0f;
  const float su = (Ru - Lu) * stepScale, sv = (Rv - Lv) * stepScale;
  const int kr = runs ? wr_find_run(runs, x) : -1;
  const int X0 = kr >= 0 ? wr_run_s(runs, kr) : P.x0;                    // start of the sub-span the span shader sees
  const int len = kr >= 0 ? wr_run_e(runs, kr) - X0 : P.x1 - P.x0;
  const float start = float(kr >= 0 ? wr_run_s(runs, 0) : P.x0) + 0.5f - P.xl;
  const float sdx = G.scale_dir[0], sdy = G.scale_dir[1];
  int span = len >= 4 ? (len & ~3) : 0;
  // init_interp (glsl.h:3084-3089)
  float px[4], py[4];
  px[0] = Lu + su * start; py[0] = Lv + sv * start;
#pragma unroll
  for (int i = 1; i < 4; i++) { px[i] = px[i - 1] + su; py[i] = py[i - 1] + sv; }
  if (kr > 0) {
    const bool spans = G.stops && wr_isfinite(((px[1] - px[0]) * 4.0f) * sdx + ((py[1] - py[0]) * 4.0f) * sdy);
    wr_run_lanes(runs, kr, Lu, su, P.xl, spans, px);
    wr_run_lanes(runs, kr, Lv, sv, P.xl, spans, py);
  }
  const float ou = px[0], ov = py[0];
  const float lu1 = px[1], lu2 = px[2], lu3 = px[3], lv1 = py[1], lv2 = py[2], lv3 = py[3];   // the lanes at the sub-span start
  const float psx = (px[1] - px[0]) * 4.0f, psy = (py[1] - py[0]) * 4.0f;   // dFdx(pos) * 4
  const float delta = psx * sdx + psy * sdy;
  if (!G.stops || G.radial >= 2 || (!G.radial && !wr_isfinite(delta))) span = 0;
  if (runs && runs->n < 0) span = 0;        // a flattened depth row: every chunk through main()
  const int n_lo = wr_imax(x - X0, 0), n_hi = wr_imin(x + (kr >= 0 ? 0 : 3) - X0, len - 1);
  if (n_hi < n_lo) return out;
  const float size = 128.0f;
  if (G.radial == 1) {
    // commitRadialGradient (swgl_ext.h:1629-1835): the row is walked from the span start -- runs of whole chunks inside one
    // merged table range (colour = colorF + deltaColorF * length(pos) per pixel), per-sample table chunks in between -- with
    // dot(pos, pos) accumulated chunk by chunk; replayed up to the chunk(s) holding x .. x+3
    const float radius = G.start_offset;
    float ddx = px[1] - px[0], ddy = py[1] - py[0];
    float dd = ddx * ddx + ddy * ddy;
    if (!wr_isfinite(dd) || !wr_isfinite(radius)) span = 0;
    if (n_lo < span) {
      const float* stops = G.stops;
      const int c_hi = wr_imin(n_hi, span - 1) >> 2, c_lo = n_lo >> 2;
      const float fspan = float(span);
      float invDelta, middleT, middleB;
      if (dd > 0.0f) {
        invDelta = 1.0f / dd;
        middleT = -(ddx * px[0] + ddy * py[0]) * invDelta;
        middleB = middleT * middleT - (px[0] * px[0] + py[0] * py[0]) * invDelta;
      } else { invDelta = 0.0f; middleT = fspan; middleB = 0.0f; }
      const float mx_ = px[0] + ddx * middleT, my_ = py[0] + ddy * middleT, ex_ = px[0] + ddx * fspan, ey_ = py[0] + ddy * fspan;
      const float mer_x = sqrtf(wr_max(mx_ * mx_ + my_ * my_, 1.0e-12f)), mer_y = sqrtf(wr_max(ex_ * ex_ + ey_ * ey_, 1.0e-12f));
      const float middleRadius = fspan < middleT ? mer_y : mer_x, endRadius = mer_y;
      ddx *= 4.0f; ddy *= 4.0f; dd *= 16.0f;
      float dotPos[4], dotPosDelta[4], off[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { dotPos[i] = px[i] * px[i] + py[i] * py[i]; dotPosDelta[i] = 2.0f * (px[i] * ddx + py[i] * ddy) + dd; }
      const float dd2 = 2.0f * dd;
      for (int t = 0; t < span && (t >> 2) <= c_hi;) {
#pragma unroll
        for (int i = 0; i < 4; i++) off[i] = sqrtf(wr_max(dotPos[i], 1.0e-12f)) - radius;
        float startRadius = radius;
        if (G.repeat != 0.0f) {
          startRadius += off[0];
#pragma unroll
          for (int i = 0; i < 4; i++) off[i] = wr_fract(off[i]);
          startRadius -= off[0];
        }
        float intercept = -1.0f;
        int minIndex = 0, maxIndex = int(1.0f + size);
        const bool past = float(t) >= middleT;
        if (off[0] < 0.0f) {
          maxIndex = minIndex;
          if (past) intercept = radius;
        } else if (off[0] < 1.0f) {
          minIndex = int(1.0f + off[0] * size);
          maxIndex = minIndex;
          const float searchOffset = (past ? endRadius : middleRadius) - startRadius;
          const int searchIndex = int(wr_clamp(1.0f + size * searchOffset, 1.0f, size));
          if (past) {
            // (while (maxIndex + 1 <= searchIndex && can_merge(maxIndex, maxIndex + 1)) maxIndex++, by the prim's merge bitmap)
            if (maxIndex + 1 <= searchIndex) maxIndex = wr_imin(wr_merge_clear_from(G, maxIndex), searchIndex);
            intercept = float(maxIndex + 1);
          } else {
            if (minIndex - 1 >= searchIndex) minIndex = wr_imax(wr_merge_clear_below(G, minIndex) + 1, searchIndex);
            intercept = float(minIndex);
          }
          intercept = wr_clamp((intercept - 1.0f) / size, 0.0f, 1.0f) + startRadius;
        } else {
          minIndex = maxIndex;
          if (!past) intercept = radius + 1.0f;
        }
        float endT = past ? fspan : float(wr_imin(span, int(middleT)));
        if (intercept >= 0.0f) {
          float b = middleB + intercept * intercept * invDelta;
          if (b > 0.0f) { b = sqrtf(b); endT = wr_min(endT, past ? middleT + b : middleT - b); }
          else endT = wr_min(endT, middleT);
        }
        if (float(t) + 4.0f <= endT) {
          const int inside = int(endT - float(t)) & ~3;
          const float* s0 = stops + 8 * minIndex; const float* s1 = stops + 8 * maxIndex;
          const float mn[4] = {s0[2] * 255.0f, s0[1] * 255.0f, s0[0] * 255.0f, s0[3] * 255.0f};
          const float mxc[4] = {(s1[2] + s1[6]) * 255.0f, (s1[1] + s1[5]) * 255.0f, (s1[0] + s1[4]) * 255.0f, (s1[3] + s1[7]) * 255.0f};
          const float k = size / float(maxIndex + 1 - minIndex);
          const float base = startRadius + float(minIndex - 1) / size;
          float dcol[4], col[4];
#pragma unroll
          for (int q = 0; q < 4; q++) { dcol[q] = (mxc[q] - mn[q]) * k; col[q] = mn[q] - dcol[q] * base; }
          for (int c = 0; c < inside; c += 4) {
            const int chunk = (t + c) >> 2;
            if (chunk >= c_lo && chunk <= c_hi) {
#pragma unroll
              for (int i = 0; i < 4; i++) {
                const int o = X0 + t + c + i - x;
                if (o >= 0 && o < 4) {
                  const float og = sqrtf(dotPos[i]);
                  const uint32_t cb = wr_u16_round1(col[0] + dcol[0] * og), cg = wr_u16_round1(col[1] + dcol[1] * og);
                  const uint32_t cr = wr_u16_round1(col[2] + dcol[2] * og), ca = wr_u16_round1(col[3] + dcol[3] * og);
                  out.v[o].bg = cb | (cg << 16); out.v[o].ra = cr | (ca << 16);
                }
              }
            }
#pragma unroll
            for (int i = 0; i < 4; i++) { dotPos[i] += dotPosDelta[i]; dotPosDelta[i] += dd2; }
          }
          t += inside;
          if (t >= span) break;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            off[i] = sqrtf(wr_max(dotPos[i], 1.0e-12f)) - radius;
            if (G.repeat != 0.0f) off[i] = wr_fract(off[i]);
          }
        }
        const int chunk = t >> 2;
        if (chunk >= c_lo && chunk <= c_hi) {
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int o = X0 + t + i - x;
            if (o >= 0 && o < 4) out.v[o] = wr_sample_gradient(stops, wr_clamp(off[i] * size + 1.0f, 0.0f, 1.0f + size));
          }
        }
        t += 4;
#pragma unroll
        for (int i = 0; i < 4; i++) { dotPos[i] += dotPosDelta[i]; dotPosDelta[i] += dd2; }
      }
    }
  } else if (n_lo < span) {
    const float* stops = G.stops;
    const int c_lo = n_lo >> 2, c_hi = wr_imin(n_hi, span - 1) >> 2;     // chunks wanted
    float dcxx = 0.25f * float(span), dcxy = 0.0f, dcyx = dcxx, dcyy = 0.0f;
    const bool tile = G.no_tile == 0;      // tileRepeat (swgl_ext.h:1411-1432)
    if (tile && psx != 0.0f) { const float r = 1.0f / psx; dcxx = (psx >= 0.0f ? 1.0f : 0.0f) * r; dcxy = 1.0f * r; }
    if (tile && psy != 0.0f) { const float r = 1.0f / psy; dcyx = (psy >= 0.0f ? 1.0f : 0.0f) * r; dcyy = 1.0f * r; }
    int left = span, chunk = 0;          // chunk: index of the next chunk to be produced
    while (left > 0 && chunk <= c_hi) {
      float chunks = 0.25f * float(left);
      float rx[4], ry[4], off[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { rx[i] = tile ? wr_fract(px[i]) : px[i]; ry[i] = tile ? wr_fract(py[i]) : py[i]; }
      if (tile) {
        chunks = wr_min(chunks, dcxx - rx[0] * dcxy);
        chunks = wr_min(chunks, dcyx - ry[0] * dcyy);
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        off[i] = rx[i] * sdx + ry[i] * sdy - G.start_offset;
        if (G.repeat != 0.0f) off[i] = wr_fract(off[i]);
      }
      float startEntry;
      int minIndex, maxIndex;
      if (off[0] < 0.0f) {
        startEntry = 0.0f; minIndex = maxIndex = 0;
        if (delta > 0.0f) chunks = wr_min(chunks, -off[0] / delta);
      } else if (off[0] < 1.0f) {
        startEntry = 1.0f + off[0] * size;
        if (delta < 0.0f) chunks = wr_min(chunks, -off[0] / delta);
        else if (delta > 0.0f) chunks = wr_min(chunks, (1.0f - off[0]) / delta);
        const float endEntry = wr_clamp(1.0f + (off[0] + delta * float(int(chunks))) * size, 0.0f, 1.0f + size);
        minIndex = maxIndex = int(startEntry);
        if (delta > 0.0f) {
          // (while (float(maxIndex + 1) < endEntry && can_merge(maxIndex, maxIndex + 1)) maxIndex++, by the prim's merge bitmap: the walk
          // ends at the first entry whose bit is clear or at the first j with j + 1 >= endEntry, i.e. j = ceil(endEntry) - 1)
          if (float(maxIndex + 1) < endEntry) maxIndex = wr_imin(wr_merge_clear_from(G, maxIndex), wr_imax(maxIndex, int(ceilf(endEntry)) - 1));
          chunks = wr_min(chunks, (float(maxIndex + 1) - startEntry) / (delta * size));
        } else if (delta < 0.0f) {
          // (while (float(minIndex - 1) > endEntry && can_merge(minIndex - 1, minIndex)) minIndex--: down to the entry above the last
          // clear bit below, or to the first j with j - 1 <= endEntry, i.e. j = floor(endEntry) + 1)
          if (float(minIndex - 1) > endEntry) minIndex = wr_imax(wr_merge_clear_below(G, minIndex) + 1, wr_imin(minIndex, int(floorf(endEntry)) + 1));
          chunks = wr_min(chunks, (float(minIndex) - startEntry) / (delta * size));
        }
      } else {
        startEntry = 1.0f + size; minIndex = maxIndex = int(startEntry);
        if (delta < 0.0f) chunks = wr_min(chunks, (1.0f - off[0]) / delta);
      }
      if (chunks >= 1.0f) {
        const int inside = int(chunks);
        if (chunk + inside > c_lo) {
          // colours of the merged range in 0..0xFF00, BGRA order
          const float* s0 = stops + 8 * minIndex; const float* s1 = stops + 8 * maxIndex;
          const float mn[4] = {s0[2] * 65280.0f, s0[1] * 65280.0f, s0[0] * 65280.0f, s0[3] * 65280.0f};
          const float mx[4] = {(s1[2] + s1[6]) * 65280.0f, (s1[1] + s1[5]) * 65280.0f, (s1[0] + s1[4]) * 65280.0f,
                               (s1[3] + s1[7]) * 65280.0f};
          const float inv = 1.0f / float(maxIndex + 1 - minIndex);
          const float se = startEntry - float(minIndex), ds = delta * size;
          for (int c = wr_imax(c_lo, chunk); c <= c_hi && c < chunk + inside; c++) {
            const int kk = c - chunk, seg = kk >> 6, r = kk & 63;
            uint32_t ch[4][4];           // [pixel][channel]
#pragma unroll
            for (int q = 0; q < 4; q++) {
              const float range = (mx[q] - mn[q]) * inv;
              float cf = mn[q] + range * se + 128.0f;
              const float dcf = range * ds;
              const uint32_t dc = wr_u16_round1(dcf);
              for (int t = 0; t < seg; t++) cf += dcf * 64.0f;
              ch[0][q] = ((wr_u16_round1(cf) + uint32_t(r) * dc) & 0xFFFF) >> 8;
              ch[1][q] = ((wr_u16_round1(cf + dcf * 0.25f) + uint32_t(r) * dc) & 0xFFFF) >> 8;
              ch[2][q] = ((wr_u16_round1(cf + dcf * 0.5f) + uint32_t(r) * dc) & 0xFFFF) >> 8;
              ch[3][q] = ((wr_u16_round1(cf + dcf * 0.75f) + uint32_t(r) * dc) & 0xFFFF) >> 8;
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int o = X0 + 4 * c + i - x;
              if (o >= 0 && o < 4) { out.v[o].bg = ch[i][0] | (ch[i][1] << 16); out.v[o].ra = ch[i][2] | (ch[i][3] << 16); }
            }
          }
        }
        chunk += inside;
        left -= inside * 4;
        if (left <= 0) break;
        const float fi = float(inside);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          px[i] += psx * fi; py[i] += psy * fi;
          off[i] = (tile ? wr_fract(px[i]) : px[i]) * sdx + (tile ? wr_fract(py[i]) : py[i]) * sdy - G.start_offset;
          if (G.repeat != 0.0f) off[i] = wr_fract(off[i]);
        }
      }
      if (chunk >= c_lo && chunk <= c_hi) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int o = X0 + 4 * chunk + i - x;
          if (o >= 0 && o < 4) out.v[o] = wr_sample_gradient(stops, wr_clamp(off[i] * size + 1.0f, 0.0f, 1.0f + size));
        }
      }
      chunk++;
      left -= 4;
#pragma unroll
      for (int i = 0; i < 4; i++) { px[i] += psx; py[i] += psy; }
    }
  }
  if (n_hi >= span) {
    // main() pixels: init_interp lane, step_interp_inputs(drawn) once, then one step per chunk run
    const WrTexDesc& gb = D->tex[WR_S_GPU_BUFFER_F];
    for (int n = wr_imax(n_lo, span); n <= n_hi; n++) {
      const int lane = (n - span) & 3, m = (n - span) >> 2;
      float lu = lane == 0 ? ou : (lane == 1 ? lu1 : (lane == 2 ? lu2 : lu3));
      float lv = lane == 0 ? ov : (lane == 1 ? lv1 : (lane == 2 ? lv2 : lv3));
      if (span > 0) {
        const float chunks = float(span) * 0.25f;
        lu = lu + (su * 4.0f) * chunks; lv = lv + (sv * 4.0f) * chunks;
      }
      lu = wr_accum(lu, (su * 4.0f) * 1.0f, m); lv = wr_accum(lv, (sv * 4.0f) * 1.0f, m);
      float offset = (G.no_tile ? lu : wr_fract(lu)) * sdx + (G.no_tile ? lv : wr_fract(lv)) * sdy - G.start_offset;
      if (G.radial == 1) offset = sqrtf(lu * lu + lv * lv) - G.start_offset;              // length(v_pos) - v_start_radius.x
      if (G.radial == 3) {                                                                // ps_quad_conic_gradient.glsl:60-81 (approx_atan2)
        const float ax_ = fabsf(lu), ay_ = fabsf(lv);
        const float slope = wr_min(ax_, ay_) / wr_max(ax_, ay_);
        const float s2 = slope * slope;
        float r = ((-0.0464964749f * s2 + 0.15931422f) * s2 - 0.327622764f) * s2 * slope + slope;
        r = ay_ > ax_ ? 1.57079637f - r : r;
        r = lu < 0.0f ? 3.14159274f - r : r;
        r = r * copysignf(1.0f, lv);
        offset = wr_fract((r + G.conic_angle) / (2.0f * 3.141592653589793f)) * G.conic_scale - G.start_offset;
      }
      if (G.radial == 2) {                                                                // cs_conic_gradient.glsl:52-65
        const float cur = atan2f(lv - G.scale_dir[1], lu - G.scale_dir[0]) + G.conic_angle;
        offset = wr_fract(cur / (2.0f * 3.141592653589793f)) * G.conic_scale - G.start_offset;
      }
      offset -= floorf(offset) * G.repeat;
      const float xe = wr_clamp(1.0f + offset * 128.0f, 0.0f, 1.0f + 128.0f);
      const float ei = floorf(xe), ef = xe - ei;
      const int addr = G.address + 2 * int(ei);
      wf4 t0, t1;
      if (G.table) { const float* te = G.table + 8 * int(ei); t0 = wf4{te[0], te[1], te[2], te[3]}; t1 = wf4{te[4], te[5], te[6], te[7]}; }
      else {
        t0 = wr_fetch_f(gb, int(unsigned(addr) % 1024u), int(unsigned(addr) / 1024u));
        t1 = wr_fetch_f(gb, int(unsigned(addr) % 1024u) + 1, int(unsigned(addr) / 1024u));
      }
      uint32_t pc[2];
      wr_pack_color(wf4{t0.x + t1.x * ef, t0.y + t1.y * ef, t0.z + t1.z * ef, t0.w + t1.w * ef}, pc);
      out.v[X0 + n - x].bg = pc[0]; out.v[X0 + n - x].ra = pc[1];
    }
  }
  return out;
}
// main() of the gradient programs for one pixel whose v_pos is (lu, lv) (brush_linear_gradient.glsl:66-83, gradient.glsl:42-61; the
// radial / conic quad patterns): what the loop above evaluates for the pixels the span shader leaves -- and what every pixel of
// a prim under a perspective transform runs, with the perspective-correct v_pos
__device__ __noinline__ WrWide wr_gradient_main(const WrGradRec* Gp, const WrDrawDesc* D, float lu, float lv) {
  const WrGradRec& G = *Gp;
  const WrTexDesc& gb = D->tex[WR_S_GPU_BUFFER_F];
  const float sdx = G.scale_dir[0], sdy = G.scale_dir[1];
  float offset = (G.no_tile ? lu : wr_fract(lu)) * sdx + (G.no_tile ? lv : wr_fract(lv)) * sdy - G.start_offset;
  if (G.radial == 1) offset = sqrtf(lu * lu + lv * lv) - G.start_offset;
  if (G.radial == 3) {
    const float ax_ = fabsf(lu), ay_ = fabsf(lv);
    const float slope = wr_min(ax_, ay_) / wr_max(ax_, ay_);
    const float s2 = slope * slope;
    float r = ((-0.0464964749f * s2 + 0.15931422f) * s2 - 0.327622764f) * s2 * slope + slope;
    r = ay_ > ax_ ? 1.57079637f - r : r;
    r = lu < 0.0f ? 3.14159274f - r : r;
    r = r * copysignf(1.0f, lv);
    offset = wr_fract((r + G.conic_angle) / (2.0f * 3.141592653589793f)) * G.conic_scale - G.start_offset;
  }
  if (G.radial == 2) {
    const float cur = atan2f(lv - G.scale_dir[1], lu - G.scale_dir[0]) + G.conic_angle;
    offset = wr_fract(cur / (2.0f * 3.141592653589793f)) * G.conic_scale - G.start_offset;
  }
  offset -= floorf(offset) * G.repeat;
  const float xe = wr_clamp(1.0f + offset * 128.0f, 0.0f, 1.0f + 128.0f);
  const float ei = floorf(xe), ef = xe - ei;
  const int addr = G.address + 2 * int(ei);
  wf4 t0, t1;
  if (G.table) { const float* te = G.table + 8 * int(ei); t0 = wf4{te[0], te[1], te[2], te[3]}; t1 = wf4{te[4], te[5], te[6], te[7]}; }
  else {
    t0 = wr_fetch_f(gb, int(unsigned(addr) % 1024u), int(unsigned(addr) / 1024u));
    t1 = wr_fetch_f(gb, int(unsigned(addr) % 1024u) + 1, int(unsigned(addr) / 1024u));
  }
  uint32_t pc[2];
  wr_pack_color(wf4{t0.x + t1.x * ef, t0.y + t1.y * ef, t0.z + t1.z * ef, t0.w + t1.w * ef}, pc);
  WrWide w; w.bg = pc[0]; w.ra = pc[1];
  return w;
}

// ---------------------------------------------------------------------------
// cs_blur, one destination pixel.  Returns the unpacked source value(s) that go
// to the blend stage: 4 x u16 (RGBA8 targets) or the value in .bg's low half (R8).
//   span part   blendGaussianBlur (swgl_ext.h:951-978): 4-pixel chunks from the
//               integer texel position of the span start, while they fit in
//               min(bounds.z, start + span, width); 8.8 fixed-point taps with
//               saturating adds (texture.h:1165-1308)
//   the rest    the float fragment shader (cs_blur.glsl:137-181)
// ---------------------------------------------------------------------------
// brush_blend fragment shader (brush_blend.glsl:91-120, blend.glsl:90-237), one pixel.
// swgl has no span shader for it: main() runs on every 4-pixel chunk with glsl.h's float
// vectors, so the restatement is per pixel in strict fp32, same operation order.
// pow() is glsl.h's approximation (glsl.h:776-799), not libm -- restated bit for bit.
WR_DEVICE float wr_glsl_floor(float v) {            // glsl.h:687-690
  const float roundtrip = float(int(v));
  return roundtrip - (roundtrip > v ? 1.0f : 0.0f);
}
WR_DEVICE float wr_approx_log2(float x) {           // glsl.h:776-784
  uint32_t b; __builtin_memcpy(&b, &x, 4);
  const float e = float(b) * (1.0f / (1 << 23));
  const uint32_t mb = (b & 0x007fffffu) | 0x3f000000u;
  float m; __builtin_memcpy(&m, &mb, 4);
  return e - 124.225514990f - 1.498030302f * m - 1.725879990f / (0.3520887068f + m);
}
WR_DEVICE float wr_approx_pow2(float x) {           // glsl.h:786-791; roundfast = cast(v * scale + 0.5f) (portable path)
  const float f = x - wr_glsl_floor(x);
  const float t = x + 121.274057500f - 1.490129070f * f + 27.728023300f / (4.84252568f - f);
  const int32_t r = int32_t((1.0f * (1 << 23)) * t + 0.5f);
  float o; __builtin_memcpy(&o, &r, 4);
  return o;
}
WR_DEVICE float wr_glsl_pow(float x, float y) {     // glsl.h:797-799
  return (x == 0.0f || x == 1.0f) ? x : wr_approx_pow2(wr_approx_log2(x) * y);
}

__device__ __noinline__ WrWide wr_filter_eval(const WrPrim* Pp, const WrFilterRec* Fp, const WrDrawDesc* D, float cu, float cv);
__device__ __noinline__ WrWide wr_filter_pixel(const WrPrim* Pp, const WrFilterRec* Fp, const WrDrawDesc* D, int x, int y, const WrRuns* runs = nullptr) {
  const WrPrim& P = *Pp;
  const WrTexDesc& t = D->tex[P.tex_slot];
  // v_uv of this pixel as the 4-wide fragment loop steps it, clamped to v_uv_sample_bounds
  const WrTexRow r = wr_tex_row(P, t, y, runs, x);
  float cu, cv;
  wr_tex_tail_uv(P, r, x - r.x0, cu, cv);
  return wr_filter_eval(Pp, Fp, D, cu, cv);
}
// ... from the (clamped) uv on: texture(), CalculateFilter, the fragment colour
__device__ __noinline__ WrWide wr_filter_eval(const WrPrim* Pp, const WrFilterRec* Fp, const WrDrawDesc* D, float cu, float cv) {
  const WrPrim& P = *Pp;
  const WrFilterRec& F = *Fp;
  const WrTexDesc& t = D->tex[P.tex_slot];
  // texture(sColor0, uv): texture.h:1028-1071 (linear RGBA8, 7-bit fractions) / nearest
  const float W = t.sw, H = t.sh;
  float cr, cg, cb, ca;
  if (!t.ptr) { cr = cg = cb = ca = 0.0f; }
  else if (t.format == WR_FMT_R8) {
    float m;
    if (t.linear) m = float(wr_sample_linear_r8(t, int(cu * W * 128.0f + (0.5f - 64.0f)), int(cv * H * 128.0f + (0.5f - 64.0f)))) * (1.0f / 255.0f);
    else m = float(((const uint8_t*)t.ptr)[(size_t)wr_clamp_coord(int(cu * W), t.width) + (size_t)wr_clamp_coord(int(cv * H), t.height) * t.stride]) * (1.0f / 255.0f);
    cr = m; cg = 0.0f; cb = 0.0f; ca = 1.0f;
  } else if (t.linear) {
    const WrWide s = wr_sample_linear_rgba8(t, int(cu * W * 128.0f + (0.5f - 64.0f)), int(cv * H * 128.0f + (0.5f - 64.0f)));
    cb = float(s.bg & 0xFFFF) * (1.0f / 255.0f); cg = float(s.bg >> 16) * (1.0f / 255.0f);
    cr = float(s.ra & 0xFFFF) * (1.0f / 255.0f); ca = float(s.ra >> 16) * (1.0f / 255.0f);
  } else {
    const uint32_t p = ((const uint32_t*)t.ptr)[(size_t)wr_clamp_coord(int(cu * W), t.width) + (size_t)wr_clamp_coord(int(cv * H), t.height) * t.stride];
    cb = float(p & 0xFF) * (1.0f / 255.0f); cg = float((p >> 8) & 0xFF) * (1.0f / 255.0f);
    cr = float((p >> 16) & 0xFF) * (1.0f / 255.0f); ca = float(p >> 24) * (1.0f / 255.0f);
  }
  // CalculateFilter (blend.glsl:190-237): un-premultiply, filter
  float alpha = ca;
  float c[3] = {alpha != 0.0f ? cr / alpha : cr, alpha != 0.0f ? cg / alpha : cg, alpha != 0.0f ? cb / alpha : cb};
  const float amount = F.amount;
  switch (F.op) {
    case 0:   // FILTER_CONTRAST
      for (int i = 0; i < 3; i++) c[i] = wr_clamp(c[i] * amount - 0.5f * amount + 0.5f, 0.0f, 1.0f);
      break;
    case 3:   // FILTER_INVERT: mix(Cs, 1 - Cs, amount)
      for (int i = 0; i < 3; i++) c[i] = ((1.0f - c[i]) - c[i]) * amount + c[i];
      break;
    case 6:   // FILTER_BRIGHTNESS
      for (int i = 0; i < 3; i++) c[i] = wr_clamp(c[i] * amount, 0.0f, 1.0f);
      break;
    case 8:   // FILTER_SRGB_TO_LINEAR
      for (int i = 0; i < 3; i++) {
        const float c1 = c[i] / 12.92f, c2 = wr_glsl_pow(c[i] / 1.055f + (0.055f / 1.055f), 2.4f);
        c[i] = c[i] <= 0.04045f ? c1 : c2;
      }
      break;
    case 9:   // FILTER_LINEAR_TO_SRGB
      for (int i = 0; i < 3; i++) {
        const float c1 = c[i] * 12.92f, c2 = 1.055f * wr_glsl_pow(c[i], 1.0f / 2.4f) - 0.055f;
        c[i] = c[i] <= 0.0031308f ? c1 : c2;
      }
      break;
    case 11: {  // FILTER_COMPONENT_TRANSFER (blend.glsl:126-188)
      float ch[4] = {c[0], c[1], c[2], alpha};
      const WrTexDesc& gc = D->tex[WR_S_GPU_CACHE];
      int offset = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int fn = int(F.funcs[i]);
        if (fn == 1 || fn == 2) {           // TABLE / DISCRETE: 256-entry lookup, 4 values per block
          const int k = int(wr_glsl_floor(ch[i] * 255.0f + 0.5f));
          const unsigned a = unsigned(F.table_address + offset + k / 4);
          const wf4 tx = wr_fetch_f(gc, int(a % 1024u), int(a / 1024u));
          const int sel = k % 4;
          const float v = sel == 0 ? tx.x : (sel == 1 ? tx.y : (sel == 2 ? tx.z : (sel == 3 ? tx.w : 0.0f)));
          ch[i] = wr_clamp(v, 0.0f, 1.0f);
          offset += 64;
        } else if (fn == 3) {               // LINEAR
          const unsigned a = unsigned(F.table_address + offset);
          const wf4 tx = wr_fetch_f(gc, int(a % 1024u), int(a / 1024u));
          ch[i] = wr_clamp(tx.x * ch[i] + tx.y, 0.0f, 1.0f);
          offset += 1;
        } else if (fn == 4) {               // GAMMA
          const unsigned a = unsigned(F.table_address + offset);
          const wf4 tx = wr_fetch_f(gc, int(a % 1024u), int(a / 1024u));
          ch[i] = wr_clamp(tx.x * wr_glsl_pow(ch[i], tx.y) + tx.z, 0.0f, 1.0f);
          offset += 1;
        }
      }
      c[0] = ch[0]; c[1] = ch[1]; c[2] = ch[2]; alpha = ch[3];
      break;
    }
    case 10:  // FILTER_FLOOD
      c[0] = F.color_offset[0]; c[1] = F.color_offset[1]; c[2] = F.color_offset[2]; alpha = F.color_offset[3];
      break;
    default: {  // colour-matrix filters: color_mat * vec4(color, alpha) + color_offset (glsl.h:2582-2598 order)
      const float* m = F.color_mat;
      float o4[4];
      for (int i = 0; i < 4; i++)
        o4[i] = wr_clamp((m[i] * c[0] + m[4 + i] * c[1] + m[8 + i] * c[2] + m[12 + i] * alpha) + F.color_offset[i], 0.0f, 1.0f);
      c[0] = o4[0]; c[1] = o4[1]; c[2] = o4[2]; alpha = o4[3];
    }
  }
  // Fragment(alpha * vec4(color, 1.0)) -> pack_pixels_RGBA8
  uint32_t pc[2];
  wr_pack_color(wf4{alpha * c[0], alpha * c[1], alpha * c[2], alpha * 1.0f}, pc);
  WrWide s; s.bg = pc[0]; s.ra = pc[1];
  return s;
}

// ---------------------------------------------------------------------------
// brush_mix_blend fragment shader (brush_mix_blend.glsl:88-330), one pixel.  No span shader in swgl: main() on every chunk;
// per pixel in strict fp32, same operation order.  The GLSL's scalar branches become selects there (every lane computes
// both sides); the selected value is the branch's.
WR_DEVICE void wr_texture_rgba_f(const WrTexDesc& t, float cu, float cv, float (&c)[4]) {      // texture(sampler, uv) -> (r, g, b, a)
  const float W = t.sw, H = t.sh;
  if (!t.ptr) { c[0] = c[1] = c[2] = c[3] = 0.0f; return; }
  if (t.format == WR_FMT_R8) {
    float m;
    if (t.linear) m = float(wr_sample_linear_r8(t, int(cu * W * 128.0f + (0.5f - 64.0f)), int(cv * H * 128.0f + (0.5f - 64.0f)))) * (1.0f / 255.0f);
    else m = float(((const uint8_t*)t.ptr)[(size_t)wr_clamp_coord(int(cu * W), t.width) + (size_t)wr_clamp_coord(int(cv * H), t.height) * t.stride]) * (1.0f / 255.0f);
    c[0] = m; c[1] = 0.0f; c[2] = 0.0f; c[3] = 1.0f;
  } else if (t.linear) {
    const WrWide s = wr_sample_linear_rgba8(t, int(cu * W * 128.0f + (0.5f - 64.0f)), int(cv * H * 128.0f + (0.5f - 64.0f)));
    c[2] = float(s.bg & 0xFFFF) * (1.0f / 255.0f); c[1] = float(s.bg >> 16) * (1.0f / 255.0f);
    c[0] = float(s.ra & 0xFFFF) * (1.0f / 255.0f); c[3] = float(s.ra >> 16) * (1.0f / 255.0f);
  } else {
    const uint32_t p = ((const uint32_t*)t.ptr)[(size_t)wr_clamp_coord(int(cu * W), t.width) + (size_t)wr_clamp_coord(int(cv * H), t.height) * t.stride];
    c[2] = float(p & 0xFF) * (1.0f / 255.0f); c[1] = float((p >> 8) & 0xFF) * (1.0f / 255.0f);
    c[0] = float((p >> 16) & 0xFF) * (1.0f / 255.0f); c[3] = float(p >> 24) * (1.0f / 255.0f);
  }
}
WR_DEVICE float wr_mix_lum(const float (&c)[3]) { return (c[0] * 0.3f + c[1] * 0.59f) + c[2] * 0.11f; }
WR_DEVICE void wr_mix_clip_color(float (&C)[3]) {
  const float L = wr_mix_lum(C);
  const float n = wr_min(C[0], wr_min(C[1], C[2])), x = wr_max(C[0], wr_max(C[1], C[2]));
  if (n < 0.0f) for (int i = 0; i < 3; i++) C[i] = L + (((C[i] - L) * L) / (L - n));
  if (x > 1.0f) for (int i = 0; i < 3; i++) C[i] = L + (((C[i] - L) * (1.0f - L)) / (x - L));
}
WR_DEVICE void wr_mix_set_lum(float (&C)[3], float l) {
  const float d = l - wr_mix_lum(C);
  for (int i = 0; i < 3; i++) C[i] = C[i] + d;
  wr_mix_clip_color(C);
}
WR_DEVICE float wr_mix_sat(const float (&c)[3]) { return wr_max(c[0], wr_max(c[1], c[2])) - wr_min(c[0], wr_min(c[1], c[2])); }
WR_DEVICE void wr_mix_set_sat_inner(float& Cmin, float& Cmid, float& Cmax, float s) {
  if (Cmax > Cmin) { Cmid = ((Cmid - Cmin) * s) / (Cmax - Cmin); Cmax = s; } else { Cmid = 0.0f; Cmax = 0.0f; }
  Cmin = 0.0f;
}
WR_DEVICE void wr_mix_set_sat(float (&C)[3], float s) {
  float& r = C[0]; float& g = C[1]; float& b = C[2];
  if (r <= g) {
    if (g <= b) wr_mix_set_sat_inner(r, g, b, s);
    else if (r <= b) wr_mix_set_sat_inner(r, b, g, s);
    else wr_mix_set_sat_inner(b, r, g, s);
  } else {
    if (r <= b) wr_mix_set_sat_inner(g, r, b, s);
    else if (g <= b) wr_mix_set_sat_inner(g, b, r, s);
    else wr_mix_set_sat_inner(b, g, r, s);
  }
}
WR_DEVICE float wr_mix_hard_light(float Cb, float Cs) {
  const float m = Cb * (2.0f * Cs);
  const float t = 2.0f * Cs - 1.0f;
  const float sc = Cb + t - (Cb * t);
  const float st = Cs < 0.5f ? 0.0f : 1.0f;         // step(edge, Cs)
  return (sc - m) * st + m;                          // mix(m, s, step)
}
__device__ __noinline__ WrWide wr_mix_blend_pixel(const WrPrim* Pp, const WrMixRec* Mp, const WrDrawDesc* D, int x, int y, const WrRuns* runs = nullptr) {
  const WrPrim& P = *Pp;
  const WrMixRec& M = *Mp;
  const WrTexDesc& tb = D->tex[WR_S_COLOR0];
  const WrTexDesc& ts = D->tex[WR_S_COLOR1];
  // v_backdrop_uv / v_src_uv of this pixel as the 4-wide fragment loop steps them, clamped to their sample bounds
  float bu, bv, su, sv;
  {
    const WrTexRow r = wr_tex_row(P, tb, y, runs, x);
    wr_tex_tail_uv(P, r, x - r.x0, bu, bv);
  }
  {
    WrPrim P2 = P;            // the same walk on the second varying's edges
    P2.uvL0[0] = M.sL0[0]; P2.uvL0[1] = M.sL0[1]; P2.uvLs[0] = M.sLs[0]; P2.uvLs[1] = M.sLs[1];
    P2.uvR0[0] = M.sR0[0]; P2.uvR0[1] = M.sR0[1]; P2.uvRs[0] = M.sRs[0]; P2.uvRs[1] = M.sRs[1];
    P2.uv_bounds[0] = M.s_bounds[0]; P2.uv_bounds[1] = M.s_bounds[1]; P2.uv_bounds[2] = M.s_bounds[2]; P2.uv_bounds[3] = M.s_bounds[3];
    P2.rows_linear = 0;
    const WrTexRow r = wr_tex_row(P2, ts, y, runs, x);
    wr_tex_tail_uv(P2, r, x - r.x0, su, sv);
  }
  return wr_mix_blend_main(Mp, D, bu, bv, su, sv);
}
// ... main() of brush_mix_blend with both sample positions in hand (brush_mix_blend.glsl: Cb / Cs unpremultiplied, the sixteen modes)
__device__ __noinline__ WrWide wr_mix_blend_main(const WrMixRec* Mp, const WrDrawDesc* D, float bu, float bv, float su, float sv) {
  const WrMixRec& M = *Mp;
  const WrTexDesc& tb = D->tex[WR_S_COLOR0];
  const WrTexDesc& ts = D->tex[WR_S_COLOR1];
  float Cb4[4], Cs4[4];
  wr_texture_rgba_f(tb, bu, bv, Cb4);
  wr_texture_rgba_f(ts, su, sv, Cs4);
  float Cb[3], Cs[3];
  for (int i = 0; i < 3; i++) { Cb[i] = Cb4[3] != 0.0f ? Cb4[i] / Cb4[3] : Cb4[i]; Cs[i] = Cs4[3] != 0.0f ? Cs4[i] / Cs4[3] : Cs4[i]; }
  float res[3] = {1.0f, 1.0f, 0.0f};
  switch (M.op & 0xFF) {
    case 1: for (int i = 0; i < 3; i++) res[i] = Cb[i] * Cs[i]; break;
    case 3: for (int i = 0; i < 3; i++) res[i] = wr_mix_hard_light(Cs[i], Cb[i]); break;
    case 4: for (int i = 0; i < 3; i++) res[i] = wr_min(Cs[i], Cb[i]); break;
    case 5: for (int i = 0; i < 3; i++) res[i] = wr_max(Cs[i], Cb[i]); break;
    case 6: for (int i = 0; i < 3; i++) res[i] = Cb[i] == 0.0f ? 0.0f : (Cs[i] == 1.0f ? 1.0f : wr_min(1.0f, Cb[i] / (1.0f - Cs[i]))); break;
    case 7: for (int i = 0; i < 3; i++) res[i] = Cb[i] == 1.0f ? 1.0f : (Cs[i] == 0.0f ? 0.0f : 1.0f - wr_min(1.0f, (1.0f - Cb[i]) / Cs[i])); break;
    case 8: for (int i = 0; i < 3; i++) res[i] = wr_mix_hard_light(Cb[i], Cs[i]); break;
    case 9:
      for (int i = 0; i < 3; i++) {
        if (Cs[i] <= 0.5f) res[i] = Cb[i] - (1.0f - 2.0f * Cs[i]) * Cb[i] * (1.0f - Cb[i]);
        else {
          const float Dd = Cb[i] <= 0.25f ? ((16.0f * Cb[i] - 12.0f) * Cb[i] + 4.0f) * Cb[i] : sqrtf(Cb[i]);
          res[i] = Cb[i] + (2.0f * Cs[i] - 1.0f) * (Dd - Cb[i]);
        }
      }
      break;
    case 10: for (int i = 0; i < 3; i++) res[i] = fabsf(Cb[i] - Cs[i]); break;
    case 12: { float c[3] = {Cs[0], Cs[1], Cs[2]}; wr_mix_set_sat(c, wr_mix_sat(Cb)); wr_mix_set_lum(c, wr_mix_lum(Cb)); res[0] = c[0]; res[1] = c[1]; res[2] = c[2]; break; }
    case 13: { float c[3] = {Cb[0], Cb[1], Cb[2]}; wr_mix_set_sat(c, wr_mix_sat(Cs)); wr_mix_set_lum(c, wr_mix_lum(Cb)); res[0] = c[0]; res[1] = c[1]; res[2] = c[2]; break; }
    case 14: { float c[3] = {Cs[0], Cs[1], Cs[2]}; wr_mix_set_lum(c, wr_mix_lum(Cb)); res[0] = c[0]; res[1] = c[1]; res[2] = c[2]; break; }
    case 15: { float c[3] = {Cb[0], Cb[1], Cb[2]}; wr_mix_set_lum(c, wr_mix_lum(Cs)); res[0] = c[0]; res[1] = c[1]; res[2] = c[2]; break; }
    default: break;
  }
  float rgb[3];
  for (int i = 0; i < 3; i++) rgb[i] = ((1.0f - Cb4[3]) * Cs[i] + Cb4[3] * res[i]) * Cs4[3];
  uint32_t pc[2];
  wr_pack_color(wf4{rgb[0], rgb[1], rgb[2], Cs4[3]}, pc);
  WrWide s; s.bg = pc[0]; s.ra = pc[1];
  return s;
}

// ---------------------------------------------------------------------------
// cs_svg_filter (cs_svg_filter.glsl:170-592) and cs_svg_filter_node (cs_svg_filter_node.glsl:397-857) fragment shaders, one
// pixel.  No span shader in swgl: main() on every chunk; per pixel in strict fp32, same operation order (the blend functions are
// brush_mix_blend's, pow() is glsl.h's approximation, the vector floor its int round trip).
WR_DEVICE float wr_svg_color_dodge(float Cb, float Cs) { return Cb == 0.0f ? 0.0f : (Cs == 1.0f ? 1.0f : wr_min(1.0f, Cb / (1.0f - Cs))); }
WR_DEVICE float wr_svg_color_burn(float Cb, float Cs) { return Cb == 1.0f ? 1.0f : (Cs == 0.0f ? 0.0f : 1.0f - wr_min(1.0f, (1.0f - Cb) / Cs)); }
WR_DEVICE float wr_svg_soft_light(float Cb, float Cs) {
  if (Cs <= 0.5f) return Cb - (1.0f - 2.0f * Cs) * Cb * (1.0f - Cb);
  const float Dd = Cb <= 0.25f ? ((16.0f * Cb - 12.0f) * Cb + 4.0f) * Cb : sqrtf(Cb);
  return Cb + (2.0f * Cs - 1.0f) * (Dd - Cb);
}
WR_DEVICE float wr_srgb_to_linear1(float c) { const float c1 = c / 12.92f, c2 = wr_glsl_pow(c / 1.055f + (0.055f / 1.055f), 2.4f); return c <= 0.04045f ? c1 : c2; }
WR_DEVICE float wr_linear_to_srgb1(float c) { const float c1 = c * 12.92f, c2 = 1.055f * wr_glsl_pow(c, 1.0f / 2.4f) - 0.055f; return c <= 0.0031308f ? c1 : c2; }
// the sixteen MixBlendModes on un-premultiplied colours: B(Cb, Cs) of the compositing spec; false: no such mode
WR_DEVICE bool wr_svg_blend_fn(int mode, const float (&Cb)[3], const float (&Cs)[3], float (&res)[3]) {
  switch (mode) {
    case 0: for (int i = 0; i < 3; i++) res[i] = Cs[i]; return true;
    case 1: for (int i = 0; i < 3; i++) res[i] = Cb[i] * Cs[i]; return true;
    case 2: for (int i = 0; i < 3; i++) res[i] = (Cb[i] + Cs[i]) - (Cb[i] * Cs[i]); return true;
    case 3: for (int i = 0; i < 3; i++) res[i] = wr_mix_hard_light(Cs[i], Cb[i]); return true;
    case 4: for (int i = 0; i < 3; i++) res[i] = wr_min(Cs[i], Cb[i]); return true;
    case 5: for (int i = 0; i < 3; i++) res[i] = wr_max(Cs[i], Cb[i]); return true;
    case 6: for (int i = 0; i < 3; i++) res[i] = wr_svg_color_dodge(Cb[i], Cs[i]); return true;
    case 7: for (int i = 0; i < 3; i++) res[i] = wr_svg_color_burn(Cb[i], Cs[i]); return true;
    case 8: for (int i = 0; i < 3; i++) res[i] = wr_mix_hard_light(Cb[i], Cs[i]); return true;
    case 9: for (int i = 0; i < 3; i++) res[i] = wr_svg_soft_light(Cb[i], Cs[i]); return true;
    case 10: for (int i = 0; i < 3; i++) res[i] = fabsf(Cb[i] - Cs[i]); return true;
    case 11: for (int i = 0; i < 3; i++) res[i] = (Cb[i] + Cs[i]) - ((2.0f * Cb[i]) * Cs[i]); return true;
    case 12: { float c[3] = {Cs[0], Cs[1], Cs[2]}; wr_mix_set_sat(c, wr_mix_sat(Cb)); wr_mix_set_lum(c, wr_mix_lum(Cb)); res[0] = c[0]; res[1] = c[1]; res[2] = c[2]; return true; }
    case 13: { float c[3] = {Cb[0], Cb[1], Cb[2]}; wr_mix_set_sat(c, wr_mix_sat(Cs)); wr_mix_set_lum(c, wr_mix_lum(Cb)); res[0] = c[0]; res[1] = c[1]; res[2] = c[2]; return true; }
    case 14: { float c[3] = {Cs[0], Cs[1], Cs[2]}; wr_mix_set_lum(c, wr_mix_lum(Cb)); res[0] = c[0]; res[1] = c[1]; res[2] = c[2]; return true; }
    case 15: { float c[3] = {Cb[0], Cb[1], Cb[2]}; wr_mix_set_lum(c, wr_mix_lum(Cs)); res[0] = c[0]; res[1] = c[1]; res[2] = c[2]; return true; }
    default: return false;
  }
}
// blend(Cs, Cb, mode) of cs_svg_filter.glsl:322-391
WR_DEVICE void wr_svg_blend(const float (&Cs)[4], const float (&Cb)[4], int mode, float (&out)[4]) {
  float res[3] = {1.0f, 0.0f, 0.0f};
  const float cb3[3] = {Cb[0], Cb[1], Cb[2]}, cs3[3] = {Cs[0], Cs[1], Cs[2]};
  wr_svg_blend_fn(mode, cb3, cs3, res);
  for (int i = 0; i < 3; i++) {
    const float rgb = ((1.0f - Cb[3]) * Cs[i]) + (Cb[3] * res[i]);
    const float x = Cb[i] * Cb[3];
    out[i] = (rgb - x) * Cs[3] + x;             // mix(vec4(Cb.rgb * Cb.a, Cb.a), vec4(rgb, 1.0), Cs.a)
  }
  out[3] = (1.0f - Cb[3]) * Cs[3] + Cb[3];
}
__device__ __noinline__ WrWide wr_svg_filter_pixel(const WrPrim* Pp, const WrSvgRec* Sp, const WrDrawDesc* D, int x, int y, const WrRuns* runs = nullptr) {
  const WrPrim& P = *Pp;
  const WrSvgRec& S = *Sp;
  const WrTexDesc& t0 = D->tex[WR_S_COLOR0];
  const WrTexDesc& t1 = D->tex[WR_S_COLOR1];
  // vInput1Uv / vInput2Uv of this pixel as the 4-wide fragment loop steps them
  float u1, v1, u2, v2;
  {
    const WrTexRow r = wr_tex_row(P, t0, y, runs, x);
    wr_tex_tail_uv(P, r, x - r.x0, u1, v1);
  }
  {
    WrPrim P2 = P;            // the same walk on the second varying's edges
    P2.uvL0[0] = S.sL0[0]; P2.uvL0[1] = S.sL0[1]; P2.uvLs[0] = S.sLs[0]; P2.uvLs[1] = S.sLs[1];
    P2.uvR0[0] = S.sR0[0]; P2.uvR0[1] = S.sR0[1]; P2.uvRs[0] = S.sRs[0]; P2.uvRs[1] = S.sRs[1];
    P2.rows_linear = 0;
    const WrTexRow r = wr_tex_row(P2, t1, y, runs, x);
    wr_tex_tail_uv(P2, r, x - r.x0, u2, v2);
  }
  float A[4] = {0.f, 0.f, 0.f, 0.f}, B[4] = {0.f, 0.f, 0.f, 0.f};       // sampleInUvRect of the two inputs
  if (S.input_count > 0) wr_texture_rgba_f(t0, wr_clamp(u1, S.rect1[0], S.rect1[2]), wr_clamp(v1, S.rect1[1], S.rect1[3]), A);
  if (S.input_count > 1) wr_texture_rgba_f(t1, wr_clamp(u2, S.rect2[0], S.rect2[2]), wr_clamp(v2, S.rect2[1], S.rect2[3]), B);
  float res[4] = {1.0f, 0.0f, 0.0f, 1.0f};
  const WrTexDesc& gc = D->tex[WR_S_GPU_CACHE];
  if (!S.node) {
    // cs_svg_filter: un-premultiplied inputs
    if (S.input_count > 0 && A[3] != 0.0f) for (int i = 0; i < 3; i++) A[i] = A[i] / A[3];
    if (S.input_count > 1 && B[3] != 0.0f) for (int i = 0; i < 3; i++) B[i] = B[i] / B[3];
    bool premul = true;
    switch (S.kind) {
      case 0: wr_svg_blend(A, B, S.data[0], res); premul = false; break;
      case 1: for (int i = 0; i < 4; i++) res[i] = S.fdata0[i]; premul = false; break;
      case 2: for (int i = 0; i < 3; i++) res[i] = wr_linear_to_srgb1(A[i]); res[3] = A[3]; break;
      case 3: for (int i = 0; i < 3; i++) res[i] = wr_srgb_to_linear1(A[i]); res[3] = A[3]; break;
      case 4: for (int i = 0; i < 3; i++) res[i] = A[i]; res[3] = A[3] * S.float0; break;
      case 5: {
        const float* m = S.color_mat;
        for (int i = 0; i < 4; i++) res[i] = wr_clamp((m[i] * A[0] + m[4 + i] * A[1] + m[8 + i] * A[2] + m[12 + i] * A[3]) + S.fdata0[i], 0.0f, 1.0f);
        break;
      }
      case 6: {
        const float shadow[4] = {S.fdata0[0], S.fdata0[1], S.fdata0[2], B[3] * S.fdata0[3]};
        wr_svg_blend(A, shadow, 0, res); premul = false;
        break;
      }
      case 7: {
        const float ou = u1 + S.fdata0[0], ov = v1 + S.fdata0[1];
        wr_texture_rgba_f(t0, wr_clamp(ou, S.rect1[0], S.rect1[2]), wr_clamp(ov, S.rect1[1], S.rect1[3]), res);
        // point_inside_rect: (step(p0, p) - step(p1, p)).x * .y
        const float sx = wr_step01(S.fdata1[0], ou) - wr_step01(S.fdata1[2], ou), sy = wr_step01(S.fdata1[1], ov) - wr_step01(S.fdata1[3], ov);
        const float in = sx * sy;
        for (int i = 0; i < 4; i++) res[i] = res[i] * in;
        premul = false;
        break;
      }
      case 8: {             // ComponentTransfer (cs_svg_filter.glsl:415-466)
        float ch[4] = {A[0], A[1], A[2], A[3]};
        int offset = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int fn = S.funcs[i];
          if (fn == 1 || fn == 2) {
            const int k = int(wr_glsl_floor(ch[i] * 255.0f + 0.5f));
            const wf4 tx = wr_fetch_f(gc, S.data[0] + (offset + k / 4), S.data[1]);
            const int sel = k % 4;
            const float v = sel == 0 ? tx.x : (sel == 1 ? tx.y : (sel == 2 ? tx.z : (sel == 3 ? tx.w : 0.0f)));
            ch[i] = wr_clamp(v, 0.0f, 1.0f);
            offset += 64;
          } else if (fn == 3) {
            const wf4 tx = wr_fetch_f(gc, S.data[0] + offset, S.data[1]);
            ch[i] = wr_clamp(tx.x * ch[i] + tx.y, 0.0f, 1.0f);
            offset += 1;
          } else if (fn == 4) {
            const wf4 tx = wr_fetch_f(gc, S.data[0] + offset, S.data[1]);
            ch[i] = wr_clamp(tx.x * wr_glsl_pow(ch[i], tx.y) + tx.z, 0.0f, 1.0f);
            offset += 1;
          }
        }
        for (int i = 0; i < 4; i++) res[i] = ch[i];
        break;
      }
      case 9: for (int i = 0; i < 4; i++) res[i] = A[i]; break;
      case 10: {            // composite(Cs = Ca, Cb, mode) (cs_svg_filter.glsl:470-507)
        const float* Cs = A; const float* Cb = B;
        float Cr[4] = {0.0f, 1.0f, 0.0f, 1.0f};
        switch (S.data[0]) {
          case 0: for (int i = 0; i < 3; i++) Cr[i] = (Cs[3] * Cs[i]) + ((Cb[3] * Cb[i]) * (1.0f - Cs[3])); Cr[3] = Cs[3] + (Cb[3] * (1.0f - Cs[3])); break;
          case 1: for (int i = 0; i < 3; i++) Cr[i] = (Cs[3] * Cs[i]) * Cb[3]; Cr[3] = Cs[3] * Cb[3]; break;
          case 2: for (int i = 0; i < 3; i++) Cr[i] = (Cs[3] * Cs[i]) * (1.0f - Cb[3]); Cr[3] = Cs[3] * (1.0f - Cb[3]); break;
          case 3: for (int i = 0; i < 3; i++) Cr[i] = ((Cs[3] * Cs[i]) * Cb[3]) + ((Cb[3] * Cb[i]) * (1.0f - Cs[3])); Cr[3] = (Cs[3] * Cb[3]) + (Cb[3] * (1.0f - Cs[3])); break;
          case 4: for (int i = 0; i < 3; i++) Cr[i] = ((Cs[3] * Cs[i]) * (1.0f - Cb[3])) + ((Cb[3] * Cb[i]) * (1.0f - Cs[3])); Cr[3] = (Cs[3] * (1.0f - Cb[3])) + (Cb[3] * (1.0f - Cs[3])); break;
          case 5: for (int i = 0; i < 3; i++) Cr[i] = (Cs[3] * Cs[i]) + (Cb[3] * Cb[i]); Cr[3] = Cs[3] + Cb[3]; for (int i = 0; i < 4; i++) Cr[i] = wr_clamp(Cr[i], 0.0f, 1.0f); break;
          case 6: for (int i = 0; i < 4; i++) Cr[i] = wr_clamp((((S.fdata0[0] * Cs[i]) * Cb[i]) + (S.fdata0[1] * Cs[i])) + (S.fdata0[2] * Cb[i]) + S.fdata0[3], 0.0f, 1.0f); break;
          default: break;
        }
        for (int i = 0; i < 4; i++) res[i] = Cr[i];
        premul = false;
        break;
      }
      default: break;
    }
    if (premul) for (int i = 0; i < 3; i++) res[i] = res[i] * res[3];
  } else {
    // cs_svg_filter_node: raw premultiplied colours Rs / Rb (A / B), normalised Ns / Nb; odd kinds work in linear light
    float* Rs = A; float* Rb = B;
    float Ns[4] = {0.f, 0.f, 0.f, 0.f}, Nb[4] = {0.f, 0.f, 0.f, 0.f};
    const bool lin = (S.kind & 1) != 0;
    if (S.input_count > 0) {
      const float ia = 1.0f / wr_max(0.000001f, Rs[3]);
      for (int i = 0; i < 3; i++) Ns[i] = Rs[i] * ia;
      Ns[3] = Rs[3];
      if (lin) for (int i = 0; i < 3; i++) { Ns[i] = wr_srgb_to_linear1(Ns[i]); Rs[i] = Ns[i] * Rs[3]; }
    }
    if (S.input_count > 1) {
      const float ia = 1.0f / wr_max(0.000001f, Rb[3]);
      for (int i = 0; i < 3; i++) Nb[i] = Rb[i] * ia;
      Nb[3] = Rb[3];
      if (lin) for (int i = 0; i < 3; i++) { Nb[i] = wr_srgb_to_linear1(Nb[i]); Rb[i] = Nb[i] * Rb[3]; }
    }
    const int k2 = S.kind >> 1;
    bool done = false;
    if (k2 == 0) { for (int i = 0; i < 4; i++) res[i] = Rs[i]; }                             // IDENTITY
    else if (k2 == 1) { for (int i = 0; i < 4; i++) res[i] = Rs[i] * S.float0; }             // OPACITY
    else if (k2 == 2) { res[0] = res[1] = res[2] = 0.0f; res[3] = Rs[3]; done = true; }      // TO_ALPHA: returns before the sRGB step
    else if (k2 >= 3 && k2 <= 18) {                                                          // FILTER_BLEND_* in the shader's alphabetical order
      // kind / 2 -> MixBlendMode of wr_svg_blend_fn; -1: the closed forms on premultiplied colours below
      const int modes[16] = {14, 7, 6, -4, -10, -11, 8, 12, -5, 15, -1, -100, 3, 13, -2, 9};
      const int mode = modes[k2 - 3];
      const float ra = (Rb[3] * (1.0f - Rs[3])) + Rs[3];
      if (mode >= 0) {
        const float nb3[3] = {Nb[0], Nb[1], Nb[2]}, ns3[3] = {Ns[0], Ns[1], Ns[2]};
        float r3[3] = {1.0f, 0.0f, 0.0f};
        wr_svg_blend_fn(mode, nb3, ns3, r3);
        for (int i = 0; i < 3; i++) res[i] = (((1.0f - Rb[3]) * Rs[i]) + ((1.0f - Rs[3]) * Rb[i])) + ((Rs[3] * Rb[3]) * r3[i]);
        res[3] = ra;
      } else if (mode == -4) { for (int i = 0; i < 3; i++) res[i] = (Rs[i] + Rb[i]) - wr_max(Rs[i] * Rb[3], Rb[i] * Rs[3]); res[3] = ra; }                 // DARKEN
      else if (mode == -10) { for (int i = 0; i < 3; i++) res[i] = (Rs[i] + Rb[i]) - (2.0f * wr_min(Rs[i] * Rb[3], Rb[i] * Rs[3])); res[3] = ra; }         // DIFFERENCE
      else if (mode == -11) { for (int i = 0; i < 3; i++) res[i] = (Rs[i] + Rb[i]) - (2.0f * (Rs[i] * Rb[i])); res[3] = ra; }                               // EXCLUSION
      else if (mode == -5) { for (int i = 0; i < 3; i++) res[i] = (Rs[i] + Rb[i]) - wr_min(Rs[i] * Rb[3], Rb[i] * Rs[3]); res[3] = ra; }                  // LIGHTEN
      else if (mode == -1) { for (int i = 0; i < 3; i++) res[i] = ((Rs[i] * (1.0f - Rb[3])) + (Rb[i] * (1.0f - Rs[3]))) + (Rs[i] * Rb[i]); res[3] = ra; }  // MULTIPLY
      else if (mode == -100) { for (int i = 0; i < 4; i++) res[i] = (Rb[i] * (1.0f - Rs[3])) + Rs[i]; }                                                    // NORMAL
      else { for (int i = 0; i < 3; i++) res[i] = (Rs[i] + Rb[i]) - (Rs[i] * Rb[i]); res[3] = ra; }                                                         // SCREEN
    } else if (k2 == 19) {                                                                   // COLOR_MATRIX
      const float* m = S.color_mat;
      for (int i = 0; i < 4; i++) res[i] = wr_clamp((m[i] * Ns[0] + m[4 + i] * Ns[1] + m[8 + i] * Ns[2] + m[12 + i] * Ns[3]) + S.fdata0[i], 0.0f, 1.0f);
      for (int i = 0; i < 3; i++) res[i] = res[i] * res[3];
    } else if (k2 == 20) {                                                                   // COMPONENT_TRANSFER: a [256] table of RGBA blocks
      int k[4];
      for (int i = 0; i < 4; i++) k[i] = int(wr_glsl_floor(wr_clamp(Ns[i] * 255.0f, 0.0f, 255.0f)));
      res[0] = wr_fetch_f(gc, S.data[0] + k[0], S.data[1]).x; res[1] = wr_fetch_f(gc, S.data[0] + k[1], S.data[1]).y;
      res[2] = wr_fetch_f(gc, S.data[0] + k[2], S.data[1]).z; res[3] = wr_fetch_f(gc, S.data[0] + k[3], S.data[1]).w;
      for (int i = 0; i < 3; i++) res[i] = res[i] * res[3];
    } else if (k2 == 21) { for (int i = 0; i < 4; i++) res[i] = wr_clamp(((((Rs[i] * Rb[i]) * S.fdata0[0]) + (Rs[i] * S.fdata0[1])) + (Rb[i] * S.fdata0[2])) + S.fdata0[3], 0.0f, 1.0f); }    // ARITHMETIC
    else if (k2 == 22) { for (int i = 0; i < 4; i++) res[i] = (Rs[i] * Rb[3]) + (Rb[i] * (1.0f - Rs[3])); }                       // ATOP
    else if (k2 == 23) { for (int i = 0; i < 4; i++) res[i] = Rs[i] * Rb[3]; }                                                   // IN
    else if (k2 == 24) { for (int i = 0; i < 4; i++) res[i] = wr_clamp(Rs[i] + Rb[i], 0.0f, 1.0f); }                             // LIGHTER
    else if (k2 == 25) { for (int i = 0; i < 4; i++) res[i] = Rs[i] * (1.0f - Rb[3]); }                                          // OUT
    else if (k2 == 26) { for (int i = 0; i < 4; i++) res[i] = Rs[i] + (Rb[i] * (1.0f - Rs[3])); }                                // OVER
    else if (k2 == 27) { for (int i = 0; i < 4; i++) res[i] = (Rs[i] * (1.0f - Rb[3])) + (Rb[i] * (1.0f - Rs[3])); }             // XOR
    else if (k2 == 35) { for (int i = 0; i < 4; i++) res[i] = Rs[i] + (S.fdata0[i] * (Rb[3] * (1.0f - Rs[3]))); }                // DROP_SHADOW
    else if (k2 == 36) { for (int i = 0; i < 4; i++) res[i] = S.fdata0[i]; }                                                     // FLOOD
    else if (k2 == 46) {                                                                     // TILE: rect_repeat(vInput1Uv, rect.xy, rect.zw), returns before the sRGB step
      // rect_repeat (rect.glsl): p0 + s * fract(is * r), r = p - p0, s = p1 - p0, is = 1 / max(s, 0.000001)
      const float sx = S.rect1[2] - S.rect1[0], sy = S.rect1[3] - S.rect1[1];
      const float isx = 1.0f / wr_max(sx, 0.000001f), isy = 1.0f / wr_max(sy, 0.000001f);
      const float rx = isx * (u1 - S.rect1[0]), ry = isy * (v1 - S.rect1[1]);
      const float tu = S.rect1[0] + sx * (rx - wr_glsl_floor(rx)), tv = S.rect1[1] + sy * (ry - wr_glsl_floor(ry));
      wr_texture_rgba_f(t0, wr_clamp(tu, S.rect1[0], S.rect1[2]), wr_clamp(tv, S.rect1[1], S.rect1[3]), res);
      done = true;
    }
    // (every other kind -- convolve, lighting, displacement, gaussian blur, image, morphology, turbulence -- has no case in the
    // reference's main(): the start colour (1, 0, 0, 1) goes through the sRGB step)
    if (!done && lin) {
      const float ia = 1.0f / wr_max(0.000001f, res[3]);
      for (int i = 0; i < 3; i++) res[i] = wr_linear_to_srgb1(res[i] * ia) * res[3];
    }
  }
  uint32_t pc[2];
  wr_pack_color(wf4{res[0], res[1], res[2], res[3]}, pc);
  WrWide w; w.bg = pc[0]; w.ra = pc[1];
  return w;
}

// ---------------------------------------------------------------------------
// brush_yuv_image: one pixel.  Span part: swgl_commitTextureLinearYUV (swgl_ext.h:1028-1340) -- every plane sampled with
// the quantised fallback stepping (LINEAR_QUANTIZE_UV, uv += uv_step per chunk, clamp, 7-bit bilinear), the samples put
// through the fixed-point matrix (YUVMatrix::convert, composite.h:722-768: 16-bit lanes, saturating adds).  Tail: main() ->
// sample_yuv (yuv.glsl:187-237) in float.
WR_DEVICE int wr_sat16(int v) { return v > 32767 ? 32767 : (v < -32768 ? -32768 : v); }
WR_DEVICE int wr_wrap16(int v) { return (int)(int16_t)v; }
// An interleaved 4:2:2 texture (YUY2, GL_RGB_RAW_422_APPLE): two-pixel chunks of four bytes, Y0 Cb Y1 Cr; offsets and the stride count
// 16-bit units (one per pixel), a chunk starts on an even one.
struct WrYuv3 { int y, u, v; };
struct WrYuy2Pair { uint32_t c0, c1; };      // two adjacent chunks of one row: g0 b g1 r | G0 B G1 R (4-byte aligned, one 8-byte load)
// textureLinearPlanarYUY2 (texture.h:877-949) for ONE pixel, (qx, qy) the quantised coordinate (x 128) after the LINEAR_QUANTIZE_UV
// clamp: the row pair blended first, then the columns, a + (((b - a) * f) >> 7) in 16-bit lanes.  Luma goes g0 -> g1 or g1 -> G0 by
// the pixel's place in its chunk (the selector), chroma (b, r) -> (B, R) of the next chunk with half the luma's fraction.
// The reads stay inside the texture: computeRow's margin of 2 clamps the column to width - 3, the chunk it lies in starts at most at
// column width - 4 (wr_yuv_planes_ok: the width is even and >= 4), so the 8 bytes end with the row; the stride is 2 * width bytes (even
// in 16-bit units, the selector is the column's parity), the second row is row + 1 only while row < height - 1 -- on the last chunk
// of the last row both loads end on the allocation's last byte, and nothing reads past them.
__device__ __noinline__ WrYuv3 wr_yuy2_linear(const WrTexDesc* tp, int qx, int qy) {
  const WrTexDesc& t = *tp;
  const int ix = qx >> 7, iy = qy >> 7;
  const size_t row = (size_t)wr_clamp_coord(ix, t.width - 2) + (size_t)wr_clamp_coord(iy, t.height) * t.stride;      // computeRow(sampler, i, 2)
  const int sel = int(row & 1);
  const size_t row0 = row & ~size_t(1), row1 = row0 + ((iy >= 0 && iy < t.height - 1) ? t.stride : 0);
  const int fx = ix >= 0 ? qx : 0;                      // frac.x &= (i.x >= 0)
  const int over = ix > t.width - 3 ? -1 : 0;           // both fractions saturate where the next chunk would lie outside
  const int fracl = (fx | over) & 0x7F, fracc = ((fx >> 1) | over) & 0x7F, fracy = qy & 0x7F;
  const uint16_t* buf = (const uint16_t*)t.ptr;
  const WrYuy2Pair a = *(const WrYuy2Pair*)(buf + row0), b = *(const WrYuy2Pair*)(buf + row1);
  auto rows = [&](uint32_t wa, uint32_t wb, int k) -> int {
    const int p = int((wa >> (8 * k)) & 0xFF), q = int((wb >> (8 * k)) & 0xFF);
    return wr_wrap16(p + wr_wrap16(wr_wrap16((q - p) * fracy) >> 7));
  };
  auto cols = [](int p, int q, int f) -> int { return wr_wrap16(p + wr_wrap16(wr_wrap16((q - p) * f) >> 7)); };
  const int g1 = rows(a.c0, b.c0, 2);
  WrYuv3 s;
  s.y = sel ? cols(g1, rows(a.c1, b.c1, 0), fracl) : cols(rows(a.c0, b.c0, 0), g1, fracl);
  s.u = cols(rows(a.c0, b.c0, 1), rows(a.c1, b.c1, 1), fracc);
  s.v = cols(rows(a.c0, b.c0, 3), rows(a.c1, b.c1, 3), fracc);
  return s;
}
// texelFetchYUY2 (texture.h:192-214): texel (x, y), clamped by the caller -- the chunk it lies in, luma by the selector
WR_DEVICE WrYuv3 wr_yuy2_fetch(const WrTexDesc& t, int x, int y) {
  const size_t off = (size_t)x + (size_t)y * t.stride;
  const uint32_t c = *(const uint32_t*)((const uint16_t*)t.ptr + (off & ~size_t(1)));
  WrYuv3 s;
  s.y = int(((off & 1) ? c >> 16 : c) & 0xFF); s.u = int((c >> 8) & 0xFF); s.v = int(c >> 24);
  return s;
}
WR_DEVICE WrWide wr_yuv_convert(const WrYuvRec& Y, int y, int u, int v) {
  // yy = (u16(y) * yCoeffs) >> 1 (16-bit wrap), - yBias; uv - uvBias; br = addsat(yy & mask, coeff * uv) >> 6;
  // gg = addsat(yy, addsat(gu * u, gv * v)) >> 6; pack with unsigned saturation, alpha 255
  int yy = wr_wrap16(int((uint32_t(uint16_t(y)) * uint32_t(uint16_t(Y.ycoeff))) & 0xFFFFu) >> 1);
  yy = wr_wrap16(yy - Y.ybias);
  const int uu = wr_wrap16(u - Y.uvbias), vv = wr_wrap16(v - Y.uvbias);
  const int b = wr_sat16((yy & Y.brmask) + wr_wrap16(Y.bu * uu)) >> 6, r = wr_sat16((yy & Y.brmask) + wr_wrap16(Y.rv * vv)) >> 6;
  const int g = wr_sat16(yy + wr_sat16(wr_wrap16(Y.gu * uu) + wr_wrap16(Y.gv * vv))) >> 6;
  auto pk = [](int c) { return uint32_t(c < 0 ? 0 : (c > 255 ? 255 : c)); };
  WrWide s;
  s.bg = pk(b) | (pk(g) << 16); s.ra = pk(r) | (255u << 16);
  return s;
}
// linear_row_yuv's row-invariant integers (composite.h:999-1011, 1081-1122): the first chunk's 8.8 coordinates per lane, the steps per
// chunk, the chunk range that takes upscaleYUV42R8 and its averaged chroma coordinates at that range's start
struct WrYuvRowArgs { int yU[4], cU[4], yDU, cDU, fast0, fast1, cA, cB, color_depth; };
WR_DEVICE void wr_yuv_row_chunk(const WrTexDesc& Ty, const WrTexDesc& Tu, const WrTexDesc& Tv, const WrYuvRowArgs& R, int yV, int cV, int c,
                                int (&ys)[4], int (&us)[4], int (&vs)[4]);
// linear_row_yuv's setup for a run of `span` pixels from (su, du) on the luma plane and (cu, cdu) on the chroma planes, 1/128 texels
// (the device-side twin of what CompositeYUV's host code computes once per call)
WR_DEVICE void wr_yuv_row_setup(WrYuvRowArgs& R, const WrTexDesc& Ty, const WrTexDesc& Tu, float su, float du, float cu, float cdu, int span) {
  const int STEP_BITS = 8;
  const float yl1 = su + du, yl2 = yl1 + du, yl3 = yl2 + du, cl1 = cu + cdu, cl2 = cl1 + cdu, cl3 = cl2 + cdu;      // init_interp
  R.yU[0] = int(su * float(1 << STEP_BITS)); R.yU[1] = int(yl1 * float(1 << STEP_BITS)); R.yU[2] = int(yl2 * float(1 << STEP_BITS)); R.yU[3] = int(yl3 * float(1 << STEP_BITS));
  R.cU[0] = int(cu * float(1 << STEP_BITS)); R.cU[1] = int(cl1 * float(1 << STEP_BITS)); R.cU[2] = int(cl2 * float(1 << STEP_BITS)); R.cU[3] = int(cl3 * float(1 << STEP_BITS));
  R.yDU = int(float(4 << STEP_BITS) * du); R.cDU = int(float(4 << STEP_BITS) * cdu);
  R.fast0 = R.fast1 = 0; R.cA = R.cB = 0;
  if (Ty.format != WR_FMT_R16 && R.yDU >= R.cDU && R.cDU > 0 && R.yDU <= (4 << (STEP_BITS + 7)) && R.cDU <= (2 << (STEP_BITS + 7))) {
    // the half-resolution fast path (composite.h:1081-1122): chunks until both coordinates are positive, then as many whole chunks
    // as stay four texels inside both planes
    int left = span, chunk = 0;
    int yx = R.yU[0], cx = R.cU[0];
    int cl[4] = {R.cU[0], R.cU[1], R.cU[2], R.cU[3]};
    for (; (yx < 0 || cx < 0) && left >= 4; left -= 4) {
      yx = int(uint32_t(yx) + uint32_t(R.yDU)); cx = int(uint32_t(cx) + uint32_t(R.cDU));
      for (int i = 0; i < 4; i++) cl[i] = int(uint32_t(cl[i]) + uint32_t(R.cDU));
      chunk++;
    }
    const int inside = wr_imin(wr_imin((((Ty.width - 4) << (STEP_BITS + 7)) - yx) / R.yDU, (((Tu.width - 4) << (STEP_BITS + 7)) - cx) / R.cDU) * 4, left & ~3);
    if (inside > 0) {
      R.fast0 = chunk; R.fast1 = chunk + inside / 4;
      R.cA = (cl[0] + cl[1]) >> 1; R.cB = (cl[2] + cl[3]) >> 1;      // cU = (cU.xzxz + cU.ywyw) >> 1
    }
  }
}

// The prim as chroma plane `pl` (1: vUv_U, 2: vUv_V) sees it: that plane's edge interpolants and bounds.  `row`: the prim is one row of a
// general quad (wr_quad_tex_pixel_rgba8), and these are the planes' edge values on it -- vUv_U left (u, v), right (u, v), then vUv_V
WR_DEVICE void wr_yuv_chroma_prim(WrPrim& P2, const WrYuvRec& Y, int pl, const float* row) {
  const float* Bd = pl == 1 ? Y.u_bounds : Y.v_bounds;
  if (row) {
    const float* e = row + 4 * (pl - 1);
    P2.uvL0[0] = e[0]; P2.uvL0[1] = e[1]; P2.uvR0[0] = e[2]; P2.uvR0[1] = e[3];
    P2.uvLs[0] = P2.uvLs[1] = P2.uvRs[0] = P2.uvRs[1] = 0.0f;
  } else {
    const float* L0 = pl == 1 ? Y.uL0 : Y.vL0; const float* Ls = pl == 1 ? Y.uLs : Y.vLs;
    const float* R0 = pl == 1 ? Y.uR0 : Y.vR0; const float* Rs = pl == 1 ? Y.uRs : Y.vRs;
    P2.uvL0[0] = L0[0]; P2.uvL0[1] = L0[1]; P2.uvLs[0] = Ls[0]; P2.uvLs[1] = Ls[1];
    P2.uvR0[0] = R0[0]; P2.uvR0[1] = R0[1]; P2.uvRs[0] = Rs[0]; P2.uvRs[1] = Rs[1];
  }
  P2.uv_bounds[0] = Bd[0]; P2.uv_bounds[1] = Bd[1]; P2.uv_bounds[2] = Bd[2]; P2.uv_bounds[3] = Bd[3];
  P2.rows_linear = 0;
}

// The span pixels of a PLANAR frame under a TEXTURE_RECT key: three linear sampler2DRect planes select blendYUV's second overload
// (swgl_ext.h:1195-1283).  When the planes agree (one format, chroma planes of one size sampled at the same coordinates, no change of
// row along the span, x increasing) the span is cut in three: chunks before both clamp rects are entered take the quantised float
// stepping (blendYUVFallback), the chunks inside them CompositeYUV's inner loop (linear_row_yuv from the coordinates reached by
// ONE multiply-add), the rest the float stepping again from where that run ended.  Returns false where the shared routine's value is
// the reference's (conditions not met, or the pixel lies in the first part).
WR_DEVICE bool wr_yuv_rect_span_pixel(const WrPrim* Pp, const WrYuvRec& Y, const WrDrawDesc* D, int x, int y, const WrRuns* runs, WrWide& out,
                                      const float* row) {
  const WrTexDesc& T0 = D->tex[WR_S_COLOR0]; const WrTexDesc& T1 = D->tex[WR_S_COLOR1]; const WrTexDesc& T2 = D->tex[WR_S_COLOR2];
  if (!(T0.format == T1.format && T1.format == T2.format && T1.width == T2.width && T1.height == T2.height)) return false;
  float q[3][4], qy[3][4], stepx[3], stepy[3], minx[3], maxx[3], miny[3], maxy[3];
  int n = 0, span = 0;
  for (int pl = 0; pl < 3; pl++) {
    WrPrim P2 = *Pp;
    P2.kind = WR_PK_TEX_R8;
    if (pl > 0) wr_yuv_chroma_prim(P2, Y, pl, row);
    const WrTexDesc& t = D->tex[WR_S_COLOR0 + pl];
    const WrTexRow r = wr_tex_row(P2, t, y, runs, x, false);
    if (pl == 0) { n = x - r.x0; span = r.span; if (n >= span) return false; }
    const float W = t.sw, H = t.sh, qs = 128.0f, qo = 0.5f - 0.5f * qs;
    for (int i = 0; i < 4; i++) { q[pl][i] = r.lu[i] * W * qs + qo; qy[pl][i] = r.lv[i] * H * qs + qo; }
    stepx[pl] = 4.0f * (q[pl][1] - q[pl][0]); stepy[pl] = 4.0f * (qy[pl][1] - qy[pl][0]);
    minx[pl] = wr_max(P2.uv_bounds[0] * W * qs + qo, 0.0f); miny[pl] = wr_max(P2.uv_bounds[1] * H * qs + qo, 0.0f);
    maxx[pl] = wr_max(P2.uv_bounds[2] * W * qs + qo, minx[pl]); maxy[pl] = wr_max(P2.uv_bounds[3] * H * qs + qo, miny[pl]);
  }
  if (!(stepy[0] == 0.0f && stepx[0] > 0.0f && stepy[1] == 0.0f && stepx[1] > 0.0f && stepx[1] == stepx[2] && stepy[1] == stepy[2] &&
        q[1][0] == q[2][0] && qy[1][0] == qy[2][0])) return false;
  const int chunks = span >> 2, c = n >> 2, k = n & 3;
  int outside = wr_imin(int(ceilf(wr_max((minx[0] - q[0][0]) / stepx[0], (minx[1] - q[1][0]) / stepx[1]))), chunks);
  if (outside < 0) outside = 0;
  if (c < outside) return false;
  float u0[4], u1[4], u2[4];
  for (int i = 0; i < 4; i++) { u0[i] = q[0][i]; u1[i] = q[1][i]; u2[i] = q[2][i]; }
  if (outside > 0) for (int i = 0; i < 4; i++) { u0[i] += float(outside) * stepx[0]; u1[i] += float(outside) * stepx[1]; u2[i] += float(outside) * stepx[2]; }
  int inside = wr_imin(int(wr_min((maxx[0] - u0[0]) / stepx[0], (maxx[1] - u1[0]) / stepx[1])), chunks - outside);
  if (inside < 0) inside = 0;
  int s3[3];
  if (c < outside + inside) {
    WrYuvRowArgs R;
    R.color_depth = (T0.format == WR_FMT_R16 ? 16 : 8) - Y.rescale;
    wr_yuv_row_setup(R, T0, T1, u0[0], stepx[0] / 4.0f, u1[0], stepx[1] / 4.0f, inside * 4);
    int ys[4], us[4], vs[4];
    wr_yuv_row_chunk(T0, T1, T2, R, int(qy[0][0]), int(qy[1][0]), c - outside, ys, us, vs);
    s3[0] = wr_pick4i(ys, k); s3[1] = wr_pick4i(us, k); s3[2] = wr_pick4i(vs, k);
  } else {
    // what is left of the span: the float stepping again, from the coordinates the inside run ended on
    if (inside > 0) for (int i = 0; i < 4; i++) { u0[i] += float(inside) * stepx[0]; u1[i] += float(inside) * stepx[1]; u2[i] += float(inside) * stepx[2]; }
    const int cc = c - outside - inside;
    const float us3[3] = {wr_pick4(u0, k), wr_pick4(u1, k), wr_pick4(u2, k)};
    for (int pl = 0; pl < 3; pl++) {
      const WrTexDesc& t = D->tex[WR_S_COLOR0 + pl];
      const int iqx = int(wr_clamp(wr_accum(us3[pl], stepx[pl], cc), minx[pl], maxx[pl]));
      const int iqy = int(wr_clamp(wr_accum(wr_pick4(qy[pl], k), stepy[pl], cc), miny[pl], maxy[pl]));
      int v4[4];
      if (t.format == WR_FMT_R16) { wr_bilinear16<1>(t, iqx, iqy, v4); s3[pl] = v4[0] >> ((16 - Y.rescale - 1) - 8); }
      else { wr_bilinear<1>(t, iqx, iqy, v4); s3[pl] = v4[0]; }
    }
  }
  out = wr_yuv_convert(Y, s3[0], s3[1], s3[2]);
  return true;
}

// main()'s sample of one plane (sample_yuv: TEX_SAMPLE of the clamped uv) as floats in fs[pl] (RG planes: fs[1], fs[2]; the one
// interleaved plane: all three)
WR_DEVICE void wr_yuv_main_sample(const WrTexDesc& t, int pl, float cu, float cv, float (&fs)[3]) {
  const float W = t.sw, H = t.sh;
  if (t.format == WR_FMT_YUY2) {      // texture(sColor0, uv).gbr: textureLinearYUY2 (texture.h:951-959) / texelFetchYUY2, (y, cb, cr) * (1 / 255)
    const WrYuv3 s = t.linear ? wr_yuy2_linear(&t, int(cu * W * 128.0f + (0.5f - 64.0f)), int(cv * H * 128.0f + (0.5f - 64.0f)))
                              : wr_yuy2_fetch(t, wr_clamp_coord(int(cu * W), t.width), wr_clamp_coord(int(cv * H), t.height));
    fs[0] = float(s.y) * (1.0f / 255.0f); fs[1] = float(s.u) * (1.0f / 255.0f); fs[2] = float(s.v) * (1.0f / 255.0f);
  } else if (t.format == WR_FMT_R16 || t.format == WR_FMT_RG16) {      // textureLinearR16 / RG16: sample * (1 / 32767)
    int v4[4] = {0, 0, 0, 0};
    const int iqx = int(cu * W * 128.0f + (0.5f - 64.0f)), iqy = int(cv * H * 128.0f + (0.5f - 64.0f));
    if (t.format == WR_FMT_RG16) { wr_bilinear16<2>(t, iqx, iqy, v4); fs[1] = float(v4[0]) * (1.0f / 32767.0f); fs[2] = float(v4[1]) * (1.0f / 32767.0f); }
    else { wr_bilinear16<1>(t, iqx, iqy, v4); fs[pl] = float(v4[0]) * (1.0f / 32767.0f); }
  } else if (t.format == WR_FMT_RG8) {
    int v4[4] = {0, 0, 0, 0};
    if (t.linear) wr_bilinear<2>(t, int(cu * W * 128.0f + (0.5f - 64.0f)), int(cv * H * 128.0f + (0.5f - 64.0f)), v4);
    else wr_fetch_texel<2>(t, (size_t)wr_clamp_coord(int(cu * W), t.width) + (size_t)wr_clamp_coord(int(cv * H), t.height) * t.stride, v4);
    fs[1] = float(v4[0]) * (1.0f / 255.0f); fs[2] = float(v4[1]) * (1.0f / 255.0f);
  } else {
    fs[pl] = wr_r8_texture(t, cu, cv);
  }
}
// ... and the rest of main(): rgb = vRgbFromDebiasedYcbcr * (ycbcr_sample - vYcbcrBias); ALPHA_PASS: clamp to [0, 1]; alpha 1
WR_DEVICE WrWide wr_yuv_main_rgb(const WrYuvRec& Y, const float (&fs)[3], bool clamp01) {
  const float d0 = fs[0] - Y.bias[0], d1 = fs[1] - Y.bias[1], d2 = fs[2] - Y.bias[2];
  float rgb[3];
  for (int i = 0; i < 3; i++) rgb[i] = Y.mat[i] * d0 + Y.mat[3 + i] * d1 + Y.mat[6 + i] * d2;
  if (clamp01) for (int i = 0; i < 3; i++) rgb[i] = wr_clamp(rgb[i], 0.0f, 1.0f);
  uint32_t pc[2];
  wr_pack_color(wf4{rgb[0], rgb[1], rgb[2], 1.0f}, pc);
  WrWide s; s.bg = pc[0]; s.ra = pc[1];
  return s;
}

// `row`: see wr_yuv_chroma_prim (nullptr: the chroma planes' edges of the record)
__device__ __noinline__ WrWide wr_yuv_pixel(const WrPrim* Pp, const WrYuvRec* Yp, const WrDrawDesc* D, int x, int y, const WrRuns* runs = nullptr,
                                            const float* row = nullptr) {
  const WrYuvRec& Y = *Yp;
  const int planes = Y.format == 3 ? 3 : (Y.format == 4 ? 1 : 2);      // (YUV_FORMAT_INTERLEAVED: blendYUV's one-sampler overload, swgl_ext.h:1027-1047)
  bool all_linear = true;
  for (int pl = 0; pl < planes; pl++) all_linear = all_linear && D->tex[WR_S_COLOR0 + pl].linear != 0;
  if ((D->flags & WR_DF_TEX_RECT) && planes == 3 && all_linear) {
    WrWide w;
    if (wr_yuv_rect_span_pixel(Pp, Y, D, x, y, runs, w, row)) return w;
  }
  int sample[3] = {0, 0, 0};          // y, u, v as the span shader's u16 lanes
  float fs[3] = {0.f, 0.f, 0.f};      // ... and as main()'s floats
  bool tail = false;
  for (int pl = 0; pl < planes; pl++) {
    WrPrim P2 = *Pp;                  // the same walk on this plane's varying (wr_mix_blend_pixel)
    P2.kind = WR_PK_TEX_R8;           // (the quantised fallback stepping of an R8 / RG8 plane: filter 1)
    if (pl > 0) wr_yuv_chroma_prim(P2, Y, pl, row);
    const WrTexDesc& t = D->tex[WR_S_COLOR0 + pl];
    const WrTexRow r = wr_tex_row(P2, t, y, runs, x, !all_linear);
    const int n = x - r.x0;
    const float W = t.sw, H = t.sh;
    if (n < r.span) {
      const float qs = 128.0f, qo = 0.5f - 0.5f * qs;
      float q[4], qy[4];
      for (int i = 0; i < 4; i++) { q[i] = r.lu[i] * W * qs + qo; qy[i] = r.lv[i] * H * qs + qo; }
      const float stepx = 4.0f * (q[1] - q[0]), stepy = 4.0f * (qy[1] - qy[0]);
      const float minx = wr_max(P2.uv_bounds[0] * W * qs + qo, 0.0f), miny = wr_max(P2.uv_bounds[1] * H * qs + qo, 0.0f);
      const float maxx = wr_max(P2.uv_bounds[2] * W * qs + qo, minx), maxy = wr_max(P2.uv_bounds[3] * H * qs + qo, miny);
      int v4[4];
      if (t.format == WR_FMT_YUY2) {
        // (the same stepping; sampleYUV's one-sampler overload hands textureLinearPlanarYUY2's lanes to the matrix as (y, u, v))
        const int c = n >> 2, k = n & 3;
        const WrYuv3 s = wr_yuy2_linear(&t, int(wr_clamp(wr_accum(q[k], stepx, c), minx, maxx)), int(wr_clamp(wr_accum(qy[k], stepy, c), miny, maxy)));
        sample[0] = s.y; sample[1] = s.u; sample[2] = s.v;
      } else if (t.format == WR_FMT_R16 || t.format == WR_FMT_RG16) {
        // (blendYUV's stepping, as wr_linear_span_pixel's fallback does it; the samples shifted down to the matrix's 8 + rescale bits)
        const int c = n >> 2, k = n & 3;
        const int iqx = int(wr_clamp(wr_accum(q[k], stepx, c), minx, maxx)), iqy = int(wr_clamp(wr_accum(qy[k], stepy, c), miny, maxy));
        const int bits = (16 - Y.rescale - 1) - 8;
        if (t.format == WR_FMT_RG16) { wr_bilinear16<2>(t, iqx, iqy, v4); sample[1] = v4[0] >> bits; sample[2] = v4[1] >> bits; }
        else { wr_bilinear16<1>(t, iqx, iqy, v4); sample[pl] = v4[0] >> bits; }
      } else if (t.format == WR_FMT_RG8) {
        wr_linear_span_pixel<2>(t, q, qy, stepx, stepy, minx, maxx, miny, maxy, 1, r.span, n, v4);
        sample[1] = v4[0]; sample[2] = v4[1];
      } else {
        wr_linear_span_pixel<1>(t, q, qy, stepx, stepy, minx, maxx, miny, maxy, 1, r.span, n, v4);
        sample[pl] = v4[0];
      }
    } else {
      tail = true;
      float cu, cv;
      wr_tex_tail_uv(P2, r, n, cu, cv);
      wr_yuv_main_sample(t, pl, cu, cv, fs);
    }
  }
  if (!tail) return wr_yuv_convert(Y, sample[0], sample[1], sample[2]);
  return wr_yuv_main_rgb(Y, fs, (Pp->flags & WR_PF_TAIL_MODULATE) != 0);
}

// ---------------------------------------------------------------------------
// CompositeYUV: linear_row_yuv (composite.h:993-1157) chunk by chunk.  One thread = one 4-pixel chunk of one destination row.
WR_DEVICE int wr_i16(int v) { return (int)(int16_t)v; }
// textureLinearRowR8 / textureLinearRowPairedR8 for one lane: x in 1/128 texels, the row pair and its 7-bit fraction given
WR_DEVICE int wr_yuv_row_tap(const WrTexDesc& t, int qx, long long row_off, long long row_stride, int fracv) {
  int ix = qx >> 7;
  const int fracx = (((ix >= 0) ? qx : 0) | (ix > t.width - 2 ? -1 : 0)) & 0x7F;      // (127, not 128, past the last pair: composite.h:806)
  ix = wr_clamp_coord(ix, t.width - 1);
  const uint8_t* b = (const uint8_t*)t.ptr + row_off;
  const int a0 = b[ix], a1 = b[ix + 1], b0 = b[row_stride + ix], b1 = b[row_stride + ix + 1];
  const int l = wr_i16(a0 + wr_i16(wr_i16((b0 - a0) * fracv) >> 7)), r = wr_i16(a1 + wr_i16(wr_i16((b1 - a1) * fracv) >> 7));
  return wr_i16(l + wr_i16(wr_i16((r - l) * fracx) >> 7));
}
WR_DEVICE int wr_yuv_vlerp(const uint8_t* row, long long stride, long long x, int fracv) {      // one column of a row pair
  const int a = row[x], b = row[x + stride];
  return wr_i16(a + wr_i16(wr_i16((b - a) * fracv) >> 7));
}
// ... and one 4-pixel chunk `c` of the row: the planes' samples as the colour matrix takes them (yV, cV: int32_t(srcUV.y))
WR_DEVICE void wr_yuv_row_chunk(const WrTexDesc& Ty, const WrTexDesc& Tu, const WrTexDesc& Tv, const WrYuvRowArgs& R, int yV, int cV, int c,
                                int (&ys)[4], int (&us)[4], int (&vs)[4]) {
    int yq[4], cq[4];
    for (int i = 0; i < 4; i++) { yq[i] = (int)((uint32_t)R.yU[i] + (uint32_t)c * (uint32_t)R.yDU); cq[i] = (int)((uint32_t)R.cU[i] + (uint32_t)c * (uint32_t)R.cDU); }
    if (Ty.format == WR_FMT_R16) {
      const int bits = (R.color_depth - 1) - 8;
      for (int i = 0; i < 4; i++) {
        int t4[4];
        wr_bilinear16<1>(Ty, yq[i] >> 8, yV, t4); ys[i] = t4[0] >> bits;
        wr_bilinear16<1>(Tu, cq[i] >> 8, cV, t4); us[i] = t4[0] >> bits;
        wr_bilinear16<1>(Tv, cq[i] >> 8, cV, t4); vs[i] = t4[0] >> bits;
      }
    } else {
      const int yfv = yV & 0x7F, cfv = cV & 0x7F;
      yV >>= 7; cV >>= 7;
      const long long yoff = (long long)wr_clamp_coord(yV, Ty.height) * Ty.stride, ystr = (yV >= 0 && yV < Ty.height - 1) ? Ty.stride : 0;
      const long long coff = (long long)wr_clamp_coord(cV, Tu.height) * Tu.stride, cstr = (cV >= 0 && cV < Tu.height - 1) ? Tu.stride : 0;
      if (c >= R.fast0 && c < R.fast1) {
        // upscaleYUV42R8 (composite.h:857-986): luma per lane out of a 4 + 4 texel window, chroma at the chunk's two averaged
        // coordinates, the four pixels' chroma estimated from those two samples
        const int k = c - R.fast0;
        const uint8_t* yrow = (const uint8_t*)Ty.ptr + yoff;
        const uint8_t* urow = (const uint8_t*)Tu.ptr + coff;
        const uint8_t* vrow = (const uint8_t*)Tv.ptr + coff;
        const int ca = (int)((uint32_t)R.cA + (uint32_t)k * (uint32_t)R.cDU), cb = (int)((uint32_t)R.cB + (uint32_t)k * (uint32_t)R.cDU);
        int yI[4]; for (int i = 0; i < 4; i++) yI[i] = yq[i] >> 15;
        const int cIx = ca >> 15, cIy = cb >> 15;
        const int yInx = (int)((uint32_t)yq[0] + (uint32_t)R.yDU) >> 15, cInx = (int)((uint32_t)ca + (uint32_t)R.cDU) >> 15;
        int s[4], n[4];
        for (int i = 0; i < 4; i++) { s[i] = wr_yuv_vlerp(yrow, ystr, (long long)yI[0] + i, yfv); n[i] = wr_yuv_vlerp(yrow, ystr, (long long)yInx + i, yfv); }
        int ysh[4] = {s[0], s[1], s[2], s[3]};
        int ysn[4] = {s[1], s[2], s[3], yInx == yI[3] ? n[1] : n[0]};
        if (yI[1] == yI[0]) { const int a[4] = {ysh[0], ysh[0], ysh[1], ysh[2]}, b[4] = {ysn[0], ysn[0], ysn[1], ysn[2]}; for (int i = 0; i < 4; i++) { ysh[i] = a[i]; ysn[i] = b[i]; } }
        if (yI[2] == yI[1]) { const int a[4] = {ysh[0], ysh[1], ysh[1], ysh[2]}, b[4] = {ysn[0], ysn[1], ysn[1], ysn[2]}; for (int i = 0; i < 4; i++) { ysh[i] = a[i]; ysn[i] = b[i]; } }
        if (yI[3] == yI[2]) { const int a[4] = {ysh[0], ysh[1], ysh[2], ysh[2]}, b[4] = {ysn[0], ysn[1], ysn[2], ysn[2]}; for (int i = 0; i < 4; i++) { ysh[i] = a[i]; ysn[i] = b[i]; } }
        const int u0 = wr_yuv_vlerp(urow, cstr, cIx, cfv), u1 = wr_yuv_vlerp(urow, cstr, (long long)cIx + 1, cfv);
        const int v0 = wr_yuv_vlerp(vrow, cstr, cIx, cfv), v1 = wr_yuv_vlerp(vrow, cstr, (long long)cIx + 1, cfv);
        const int nu0 = wr_yuv_vlerp(urow, cstr, cInx, cfv), nu1 = wr_yuv_vlerp(urow, cstr, (long long)cInx + 1, cfv);
        const int nv0 = wr_yuv_vlerp(vrow, cstr, cInx, cfv), nv1 = wr_yuv_vlerp(vrow, cstr, (long long)cInx + 1, cfv);
        int csh[4] = {u0, u1, v0, v1};
        int csn[4] = {u1, cInx == cIy ? nu1 : nu0, v1, cInx == cIy ? nv1 : nv0};
        if (cIy == cIx) { csh[1] = csh[0]; csh[3] = csh[2]; csn[1] = csn[0]; csn[3] = csn[2]; }
        const int fr[8] = {(yq[0] >> 8) & 0x7F, (yq[1] >> 8) & 0x7F, (yq[2] >> 8) & 0x7F, (yq[3] >> 8) & 0x7F, (ca >> 8) & 0x7F, (cb >> 8) & 0x7F, (ca >> 8) & 0x7F, (cb >> 8) & 0x7F};
        int px[8];
        for (int i = 0; i < 4; i++) px[i] = wr_i16(ysh[i] + wr_i16(wr_i16((ysn[i] - ysh[i]) * fr[i]) >> 7));
        for (int i = 0; i < 4; i++) px[4 + i] = wr_i16(csh[i] + wr_i16(wr_i16((csn[i] - csh[i]) * fr[4 + i]) >> 7));
        const int uA = px[4], uB = px[5], vA = px[6], vB = px[7];
        for (int i = 0; i < 4; i++) ys[i] = px[i];
        us[0] = wr_i16(uA + (wr_i16(uA - uB) >> 2)); us[1] = wr_i16(uA + (wr_i16(uB - uA) >> 2)); us[2] = wr_i16(uB + (wr_i16(uA - uB) >> 2)); us[3] = wr_i16(uB + (wr_i16(uB - uA) >> 2));
        vs[0] = wr_i16(vA + (wr_i16(vA - vB) >> 2)); vs[1] = wr_i16(vA + (wr_i16(vB - vA) >> 2)); vs[2] = wr_i16(vB + (wr_i16(vA - vB) >> 2)); vs[3] = wr_i16(vB + (wr_i16(vB - vA) >> 2));
      } else {
        for (int i = 0; i < 4; i++) {
          ys[i] = wr_yuv_row_tap(Ty, yq[i] >> 8, yoff, ystr, yfv);
          us[i] = wr_yuv_row_tap(Tu, cq[i] >> 8, coff, cstr, cfv);
          vs[i] = wr_yuv_row_tap(Tv, cq[i] >> 8, coff, cstr, cfv);
        }
      }
    }
}
#ifndef WR_INST_ONLY
__global__ void wr_composite_yuv_kernel(WrYuvBlitArgs A) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int chunks = (A.span + 3) >> 2;
  if (tid >= (long long)chunks * A.rows) return;
  const int row = (int)(tid / chunks), c = (int)(tid % chunks);
  const int left = A.span - 4 * c, npx = left < 4 ? left : 4;
  uint32_t* dst = (uint32_t*)((uint8_t*)A.dst + (size_t)(A.dy0 + row) * A.dst_stride) + A.dx0 + 4 * c;
  WrYuvRec M;
  M.bu = A.bu; M.rv = A.rv; M.gu = A.gu; M.gv = A.gv; M.ycoeff = A.ycoeff; M.ybias = A.ybias; M.uvbias = A.uvbias; M.brmask = A.brmask;
  // the row's v coordinates: `srcUV.y += srcDUV.y` once per row
  const float sv = wr_accum(A.src_v0, A.src_dv, row), cvf = wr_accum(A.chroma_v0, A.chroma_dv, row);
  uint32_t out[4];
  if (A.nearest) {
    // a single texel of every plane, nearest, converted once (composite.h:1014-1031)
    auto fetch = [](const WrTexDesc& t, float fu, float fv) -> float {
      const int x = wr_clamp_coord(int(fu), t.width), y = wr_clamp_coord(int(fv), t.height);
      if (t.format == WR_FMT_R16) return float(((const uint16_t*)t.ptr)[(size_t)y * t.stride + x]) * (1.0f / 65535.0f);
      return float(((const uint8_t*)t.ptr)[(size_t)y * t.stride + x]) * (1.0f / 255.0f);
    };
    float yf = fetch(A.y, A.src_u0, sv), uf = fetch(A.u, A.chroma_u0, cvf), vf = fetch(A.v, A.chroma_u0, cvf);
    if (A.color_depth > 8) { const float k = float(1 << (16 - A.color_depth)); yf *= k; uf *= k; vf *= k; }
    const WrWide w = wr_yuv_convert(M, wr_i16(wr_round_pixel(yf)), wr_i16(wr_round_pixel(uf)), wr_i16(wr_round_pixel(vf)));
    const uint32_t p = wr_pack(w);
    for (int i = 0; i < 4; i++) out[i] = p;
  } else {
    int ys[4], us[4], vs[4];
    WrYuvRowArgs R;
    for (int i = 0; i < 4; i++) { R.yU[i] = A.yU[i]; R.cU[i] = A.cU[i]; }
    R.yDU = A.yDU; R.cDU = A.cDU; R.fast0 = A.fast0; R.fast1 = A.fast1; R.cA = A.cA; R.cB = A.cB; R.color_depth = A.color_depth;
    wr_yuv_row_chunk(A.y, A.u, A.v, R, int(sv), int(cvf), c, ys, us, vs);      // (int32_t(srcUV.y): truncation)
    for (int i = 0; i < 4; i++) out[i] = wr_pack(wr_yuv_convert(M, ys[i], us[i], vs[i]));
  }
  for (int i = 0; i < npx; i++) dst[i] = out[i];
}
#endif

// The part of a cs_blur row that every pixel of the row shares: the interpolants at the span start, the integer texel position the span
// shader starts from and how many pixels it draws (the rest of the row is main()'s).
struct WrBlurRow { float ou, ov, su, sv; int startX, curY, drawn; };
template <int FMT>
WR_DEVICE WrBlurRow wr_blur_row_setup(const WrPrim& P, const WrBlurRec& B, int y) {
  WrBlurRow R;
  const int tw = int(B.wh & 0xFFFF);
  const float W = float(tw), H = float(int(B.wh >> 16));
  // interpolants at the span start (as wr_tex_row)
  const int k = y - P.y0;
  const float Lu = wr_accum(P.uvL0[0], P.uvLs[0], k), Lv = wr_accum(P.uvL0[1], P.uvLs[1], k);
  const float Ru = wr_accum(P.uvR0[0], P.uvRs[0], k), Rv = wr_accum(P.uvR0[1], P.uvRs[1], k);
  float stepScale = 1.0f / (P.xr - P.xl);
  if (!wr_isfinite(stepScale)) stepScale = 0.0f;
  R.su = (Ru - Lu) * stepScale; R.sv = (Rv - Lv) * stepScale;
  const float start = float(P.x0) + 0.5f - P.xl;
  R.ou = Lu + R.su * start; R.ov = Lv + R.sv * start;
  const int len = P.x1 - P.x0, span = len >= 4 ? (len & ~3) : 0;
  const bool fmt_ok = B.format == FMT && B.ptr != nullptr;
  R.startX = int(R.ou * W); R.curY = int(R.ov * H);
  R.drawn = 0;
  if (fmt_ok && span > 0) {
    const int endX = wr_imin(wr_imin(B.bounds[2], R.startX + span), tw);
    if (endX - R.startX >= 4) R.drawn = (endX - R.startX) & ~3;
  }
  return R;
}
// Span pixel n < drawn of the row (blendGaussianBlur -> gaussianBlurHorizontal / Vertical, texture.h:1165-1308): the chunk's texel
// position is the integer position of the span start plus whole chunks; tap o reads the texels o to either side, each side clamped to
// the blur bounds -- along the row in whole-chunk terms for the horizontal pass (taps inside the chunk's own four texels are never
// clamped), along the column for the vertical one; 8.8 fixed-point weights, 16-bit wrap of every product, saturating adds.
// One loop for both directions and both formats: this is the code a thin blur level runs from a cold instruction cache.
template <int FMT>
WR_DEVICE WrWide wr_blur_span_px(const WrBlurRec& B, const WrBlurRow& R, const int n) {
  const int tw = int(B.wh & 0xFFFF), th = int(B.wh >> 16);
  constexpr int NCH = FMT == WR_FMT_RGBA8 ? 4 : 1;
  const int kk = n & 3, ix = R.startX + (n & ~3), curY = R.curY;
  const int radius = B.radius;
  const ptrdiff_t at = (ptrdiff_t)wr_clamp_coord(ix, tw - 1) + (ptrdiff_t)wr_clamp_coord(curY, th) * B.stride + kk;
  const bool hori = B.hori != 0;
  // horizontal: offsets in texels relative to the chunk start (rb / lb: how far the chunk start is from the bounds);
  // vertical: offsets in rows (amax / bmax)
  const int rlim = hori ? wr_imin(B.bounds[2], tw - 1) - ix : wr_imax(wr_imin(B.bounds[3], th - 1) - curY, 0);
  const int llim = hori ? ix - wr_imax(B.bounds[0], 0) : wr_imax(curY - wr_imax(B.bounds[1], 0), 0);
  const ptrdiff_t unit = hori ? 1 : (ptrdiff_t)B.stride;
  auto texel = [&](ptrdiff_t i) -> uint32_t { return FMT == WR_FMT_RGBA8 ? ((const uint32_t*)B.ptr)[i] : (uint32_t)((const uint8_t*)B.ptr)[i]; };
  uint32_t sum[NCH];
  {
    const uint32_t c = texel(at), w0 = B.weights[0];
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) sum[ch] = (((c >> (8 * ch)) & 0xFF) * w0) & 0xFFFF;
  }
  // taps in batches of eight: the sixteen texel loads of a batch are issued together and waited for once (a tap per round trip
  // made a thin level as long as radius x pixels-per-lane dependent L2 accesses); a tap beyond the radius re-reads the last one
  // with weight 0, which leaves the saturating sum as it is
  for (int o0 = 1; o0 <= radius; o0 += 8) {
    uint32_t rr[8], ll[8], ww[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int o = wr_imin(o0 + j, radius);
      // (hori: kk + o stays unclamped while it is inside the chunk, then min(kk + o, rb) from the chunk start; likewise to the left)
      const int ro = hori ? ((kk + o <= 3) ? o : wr_imin(kk + o, rlim) - kk) : wr_imin(o, rlim);
      const int lo = hori ? ((o <= kk) ? o : wr_imin(o - kk, llim) + kk) : wr_imin(o, llim);
      rr[j] = texel(at + (ptrdiff_t)ro * unit); ll[j] = texel(at - (ptrdiff_t)lo * unit);
      ww[j] = o0 + j <= radius ? (uint32_t)B.weights[o] : 0u;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
#pragma unroll
      for (int ch = 0; ch < NCH; ch++) {
        const uint32_t t = ((((rr[j] >> (8 * ch)) & 0xFF) + ((ll[j] >> (8 * ch)) & 0xFF)) * ww[j]) & 0xFFFF;
        const uint32_t a = sum[ch] + t;
        sum[ch] = a > 0xFFFF ? 0xFFFF : a;
      }
    }
  }
  WrWide out;
  if (FMT == WR_FMT_RGBA8) {
    out.bg = (sum[0] >> 8) | ((sum[1] >> 8) << 16);
    out.ra = (sum[2] >> 8) | ((sum[3] >> 8) << 16);
  } else {
    out.bg = sum[0] >> 8; out.ra = 0;
  }
  return out;
}
// A pixel the span shader leaves to main() (cs_blur.glsl:137-181): the row's last (len & 3) pixels, or every pixel of a row it did not draw
template <int FMT>
__device__ __noinline__ WrWide wr_blur_tail_px(const WrPrim* Pp, const WrBlurRec* Bp, const WrBlurRow* Rp, const int n) {
  const WrPrim& P = *Pp; const WrBlurRec& B = *Bp; const WrBlurRow& R = *Rp;
  (void)P;
  const int tw = int(B.wh & 0xFFFF), th = int(B.wh >> 16);
  const float W = float(tw), H = float(th);
  const float su = R.su, sv = R.sv, ou = R.ou, ov = R.ov;
  const int drawn = R.drawn;
  WrWide out; out.bg = out.ra = 0;
  // ---- fragment shader: uv of this pixel = its init_interp lane, stepped by
  // `drawn` at once (DISPATCH_DRAW_SPAN) and then chunk by chunk
  const int lane = (n - drawn) & 3, m = (n - drawn) >> 2;
  float lu = ou, lv = ov;
  for (int i = 0; i < lane; i++) { lu += su; lv += sv; }
  if (drawn > 0) { const float chunks = float(drawn) * 0.25f; lu = lu + (su * 4.0f) * chunks; lv = lv + (sv * 4.0f) * chunks; }
  lu = wr_accum(lu, (su * 4.0f) * 1.0f, m); lv = wr_accum(lv, (sv * 4.0f) * 1.0f, m);
  const WrTexDesc t{B.ptr, tw, th, B.stride, (int16_t)B.format, (int16_t)B.linear, W, H};
  auto sample = [&](float uu, float vv, float (&c)[4]) {
    // texture(sColor0, uv): linear (texture.h:1028-1071 / 576-583) or nearest
    if (B.format == WR_FMT_R8) {
      float r;
      if (t.linear) r = float(wr_sample_linear_r8(t, int(uu * W * 128.0f + (0.5f - 64.0f)), int(vv * H * 128.0f + (0.5f - 64.0f)))) * (1.0f / 255.0f);
      else r = float(((const uint8_t*)t.ptr)[(size_t)wr_clamp_coord(int(uu * W), tw) + (size_t)wr_clamp_coord(int(vv * H), th) * t.stride]) * (1.0f / 255.0f);
      c[0] = r; c[1] = 0.0f; c[2] = 0.0f; c[3] = 1.0f;
    } else {
      uint32_t b, g, r, a;
      if (t.linear) {
        const WrWide s = wr_sample_linear_rgba8(t, int(uu * W * 128.0f + (0.5f - 64.0f)), int(vv * H * 128.0f + (0.5f - 64.0f)));
        b = s.bg & 0xFFFF; g = s.bg >> 16; r = s.ra & 0xFFFF; a = s.ra >> 16;
      } else {
        const uint32_t p = ((const uint32_t*)t.ptr)[(size_t)wr_clamp_coord(int(uu * W), tw) + (size_t)wr_clamp_coord(int(vv * H), th) * t.stride];
        b = p & 0xFF; g = (p >> 8) & 0xFF; r = (p >> 16) & 0xFF; a = p >> 24;
      }
      c[0] = float(r) * (1.0f / 255.0f); c[1] = float(g) * (1.0f / 255.0f);
      c[2] = float(b) * (1.0f / 255.0f); c[3] = float(a) * (1.0f / 255.0f);
    }
  };
  float gx = B.coeffs[0], gy = B.coeffs[1];
  const float gz = gy * gy;
  float c0[4], avg[4];
  if (!t.ptr) { c0[0] = c0[1] = c0[2] = c0[3] = 0.0f; } else sample(lu, lv, c0);
  for (int ch = 0; ch < 4; ch++) avg[ch] = c0[ch] * gx;
  const int support = wr_imin(B.radius, 300);
  for (int i = 1; i <= support; i += 2) {
    gx *= gy; gy *= gz;
    float sub = gx;
    gx *= gy; gy *= gz;
    sub += gx;
    const float ratio = gx / sub;
    const float offx = B.offset_scale[0] * (float(i) + ratio), offy = B.offset_scale[1] * (float(i) + ratio);
    float a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    if (t.ptr) {
      sample(wr_max(lu - offx, B.uv_rect[0]), wr_max(lv - offy, B.uv_rect[1]), a);
      sample(wr_min(lu + offx, B.uv_rect[2]), wr_min(lv + offy, B.uv_rect[3]), b);
    }
    for (int ch = 0; ch < 4; ch++) avg[ch] += (a[ch] + b[ch]) * sub;
  }
  if (FMT == WR_FMT_RGBA8) {
    if (B.format == WR_FMT_R8) { avg[1] = avg[2] = avg[3] = avg[0]; }   // ALPHA_TARGET shader on a colour target: vec4(r)
    uint32_t pc[2];
    wr_pack_color(wf4{avg[0], avg[1], avg[2], avg[3]}, pc);
    out.bg = pc[0]; out.ra = pc[1];
  } else {
    out.bg = uint32_t(wr_round_pixel(avg[0])) & 0xFFFF;
  }
  return out;
}
// pixel n of the row (n = x - P.x0)
template <int FMT>
WR_DEVICE WrWide wr_blur_row_pixel(const WrPrim& P, const WrBlurRec& B, const WrBlurRow& R, const int n) {
  if (n < R.drawn) return wr_blur_span_px<FMT>(B, R, n);
  return wr_blur_tail_px<FMT>(&P, &B, &R, n);
}
template <int FMT>
__device__ __noinline__ WrWide wr_blur_pixel(const WrPrim* Pp, const WrBlurRec* Bp, int x, int y) {
  const WrBlurRow R = wr_blur_row_setup<FMT>(*Pp, *Bp, y);
  return wr_blur_row_pixel<FMT>(*Pp, *Bp, R, x - Pp->x0);
}

// ---------------------------------------------------------------------------
// cs_clip_rectangle, one destination pixel of an R8 mask (returns the u16 value
// handed to the blend stage).  Span part: the rounded-rectangle span rasteriser
// of cs_clip_rectangle.glsl:223-495, replayed per pixel -- the run lengths are
// closed-form in chunk units, the local position of an AA chunk follows the
// same jump-then-accumulate sequence as the reference.  Tail (< 4 pixels) and
// spans shorter than 4: the fragment shader (:170-199).
WR_DEVICE float wr_clip_dist(const WrClipRec& C, float px, float py) {
  if (C.fast) {   // sd_rounded_box
    const float dx = fabsf(px) - C.params[0], dy = fabsf(py) - C.params[1];
    const float mx = wr_max(dx, 0.0f), my = wr_max(dy, 0.0f);
    return (sqrtf(mx * mx + my * my) + wr_min(wr_max(dx, dy), 0.0f)) - C.params[2];
  }
  // distance_to_rounded_rect, ellipse.glsl:50-92
  float cx = 1.0e-6f, cy = 1.0e-6f, cz = 1.0f, cw = 1.0f;
  if (px * C.plane[0][0] + py * C.plane[0][1] > C.plane[0][2]) { cx = C.center_radius[0][0] - px; cy = C.center_radius[0][1] - py; cz = C.center_radius[0][2]; cw = C.center_radius[0][3]; }
  if (px * C.plane[1][0] + py * C.plane[1][1] > C.plane[1][2]) { cx = (C.center_radius[1][0] - px) * -1.0f; cy = (C.center_radius[1][1] - py) * 1.0f; cz = C.center_radius[1][2]; cw = C.center_radius[1][3]; }
  if (px * C.plane[2][0] + py * C.plane[2][1] > C.plane[2][2]) { cx = px - C.center_radius[2][0]; cy = py - C.center_radius[2][1]; cz = C.center_radius[2][2]; cw = C.center_radius[2][3]; }
  if (px * C.plane[3][0] + py * C.plane[3][1] > C.plane[3][2]) { cx = (C.center_radius[3][0] - px) * 1.0f; cy = (C.center_radius[3][1] - py) * -1.0f; cz = C.center_radius[3][2]; cw = C.center_radius[3][3]; }
  const float prx = cx * cz, pry = cy * cw;
  const float g = (cx * prx + cy * pry) - 1.0f;
  const float dgx = (1.0f + 1.0f) * prx, dgy = (1.0f + 1.0f) * pry;
  const float e = g * (1.0f / sqrtf(dgx * dgx + dgy * dgy));
  const float r = wr_max(wr_max(C.bounds[0] - px, px - C.bounds[2]), wr_max(C.bounds[1] - py, py - C.bounds[3]));
  return wr_max(e, r);
}

// ps_quad_mask fragment (ps_quad.glsl:399-415, ps_quad_mask.glsl:167-200): one pixel of main(), which
// runs four pixels at a time -- fwidth() of the chunk is |lane1 - lane0| in x plus in y (glsl.h:765-768).
// `wrow`: a row of a general quad under a projective clip transform (C.proj) -- vClipLocalPos.w of the left and right edge on this row.
__device__ __noinline__ WrWide wr_quad_mask_pixel(const WrPrim* Pp, const WrClipRec* Cp, const WrDrawDesc* D, int x, int y, const WrRuns* runs = nullptr,
                                                  const float* wrow = nullptr) {
  const WrPrim& P = *Pp;
  const WrClipRec& C = *Cp;
  const WrTexRow r = wr_tex_row(P, D->tex[0], y, runs, x);   // span == 0 for this kind: interpolants only (of the depth run holding x)
  const int n = x - r.x0, n0 = n & ~3;
  float f0x, f0y, f1x, f1y, qx, qy;
  wr_tex_tail_uv(P, r, n0, f0x, f0y);
  wr_tex_tail_uv(P, r, n0 + 1, f1x, f1y);
  wr_tex_tail_uv(P, r, n, qx, qy);
  float w0 = C.w, w1 = C.w, wq = C.w;
  if (C.proj) {
    // a projective clip transform: .w is a varying like .xy -- the same walk on its edges (init_interp lane, one step per chunk,
    // restarted at depth runs), divided per pixel and for lanes 0 / 1 of the chunk (fwidth of the divided position)
    WrPrim P2 = P;
    P2.uvL0[0] = wrow ? wrow[0] : C.wv[0]; P2.uvLs[0] = wrow ? 0.0f : C.wv[1];
    P2.uvR0[0] = wrow ? wrow[1] : C.wv[2]; P2.uvRs[0] = wrow ? 0.0f : C.wv[3];
    P2.uvL0[1] = P2.uvLs[1] = P2.uvR0[1] = P2.uvRs[1] = 0.0f;
    P2.rows_linear = 0;
    const WrTexRow r2 = wr_tex_row(P2, D->tex[0], y, runs, x);
    float unused;
    wr_tex_tail_uv(P2, r2, n0, w0, unused);
    wr_tex_tail_uv(P2, r2, n0 + 1, w1, unused);
    wr_tex_tail_uv(P2, r2, n, wq, unused);
  }
  f0x = f0x / w0; f0y = f0y / w0; f1x = f1x / w1; f1y = f1y / w1; qx = qx / wq; qy = qy / wq;   // vClipLocalPos.xy / vClipLocalPos.w
  return wr_quad_mask_eval(C, f0x, f0y, f1x, f1y, qx, qy);
}
// ... from clip_local_pos of the pixel (qx, qy) and of lanes 0 / 1 of its chunk (fwidth) on
WR_DEVICE WrWide wr_quad_mask_eval(const WrClipRec& C, float f0x, float f0y, float f1x, float f1y, float qx, float qy) {
  const float aa_range = 1.0f / (fabsf(f1x - f0x) + fabsf(f1y - f0y));   // recip(fwidth(pos).x), shared.glsl:145-148
  const float dist = wr_clip_dist(C, qx, qy);
  const float alpha = wr_clamp(0.5f - dist * aa_range, 0.0f, 1.0f);
  const float fin = ((1.0f - alpha) - alpha) * C.mode + alpha;
  uint32_t pc[2];
  wr_pack_color(wf4{fin, fin, fin, fin}, pc);
  WrWide s; s.bg = pc[0]; s.ra = pc[1];
  return s;
}

// cs_border_solid main() (cs_border_solid.glsl:132-177; ellipse.glsl:31-45, shared.glsl:110-189), one pixel: vPos of the pixel
// and of lanes 0 / 1 of its 4-pixel chunk (fwidth).  normalize() of the flat colour-line direction is a / hypotf(a.x, a.y)
// (glsl.h:630-640): glibc evaluates hypotf in double.
WR_DEVICE float wr_ellipse_dist(float px, float py, float rx, float ry) {      // distance_to_ellipse
  const float ix = 1.0f / wr_max(rx * rx, 1.0e-6f), iy = 1.0f / wr_max(ry * ry, 1.0e-6f);
  const float scale = (rx > 0.0f && ry > 0.0f) ? 1.0f : 0.0f;
  const float prx = px * ix, pry = py * iy;
  const float g = (px * prx + py * pry) - scale;
  const float dgx = (1.0f + scale) * prx, dgy = (1.0f + scale) * pry;
  return g * (1.0f / sqrtf(dgx * dgx + dgy * dgy));
}
__device__ __noinline__ WrWide wr_border_solid_pixel(const WrPrim* Pp, const WrBorderRec* Bp, const WrDrawDesc* D, int x, int y, const WrRuns* runs = nullptr) {
  const WrPrim& P = *Pp;
  const WrBorderRec& B = *Bp;
  const WrTexRow r = wr_tex_row(P, D->tex[0], y, runs, x);   // span == 0 for this kind: interpolants only
  const int n = x - r.x0, n0 = n & ~3;
  float f0x, f0y, f1x, f1y, qx, qy;
  wr_tex_tail_uv(P, r, n0, f0x, f0y);
  wr_tex_tail_uv(P, r, n0 + 1, f1x, f1y);
  wr_tex_tail_uv(P, r, n, qx, qy);
  const float aa_range = 1.0f / (fabsf(f1x - f0x) + fabsf(f1y - f0y));
  const bool do_aa = B.mix != 2;
  float mix_factor = 0.0f;
  if (B.mix != 0) {
    const float len = float(sqrt(double(B.color_line[2]) * double(B.color_line[2]) + double(B.color_line[3]) * double(B.color_line[3])));
    const float nx = B.color_line[2] / len, ny = B.color_line[3] / len;
    const float d_line = nx * (B.color_line[0] - qx) + ny * (B.color_line[1] - qy);
    if (do_aa) mix_factor = wr_clamp(0.5f - (-d_line) * aa_range, 0.0f, 1.0f);
    else mix_factor = (d_line + 0.0001f >= 0.0f) ? 1.0f : 0.0f;
  }
  float d = -1.0f;
  {
    const float rx = qx - B.clip_center_sign[0], ry = qy - B.clip_center_sign[1];
    if (B.clip_center_sign[2] * rx < 0.0f && B.clip_center_sign[3] * ry < 0.0f) {
      const float da = wr_ellipse_dist(rx, ry, B.clip_radii[0], B.clip_radii[1]), db = wr_ellipse_dist(rx, ry, B.clip_radii[2], B.clip_radii[3]);
      d = wr_max(da, -db);
    }
  }
  {
    const float rx = qx - B.h_center_sign[0], ry = qy - B.h_center_sign[1];
    if (B.h_center_sign[2] * rx < 0.0f && B.h_center_sign[3] * ry < 0.0f) d = wr_max(wr_ellipse_dist(rx, ry, B.h_radii[0], B.h_radii[1]), d);
  }
  {
    const float rx = qx - B.v_center_sign[0], ry = qy - B.v_center_sign[1];
    if (B.v_center_sign[2] * rx < 0.0f && B.v_center_sign[3] * ry < 0.0f) d = wr_max(wr_ellipse_dist(rx, ry, B.v_radii[0], B.v_radii[1]), d);
  }
  const float alpha = do_aa ? wr_clamp(0.5f - d * aa_range, 0.0f, 1.0f) : 1.0f;
  float c[4];
#pragma unroll
  for (int i = 0; i < 4; i++) c[i] = ((B.color1[i] - B.color0[i]) * mix_factor + B.color0[i]) * alpha;
  uint32_t pc[2];
  wr_pack_color(wf4{c[0], c[1], c[2], c[3]}, pc);
  WrWide s; s.bg = pc[0]; s.ra = pc[1];
  return s;
}

// cs_border_segment main() (cs_border_segment.glsl:271-449), one pixel
WR_DEVICE float wr_dist_aa(float aa_range, float sd) { return wr_clamp(0.5f - sd * aa_range, 0.0f, 1.0f); }
WR_DEVICE float wr_dist_line(float p0x, float p0y, float dx, float dy, float px, float py) {     // distance_to_line, shared.glsl:110-113
  const float len = wr_hypotf(dx, dy);
  const float nx = dx / len, ny = dy / len;
  return nx * (p0x - px) + ny * (p0y - py);
}
WR_DEVICE void wr_border_corner_color(const WrBorderSegRec& B, float rx, float ry, int style, const float* c0in, const float* c1in,
                                      float mix_factor, float aa_range, float* out) {
  float c0[4] = {c0in[0], c0in[1], c0in[2], c0in[3]};
  if (style == 2) {
    const float da = wr_ellipse_dist(rx, ry, B.clip_radii[0] - B.partial_widths[0], B.clip_radii[1] - B.partial_widths[1]);
    const float db = wr_ellipse_dist(rx, ry, B.clip_radii[0] - 2.0f * B.partial_widths[0], B.clip_radii[1] - 2.0f * B.partial_widths[1]);
    const float a = wr_dist_aa(aa_range, wr_min(-da, db));
    for (int i = 0; i < 4; i++) c0[i] *= a;
  } else if (style == 6 || style == 7) {
    const float d = wr_ellipse_dist(rx, ry, B.clip_radii[0] - B.partial_widths[2], B.clip_radii[1] - B.partial_widths[3]);
    const float alpha = wr_dist_aa(aa_range, d);
    float sf = 0.0f;
    if (B.segment == 1) sf = mix_factor; else if (B.segment == 2) sf = 1.0f; else if (B.segment == 3) sf = 1.0f - mix_factor;
    for (int i = 0; i < 4; i++) {
      const float a0 = (c0in[i] - c1in[i]) * sf + c1in[i];       // mix(color1, color0, sf)
      const float a1 = (c1in[i] - c0in[i]) * sf + c0in[i];       // mix(color0, color1, sf)
      c0[i] = (a1 - a0) * alpha + a0;
    }
  }
  for (int i = 0; i < 4; i++) out[i] = c0[i];
}
WR_DEVICE void wr_border_edge_color(const WrBorderSegRec& B, float px, float py, int style, const float* c0in, const float* c1in,
                                    float aa_range, int axis_id, float* out) {
  const float ax = axis_id != 0 ? 0.0f : 1.0f, ay = axis_id != 0 ? 1.0f : 0.0f;
  const float pos = px * ax + py * ay;
  float c0[4] = {c0in[0], c0in[1], c0in[2], c0in[3]};
  if (style == 2) {
    float d = -1.0f;
    const float pw = B.partial_widths[0] * ax + B.partial_widths[1] * ay;
    if (pw >= 1.0f) {
      const float r0 = (B.edge_reference[0] * ax + B.edge_reference[1] * ay) + pw, r1 = (B.edge_reference[2] * ax + B.edge_reference[3] * ay) - pw;
      d = wr_min(pos - r0, r1 - pos);
    }
    const float a = wr_dist_aa(aa_range, d);
    for (int i = 0; i < 4; i++) c0[i] *= a;
  } else if (style == 6 || style == 7) {
    const float ref = (B.edge_reference[0] + B.partial_widths[2]) * ax + (B.edge_reference[1] + B.partial_widths[3]) * ay;
    const float alpha = wr_dist_aa(aa_range, pos - ref);
    for (int i = 0; i < 4; i++) c0[i] = (c1in[i] - c0in[i]) * alpha + c0in[i];
  }
  for (int i = 0; i < 4; i++) out[i] = c0[i];
}
__device__ __noinline__ WrWide wr_border_segment_pixel(const WrPrim* Pp, const WrBorderSegRec* Bp, const WrDrawDesc* D, int x, int y, const WrRuns* runs = nullptr) {
  const WrPrim& P = *Pp;
  const WrBorderSegRec& B = *Bp;
  const WrTexRow r = wr_tex_row(P, D->tex[0], y, runs, x);
  const int n = x - r.x0, n0 = n & ~3;
  float f0x, f0y, f1x, f1y, qx, qy;
  wr_tex_tail_uv(P, r, n0, f0x, f0y);
  wr_tex_tail_uv(P, r, n0 + 1, f1x, f1y);
  wr_tex_tail_uv(P, r, n, qx, qy);
  const float aa_range = 1.0f / (fabsf(f1x - f0x) + fabsf(f1y - f0y));
  float mix_factor = 0.0f;
  if (B.edge_axis[0] != B.edge_axis[1]) mix_factor = wr_dist_aa(aa_range, -wr_dist_line(B.color_line[0], B.color_line[1], B.color_line[2], B.color_line[3], qx, qy));
  const float rx = qx - B.clip_center_sign[0], ry = qy - B.clip_center_sign[1];
  const bool in_clip = B.clip_center_sign[2] * rx < 0.0f && B.clip_center_sign[3] * ry < 0.0f;
  float d = -1.0f;
  if (B.clip_mode == 3) {
    const float dx = B.cp1[0] - qx, dy = B.cp1[1] - qy;
    d = sqrtf(dx * dx + dy * dy) - B.cp1[2];
  } else if (B.clip_mode == 2) {
    const bool is_vertical = B.cp1[0] == 0.0f;
    const float half_dash = is_vertical ? B.cp1[1] : B.cp1[0];
    const float pos = is_vertical ? qy : qx;
    if (!(pos < half_dash || pos > 3.0f * half_dash)) d = 1.0f;
  } else if (B.clip_mode == 1) {
    const float d0 = wr_dist_line(B.cp1[0], B.cp1[1], B.cp1[2], B.cp1[3], qx, qy), d1 = wr_dist_line(B.cp2[0], B.cp2[1], B.cp2[2], B.cp2[3], qx, qy);
    d = wr_max(d0, -d1);
  }
  float c0[4], c1[4];
  if (in_clip) {
    const float da = wr_ellipse_dist(rx, ry, B.clip_radii[0], B.clip_radii[1]), db = wr_ellipse_dist(rx, ry, B.clip_radii[2], B.clip_radii[3]);
    d = wr_max(d, wr_max(da, -db));
    wr_border_corner_color(B, rx, ry, B.style0, B.color00, B.color01, mix_factor, aa_range, c0);
    wr_border_corner_color(B, rx, ry, B.style1, B.color10, B.color11, mix_factor, aa_range, c1);
  } else {
    wr_border_edge_color(B, qx, qy, B.style0, B.color00, B.color01, aa_range, B.edge_axis[0], c0);
    wr_border_edge_color(B, qx, qy, B.style1, B.color10, B.color11, aa_range, B.edge_axis[1], c1);
  }
  const float alpha = wr_dist_aa(aa_range, d);
  float c[4];
#pragma unroll
  for (int i = 0; i < 4; i++) c[i] = ((c1[i] - c0[i]) * mix_factor + c0[i]) * alpha;
  uint32_t pc[2];
  wr_pack_color(wf4{c[0], c[1], c[2], c[3]}, pc);
  WrWide s; s.bg = pc[0]; s.ra = pc[1];
  return s;
}

// cs_fast_linear_gradient main() (:28-30) and cs_line_decoration main() (:104-163), one pixel
WR_DEVICE float wr_dist_line_v(float p0x, float p0y, float dx, float dy, float px, float py) {   // distance_to_line with a per-pixel direction:
  const float len = sqrtf(dx * dx + dy * dy);                                                    // normalize() = a / sqrt(dot) (glsl.h:628, 637-640)
  const float nx = dx / len, ny = dy / len;
  return nx * (p0x - px) + ny * (p0y - py);
}
__device__ __noinline__ WrWide wr_cache_shader_pixel(const WrPrim* Pp, const WrAux* Ap, const WrDrawDesc* D, int x, int y, const WrRuns* runs = nullptr) {
  const WrPrim& P = *Pp;
  const WrTexRow r = wr_tex_row(P, D->tex[0], y, runs, x);
  const int n = x - r.x0, n0 = n & ~3;
  float qx, qy;
  wr_tex_tail_uv(P, r, n, qx, qy);
  float c[4];
  if (P.kind == WR_PK_FAST_GRADIENT) {
    const WrFastGradRec& G = Ap->fgrad;
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = (G.color1[i] - G.color0[i]) * qx + G.color0[i];
  } else {
    const WrLineRec& L = Ap->line;
    float f0x, f0y, f1x, f1y;
    wr_tex_tail_uv(P, r, n0, f0x, f0y);
    wr_tex_tail_uv(P, r, n0 + 1, f1x, f1y);
    const float aa_range = 1.0f / (fabsf(f1x - f0x) + fabsf(f1y - f0y));
    float alpha = 1.0f;
    if (L.style == 2) {
      alpha = (L.params[1] >= floorf(qx + 0.5f)) ? 1.0f : 0.0f;                   // step(floor(pos.x + 0.5), vParams.y)
    } else if (L.style == 1) {
      const float dx = qx - L.params[1], dy = qy - L.params[2];
      alpha = wr_dist_aa(aa_range, sqrtf(dx * dx + dy * dy) - L.params[1]);
    } else if (L.style == 3) {
      const float half_line_thickness = L.params[0], slope_length = L.params[1], flat_length = L.params[2], vertical_bounds = L.params[3];
      const float half_period = slope_length + flat_length;
      const float mid_height = vertical_bounds / 2.0f;
      float peak_offset = mid_height - half_line_thickness;
      const float two_hp = 2.0f * half_period;
      const float m2 = qx - two_hp * floorf(qx / two_hp);                           // mod(pos.x, 2 * half_period)
      const float flip = -2.0f * (((half_period >= m2) ? 1.0f : 0.0f) - 0.5f);      // step(m2, half_period)
      peak_offset *= flip;
      const float peak_height = mid_height + peak_offset;
      const float px_ = qx - half_period * floorf(qx / half_period);                // mod(pos.x, half_period)
      const float dist1 = wr_dist_line_v(0.0f, peak_height, 1.0f, -flip, px_, qy);
      const float dist2 = wr_dist_line_v(0.0f, peak_height, 0.0f, -flip, px_, qy);
      const float dist3 = wr_dist_line_v(flat_length, peak_height, -1.0f, -flip, px_, qy);
      const float dist = fabsf(wr_max(wr_max(dist1, dist2), dist3));
      alpha = wr_dist_aa(aa_range, dist - half_line_thickness);
      if (half_line_thickness <= 1.0f) alpha = 1.0f - ((0.5f >= alpha) ? 1.0f : 0.0f);   // 1 - step(alpha, 0.5)
    }
    c[0] = c[1] = c[2] = c[3] = alpha;
  }
  uint32_t pc[2];
  wr_pack_color(wf4{c[0], c[1], c[2], c[3]}, pc);
  WrWide s; s.bg = pc[0]; s.ra = pc[1];
  return s;
}

struct WrRow4 { uint32_t v[4]; };

// Four horizontally adjacent pixels (x .. x+3) of row y: the span-level setup is
// evaluated once, each pixel then only classifies its chunk.
// Interpolants of one target row at the span start (origin o[], per-pixel step s[]): what
// Edge::nextRow has accumulated after (y - y0) rows.  They are the same for every pixel of the
// row, and a wave's strip has 16 rows, so the raster stage evaluates them once per wave with 16
// row-owning lanes and hands them round with ds_bpermute (wr_apply_prim) instead of once per lane-row.
WR_DEVICE WrRowVals wr_clip_row_vals(const WrPrim& P, int y, const WrAccTabs* tabs = nullptr) {
  WrRowVals rv;
  const int k = y - P.y0;
  const bool lin = P.rows_linear != 0;
  float Lu, Lv, Ru, Rv;
  if (tabs) { Lu = wr_acctabs_row_any(tabs, 0, k); Lv = wr_acctabs_row_any(tabs, 1, k); Ru = wr_acctabs_row_any(tabs, 2, k); Rv = wr_acctabs_row_any(tabs, 3, k); }
  else {
    Lu = wr_row_interp(P.uvL0[0], P.uvLs[0], k, lin); Lv = wr_row_interp(P.uvL0[1], P.uvLs[1], k, lin);
    Ru = wr_row_interp(P.uvR0[0], P.uvRs[0], k, lin); Rv = wr_row_interp(P.uvR0[1], P.uvRs[1], k, lin);
  }
  float stepScale = 1.0f / (P.xr - P.xl);
  if (!wr_isfinite(stepScale)) stepScale = 0.0f;
  const float start = float(P.x0) + 0.5f - P.xl;
  rv.s[0] = (Ru - Lu) * stepScale; rv.s[1] = (Rv - Lv) * stepScale;
  rv.o[0] = Lu + rv.s[0] * start; rv.o[1] = Lv + rv.s[1] * start;
  rv.s[2] = rv.s[3] = rv.o[2] = rv.o[3] = 0.0f;
  return rv;
}
#ifndef WRHIP_HOSTSIM
// (a row the whole wave works on: the four sums on four lanes at once, see wr_box_row_vals_wave)
WR_DEVICE WrRowVals wr_clip_row_vals_wave(const WrPrim& P, int y, int lane, const WrAccTabs* tabs = nullptr) {
  WrRowVals rv;
  const int k = y - P.y0;
  const bool lin = P.rows_linear != 0;
  const int i = lane & 3;
  const float s0 = i == 0 ? P.uvL0[0] : i == 1 ? P.uvL0[1] : i == 2 ? P.uvR0[0] : P.uvR0[1];
  const float st = i == 0 ? P.uvLs[0] : i == 1 ? P.uvLs[1] : i == 2 ? P.uvRs[0] : P.uvRs[1];
  float r;
  if (tabs) {
    const int m = tabs->mode[i];
    r = wr_acctabs_row(tabs, i, k);
    const float other = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(((lane & 63) - 2) << 2, __builtin_bit_cast(int, r)));
    if (m == 4) r = other;
  } else r = wr_row_interp(s0, st, k, lin);
  const float Lu = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), 0)), Lv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), 1));
  const float Ru = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), 2)), Rv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), 3));
  float stepScale = 1.0f / (P.xr - P.xl);
  if (!wr_isfinite(stepScale)) stepScale = 0.0f;
  const float start = float(P.x0) + 0.5f - P.xl;
  rv.s[0] = (Ru - Lu) * stepScale; rv.s[1] = (Rv - Lv) * stepScale;
  rv.o[0] = Lu + rv.s[0] * start; rv.o[1] = Lv + rv.s[1] * start;
  rv.s[2] = rv.s[3] = rv.o[2] = rv.o[3] = 0.0f;
  return rv;
}
#endif

// Span-level setup of a cs_clip_rectangle row (cs_clip_rectangle.glsl:223-420): the lengths, in 4-pixel chunks, of the
// five phases [clear n1][AA n2][opaque n3][AA n4][clear ...] and the corners the two AA phases belong to.  It depends on
// the prim and the row only, so the raster stage evaluates it once per wave with the 16 row-owning lanes (next to the row
// interpolants) and hands it round; a 4-pixel group in a solid phase then costs a compare and a constant.
struct WrClipRow { float w, aa_range, stx, sty; int n12, n34, corners; };     // n12 = n1 | n2 << 16, n34 likewise, corners = (start + 1) | (end + 1) << 8
// `wv`: vLocalPos.w of the row (C.w; under a projective transform the row's own value, WrRowW)
WR_DEVICE WrClipRow wr_clip_row_setup(const WrPrim& P, const WrClipRec& C, const WrRowVals& rv, const float wv) {
  WrClipRow cr;
  const float su = rv.s[0], sv = rv.s[1];
  const float ou = rv.o[0], ov = rv.o[1];
  const int len = P.x1 - P.x0, span = len >= 4 ? (len & ~3) : 0;
  const float lx0 = ou, lx1 = lx0 + su;
  const float ly0 = ov, ly1 = ly0 + sv;
  const float w = 1.0f / wv;
  const float p0x = lx0 * w, p0y = ly0 * w, p1x = lx1 * w, p1y = ly1 * w;
  const float stx = (su * 4.0f) * w, sty = (sv * 4.0f) * w;
  const float aa_range = 1.0f / (fabsf(p1x - p0x) + fabsf(p1y - p0y));
  int n1 = 0, n2 = 0, n3 = 0, n4 = 0, start_corner = -1, end_corner = -1;
  if (span > 0 && wv > 0.0f) {
    const float step_scale = wr_max(stx * stx + sty * sty, 1.0e-6f);
    float aa_margin = 1.0f / sqrtf(aa_range * aa_range * step_scale);
    float cr0, cr1, cr2, cr3;
    if (C.fast) { cr0 = -C.params[0] - C.params[2]; cr1 = -C.params[1] - C.params[2]; cr2 = C.params[0] + C.params[2]; cr3 = C.params[1] + C.params[2]; }
    else { cr0 = C.bounds[0]; cr1 = C.bounds[1]; cr2 = C.bounds[2]; cr3 = C.bounds[3]; }
    const bool negx = stx < 0.0f, negy = sty < 0.0f;
    float cd0 = (negx ? cr2 : cr0) - p0x, cd1 = (negy ? cr3 : cr1) - p0y, cd2 = (negx ? cr0 : cr2) - p0x, cd3 = (negy ? cr1 : cr3) - p0y;
    const float rsx = 1.0f / stx, rsy = 1.0f / sty;
    cd0 = stx != 0.0f ? cd0 * rsx : 1.0e6f * wr_step01(0.0f, cd0);
    cd1 = sty != 0.0f ? cd1 * rsy : 1.0e6f * wr_step01(0.0f, cd1);
    cd2 = stx != 0.0f ? cd2 * rsx : 1.0e6f * wr_step01(0.0f, cd2);
    cd3 = sty != 0.0f ? cd3 * rsy : 1.0e6f * wr_step01(0.0f, cd3);
    float opaque_start = wr_max(cd0, cd1), opaque_end = wr_min(cd2, cd3);
    float aa_start = opaque_start, aa_end = opaque_end;
    const float offset = (C.params[0] + C.params[1] + C.params[2]) * C.params[2], z = C.params[2];
#pragma unroll
    for (int c = 0; c < 4; c++) {                    // CLIP_CORNER in TL, TR, BR, BL order
      float pa, pb, pc;
      if (C.fast) { pa = (c == 0 || c == 3) ? -z : z; pb = (c < 2) ? -z : z; pc = offset; }
      else { pa = C.plane[c][0]; pb = C.plane[c][1]; pc = C.plane[c][2]; }
      const float dist = (p0x * pa + p0y * pb) - pc;
      const float scale = -(stx * pa + sty * pb);
      if (scale >= 0.0f) {
        if (dist > opaque_start * scale) {
          start_corner = c;
          const float inv_scale = 1.0f / wr_max(scale, 1.0e-6f);
          opaque_start = dist * inv_scale;
          const float apex = (0.7071f - 0.5f) * 2.0f * fabsf(pa * pb);
          aa_start = opaque_start - apex * inv_scale;
        }
      } else if (dist > opaque_end * scale) {
        end_corner = c;
        const float inv_scale = 1.0f / wr_min(scale, -1.0e-6f);
        opaque_end = dist * inv_scale;
        const float apex = (0.7071f - 0.5f) * 2.0f * fabsf(pa * pb);
        aa_end = opaque_end - apex * inv_scale;
      }
    }
    aa_margin = wr_max(aa_margin - wr_max(aa_start - aa_end, 0.0f), 0.0f);
    aa_start -= aa_margin; aa_end += aa_margin;
    const float sl = float(span), ss = 4.0f;
    const int A = int(wr_clamp(sl - ss * floorf(aa_start), 0.0f, sl)) >> 2, B = int(wr_clamp(sl - ss * ceilf(opaque_start), 0.0f, sl)) >> 2;
    const int Cc = int(wr_clamp(sl - ss * floorf(opaque_end), 0.0f, sl)) >> 2, D = int(wr_clamp(sl - ss * ceilf(aa_end), 0.0f, sl)) >> 2;
    // remaining-length bookkeeping of the five phases, in chunks
    const int S = span >> 2;
    const int R1 = S > A ? A : S;
    n1 = S - R1;
    n2 = R1 > B ? R1 - B : 0;
    const int R2 = R1 - n2;
    n3 = R2 > Cc ? R2 - Cc : 0;
    const int R3 = R2 - n3;
    n4 = R3 > D ? R3 - D : 0;
  }
  cr.w = w; cr.aa_range = aa_range; cr.stx = stx; cr.sty = sty;
  cr.n12 = n1 | (n2 << 16); cr.n34 = n3 | (n4 << 16); cr.corners = (start_corner + 1) | ((end_corner + 1) << 8);
  return cr;
}
WR_DEVICE WrClipRow wr_clip_row_setup(const WrPrim& P, const WrClipRec& C, const WrRowVals& rv) { return wr_clip_row_setup(P, C, rv, C.w); }

// one pixel (n = x - P.x0) of a cs_clip_rectangle row
WR_DEVICE uint32_t wr_clip_rect_px(const WrPrim& P, const WrClipRec& C, const WrRowVals& rv, const WrClipRow& cr, int n, const float wv) {
  const float su = rv.s[0], sv = rv.s[1];
  const float ou = rv.o[0], ov = rv.o[1];
  const int len = P.x1 - P.x0, span = len >= 4 ? (len & ~3) : 0;
  const float mode = C.mode;
  // the four SIMD lanes of vLocalPos.xy at the span start (init_interp)
  const float lx0 = ou, lx1 = lx0 + su, lx2 = lx1 + su, lx3 = lx2 + su;
  const float ly0 = ov, ly1 = ly0 + sv, ly2 = ly1 + sv, ly3 = ly2 + sv;
  const float w = cr.w, aa_range = cr.aa_range, stx = cr.stx, sty = cr.sty;
  const int n1 = cr.n12 & 0xFFFF, n2 = cr.n12 >> 16, n3 = cr.n34 & 0xFFFF, n4 = cr.n34 >> 16;
  const int start_corner = (cr.corners & 0xFF) - 1, end_corner = (cr.corners >> 8) - 1;
  const uint32_t v_clear = uint32_t(wr_round_pixel(mode)) & 0xFFFF, v_opaque = uint32_t(wr_round_pixel(1.0f - mode)) & 0xFFFF;
  if (n < 0 || n >= len) return 0;
  const int lane = n & 3;
  const float lxl = lane == 0 ? lx0 : (lane == 1 ? lx1 : (lane == 2 ? lx2 : lx3));
  const float lyl = lane == 0 ? ly0 : (lane == 1 ? ly1 : (lane == 2 ? ly2 : ly3));
  if (n < span) {
    if (wv <= 0.0f) return 0;     // swgl_commitSolidR8(0.0)
    const int c = n >> 2;
    if (c < n1) return v_clear;
    float qx = lxl * w, qy = lyl * w;
    if (n1 > 0) { qx = qx + float(n1) * stx; qy = qy + float(n1) * sty; }
    int corner;
    if (c < n1 + n2) {
      qx = wr_accum(qx, stx, c - n1); qy = wr_accum(qy, sty, c - n1);
      corner = start_corner;
    } else if (c < n1 + n2 + n3) {
      return v_opaque;
    } else if (c < n1 + n2 + n3 + n4) {
      qx = wr_accum(qx, stx, n2); qy = wr_accum(qy, sty, n2);
      if (n3 > 0) { qx = qx + float(n3) * stx; qy = qy + float(n3) * sty; }
      qx = wr_accum(qx, stx, c - n1 - n2 - n3); qy = wr_accum(qy, sty, c - n1 - n2 - n3);
      corner = end_corner;
    } else {
      return v_clear;
    }
    float dist;
    if (C.fast) {
      dist = wr_clip_dist(C, qx, qy);
    } else {
      dist = wr_max(wr_max(C.bounds[0] - qx, qx - C.bounds[2]), wr_max(C.bounds[1] - qy, qy - C.bounds[3]));
      if (corner >= 0 && qx * C.plane[corner][0] + qy * C.plane[corner][1] > C.plane[corner][2]) {
        const float ex = qx - C.center_radius[corner][0], ey = qy - C.center_radius[corner][1];
        const float prx = ex * C.center_radius[corner][2], pry = ey * C.center_radius[corner][3];
        const float g = (ex * prx + ey * pry) - 1.0f;
        const float dgx = (1.0f + 1.0f) * prx, dgy = (1.0f + 1.0f) * pry;
        dist = g * (1.0f / sqrtf(dgx * dgx + dgy * dgy));
      }
    }
    const float alpha = wr_clamp(0.5f - dist * aa_range, 0.0f, 1.0f);
    return uint32_t(wr_round_pixel(((1.0f - alpha) - alpha) * mode + alpha)) & 0xFFFF;
  }
  // tail chunk (fragment shader): this pixel's lane and lanes 0/1 (fwidth) of its chunk, lanes stepped by `span` at once
  const float chunks = float(span) * 0.25f;
  const float tjx = (su * 4.0f) * chunks, tjy = (sv * 4.0f) * chunks;
  const int m = (n - span) >> 2;
  float t0x = lx0, t0y = ly0, t1x = lx1, t1y = ly1, tlx = lxl, tly = lyl;
  if (span > 0) { t0x = t0x + tjx; t0y = t0y + tjy; t1x = t1x + tjx; t1y = t1y + tjy; tlx = tlx + tjx; tly = tly + tjy; }
  const float sx4 = (su * 4.0f) * 1.0f, sy4 = (sv * 4.0f) * 1.0f;
  const float f0x = wr_accum(t0x, sx4, m) / wv, f0y = wr_accum(t0y, sy4, m) / wv;
  const float f1x = wr_accum(t1x, sx4, m) / wv, f1y = wr_accum(t1y, sy4, m) / wv;
  const float qx = wr_accum(tlx, sx4, m) / wv, qy = wr_accum(tly, sy4, m) / wv;
  const float far = 1.0f / (fabsf(f1x - f0x) + fabsf(f1y - f0y));
  const float dist = wr_clip_dist(C, qx, qy);
  const float alpha = wr_clamp(0.5f - dist * far, 0.0f, 1.0f);
  const float fin = ((1.0f - alpha) - alpha) * mode + alpha;
  return uint32_t(wr_round_pixel(wv > 0.0f ? fin : 0.0f)) & 0xFFFF;
}
WR_DEVICE uint32_t wr_clip_rect_px(const WrPrim& P, const WrClipRec& C, const WrRowVals& rv, const WrClipRow& cr, int n) { return wr_clip_rect_px(P, C, rv, cr, n, C.w); }

WR_DEVICE float wr_sel4(float a0, float a1, float a2, float a3, int i) { return i == 0 ? a0 : (i == 1 ? a1 : (i == 2 ? a2 : a3)); }

// ---- cs_clip_* under a projective clip or prim transform (WrClipRec::proj, WrBoxRec::proj) ----
// vLocalPos.w is a varying like .xy: its left / right edge values on a row are the row-by-row sums of its edge interpolants (wv[]), and
// the row's origin and step come out of them as the other varyings' do (rasterize.h:1011-1016).  Both span shaders begin with
// `if (swgl_interpStep(vLocalPos).w != 0.0) return;` -- interp_step is the step of a 4-pixel chunk --, so the decision is the ROW's:
// where w does not move along the row the span rasteriser runs with the row's own w, elsewhere every chunk of the row runs main().
struct WrRowW { float o, s; };
WR_DEVICE WrRowW wr_proj_row_w(const WrPrim& P, const float (&wv)[4], int y) {
  WrRowW rw;
  const int k = y - P.y0;
  const float Lw = wr_accum(wv[0], wv[1], k), Rw = wr_accum(wv[2], wv[3], k);
  float stepScale = 1.0f / (P.xr - P.xl);
  if (!wr_isfinite(stepScale)) stepScale = 0.0f;
  const float start = float(P.x0) + 0.5f - P.xl;
  rw.s = (Rw - Lw) * stepScale;
  rw.o = Lw + rw.s * start;
  return rw;
}
WR_DEVICE bool wr_proj_row_steps(const WrRowW& rw) { return rw.s * 4.0f != 0.0f; }
// One varying of pixel n of a row that main() walks from its first chunk on: the lane's start value (init_interp: o, + s, + s, + s),
// then one `+= interp_step` per chunk (step_interp_inputs).
WR_DEVICE float wr_main_walk(float o, float s, int lane, int m) {
  const float l1 = o + s, l2 = l1 + s, l3 = l2 + s;
  return wr_accum(wr_sel4(o, l1, l2, l3, lane), (s * 4.0f) * 1.0f, m);
}
// cs_clip_rectangle main() (cs_clip_rectangle.glsl:170-199) on pixel n of such a row: vLocalPos.xy / vLocalPos.w per lane, the AA range
// from lanes 0 / 1 of the pixel's chunk (fwidth of the divided position), 0 where w <= 0
WR_DEVICE uint32_t wr_clip_rect_main_px(const WrClipRec& C, const WrRowVals& rv, const WrRowW& rw, int n) {
  const int lane = n & 3, m = n >> 2;
  const float w0 = wr_main_walk(rw.o, rw.s, 0, m), w1 = wr_main_walk(rw.o, rw.s, 1, m), wq = wr_main_walk(rw.o, rw.s, lane, m);
  const float f0x = wr_main_walk(rv.o[0], rv.s[0], 0, m) / w0, f0y = wr_main_walk(rv.o[1], rv.s[1], 0, m) / w0;
  const float f1x = wr_main_walk(rv.o[0], rv.s[0], 1, m) / w1, f1y = wr_main_walk(rv.o[1], rv.s[1], 1, m) / w1;
  const float qx = wr_main_walk(rv.o[0], rv.s[0], lane, m) / wq, qy = wr_main_walk(rv.o[1], rv.s[1], lane, m) / wq;
  const float far = 1.0f / (fabsf(f1x - f0x) + fabsf(f1y - f0y));
  const float dist = wr_clip_dist(C, qx, qy);
  const float alpha = wr_clamp(0.5f - dist * far, 0.0f, 1.0f);
  const float fin = ((1.0f - alpha) - alpha) * C.mode + alpha;
  return uint32_t(wr_round_pixel(wq > 0.0f ? fin : 0.0f)) & 0xFFFF;
}
// four pixels (x .. x + 3) of row y of a projective cs_clip_rectangle prim, everything from the prim (the bin raster's route: rows outside
// the mask-row store, WRHIP_NO_MASK_ROWS)
__device__ __noinline__ WrRow4 wr_clip_rect_proj_row4(const WrPrim* Pp, const WrClipRec* Cp, int x, int y) {
  const WrPrim& P = *Pp;
  const WrRowVals rv = wr_clip_row_vals(P, y);
  const WrRowW rw = wr_proj_row_w(P, Cp->wv, y);
  const int len = P.x1 - P.x0;
  WrRow4 out;
  if (wr_proj_row_steps(rw)) {
    for (int i = 0; i < 4; i++) { const int n = x + i - P.x0; out.v[i] = (n < 0 || n >= len) ? 0u : wr_clip_rect_main_px(*Cp, rv, rw, n); }
    return out;
  }
  const WrClipRow cr = wr_clip_row_setup(P, *Cp, rv, rw.o);
  for (int i = 0; i < 4; i++) out.v[i] = wr_clip_rect_px(P, *Cp, rv, cr, x + i - P.x0, rw.o);
  return out;
}
__device__ __noinline__ WrRow4 wr_clip_rect_row4(const WrPrim* Pp, const WrClipRec* Cp, WrRowVals rv, WrClipRow cr, int x, int y) {
  WrRow4 out;
#pragma unroll
  for (int i = 0; i < 4; i++) out.v[i] = wr_clip_rect_px(*Pp, *Cp, rv, cr, x + i - Pp->x0);
  return out;
}

// ---------------------------------------------------------------------------
// cs_clip_box_shadow, one destination pixel of an R8 mask: the nine-patch span
// shader (cs_clip_box_shadow.glsl:150-324) replayed up to the pixel's chunk --
// solid lead-in, then [transitional chunk, sector run] pairs whose runs are
// swgl_commitPartialTextureLinear(Invert)R8 / solid centre fills -- or the
// fragment shader (:123-138) for the tail.
WR_DEVICE float wr_r8_texture(const WrTexDesc& t, float u, float v) {   // texture(sColor0, uv).r of an R8 sampler
  const float W = t.sw, H = t.sh;
  if (t.linear) return float(wr_sample_linear_r8(t, int(u * W * 128.0f + (0.5f - 64.0f)), int(v * H * 128.0f + (0.5f - 64.0f)))) * (1.0f / 255.0f);
  return float(((const uint8_t*)t.ptr)[(size_t)wr_clamp_coord(int(u * W), t.width) + (size_t)wr_clamp_coord(int(v * H), t.height) * t.stride]) * (1.0f / 255.0f);
}
WR_DEVICE void wr_box_map_uv(const WrBoxRec& B, float ul, float vl, float& u, float& v) {   // :124-127
  u = wr_clamp(ul, 0.0f, B.edge[0]); v = wr_clamp(vl, 0.0f, B.edge[1]);
  u += wr_max(0.0f, ul - B.edge[2]); v += wr_max(0.0f, vl - B.edge[3]);
  u = (B.uv_noclamp[2] - B.uv_noclamp[0]) * u + B.uv_noclamp[0];
  v = (B.uv_noclamp[3] - B.uv_noclamp[1]) * v + B.uv_noclamp[1];
}
WR_DEVICE float wr_box_shade(const WrBoxRec& B, const WrTexDesc& t, float ul, float vl, float lx, float ly) {
  float u, v;
  wr_box_map_uv(B, ul, vl, u, v);
  u = wr_clamp(u, B.uv_bounds[0], B.uv_bounds[2]); v = wr_clamp(v, B.uv_bounds[1], B.uv_bounds[3]);
  const float in = (wr_step01(B.bounds[0], lx) - wr_step01(B.bounds[2], lx)) * (wr_step01(B.bounds[1], ly) - wr_step01(B.bounds[3], ly));
  const float texel = wr_r8_texture(t, u, v);
  const float alpha = ((1.0f - texel) - texel) * B.mode + texel;
  return (alpha - B.mode) * in + B.mode;
}

// Four horizontally adjacent pixels (x .. x+3) of row y: one span-level setup and
// one walk of the nine-patch state machine serve all four.
// row interpolants of a cs_clip_box_shadow prim: c = 0,1 vUv; 2,3 vLocalPos.xy
// cs_clip_box_shadow main() (cs_clip_box_shadow.glsl:123-138) on pixel n of a row along which vLocalPos.w steps (see WrRowW): vUv and
// vLocalPos.xy divided by the lane's own w, 0 where it is <= 0
WR_DEVICE uint32_t wr_box_shadow_main_px(const WrBoxRec& B, const WrRowVals& rv, const WrRowW& rw, int n) {
  const WrTexDesc t{B.ptr, int(B.wh & 0xFFFF), int(B.wh >> 16), B.stride, (int16_t)B.format, (int16_t)B.linear, float(B.wh & 0xFFFF), float(B.wh >> 16)};
  const int lane = n & 3, m = n >> 2;
  const float wq = wr_main_walk(rw.o, rw.s, lane, m);
  float v4[4];
#pragma unroll
  for (int c = 0; c < 4; c++) v4[c] = wr_main_walk(rv.o[c], rv.s[c], lane, m) / wq;
  const float r = wr_box_shade(B, t, v4[0], v4[1], v4[2], v4[3]);
  return uint32_t(wr_round_pixel(wq > 0.0f ? r : 0.0f)) & 0xFFFF;
}
// `wv`: vLocalPos.w of the row (B.w; under a projective transform the row's own value)
WR_DEVICE WrRow4 wr_box_shadow_row4_w(const WrPrim* Pp, const WrBoxRec* Bp, const WrRowVals& rv, const WrBoxRow& br, int x, int y, const float wv) {
  const WrPrim& P = *Pp;
  const WrBoxRec& B = *Bp;
  WrRow4 out;
  out.v[0] = out.v[1] = out.v[2] = out.v[3] = 0;
  const WrTexDesc t{B.ptr, int(B.wh & 0xFFFF), int(B.wh >> 16), B.stride, (int16_t)B.format, (int16_t)B.linear, float(B.wh & 0xFFFF), float(B.wh >> 16)};
  float o4[4], s4[4];
#pragma unroll
  for (int c = 0; c < 4; c++) { o4[c] = rv.o[c]; s4[c] = rv.s[c]; }
  const int len = P.x1 - P.x0, span = len >= 4 ? (len & ~3) : 0;
  const int n0 = x - P.x0;
  const float mode = B.mode;
  const uint32_t v_clear = uint32_t(wr_round_pixel(mode)) & 0xFFFF;
  // SIMD lanes at the span start: [component][lane]
  float ln[4][4];
#pragma unroll
  for (int c = 0; c < 4; c++) { ln[c][0] = o4[c]; ln[c][1] = ln[c][0] + s4[c]; ln[c][2] = ln[c][1] + s4[c]; ln[c][3] = ln[c][2] + s4[c]; }
  // ---- tail pixels: fragment shader
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int n = n0 + i;
    if (n < span || n >= len || n < 0) continue;
    const int lane = (n - span) & 3, m = (n - span) >> 2;
    float v4[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float a = wr_sel4(ln[c][0], ln[c][1], ln[c][2], ln[c][3], lane);
      if (span > 0) a = a + (s4[c] * 4.0f) * (float(span) * 0.25f);
      v4[c] = wr_accum(a, (s4[c] * 4.0f) * 1.0f, m);
    }
    const float r = wr_box_shade(B, t, v4[0] / wv, v4[1] / wv, v4[2] / wv, v4[3] / wv);
    out.v[i] = uint32_t(wr_round_pixel(wv > 0.0f ? r : 0.0f)) & 0xFFFF;
  }
  // ---- span pixels
  const int first = n0 < 0 ? 0 : n0, last = (n0 + 3 < span - 1) ? n0 + 3 : span - 1;    // my pixels inside [0, span)
  if (first > last) return out;
  float w = wv;
  if (w <= 0.0f) return out;                 // swgl_commitSolidR8(0.0): zeros
  w = 1.0f / w;
  float cur[4][4], st[4];        // uv_linear.x, uv_linear.y, local_pos.x, local_pos.y lanes; per-chunk steps
#pragma unroll
  for (int c = 0; c < 4; c++) {
#pragma unroll
    for (int i = 0; i < 4; i++) cur[c][i] = ln[c][i] * w;
    st[c] = (s4[c] * 4.0f) * w;
  }
  const float sl = float(span), ss = 4.0f;
  const int shadow_start_len = br.ss_se & 0xFFFF, shadow_end_len = br.ss_se >> 16;
  const int os0 = br.os01 & 0xFFFF, os1 = br.os01 >> 16, os2 = br.os23 & 0xFFFF, os3 = br.os23 >> 16;
  // everything not claimed by the walk below is the solid lead-in / lead-out
#pragma unroll
  for (int i = 0; i < 4; i++) if (n0 + i >= 0 && n0 + i < span) out.v[i] = v_clear;
  int R = span, pos = 0;
  if (R > shadow_start_len) {
    const int nb = R - shadow_start_len;
    const float f = float(nb / 4);
#pragma unroll
    for (int c = 0; c < 4; c++) {
#pragma unroll
      for (int i = 0; i < 4; i++) cur[c][i] += f * st[c];
    }
    R -= nb; pos += nb;
  }
  while (R > 0 && pos <= last) {
    if (pos + 4 > first) {            // transitional chunk holds some of my pixels: per-fragment mapping
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int n = n0 + i;
        if (n < pos || n >= pos + 4 || n >= span) continue;
        const int lane = n & 3;
        out.v[i] = uint32_t(wr_round_pixel(wr_box_shade(B, t, wr_sel4(cur[0][0], cur[0][1], cur[0][2], cur[0][3], lane),
                                                         wr_sel4(cur[1][0], cur[1][1], cur[1][2], cur[1][3], lane),
                                                         wr_sel4(cur[2][0], cur[2][1], cur[2][2], cur[2][3], lane),
                                                         wr_sel4(cur[3][0], cur[3][1], cur[3][2], cur[3][3], lane)))) & 0xFFFF;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
#pragma unroll
      for (int i = 0; i < 4; i++) cur[c][i] += st[c];
    }
    R -= 4; pos += 4;
    if (R <= shadow_end_len) break;
    int num_inside = R - 4 - shadow_end_len;
    float ub0 = B.uv_bounds[0], ub1 = B.uv_bounds[1], ub2 = B.uv_bounds[2], ub3 = B.uv_bounds[3];
    if (R >= os1) {
      num_inside = wr_imin(num_inside, R - os1);
    } else if (R >= os3) {
      num_inside = wr_imin(num_inside, R - os3);
      const float cc = wr_clamp((B.uv_noclamp[3] - B.uv_noclamp[1]) * B.edge[1] + B.uv_noclamp[1], B.uv_bounds[1], B.uv_bounds[3]);
      ub1 = cc; ub3 = cc;
    }
    if (R >= os0) {
      num_inside = wr_imin(num_inside, R - os0);
    } else if (R >= os2) {
      num_inside = wr_imin(num_inside, R - os2);
      const float cc = wr_clamp((B.uv_noclamp[2] - B.uv_noclamp[0]) * B.edge[0] + B.uv_noclamp[0], B.uv_bounds[0], B.uv_bounds[2]);
      ub0 = cc; ub2 = cc;
    }
    if (num_inside > 0) {
      if (pos + num_inside > first && pos <= last) {
        float pu[4], pv[4];
#pragma unroll
        for (int i = 0; i < 4; i++) wr_box_map_uv(B, cur[0][i], cur[1][i], pu[i], pv[i]);
        const bool centre = ub0 == ub2 && ub1 == ub3;
        const float W = float(t.width), H = float(t.height);
        int filter = 0;
        if (!centre) {   // needsTextureLinear (swgl_ext.h:553-587)
          if (t.width < 2) filter = 0;
          else if (pv[0] != pv[1]) filter = 1;
          else {
            const float px0 = pu[0] * W, px1 = pu[1] * W, py0 = pv[0] * H;
            const int sp = (num_inside & ~127) + 128;
            const int scaled = int(roundf((px1 - px0) * float(sp)));
            if (scaled != sp) filter = (px0 < px1 && px1 - px0 <= 1.0f) ? 2 : (scaled == sp * 2 ? 4 : 1);
            else if ((int(px0 * 4.0f + 0.5f) & 3) != 2 || (int(py0 * 4.0f + 0.5f) & 3) != 2) filter = 3;
            else filter = 0;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int n = n0 + i;
          if (n < pos || n >= pos + num_inside || n >= span) continue;
          const int lane = n & 3;
          if (centre) {
            // centre sector: one texel for the whole run (pattern of the 4 lanes repeated)
            const float texel = wr_r8_texture(t, wr_clamp(wr_sel4(pu[0], pu[1], pu[2], pu[3], lane), ub0, ub2),
                                              wr_clamp(wr_sel4(pv[0], pv[1], pv[2], pv[3], lane), ub1, ub3));
            out.v[i] = uint32_t(wr_round_pixel(((1.0f - texel) - texel) * mode + texel)) & 0xFFFF;
            continue;
          }
          // swgl_commitTextureLinear(R8, sColor0, uv, uv_bounds, NoColor/InvertColor, num_inside)
          const int j = n - pos;
          int v;
          if (filter == 0) {
            // blendTextureNearestFast (swgl_ext.h:475-537)
            const int ix = int(pu[0] * W), iy = int(pv[0] * H);
            const int minUx = int(ub0 * W), minUy = int(ub1 * H), maxUx = int(ub2 * W), maxUy = int(ub3 * H);
            const int srow = wr_clamp_coord(wr_iclamp(iy, minUy, maxUy), t.height);
            const int minX = wr_iclamp(minUx, 0, t.width - 1), maxX = wr_iclamp(maxUx, minX, t.width - 1);
            v = ((const uint8_t*)t.ptr)[(size_t)srow * t.stride + wr_iclamp(ix + j, minX, maxX)];
          } else {
            const float qs = 128.0f, qo = 0.5f - 0.5f * qs;
            float q[4], qy[4];
#pragma unroll
            for (int a = 0; a < 4; a++) { q[a] = pu[a] * W * qs + qo; qy[a] = pv[a] * H * qs + qo; }
            const float stepx = 4.0f * (q[1] - q[0]), stepy = 4.0f * (qy[1] - qy[0]);
            const float minx = wr_max(ub0 * W * qs + qo, 0.0f), miny = wr_max(ub1 * H * qs + qo, 0.0f);
            const float maxx = wr_max(ub2 * W * qs + qo, minx), maxy = wr_max(ub3 * H * qs + qo, miny);
            int o[4];
            wr_linear_span_pixel<1>(t, q, qy, stepx, stepy, minx, maxx, miny, maxy, filter, num_inside, j, o);
            v = o[0];
          }
          if (mode != 0.0f) v = 255 - v;               // applyColor(src, InvertColor)
          out.v[i] = uint32_t(v) & 0xFFFF;
        }
      }
      const float f = float(num_inside / 4);
#pragma unroll
      for (int c = 0; c < 4; c++) {
#pragma unroll
        for (int i = 0; i < 4; i++) cur[c][i] += f * st[c];
      }
      R -= num_inside; pos += num_inside;
    }
  }
  return out;
}

__device__ __noinline__ WrRow4 wr_box_shadow_row4(const WrPrim* Pp, const WrBoxRec* Bp, WrRowVals rv, WrBoxRow br, int x, int y) {
  return wr_box_shadow_row4_w(Pp, Bp, rv, br, x, y, Bp->w);
}
// four pixels (x .. x + 3) of row y of a projective cs_clip_box_shadow prim, everything from the prim (the bin raster's route)
__device__ __noinline__ WrRow4 wr_box_shadow_proj_row4(const WrPrim* Pp, const WrBoxRec* Bp, int x, int y) {
  const WrPrim& P = *Pp;
  const WrRowVals rv = wr_box_row_vals(P, *Bp, y);
  const WrRowW rw = wr_proj_row_w(P, Bp->wv, y);
  const int len = P.x1 - P.x0;
  if (wr_proj_row_steps(rw)) {
    WrRow4 out;
    for (int i = 0; i < 4; i++) { const int n = x + i - P.x0; out.v[i] = (n < 0 || n >= len) ? 0u : wr_box_shadow_main_px(*Bp, rv, rw, n); }
    return out;
  }
  const WrBoxRow br = wr_box_row_setup(P, *Bp, rv, rw.o);      // (xc / vrow are the caller's shortcut: not used here)
  return wr_box_shadow_row4_w(Pp, Bp, rv, br, x, y, rw.o);
}

// the one value of the row's u-clamped run (WrBoxRow::xc): stepx is exactly 0 there, so whichever filter the run takes,
// every pixel of it gets what its first pixel gets
WR_DEVICE void wr_box_row_finish(const WrPrim* Pp, const WrBoxRec* Bp, const WrRowVals& rv, WrBoxRow& br, int y) {
  if (br.xc == 0 || rv.s[1] != 0.0f) { br.xc = 0; return; }      // (v must not move along the row either: axis-aligned prims)
  br.vrow = wr_box_shadow_row4(Pp, Bp, rv, br, Pp->x0 + (br.xc & 0xFFFF), y).v[0];
}
