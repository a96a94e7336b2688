// The payload of a delta grab (include/wrhip.h, WrhipGrabTexture) on the host: walking its entries, checking them, patching them into
// an image of the rect -- and, for the host simulation and for programs that want a payload to feed the decoder, the encoding of one
// block.  Plain C++: no HIP, no library state, nothing but this file is needed (tools/grab_codec_check.cpp includes it alone).
//
// A payload: a 16-byte header (word 0: the bytes of the entries behind it) and the entries.
//   plain   entries of 16 + 64 * 64 * bpp bytes: a record x, y, w, h (four little-endian words; the block relative to the rect, cut
//           to it) and the block's rows at a pitch of 64 * bpp
//   packed  (WRHIP_GRAB_PACKED) entries of a multiple of 16 bytes: a record x, y, w | h << 8 | mode << 16, aux and a body
//           RAW   0  aux 0; the body of a plain entry, bytes outside the cut block zero
//           SOLID 1  aux: the one value of the block; no body
//           RUNS  2  aux: n, the run starts; h words of 64 bits (bit c of word r: pixel (r, c) starts a run), the n values, zeros
//                    to the next multiple of 16
//           Pixel i of the cut block in row-major order starts a run if i == 0 or its value differs from pixel i - 1's.  One run
//           start: SOLID; otherwise RUNS if that entry is smaller than a RAW one, else RAW.
//   scroll  (WRHIP_GRAB_SCROLL) a packed payload whose header word 1 is dy, the scroll vector (int32, |dy| <= 512), and that may hold
//           COPY  3  aux 0; no body: the block -- one of the rect's 64 x 64 blocks, cut to it -- takes the pixels the image had
//                    BEFORE the decode dy rows further down (y + dy; the source rows lie inside the rect).  dy is not 0 then.
//           The decode is in place: the COPY entries first, by ascending y for dy > 0 and descending y for dy < 0 -- a block's
//           source rows are then still the old ones --, every other entry after them.
#ifndef WR_GRAB_CODEC_H
#define WR_GRAB_CODEC_H
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define WR_GC_HEADER 16
#define WR_GC_BLOCK 64
#define WR_GC_SCROLL_MAX 512
enum { WR_GC_RAW = 0, WR_GC_SOLID = 1, WR_GC_RUNS = 2, WR_GC_COPY = 3 };

struct WrGrabEntry {
  int32_t x, y, w, h;      // the block, relative to the rect
  int32_t mode;            // WR_GC_*; RAW for a plain entry
  uint32_t aux;
  size_t size;             // of the whole entry, record included
};

static inline size_t wr_gc_raw_size(int bpp) { return 16 + (size_t)WR_GC_BLOCK * WR_GC_BLOCK * bpp; }
static inline size_t wr_gc_runs_size(int h, uint32_t n, int bpp) { return 16 + (((size_t)8 * h + (size_t)n * bpp + 15) & ~(size_t)15); }
// the mode the rule gives a cut block of h rows with n run starts
static inline int wr_gc_mode(int h, uint32_t n, int bpp) {
  if (n == 1) return WR_GC_SOLID;
  return wr_gc_runs_size(h, n, bpp) < wr_gc_raw_size(bpp) ? WR_GC_RUNS : WR_GC_RAW;
}
static inline uint32_t wr_gc_load32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static inline void wr_gc_store32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static inline uint64_t wr_gc_load64(const uint8_t* p) { return (uint64_t)wr_gc_load32(p) | (uint64_t)wr_gc_load32(p + 4) << 32; }

// The entry at `p`, of which `avail` bytes belong to the payload, against a rect of rw x rh: false if its record or its body is
// not one the format allows or does not fit.  Everything wr_gc_patch relies on is checked here.
// scroll: the payload is a scroll grab's, dy its header word 1 -- a COPY entry is allowed, and checked against dy.
static inline bool wr_gc_entry(const uint8_t* p, size_t avail, int bpp, bool packed, int rw, int rh, WrGrabEntry* E, bool checked = false,
                               bool scroll = false, int32_t dy = 0) {
  if (avail < 16) return false;
  const uint32_t w0 = wr_gc_load32(p), w1 = wr_gc_load32(p + 4), w2 = wr_gc_load32(p + 8), w3 = wr_gc_load32(p + 12);
  uint32_t w, h, mode = WR_GC_RAW, aux = 0;
  if (packed) { w = w2 & 0xFFu; h = (w2 >> 8) & 0xFFu; mode = w2 >> 16; aux = w3; }
  else { w = w2; h = w3; }
  if (w < 1 || h < 1 || w > WR_GC_BLOCK || h > WR_GC_BLOCK || mode > (scroll && packed ? WR_GC_COPY : WR_GC_RUNS)) return false;
  if (w > (uint32_t)rw || h > (uint32_t)rh || w0 > (uint32_t)rw - w || w1 > (uint32_t)rh - h) return false;
  E->x = (int32_t)w0; E->y = (int32_t)w1; E->w = (int32_t)w; E->h = (int32_t)h; E->mode = (int32_t)mode; E->aux = aux;
  if (mode == WR_GC_COPY) {
    // one of the rect's blocks, whole; its source rows inside the rect
    if (aux != 0 || dy == 0 || dy < -WR_GC_SCROLL_MAX || dy > WR_GC_SCROLL_MAX) return false;
    if (w0 % WR_GC_BLOCK || w1 % WR_GC_BLOCK) return false;
    if (w != ((uint32_t)rw - w0 < WR_GC_BLOCK ? (uint32_t)rw - w0 : WR_GC_BLOCK) || h != ((uint32_t)rh - w1 < WR_GC_BLOCK ? (uint32_t)rh - w1 : WR_GC_BLOCK)) return false;
    const int64_t sy = (int64_t)w1 + dy;
    if (sy < 0 || sy + (int64_t)h > (int64_t)rh) return false;
    E->size = 16;
    return true;
  }
  if (mode == WR_GC_SOLID) { E->size = 16; return true; }
  if (mode == WR_GC_RAW) { E->size = wr_gc_raw_size(bpp); return E->size <= avail; }
  const uint32_t n = aux;
  if (n < 1 || n > w * h) return false;
  E->size = wr_gc_runs_size((int)h, n, bpp);
  if (E->size > avail) return false;
  if (checked) return true;      // (an entry this function has passed before: its record and size are all the caller is after)
  // the bitmap: no bit at a column >= w, the first pixel starts a run, as many bits as values
  const uint64_t beyond = w == 64 ? 0ull : ~0ull << w;
  uint32_t bits = 0;
  for (uint32_t r = 0; r < h; r++) {
    const uint64_t m = wr_gc_load64(p + 16 + 8 * r);
    if (m & beyond) return false;
    bits += (uint32_t)__builtin_popcountll(m);
  }
  return bits == n && (p[16] & 1u) != 0;
}

// n pixels of one value
static inline void wr_gc_fill(uint8_t* d, const uint8_t* v, int n, int bpp) {
  if (bpp == 1) { memset(d, v[0], (size_t)n); return; }
  uint32_t w;
  memcpy(&w, v, 4);
  for (int i = 0; i < n; i++) memcpy(d + 4 * (size_t)i, &w, 4);
}
// A checked entry's pixels into the image of the rect (`dst`, rows of `ds` bytes); runs are filled whole, not pixel by pixel
static inline void wr_gc_patch(const uint8_t* p, const WrGrabEntry& E, int bpp, uint8_t* dst, size_t ds) {
  uint8_t* d0 = dst + (size_t)E.y * ds + (size_t)E.x * bpp;
  if (E.mode == WR_GC_RAW) {
    for (int r = 0; r < E.h; r++) memcpy(d0 + (size_t)r * ds, p + 16 + (size_t)r * WR_GC_BLOCK * bpp, (size_t)E.w * bpp);
    return;
  }
  if (E.mode == WR_GC_SOLID) {
    uint8_t v[4];
    wr_gc_store32(v, E.aux);
    for (int r = 0; r < E.h; r++) wr_gc_fill(d0 + (size_t)r * ds, v, E.w, bpp);
    return;
  }
  const uint8_t* lit = p + 16 + 8 * (size_t)E.h;
  const uint8_t* cur = lit;      // (the first pixel starts a run: never read before it is set)
  for (int r = 0; r < E.h; r++) {
    const uint64_t m = wr_gc_load64(p + 16 + 8 * (size_t)r);
    uint8_t* d = d0 + (size_t)r * ds;
    for (int c = 0; c < E.w;) {
      if ((m >> c) & 1ull) { cur = lit; lit += bpp; }
      const uint64_t above = c == 63 ? 0ull : (m >> (c + 1)) << (c + 1);      // (the starts right of c: none at a column >= w)
      const int e = above ? __builtin_ctzll(above) : E.w;
      wr_gc_fill(d + (size_t)c * bpp, cur, e - c, bpp);
      c = e;
    }
  }
}

// The COPY entries of a scroll payload in the order they are applied in: by y, ascending; a decoder walks them from the first on
// for dy > 0 and from the last on for dy < 0.  false: two of them name one block.
struct WrGrabCopy { int32_t x, y, w, h; };
static inline int wr_gc_copy_cmp(const void* a, const void* b) {
  const WrGrabCopy* p = (const WrGrabCopy*)a; const WrGrabCopy* q = (const WrGrabCopy*)b;
  if (p->y != q->y) return p->y < q->y ? -1 : 1;
  return p->x < q->x ? -1 : p->x > q->x ? 1 : 0;
}
static inline bool wr_gc_copy_order(WrGrabCopy* c, size_t n) {
  if (n > 1) qsort(c, n, sizeof(WrGrabCopy), wr_gc_copy_cmp);
  for (size_t i = 1; i < n; i++) if (c[i].x == c[i - 1].x && c[i].y == c[i - 1].y) return false;
  return true;
}
// one COPY entry in place: the rows in the order in which a row's source has not been written yet
static inline void wr_gc_copy(const WrGrabCopy& E, int32_t dy, int bpp, uint8_t* dst, size_t ds) {
  const size_t row = (size_t)E.w * bpp;
  for (int i = 0; i < E.h; i++) {
    const int r = dy > 0 ? i : E.h - 1 - i;
    memcpy(dst + (size_t)(E.y + r) * ds + (size_t)E.x * bpp, dst + (size_t)(E.y + r + dy) * ds + (size_t)E.x * bpp, row);
  }
}
// A whole payload (`payload`: its header; `bytes`: what the caller holds of it) patched into `dst`: 0, with the bounding box of the
// entries' blocks and their number, or -1 for a malformed one -- nothing is written then: every entry is checked before the first
// is patched.  scroll: a scroll grab's payload (header word 1: dy; COPY entries); any other payload's header word 1 is 0.
static inline int wr_gc_decode(const void* payload, uint64_t bytes, int bpp, bool packed, int rw, int rh, void* dst, int64_t dst_stride,
                               int32_t damage[4], uint32_t* blocks, bool scroll = false, uint32_t* copied = nullptr) {
  if (!payload || bytes < WR_GC_HEADER || (bpp != 1 && bpp != 4) || rw < 1 || rh < 1 || (scroll && !packed)) return -1;
  const int32_t dy = (int32_t)wr_gc_load32((const uint8_t*)payload + 4);
  if (scroll ? dy < -WR_GC_SCROLL_MAX || dy > WR_GC_SCROLL_MAX : dy != 0) return -1;
  const int64_t tight = (int64_t)rw * bpp;
  if (dst && dst_stride != 0 && dst_stride < tight) return -1;
  const uint8_t* p = (const uint8_t*)payload;
  const uint64_t count = wr_gc_load32(p);
  if (count > bytes - WR_GC_HEADER) return -1;
  p += WR_GC_HEADER;
  int x0 = rw, y0 = rh, x1 = 0, y1 = 0;
  uint32_t n = 0;
  size_t ncopy = 0;
  WrGrabEntry E;
  for (size_t at = 0; at < count; at += E.size, n++) {
    if (!wr_gc_entry(p + at, (size_t)(count - at), bpp, packed, rw, rh, &E, false, scroll, dy)) return -1;
    if (E.mode == WR_GC_COPY) ncopy++;
    x0 = E.x < x0 ? E.x : x0; y0 = E.y < y0 ? E.y : y0;
    x1 = E.x + E.w > x1 ? E.x + E.w : x1; y1 = E.y + E.h > y1 ? E.y + E.h : y1;
  }
  const size_t ds = dst_stride ? (size_t)dst_stride : (size_t)tight;
  if (ncopy) {
    // (two COPY entries of one block are refused whether or not anything is patched)
    WrGrabCopy* copies = (WrGrabCopy*)malloc(ncopy * sizeof(WrGrabCopy));
    if (!copies) return -1;
    size_t k = 0;
    for (size_t at = 0; at < count; at += E.size) {
      wr_gc_entry(p + at, (size_t)(count - at), bpp, packed, rw, rh, &E, true, scroll, dy);
      if (E.mode == WR_GC_COPY) copies[k++] = WrGrabCopy{E.x, E.y, E.w, E.h};
    }
    if (!wr_gc_copy_order(copies, ncopy)) { free(copies); return -1; }
    if (dst) for (size_t i = 0; i < ncopy; i++) wr_gc_copy(copies[dy > 0 ? i : ncopy - 1 - i], dy, bpp, (uint8_t*)dst, ds);
    free(copies);
  }
  if (dst) {
    for (size_t at = 0; at < count; at += E.size) {
      wr_gc_entry(p + at, (size_t)(count - at), bpp, packed, rw, rh, &E, true, scroll, dy);
      if (E.mode != WR_GC_COPY) wr_gc_patch(p + at, E, bpp, (uint8_t*)dst, ds);
    }
  }
  if (copied) *copied = (uint32_t)ncopy;
  if (damage) {
    damage[0] = damage[1] = damage[2] = damage[3] = 0;
    if (x1 > x0 && y1 > y0) { damage[0] = x0; damage[1] = y0; damage[2] = x1 - x0; damage[3] = y1 - y0; }
  }
  if (blocks) *blocks = n;
  return 0;
}

// The index of a payload put (include/wrhip.h, WrhipPutTexturePayload): what wr_gc_decode's checking walk learns about a payload,
// kept for a decoder that gives every entry a worker of its own and so cannot find entry k by walking.  `words`, malloc'ed:
//   [0, n_patch)            the byte offset, from the payload's header on, of every entry that is no COPY, in payload order
//   [.., + n_cols + 1)      for every block column of the rect that has a COPY entry, where its blocks start among the n_copy below;
//                           the last word is n_copy
//   [.., + n_copy)          the COPY blocks, x / 64 | (y / 64) << 16, column by column and inside a column in the order the in-place
//                           rule applies them in: ascending y for dy > 0, descending for dy < 0.  (Block columns do not touch each
//                           other, so this order gives the bytes of wr_gc_decode's, which goes by y first.)
// -1 for everything wr_gc_decode refuses -- the same calls of wr_gc_entry and wr_gc_copy_order decide --, and for one thing more: two
// entries that are no COPY and share a pixel.  wr_gc_decode patches those in payload order; workers of their own have no order.  No
// grab emits such a payload.  Nothing is allocated then.
struct WrGcPutIndex {
  uint32_t n_patch, n_copy, n_cols;
  int32_t dy;
  uint32_t* words;
  size_t nwords;
};
static inline void wr_gc_put_index_free(WrGcPutIndex* I) { free(I->words); I->words = nullptr; I->nwords = 0; }
static inline int wr_gc_put_index(const void* payload, uint64_t bytes, int bpp, bool packed, bool scroll, int rw, int rh, WrGcPutIndex* I) {
  I->n_patch = I->n_copy = I->n_cols = 0; I->dy = 0; I->words = nullptr; I->nwords = 0;
  if (!payload || bytes < WR_GC_HEADER || (bpp != 1 && bpp != 4) || rw < 1 || rh < 1 || (scroll && !packed)) return -1;
  const int32_t dy = (int32_t)wr_gc_load32((const uint8_t*)payload + 4);
  if (scroll ? dy < -WR_GC_SCROLL_MAX || dy > WR_GC_SCROLL_MAX : dy != 0) return -1;
  const uint8_t* p = (const uint8_t*)payload;
  const uint64_t count = wr_gc_load32(p);
  if (count > bytes - WR_GC_HEADER) return -1;
  p += WR_GC_HEADER;
  size_t n = 0, ncopy = 0;
  WrGrabEntry E;
  for (size_t at = 0; at < count; at += E.size, n++) {
    if (!wr_gc_entry(p + at, (size_t)(count - at), bpp, packed, rw, rh, &E, false, scroll, dy)) return -1;
    if (E.mode == WR_GC_COPY) ncopy++;
  }
  const size_t npatch = n - ncopy;
  const size_t bxn = ((size_t)rw + WR_GC_BLOCK - 1) / WR_GC_BLOCK, byn = ((size_t)rh + WR_GC_BLOCK - 1) / WR_GC_BLOCK;
  // work memory: the COPY blocks; the other entries' blocks; per cell of the rect's 64 x 64 grid the list of entries that touch it
  // (a node per entry and cell: a block of at most 64 x 64 touches four); per block column its COPY blocks
  WrGrabCopy* copies = (WrGrabCopy*)malloc((ncopy + npatch + 1) * sizeof(WrGrabCopy));
  int32_t* cell = (int32_t*)malloc((bxn * byn + 4 * npatch + 1) * sizeof(int32_t));
  uint32_t* col = (uint32_t*)calloc(bxn + 1, sizeof(uint32_t));
  uint32_t* words = (uint32_t*)malloc((npatch + ncopy + bxn + 2) * sizeof(uint32_t));
  bool ok = copies && cell && col && words;
  if (ok) {
    WrGrabCopy* patches = copies + ncopy;
    int32_t* next = cell + bxn * byn;
    for (size_t i = 0; i < bxn * byn; i++) cell[i] = -1;
    size_t k = 0, q = 0;
    for (size_t at = 0; at < count && ok; at += E.size) {
      wr_gc_entry(p + at, (size_t)(count - at), bpp, packed, rw, rh, &E, true, scroll, dy);
      if (E.mode == WR_GC_COPY) { copies[k++] = WrGrabCopy{E.x, E.y, E.w, E.h}; continue; }
      const size_t cx0 = (size_t)E.x / WR_GC_BLOCK, cx1 = (size_t)(E.x + E.w - 1) / WR_GC_BLOCK;
      const size_t cy0 = (size_t)E.y / WR_GC_BLOCK, cy1 = (size_t)(E.y + E.h - 1) / WR_GC_BLOCK;
      int node = 4 * (int)q;
      for (size_t cy = cy0; cy <= cy1 && ok; cy++) {
        for (size_t cx = cx0; cx <= cx1 && ok; cx++, node++) {
          int32_t& head = cell[cy * bxn + cx];
          for (int32_t j = head; j >= 0 && ok; j = next[j]) {
            const WrGrabCopy& o = patches[j / 4];
            ok = !(o.x < E.x + E.w && E.x < o.x + o.w && o.y < E.y + E.h && E.y < o.y + o.h);
          }
          next[node] = head; head = node;
        }
      }
      patches[q] = WrGrabCopy{E.x, E.y, E.w, E.h};
      words[q++] = (uint32_t)(WR_GC_HEADER + at);
    }
    ok = ok && wr_gc_copy_order(copies, ncopy);
  }
  if (ok) {
    // the columns that have COPY blocks, in order; then the blocks, each to its column's next place
    for (size_t i = 0; i < ncopy; i++) col[(size_t)copies[i].x / WR_GC_BLOCK + 1]++;
    uint32_t* starts = words + npatch;
    size_t ncols = 0;
    uint32_t sum = 0;
    for (size_t cx = 0; cx < bxn; cx++) {
      const uint32_t c = col[cx + 1];
      col[cx + 1] = sum;             // (col[cx + 1]: where column cx's next block goes)
      if (c) { starts[ncols++] = sum; sum += c; }
    }
    starts[ncols] = sum;
    uint32_t* blocks = starts + ncols + 1;
    for (size_t i = 0; i < ncopy; i++) {
      const WrGrabCopy& C = copies[dy > 0 ? i : ncopy - 1 - i];
      blocks[col[(size_t)C.x / WR_GC_BLOCK + 1]++] = (uint32_t)(C.x / WR_GC_BLOCK) | (uint32_t)(C.y / WR_GC_BLOCK) << 16;
    }
    I->n_patch = (uint32_t)npatch; I->n_copy = (uint32_t)ncopy; I->n_cols = (uint32_t)ncols; I->dy = dy;
    I->words = words; I->nwords = npatch + (ncopy ? ncols + 1 + ncopy : 0);
    if (!ncopy) I->n_cols = 0;
  }
  free(copies); free(cell); free(col);
  if (!ok) free(words);
  return ok ? 0 : -1;
}

// The payload of a delta YUV grab (include/wrhip.h, WrhipGrabTextureYuvDelta; format 0: I420, 1: NV12, 2: I444): entries of one
// size, a record x, y, w, h -- a block of 64 x 64 luma samples of the image, aligned to its origin, cut to it -- and the block's
// planes at fixed pitches: Y, 64 rows of 64; then I420: Cb, Cr, 32 rows of 32 each; NV12: 32 rows of 32 pairs; I444: Cb, Cr, 64
// rows of 64 each.  A cut block of w x h has (w + 1) / 2 x (h + 1) / 2 chroma samples in 4:2:0; no byte beyond them is read.
static inline size_t wr_gc_yuv_entry_size(uint32_t format) {
  const size_t luma = (size_t)WR_GC_BLOCK * WR_GC_BLOCK;
  return 16 + (format == 2 ? 3 * luma : luma + luma / 2);
}
// the record at `p` against an image of rw x rh: false unless it names one of the image's blocks, cut as the image cuts it
static inline bool wr_gc_yuv_record(const uint8_t* p, int rw, int rh, WrGrabEntry* E) {
  const uint32_t x = wr_gc_load32(p), y = wr_gc_load32(p + 4), w = wr_gc_load32(p + 8), h = wr_gc_load32(p + 12);
  if (x % WR_GC_BLOCK || y % WR_GC_BLOCK || x >= (uint32_t)rw || y >= (uint32_t)rh) return false;
  const uint32_t bw = (uint32_t)rw - x < WR_GC_BLOCK ? (uint32_t)rw - x : WR_GC_BLOCK, bh = (uint32_t)rh - y < WR_GC_BLOCK ? (uint32_t)rh - y : WR_GC_BLOCK;
  if (w != bw || h != bh) return false;
  E->x = (int32_t)x; E->y = (int32_t)y; E->w = (int32_t)w; E->h = (int32_t)h; E->mode = WR_GC_RAW; E->aux = 0; E->size = 16;
  return true;
}
// a checked entry's samples into the caller's planes: Y rows of `ys` bytes, chroma rows of `cs` (NV12: c0 is the plane of pairs)
static inline void wr_gc_yuv_patch(const uint8_t* p, const WrGrabEntry& E, uint32_t format, uint8_t* y, size_t ys, uint8_t* c0, uint8_t* c1, size_t cs) {
  const size_t B = WR_GC_BLOCK;
  const uint8_t* body = p + 16;
  for (int r = 0; r < E.h; r++) memcpy(y + (size_t)(E.y + r) * ys + (size_t)E.x, body + (size_t)r * B, (size_t)E.w);
  body += B * B;
  if (format == 2) {
    for (int r = 0; r < E.h; r++) {
      memcpy(c0 + (size_t)(E.y + r) * cs + (size_t)E.x, body + (size_t)r * B, (size_t)E.w);
      memcpy(c1 + (size_t)(E.y + r) * cs + (size_t)E.x, body + B * B + (size_t)r * B, (size_t)E.w);
    }
    return;
  }
  const int cw = (E.w + 1) / 2, ch = (E.h + 1) / 2;
  for (int r = 0; r < ch; r++) {
    if (format == 1) {
      memcpy(c0 + (size_t)(E.y / 2 + r) * cs + (size_t)E.x, body + (size_t)r * B, (size_t)2 * cw);
    } else {
      memcpy(c0 + (size_t)(E.y / 2 + r) * cs + (size_t)(E.x / 2), body + (size_t)r * (B / 2), (size_t)cw);
      memcpy(c1 + (size_t)(E.y / 2 + r) * cs + (size_t)(E.x / 2), body + B * B / 4 + (size_t)r * (B / 2), (size_t)cw);
    }
  }
}
// The payload of a scroll-aware delta YUV grab (WrhipGrabTextureYuvDelta with WRHIP_GRAB_SCROLL): header word 1 is dy, the scroll
// vector (int32, |dy| <= 512), and every record is x, y, w | h << 8 | mode << 16, 0 -- the packed payload's record layout.
//   SAMPLES 0  the record, then the block's planes as a delta YUV entry lays them out: wr_gc_yuv_entry_size(format) bytes
//   COPY    3  the record alone: the block takes, in every plane, the samples the planes had BEFORE the decode dy luma rows further
//              down -- chroma rows dy / 2 further down in 4:2:0, where dy is even.  dy is not 0 then, and the source rows lie
//              inside the image.
// The decode is in place: the COPY entries first, by ascending y for dy > 0 and descending y for dy < 0, then the SAMPLES entries.
// the record at `p` (avail bytes of the payload from it on) against an image of rw x rh and the vector dy: false unless it is one
// the format allows; E->size: the whole entry's
static inline bool wr_gc_yuv_scroll_record(const uint8_t* p, size_t avail, uint32_t format, int rw, int rh, int32_t dy, WrGrabEntry* E) {
  if (avail < 16) return false;
  const uint32_t x = wr_gc_load32(p), y = wr_gc_load32(p + 4), w2 = wr_gc_load32(p + 8), w3 = wr_gc_load32(p + 12);
  const uint32_t w = w2 & 0xFFu, h = (w2 >> 8) & 0xFFu, mode = w2 >> 16;
  if ((mode != WR_GC_RAW && mode != WR_GC_COPY) || w3 != 0) return false;
  if (x % WR_GC_BLOCK || y % WR_GC_BLOCK || x >= (uint32_t)rw || y >= (uint32_t)rh) return false;
  const uint32_t bw = (uint32_t)rw - x < WR_GC_BLOCK ? (uint32_t)rw - x : WR_GC_BLOCK, bh = (uint32_t)rh - y < WR_GC_BLOCK ? (uint32_t)rh - y : WR_GC_BLOCK;
  if (w != bw || h != bh) return false;
  E->x = (int32_t)x; E->y = (int32_t)y; E->w = (int32_t)w; E->h = (int32_t)h; E->mode = (int32_t)mode; E->aux = 0;
  if (mode == WR_GC_COPY) {
    if (dy == 0 || dy < -WR_GC_SCROLL_MAX || dy > WR_GC_SCROLL_MAX || (format != 2 && (dy & 1))) return false;
    const int64_t sy = (int64_t)y + dy;
    if (sy < 0 || sy + (int64_t)h > (int64_t)rh) return false;
    E->size = 16;
    return true;
  }
  E->size = wr_gc_yuv_entry_size(format);
  return E->size <= avail;
}
// one COPY entry in place, all planes: each plane's rows in the order in which a row's source has not been written yet
static inline void wr_gc_yuv_copy(const WrGrabCopy& E, int32_t dy, uint32_t format, uint8_t* y, size_t ys, uint8_t* c0, uint8_t* c1, size_t cs) {
  wr_gc_copy(E, dy, 1, y, ys);
  if (format == 2) { wr_gc_copy(E, dy, 1, c0, cs); wr_gc_copy(E, dy, 1, c1, cs); return; }
  // (4:2:0: the block's chroma samples, (w + 1) / 2 x (h + 1) / 2 of them from (x / 2, y / 2) on, move by dy / 2 rows)
  const WrGrabCopy C = {E.x / 2, E.y / 2, (E.w + 1) / 2, (E.h + 1) / 2};
  if (format == 1) wr_gc_copy(C, dy / 2, 2, c0, cs);
  else { wr_gc_copy(C, dy / 2, 1, c0, cs); wr_gc_copy(C, dy / 2, 1, c1, cs); }
}
// the record of a scroll payload's entry (mode: WR_GC_RAW for SAMPLES, WR_GC_COPY), written to `out`
static inline void wr_gc_yuv_encode_record(int x, int y, int w, int h, int mode, uint8_t* out) {
  wr_gc_store32(out, (uint32_t)x); wr_gc_store32(out + 4, (uint32_t)y);
  wr_gc_store32(out + 8, (uint32_t)w | (uint32_t)h << 8 | (uint32_t)mode << 16); wr_gc_store32(out + 12, 0u);
}
// A whole scroll payload checked and patched: wr_gc_decode_yuv's second half (its arguments checked there).  A block named twice is
// refused, and nothing is written before every entry has been checked.
static inline int wr_gc_decode_yuv_scroll(const uint8_t* p, uint64_t count, uint32_t format, int rw, int rh, uint8_t* y, size_t ys,
                                          uint8_t* c0, uint8_t* c1, size_t cs, int32_t dy, int32_t damage[4], uint32_t* blocks, uint32_t* copied) {
  if (dy < -WR_GC_SCROLL_MAX || dy > WR_GC_SCROLL_MAX) return -1;
  const size_t bx = (size_t)(rw + WR_GC_BLOCK - 1) / WR_GC_BLOCK, by = (size_t)(rh + WR_GC_BLOCK - 1) / WR_GC_BLOCK;
  uint8_t* seen = (uint8_t*)calloc(bx * by, 1);
  if (!seen) return -1;
  int x0 = rw, y0 = rh, x1 = 0, y1 = 0;
  uint32_t n = 0;
  size_t ncopy = 0;
  WrGrabEntry E;
  for (uint64_t at = 0; at < count; at += E.size, n++) {
    if (!wr_gc_yuv_scroll_record(p + at, (size_t)(count - at), format, rw, rh, dy, &E)) { free(seen); return -1; }
    uint8_t& s = seen[(size_t)(E.y / WR_GC_BLOCK) * bx + (size_t)(E.x / WR_GC_BLOCK)];
    if (s) { free(seen); return -1; }
    s = 1;
    if (E.mode == WR_GC_COPY) ncopy++;
    x0 = E.x < x0 ? E.x : x0; y0 = E.y < y0 ? E.y : y0;
    x1 = E.x + E.w > x1 ? E.x + E.w : x1; y1 = E.y + E.h > y1 ? E.y + E.h : y1;
  }
  free(seen);
  if (y && ncopy) {
    WrGrabCopy* copies = (WrGrabCopy*)malloc(ncopy * sizeof(WrGrabCopy));
    if (!copies) return -1;
    size_t k = 0;
    for (uint64_t at = 0; at < count; at += E.size) {
      wr_gc_yuv_scroll_record(p + at, (size_t)(count - at), format, rw, rh, dy, &E);
      if (E.mode == WR_GC_COPY) copies[k++] = WrGrabCopy{E.x, E.y, E.w, E.h};
    }
    wr_gc_copy_order(copies, ncopy);
    for (size_t i = 0; i < ncopy; i++) wr_gc_yuv_copy(copies[dy > 0 ? i : ncopy - 1 - i], dy, format, y, ys, c0, c1, cs);
    free(copies);
  }
  if (y) {
    for (uint64_t at = 0; at < count; at += E.size) {
      wr_gc_yuv_scroll_record(p + at, (size_t)(count - at), format, rw, rh, dy, &E);
      if (E.mode != WR_GC_COPY) wr_gc_yuv_patch(p + at, E, format, y, ys, c0, c1, cs);
    }
  }
  if (copied) *copied = (uint32_t)ncopy;
  if (damage) {
    damage[0] = damage[1] = damage[2] = damage[3] = 0;
    if (x1 > x0 && y1 > y0) { damage[0] = x0; damage[1] = y0; damage[2] = x1 - x0; damage[3] = y1 - y0; }
  }
  if (blocks) *blocks = n;
  return 0;
}
// A whole payload patched into the caller's planes (byte strides, 0: tight; NV12: c0 the pairs, c1 NULL; y, c0 and c1 all NULL:
// only checked): 0, with the bounding box of the entries' blocks and their number, or -1 for a malformed one -- a count that is
// not k entries or more than the caller holds, a record that is not a block of the image, more entries than blocks, a non-zero
// header word 1 -- or for planes given in part or with a stride below a row; nothing is written then.
// scroll: a scroll grab's payload (above); `copied`: its COPY entries.
static inline int wr_gc_decode_yuv(const void* payload, uint64_t bytes, uint32_t format, int rw, int rh, void* y, int64_t y_stride,
                                   void* c0, void* c1, int64_t c_stride, int32_t damage[4], uint32_t* blocks, bool scroll = false,
                                   uint32_t* copied = nullptr) {
  if (!payload || bytes < WR_GC_HEADER || format > 2 || rw < 1 || rh < 1) return -1;
  const int64_t c_row = format == 2 ? rw : format == 1 ? 2 * (((int64_t)rw + 1) / 2) : ((int64_t)rw + 1) / 2;
  const bool patch = y || c0 || c1;
  if (patch && (!y || !c0 || (format == 1 ? c1 != nullptr : c1 == nullptr))) return -1;
  if (patch && ((y_stride != 0 && y_stride < rw) || (c_stride != 0 && c_stride < c_row))) return -1;
  const int32_t dy = (int32_t)wr_gc_load32((const uint8_t*)payload + 4);
  if (!scroll && dy != 0) return -1;
  if (copied) *copied = 0;
  if (scroll) {
    const uint64_t n = wr_gc_load32((const uint8_t*)payload);
    if (n > bytes - WR_GC_HEADER) return -1;
    return wr_gc_decode_yuv_scroll((const uint8_t*)payload + WR_GC_HEADER, n, format, rw, rh, (uint8_t*)y, y_stride ? (size_t)y_stride : (size_t)rw,
                                   (uint8_t*)c0, (uint8_t*)c1, c_stride ? (size_t)c_stride : (size_t)c_row, dy, damage, blocks, copied);
  }
  const uint8_t* p = (const uint8_t*)payload;
  const uint64_t count = wr_gc_load32(p), entry = wr_gc_yuv_entry_size(format);
  const uint64_t total = (uint64_t)((rw + WR_GC_BLOCK - 1) / WR_GC_BLOCK) * (uint64_t)((rh + WR_GC_BLOCK - 1) / WR_GC_BLOCK);
  if (count > bytes - WR_GC_HEADER || count % entry != 0 || count / entry > total) return -1;
  p += WR_GC_HEADER;
  int x0 = rw, y0 = rh, x1 = 0, y1 = 0;
  WrGrabEntry E;
  for (uint64_t at = 0; at < count; at += entry) {
    if (!wr_gc_yuv_record(p + at, rw, rh, &E)) return -1;
    x0 = E.x < x0 ? E.x : x0; y0 = E.y < y0 ? E.y : y0;
    x1 = E.x + E.w > x1 ? E.x + E.w : x1; y1 = E.y + E.h > y1 ? E.y + E.h : y1;
  }
  if (patch) {
    const size_t ys = y_stride ? (size_t)y_stride : (size_t)rw, cs = c_stride ? (size_t)c_stride : (size_t)c_row;
    for (uint64_t at = 0; at < count; at += entry) {
      wr_gc_yuv_record(p + at, rw, rh, &E);
      wr_gc_yuv_patch(p + at, E, format, (uint8_t*)y, ys, (uint8_t*)c0, (uint8_t*)c1, cs);
    }
  }
  if (damage) {
    damage[0] = damage[1] = damage[2] = damage[3] = 0;
    if (x1 > x0 && y1 > y0) { damage[0] = x0; damage[1] = y0; damage[2] = x1 - x0; damage[3] = y1 - y0; }
  }
  if (blocks) *blocks = (uint32_t)(count / entry);
  return 0;
}

// The packed entry of one cut block (w x h pixels at `px`, rows of `stride` bytes) at (x, y) of the rect, written to `out` (room
// for wr_gc_raw_size(bpp) bytes): -> its size.  Serial; the device's kernel (wr_grab_pack_runs_kernel) writes the same bytes.
static inline size_t wr_gc_encode_block(const uint8_t* px, size_t stride, int x, int y, int w, int h, int bpp, uint8_t* out) {
  uint32_t n = 0;
  uint64_t bitmap[WR_GC_BLOCK];
  const uint8_t* prev = nullptr;
  for (int r = 0; r < h; r++) {
    bitmap[r] = 0;
    for (int c = 0; c < w; c++) {
      const uint8_t* q = px + (size_t)r * stride + (size_t)c * bpp;
      if (!prev || memcmp(q, prev, (size_t)bpp) != 0) { bitmap[r] |= 1ull << c; n++; }
      prev = q;
    }
  }
  const int mode = wr_gc_mode(h, n, bpp);
  uint32_t aux = 0;
  if (mode == WR_GC_SOLID) { uint8_t v[4] = {0, 0, 0, 0}; memcpy(v, px, (size_t)bpp); aux = wr_gc_load32(v); }
  if (mode == WR_GC_RUNS) aux = n;
  wr_gc_store32(out, (uint32_t)x); wr_gc_store32(out + 4, (uint32_t)y);
  wr_gc_store32(out + 8, (uint32_t)w | (uint32_t)h << 8 | (uint32_t)mode << 16); wr_gc_store32(out + 12, aux);
  if (mode == WR_GC_SOLID) return 16;
  if (mode == WR_GC_RAW) {
    const size_t pitch = (size_t)WR_GC_BLOCK * bpp;
    memset(out + 16, 0, pitch * WR_GC_BLOCK);
    for (int r = 0; r < h; r++) memcpy(out + 16 + (size_t)r * pitch, px + (size_t)r * stride, (size_t)w * bpp);
    return wr_gc_raw_size(bpp);
  }
  const size_t size = wr_gc_runs_size(h, n, bpp);
  memset(out + 16, 0, size - 16);
  uint8_t* lit = out + 16 + 8 * (size_t)h;
  for (int r = 0; r < h; r++) {
    wr_gc_store32(out + 16 + 8 * (size_t)r, (uint32_t)bitmap[r]); wr_gc_store32(out + 20 + 8 * (size_t)r, (uint32_t)(bitmap[r] >> 32));
    for (int c = 0; c < w; c++)
      if ((bitmap[r] >> c) & 1ull) { memcpy(lit, px + (size_t)r * stride + (size_t)c * bpp, (size_t)bpp); lit += bpp; }
  }
  return size;
}
// The COPY entry of a cut block at (x, y) of the rect (a scroll grab's payload), written to `out`: -> its size
static inline size_t wr_gc_encode_copy(int x, int y, int w, int h, uint8_t* out) {
  wr_gc_store32(out, (uint32_t)x); wr_gc_store32(out + 4, (uint32_t)y);
  wr_gc_store32(out + 8, (uint32_t)w | (uint32_t)h << 8 | (uint32_t)WR_GC_COPY << 16); wr_gc_store32(out + 12, 0u);
  return 16;
}
#endif
