// The index builder of a payload put (webrender_amd/csrc/wr_grab_codec.h, wr_gc_put_index, included alone) on good, shuffled,
// truncated and inconsistent payloads.  Meant to be built with -fsanitize=address,undefined (tests/test_put_payload.py does): every
// payload lives in a heap block of exactly its size, so that a read beyond it is reported, and an index that is refused must not
// leak (LeakSanitizer reports at exit).
//   g++ -std=c++17 -g -fsanitize=address,undefined -I webrender_amd/csrc tools/put_payload_check.cpp -o put_payload_check
// Exit status 0 and "put_payload_check: ok" if every case behaved; otherwise the failed cases are named and the status is 1.
// A good payload's index is checked by applying it: the entries it lists, in its order, patched with the decoder's own functions
// into an image must give wr_gc_decode's image.
#include "wr_grab_codec.h"
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

static int failures = 0;
static void check(bool ok, const char* what) {
  if (!ok) { printf("FAILED: %s\n", what); failures++; }
}
typedef std::vector<uint8_t> Bytes;
static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static Bytes payload_of(const std::vector<Bytes>& entries, int32_t dy = 0) {
  Bytes p(WR_GC_HEADER, 0);
  for (const Bytes& e : entries) p.insert(p.end(), e.begin(), e.end());
  wr_gc_store32(p.data(), (uint32_t)(p.size() - WR_GC_HEADER));
  wr_gc_store32(p.data() + 4, (uint32_t)dy);
  return p;
}
// the index of `p`, built from a heap block of exactly `held` bytes of it
static int index_of(const Bytes& p, size_t held, uint64_t bytes, int bpp, bool packed, bool scroll, int rw, int rh, WrGcPutIndex* I) {
  uint8_t* src = (uint8_t*)malloc(held ? held : 1);
  memcpy(src, p.data(), held);
  const int rc = wr_gc_put_index(src, bytes, bpp, packed, scroll, rw, rh, I);
  free(src);
  return rc;
}
static void refused(const Bytes& p, uint64_t bytes, int bpp, bool packed, bool scroll, int rw, int rh, const char* what) {
  WrGcPutIndex I;
  const int rc = index_of(p, p.size(), bytes, bpp, packed, scroll, rw, rh, &I);
  check(rc == -1 && I.words == nullptr && I.nwords == 0, what);
  // whatever the index refuses for the decoder's reasons, the decoder refuses
  if (rc == 0) wr_gc_put_index_free(&I);
}
// A good payload: the index applied -- COPY blocks column by column in the listed order, then the listed entries -- against wr_gc_decode
static void applied(const Bytes& p, int bpp, bool packed, bool scroll, int rw, int rh, uint32_t seed, const char* what) {
  const size_t n = (size_t)rw * rh * bpp;
  Bytes a(n), b;
  for (size_t i = 0; i < n; i++) a[i] = (uint8_t)rnd(seed);
  b = a;
  int32_t damage[4];
  uint32_t blocks = 0, copied = 0;
  const int rd = wr_gc_decode(p.data(), p.size(), bpp, packed, rw, rh, a.data(), 0, damage, &blocks, scroll, &copied);
  WrGcPutIndex I;
  const int ri = index_of(p, p.size(), p.size(), bpp, packed, scroll, rw, rh, &I);
  check(rd == 0 && ri == 0, what);
  if (ri != 0) return;
  check(I.n_patch + I.n_copy == blocks && I.n_copy == copied, "the index counts the decoder's entries");
  check(I.nwords == I.n_patch + (I.n_copy ? I.n_cols + 1 + I.n_copy : 0) && I.nwords * 4 <= 16 * (size_t)blocks, "the index is 16 bytes per entry at most");
  const uint32_t* starts = I.words + I.n_patch;
  const uint32_t* cb = starts + I.n_cols + 1;
  bool ordered = I.n_copy == 0 || (starts[0] == 0 && starts[I.n_cols] == I.n_copy);
  for (uint32_t c = 0; c < I.n_cols && ordered; c++) {
    ordered = starts[c] < starts[c + 1];
    for (uint32_t k = starts[c]; k < starts[c + 1]; k++) {
      const int x = (int)(cb[k] & 0xFFFFu) * WR_GC_BLOCK, y = (int)(cb[k] >> 16) * WR_GC_BLOCK;
      ordered = ordered && (cb[k] & 0xFFFFu) == (cb[starts[c]] & 0xFFFFu) && x < rw && y < rh;
      if (!ordered) break;
      const WrGrabCopy C = {x, y, rw - x < WR_GC_BLOCK ? rw - x : WR_GC_BLOCK, rh - y < WR_GC_BLOCK ? rh - y : WR_GC_BLOCK};
      wr_gc_copy(C, I.dy, bpp, b.data(), (size_t)rw * bpp);
    }
  }
  check(ordered, "the column table is in order and every COPY block lies in its column");
  for (uint32_t k = 0; k < I.n_patch; k++) {
    WrGrabEntry E;
    const uint32_t off = I.words[k];
    const bool ok = off >= WR_GC_HEADER && off < p.size() && wr_gc_entry(p.data() + off, p.size() - off, bpp, packed, rw, rh, &E, true) && E.mode != WR_GC_COPY;
    check(ok, "a listed offset is an entry that is no COPY");
    if (ok) wr_gc_patch(p.data() + off, E, bpp, b.data(), (size_t)rw * bpp);
  }
  check(a == b, what);
  wr_gc_put_index_free(&I);
}

// every block of a w x h image, packed; flat, striped and noise blocks
static std::vector<Bytes> packed_entries(const Bytes& img, int w, int h, int bpp) {
  std::vector<Bytes> out;
  for (int y = 0; y < h; y += WR_GC_BLOCK)
    for (int x = 0; x < w; x += WR_GC_BLOCK) {
      const int bw = w - x < WR_GC_BLOCK ? w - x : WR_GC_BLOCK, bh = h - y < WR_GC_BLOCK ? h - y : WR_GC_BLOCK;
      Bytes e(wr_gc_raw_size(bpp));
      e.resize(wr_gc_encode_block(img.data() + ((size_t)y * w + x) * bpp, (size_t)w * bpp, x, y, bw, bh, bpp, e.data()));
      out.push_back(e);
    }
  return out;
}
static Bytes test_image(int w, int h, int bpp, uint32_t seed) {
  Bytes img((size_t)w * h * bpp);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const int kind = (x / WR_GC_BLOCK + 2 * (y / WR_GC_BLOCK)) % 3;
      for (int k = 0; k < bpp; k++)
        img[((size_t)y * w + x) * bpp + k] = kind == 0 ? (uint8_t)(17 + k) : kind == 1 ? (uint8_t)((x / 7) * 31 + y / 5 + k) : (uint8_t)rnd(seed);
    }
  return img;
}
static Bytes plain_entry(const Bytes& img, int w, int bpp, int x, int y, int bw, int bh) {
  Bytes q(wr_gc_raw_size(bpp), 0);
  wr_gc_store32(q.data(), (uint32_t)x); wr_gc_store32(q.data() + 4, (uint32_t)y); wr_gc_store32(q.data() + 8, (uint32_t)bw); wr_gc_store32(q.data() + 12, (uint32_t)bh);
  for (int r = 0; r < bh; r++) memcpy(q.data() + 16 + (size_t)r * WR_GC_BLOCK * bpp, img.data() + ((size_t)(y + r) * w + x) * bpp, (size_t)bw * bpp);
  return q;
}
static Bytes copy_entry(int x, int y, int rw, int rh) {
  Bytes e(16);
  wr_gc_encode_copy(x, y, rw - x < WR_GC_BLOCK ? rw - x : WR_GC_BLOCK, rh - y < WR_GC_BLOCK ? rh - y : WR_GC_BLOCK, e.data());
  return e;
}

int main() {
  for (int bpp = 1; bpp <= 4; bpp += 3) {
    const int w = 200, h = 330;
    const Bytes img = test_image(w, h, bpp, 77u + (uint32_t)bpp);
    std::vector<Bytes> packed = packed_entries(img, w, h, bpp);
    const std::vector<Bytes> grid = packed;
    applied(payload_of(packed), bpp, true, false, w, h, 1, "a packed payload in the grab's order");
    uint32_t s = 5;
    for (int round = 0; round < 3; round++) {
      for (size_t i = packed.size() - 1; i > 0; i--) std::swap(packed[i], packed[rnd(s) % (i + 1)]);
      applied(payload_of(packed), bpp, true, false, w, h, 2 + (uint32_t)round, "a packed payload shuffled");
    }
    std::vector<Bytes> plain;
    for (int y = 0; y < h; y += WR_GC_BLOCK)
      for (int x = 0; x < w; x += WR_GC_BLOCK) plain.push_back(plain_entry(img, w, bpp, x, y, std::min(WR_GC_BLOCK, w - x), std::min(WR_GC_BLOCK, h - y)));
    std::reverse(plain.begin(), plain.end());
    applied(payload_of(plain), bpp, false, false, w, h, 9, "a plain payload reversed");
    applied(payload_of({}), bpp, true, false, w, h, 10, "a payload of no entry");
    applied(payload_of({}), bpp, false, false, 1, 1, 10, "a payload of no entry for a rect of one pixel");
    // plain entries that are no blocks of the grid and touch without sharing a pixel
    applied(payload_of({plain_entry(img, w, bpp, 3, 5, 64, 64), plain_entry(img, w, bpp, 67, 5, 30, 64), plain_entry(img, w, bpp, 3, 69, 64, 1)}), bpp, false, false, w, h, 11,
            "plain entries off the grid that touch");
    // scroll payloads: COPY entries of both signs, |dy| below and above a block, every order; the rest of the blocks packed
    const int dys[8] = {1, 7, 63, 64, 65, -1, -37, -300};
    for (int d = 0; d < 8; d++) {
      const int dy = dys[d];
      std::vector<Bytes> ent;
      int k = 0;
      for (int y = 0; y < h; y += WR_GC_BLOCK)
        for (int x = 0; x < w; x += WR_GC_BLOCK, k++) {
          const int bh = std::min(WR_GC_BLOCK, h - y);
          const bool fits = y + dy >= 0 && y + dy + bh <= h;
          if (fits && k % 5 != 0) ent.push_back(copy_entry(x, y, w, h));
          else if (k % 3 != 0) ent.push_back(grid[(size_t)k]);
        }
      for (int round = 0; round < 3; round++) {
        applied(payload_of(ent, dy), bpp, true, true, w, h, 20 + (uint32_t)d, "a scroll payload");
        for (size_t i = ent.size() - 1; i > 0; i--) std::swap(ent[i], ent[rnd(s) % (i + 1)]);
      }
      // the same block named by two COPY entries; by a COPY and another entry (allowed: the COPY goes first)
      std::vector<Bytes> twice = ent;
      twice.push_back(copy_entry(0, 64, w, h));
      twice.push_back(copy_entry(0, 64, w, h));
      refused(payload_of(twice, dy), payload_of(twice, dy).size(), bpp, true, true, w, h, "a block named by two COPY entries");
    }
    applied(payload_of({copy_entry(0, 64, w, h), grid[4]}, 7), bpp, true, true, w, h, 30, "a COPY entry and a packed entry of one block");
    // inconsistent: what wr_gc_decode refuses, and two entries that are no COPY and share a pixel
    Bytes good = payload_of({grid[0], grid[1]});
    refused(good, 15, bpp, true, false, w, h, "fewer bytes than a header");
    refused(good, good.size() - 1, bpp, true, false, w, h, "fewer bytes than the header says");
    { Bytes cut(good.begin(), good.begin() + 16 + 8); wr_gc_store32(cut.data(), 8); refused(cut, cut.size(), bpp, true, false, w, h, "truncated inside a record"); }
    refused(payload_of({grid[0]}, 3), 16 + grid[0].size(), bpp, true, false, w, h, "a dy in a payload that is no scroll grab's");
    refused(payload_of({grid[0]}, 513), 16 + grid[0].size(), bpp, true, true, w, h, "|dy| above 512");
    refused(payload_of({copy_entry(0, 0, w, h)}, 0), 32, bpp, true, true, w, h, "a COPY entry with dy 0");
    refused(payload_of({copy_entry(0, 0, w, h)}, -1), 32, bpp, true, true, w, h, "a COPY source above the rect");
    refused(payload_of({copy_entry(0, 320, w, h)}, 1), 32, bpp, true, true, w, h, "a COPY source below the rect");
    refused(payload_of({copy_entry(0, 0, w, h)}, 7), 32, bpp, true, false, w, h, "mode 3 without SCROLL");
    refused(payload_of({copy_entry(0, 0, w, h)}, 7), 32, bpp, false, true, w, h, "SCROLL without PACKED");
    { Bytes m = copy_entry(0, 0, w, h); wr_gc_store32(m.data(), 1); refused(payload_of({m}, 7), 32, bpp, true, true, w, h, "a COPY block off the grid"); }
    { Bytes m = copy_entry(0, 0, w, h); wr_gc_store32(m.data() + 8, 63u | 64u << 8 | 3u << 16); refused(payload_of({m}, 7), 32, bpp, true, true, w, h, "a COPY block that is not whole"); }
    refused(payload_of({grid[0], grid[0]}), 16 + 2 * grid[0].size(), bpp, true, false, w, h, "a block named by two entries that are no COPY");
    refused(payload_of({plain_entry(img, w, bpp, 3, 5, 64, 64), plain_entry(img, w, bpp, 66, 68, 10, 10)}), 16 + 2 * wr_gc_raw_size(bpp), bpp, false, false, w, h,
            "two plain entries off the grid that share one pixel");
    for (size_t i = 0; i < grid.size(); i++) {
      // a RUNS entry spoilt: n against the popcount, a bit at a column >= w (the block at the right edge is 8 wide)
      Bytes m = grid[i];
      if ((wr_gc_load32(m.data() + 8) >> 16) != WR_GC_RUNS) continue;
      wr_gc_store32(m.data() + 12, wr_gc_load32(m.data() + 12) + 1);
      refused(payload_of({m}), 16 + m.size(), bpp, true, false, w, h, "n larger than the bitmap's popcount");
      m = grid[i];
      if ((wr_gc_load32(m.data() + 8) & 0xFFu) < 64u) { m[16 + 7] |= 0x80u; refused(payload_of({m}), 16 + m.size(), bpp, true, false, w, h, "a bitmap bit at a column >= w"); }
    }
    refused(good, good.size(), 2, true, false, w, h, "two bytes per pixel");
    refused(good, good.size(), bpp, true, false, 0, h, "an empty rect");
    WrGcPutIndex I;
    check(wr_gc_put_index(nullptr, 64, bpp, true, false, w, h, &I) == -1 && !I.words, "no payload");
  }
  if (failures) return 1;
  printf("put_payload_check: ok\n");
  return 0;
}
