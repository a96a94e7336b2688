// The host decoder of scroll-grab payloads (webrender_amd/csrc/wr_grab_codec.h, included alone; the contract: include/wrhip.h,
// WRHIP_GRAB_SCROLL) on hostile input and on COPY entries in the adverse order.  Meant to be built with
// -fsanitize=address,undefined (tests/test_grab_scroll.py does): every payload lives in a heap block of exactly its size and the
// image in one of exactly its size, so that a read or a write beyond either is reported.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I webrender_amd/csrc tools/grab_scroll_check.cpp -o grab_scroll_check
// Exit status 0 and "grab_scroll_check: ok" if every case behaved; otherwise the failed cases are named and the status is 1.
#include "wr_grab_codec.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int failures = 0;
static void check(bool ok, const char* what) {
  if (!ok) { printf("FAILED: %s\n", what); failures++; }
}

typedef std::vector<uint8_t> Bytes;

static Bytes record(uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t mode, uint32_t aux) {
  Bytes e(16);
  wr_gc_store32(e.data(), x); wr_gc_store32(e.data() + 4, y); wr_gc_store32(e.data() + 8, w | h << 8 | mode << 16); wr_gc_store32(e.data() + 12, aux);
  return e;
}
// header (word 0: the entries' bytes, word 1: dy) + entries
static Bytes payload_of(int32_t dy, const std::vector<Bytes>& entries) {
  Bytes p(WR_GC_HEADER, 0);
  for (const Bytes& e : entries) p.insert(p.end(), e.begin(), e.end());
  wr_gc_store32(p.data(), (uint32_t)(p.size() - WR_GC_HEADER));
  wr_gc_store32(p.data() + 4, (uint32_t)dy);
  return p;
}
static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static Bytes noise(int w, int h, int bpp, uint32_t seed) {
  Bytes img((size_t)w * h * bpp);
  for (uint8_t& b : img) b = (uint8_t)rnd(seed);
  return img;
}
// decode `bytes` of `p` (in a heap block of its own size) into a copy of `image` (a heap block of its size): the result and the image
static int decode(const Bytes& p, uint64_t bytes, int bpp, bool scroll, int rw, int rh, const Bytes& image, Bytes* out, uint32_t* blocks = nullptr, uint32_t* copied = nullptr) {
  uint8_t* src = (uint8_t*)malloc(p.size() ? p.size() : 1);
  if (!p.empty()) memcpy(src, p.data(), p.size());
  uint8_t* img = (uint8_t*)malloc(image.size());
  memcpy(img, image.data(), image.size());
  int32_t damage[4];
  const int rc = wr_gc_decode(src, bytes, bpp, true, rw, rh, img, 0, damage, blocks, scroll, copied);
  out->assign(img, img + image.size());
  free(img);
  free(src);
  return rc;
}
static void refused(const Bytes& p, uint64_t bytes, int bpp, bool scroll, int rw, int rh, const char* what) {
  const Bytes image = noise(rw, rh, bpp, 99);
  Bytes out;
  const int rc = decode(p, bytes, bpp, scroll, rw, rh, image, &out);
  check(rc == -1 && out == image, what);
}

int main() {
  for (int bpp = 1; bpp <= 4; bpp += 3) {
    const int rw = 130, rh = 200;            // 3 x 4 blocks; the last column 2 wide, the last row 8 high
    const Bytes solid = record(64, 64, 64, 64, WR_GC_SOLID, 7);
    // ---- malformed payloads: -1, nothing written
    refused(payload_of(0, {record(0, 0, 64, 64, WR_GC_COPY, 0)}), 32, bpp, true, rw, rh, "a COPY entry with dy == 0");
    refused(payload_of(513, {solid}), 32, bpp, true, rw, rh, "dy above the bound");
    refused(payload_of(-513, {solid}), 32, bpp, true, rw, rh, "dy below the bound");
    refused(payload_of((int32_t)0x80000000u, {record(0, 64, 64, 64, WR_GC_COPY, 0)}), 32, bpp, true, rw, rh, "the most negative dy");
    refused(payload_of(5, {record(0, 128, 64, 64, WR_GC_COPY, 0), record(0, 192, 64, 8, WR_GC_COPY, 0)}), 48, bpp, true, rw, rh, "a COPY source below the rect");
    refused(payload_of(-5, {solid, record(64, 0, 64, 64, WR_GC_COPY, 0)}), 48, bpp, true, rw, rh, "a COPY source above the rect");
    refused(payload_of(137, {record(0, 0, 64, 64, WR_GC_COPY, 0)}), 32, bpp, true, rw, rh, "a COPY source that ends one row below the rect");
    refused(payload_of(3, {record(0, 0, 64, 64, WR_GC_COPY, 1)}), 32, bpp, true, rw, rh, "a COPY record with a non-zero aux");
    refused(payload_of(3, {record(0, 0, 64, 64, WR_GC_COPY, 0)}), 32, bpp, false, rw, rh, "mode 3 without SCROLL");
    refused(payload_of(3, {solid}), 32, bpp, false, rw, rh, "a non-zero header word 1 without SCROLL");
    refused(payload_of(3, {record(0, 0, 64, 64, 4, 0)}), 32, bpp, true, rw, rh, "mode 4");
    refused(payload_of(3, {record(1, 0, 64, 64, WR_GC_COPY, 0)}), 32, bpp, true, rw, rh, "a COPY entry that is not on the block grid");
    refused(payload_of(3, {record(0, 0, 63, 64, WR_GC_COPY, 0)}), 32, bpp, true, rw, rh, "a COPY entry that is not the whole block");
    refused(payload_of(3, {record(128, 0, 64, 64, WR_GC_COPY, 0)}), 32, bpp, true, rw, rh, "a COPY entry wider than the cut block");
    refused(payload_of(3, {record(0, 0, 64, 64, WR_GC_COPY, 0), solid, record(0, 0, 64, 64, WR_GC_COPY, 0)}), 64, bpp, true, rw, rh, "two COPY entries of one block");
    {
      // (plain entries cannot be scroll payloads: the flag needs PACKED)
      const Bytes p = payload_of(0, {});
      uint8_t img[4] = {1, 2, 3, 4};
      check(wr_gc_decode(p.data(), p.size(), bpp, false, 1, 1, img, 0, nullptr, nullptr, true) == -1 && img[0] == 1, "SCROLL without PACKED");
    }
    // ---- truncated payloads
    {
      const Bytes good = payload_of(3, {record(0, 0, 64, 64, WR_GC_COPY, 0), record(64, 0, 64, 64, WR_GC_COPY, 0)});
      Bytes out;
      const Bytes image = noise(rw, rh, bpp, 5);
      check(decode(good, good.size(), bpp, true, rw, rh, image, &out) == 0 && out != image, "the good payload decodes");
      for (size_t held = 0; held < good.size(); held++) {
        Bytes cut(good.begin(), good.begin() + held);
        refused(cut, held, bpp, true, rw, rh, "fewer bytes than the header says");
      }
      for (uint32_t count = 1; count < 32; count++) {
        if (count == 16) continue;             // (one whole entry: a good payload)
        Bytes m = good;
        wr_gc_store32(m.data(), count);
        refused(m, m.size(), bpp, true, rw, rh, "a count that cuts a COPY record");
      }
    }
    // ---- all blocks COPY, dy = 1 and dy = -1, entries in the adverse order: the pre-image's pixels all the same
    for (int dy = -1; dy <= 1; dy += 2) {
      const Bytes image = noise(rw, rh, bpp, 7 + dy);
      std::vector<Bytes> entries;
      uint32_t ncopy = 0;
      // adverse: descending y for dy > 0, ascending y for dy < 0; the block rows whose source leaves the rect are not copied
      for (int k = 0; k < 4; k++) {
        const int y = dy > 0 ? 64 * (3 - k) : 64 * k;
        const int h = rh - y < 64 ? rh - y : 64;
        if (y + dy < 0 || y + dy + h > rh) continue;
        for (int x = 128; x >= 0; x -= 64) { entries.push_back(record(x, y, rw - x < 64 ? rw - x : 64, h, WR_GC_COPY, 0)); ncopy++; }
      }
      // a SOLID entry in their middle is applied after them: its block is a COPY's source
      const int sy = dy > 0 ? 192 : 0, sh = dy > 0 ? 8 : 64;
      entries.insert(entries.begin() + 2, record(0, sy, 64, sh, WR_GC_SOLID, 0x5A5A5A5Au));
      Bytes out;
      uint32_t blocks = 0, copied = 0;
      const Bytes p = payload_of(dy, entries);
      check(decode(p, p.size(), bpp, true, rw, rh, image, &out, &blocks, &copied) == 0, "the adverse-order payload decodes");
      check(blocks == ncopy + 1 && copied == ncopy && ncopy == 9, "the adverse-order payload's counts");
      bool ok = true;
      for (int y = 0; y < rh; y++)
        for (int x = 0; x < rw * bpp; x++) {
          const bool in_solid = y >= sy && y < sy + sh && x < 64 * bpp;
          const bool copied_row = dy > 0 ? y < 192 : y >= 64;      // (the block row at the rect's far edge is not copied)
          const uint8_t want = in_solid ? 0x5A : image[(size_t)(copied_row ? y + dy : y) * rw * bpp + x];
          ok = ok && out[(size_t)y * rw * bpp + x] == want;
        }
      check(ok, dy > 0 ? "dy = 1: every COPY block holds the pre-image one row down" : "dy = -1: every COPY block holds the pre-image one row up");
    }
    // ---- a decode that only checks (dst NULL) accepts what a patching one does
    {
      const Bytes p = payload_of(-64, {record(0, 64, 64, 64, WR_GC_COPY, 0)});
      uint32_t blocks = 0, copied = 0;
      check(wr_gc_decode(p.data(), p.size(), bpp, true, rw, rh, nullptr, 0, nullptr, &blocks, true, &copied) == 0 && blocks == 1 && copied == 1, "a checking decode");
    }
  }
  if (failures) { printf("grab_scroll_check: %d case(s) failed\n", failures); return 1; }
  printf("grab_scroll_check: ok\n");
  return 0;
}
