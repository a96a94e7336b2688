// The host decoder of delta-grab payloads (webrender_amd/csrc/wr_grab_codec.h, included alone) on good and on hostile input.
// Meant to be built with -fsanitize=address,undefined (tests/test_grab_packed.py does): every payload lives in a heap block of
// exactly its size and the image in one of exactly its size, so that a read or a write beyond either is reported.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I webrender_amd/csrc tools/grab_codec_check.cpp -o grab_codec_check
// Exit status 0 and "grab_codec_check: ok" if every case behaved; otherwise the failed cases are named and the status is 1.
#include "wr_grab_codec.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int failures = 0;
static void check(bool ok, const char* what) {
  if (!ok) { printf("FAILED: %s\n", what); failures++; }
}

typedef std::vector<uint8_t> Bytes;

// header + entries
static Bytes payload_of(const std::vector<Bytes>& entries) {
  Bytes p(WR_GC_HEADER, 0);
  for (const Bytes& e : entries) p.insert(p.end(), e.begin(), e.end());
  wr_gc_store32(p.data(), (uint32_t)(p.size() - WR_GC_HEADER));
  return p;
}
// decode `p` (in a heap block of its own size) into an image of 0xA5: the result, and whether the image was left alone
static int decode(const Bytes& p, uint64_t bytes, int bpp, bool packed, int rw, int rh, bool* untouched, Bytes* image = nullptr) {
  uint8_t* src = (uint8_t*)malloc(p.size() ? p.size() : 1);
  memcpy(src, p.data(), p.size());
  const size_t n = (size_t)rw * rh * bpp;
  uint8_t* img = (uint8_t*)malloc(n);
  memset(img, 0xA5, n);
  int32_t damage[4];
  uint32_t blocks = 0;
  const int rc = wr_gc_decode(src, bytes, bpp, packed, rw, rh, img, 0, damage, &blocks);
  bool same = true;
  for (size_t i = 0; i < n; i++) same = same && img[i] == 0xA5;
  if (untouched) *untouched = same;
  if (image) image->assign(img, img + n);
  free(img);
  free(src);
  return rc;
}
static void refused(const Bytes& p, uint64_t bytes, int bpp, int rw, int rh, const char* what) {
  bool untouched = false;
  const int rc = decode(p, bytes, bpp, true, rw, rh, &untouched);
  check(rc == -1 && untouched, what);
}
static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// an image of blocks that are flat, striped, noise: every mode occurs
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
static void round_trip(int w, int h, int bpp) {
  const Bytes img = test_image(w, h, bpp, (uint32_t)(w * 131 + h));
  std::vector<Bytes> packed, plain;
  int modes[3] = {0, 0, 0};
  for (int y = 0; y < h; y += WR_GC_BLOCK)
    for (int x = 0; x < w; x += WR_GC_BLOCK) {
      const int bw = w - x < WR_GC_BLOCK ? w - x : WR_GC_BLOCK, bh = h - y < WR_GC_BLOCK ? h - y : WR_GC_BLOCK;
      Bytes e(wr_gc_raw_size(bpp));
      e.resize(wr_gc_encode_block(img.data() + ((size_t)y * w + x) * bpp, (size_t)w * bpp, x, y, bw, bh, bpp, e.data()));
      modes[(wr_gc_load32(e.data() + 8) >> 16) & 3]++;
      packed.push_back(e);
      Bytes q(wr_gc_raw_size(bpp), 0);
      wr_gc_store32(q.data(), (uint32_t)x); wr_gc_store32(q.data() + 4, (uint32_t)y); wr_gc_store32(q.data() + 8, (uint32_t)bw); wr_gc_store32(q.data() + 12, (uint32_t)bh);
      for (int r = 0; r < bh; r++) memcpy(q.data() + 16 + (size_t)r * WR_GC_BLOCK * bpp, img.data() + ((size_t)(y + r) * w + x) * bpp, (size_t)bw * bpp);
      plain.push_back(q);
    }
  Bytes out;
  const Bytes pp = payload_of(packed), pl = payload_of(plain);
  check(decode(pp, pp.size(), bpp, true, w, h, nullptr, &out) == 0 && out == img, "a valid packed payload decodes to the image");
  check(decode(pl, pl.size(), bpp, false, w, h, nullptr, &out) == 0 && out == img, "a valid plain payload decodes to the image");
  check(pp.size() < pl.size(), "the packed payload is the smaller one");
  if (w >= 3 * WR_GC_BLOCK && h >= WR_GC_BLOCK) check(modes[0] && modes[1] && modes[2], "the image has blocks of every mode");
}

int main() {
  round_trip(130, 67, 4);
  round_trip(333, 201, 4);
  round_trip(61, 37, 1);
  round_trip(200, 130, 1);
  round_trip(1, 1, 4);

  for (int bpp = 1; bpp <= 4; bpp += 3) {
    // one RUNS entry: a 10 x 5 block at (3, 2) of a 20 x 10 rect, vertical stripes 2 pixels wide (pixels 0 and 1 share a value)
    const int rw = 20, rh = 10, w = 10, h = 5;
    Bytes blk((size_t)w * h * bpp);
    for (int i = 0; i < w * h; i++)
      for (int k = 0; k < bpp; k++) blk[(size_t)i * bpp + k] = (uint8_t)(((i % w) / 2) * 40 + k);
    Bytes e(wr_gc_raw_size(bpp));
    e.resize(wr_gc_encode_block(blk.data(), (size_t)w * bpp, 3, 2, w, h, bpp, e.data()));
    const uint32_t n = wr_gc_load32(e.data() + 12);
    check((wr_gc_load32(e.data() + 8) >> 16) == WR_GC_RUNS && n == 25, "the stripes are a RUNS entry of 25 starts");
    const Bytes good = payload_of({e});
    bool untouched = true;
    check(decode(good, good.size(), bpp, true, rw, rh, &untouched) == 0 && !untouched, "the RUNS entry decodes");

    // truncated: the caller holds fewer bytes than the header says, or the header itself says fewer than the entry needs
    const size_t cuts[3] = {8, 16 + 12, 16 + 8 * (size_t)h + (size_t)bpp * 3 / 2 + 1};
    const char* cut_names[3] = {"truncated inside the record", "truncated inside the bitmap", "truncated inside the literals"};
    for (int c = 0; c < 3; c++) {
      Bytes held(good.begin(), good.begin() + WR_GC_HEADER + cuts[c]);
      refused(held, held.size(), bpp, rw, rh, cut_names[c]);
      wr_gc_store32(held.data(), (uint32_t)cuts[c]);
      refused(held, held.size(), bpp, rw, rh, cut_names[c]);
    }
    refused(good, 15, bpp, rw, rh, "fewer bytes than a header");
    // n against the bitmap's popcount
    Bytes m = e;
    wr_gc_store32(m.data() + 12, n + 1); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "n larger than the bitmap's popcount");
    wr_gc_store32(m.data() + 12, n - 1); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "n smaller than the bitmap's popcount");
    wr_gc_store32(m.data() + 12, 0xFFFFFFF0u); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "an n that overflows the size");
    // w, h
    const uint32_t whs[4][2] = {{0, 5}, {10, 0}, {65, 5}, {10, 65}};
    for (int k = 0; k < 4; k++) {
      m = e; m.resize(wr_gc_raw_size(bpp), 0);
      wr_gc_store32(m.data() + 8, whs[k][0] | whs[k][1] << 8 | (uint32_t)WR_GC_RUNS << 16);
      refused(payload_of({m}), 16 + m.size(), bpp, 200, 200, "w or h of 0 or above 64");
      wr_gc_store32(m.data() + 8, whs[k][0] | whs[k][1] << 8 | (uint32_t)WR_GC_SOLID << 16);
      refused(payload_of({m}), 16 + m.size(), bpp, 200, 200, "w or h of 0 or above 64 (SOLID)");
      wr_gc_store32(m.data() + 8, whs[k][0] | whs[k][1] << 8);
      refused(payload_of({m}), 16 + m.size(), bpp, 200, 200, "w or h of 0 or above 64 (RAW)");
    }
    // the block against the rect
    m = e; wr_gc_store32(m.data(), 11); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "x + w beyond the rect");
    m = e; wr_gc_store32(m.data() + 4, 6); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "y + h beyond the rect");
    m = e; wr_gc_store32(m.data(), 0xFFFFFFFEu); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "a negative x");
    m = e; wr_gc_store32(m.data() + 4, 0x80000000u); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "a negative y");
    refused(good, good.size(), bpp, 9, 4, "a rect smaller than the block");
    // mode 3
    m = e; wr_gc_store32(m.data() + 8, (uint32_t)w | (uint32_t)h << 8 | 3u << 16); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "mode 3");
    // a bitmap bit at a column >= w (in place of one inside: the popcount stays n)
    m = e; m[16 + 8] = (uint8_t)(m[16 + 8] & ~1u); m[16 + 8 + 1] |= 1u << 2; refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "a bitmap bit at a column >= w");
    // the first pixel without a start bit (pixel 1 gets it: the popcount stays n)
    m = e; m[16] = (uint8_t)((m[16] & ~1u) | 2u); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "a first pixel without a start bit");
    // a good entry ahead of a bad one: nothing of either is written
    m = e; wr_gc_store32(m.data() + 8, (uint32_t)w | (uint32_t)h << 8 | 3u << 16);
    refused(payload_of({e, m}), 16 + e.size() + m.size(), bpp, rw, rh, "a good entry ahead of a bad one");
    // RAW cut short
    m = e; wr_gc_store32(m.data() + 8, (uint32_t)w | (uint32_t)h << 8); refused(payload_of({m}), 16 + m.size(), bpp, rw, rh, "a RAW entry without its body");
  }
  if (failures) return 1;
  printf("grab_codec_check: ok\n");
  return 0;
}
