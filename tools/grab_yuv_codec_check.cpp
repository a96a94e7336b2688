// The host decoder of delta YUV grab payloads (webrender_amd/csrc/wr_grab_codec.h, included alone: wr_gc_decode_yuv, the function
// behind WrhipGrabDecodeYuv) on good and on hostile input.  Meant to be built with -fsanitize=address,undefined
// (tests/test_grab_yuv_delta.py does): every payload and every plane lives in a heap block of exactly its size, so that a read or a
// write beyond either is reported.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I webrender_amd/csrc tools/grab_yuv_codec_check.cpp -o grab_yuv_codec_check
// Exit status 0 and "grab_yuv_codec_check: ok" if every case behaved; otherwise the failed cases are named and the status is 1.
#include "wr_grab_codec.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int failures = 0;
static void check(bool ok, const char* what, int fmt) {
  if (!ok) { printf("FAILED (format %d): %s\n", fmt, what); failures++; }
}

typedef std::vector<uint8_t> Bytes;
static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// the planes of a w x h image: Y; Cb, Cr (I420, I444) or the pairs (NV12), tight
struct Planes {
  int fmt, w, h;
  size_t c_row, c_rows;
  Bytes y, c0, c1;
  Planes(int fmt_, int w_, int h_, uint32_t seed, bool guard) : fmt(fmt_), w(w_), h(h_) {
    c_row = fmt == 2 ? (size_t)w : fmt == 1 ? 2 * (((size_t)w + 1) / 2) : ((size_t)w + 1) / 2;
    c_rows = fmt == 2 ? (size_t)h : ((size_t)h + 1) / 2;
    y.resize((size_t)w * h); c0.resize(c_row * c_rows); c1.resize(fmt == 1 ? 0 : c_row * c_rows);
    for (Bytes* p : {&y, &c0, &c1}) for (uint8_t& v : *p) v = guard ? 0xA5 : (uint8_t)rnd(seed);
  }
  bool all_guard() const {
    for (const Bytes* p : {&y, &c0, &c1}) for (uint8_t v : *p) if (v != 0xA5) return false;
    return true;
  }
};
// the entry of the block at (x, y) of `P`, cut to the image; bytes beyond the cut block are noise
static Bytes entry_of(const Planes& P, int x, int y, uint32_t seed) {
  const int bw = P.w - x < WR_GC_BLOCK ? P.w - x : WR_GC_BLOCK, bh = P.h - y < WR_GC_BLOCK ? P.h - y : WR_GC_BLOCK;
  Bytes e(wr_gc_yuv_entry_size((uint32_t)P.fmt));
  for (uint8_t& v : e) v = (uint8_t)rnd(seed);
  wr_gc_store32(e.data(), (uint32_t)x); wr_gc_store32(e.data() + 4, (uint32_t)y); wr_gc_store32(e.data() + 8, (uint32_t)bw); wr_gc_store32(e.data() + 12, (uint32_t)bh);
  uint8_t* body = e.data() + 16;
  for (int r = 0; r < bh; r++) memcpy(body + 64 * r, P.y.data() + (size_t)(y + r) * P.w + x, (size_t)bw);
  body += 4096;
  if (P.fmt == 2) {
    for (int r = 0; r < bh; r++) {
      memcpy(body + 64 * r, P.c0.data() + (size_t)(y + r) * P.c_row + x, (size_t)bw);
      memcpy(body + 4096 + 64 * r, P.c1.data() + (size_t)(y + r) * P.c_row + x, (size_t)bw);
    }
    return e;
  }
  const int cw = (bw + 1) / 2, ch = (bh + 1) / 2;
  for (int r = 0; r < ch; r++) {
    if (P.fmt == 1) memcpy(body + 64 * r, P.c0.data() + (size_t)(y / 2 + r) * P.c_row + x, (size_t)2 * cw);
    else {
      memcpy(body + 32 * r, P.c0.data() + (size_t)(y / 2 + r) * P.c_row + x / 2, (size_t)cw);
      memcpy(body + 1024 + 32 * r, P.c1.data() + (size_t)(y / 2 + r) * P.c_row + x / 2, (size_t)cw);
    }
  }
  return e;
}
// header + entries; count: the header's word (-1: what the entries come to)
static Bytes payload_of(const std::vector<Bytes>& entries, long long count = -1) {
  Bytes p(WR_GC_HEADER, 0);
  for (const Bytes& e : entries) p.insert(p.end(), e.begin(), e.end());
  wr_gc_store32(p.data(), count < 0 ? (uint32_t)(p.size() - WR_GC_HEADER) : (uint32_t)count);
  return p;
}
// decode the first `bytes` of `p`, held in a heap block of exactly that size, into `out` -- planes in heap blocks of exactly their
// sizes -- or check it only (out == nullptr)
static int decode(const Bytes& p, size_t bytes, Planes* out, int fmt, int w, int h, int32_t damage[4], uint32_t* blocks) {
  uint8_t* src = (uint8_t*)malloc(bytes ? bytes : 1);
  memcpy(src, p.data(), bytes);
  uint8_t *y = nullptr, *c0 = nullptr, *c1 = nullptr;
  if (out) {
    y = (uint8_t*)malloc(out->y.size()); c0 = (uint8_t*)malloc(out->c0.size()); c1 = fmt == 1 ? nullptr : (uint8_t*)malloc(out->c1.size());
    memcpy(y, out->y.data(), out->y.size()); memcpy(c0, out->c0.data(), out->c0.size());
    if (c1) memcpy(c1, out->c1.data(), out->c1.size());
  }
  const int rc = wr_gc_decode_yuv(src, bytes, (uint32_t)fmt, w, h, y, 0, c0, c1, 0, damage, blocks);
  if (out) {
    memcpy(out->y.data(), y, out->y.size()); memcpy(out->c0.data(), c0, out->c0.size());
    if (c1) memcpy(out->c1.data(), c1, out->c1.size());
    free(y); free(c0); free(c1);
  }
  free(src);
  return rc;
}
static void refused(const Bytes& p, size_t bytes, int fmt, int w, int h, const char* what) {
  Planes out(fmt, w, h, 0, true);
  int32_t damage[4];
  uint32_t blocks = 0;
  check(decode(p, bytes, &out, fmt, w, h, damage, &blocks) == -1 && out.all_guard(), what, fmt);
  check(decode(p, bytes, nullptr, fmt, w, h, damage, &blocks) == -1, what, fmt);      // check-only mode agrees
}

static void one_format(int fmt, int w, int h) {
  const Planes img(fmt, w, h, (uint32_t)(w * 131 + h + fmt), false);
  const size_t entry = wr_gc_yuv_entry_size((uint32_t)fmt);
  check(entry == (fmt == 2 ? 16u + 12288u : 16u + 6144u), "the entry's size", fmt);
  std::vector<Bytes> all;
  uint32_t seed = 77;
  for (int y = h - 1 - (h - 1) % WR_GC_BLOCK; y >= 0; y -= WR_GC_BLOCK)          // (the order of the entries is free: last block first)
    for (int x = w - 1 - (w - 1) % WR_GC_BLOCK; x >= 0; x -= WR_GC_BLOCK) all.push_back(entry_of(img, x, y, rnd(seed)));
  int32_t damage[4];
  uint32_t blocks = 0;
  {
    Planes out(fmt, w, h, 0, true);
    const Bytes p = payload_of(all);
    check(decode(p, p.size(), &out, fmt, w, h, damage, &blocks) == 0 && out.y == img.y && out.c0 == img.c0 && out.c1 == img.c1, "every block decodes to the planes", fmt);
    check(blocks == all.size() && damage[0] == 0 && damage[1] == 0 && damage[2] == w && damage[3] == h, "blocks and damage of every block", fmt);
    // check-only mode: the same answer, nothing to write to
    blocks = 0;
    check(decode(p, p.size(), nullptr, fmt, w, h, damage, &blocks) == 0 && blocks == all.size() && damage[2] == w && damage[3] == h, "check-only mode", fmt);
    check(wr_gc_decode_yuv(p.data(), p.size(), (uint32_t)fmt, w, h, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == 0, "check-only mode without outputs", fmt);
  }
  {
    // one entry, the last (cut) block: only its samples are written
    Planes out(fmt, w, h, 0, true);
    const Bytes p = payload_of({all[0]});
    const int x = w - 1 - (w - 1) % WR_GC_BLOCK, y = h - 1 - (h - 1) % WR_GC_BLOCK;
    check(decode(p, p.size(), &out, fmt, w, h, damage, &blocks) == 0 && blocks == 1 && damage[0] == x && damage[1] == y && damage[2] == w - x && damage[3] == h - y, "one cut block", fmt);
    size_t written = 0;
    for (const Bytes* q : {&out.y, &out.c0, &out.c1}) for (uint8_t v : *q) written += v != 0xA5;
    const size_t bw = (size_t)(w - x), bh = (size_t)(h - y);
    const size_t most = fmt == 2 ? 3 * bw * bh : bw * bh + 2 * ((bw + 1) / 2) * ((bh + 1) / 2);
    check(written <= most && written + most / 8 + 4 >= most, "one cut block writes its samples alone", fmt);      // (a sample may BE 0xA5)
    const Bytes none = payload_of({});
    check(decode(none, none.size(), &out, fmt, w, h, damage, &blocks) == 0 && blocks == 0 && damage[2] == 0 && damage[3] == 0, "an empty payload", fmt);
  }
  const Bytes& good = all.back();      // the block at (0, 0)
  const Bytes gp = payload_of({good});
  // truncated
  refused(gp, gp.size() - 1, fmt, w, h, "truncated by a byte");
  refused(gp, WR_GC_HEADER + 8, fmt, w, h, "truncated inside the record");
  refused(gp, WR_GC_HEADER + 16 + 100, fmt, w, h, "truncated inside the body");
  refused(gp, 15, fmt, w, h, "fewer bytes than a header");
  // a bad header count
  Bytes m = payload_of({good}, (long long)entry - 16); refused(m, m.size(), fmt, w, h, "a count that is not k entries");
  m = payload_of({good}, (long long)entry + 1); refused(m, m.size(), fmt, w, h, "a count one above an entry");
  m = payload_of({good}, 2 * (long long)entry); refused(m, m.size(), fmt, w, h, "a count of more than is held");
  m = payload_of({good}, 0xFFFFFFF0ll); refused(m, m.size(), fmt, w, h, "a huge count");
  // x, y
  const uint32_t xy[7][2] = {{32, 0}, {0, 1}, {63, 64}, {(uint32_t)((w + 63) / 64 * 64), 0}, {0, (uint32_t)((h + 63) / 64 * 64)}, {0xFFFFFFC0u, 0}, {0, 0x80000000u}};
  for (int k = 0; k < 7; k++) {
    Bytes e = good;
    wr_gc_store32(e.data(), xy[k][0]); wr_gc_store32(e.data() + 4, xy[k][1]);
    const Bytes p = payload_of({e});
    refused(p, p.size(), fmt, w, h, "a misaligned or outside x / y");
  }
  // w, h: not the cut block's
  const uint32_t wh[6][2] = {{0, 64}, {64, 0}, {63, 64}, {64, 63}, {65, 64}, {0xFFFFFFFFu, 64}};
  for (int k = 0; k < 6; k++) {
    Bytes e = good;
    wr_gc_store32(e.data() + 8, wh[k][0]); wr_gc_store32(e.data() + 12, wh[k][1]);
    const Bytes p = payload_of({e});
    refused(p, p.size(), fmt, w, h, "a w / h that is not the cut block's");
  }
  if (w % WR_GC_BLOCK || h % WR_GC_BLOCK) {
    Bytes e = all[0];                  // the cut corner block, claimed whole
    wr_gc_store32(e.data() + 8, 64); wr_gc_store32(e.data() + 12, 64);
    const Bytes p = payload_of({e});
    refused(p, p.size(), fmt, w, h, "a cut block claimed whole");
  }
  // too many entries; a good entry ahead of a bad one
  std::vector<Bytes> more = all;
  more.push_back(good);
  m = payload_of(more); refused(m, m.size(), fmt, w, h, "more entries than blocks");
  Bytes bad = good;
  wr_gc_store32(bad.data(), 32);
  m = payload_of({good, bad}); refused(m, m.size(), fmt, w, h, "a good entry ahead of a bad one");
  // the rect, the format
  check(wr_gc_decode_yuv(gp.data(), gp.size(), (uint32_t)fmt, 0, h, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == -1, "an empty image", fmt);
  check(wr_gc_decode_yuv(gp.data(), gp.size(), 3u, w, h, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == -1, "an unknown format", fmt);
}

int main() {
  for (int fmt = 0; fmt < 3; fmt++) {
    one_format(fmt, 130, 67);
    one_format(fmt, 333, 201);
    one_format(fmt, 64, 64);
    one_format(fmt, 1, 1);
  }
  if (failures) return 1;
  printf("grab_yuv_codec_check: ok\n");
  return 0;
}
