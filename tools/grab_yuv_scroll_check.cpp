// The host decoder of scroll-aware delta YUV payloads (webrender_amd/csrc/wr_grab_codec.h, included alone; the contract:
// include/wrhip.h, WrhipGrabTextureYuvDelta with WRHIP_GRAB_SCROLL) on hostile input and on COPY entries in the adverse order.
// Meant to be built with -fsanitize=address,undefined (tests/test_grab_yuv_scroll.py does): every payload lives in a heap block of
// exactly its size and every plane in one of exactly its size, so that a read or a write beyond either is reported.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I webrender_amd/csrc tools/grab_yuv_scroll_check.cpp -o grab_yuv_scroll_check
// Exit status 0 and "grab_yuv_scroll_check: ok" if every case behaved; otherwise the failed cases are named and the status is 1.
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

// an entry: the record, and for mode 0 a body of noise
static Bytes entry(int fmt, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t mode, uint32_t word3 = 0, uint32_t seed = 1) {
  Bytes e(mode == WR_GC_RAW ? wr_gc_yuv_entry_size((uint32_t)fmt) : 16);
  wr_gc_store32(e.data(), x); wr_gc_store32(e.data() + 4, y); wr_gc_store32(e.data() + 8, w | h << 8 | mode << 16); wr_gc_store32(e.data() + 12, word3);
  for (size_t i = 16; i < e.size(); i++) e[i] = (uint8_t)rnd(seed);
  return e;
}
static Bytes payload_of(int32_t dy, const std::vector<Bytes>& entries) {
  Bytes p(WR_GC_HEADER, 0);
  for (const Bytes& e : entries) p.insert(p.end(), e.begin(), e.end());
  wr_gc_store32(p.data(), (uint32_t)(p.size() - WR_GC_HEADER));
  wr_gc_store32(p.data() + 4, (uint32_t)dy);
  return p;
}
// the three planes of a w x h image, each a vector of exactly its size (NV12: c1 empty)
struct Planes {
  Bytes y, c0, c1;
  size_t cs = 0;
  int crows = 0;
  bool operator==(const Planes& o) const { return y == o.y && c0 == o.c0 && c1 == o.c1; }
};
static Planes planes_of(int fmt, int w, int h, uint32_t seed) {
  Planes P;
  P.cs = fmt == 2 ? (size_t)w : fmt == 1 ? 2 * (((size_t)w + 1) / 2) : ((size_t)w + 1) / 2;
  P.crows = fmt == 2 ? h : (h + 1) / 2;
  P.y.resize((size_t)w * h); P.c0.resize(P.cs * P.crows);
  if (fmt != 1) P.c1.resize(P.cs * P.crows);
  for (uint8_t& b : P.y) b = (uint8_t)rnd(seed);
  for (uint8_t& b : P.c0) b = (uint8_t)rnd(seed);
  for (uint8_t& b : P.c1) b = (uint8_t)rnd(seed);
  return P;
}
// decode `bytes` of `p` (in a heap block of its own size) into copies of the planes (heap blocks of their sizes)
static int decode(const Bytes& p, uint64_t bytes, int fmt, bool scroll, int rw, int rh, const Planes& in, Planes* out, uint32_t* blocks = nullptr, uint32_t* copied = nullptr) {
  uint8_t* src = (uint8_t*)malloc(p.size() ? p.size() : 1);
  if (!p.empty()) memcpy(src, p.data(), p.size());
  uint8_t* y = (uint8_t*)malloc(in.y.size());
  uint8_t* c0 = (uint8_t*)malloc(in.c0.size());
  uint8_t* c1 = in.c1.empty() ? nullptr : (uint8_t*)malloc(in.c1.size());
  memcpy(y, in.y.data(), in.y.size()); memcpy(c0, in.c0.data(), in.c0.size());
  if (c1) memcpy(c1, in.c1.data(), in.c1.size());
  int32_t damage[4];
  const int rc = wr_gc_decode_yuv(src, bytes, (uint32_t)fmt, rw, rh, y, 0, c0, c1, 0, damage, blocks, scroll, copied);
  *out = in;
  out->y.assign(y, y + in.y.size()); out->c0.assign(c0, c0 + in.c0.size());
  if (c1) out->c1.assign(c1, c1 + in.c1.size());
  free(c1); free(c0); free(y); free(src);
  return rc;
}
static void refused(const Bytes& p, uint64_t bytes, int fmt, bool scroll, int rw, int rh, const char* what) {
  const Planes in = planes_of(fmt, rw, rh, 99);
  Planes out;
  const int rc = decode(p, bytes, fmt, scroll, rw, rh, in, &out);
  check(rc == -1 && out == in, what, fmt);
}

int main() {
  for (int fmt = 0; fmt <= 2; fmt++) {
    const int rw = 130, rh = 201;            // 3 x 4 blocks; the last column 2 wide, the last row 9 high; 101 chroma rows in 4:2:0
    const uint32_t C = WR_GC_COPY, S = WR_GC_RAW;
    auto E = [&](uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t mode, uint32_t word3 = 0) { return entry(fmt, x, y, w, h, mode, word3); };
    const Bytes samples = E(64, 64, 64, 64, S);
    // ---- malformed payloads: -1, nothing written
    refused(payload_of(4, {E(0, 0, 64, 64, 1)}), ~0ull, fmt, true, rw, rh, "mode 1");
    refused(payload_of(4, {E(0, 0, 64, 64, 2)}), ~0ull, fmt, true, rw, rh, "mode 2");
    refused(payload_of(4, {E(0, 0, 64, 64, 4)}), ~0ull, fmt, true, rw, rh, "mode 4");
    refused(payload_of(4, {E(0, 0, 64, 64, 0xFFFF)}), ~0ull, fmt, true, rw, rh, "mode 65535");
    refused(payload_of(4, {E(0, 0, 64, 64, C, 1)}), ~0ull, fmt, true, rw, rh, "a COPY record with a non-zero word 3");
    refused(payload_of(4, {E(64, 64, 64, 64, S, 7)}), ~0ull, fmt, true, rw, rh, "a SAMPLES record with a non-zero word 3");
    refused(payload_of(0, {E(0, 0, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "COPY with dy == 0");
    refused(payload_of(514, {samples}), ~0ull, fmt, true, rw, rh, "dy above the bound");
    refused(payload_of(-514, {samples}), ~0ull, fmt, true, rw, rh, "dy below the bound");
    refused(payload_of(514, {E(0, 0, 64, 64, C)}), ~0ull, fmt, true, 64, 700, "COPY with dy above the bound, the source inside the image");
    refused(payload_of((int32_t)0x80000000u, {E(0, 64, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "the most negative dy");
    if (fmt != 2) {
      refused(payload_of(3, {E(0, 0, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "COPY with an odd dy in a 4:2:0 format");
      refused(payload_of(-1, {E(0, 64, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "COPY with dy == -1 in a 4:2:0 format");
    }
    refused(payload_of(6, {E(0, 128, 64, 64, C), E(0, 192, 64, 9, C)}), ~0ull, fmt, true, rw, rh, "a COPY source below the image");
    refused(payload_of(-6, {samples, E(64, 0, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "a COPY source above the image");
    refused(payload_of(138, {E(0, 0, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "a COPY source that ends one row below the image");
    refused(payload_of(4, {E(2, 0, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "a COPY entry that is not on the block grid");
    refused(payload_of(4, {E(0, 0, 62, 64, C)}), ~0ull, fmt, true, rw, rh, "a COPY entry that is not the whole block");
    refused(payload_of(4, {E(128, 0, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "a COPY entry wider than the cut block");
    refused(payload_of(4, {E(0, 192, 64, 64, S)}), ~0ull, fmt, true, rw, rh, "a SAMPLES entry taller than the cut block");
    refused(payload_of(4, {E(192, 0, 64, 64, S)}), ~0ull, fmt, true, rw, rh, "a SAMPLES entry outside the image");
    refused(payload_of(4, {E(0, 0, 64, 64, C), samples, E(0, 0, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "two COPY entries of one block");
    refused(payload_of(4, {samples, E(64, 64, 64, 64, C)}), ~0ull, fmt, true, rw, rh, "a SAMPLES and a COPY entry of one block");
    refused(payload_of(4, {samples, samples}), ~0ull, fmt, true, rw, rh, "two SAMPLES entries of one block");
    refused(payload_of(4, {E(0, 0, 64, 64, C)}), ~0ull, fmt, false, rw, rh, "mode 3 without the SCROLL bit");
    {
      // (a plain delta YUV payload: records x, y, w, h)
      Bytes plain = entry(fmt, 64, 64, 0, 0, S);
      wr_gc_store32(plain.data() + 8, 64); wr_gc_store32(plain.data() + 12, 64);
      Planes out;
      const Planes in = planes_of(fmt, rw, rh, 3);
      Bytes ok = payload_of(0, {plain});
      check(decode(ok, ok.size(), fmt, false, rw, rh, in, &out) == 0 && !(out == in), "a plain payload decodes without the bit", fmt);
      refused(payload_of(4, {plain}), ~0ull, fmt, false, rw, rh, "a non-zero header word 1 without the SCROLL bit");
      refused(ok, ok.size(), fmt, true, rw, rh, "a plain record with the SCROLL bit");
    }
    // ---- truncations: every 16-byte boundary of a valid payload, as bytes held and as the header's count
    {
      const Bytes good = payload_of(4, {E(0, 0, 64, 64, C), samples, E(64, 0, 64, 64, C)});
      Planes out;
      const Planes in = planes_of(fmt, rw, rh, 5);
      check(decode(good, good.size(), fmt, true, rw, rh, in, &out) == 0 && !(out == in), "the good payload decodes", fmt);
      for (size_t held = 0; held < good.size(); held += 16) {
        Bytes cut(good.begin(), good.begin() + held);
        refused(cut, held, fmt, true, rw, rh, "fewer bytes than the header says");
      }
      for (size_t held = 1; held < 48; held++) {
        Bytes cut(good.begin(), good.begin() + held);
        refused(cut, held, fmt, true, rw, rh, "a payload cut inside the header or the first record");
      }
      const uint32_t whole[3] = {0, 16, 16 + (uint32_t)samples.size()};
      for (uint32_t count = 0; count < (uint32_t)(good.size() - WR_GC_HEADER); count += 16) {
        if (count == whole[0] || count == whole[1] || count == whole[2]) continue;      // (whole entries: a good payload)
        Bytes m = good;
        wr_gc_store32(m.data(), count);
        refused(m, m.size(), fmt, true, rw, rh, "a count that cuts a SAMPLES entry");
      }
      for (uint32_t count = 1; count < 16; count++) {
        Bytes m = good;
        wr_gc_store32(m.data(), count);
        refused(m, m.size(), fmt, true, rw, rh, "a count that cuts a record");
      }
    }
    // ---- all blocks COPY, entries in the adverse order, a SAMPLES entry whose block is a COPY's source among them
    for (int dy = -2; dy <= 2; dy += 4) {
      const Planes in = planes_of(fmt, rw, rh, 7 + dy);
      std::vector<Bytes> entries;
      uint32_t ncopy = 0;
      // adverse: descending y for dy > 0, ascending y for dy < 0; the block rows whose source leaves the image are not copied
      for (int k = 0; k < 4; k++) {
        const int y = dy > 0 ? 64 * (3 - k) : 64 * k;
        const int h = rh - y < 64 ? rh - y : 64;
        if (y + dy < 0 || y + dy + h > rh) continue;
        for (int x = 128; x >= 0; x -= 64) { entries.push_back(E(x, y, rw - x < 64 ? rw - x : 64, h, C)); ncopy++; }
      }
      const int sy = dy > 0 ? 192 : 0, sh = dy > 0 ? 9 : 64;
      const Bytes smp = E(0, sy, 64, sh, S);
      entries.insert(entries.begin() + 2, smp);
      Planes out;
      uint32_t blocks = 0, copied = 0;
      const Bytes p = payload_of(dy, entries);
      check(decode(p, p.size(), fmt, true, rw, rh, in, &out, &blocks, &copied) == 0, "the adverse-order payload decodes", fmt);
      check(blocks == ncopy + 1 && copied == ncopy && ncopy == 9, "the adverse-order payload's counts", fmt);
      // luma: every copied row holds the pre-image dy rows away; the SAMPLES block holds its body
      bool ok = true;
      for (int y = 0; y < rh; y++)
        for (int x = 0; x < rw; x++) {
          const bool in_s = y >= sy && y < sy + sh && x < 64;
          const bool copied_row = dy > 0 ? y < 192 : y >= 64;
          const uint8_t want = in_s ? smp[16 + (size_t)(y - sy) * 64 + x] : in.y[(size_t)(copied_row ? y + dy : y) * rw + x];
          ok = ok && out.y[(size_t)y * rw + x] == want;
        }
      check(ok, "the luma plane after the adverse-order payload", fmt);
      // chroma: rows move by dy (I444) or dy / 2 (4:2:0); the first chroma plane outside the SAMPLES block
      ok = true;
      const int cd = fmt == 2 ? dy : dy / 2, cx0 = fmt == 2 ? 64 : fmt == 1 ? 64 : 32;
      const int c_first = fmt == 2 ? (dy > 0 ? 0 : 64) : (dy > 0 ? 0 : 32), c_end = fmt == 2 ? (dy > 0 ? 192 : rh) : (dy > 0 ? 96 : in.crows);
      for (int r = 0; r < in.crows; r++)
        for (size_t x = (size_t)cx0; x < in.cs; x++) {
          const bool copied_row = r >= c_first && r < c_end;
          ok = ok && out.c0[(size_t)r * in.cs + x] == in.c0[(size_t)(copied_row ? r + cd : r) * in.cs + x];
        }
      check(ok, "the first chroma plane after the adverse-order payload", fmt);
    }
    // ---- a decode that only checks (no planes) accepts what a patching one does
    {
      const Bytes p = payload_of(-64, {E(0, 64, 64, 64, C), samples});
      uint32_t blocks = 0, copied = 0;
      check(wr_gc_decode_yuv(p.data(), p.size(), (uint32_t)fmt, rw, rh, nullptr, 0, nullptr, nullptr, 0, nullptr, &blocks, true, &copied) == 0 && blocks == 2 && copied == 1, "a checking decode", fmt);
    }
  }
  if (failures) { printf("grab_yuv_scroll_check: %d case(s) failed\n", failures); return 1; }
  printf("grab_yuv_scroll_check: ok\n");
  return 0;
}
