// The two roundings of a tensor grab (include/wrhip.h, WrhipGrabTextureTensor), and below them the two conversions of a tensor put: the bits of a float32 to the bits of the nearest
// float16 / bfloat16, ties to even, as integer arithmetic -- the device build and the host simulation compile this very text, so
// they cannot disagree.  float16: subnormals are produced (the smallest is 2^-24; 2^-25 and below, a tie included, give zero),
// 65520 and above go to infinity, infinity stays, a NaN stays a quiet NaN of its sign.  Plain C++: nothing but this file is needed.
#ifndef WR_TENSOR_ROUND_H
#define WR_TENSOR_ROUND_H
#include <stdint.h>

#ifdef WR_DEVICE
#define WR_TR_FN WR_DEVICE
#else
#define WR_TR_FN static inline
#endif

WR_TR_FN uint16_t wr_f32_to_f16_bits(uint32_t u) {
  const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);
  if (a >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);             // 65536 and above, infinity
  if (a >= 0x38800000u) {
    // normal (2^-14 and above): the exponent rebased, 13 mantissa bits rounded away -- a carry runs into the exponent, up to infinity
    const uint32_t r = a - 0x38000000u;
    return (uint16_t)(sign | ((r + 0xFFFu + ((r >> 13) & 1u)) >> 13));
  }
  if (a < 0x33000000u) return (uint16_t)sign;                          // below 2^-25
  // subnormal: the 24-bit significand in units of 2^-24, i.e. shifted right by 126 - e (14 .. 24) bits
  const uint32_t e = a >> 23, m = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - e;
  const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
}

WR_TR_FN uint16_t wr_f32_to_bf16_bits(uint32_t u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// The way back, for a tensor put (include/wrhip.h, WrhipPutTextureTensor).  The bits of a float16 to the bits of the float32 of the
// same value: exact for every pattern -- subnormals are normalised, infinity stays, a NaN keeps its sign and its payload's bits.
WR_TR_FN uint32_t wr_f16_bits_to_f32_bits(uint16_t h) {
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = ((uint32_t)h >> 10) & 31u;
  uint32_t m = (uint32_t)h & 0x3FFu;
  if (e == 31u) return sign | 0x7F800000u | (m << 13);
  if (e != 0u) return sign | ((e + 112u) << 23) | (m << 13);
  if (m == 0u) return sign;
  // subnormal: m * 2^-24; shifted up until its leading bit is the implicit one (s = 1 .. 10 shifts: 2^-14-s)
  uint32_t s = 0;
  while (!(m & 0x400u)) { m <<= 1; s++; }
  return sign | ((113u - s) << 23) | ((m & 0x3FFu) << 13);
}
// The bits of a float32 y to the stored byte: 0 for a NaN and for y < 0 (and -0), 255 for y >= 255, otherwise y rounded to nearest,
// ties to even (0.5 -> 0, 1.5 -> 2, 2.5 -> 2) -- what cvtps2dq does to a value in range.
WR_TR_FN uint8_t wr_f32_bits_to_byte(uint32_t u) {
  if ((u >> 31) || u > 0x7F800000u) return 0;                          // negative, or a NaN of either sign
  if (u >= 0x437F0000u) return 255;                                    // 255 and above, infinity
  if (u < 0x3F000000u) return 0;                                       // below 0.5
  // 0.5 <= y < 255: the 24-bit significand in units of 2^(e - 150), i.e. shifted right by 150 - e (16 .. 24) bits
  const uint32_t e = u >> 23, m = (u & 0x7FFFFFu) | 0x800000u, shift = 150u - e;
  const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  return (uint8_t)(q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
}

#endif
