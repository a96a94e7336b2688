// The two roundings of a tensor grab (include/wrhip.h, WrhipGrabTextureTensor): the bits of a float32 to the bits of the nearest
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

#endif
