// Decode of one Radiance RGBE pixel code (r | g << 8 | b << 16 | e << 24, the bytes in memory
// order), shared by the codec (hdrio.hip) and the HDR pair generator (hdrpairs.hip).  Exact, done on
// the bit patterns: see hdrio.hip.
#pragma once
#include "common.h"

__device__ __forceinline__ float decode_c(uint32_t m, uint32_t E) {
  if (m == 0u) return 0.f;
  const int p = 31 - __builtin_clz(m);  // 0..7
  const int be = p + (int)E - 9;        // biased fp32 exponent of m * 2^(E - 136); <= 253
  if (be >= 1) return __uint_as_float(((uint32_t)be << 23) | ((m << (23 - p)) & 0x7FFFFFu));
  return __uint_as_float(m << (E + 13u));  // denormal: m * 2^(E - 136) = (m << (E + 13)) * 2^-149
}

// channel ch (0..2) of the pixel code q
__device__ __forceinline__ float decode_ch(uint32_t q, int ch) {
  const uint32_t E = q >> 24;
  return E == 0u ? 0.f : decode_c((q >> (8 * ch)) & 255u, E);
}
