// Per-value pieces of the HDR quality metrics (hdrmetrics.hip): the perceptual encodings of a
// display-referred luminance x in cd/m^2, and the histogram bin of a luminance.  Float64 with no
// FMA contraction, like tonemap_px.h, so that the numpy restatement rounds the same way.
#pragma once
#include "common.h"

// The pragma holds to the end of the including file, which its user wants.
#pragma clang fp contract(off)

#define HDR_ENC_PQ 0
#define HDR_ENC_LOG 1

constexpr double HDR_PEAK = 1e4;         // cd/m^2: the top of both encodings
constexpr double HDR_LOG_FLOOR = 0.005;  // cd/m^2: the bottom of the log encoding

// SMPTE ST 2084 (every constant is exact in binary)
constexpr double PQ_M1 = 2610.0 / 16384.0;
constexpr double PQ_M2 = 2523.0 / 4096.0 * 128.0;
constexpr double PQ_C1 = 3424.0 / 4096.0;
constexpr double PQ_C2 = 2413.0 / 4096.0 * 32.0;
constexpr double PQ_C3 = 2392.0 / 4096.0 * 32.0;

// NaN and negatives -> E(0) (C fmax / fmin return the operand that is a number), +inf -> 1
__device__ __forceinline__ float pq_encode(double x) {
  const double L = fmin(fmax(x, 0.0), HDR_PEAK);
  const double yp = pow(L / HDR_PEAK, PQ_M1);
  return (float)pow((PQ_C1 + PQ_C2 * yp) / (1.0 + PQ_C3 * yp), PQ_M2);
}

// log_lo = log10(HDR_LOG_FLOOR) from the same log10 as the value's, so the floor encodes to exactly 0
__device__ __forceinline__ float log_encode(double x, double log_lo) {
  const double L = fmin(fmax(x, HDR_LOG_FLOOR), HDR_PEAK);
  return (float)((log10(L) - log_lo) / (4.0 - log_lo));
}

// Luminance histogram on the float bits: 64 octaves [2^-32, 2^32) x 64 bins per octave (the top
// 6 mantissa bits).  Below 2^-32, zero, negatives and NaN -> bin 0; 2^32 and above (+inf) -> the
// last bin.  The upper edge of bin b is the float with the bits (b + 1 + LUM_BIN_BASE) << 17.
constexpr int LUM_BINS = 4096;
constexpr uint32_t LUM_BIN_BASE = 0x2F800000u >> 17;  // bits(2^-32f) >> 17

__device__ __forceinline__ int lum_bin(double Y) {
  const uint32_t u = __float_as_uint((float)Y);
  if (u > 0x7F800000u) return 0;  // sign bit set, or a positive NaN
  const uint32_t k = u >> 17;
  if (k < LUM_BIN_BASE) return 0;
  return k - LUM_BIN_BASE > (uint32_t)(LUM_BINS - 1) ? LUM_BINS - 1 : (int)(k - LUM_BIN_BASE);
}

__device__ __forceinline__ float lum_bin_upper_edge(int b) {
  return __uint_as_float(((uint32_t)b + 1u + LUM_BIN_BASE) << 17);
}
