// Per-pixel pieces of the tone-mapping maps shared by tonemap.hip and hdrpairs.hip: the luminance,
// MATLAB's realmin and imwrite's double -> uint8.  Float64 like MATLAB's doubles.
#pragma once
#include "common.h"

// no FMA contraction: the products and sums round like MATLAB's (and numpy's) doubles.  The pragma
// holds to the end of the including file, which both users want.
#pragma clang fp contract(off)

constexpr double REALMIN = 2.2250738585072014e-308;

struct Lum {
  double r, g, b;
};

__device__ __forceinline__ double lum(const Lum& c, double R, double G, double B) { return c.r * R + c.g * G + c.b * B; }

// MATLAB uint8(255*x): round half away from zero, saturate, NaN -> 0
__device__ __forceinline__ uint8_t im2uint8(double x) {
  const double v = 255.0 * x;
  if (!(v > 0.0)) return 0;  // also NaN
  if (v >= 255.0) return 255;
  return (uint8_t)floor(v + 0.5);
}

// host: the three weights of RGB2Lum, NULL = Rec. 709
static inline Lum lum_of(const double* c) { return c ? Lum{c[0], c[1], c[2]} : Lum{0.2126, 0.7152, 0.0722}; }
