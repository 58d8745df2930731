// Per-pixel pieces of the sensor-noise model shared by the kernels of hdrpairs.hip: the counter-based
// generator Philox4x64-10 (Salmon et al. 2011, numpy's np.random.Philox), the Box-Muller normals of
// one pixel and the Poisson-Gaussian noise law.  Integers and float64, plain C++.
//
// Counter convention.  The block of pixel p = r * w + c of a frame is
//   philox(counter = (p + 1, 0, 0, 0), key = (k0, k1)),
// which is row p of np.random.Philox(key=[k0, k1], counter=[0, 0, 0, 0]).random_raw(4 * h * w)
// .reshape(-1, 4): numpy increments the counter before it generates a block.  p < 2^31, so the
// counter never carries into its second word here.  The block depends on the key and on the pixel's
// place in its own frame alone: the same frame gets the same noise at any batch position.
#pragma once
#include "common.h"

// no FMA contraction: every product and sum rounds on its own, as numpy's doubles.  The pragma
// holds to the end of the including file, which the user wants too.
#pragma clang fp contract(off)

struct PhiloxBlock {
  uint64_t v[4];
};

// ten rounds; the key is bumped by the Weyl constants between rounds
__device__ __forceinline__ PhiloxBlock philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0,
                                                     uint64_t k1) {
  constexpr uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
  constexpr uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t hi0 = __umul64hi(M0, c0), lo0 = M0 * c0;
    const uint64_t hi1 = __umul64hi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return PhiloxBlock{{c0, c1, c2, c3}};
}

// sqrt(-2 ln u1) and 2 pi u2 of a pair of raw words: u1 = ((a >> 11) + 1) 2^-53 in (0, 1],
// u2 = (b >> 11) 2^-53 in [0, 1)
__device__ __forceinline__ void box_muller(uint64_t a, uint64_t b, double* radius, double* angle) {
  const double u1 = (double)((a >> 11) + 1) * 0x1p-53;
  const double u2 = (double)(b >> 11) * 0x1p-53;
  *radius = sqrt(-2.0 * log(u1));
  *angle = (2.0 * 3.141592653589793) * u2;
}

// the three standard normals (R, G, B) of pixel p of a frame with key (k0, k1): R and G are the
// cosine and sine branch on the block's words (0, 1), B the cosine branch on the words (2, 3)
__device__ __forceinline__ void sensor_normals(uint64_t k0, uint64_t k1, uint64_t p, double* z) {
  const PhiloxBlock blk = philox4x64_10(p + 1, 0, 0, 0, k0, k1);
  double rad, ang;
  box_muller(blk.v[0], blk.v[1], &rad, &ang);
  z[0] = rad * cos(ang);
  z[1] = rad * sin(ang);
  box_muller(blk.v[2], blk.v[3], &rad, &ang);
  z[2] = rad * cos(ang);
}

// Poisson-Gaussian noise on an exposure e in units of full well: variance a max(e, 0) + b^2
// (a: shot-noise factor, b: read-noise standard deviation), z a standard normal
__device__ __forceinline__ double sensor_noisy(double e, double a, double b, double z) {
  return e + sqrt(a * fmax(e, 0.0) + b * b) * z;
}
