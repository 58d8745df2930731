// Radiance RGBE (shared-exponent) pixel codec: cnnitmo_rgbe_encode / cnnitmo_rgbe_decode.
//
//   encode, per pixel of [npix][3] fp32:
//     NaN -> 0, each component clamped to [0, 255 * 2^119] (the largest RGBE value);
//     v = max(r, g, b); v < 1e-32f -> (0, 0, 0, 0); else frexpf(v) = (m, e),
//     mantissa_c = floor(ldexpf(c, 8 - e)), exponent byte = e + 128.
//   decode, per pixel of [npix][4] bytes:
//     E = 0 -> (0, 0, 0); else c = (float)mantissa_c * 2^(E - 136)   (no +0.5: rgbe.c / hdrread).
//
// Both maps are exact (a scaling by a power of two and a floor), so they are done on the bit
// patterns: no rounding mode, contraction or denormal mode of the float unit can change a result.
//   encode: a positive fp32 is ordered like its bit pattern, so the NaN / sign / clamp tests and the
//     maximum are integer compares.  v >= 1e-32f is normal: e = (bits(v) >> 23) - 126.  A normal
//     c = s * 2^(bc - 150), s = 2^23 | frac, so c * 2^(8 - e) = s >> (bv - bc + 16) floored (0 once
//     the shift passes 24 bits); a denormal c is < 2^-126 and v >= 2^-107, so it floors to 0.
//   decode: m * 2^(E - 136) with the top set bit p of m has the biased exponent p + E - 9; below 1
//     the value is the denormal m << (E + 13) (E = 1, and small mantissas up to E = 9), which is
//     written as such, never flushed.
//
// HBM-bound, 16 B per pixel.  Encode: a thread takes four pixels -- three 16-byte loads and one
// 16-byte store (the loads of a wave are 48 B apart, but its three loads share their cache lines).
// Decode writes 12 of the 16 bytes, and the mirror image (one 16-byte load, three 16-byte stores
// 48 B apart per thread) scatters every store instruction of a wave over 64 separate 16-byte
// pieces: measured at 8 x 1080 x 1920 it ran at 0.7x the one-pixel path.  So decode keeps three
// 16-byte stores per thread but deals them out by destination: a workgroup owns 1024 pixels =
// 768 float4 of output, and store k of thread t is float4 k*256 + t, contiguous over the
// workgroup; the four floats of an output float4 come from two neighbouring pixel codes, read as
// two dwords (4 B per pixel of cached reads).  The npix % 4 tail, and every pixel when a pointer
// is not 16-byte aligned (nvec = 0), take the one-pixel path of the same kernel; all paths call
// the same per-component functions, so they give the same bytes.
#include "common.h"
#include "rgbe_px.h"

namespace {

constexpr int NT = 256;
constexpr uint32_t MAX_BITS = 0x7EFF0000u;   // 255 * 2^119 = 1.9921875 * 2^126
constexpr uint32_t TINY_BITS = 0x0A4FB11Fu;  // 1e-32f

// NaN, negatives and -0 -> 0; above the RGBE range (inf included) -> 255 * 2^119
__device__ __forceinline__ uint32_t clamp_bits(float c) {
  const uint32_t u = __float_as_uint(c);
  if (u > 0x7F800000u) return 0u;  // sign bit set, or a positive NaN
  return u > MAX_BITS ? MAX_BITS : u;
}

__device__ __forceinline__ uint32_t mant_of(uint32_t u, uint32_t bv) {
  const uint32_t bc = u >> 23;
  const uint32_t sh = bv - bc + 16u;  // bc <= bv: u <= v
  if (bc == 0u || sh >= 24u) return 0u;
  return ((u & 0x7FFFFFu) | 0x800000u) >> sh;
}

// one pixel -> r | g << 8 | b << 16 | e << 24 (the bytes in memory order)
__device__ __forceinline__ uint32_t encode_px(float r, float g, float b) {
  const uint32_t ur = clamp_bits(r), ug = clamp_bits(g), ub = clamp_bits(b);
  uint32_t v = ur > ug ? ur : ug;
  v = v > ub ? v : ub;
  if (v < TINY_BITS) return 0u;
  const uint32_t bv = v >> 23;  // e = bv - 126, exponent byte = bv + 2 (<= 255: bv <= 253)
  return mant_of(ur, bv) | (mant_of(ug, bv) << 8) | (mant_of(ub, bv) << 16) | ((bv + 2u) << 24);
}

// decode_c / decode_ch: rgbe_px.h

__device__ __forceinline__ void decode_px(uint32_t q, float& r, float& g, float& b) {
  r = decode_ch(q, 0);
  g = decode_ch(q, 1);
  b = decode_ch(q, 2);
}

// threads [0, nvec): pixels 4i .. 4i+3 with 16-byte accesses; threads [nvec, nvec + npix - 4 nvec):
// one pixel each
__global__ __launch_bounds__(NT) void rgbe_encode_kernel(const float* __restrict__ rgb, uint8_t* __restrict__ rgbe,
                                                         long nvec, long npix) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i < nvec) {
    const float4* src = reinterpret_cast<const float4*>(rgb) + 3 * i;
    const float4 a = src[0], b = src[1], c = src[2];
    uint4 q;
    q.x = encode_px(a.x, a.y, a.z);
    q.y = encode_px(a.w, b.x, b.y);
    q.z = encode_px(b.z, b.w, c.x);
    q.w = encode_px(c.y, c.z, c.w);
    reinterpret_cast<uint4*>(rgbe)[i] = q;
    return;
  }
  const long p = 4 * nvec + (i - nvec);
  if (p >= npix) return;
  const uint32_t q = encode_px(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
  if (((uintptr_t)rgbe & 3) == 0) {
    reinterpret_cast<uint32_t*>(rgbe)[p] = q;
  } else {
    rgbe[4 * p] = (uint8_t)q;
    rgbe[4 * p + 1] = (uint8_t)(q >> 8);
    rgbe[4 * p + 2] = (uint8_t)(q >> 16);
    rgbe[4 * p + 3] = (uint8_t)(q >> 24);
  }
}

// workgroups [0, vblocks): float4 j = blockIdx * 768 + k * 256 + thread, k < 3, of the 3 * nvec output
// float4 of the first 4 * nvec pixels; its floats 4j .. 4j+3 are channels c0 .. c0+3 counted from pixel
// p0 = 4j / 3, i.e. of pixels p0 and p0 + 1 (<= 4 nvec - 1, since 4j + 3 <= 12 nvec - 1).
// Threads of the workgroups after those: one pixel each, from pixel 4 * nvec on.
__global__ __launch_bounds__(NT) void rgbe_decode_kernel(const uint8_t* __restrict__ rgbe, float* __restrict__ rgb,
                                                         long nvec, long vblocks, long npix) {
  if ((long)blockIdx.x < vblocks) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(rgbe);
    float4* dst = reinterpret_cast<float4*>(rgb);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int jl = k * NT + (int)threadIdx.x;  // within the workgroup's 3 * NT float4 = 4 * NT pixels
      const long j = (long)blockIdx.x * (3 * NT) + jl;
      if (j >= 3 * nvec) break;
      const long p0 = (long)blockIdx.x * (4 * NT) + (4 * jl) / 3;
      const int c0 = (4 * jl) % 3;
      const uint32_t q0 = src[p0], q1 = src[p0 + 1];
      float v[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int ch = c0 + t;
        v[t] = ch < 3 ? decode_ch(q0, ch) : decode_ch(q1, ch - 3);
      }
      dst[j] = make_float4(v[0], v[1], v[2], v[3]);
    }
    return;
  }
  const long i = ((long)blockIdx.x - vblocks) * NT + threadIdx.x;
  const long p = 4 * nvec + i;
  if (p >= npix) return;
  uint32_t q;
  if (((uintptr_t)rgbe & 3) == 0)
    q = reinterpret_cast<const uint32_t*>(rgbe)[p];
  else
    q = (uint32_t)rgbe[4 * p] | ((uint32_t)rgbe[4 * p + 1] << 8) | ((uint32_t)rgbe[4 * p + 2] << 16) |
        ((uint32_t)rgbe[4 * p + 3] << 24);
  float r, g, b;
  decode_px(q, r, g, b);
  rgb[3 * p] = r;
  rgb[3 * p + 1] = g;
  rgb[3 * p + 2] = b;
}

// groups of four pixels that take the 16-byte path
long vec_groups(const void* a, const void* b, long npix) {
  return ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) ? npix / 4 : 0;
}

constexpr long MAX_GRID = 0x7FFFFFFFL;

}  // namespace

extern "C" int cnnitmo_rgbe_encode(const float* rgb, long npix, uint8_t* rgbe, void* stream) {
  CNN_REQUIRE(rgb && rgbe, "rgbe_encode: null pointer");
  CNN_REQUIRE(npix > 0, "rgbe_encode: npix %ld", npix);
  CNN_REQUIRE(((uintptr_t)rgb & 3) == 0, "rgbe_encode: rgb is not 4-byte aligned");
  const long nvec = vec_groups(rgb, rgbe, npix);
  const long blocks = (nvec + (npix - 4 * nvec) + NT - 1) / NT;  // one thread per group, then per pixel
  CNN_REQUIRE(blocks <= MAX_GRID, "rgbe_encode: npix %ld too large", npix);
  hipLaunchKernelGGL(rgbe_encode_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, rgb, rgbe, nvec,
                     npix);
  return cnnitmo_check_launch("rgbe_encode");
}

extern "C" int cnnitmo_rgbe_decode(const uint8_t* rgbe, long npix, float* rgb, void* stream) {
  CNN_REQUIRE(rgb && rgbe, "rgbe_decode: null pointer");
  CNN_REQUIRE(npix > 0, "rgbe_decode: npix %ld", npix);
  CNN_REQUIRE(((uintptr_t)rgb & 3) == 0, "rgbe_decode: rgb is not 4-byte aligned");
  const long nvec = vec_groups(rgb, rgbe, npix);
  const long vblocks = (nvec + NT - 1) / NT;  // NT groups = 3 * NT output float4 per workgroup
  const long blocks = vblocks + ((npix - 4 * nvec) + NT - 1) / NT;
  CNN_REQUIRE(blocks <= MAX_GRID, "rgbe_decode: npix %ld too large", npix);
  hipLaunchKernelGGL(rgbe_decode_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, rgbe, rgb, nvec,
                     vblocks, npix);
  return cnnitmo_check_launch("rgbe_decode");
}
