// Training pairs straight from HDR pictures: cnnitmo_hdr_pairs.
//
// For every output frame i a descriptor names a source picture (fp32 RGB or RGBE bytes, any size)
// and a clamp window inside it.  Per output pixel (r, c):
//
//   (r', c') = (fv ? h-1-r : r, fh ? w-1-c : c)                 flips as cnnitmo_augment_affine
//   (rin, cin) = mats[i] * (r', c', 1)                          float64, SOURCE-picture coordinates
//   hdr = float32(bilinear(src, rin, cin))                      float64, the four neighbours clamped to
//                                                               the window [r0, r1] x [c0, c1]; an RGBE
//                                                               tap is decoded as cnnitmo_rgbe_decode does
//   Y = lum(hdr);  logsum[i] = sum log(max(Y, realmin));  G = exp(logsum * (1 / (h*w)))
//   target y_c = hdr_c * (L / Y),  X = key/G * Y,        L = X / (1 + X)                     (Reinhard.m)
//   input  x_c = hdr_c * (L / Y),  X = cam[i][0]/G * Y,  L = min(1, (1+n) X^y / (n + X^y))   (virtual_camera.m)
//   store: NaN -> 0, clamp to [0, 1]; (float)v, or when quantised (float)uint8(255 v) * (float)(1/255)
//
// The arithmetic after the gather is tonemap.hip's (float64, no FMA contraction); the gather is
// augment.hip's formula.  Contraction is off for the whole file, so the two passes below, which
// both run the gather, get the same float32 pixel: every product and sum is rounded on its own.
//
// Three launches, the warped picture is never stored unless asked for:
//   1. hdr_logsum_partial  grid (PARTS, n): gather, Y, block sum of the logs in a fixed tree
//                          -> part[n][PARTS]                      (reads 4 taps per pixel)
//   2. hdr_logsum_fold     one thread per frame, the PARTS partial sums in index order -> logsum, G
//   3. hdr_pairs_apply     one thread per output pixel: the gather again, both curves from that one
//                          pixel, x / y (/ warped) staged in LDS and stored by consecutive lanes to
//                          consecutive dwords (a wave instruction writes 256 contiguous bytes; a
//                          12-byte pixel per lane would spread it over 768)
// HBM traffic per output pixel: 24 B written (x, y) + the source taps of two gathers.  The taps of
// neighbouring pixels overlap, so a gather reads each source byte of its footprint about once from
// HBM: 2 x 4 B (RGBE) or 2 x 12 B (fp32) at unit zoom -> 32 B / 48 B per pixel, + 12 B with `warped`.
// No atomics: the reduction is a fixed partition and a fixed-order fold, bitwise reproducible.
#include "common.h"
#include "rgbe_px.h"
#include "tonemap_px.h"  // Lum, lum, REALMIN, im2uint8, lum_of

#include <limits.h>

// no FMA contraction: see above
#pragma clang fp contract(off)

namespace {

constexpr int TB = 256;     // threads per block
constexpr int PARTS = 128;  // partial sums per frame

struct Px {
  float r, g, b;
};

// pixel (r, c) of the picture as float64; (r, c) is inside it
__device__ __forceinline__ void tap(const cnnitmo_hdr_src& s, int r, int c, double* v) {
  const size_t p = (size_t)r * s.w + c;
  if (s.fmt == 0) {
    const float* q = (const float*)s.pix + 3 * p;
    v[0] = q[0];
    v[1] = q[1];
    v[2] = q[2];
  } else {
    const uint8_t* b = (const uint8_t*)s.pix + 4 * p;
    uint32_t q;
    if (((uintptr_t)s.pix & 3) == 0)
      q = *reinterpret_cast<const uint32_t*>(b);
    else
      q = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    v[0] = decode_ch(q, 0);
    v[1] = decode_ch(q, 1);
    v[2] = decode_ch(q, 2);
  }
}

// the warped HDR pixel of output (r, c) of an h x w frame
__device__ __forceinline__ Px gather(const cnnitmo_hdr_src& s, const double* __restrict__ m, int fl, int h, int w,
                                     int r, int c) {
  if (fl & 2) r = h - 1 - r;  // flip_vertical (row axis)
  if (fl & 1) c = w - 1 - c;  // flip_horizontal (column axis)
  const double rin = m[0] * r + m[1] * c + m[2];
  const double cin = m[3] * r + m[4] * c + m[5];
  const double rf = floor(rin), cf = floor(cin);
  const double fr = rin - rf, fc = cin - cf;
  // clamp-to-edge neighbours (mode 'nearest') of the window; coordinates beyond +-2^30 saturate.
  // The window is cut to the picture here as well: no descriptor can send a tap outside it.
  const long ri = (long)fmin(fmax(rf, -1073741824.0), 1073741824.0);
  const long ci = (long)fmin(fmax(cf, -1073741824.0), 1073741824.0);
  const long wr0 = max(s.r0, 0), wr1 = min(max(s.r1, 0), s.h - 1);
  const long wc0 = max(s.c0, 0), wc1 = min(max(s.c1, 0), s.w - 1);
  const int ra = (int)min(max(ri, wr0), wr1), rb = (int)min(max(ri + 1, wr0), wr1);
  const int ca = (int)min(max(ci, wc0), wc1), cb = (int)min(max(ci + 1, wc0), wc1);
  double p00[3], p01[3], p10[3], p11[3];
  tap(s, ra, ca, p00);
  tap(s, ra, cb, p01);
  tap(s, rb, ca, p10);
  tap(s, rb, cb, p11);
  float o[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double top = (1.0 - fc) * p00[k] + fc * p01[k];
    const double bot = (1.0 - fc) * p10[k] + fc * p11[k];
    o[k] = (float)((1.0 - fr) * top + fr * bot);
  }
  return Px{o[0], o[1], o[2]};
}

__global__ __launch_bounds__(TB) void hdr_logsum_partial(const cnnitmo_hdr_src* __restrict__ srcs, int h, int w,
                                                         const double* __restrict__ mats,
                                                         const int* __restrict__ flips, Lum lc,
                                                         double* __restrict__ part) {
  const int im = blockIdx.y;
  const cnnitmo_hdr_src s = srcs[im];
  const double* m = mats + 6 * (long)im;
  const int fl = flips[im];
  const long hw = (long)h * w;
  double acc = 0.0;
  for (long p = (long)blockIdx.x * TB + threadIdx.x; p < hw; p += (long)PARTS * TB) {
    const int r = (int)(p / w), c = (int)(p - (long)r * w);
    const Px v = gather(s, m, fl, h, w, r, c);
    acc += log(fmax(lum(lc, v.r, v.g, v.b), REALMIN));
  }
  // The tree is written out, not reduce.h's tree_sum (same additions): with it cnnitmo_hdr_pairs on
  // [32,512,512,3] measured a median of 0.2945 ms where this loop's slower median was 0.2926 ms and
  // its own two medians 0.0008 ms apart (tools/hdrgen_timing.py).
  __shared__ double sh[TB];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = TB / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(long)im * PARTS + blockIdx.x] = sh[0];
}

// logsum[im] and G[im] = exp(logsum / (h*w)); logsum_out: the caller's array, may be null
__global__ void hdr_logsum_fold(const double* __restrict__ part, int n, double inv_hw, double* __restrict__ G,
                                double* __restrict__ logsum_out) {
  const int im = blockIdx.x * blockDim.x + threadIdx.x;
  if (im >= n) return;
  double s = 0.0;
  for (int b = 0; b < PARTS; ++b) s += part[(long)im * PARTS + b];
  G[im] = exp(s * inv_hw);
  if (logsum_out) logsum_out[im] = s;
}

__device__ __forceinline__ float finish(double v, bool quant) {
  v = v != v ? 0.0 : fmin(fmax(v, 0.0), 1.0);
  return quant ? (float)im2uint8(v) * (float)(1 / 255.) : (float)v;
}

// the first nfl floats of the block's staged tile to dst: lane j -> dword j
__device__ __forceinline__ void store_tile(float* __restrict__ dst, const float* tile, int nfl) {
  for (int j = threadIdx.x; j < nfl; j += TB) dst[j] = tile[j];
}

__global__ __launch_bounds__(TB) void hdr_pairs_apply(const cnnitmo_hdr_src* __restrict__ srcs, int h, int w,
                                                      const double* __restrict__ mats,
                                                      const int* __restrict__ flips, Lum lc, double key,
                                                      const double* __restrict__ cam,
                                                      const double* __restrict__ G, int quantize,
                                                      float* __restrict__ x, float* __restrict__ y,
                                                      float* __restrict__ warped, long total) {
  __shared__ float sx[3 * TB], sy[3 * TB], sw[3 * TB];
  const long base = (long)blockIdx.x * TB;
  const long i = base + threadIdx.x;
  if (i < total) {
    const long hw = (long)h * w;
    const int im = (int)(i / hw);
    const long rem = i - (long)im * hw;
    const int r = (int)(rem / w), c = (int)(rem - (long)r * w);
    const cnnitmo_hdr_src s = srcs[im];
    const Px v = gather(s, mats + 6 * (long)im, flips[im], h, w, r, c);
    const double R = v.r, Gc = v.g, B = v.b;
    const double Y = lum(lc, R, Gc, B);
    const double g = G[im];
    // target: Reinhard.m
    const double Xt = (key / g) * Y;
    const double ft = (Xt / (1.0 + Xt)) / Y;
    // input: virtual_camera.m
    const double cn = cam[3 * (long)im + 1], cy = cam[3 * (long)im + 2];
    const double Xc = (cam[3 * (long)im] / g) * Y;
    const double Xy = pow(Xc, cy);
    const double fx = fmin(1.0, (1.0 + cn) * (Xy / (cn + Xy))) / Y;
    const int t = 3 * threadIdx.x;
    sx[t] = finish(R * fx, quantize & 1);
    sx[t + 1] = finish(Gc * fx, quantize & 1);
    sx[t + 2] = finish(B * fx, quantize & 1);
    sy[t] = finish(R * ft, quantize & 2);
    sy[t + 1] = finish(Gc * ft, quantize & 2);
    sy[t + 2] = finish(B * ft, quantize & 2);
    if (warped) {
      sw[t] = v.r;
      sw[t + 1] = v.g;
      sw[t + 2] = v.b;
    }
  }
  __syncthreads();
  const long left = total - base;
  const int nfl = 3 * (int)(left < TB ? left : TB);
  store_tile(x + 3 * base, sx, nfl);
  store_tile(y + 3 * base, sy, nfl);
  if (warped) store_tile(warped + 3 * base, sw, nfl);
}

}  // namespace

// part [n][PARTS], then G [n]
extern "C" size_t cnnitmo_hdr_pairs_workspace_bytes(int n) {
  return n > 0 ? (size_t)n * (PARTS + 1) * sizeof(double) : 0;
}

extern "C" int cnnitmo_hdr_pairs(const cnnitmo_hdr_src* srcs, int n, int h, int w, const double* mats,
                                 const int* flips, const double* lum_coef, double key, const double* cam,
                                 int quantize, float* x, float* y, float* warped, double* logsum, void* workspace,
                                 size_t ws_bytes, void* stream) {
  CNN_REQUIRE(srcs && mats && flips && cam && x && y && workspace, "hdr_pairs: null pointer");
  CNN_REQUIRE(n > 0 && h > 0 && w > 0, "hdr_pairs: bad shape %d x %d x %d", n, h, w);
  CNN_REQUIRE(n <= 65535, "hdr_pairs: n %d > 65535 frames", n);
  CNN_REQUIRE((long)h * w <= INT_MAX && (long)n * h * w < (1L << 38), "hdr_pairs: too large");
  CNN_REQUIRE((quantize & ~3) == 0, "hdr_pairs: quantize %d", quantize);
  CNN_REQUIRE(ws_bytes >= cnnitmo_hdr_pairs_workspace_bytes(n), "hdr_pairs: workspace too small");
  CNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "hdr_pairs: workspace is not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const Lum lc = lum_of(lum_coef);
  double* part = (double*)workspace;
  double* G = part + (size_t)n * PARTS;
  const long hw = (long)h * w, total = (long)n * hw;
  hipLaunchKernelGGL(hdr_logsum_partial, dim3(PARTS, n), dim3(TB), 0, s, srcs, h, w, mats, flips, lc, part);
  hipLaunchKernelGGL(hdr_logsum_fold, dim3((n + 63) / 64), dim3(64), 0, s, (const double*)part, n,
                     1.0 / (double)hw, G, logsum);
  hipLaunchKernelGGL(hdr_pairs_apply, dim3((unsigned)((total + TB - 1) / TB)), dim3(TB), 0, s, srcs, h, w, mats,
                     flips, lc, key, cam, (const double*)G, quantize, x, y, warped, total);
  return cnnitmo_check_launch("hdr_pairs");
}
