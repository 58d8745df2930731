// Training pairs straight from HDR pictures: cnnitmo_hdr_pairs, cnnitmo_hdr_pairs_sensor and the
// stand-alone cnnitmo_sensor_noise.
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
// cnnitmo_hdr_pairs_sensor, response 1 (a sensor clips every channel at its own full well, so an
// overexposed colour goes to white; the curve above clips the luminance and keeps the hue):
//   e_c  = cam[i][0]/G * hdr_c                                   exposure in units of full well
//   e'_c = max(0, e_c + sqrt(a max(e_c, 0) + b^2) z_c)           only with noise[i] = (a, b) != (0, 0);
//                                                                z from Philox4x64-10, sensor_px.h
//   x_c  = min(1, (1+n) e'_c^y / (n + e'_c^y))                   the same store; y is untouched
// Response 0 without noise is cnnitmo_hdr_pairs, the same instantiation of the same kernel.
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
#include "sensor_px.h"   // sensor_normals, sensor_noisy
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

// the camera curve of virtual_camera.m on one exposure
__device__ __forceinline__ double camera_curve(double X, double cn, double cy) {
  const double Xy = pow(X, cy);
  return fmin(1.0, (1.0 + cn) * (Xy / (cn + Xy)));
}

// RESPONSE 0: the curve acts on the luminance, the three channels share its factor; 1: on every
// channel's own exposure.  NOISY (RESPONSE 1 only): sensor noise on the exposures, noise [n][2] =
// (a, b) and keys [n][2] per frame; a frame with a = b = 0 takes the path without noise.
template <int RESPONSE, bool NOISY>
__global__ __launch_bounds__(TB) void hdr_pairs_apply(const cnnitmo_hdr_src* __restrict__ srcs, int h, int w,
                                                      const double* __restrict__ mats,
                                                      const int* __restrict__ flips, Lum lc, double key,
                                                      const double* __restrict__ cam,
                                                      const double* __restrict__ G, int quantize,
                                                      const double* __restrict__ noise,
                                                      const uint64_t* __restrict__ keys, float* __restrict__ x,
                                                      float* __restrict__ y, float* __restrict__ warped,
                                                      long total) {
  static_assert(RESPONSE == 1 || !NOISY, "the noise model is defined on channel exposures");
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
    const int t = 3 * threadIdx.x;
    if (RESPONSE == 0) {
      const double Xc = (cam[3 * (long)im] / g) * Y;
      const double Xy = pow(Xc, cy);
      const double fx = fmin(1.0, (1.0 + cn) * (Xy / (cn + Xy))) / Y;
      sx[t] = finish(R * fx, quantize & 1);
      sx[t + 1] = finish(Gc * fx, quantize & 1);
      sx[t + 2] = finish(B * fx, quantize & 1);
    } else {
      const double dt = cam[3 * (long)im] / g;
      double e[3] = {dt * R, dt * Gc, dt * B};
      if (NOISY) {
        const double a = noise[2 * (long)im], b = noise[2 * (long)im + 1];
        if (a != 0.0 || b != 0.0) {  // uniform over a frame
          double z[3];
          sensor_normals(keys[2 * (long)im], keys[2 * (long)im + 1], (uint64_t)rem, z);
#pragma unroll
          for (int k = 0; k < 3; ++k) e[k] = fmax(0.0, sensor_noisy(e[k], a, b, z[k]));
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) sx[t + k] = finish(camera_curve(e[k], cn, cy), quantize & 1);
    }
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

// out = (float)sensor_noisy(e, a, b, z) of every channel value, unclamped.  One thread makes the
// three normals of one pixel into LDS; then consecutive lanes take consecutive floats of the block's
// 3 * TB, so a wave instruction reads and writes 256 contiguous bytes.
__global__ __launch_bounds__(TB) void sensor_noise_kernel(const float* __restrict__ e, long hw,
                                                          const double* __restrict__ noise,
                                                          const uint64_t* __restrict__ keys,
                                                          float* __restrict__ out, long total) {
  __shared__ double sz[3 * TB];
  const long base = (long)blockIdx.x * TB;
  const long i = base + threadIdx.x;
  if (i < total) {
    const long im = i / hw;
    double z[3] = {0.0, 0.0, 0.0};
    if (noise[2 * im] != 0.0 || noise[2 * im + 1] != 0.0)
      sensor_normals(keys[2 * im], keys[2 * im + 1], (uint64_t)(i - im * hw), z);
    sz[3 * threadIdx.x] = z[0];
    sz[3 * threadIdx.x + 1] = z[1];
    sz[3 * threadIdx.x + 2] = z[2];
  }
  __syncthreads();
  const long left = total - base;
  const int nfl = 3 * (int)(left < TB ? left : TB);
  for (int j = threadIdx.x; j < nfl; j += TB) {
    const long im = (base + j / 3) / hw;
    const double a = noise[2 * im], b = noise[2 * im + 1];
    const float v = e[3 * base + j];
    out[3 * base + j] = a != 0.0 || b != 0.0 ? (float)sensor_noisy((double)v, a, b, sz[j]) : v;
  }
}

}  // namespace

// part [n][PARTS], then G [n]
extern "C" size_t cnnitmo_hdr_pairs_workspace_bytes(int n) {
  return n > 0 ? (size_t)n * (PARTS + 1) * sizeof(double) : 0;
}

// the three launches of both entry points; `who` names the entry in error messages
static int hdr_pairs_run(const char* who, const cnnitmo_hdr_src* srcs, int n, int h, int w, const double* mats,
                         const int* flips, const double* lum_coef, double key, const double* cam, int quantize,
                         int response, const double* noise, const uint64_t* keys, float* x, float* y, float* warped,
                         double* logsum, void* workspace, size_t ws_bytes, void* stream) {
  CNN_REQUIRE(srcs && mats && flips && cam && x && y && workspace, "%s: null pointer", who);
  CNN_REQUIRE(n > 0 && h > 0 && w > 0, "%s: bad shape %d x %d x %d", who, n, h, w);
  CNN_REQUIRE(n <= 65535, "%s: n %d > 65535 frames", who, n);
  CNN_REQUIRE((long)h * w <= INT_MAX && (long)n * h * w < (1L << 38), "%s: too large", who);
  CNN_REQUIRE((quantize & ~3) == 0, "%s: quantize %d", who, quantize);
  CNN_REQUIRE(response == 0 || response == 1, "%s: response %d", who, response);
  CNN_REQUIRE(!noise || response == 1, "%s: noise needs response 1, the model is defined on channel exposures",
              who);
  CNN_REQUIRE(!noise || keys, "%s: noise without keys", who);
  CNN_REQUIRE((((uintptr_t)noise | (uintptr_t)keys) & 7) == 0, "%s: noise or keys not 8-byte aligned", who);
  CNN_REQUIRE(ws_bytes >= cnnitmo_hdr_pairs_workspace_bytes(n), "%s: workspace too small", who);
  CNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace is not 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const Lum lc = lum_of(lum_coef);
  double* part = (double*)workspace;
  double* G = part + (size_t)n * PARTS;
  const long hw = (long)h * w, total = (long)n * hw;
  hipLaunchKernelGGL(hdr_logsum_partial, dim3(PARTS, n), dim3(TB), 0, s, srcs, h, w, mats, flips, lc, part);
  hipLaunchKernelGGL(hdr_logsum_fold, dim3((n + 63) / 64), dim3(64), 0, s, (const double*)part, n,
                     1.0 / (double)hw, G, logsum);
  auto* apply = response == 0 ? hdr_pairs_apply<0, false> : noise ? hdr_pairs_apply<1, true> : hdr_pairs_apply<1, false>;
  hipLaunchKernelGGL(apply, dim3((unsigned)((total + TB - 1) / TB)), dim3(TB), 0, s, srcs, h, w, mats, flips, lc, key,
                     cam, (const double*)G, quantize, noise, keys, x, y, warped, total);
  return cnnitmo_check_launch(who);
}

extern "C" int cnnitmo_hdr_pairs(const cnnitmo_hdr_src* srcs, int n, int h, int w, const double* mats,
                                 const int* flips, const double* lum_coef, double key, const double* cam,
                                 int quantize, float* x, float* y, float* warped, double* logsum, void* workspace,
                                 size_t ws_bytes, void* stream) {
  return hdr_pairs_run("hdr_pairs", srcs, n, h, w, mats, flips, lum_coef, key, cam, quantize, 0, nullptr, nullptr, x,
                       y, warped, logsum, workspace, ws_bytes, stream);
}

extern "C" int cnnitmo_hdr_pairs_sensor(const cnnitmo_hdr_src* srcs, int n, int h, int w, const double* mats,
                                        const int* flips, const double* lum_coef, double key, const double* cam,
                                        int quantize, int response, const double* noise, const uint64_t* keys,
                                        float* x, float* y, float* warped, double* logsum, void* workspace,
                                        size_t ws_bytes, void* stream) {
  return hdr_pairs_run("hdr_pairs_sensor", srcs, n, h, w, mats, flips, lum_coef, key, cam, quantize, response, noise,
                       keys, x, y, warped, logsum, workspace, ws_bytes, stream);
}

extern "C" int cnnitmo_sensor_noise(const float* e, int n, int h, int w, const double* noise, const uint64_t* keys,
                                    float* out, void* stream) {
  CNN_REQUIRE(e && noise && keys && out, "sensor_noise: null pointer");
  CNN_REQUIRE(n > 0 && h > 0 && w > 0, "sensor_noise: bad shape %d x %d x %d", n, h, w);
  CNN_REQUIRE((long)h * w <= INT_MAX && (long)n * h * w < (1L << 38), "sensor_noise: too large");
  CNN_REQUIRE((((uintptr_t)noise | (uintptr_t)keys) & 7) == 0 && (((uintptr_t)e | (uintptr_t)out) & 3) == 0,
              "sensor_noise: misaligned pointer");
  const long hw = (long)h * w, total = (long)n * hw;
  hipLaunchKernelGGL(sensor_noise_kernel, dim3((unsigned)((total + TB - 1) / TB)), dim3(TB), 0, (hipStream_t)stream,
                     e, hw, noise, keys, out, total);
  return cnnitmo_check_launch("sensor_noise");
}
