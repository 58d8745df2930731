// HDR quality metrics: the two maps that put a linear-radiance image in front of the PSNR / SSIM
// kernel of metrics.hip (cnnitmo_hdr_encode, cnnitmo_lum_percentile).
//
//   encode, per channel value v of image i of [n][h][w][3] fp32:
//     x = (double)v * scale[i]                            (scale: cd/m^2 per unit, per image)
//     PQ  (SMPTE ST 2084): L = fmin(fmax(x, 0), 1e4), y = L / 1e4,
//                          E = pow((c1 + c2 y^m1) / (1 + c3 y^m1), m2)
//     log:                 L = fmin(fmax(x, 0.005), 1e4),
//                          E = (log10 L - log10 0.005) / (4 - log10 0.005)
//     out = (float)E.  NaN and negatives encode like 0 (like 0.005), +inf like 1e4.
//   percentile Q_q of the luminance Y (tonemap_px.h's lum) of each image, on the float bits of
//     (float)Y: a 4096-bin histogram (hdr_px.h's lum_bin: 64 octaves x 64 bins), need =
//     max(1, ceil(q h w)), b = the first bin whose cumulative count reaches need, Q = the upper
//     edge of b.  So Q >= the true order statistic, by less than a factor 1 + 1/64.
//
// The encode is elementwise: a thread takes 16 bytes when 3*h*w % 4 == 0 and both bases are
// 16-byte aligned (the four values then belong to one image), one value otherwise; every element
// of out is written exactly once.  It is not fused into the staging of ssim_tile.h: a tile stages
// 26 x 80 elements for 16 x 48 outputs, so the two fp64 pow per element would run 2.7x as often.
//
// The histogram: a workgroup counts its pixels in LDS (4096 x 4 B), then adds its non-empty bins to
// the image's histogram in the workspace with integer atomics; the entry point zeroes the workspace
// first.  One workgroup per image then scans the 4096 counts.  Integer counts: the result does not
// depend on the order of the atomics, two runs are bitwise equal.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "tonemap_px.h"  // Lum, lum, lum_of
#include "hdr_px.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr long HIST_PIX_PER_BLK = 8192;  // pixels a histogram workgroup takes at least ...
constexpr long HIST_MAX_BLK = 128;       // ... unless that needs more workgroups per image than this
constexpr long MAX_GRID = 0x7FFFFFFFL;

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int ENC> __device__ __forceinline__ float encode_value(float v, double scale, double log_lo) {
  const double x = (double)v * scale;
  return ENC == HDR_ENC_PQ ? pq_encode(x) : log_encode(x, log_lo);
}

// len = 3*h*w values per image, total = n*len.  VEC: len % 4 == 0, 16-byte aligned bases, a thread
// takes values 4t .. 4t+3; else value t.  log_floor = HDR_LOG_FLOOR (an argument, so that its log10
// is the device's own).
template <int ENC, bool VEC>
__global__ __launch_bounds__(NT) void hdr_encode_kernel(const float* __restrict__ img, long len, long total,
                                                        const double* __restrict__ scale, double log_floor,
                                                        float* __restrict__ out) {
  const long i = ((long)blockIdx.x * NT + threadIdx.x) * (VEC ? 4 : 1);
  if (i >= total) return;
  const double sc = scale[i / len];
  const double log_lo = ENC == HDR_ENC_LOG ? log10(log_floor) : 0.0;
  if (VEC) {
    const float4 v = *reinterpret_cast<const float4*>(img + i);
    float4 e;
    e.x = encode_value<ENC>(v.x, sc, log_lo);
    e.y = encode_value<ENC>(v.y, sc, log_lo);
    e.z = encode_value<ENC>(v.z, sc, log_lo);
    e.w = encode_value<ENC>(v.w, sc, log_lo);
    *reinterpret_cast<float4*>(out + i) = e;
  } else {
    out[i] = encode_value<ENC>(img[i], sc, log_lo);
  }
}

__global__ __launch_bounds__(NT) void hist_zero_kernel(unsigned* __restrict__ hist, long count) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i < count) hist[i] = 0u;
}

// grid (blocks per image, n); hist [n][LUM_BINS].  VEC: h*w % 4 == 0 and a 16-byte aligned img: four
// pixels = three 16-byte loads.
template <bool VEC>
__global__ __launch_bounds__(NT) void lum_hist_kernel(const float* __restrict__ img, long hw, Lum lc,
                                                      unsigned* __restrict__ hist) {
  __shared__ unsigned sh[LUM_BINS];
  for (int b = threadIdx.x; b < LUM_BINS; b += NT) sh[b] = 0u;
  __syncthreads();
  const float* base = img + (long)blockIdx.y * hw * 3;
  const long first = (long)blockIdx.x * NT + threadIdx.x, step = (long)gridDim.x * NT;
  if (VEC) {
    for (long g = first; g < hw / 4; g += step) {
      const float4* src = reinterpret_cast<const float4*>(base) + 3 * g;
      const float4 a = src[0], b = src[1], c = src[2];
      atomicAdd(&sh[lum_bin(lum(lc, a.x, a.y, a.z))], 1u);
      atomicAdd(&sh[lum_bin(lum(lc, a.w, b.x, b.y))], 1u);
      atomicAdd(&sh[lum_bin(lum(lc, b.z, b.w, c.x))], 1u);
      atomicAdd(&sh[lum_bin(lum(lc, c.y, c.z, c.w))], 1u);
    }
  } else {
    for (long p = first; p < hw; p += step) {
      const float* q = base + 3 * p;
      atomicAdd(&sh[lum_bin(lum(lc, q[0], q[1], q[2]))], 1u);
    }
  }
  __syncthreads();
  unsigned* dst = hist + (long)blockIdx.y * LUM_BINS;
  for (int b = threadIdx.x; b < LUM_BINS; b += NT)
    if (sh[b] != 0u) atomicAdd(&dst[b], sh[b]);
}

// one workgroup per image: thread t owns the bins [16 t, 16 t + 16); the thread whose range holds the
// first bin with a cumulative count >= need writes that bin's upper edge
__global__ __launch_bounds__(NT) void lum_scan_kernel(const unsigned* __restrict__ hist, unsigned need,
                                                      float* __restrict__ out) {
  constexpr int PER = LUM_BINS / NT;
  __shared__ unsigned part[NT];
  const unsigned* h = hist + (long)blockIdx.x * LUM_BINS + threadIdx.x * PER;
  unsigned c[PER], own = 0u;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = h[j];
    own += c[j];
  }
  part[threadIdx.x] = own;
  __syncthreads();
  unsigned before = 0u;
  for (int t = 0; t < (int)threadIdx.x; ++t) before += part[t];
  if (before < need && need <= before + own) {
    int b = PER - 1;
    unsigned cum = before;
    bool found = false;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      cum += c[j];
      if (!found && cum >= need) {
        b = j;
        found = true;
      }
    }
    out[blockIdx.x] = lum_bin_upper_edge((int)threadIdx.x * PER + b);
  } else if (threadIdx.x == NT - 1 && before + own < need) {
    out[blockIdx.x] = lum_bin_upper_edge(LUM_BINS - 1);  // need > h*w: not reachable from the entry point
  }
}

}  // namespace

extern "C" int cnnitmo_hdr_encode(int encoding, const float* img, int n, int h, int w, const double* scale,
                                  float* out, void* stream) {
  CNN_REQUIRE(img && scale && out, "hdr_encode: null pointer");
  CNN_REQUIRE(encoding == HDR_ENC_PQ || encoding == HDR_ENC_LOG, "hdr_encode: encoding %d (0 = PQ, 1 = log)",
              encoding);
  CNN_REQUIRE(n > 0 && h > 0 && w > 0, "hdr_encode: bad shape n=%d h=%d w=%d", n, h, w);
  CNN_REQUIRE(((uintptr_t)img & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)scale & 7) == 0,
              "hdr_encode: misaligned pointer");
  const long len = 3L * h * w, total = (long)n * len;
  const bool vec = len % 4 == 0 && aligned16(img) && aligned16(out);
  const long blocks = ((vec ? total / 4 : total) + NT - 1) / NT;
  CNN_REQUIRE(blocks <= MAX_GRID, "hdr_encode: %d images of %d x %d are too many values", n, h, w);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(NT);
  if (encoding == HDR_ENC_PQ) {
    if (vec)
      hipLaunchKernelGGL((hdr_encode_kernel<HDR_ENC_PQ, true>), grid, block, 0, s, img, len, total, scale,
                         HDR_LOG_FLOOR, out);
    else
      hipLaunchKernelGGL((hdr_encode_kernel<HDR_ENC_PQ, false>), grid, block, 0, s, img, len, total, scale,
                         HDR_LOG_FLOOR, out);
  } else {
    if (vec)
      hipLaunchKernelGGL((hdr_encode_kernel<HDR_ENC_LOG, true>), grid, block, 0, s, img, len, total, scale,
                         HDR_LOG_FLOOR, out);
    else
      hipLaunchKernelGGL((hdr_encode_kernel<HDR_ENC_LOG, false>), grid, block, 0, s, img, len, total, scale,
                         HDR_LOG_FLOOR, out);
  }
  return cnnitmo_check_launch("hdr_encode");
}

extern "C" long cnnitmo_lum_percentile_workspace_bytes(int n) {
  return n <= 0 ? 0 : (long)n * LUM_BINS * (long)sizeof(unsigned);
}

extern "C" int cnnitmo_lum_percentile(const float* img, int n, int h, int w, const double* lum_coef, double q,
                                      float* out, void* workspace, long workspace_bytes, void* stream) {
  CNN_REQUIRE(img && out && workspace, "lum_percentile: null pointer");
  CNN_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0, "lum_percentile: bad shape n=%d h=%d w=%d", n, h, w);
  CNN_REQUIRE((long)h * w < (1L << 31), "lum_percentile: image %d x %d too large", h, w);
  CNN_REQUIRE(q > 0.0 && q <= 1.0, "lum_percentile: q %g outside (0, 1]", q);  // (also NaN)
  CNN_REQUIRE(((uintptr_t)img & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
              "lum_percentile: misaligned pointer");
  CNN_REQUIRE(workspace_bytes >= cnnitmo_lum_percentile_workspace_bytes(n),
              "lum_percentile: workspace too small (%ld < %ld bytes)", workspace_bytes,
              cnnitmo_lum_percentile_workspace_bytes(n));
  hipStream_t s = (hipStream_t)stream;
  unsigned* hist = (unsigned*)workspace;
  const long hw = (long)h * w, count = (long)n * LUM_BINS;
  const double need_d = ceil(q * (double)h * (double)w);
  const unsigned need = need_d < 1.0 ? 1u : (unsigned)need_d;  // <= h*w < 2^31
  const long blk = std::min(HIST_MAX_BLK, (hw + HIST_PIX_PER_BLK - 1) / HIST_PIX_PER_BLK);
  const Lum lc = lum_of(lum_coef);
  hipLaunchKernelGGL(hist_zero_kernel, dim3((unsigned)((count + NT - 1) / NT)), dim3(NT), 0, s, hist, count);
  if (hw % 4 == 0 && aligned16(img))
    hipLaunchKernelGGL(lum_hist_kernel<true>, dim3((unsigned)blk, n), dim3(NT), 0, s, img, hw, lc, hist);
  else
    hipLaunchKernelGGL(lum_hist_kernel<false>, dim3((unsigned)blk, n), dim3(NT), 0, s, img, hw, lc, hist);
  hipLaunchKernelGGL(lum_scan_kernel, dim3(n), dim3(NT), 0, s, (const unsigned*)hist, need, out);
  return cnnitmo_check_launch("lum_percentile");
}
