// Highlight-weighted training loss of a prediction y against a target t with the mask taken
// from a source image s (all NHWC RGB fp32), per image, with its gradient
// (cnnitmo_highlight_loss_grad).  Per pixel p:
//
//   m   = max(s[p][0], s[p][1], s[p][2])
//   a   = fmin(fmax((m - tau) / (1 - tau), 0), 1)         the soft saturation mask of Eilertsen et al. 2017
//   wgt = 1 + gain a
//   l   = (y-t)^2 ('mse') or |y-t| ('mae'),  l' = 2 (y-t) or sign(y-t), sign(0) = 0
//
// and per image, N = 3 h w:  A = sum_p a / (h w),  B = sum l / N,  L = sum wgt l / N,
// H = sum a l / (3 sum_p a) (0 where no pixel is masked);  dy = (float)((wgt l') / (F N)).
// L is not divided by sum wgt: gain 0 is the base loss, and an unmasked pixel keeps the gradient it
// has under the base loss.
//
// HBM-bound: 36 B read and 12 B written per pixel (36 B without dy).  As in hdrio.hip a thread
// takes four pixels, three 16-byte loads per operand (the three channels of a pixel must be
// together for m) and three 16-byte stores.  A workgroup owns B4 = 4 NT = 1024 consecutive pixels
// of one image (grid y = image), so no workgroup straddles two images.  An image whose base is not
// 16-byte aligned in any operand (h w 3 % 4 != 0 for the images after the first, or a caller's
// view) reads and writes its pixels one float at a time, as do the h w % 4 last pixels of an
// aligned image.  Either way thread i of a workgroup takes the same four pixels in the same order
// through the same per-pixel function, so both paths give the same bits, sums included.
//
// Numerics: fp64 after the loads, no FMA contraction, operations in the order written above.
// Each workgroup writes four fp64 partial sums (fixed tree), highlight_final_kernel folds them per
// image in a fixed order.  No atomics: two runs are bitwise equal.  s may alias t.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int PX = 4;        // pixels per thread
constexpr int B4 = PX * NT;  // pixels per workgroup

struct Sums {
  double a, l, wl, al;
};

// one pixel: adds to the thread's sums; GRAD: g[c] = dy of the three channels
template <bool GRAD>
__device__ __forceinline__ void pixel(const float* s, const float* y, const float* t, int base, double tau,
                                      double den, double gain, double fn, Sums& acc, float* g) {
  const float m = fmaxf(fmaxf(s[0], s[1]), s[2]);
  const double a = fmin(fmax(((double)m - tau) / den, 0.0), 1.0);
  const double wgt = 1.0 + gain * a;
  acc.a += a;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double d = (double)y[c] - (double)t[c];
    double l, lp;
    if (base == CNNITMO_BASE_MSE) {
      l = d * d;
      lp = 2.0 * d;
    } else {
      l = fabs(d);
      lp = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    }
    acc.l += l;
    acc.wl += wgt * l;
    acc.al += a * l;
    if (GRAD) g[c] = (float)((wgt * lp) / fn);
  }
}

// grid (blocks per image, n).  part [n][gridDim.x][4] = the workgroup's sums of (a, l, wgt l, a l)
template <bool GRAD>
__global__ __launch_bounds__(NT) void highlight_kernel(const float* s, const float* y, const float* t, long npix,
                                                       int base, double tau, double den, double gain, double fn,
                                                       double* __restrict__ part, float* dy) {
  __shared__ double sh[4][NT];
  const int tid = threadIdx.x;
  const long img = (long)blockIdx.y * npix * 3;
  const float* si = s + img;
  const float* yi = y + img;
  const float* ti = t + img;
  float* di = GRAD ? dy + img : nullptr;
  const bool vec = (((uintptr_t)si | (uintptr_t)yi | (uintptr_t)ti | (uintptr_t)di) & 15) == 0;
  const long p0 = (long)blockIdx.x * B4 + (long)tid * PX;
  Sums acc = {0.0, 0.0, 0.0, 0.0};
  if (vec && p0 + PX <= npix) {
    float sv[12], yv[12], tv[12], gv[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Pack16<float>::load(si + 3 * p0 + 4 * k, sv + 4 * k);
      Pack16<float>::load(yi + 3 * p0 + 4 * k, yv + 4 * k);
      Pack16<float>::load(ti + 3 * p0 + 4 * k, tv + 4 * k);
    }
#pragma unroll
    for (int q = 0; q < PX; ++q)
      pixel<GRAD>(sv + 3 * q, yv + 3 * q, tv + 3 * q, base, tau, den, gain, fn, acc, gv + 3 * q);
    if (GRAD) {
#pragma unroll
      for (int k = 0; k < 3; ++k) Pack16<float>::store(di + 3 * p0 + 4 * k, gv + 4 * k);
    }
  } else {
    for (int q = 0; q < PX; ++q) {
      const long p = p0 + q;
      if (p >= npix) break;
      float sv[3], yv[3], tv[3], gv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sv[c] = si[3 * p + c];
        yv[c] = yi[3 * p + c];
        tv[c] = ti[3 * p + c];
      }
      pixel<GRAD>(sv, yv, tv, base, tau, den, gain, fn, acc, gv);
      if (GRAD) {
#pragma unroll
        for (int c = 0; c < 3; ++c) di[3 * p + c] = gv[c];
      }
    }
  }
  // The tree here and the fold and tree of highlight_final_kernel are written out, not reduce.h's
  // tree_sum / fold_tree_sum (same additions): with them the call on [8,1080,1920,3] measured medians of
  // 0.1281 and 0.1282 ms where these loops' slower median was 0.1275 ms and their own two medians
  // 0.0004 ms apart (loss only: 0.0874 against 0.0864 ms, 0.0007 ms apart).
  sh[0][tid] = acc.a;
  sh[1][tid] = acc.l;
  sh[2][tid] = acc.wl;
  sh[3][tid] = acc.al;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sh[k][tid] += sh[k][tid + o];
    }
    __syncthreads();
  }
  if (tid < 4) part[((long)blockIdx.y * gridDim.x + blockIdx.x) * 4 + tid] = sh[tid][0];
}

// one workgroup per image: thread i folds the partials of workgroups i, i + NT, ... in order, then a
// fixed tree.  out [n][4] = {A, B, L, H}
__global__ __launch_bounds__(NT) void highlight_final_kernel(const double* __restrict__ part, long nblk, double npix,
                                                             double* __restrict__ out) {
  __shared__ double sh[4][NT];
  const int tid = threadIdx.x;
  const double* pi = part + (long)blockIdx.x * nblk * 4;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (long i = tid; i < nblk; i += NT) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += pi[4 * i + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) sh[k][tid] = v[k];
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sh[k][tid] += sh[k][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double sa = sh[0][0], n_elem = npix * 3.0;
    double* o = out + 4 * (long)blockIdx.x;
    o[0] = sa / npix;
    o[1] = sh[1][0] / n_elem;
    o[2] = sh[2][0] / n_elem;
    o[3] = sa == 0.0 ? 0.0 : sh[3][0] / (3.0 * sa);
  }
}

// workgroups per image; 0 for a shape the launch cannot take
long blocks_of(int n, int h, int w) {
  if (n < 1 || n > 65535 || h < 1 || w < 1) return 0;
  const long nblk = ((long)h * w + B4 - 1) / B4;
  return nblk <= 0x7FFFFFFFL ? nblk : 0;
}

}  // namespace

extern "C" long cnnitmo_highlight_workspace_bytes(int n, int h, int w) {
  return (long)n * blocks_of(n, h, w) * 4 * (long)sizeof(double);
}

extern "C" int cnnitmo_highlight_loss_grad(int base, double tau, double gain, const float* s, const float* y,
                                           const float* t, int n, int h, int w, double grad_frames, double* out,
                                           float* dy, void* workspace, long workspace_bytes, void* stream) {
  CNN_REQUIRE(base == CNNITMO_BASE_MAE || base == CNNITMO_BASE_MSE, "highlight: base %d (MAE or MSE)", base);
  CNN_REQUIRE(tau >= 0.0 && tau < 1.0, "highlight: tau %g outside [0, 1)", tau);
  CNN_REQUIRE(gain >= 0.0 && gain <= 1.7976931348623157e308, "highlight: gain %g negative or not finite", gain);
  CNN_REQUIRE(s && y && t && out && workspace, "highlight: null pointer");
  CNN_REQUIRE((((uintptr_t)s | (uintptr_t)y | (uintptr_t)t | (uintptr_t)dy) & 3) == 0,
              "highlight: an image pointer is not 4-byte aligned");
  CNN_REQUIRE(n > 0 && h > 0 && w > 0, "highlight: bad shape n=%d h=%d w=%d", n, h, w);
  const long nblk = blocks_of(n, h, w);
  CNN_REQUIRE(nblk > 0, "highlight: batch %d of %d x %d too large", n, h, w);
  CNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "highlight: workspace not 8-byte aligned");
  const long need = cnnitmo_highlight_workspace_bytes(n, h, w);
  CNN_REQUIRE(workspace_bytes >= need, "highlight: workspace too small (%ld < %ld bytes)", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const long npix = (long)h * w;
  const double frames = grad_frames > 0.0 ? grad_frames : (double)n;
  const double fn = frames * ((double)npix * 3.0), den = 1.0 - tau;
  double* part = (double*)workspace;
  const dim3 grid((unsigned)nblk, (unsigned)n);
  if (dy)
    hipLaunchKernelGGL(highlight_kernel<true>, grid, dim3(NT), 0, st, s, y, t, npix, base, tau, den, gain, fn, part,
                       dy);
  else
    hipLaunchKernelGGL(highlight_kernel<false>, grid, dim3(NT), 0, st, s, y, t, npix, base, tau, den, gain, fn, part,
                       (float*)nullptr);
  hipLaunchKernelGGL(highlight_final_kernel, dim3(n), dim3(NT), 0, st, (const double*)part, nblk, (double)npix, out);
  return cnnitmo_check_launch("highlight_loss_grad");
}
