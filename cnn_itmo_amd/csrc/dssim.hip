// Structural-dissimilarity training loss of a prediction y against a target t (NHWC RGB fp32),
// per image, with its gradient (cnnitmo_dssim_loss_grad):
//
//   L = alpha (1 - SSIM(y, t)) + (1 - alpha) B,   B = mean |y-t| ('mae') or mean (y-t)^2 ('mse')
//
// SSIM is the metric of metrics.hip (11x11 Gaussian window, sigma 1.5, valid positions, max_val
// 1); window, constants, tile and float-column addressing are those of ssim_mse_kernel and the
// forward numbers agree with cnnitmo_image_metrics: both kernels are ssim_tile.h's tile_pass.
//
// Gradient.  With the Gaussian-weighted moments my, mt, s_yy, s_tt, s_yt of a map position q,
//   A1 = 2 my mt + C1, A2 = 2 (s_yt - my mt) + C2, B1 = my^2 + mt^2 + C1,
//   B2 = (s_yy - my^2) + (s_tt - mt^2) + C2,  S = A1 A2 / (B1 B2),
// S depends on y through my, s_yy and s_yt only, and d my/dy_p = g(p-q), d s_yy/dy_p =
// 2 g(p-q) y_p, d s_yt/dy_p = g(p-q) t_p.  Collecting the three factors per position,
//   Pc = 2 A1 / (B1 B2),  Pb = -2 S / B2,
//   Pa = 2 mt A2 / (B1 B2) - 2 my S / B1 - mt Pc - my Pb,
//   d(sum_q S_q)/dy_p = Fa_p + y_p Fb_p + t_p Fc_p,   F. = sum_q g(p-q) P._q,
// F the full (zero-padded) correlation of a coefficient plane with the window: the adjoint of
// the valid filter.
//
// dssim_coef_kernel (pass 1) is ssim_mse_kernel's tile pass with the base term in place of the
// squared error and, with a gradient asked for, the three coefficients of every map element stored
// into fp64 workspace planes [n][3][h-10][3(w-10)].  fp32 planes were measured on the CPU at
// 4.6e-6 of max|dy| on a nearly flat pair (1/B2 ~ 1e3), outside the 1e-6 the tests hold.
//
// dssim_grad_kernel (pass 2): one workgroup owns TR x TC image rows x float-columns.  One plane
// at a time ssim_tile.h's adjoint_pass stages the (TR+10) x (TC+30) window of the plane above and to the left of its
// tile (zero outside the map), runs the horizontal pass into fp64 row sums in LDS and the
// vertical pass into registers: 27 KB of LDS instead of the 80 KB of three planes at once, at
// the price of three rounds of barriers.  Each thread then holds Fa, Fb, Fc of 4 rows of one
// column, reads y and t from global memory (consecutive lanes, consecutive floats), adds the
// base term's derivative and writes dy: every element of [n][h][w][3] exactly once.
//
// Numerics as in metrics.hip: fp64 after the loads, taps with explicit fma(), everything else
// under `#pragma clang fp contract(off)`; per-workgroup sums, folded in a fixed order
// (reduce.h) by dssim_final_kernel.  No atomics: two runs are bitwise equal.  The two scale factors of dy
// are formed on the host, so a doubled grad_frames halves every product exactly.
//
// cnnitmo_rgb_accuracy: the head's 'accuracy' (argmax over RGB of prediction and target agree)
// for the loss-only path, where no head backward kernel runs.  It counts with integer atomics:
// the count does not depend on their order.
#include <math.h>

#include <algorithm>

#include "common.h"

#pragma clang fp contract(off)

#include "ssim_tile.h"

namespace {

using namespace ssim_tile;  // the tile, its staging and the separable fp64 filters of both passes (ssim_tile.h)

// Pass 1.  part [n][nblk][2] = (sum of S, sum of the base term) of a tile; GRAD: planes
// [n][3][mh][mw3] = (Pa, Pb, Pc) of every map element.  grid (tiles_x, tiles_y, n)
template <bool VEC, bool GRAD>
__global__ __launch_bounds__(NT) void dssim_coef_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        int h, int w, int base, Taps tp, double c1, double c2,
                                                        double* __restrict__ part, double* __restrict__ planes) {
  tile_pass<VEC, GRAD ? BASE_TERM_AND_PLANES : BASE_TERM>(a, b, h, w, base, tp, c1, c2, part, planes);
}

// Pass 2.  dy [n][h][w3] = ks (Fa + y Fb + t Fc) + kb b'(y - t); grid (tiles_x, tiles_y, n) over the image
__global__ __launch_bounds__(NT) void dssim_grad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const double* __restrict__ planes, int h, int w, int base,
                                                        Taps tp, double ks, double kb, float* __restrict__ dy) {
  const int tid = threadIdx.x;
  const int w3 = 3 * w;
  const int r0 = blockIdx.y * TR, c0 = blockIdx.x * TC;
  const int rb = (tid / TC) * G, c = tid % TC;  // this thread's outputs: rows rb..rb+3 of column c (tid < 192)

  double f[3][G];
  adjoint_pass(planes, h - 2 * R, 3 * (w - 2 * R), tp, f);

  if (tid >= (TR / G) * TC || c0 + c >= w3) return;
  const long img = (long)blockIdx.z * h * w3;
#pragma unroll
  for (int t = 0; t < G; ++t) {
    const int gr = r0 + rb + t;
    if (gr < h) {
      const long o = img + (long)gr * w3 + (c0 + c);
      const double y = (double)a[o], tg = (double)b[o];
      const double s = (f[0][t] + y * f[1][t]) + tg * f[2][t];
      dy[o] = (float)(ks * s + kb * base_term_slope(base, y - tg));
    }
  }
}

// one workgroup per image: thread t folds pairs t, t + NT, ... in order, then a fixed tree.
// out [n][3] = {ssim, B, L}
__global__ __launch_bounds__(NT) void dssim_final_kernel(const double* __restrict__ part, long nblk, double n_elem,
                                                         double n_pos, double alpha, double* __restrict__ out) {
  __shared__ double sh[2][NT];
  const int im = blockIdx.x;
  reduce::fold_tree_sum<2, NT>(part + (long)im * nblk * 2, nblk, sh);
  if (threadIdx.x == 0) {
    const double ssim = sh[0][0] / n_pos, bt = sh[1][0] / n_elem;
    out[3 * im] = ssim;
    out[3 * im + 1] = bt;
    out[3 * im + 2] = alpha * (1.0 - ssim) + (1.0 - alpha) * bt;
  }
}

// count += pixels whose argmax over RGB agrees between y and t (the head kernels' tie rule)
__global__ __launch_bounds__(NT) void rgb_accuracy_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                          long npix, unsigned long long* __restrict__ count) {
  __shared__ unsigned int sh[NT / 64];
  unsigned int cnt = 0;
  for (long p = (long)blockIdx.x * NT + threadIdx.x; p < npix; p += (long)gridDim.x * NT) {
    const float y0 = y[3 * p], y1 = y[3 * p + 1], y2 = y[3 * p + 2];
    const float t0 = t[3 * p], t1 = t[3 * p + 1], t2 = t[3 * p + 2];
    const int at = (t1 > t0) ? ((t2 > t1) ? 2 : 1) : ((t2 > t0) ? 2 : 0);
    const int ap = (y1 > y0) ? ((y2 > y1) ? 2 : 1) : ((y2 > y0) ? 2 : 0);
    cnt += at == ap ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int s = 0;
    for (int i = 0; i < NT / 64; ++i) s += sh[i];
    atomicAdd(count, (unsigned long long)s);
  }
}

bool good_shape(int n, int h, int w) {
  return n > 0 && n <= 65535 && h >= NTAP && w >= NTAP && 3L * w < (1L << 30) && h <= 65535 * TR;
}

}  // namespace

extern "C" long cnnitmo_dssim_workspace_bytes(int n, int h, int w, int with_grad) {
  if (!good_shape(n, h, w)) return 0;
  long bytes = (long)n * tiles_of(h, w) * 2 * (long)sizeof(double);
  if (with_grad) bytes += (long)n * 3 * (h - 2 * R) * 3 * (w - 2 * R) * (long)sizeof(double);
  return bytes;
}

extern "C" int cnnitmo_dssim_loss_grad(int base, double alpha, const float* y, const float* t, int n, int h, int w,
                                       double grad_frames, double* out, float* dy, void* workspace,
                                       long workspace_bytes, void* stream) {
  CNN_REQUIRE(base >= CNNITMO_BASE_NONE && base <= CNNITMO_BASE_MSE, "dssim: unknown base %d", base);
  CNN_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "dssim: alpha %g outside [0, 1]", alpha);
  CNN_REQUIRE(base != CNNITMO_BASE_NONE || alpha == 1.0, "dssim: alpha %g without a base term", alpha);
  CNN_REQUIRE(y && t && out && workspace, "dssim: null pointer");
  CNN_REQUIRE(n > 0 && h > 0 && w > 0, "dssim: bad shape n=%d h=%d w=%d", n, h, w);
  CNN_REQUIRE(h >= NTAP && w >= NTAP, "dssim: SSIM needs h, w >= %d, got %d x %d", NTAP, h, w);
  CNN_REQUIRE(good_shape(n, h, w), "dssim: batch %d of %d x %d too large", n, h, w);
  CNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "dssim: workspace not 8-byte aligned");
  const long need = cnnitmo_dssim_workspace_bytes(n, h, w, dy != nullptr);
  CNN_REQUIRE(workspace_bytes >= need, "dssim: workspace too small (%ld < %ld bytes)", workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const int mh = h - 2 * R, mw = w - 2 * R;
  const Taps tp = make_taps();
  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  const dim3 grid = map_grid(h, w, n);
  const long nblk = tiles_of(h, w);
  double* part = (double*)workspace;
  double* planes = part + (long)n * nblk * 2;
  const bool vec = (3L * w) % 4 == 0 && aligned16(y) && aligned16(t);
  const double n_elem = (double)h * w * 3.0, n_pos = (double)mh * mw * 3.0;
#define COEF(V, GR)                                                                                             \
  hipLaunchKernelGGL((dssim_coef_kernel<V, GR>), grid, dim3(NT), 0, s, y, t, h, w, base, tp, c1, c2, part, \
                     GR ? planes : nullptr)
  if (dy) {
    if (vec) COEF(true, true);
    else COEF(false, true);
    const double frames = grad_frames > 0.0 ? grad_frames : (double)n;
    const double ks = -alpha / (frames * n_pos), kb = base == CNNITMO_BASE_NONE ? 0.0 : (1.0 - alpha) / (frames * n_elem);
    hipLaunchKernelGGL(dssim_grad_kernel, image_grid(h, w, n), dim3(NT), 0, s, y, t, (const double*)planes, h, w, base,
                       tp, ks, kb, dy);
  } else {
    if (vec) COEF(true, false);
    else COEF(false, false);
  }
#undef COEF
  hipLaunchKernelGGL(dssim_final_kernel, dim3(n), dim3(NT), 0, s, (const double*)part, nblk, n_elem, n_pos, alpha, out);
  return cnnitmo_check_launch("dssim_loss_grad");
}

extern "C" int cnnitmo_rgb_accuracy(const float* y, const float* t, long npix, unsigned long long* count,
                                    void* stream) {
  CNN_REQUIRE(y && t && count, "rgb_accuracy: null pointer");
  CNN_REQUIRE(npix > 0, "rgb_accuracy: %ld pixels", npix);
  const int blocks = (int)std::min<long>(1024, (npix + NT - 1) / NT);
  hipLaunchKernelGGL(rgb_accuracy_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, y, t, npix, count);
  return cnnitmo_check_launch("rgb_accuracy");
}
