// Multi-scale SSIM of a prediction y against a target t (NHWC RGB fp32), per image, as a metric
// and as a training loss with its gradient (cnnitmo_msssim_loss_grad), after
// tf.image.ssim_multiscale:
//
//   level 0 = the image; level k+1 = the 2x2 mean of level k after an odd side was extended by a
//             copy of its last row / column (SYMMETRIC pad 1, avg_pool VALID): h' = ceil(h / 2)
//   cs = (2 cov + C2) / (vy + vt + C2),  l = (2 my mt + C1) / (my^2 + mt^2 + C1)   (ssim_tile.h's
//             Gaussian-weighted moments: 11 taps, sigma 1.5, valid positions, C = (K max_val)^2)
//   F[k][c] = mean_q cs (k < M-1),  F[M-1][c] = mean_q l cs,   per channel c
//   MS_c = prod_k max(F[k][c], 0)^w_k,   MS-SSIM = (MS_0 + MS_1 + MS_2) / 3
//   L = alpha (1 - MS-SSIM) + (1 - alpha) B,   B = dssim.hip's base term
//
// Gradient.  dMS/dy = 1/3 sum_c MS_c sum_k (w_k / F[k][c]) dF[k][c]/dy, and a channel with any
// factor <= 0 contributes exactly 0.  At level k, dF/dy_k is dssim.hip's form (Fa + y_k Fb +
// t_k Fc) / n_pos_k with the coefficient planes of S at the last level and of cs (A1 = B1 = 1:
// Pc = 2 / B2, Pb = -2 cs / B2, Pa = -mt Pc - my Pb) below it.  The level gradients go from
// coarse to fine, g_k = own_k + D^T g_{k+1}: every fine pixel reads a quarter of its one coarse
// parent, twice that in a last row / column that was copied into the pad (a gather, no atomics).
//
// Kernels, all on the caller's stream:
//   msssim_pool_kernel   level k -> level k+1 of y and t, fp64 in the workspace
//   msssim_coef_kernel   ssim_tile.h's tile_pass per level: per-channel sums of the factor, the
//                        base term's sum (level 0), and with a gradient the fp64 planes
//   msssim_final_kernel  one workgroup per image folds the per-tile sums in a fixed order, writes
//                        out and the scalars MS_c w_k / F[k][c] (0 for a clamped channel) that
//                        the gradient kernels read from device memory: nothing goes to the host
//   msssim_grad_kernel   coarse to fine: ssim_tile.h's adjoint_pass, the own term, the parent's
//                        share; level 0 adds the base term's derivative and writes dy as fp32
//
// Workspace (cnnitmo_msssim_workspace_bytes, exact), P_k = n h_k w_k pixels of level k,
// Q_k = n (h_k - 10)(w_k - 10) map positions:
//   levels      48 B x P_k, k >= 1     (y and t, 3 fp64 each)
//   partials    32 B per tile and level, scalars 24 B x n x scales
//   with a gradient: planes 72 B x Q_k, every k; level gradients 24 B x P_k, k >= 1
// The levels >= 1 together hold a third of level 0's pixels: 16 B per pixel of level 0 for the
// loss alone, <= 16 + 72 + (72 + 24) / 3 = 120 B per pixel with the gradient (DSSIM: 72 B).
//
// Numerics as in dssim.hip: fp64 after the loads, taps with explicit fma(), everything else
// under `#pragma clang fp contract(off)`, fixed-order reductions, no atomics: two runs are
// bitwise equal.  The scale factors -alpha / (3 F n_pos_k) and (1 - alpha) / (F n_elem) are
// formed on the host, so a doubled grad_frames halves every product exactly.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

#include "ssim_tile.h"

namespace {

using namespace ssim_tile;

constexpr int MAX_SCALES = 5;

// level k+1 [n][h2][3 w2] of a and of b [n][h][3 w]; grid (ceil(3 w2 / NT), h2, n)
template <typename T>
__global__ __launch_bounds__(NT) void msssim_pool_kernel(const T* __restrict__ a, const T* __restrict__ b, int h,
                                                         int w, double* __restrict__ oa, double* __restrict__ ob) {
  const int h2 = (h + 1) / 2, w2 = (w + 1) / 2;
  const int c3 = blockIdx.x * NT + threadIdx.x, r = blockIdx.y;
  if (c3 >= 3 * w2) return;
  const int px = c3 / 3, ch = c3 % 3;
  const int y0 = 2 * r, y1 = min(2 * r + 1, h - 1);  // (an odd side's pad repeats its last row / column)
  const int x0 = 3 * (2 * px) + ch, x1 = 3 * min(2 * px + 1, w - 1) + ch;
  const long img = (long)blockIdx.z * h * 3 * w;
  const long o0 = img + (long)y0 * 3 * w, o1 = img + (long)y1 * 3 * w;
  const long o = ((long)blockIdx.z * h2 + r) * 3 * w2 + c3;
  oa[o] = 0.25 * (((double)a[o0 + x0] + (double)a[o0 + x1]) + ((double)a[o1 + x0] + (double)a[o1 + x1]));
  ob[o] = 0.25 * (((double)b[o0 + x0] + (double)b[o0 + x1]) + ((double)b[o1 + x0] + (double)b[o1 + x1]));
}

// part [n][nblk][4] = (sum of the level's factor over R, G, B, sum of the base term) of a tile;
// GRAD: planes [n][3][mh][mw3].  CS: a level below the last.  grid (tiles_x, tiles_y, n)
template <typename T, bool VEC, bool GRAD, bool CS>
__global__ __launch_bounds__(NT) void msssim_coef_kernel(const T* __restrict__ a, const T* __restrict__ b, int h,
                                                         int w, int base, Taps tp, double c1, double c2,
                                                         double* __restrict__ part, double* __restrict__ planes) {
  tile_pass<VEC, GRAD ? BASE_TERM_AND_PLANES : BASE_TERM, T, true, CS>(a, b, h, w, base, tp, c1, c2, part, planes);
}

struct Scales {
  int m;
  long part[MAX_SCALES];    // offset of a level's partials in the workspace, in doubles
  long nblk[MAX_SCALES];    // tiles per image
  double npos[MAX_SCALES];  // map positions per channel
  double w[MAX_SCALES];     // power factors
};

// One workgroup per image: per level, thread t folds tiles t, t + NT, ... in order, then a fixed
// tree.  out [n][3 + 3 m] = {ms_ssim, B, L, F[k][c]}; scal [n][m][3] = MS_c w_k / F[k][c], 0 for
// a channel with a factor <= 0
__global__ __launch_bounds__(NT) void msssim_final_kernel(const double* __restrict__ ws, Scales sc, double n_elem,
                                                          double alpha, double* __restrict__ out,
                                                          double* __restrict__ scal) {
  __shared__ double sh[4][NT];
  __shared__ double f[MAX_SCALES][4];
  const int im = blockIdx.x, tid = threadIdx.x;
  for (int k = 0; k < sc.m; ++k) {
    reduce::fold_tree_sum<4, NT>(ws + sc.part[k] + (long)im * sc.nblk[k] * 4, sc.nblk[k], sh);
    if (tid < 4) f[k][tid] = sh[tid][0];
    __syncthreads();
  }
  if (tid != 0) return;
  double* o = out + (long)im * (3 + 3 * sc.m);
  double ms[3];
  for (int c = 0; c < 3; ++c) {
    double p = 1.0;
    bool live = true;
    for (int k = 0; k < sc.m; ++k) {
      const double fk = f[k][c] / sc.npos[k];
      o[3 + 3 * k + c] = fk;
      live = live && fk > 0.0;
      p = p * pow(fk > 0.0 ? fk : 0.0, sc.w[k]);
    }
    ms[c] = p;
    for (int k = 0; k < sc.m; ++k)
      scal[((long)im * sc.m + k) * 3 + c] = live ? p * sc.w[k] / (f[k][c] / sc.npos[k]) : 0.0;
  }
  const double msssim = ((ms[0] + ms[1]) + ms[2]) / 3.0, bt = f[0][3] / n_elem;
  o[0] = msssim;
  o[1] = bt;
  o[2] = alpha * (1.0 - msssim) + (1.0 - alpha) * bt;
}

// g [n][h][3 w] of level k = ks scal[k][c] (Fa + y Fb + t Fc) + D^T gp + kb b'(y - t); gp: the
// next level's gradient [n][ceil(h/2)][3 ceil(w/2)] or null at the last level.  TO: float (dy,
// level 0) or double (a level gradient in the workspace).  grid (tiles_x, tiles_y, n) over the level
template <typename T, typename TO>
__global__ __launch_bounds__(NT) void msssim_grad_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                         const double* __restrict__ planes,
                                                         const double* __restrict__ scal, int k, int m, int h, int w,
                                                         int base, Taps tp, double ks, double kb,
                                                         const double* __restrict__ gp, TO* __restrict__ g) {
  const int tid = threadIdx.x;
  const int w3 = 3 * w;
  const int mh = h - 2 * R, mw3 = 3 * (w - 2 * R);
  const int r0 = blockIdx.y * TR, c0 = blockIdx.x * TC;
  const int rb = (tid / TC) * G, c = tid % TC;  // this thread's outputs: rows rb..rb+3 of column c (tid < 192)

  double f[3][G];
  adjoint_pass(planes, mh, mw3, tp, f);

  if (tid >= (TR / G) * TC || c0 + c >= w3) return;
  const int ch = c % 3, px = (c0 + c) / 3;  // (c0 is a multiple of 3)
  const double ksc = ks * scal[((long)blockIdx.z * m + k) * 3 + ch];
  const int h2 = (h + 1) / 2, w2 = (w + 1) / 2;
  // a last row / column that was copied into the pad feeds its parent twice
  const double sx = (px == w - 1 && (w & 1)) ? 0.5 : 0.25;
  const long img = (long)blockIdx.z * h * w3;
#pragma unroll
  for (int t = 0; t < G; ++t) {
    const int gr = r0 + rb + t;
    if (gr < h) {
      const long o = img + (long)gr * w3 + (c0 + c);
      const double y = (double)a[o], tg = (double)b[o];
      const double s = (f[0][t] + y * f[1][t]) + tg * f[2][t];
      double v = ksc == 0.0 ? 0.0 : ksc * s;  // (a clamped channel is exactly 0 whatever its planes hold)
      if (gp) {
        const double sy = (gr == h - 1 && (h & 1)) ? 2.0 : 1.0;
        v += (sx * sy) * gp[((long)blockIdx.z * h2 + (gr >> 1)) * 3 * w2 + 3 * (px >> 1) + ch];
      }
      g[o] = (TO)(v + kb * base_term_slope(base, y - tg));
    }
  }
}

// the sizes of the levels and where each piece of the workspace starts, in doubles
struct Plan {
  int h[MAX_SCALES], w[MAX_SCALES];
  long ly[MAX_SCALES], lt[MAX_SCALES], part[MAX_SCALES], planes[MAX_SCALES], grad[MAX_SCALES];
  long scal, total;
};

bool good_shape(int n, int h, int w, int scales) {
  if (!(n > 0 && n <= 65535 && h >= NTAP && w >= NTAP && 3L * w < (1L << 30) && h <= 65535)) return false;
  if (scales < 1 || scales > MAX_SCALES) return false;
  for (int k = 1; k < scales; ++k) h = (h + 1) / 2, w = (w + 1) / 2;
  return h >= NTAP && w >= NTAP;
}

Plan make_plan(int n, int h, int w, int scales, bool with_grad) {
  Plan p{};
  long at = 0;
  for (int k = 0; k < scales; ++k) {
    p.h[k] = k ? (p.h[k - 1] + 1) / 2 : h;
    p.w[k] = k ? (p.w[k - 1] + 1) / 2 : w;
    const long pix = (long)n * p.h[k] * p.w[k] * 3;
    if (k) {
      p.ly[k] = at, at += pix;
      p.lt[k] = at, at += pix;
      if (with_grad) p.grad[k] = at, at += pix;
    }
    p.part[k] = at, at += (long)n * tiles_of(p.h[k], p.w[k]) * 4;
    if (with_grad) p.planes[k] = at, at += (long)n * 3 * (p.h[k] - 2 * R) * 3 * (p.w[k] - 2 * R);
  }
  p.scal = at, at += (long)n * scales * 3;
  p.total = at;
  return p;
}

}  // namespace

extern "C" long cnnitmo_msssim_workspace_bytes(int n, int h, int w, int scales, int with_grad) {
  if (!good_shape(n, h, w, scales)) return 0;
  return make_plan(n, h, w, scales, with_grad != 0).total * (long)sizeof(double);
}

extern "C" int cnnitmo_msssim_loss_grad(int base, double alpha, const double* power_factors, int scales,
                                        double max_val, const float* y, const float* t, int n, int h, int w,
                                        double grad_frames, double* out, float* dy, void* workspace,
                                        long workspace_bytes, void* stream) {
  CNN_REQUIRE(base >= CNNITMO_BASE_NONE && base <= CNNITMO_BASE_MSE, "msssim: unknown base %d", base);
  CNN_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "msssim: alpha %g outside [0, 1]", alpha);
  CNN_REQUIRE(base != CNNITMO_BASE_NONE || alpha == 1.0, "msssim: alpha %g without a base term", alpha);
  CNN_REQUIRE(scales >= 1 && scales <= MAX_SCALES, "msssim: %d scales outside 1..%d", scales, MAX_SCALES);
  CNN_REQUIRE(power_factors && y && t && out && workspace, "msssim: null pointer");
  for (int k = 0; k < scales; ++k)
    CNN_REQUIRE(power_factors[k] >= 0.0 && power_factors[k] <= 1.79769313486231570e308,
                "msssim: power factor %d is %g (finite, >= 0)", k, power_factors[k]);
  CNN_REQUIRE(max_val > 0.0 && max_val <= 1.79769313486231570e308, "msssim: max_val %g", max_val);
  CNN_REQUIRE(n > 0 && h > 0 && w > 0, "msssim: bad shape n=%d h=%d w=%d", n, h, w);
  {
    int ch = h, cw = w;
    for (int k = 1; k < scales; ++k) ch = (ch + 1) / 2, cw = (cw + 1) / 2;
    CNN_REQUIRE(ch >= NTAP && cw >= NTAP, "msssim: %d scales of %d x %d end at %d x %d, under the %d x %d window",
                scales, h, w, ch, cw, NTAP, NTAP);
  }
  CNN_REQUIRE(good_shape(n, h, w, scales), "msssim: batch %d of %d x %d too large", n, h, w);
  CNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "msssim: workspace not 8-byte aligned");
  const long need = cnnitmo_msssim_workspace_bytes(n, h, w, scales, dy != nullptr);
  CNN_REQUIRE(workspace_bytes >= need, "msssim: workspace too small (%ld < %ld bytes)", workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const bool grad = dy != nullptr;
  const Plan p = make_plan(n, h, w, scales, grad);
  double* ws = (double*)workspace;
  const Taps tp = make_taps();
  const double c1 = (0.01 * max_val) * (0.01 * max_val), c2 = (0.03 * max_val) * (0.03 * max_val);

  for (int k = 0; k + 1 < scales; ++k) {  // the pyramid
    const dim3 grid((unsigned)((3 * p.w[k + 1] + NT - 1) / NT), (unsigned)p.h[k + 1], n);
    if (k == 0)
      hipLaunchKernelGGL(msssim_pool_kernel<float>, grid, dim3(NT), 0, s, y, t, h, w, ws + p.ly[1], ws + p.lt[1]);
    else
      hipLaunchKernelGGL(msssim_pool_kernel<double>, grid, dim3(NT), 0, s, (const double*)(ws + p.ly[k]),
                         (const double*)(ws + p.lt[k]), p.h[k], p.w[k], ws + p.ly[k + 1], ws + p.lt[k + 1]);
  }

  Scales sc{};
  sc.m = scales;
  const bool vec = (3L * w) % 4 == 0 && aligned16(y) && aligned16(t);
  for (int k = 0; k < scales; ++k) {  // factors and planes
    const int mh = p.h[k] - 2 * R, mw = p.w[k] - 2 * R;
    const dim3 grid = map_grid(p.h[k], p.w[k], n);
    sc.part[k] = p.part[k];
    sc.nblk[k] = tiles_of(p.h[k], p.w[k]);
    sc.npos[k] = (double)mh * mw;
    sc.w[k] = power_factors[k];
    double* planes = grad ? ws + p.planes[k] : nullptr;
    const bool cs = k + 1 < scales;
#define COEF(T, V, GR, CSO, A, B, BASE)                                                                         \
  hipLaunchKernelGGL((msssim_coef_kernel<T, V, GR, CSO>), grid, dim3(NT), 0, s, A, B, p.h[k], p.w[k], BASE, tp, \
                     c1, c2, ws + p.part[k], planes)
#define COEF_GC(T, V, A, B, BASE)                 \
  do {                                            \
    if (grad && cs) COEF(T, V, true, true, A, B, BASE);        \
    else if (grad) COEF(T, V, true, false, A, B, BASE);        \
    else if (cs) COEF(T, V, false, true, A, B, BASE);          \
    else COEF(T, V, false, false, A, B, BASE);                 \
  } while (0)
    if (k == 0) {
      if (vec) COEF_GC(float, true, y, t, base);
      else COEF_GC(float, false, y, t, base);
    } else {
      COEF_GC(double, false, (const double*)(ws + p.ly[k]), (const double*)(ws + p.lt[k]), CNNITMO_BASE_NONE);
    }
#undef COEF_GC
#undef COEF
  }

  const double n_elem = (double)h * w * 3.0;
  hipLaunchKernelGGL(msssim_final_kernel, dim3(n), dim3(NT), 0, s, (const double*)ws, sc, n_elem, alpha, out,
                     ws + p.scal);

  if (grad) {  // coarse to fine
    const double frames = grad_frames > 0.0 ? grad_frames : (double)n;
    const double kb = base == CNNITMO_BASE_NONE ? 0.0 : (1.0 - alpha) / (frames * n_elem);
    for (int k = scales - 1; k >= 0; --k) {
      const double ks = -alpha / (frames * (3.0 * sc.npos[k]));
      const dim3 grid = image_grid(p.h[k], p.w[k], n);
      const double* gp = k + 1 < scales ? ws + p.grad[k + 1] : nullptr;
      if (k == 0)
        hipLaunchKernelGGL((msssim_grad_kernel<float, float>), grid, dim3(NT), 0, s, y, t,
                           (const double*)(ws + p.planes[0]), (const double*)(ws + p.scal), 0, scales, h, w, base, tp,
                           ks, kb, gp, dy);
      else
        hipLaunchKernelGGL((msssim_grad_kernel<double, double>), grid, dim3(NT), 0, s,
                           (const double*)(ws + p.ly[k]), (const double*)(ws + p.lt[k]),
                           (const double*)(ws + p.planes[k]), (const double*)(ws + p.scal), k, scales, p.h[k], p.w[k],
                           CNNITMO_BASE_NONE, tp, ks, 0.0, gp, ws + p.grad[k]);
    }
  }
  return cnnitmo_check_launch("msssim_loss_grad");
}
