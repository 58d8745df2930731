// Image-fidelity metrics of two NHWC RGB fp32 batches, per image (cnnitmo_image_metrics):
//
//   mse   = mean over h*w*3 of (a-b)^2, psnr = 10*log10(max_val^2/mse)      (tf.image.psnr)
//   ssim  = mean over the valid window positions and the 3 channels of
//           ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2))
//           with an 11x11 Gaussian window (sigma 1.5), biased weighted moments,
//           C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2   (tf.image.ssim, Wang et al. 2004)
//
// One pass over both images; no filtered map or SSIM map goes to global memory.  A row
// of an NHWC RGB image is 3*w contiguous floats and the horizontal taps of one channel are
// 3 floats apart, so the kernel works on "float columns": the SSIM map of an image is
// (h-10) rows x 3*(w-10) columns, column j reading input columns j + 3k, k = 0..10.
//
// ssim_mse_kernel (its body is ssim_tile.h's tile_pass, which the DSSIM loss of dssim.hip
// shares): one workgroup owns TR x TC positions of that map.  It stages the
// (TR+10) x (TC+30) input window of both images through LDS (16-byte loads where the row
// pitch allows them), accumulating (a-b)^2 of the elements it owns on the way (its own
// TR x TC corner; the last tile row / column also own the 10-row / 30-column apron, so
// every element is counted once).  Then the separable filter of the five maps x, y, x^2,
// y^2, xy: the horizontal pass leaves fp64 row sums in LDS (each thread 4 outputs that
// share taps: 14 reads of each image for 4 x 11 taps), the vertical pass reads them back
// (each thread 4 rows of one column: 14 x 5 reads), forms the SSIM term and sums it.
//
// Numerics: everything after the load is fp64.  The products x^2, y^2, xy of fp32 values
// are exact in fp64, so sx^2 = E[x^2] - mx^2 cancels against C2 = 9e-4 with ~1e-16 of
// error instead of fp32's 1e-7 (which moves SSIM of flat images by 1e-4).  The filter taps
// accumulate with explicit fma(); every other expression is compiled under
// `#pragma clang fp contract(off)`.
//
// Reduction (reduce.h): block_sum, in-wave shuffles, then LDS across the waves, one (ssim sum,
// squared-error sum) pair per workgroup into the caller's workspace; metrics_final_kernel folds
// an image's pairs with fold_tree_sum, a fixed order in fp64.  No atomics: two runs are bitwise
// equal.
//
// what == 1 (MSE/PSNR only, any h, w >= 1) takes mse_kernel, a plain strided reduction
// with the same two-level fold.
#include <math.h>

#include <algorithm>

#include "common.h"

#pragma clang fp contract(off)

#include "ssim_tile.h"

namespace {

using namespace ssim_tile;                // the tile, its staging and the separable fp64 filter (ssim_tile.h)
constexpr int MSE_BLK = 128;             // workgroups per image of mse_kernel

// part [n][nblk][2] = (ssim sum, squared-error sum) of a tile; grid (tiles_x, tiles_y, n)
template <bool VEC>
__global__ __launch_bounds__(NT) void ssim_mse_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      int h, int w, Taps tp, double c1, double c2,
                                                      double* __restrict__ part) {
  tile_pass<VEC, SQUARED_ERROR>(a, b, h, w, 0, tp, c1, c2, part, nullptr);
}

// part [n][MSE_BLK][2] = (0, squared-error sum); len = h*w*3 elements per image; grid (MSE_BLK, n)
template <bool VEC>
__global__ __launch_bounds__(NT) void mse_kernel(const float* __restrict__ a, const float* __restrict__ b, long len,
                                                 double* __restrict__ part) {
  __shared__ double red[NT / 64][2];
  const long img = (long)blockIdx.y * len;
  double sq = 0.0;
  if (VEC) {  // len % 4 == 0 and 16-byte aligned bases
    for (long i = ((long)blockIdx.x * NT + threadIdx.x) * 4; i < len; i += (long)MSE_BLK * NT * 4) {
      const float4 va = *reinterpret_cast<const float4*>(a + img + i);
      const float4 vb = *reinterpret_cast<const float4*>(b + img + i);
      const double d0 = (double)va.x - (double)vb.x, d1 = (double)va.y - (double)vb.y;
      const double d2 = (double)va.z - (double)vb.z, d3 = (double)va.w - (double)vb.w;
      sq += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  } else {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < len; i += (long)MSE_BLK * NT) {
      const double d = (double)a[img + i] - (double)b[img + i];
      sq += d * d;
    }
  }
  const double s = reduce::block_sum<2, NT>({0.0, sq}, red);  // thread 0: 0, thread 1: the sum
  if (threadIdx.x < 2) part[((long)blockIdx.y * MSE_BLK + blockIdx.x) * 2 + threadIdx.x] = s;
}

// one workgroup per image: thread t folds pairs t, t + NT, ... in order, then a fixed tree
__global__ __launch_bounds__(NT) void metrics_final_kernel(const double* __restrict__ part, long nblk, int what,
                                                           double n_elem, double n_pos, double max_val,
                                                           double* __restrict__ out) {
  __shared__ double sh[2][NT];
  const int im = blockIdx.x;
  reduce::fold_tree_sum<2, NT>(part + (long)im * nblk * 2, nblk, sh);
  if (threadIdx.x == 0) {
    if (what & 1) {
      const double mse = sh[1][0] / n_elem;
      out[3 * im] = mse;
      out[3 * im + 1] = 10.0 * log10(max_val * max_val / mse);  // mse == 0: +inf
    }
    if (what & 2) out[3 * im + 2] = sh[0][0] / n_pos;
  }
}

long tiles_or_none(int h, int w) { return h < NTAP || w < NTAP ? 0 : tiles_of(h, w); }

}  // namespace

extern "C" long cnnitmo_image_metrics_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return (long)n * std::max<long>(tiles_or_none(h, w), MSE_BLK) * 2 * (long)sizeof(double);
}

extern "C" int cnnitmo_image_metrics(int what, const float* a, const float* b, int n, int h, int w, double max_val,
                                     double* out, void* workspace, long workspace_bytes, void* stream) {
  CNN_REQUIRE(what >= 1 && what <= 3, "image_metrics: what %d (bit 0 = MSE/PSNR, bit 1 = SSIM)", what);
  CNN_REQUIRE(a && b && out && workspace, "image_metrics: null pointer");
  CNN_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0, "image_metrics: bad shape n=%d h=%d w=%d", n, h, w);
  CNN_REQUIRE(3L * w < (1L << 30) && h <= 65535 * TR, "image_metrics: image %d x %d too large", h, w);
  CNN_REQUIRE(max_val > 0.0, "image_metrics: max_val %g", max_val);
  CNN_REQUIRE(!(what & 2) || (h >= NTAP && w >= NTAP), "image_metrics: SSIM needs h, w >= %d, got %d x %d", NTAP, h,
              w);
  CNN_REQUIRE(workspace_bytes >= cnnitmo_image_metrics_workspace_bytes(n, h, w),
              "image_metrics: workspace too small (%ld < %ld bytes)", workspace_bytes,
              cnnitmo_image_metrics_workspace_bytes(n, h, w));
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  const double n_elem = (double)h * w * 3.0;
  long nblk;
  double n_pos = 1.0;
  if (what & 2) {
    const Taps tp = make_taps();
    const double c1 = (0.01 * max_val) * (0.01 * max_val), c2 = (0.03 * max_val) * (0.03 * max_val);
    const dim3 grid = map_grid(h, w, n);
    nblk = tiles_of(h, w);
    n_pos = (double)(h - 2 * R) * (w - 2 * R) * 3.0;
    if ((3L * w) % 4 == 0 && aligned16(a) && aligned16(b))
      hipLaunchKernelGGL(ssim_mse_kernel<true>, grid, dim3(NT), 0, s, a, b, h, w, tp, c1, c2, part);
    else
      hipLaunchKernelGGL(ssim_mse_kernel<false>, grid, dim3(NT), 0, s, a, b, h, w, tp, c1, c2, part);
  } else {
    const long len = (long)h * w * 3;
    nblk = MSE_BLK;
    if (len % 4 == 0 && aligned16(a) && aligned16(b))
      hipLaunchKernelGGL(mse_kernel<true>, dim3(MSE_BLK, n), dim3(NT), 0, s, a, b, len, part);
    else
      hipLaunchKernelGGL(mse_kernel<false>, dim3(MSE_BLK, n), dim3(NT), 0, s, a, b, len, part);
  }
  hipLaunchKernelGGL(metrics_final_kernel, dim3(n), dim3(NT), 0, s, (const double*)part, nblk, what, n_elem, n_pos,
                     max_val, out);
  return cnnitmo_check_launch("image_metrics");
}
