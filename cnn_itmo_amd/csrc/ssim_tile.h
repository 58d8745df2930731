// The one SSIM filter of the image metrics (metrics.hip), the DSSIM training loss (dssim.hip) and
// the multi-scale loss (msssim.hip), on an NHWC RGB image addressed in float columns (see
// metrics.hip for the layout and the numerics):
//   tile_pass     the body of ssim_mse_kernel, dssim_coef_kernel and msssim_coef_kernel: one
//                 workgroup owns TR x TC positions of the SSIM map, sums the SSIM term and an
//                 element term over them (reduce.h) and, for a gradient, stores the coefficient
//                 planes.  Its horizontal pass is row_sums, whatever the input type.
//   adjoint_pass  the other direction, the body of dssim_grad_kernel and msssim_grad_kernel: the
//                 full correlation of the coefficient planes with the window.  The kernels differ
//                 in their epilogues only, which stay with them.
//   element_term, base_term_slope   the pointwise base term of the losses and its derivative
//   map_grid, image_grid, tiles_of  the launch grids of the two passes and the tiles per image
// The kernels that share a body are held to identical results and measured time, not to identical
// device code (the multi-scale section).  Include this file after
// `#pragma clang fp contract(off)`: only the filter taps accumulate with (explicit) fma().
#pragma once
#include <math.h>

#include "common.h"
#include "reduce.h"

namespace ssim_tile {

constexpr int NT = 256;                  // threads per workgroup
constexpr int TR = 16;                   // map rows per tile
constexpr int TC = 48;                   // map float-columns per tile (16 pixels)
constexpr int R = 5;                     // window radius: 11 taps
constexpr int NTAP = 2 * R + 1;
constexpr int IR = TR + 2 * R;           // staged input rows: 26
constexpr int IC = TC + 3 * 2 * R;       // staged input float-columns: 78
constexpr int ICP = 80;                  // padded to whole 16-byte chunks
constexpr int G = 4;                     // outputs per thread in either pass
constexpr int GW = G + 2 * R;            // inputs those outputs share: 14
static_assert(TC % (3 * G) == 0 && TR % G == 0 && ICP % 4 == 0 && ICP >= IC && TC % 4 == 0, "tile");

struct Taps {
  double g[NTAP];
};

// the normalised Gaussian window, sigma 1.5
static inline Taps make_taps() {
  Taps tp;
  double sum = 0.0;
  for (int i = 0; i < NTAP; ++i) sum += tp.g[i] = exp(-(double)((i - R) * (i - R)) / 4.5);
  for (int i = 0; i < NTAP; ++i) tp.g[i] /= sum;
  return tp;
}

// the launch grid of the TR x TC tiles of an n x h x w image's float columns (adjoint_pass's grid)
static inline dim3 image_grid(int h, int w, int n) {
  return dim3((unsigned)((3L * w + TC - 1) / TC), (unsigned)((h + TR - 1) / TR), (unsigned)n);
}

// the launch grid of the tiles of its SSIM map (tile_pass's grid; h, w >= NTAP)
static inline dim3 map_grid(int h, int w, int n) { return image_grid(h - 2 * R, w - 2 * R, n); }

// tiles of the SSIM map of an h x w image: the partials per image that the workspaces are sized by
static inline long tiles_of(int h, int w) {
  const dim3 g = map_grid(h, w, 1);
  return (long)g.x * g.y;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// What a tile sums beside the SSIM term, per element d = a - b, and whether it stores the
// gradient's coefficient planes (dssim.hip)
enum { SQUARED_ERROR = 0, BASE_TERM = 1, BASE_TERM_AND_PLANES = 2 };

template <int MODE>
__device__ __forceinline__ double element_term(int base, double d) {
  if constexpr (MODE == SQUARED_ERROR) return d * d;
  return base == CNNITMO_BASE_MSE ? d * d : (base == CNNITMO_BASE_MAE ? fabs(d) : 0.0);
}

// the base term's derivative in d: 2 d ('mse'), sign(d) with sign(0) = 0 ('mae'), 0 (none)
__device__ __forceinline__ double base_term_slope(int base, double d) {
  if (base == CNNITMO_BASE_MSE) return 2.0 * d;
  if (base == CNNITMO_BASE_MAE) return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
  return 0.0;
}

// (r, cb) of horizontal-pass item i < IR * (TC / G): staged row r; the thread's outputs are the
// float columns cb + 3 t, t < G (one channel of G neighbouring pixels), from inputs cb + 3 m, m < GW
__device__ __forceinline__ void row_item(int i, int& r, int& cb) {
  const int gi = i % (TC / G);
  r = i / (TC / G);
  cb = (gi / 3) * (3 * G) + gi % 3;
}

// the horizontal pass of one item: the row sums of the five maps x, y, xx, yy, xy
struct RowSums {
  double v[5][G];
};

template <typename T>
__device__ __forceinline__ RowSums row_sums(const T (&sa)[IR][ICP], const T (&sb)[IR][ICP], const Taps& tp, int r,
                                            int cb) {
  RowSums acc;
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int t = 0; t < G; ++t) acc.v[k][t] = 0.0;
#pragma unroll
  for (int m = 0; m < GW; ++m) {
    const double x = (double)sa[r][cb + 3 * m], y = (double)sb[r][cb + 3 * m];
    const double xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
    for (int t = 0; t < G; ++t) {
      if (m - t >= 0 && m - t < NTAP) {
        const double g = tp.g[m - t];
        acc.v[0][t] = fma(g, x, acc.v[0][t]);
        acc.v[1][t] = fma(g, y, acc.v[1][t]);
        acc.v[2][t] = fma(g, xx, acc.v[2][t]);
        acc.v[3][t] = fma(g, yy, acc.v[3][t]);
        acc.v[4][t] = fma(g, xy, acc.v[4][t]);
      }
    }
  }
  return acc;
}

// The body of a tile kernel; grid (tiles_x, tiles_y, n), NT threads.
// part [n][nblk][2] = (sum of the SSIM term, sum of the element term) of a tile.
// MODE == BASE_TERM_AND_PLANES: planes [n][3][mh][mw3] fp64 = (Pa, Pb, Pc) of every map element
// (dssim.hip), a the prediction and b the target.  base: a CNNITMO_BASE_* (unused in SQUARED_ERROR).
// The multi-scale loss (msssim.hip) adds: T = double, a pyramid level (scalar staging only);
// PER_CHANNEL, part [n][nblk][4] = (the term's sum over the R, G, B columns, the element term's
// sum): a float column's channel is column % 3 and TC is a multiple of 3; CS_ONLY, the term is
// the contrast-structure factor cs = A2 / B2 and the planes are those of S with A1 = B1 = 1.
template <bool VEC, int MODE, typename T = float, bool PER_CHANNEL = false, bool CS_ONLY = false>
__device__ __forceinline__ void tile_pass(const T* __restrict__ a, const T* __restrict__ b, int h, int w,
                                          int base, Taps tp, double c1, double c2,
                                          double* __restrict__ part, double* __restrict__ planes) {
  static_assert(!VEC || sizeof(T) == sizeof(float), "the 16-byte staging path is fp32's");
  static_assert(TC % 3 == 0, "a tile's first float column is a red one");
  // fp64 input doubles the staged windows; to stay at two workgroups per CU (80 KB each) the row
  // sums of yy and xy then take the windows' place once the horizontal pass has read them
  constexpr bool ALIAS = sizeof(T) == sizeof(double);
  constexpr int HI = (IR * (TC / G) + NT - 1) / NT;  // horizontal-pass rounds per thread
  static_assert(!ALIAS || ICP >= TC, "a window holds a plane of row sums");
  __shared__ T sa[IR][ICP];
  __shared__ T sb[IR][ICP];
  __shared__ double hs[ALIAS ? 3 : 5][IR][TC];
  constexpr int NP = PER_CHANNEL ? 4 : 2;  // partial sums per tile
  __shared__ double red[NT / 64][NP];

  const int tid = threadIdx.x;
  const int w3 = 3 * w;
  const int mh = h - 2 * R, mw3 = 3 * (w - 2 * R);  // the map's size
  const int r0 = blockIdx.y * TR, c0 = blockIdx.x * TC;
  const long img = (long)blockIdx.z * h * w3;
  // rows / columns of the staged window whose element term this tile counts
  const int own_r = blockIdx.y == gridDim.y - 1 ? IR : TR;
  const int own_c = blockIdx.x == gridDim.x - 1 ? ICP : TC;

  double sq = 0.0;
  if constexpr (VEC) {  // w3 % 4 == 0 and 16-byte aligned bases: a chunk is inside the row or outside it
    for (int i = tid; i < IR * (ICP / 4); i += NT) {
      const int r = i / (ICP / 4), c = (i % (ICP / 4)) * 4;
      const int gr = r0 + r, gc = c0 + c;
      float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
      if (gr < h && gc < w3) {
        const long o = img + (long)gr * w3 + gc;
        va = *reinterpret_cast<const float4*>(a + o);
        vb = *reinterpret_cast<const float4*>(b + o);
        if (r < own_r && c < own_c) {
          const double d0 = (double)va.x - (double)vb.x, d1 = (double)va.y - (double)vb.y;
          const double d2 = (double)va.z - (double)vb.z, d3 = (double)va.w - (double)vb.w;
          sq += (element_term<MODE>(base, d0) + element_term<MODE>(base, d1)) +
                (element_term<MODE>(base, d2) + element_term<MODE>(base, d3));
        }
      }
      *reinterpret_cast<float4*>(&sa[r][c]) = va;
      *reinterpret_cast<float4*>(&sb[r][c]) = vb;
    }
  } else {
    for (int i = tid; i < IR * ICP; i += NT) {
      const int r = i / ICP, c = i % ICP;
      const int gr = r0 + r, gc = c0 + c;
      T va = 0, vb = 0;
      if (gr < h && gc < w3) {
        const long o = img + (long)gr * w3 + gc;
        va = a[o];
        vb = b[o];
        if (r < own_r && c < own_c) sq += element_term<MODE>(base, (double)va - (double)vb);
      }
      sa[r][c] = va;
      sb[r][c] = vb;
    }
  }
  __syncthreads();

  // horizontal pass (row_sums): the five row sums of every item go to hs; ALIAS has room for three
  double (*hs3)[TC] = nullptr, (*hs4)[TC] = nullptr;  // ALIAS: the row sums of yy and xy
  if constexpr (ALIAS) {
    double keep[HI][2][G];  // yy and xy stay in registers until every thread has read the windows
#pragma unroll
    for (int it = 0; it < HI; ++it) {
      const int i = tid + it * NT;
      if (i < IR * (TC / G)) {
        int r, cb;
        row_item(i, r, cb);
        const RowSums acc = row_sums(sa, sb, tp, r, cb);
#pragma unroll
        for (int t = 0; t < G; ++t) {
#pragma unroll
          for (int k = 0; k < 3; ++k) hs[k][r][cb + 3 * t] = acc.v[k][t];
          keep[it][0][t] = acc.v[3][t];
          keep[it][1][t] = acc.v[4][t];
        }
      }
    }
    __syncthreads();
    hs3 = reinterpret_cast<double (*)[TC]>(&sa[0][0]);
    hs4 = reinterpret_cast<double (*)[TC]>(&sb[0][0]);
#pragma unroll
    for (int it = 0; it < HI; ++it) {
      const int i = tid + it * NT;
      if (i < IR * (TC / G)) {
        int r, cb;
        row_item(i, r, cb);
#pragma unroll
        for (int t = 0; t < G; ++t) {
          hs3[r][cb + 3 * t] = keep[it][0][t];
          hs4[r][cb + 3 * t] = keep[it][1][t];
        }
      }
    }
  } else {
    for (int i = tid; i < IR * (TC / G); i += NT) {
      int r, cb;
      row_item(i, r, cb);
      const RowSums acc = row_sums(sa, sb, tp, r, cb);
#pragma unroll
      for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int t = 0; t < G; ++t) hs[k][r][cb + 3 * t] = acc.v[k][t];
    }
  }
  __syncthreads();

  // vertical pass: thread = (row group, column); outputs rows 4*rg + t from row sums 4*rg + m
  double ss = 0.0;
  for (int i = tid; i < (TR / G) * TC; i += NT) {
    const int rb = (i / TC) * G, c = i % TC;
    if (r0 + rb >= mh || c0 + c >= mw3) continue;
    double acc[5][G];
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int t = 0; t < G; ++t) acc[k][t] = 0.0;
#pragma unroll
    for (int m = 0; m < GW; ++m) {
      double v[5];
#pragma unroll
      for (int k = 0; k < (ALIAS ? 3 : 5); ++k) v[k] = hs[k][rb + m][c];
      if constexpr (ALIAS) {
        v[3] = hs3[rb + m][c];
        v[4] = hs4[rb + m][c];
      }
#pragma unroll
      for (int t = 0; t < G; ++t) {
        if (m - t >= 0 && m - t < NTAP) {
          const double g = tp.g[m - t];
#pragma unroll
          for (int k = 0; k < 5; ++k) acc[k][t] = fma(g, v[k], acc[k][t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < G; ++t) {
      if (r0 + rb + t < mh) {
        const double mx = acc[0][t], my = acc[1][t];
        const double mxx = mx * mx, myy = my * my, mxy = mx * my;
        const double vx = acc[2][t] - mxx, vy = acc[3][t] - myy, cxy = acc[4][t] - mxy;
        const double a2 = 2.0 * cxy + c2, b2 = vx + vy + c2;
        if constexpr (CS_ONLY) {
          const double s = a2 / b2;
          ss += s;
          if constexpr (MODE == BASE_TERM_AND_PLANES) {
            const double pc = 2.0 / b2;
            const double pb = -2.0 * s / b2;
            const long plane = (long)mh * mw3;
            double* d = planes + (long)blockIdx.z * 3 * plane + (long)(r0 + rb + t) * mw3 + (c0 + c);
            d[0] = -my * pc - mx * pb;
            d[plane] = pb;
            d[2 * plane] = pc;
          }
          continue;
        }
        const double num = (2.0 * mxy + c1) * a2;
        const double den = (mxx + myy + c1) * b2;
        const double s = num / den;
        ss += s;
        if constexpr (MODE == BASE_TERM_AND_PLANES) {
          // a = y (prediction), b = t: A1 = 2 my mt + C1, B1 = my^2 + mt^2 + C1 (dssim.hip)
          const double pc = 2.0 * (2.0 * mxy + c1) / den;
          const double pb = -2.0 * s / b2;
          const double pa = 2.0 * my * a2 / den - 2.0 * mx * s / (mxx + myy + c1) - my * pc - mx * pb;
          const long plane = (long)mh * mw3;
          double* d = planes + (long)blockIdx.z * 3 * plane + (long)(r0 + rb + t) * mw3 + (c0 + c);
          d[0] = pa;
          d[plane] = pb;
          d[2 * plane] = pc;
        }
      }
    }
  }

  // the tile's NP sums, one thread each (reduce.h); PER_CHANNEL: the vertical pass gave this thread
  // column tid % TC of a tile that starts at a red column
  double v[NP];
  if constexpr (PER_CHANNEL) {
    const int ch = (tid % TC) % 3;
    v[0] = ch == 0 ? ss : 0.0, v[1] = ch == 1 ? ss : 0.0, v[2] = ch == 2 ? ss : 0.0, v[3] = sq;
  } else {
    v[0] = ss, v[1] = sq;
  }
  const double s = reduce::block_sum<NP, NT>(v, red);
  if (tid < NP) {
    const long nblk = (long)gridDim.x * gridDim.y;
    part[((long)blockIdx.z * nblk + (long)blockIdx.y * gridDim.x + blockIdx.x) * NP + tid] = s;
  }
}

// The gradient filter of dssim.hip's pass 2 as a function: the workgroup of image tile
// (blockIdx.y, blockIdx.x) leaves in f[k][t], for tid < (TR / G) * TC, the full (zero-padded)
// correlation of plane k of image blockIdx.z of planes [n][3][mh][mw3] with the window at image
// rows blockIdx.y * TR + (tid / TC) * G + t, float column blockIdx.x * TC + tid % TC.  One plane
// at a time: stage the (TR+10) x (TC+30) window of the plane above and to the left of the tile
// (zero outside the map), horizontal pass into fp64 row sums in LDS, vertical pass into registers.
__device__ __forceinline__ void adjoint_pass(const double* __restrict__ planes, int mh, int mw3, Taps tp,
                                             double (&f)[3][G]) {
  static_assert((TR / G) * TC <= NT, "a thread's outputs stay in registers across the planes");
  __shared__ double sp[IR][ICP];
  __shared__ double hs[IR][TC];

  const int tid = threadIdx.x;
  const int r0 = blockIdx.y * TR, c0 = blockIdx.x * TC;
  const long plane = (long)mh * mw3;
  // the staged window's first map row / column: pixel (r, c) collects map rows r-10..r, columns c-30..c
  const int q0 = r0 - 2 * R, p0 = c0 - 3 * 2 * R;
  const int rb = (tid / TC) * G, c = tid % TC;  // this thread's outputs: rows rb..rb+3 of column c (tid < 192)

#pragma unroll  // (f[k] stays in registers only with k a constant)
  for (int k = 0; k < 3; ++k) {
    const double* __restrict__ pk = planes + ((long)blockIdx.z * 3 + k) * plane;
    for (int i = tid; i < IR * ICP; i += NT) {
      const int r = i / ICP, cc = i % ICP;
      const int qr = q0 + r, qc = p0 + cc;
      double v = 0.0;
      if (cc < IC && qr >= 0 && qr < mh && qc >= 0 && qc < mw3) v = pk[(long)qr * mw3 + qc];
      sp[r][cc] = v;
    }
    __syncthreads();
    // horizontal pass: staged column cb + 3m holds map column c0 + cb - 30 + 3m; output column
    // cb + 3t takes it with tap g[10 - (m - t)]
    for (int i = tid; i < IR * (TC / G); i += NT) {
      int r, cb;
      row_item(i, r, cb);
      double acc[G];
#pragma unroll
      for (int t = 0; t < G; ++t) acc[t] = 0.0;
#pragma unroll
      for (int m = 0; m < GW; ++m) {
        const double x = sp[r][cb + 3 * m];
#pragma unroll
        for (int t = 0; t < G; ++t)
          if (m - t >= 0 && m - t < NTAP) acc[t] = fma(tp.g[NTAP - 1 - (m - t)], x, acc[t]);
      }
#pragma unroll
      for (int t = 0; t < G; ++t) hs[r][cb + 3 * t] = acc[t];
    }
    __syncthreads();
    // vertical pass into this thread's registers
#pragma unroll
    for (int t = 0; t < G; ++t) f[k][t] = 0.0;
    if (tid < (TR / G) * TC) {
#pragma unroll
      for (int m = 0; m < GW; ++m) {
        const double v = hs[rb + m][c];
#pragma unroll
        for (int t = 0; t < G; ++t)
          if (m - t >= 0 && m - t < NTAP) f[k][t] = fma(tp.g[NTAP - 1 - (m - t)], v, f[k][t]);
      }
    }
    __syncthreads();  // (sp and hs are written again for the next plane)
  }
}

}  // namespace ssim_tile
