// BatchNormalization of the U-Net step: forward finalize / inference coefficients / apply, the
// backward reduce / finalize / apply (with its pooled and g3 forms), and the sums that let a
// folded-BN consumer skip a pass over the activations (border sums, consumer sums).
// Conventions: colsum.h.
#include <cstdlib>

#include "bn_rows.h"
#include "colsum.h"

// ----------------------------------------------------------------------------
// BatchNormalization forward (training) finalize -- model.py:196,200.
// stat_part [rows][2][groups*C]: (sum r, sum r^2) per GEMM column.
// ----------------------------------------------------------------------------
__global__ void bn_fwd_final_kernel(const double* __restrict__ ws, int G, int C, int groups,
                                    double count, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, float* mm, float* mv,
                                    float momentum, float eps, float* scale, float* shift,
                                    float* smean, float* sinv) {
  const int c = wave_col();
  if (c >= C) return;
  const int cols = 2 * groups * C;
  double s1 = 0.0, s2 = 0.0;
  for (int gr = 0; gr < groups; ++gr) {
    s1 += fold(ws, G, cols, gr * C + c);
    s2 += fold(ws, G, cols, groups * C + gr * C + c);
  }
  const double mean = s1 / count;
  const double var = fmax(s2 / count - mean * mean, 0.0);  // biased (tf.nn.moments)
  const double inv = 1.0 / sqrt(var + (double)eps);
  const double sc = (double)gamma[c] * inv;
  if ((threadIdx.x & 63) != 0) return;
  scale[c] = (float)sc;
  shift[c] = (float)((double)beta[c] - mean * sc);
  smean[c] = (float)mean;
  sinv[c] = (float)inv;
  if (mm && mv) {
    // Keras 2.2.x on TF 1.x takes tf.nn.fused_batch_norm for 4-D NHWC input, whose
    // batch variance output is already Bessel-corrected (n/(n-1)); Keras then
    // multiplies by n/(n-(1+eps)) again before K.moving_average_update:
    // moving = moving*m + v*(1-m) with v = var_biased * n/(n-1) * n/(n-1-eps).
    const double var_u = var * (count / (count - 1.0)) * (count / (count - (1.0 + (double)eps)));
    mm[c] = (float)((double)mm[c] * momentum + mean * (1.0 - momentum));
    mv[c] = (float)((double)mv[c] * momentum + var_u * (1.0 - momentum));
  }
}

extern "C" int cnnitmo_bn_fwd_finalize(const float* stat_part, long rows, int c, int groups,
                                       double count, const float* gamma, const float* beta,
                                       float* moving_mean, float* moving_var, float momentum,
                                       float eps, float* scale, float* shift, float* save_mean,
                                       float* save_invstd, void* workspace, void* stream) {
  CNN_REQUIRE(rows > 0 && c > 0 && groups >= 1 && count > 1.0, "bn_fwd_finalize: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  const int G = colsum_stage1_launch(stat_part, rows, 2 * groups * c, workspace, s);
  hipLaunchKernelGGL(bn_fwd_final_kernel, dim3(wave_grid(c)), dim3(256), 0, s,
                     (const double*)workspace, G, c, groups, count, gamma, beta, moving_mean,
                     moving_var, momentum, eps, scale, shift, save_mean, save_invstd);
  return cnnitmo_check_launch("bn_fwd_finalize");
}

__global__ void bn_infer_kernel(int C, const float* g, const float* b, const float* mm,
                                const float* mv, float eps, float* scale, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float sc = g[c] / sqrtf(mv[c] + eps);
  scale[c] = sc;
  shift[c] = b[c] - mm[c] * sc;
}

extern "C" int cnnitmo_bn_infer_coeffs(int c, const float* gamma, const float* beta,
                                       const float* mmean, const float* mvar, float eps,
                                       float* scale, float* shift, void* stream) {
  hipLaunchKernelGGL(bn_infer_kernel, dim3((c + 255) / 256), dim3(256), 0, (hipStream_t)stream, c,
                     gamma, beta, mmean, mvar, eps, scale, shift);
  return cnnitmo_check_launch("bn_infer_coeffs");
}

// y view = r*scale + shift [+ Dropout(0.5)].  One thread = one 16-byte vector.  lg >= 0:
// C / VE = 2^lg and fewer than 2^31 vectors, so the (pixel, channel) split of a vector index
// is a shift and a mask in 32 bits (the 64-bit division cost as much as the hash).
template <typename T>
__global__ void bn_apply_kernel(const T* __restrict__ r, long P, int C, const float* __restrict__ sc,
                                const float* __restrict__ sh, T* __restrict__ y, long y_ld, int y_off,
                                int drop, uint64_t dbase, int lg) {
  constexpr int VE = Vec16<T>::N;
  const int cv = C / VE;
  const long total = P * cv;
  auto one = [&](long p, int c0) {
    float v[VE], a[VE], b[VE];
    Pack16<T>::load(r + (size_t)p * C + c0, v);
#pragma unroll
    for (int e = 0; e < VE; e += 4) {
      const float4 s4 = *reinterpret_cast<const float4*>(sc + c0 + e), h4 = *reinterpret_cast<const float4*>(sh + c0 + e);
      a[e] = s4.x; a[e + 1] = s4.y; a[e + 2] = s4.z; a[e + 3] = s4.w;
      b[e] = h4.x; b[e + 1] = h4.y; b[e + 2] = h4.z; b[e + 3] = h4.w;
    }
    const uint64_t i0 = (uint64_t)p * C + c0;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      float o = v[e] * a[e] + b[e];
      if (drop) o = dropout_keep(dbase, i0 + e) ? o * 2.f : 0.f;
      v[e] = o;
    }
    Pack16<T>::store(y + (size_t)p * y_ld + y_off + c0, v);
  };
  if (lg >= 0) {
    const unsigned tot = (unsigned)total, msk = (unsigned)cv - 1u;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += gridDim.x * blockDim.x)
      one((long)(i >> lg), (int)(i & msk) * VE);
    return;
  }
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long p = i / cv;
    one(p, (int)(i - p * cv) * VE);
  }
}

extern "C" int cnnitmo_bn_apply(int dtype, const void* r, long p, int c, const float* scale,
                                const float* shift, void* y, int y_ld, int y_off, int flags,
                                uint64_t drop_seed, int drop_layer, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int drop = (flags & CNNITMO_DROPOUT) ? 1 : 0;
  const uint64_t base = dropout_base(drop_seed, (uint64_t)drop_layer);
  CNN_REQUIRE(c % 8 == 0 && y_ld % 8 == 0 && y_off % 8 == 0, "bn_apply: channels must be multiples of 8");
  CNN_REQUIRE((uintptr_t)scale % 16 == 0 && (uintptr_t)shift % 16 == 0, "bn_apply: scale/shift must be 16-byte aligned");
  const int ve = dtype == CNNITMO_BF16 ? 8 : 4, cv = c / ve;
  const int lg = ((cv & (cv - 1)) == 0 && p * cv < (1L << 31)) ? __builtin_ctz((unsigned)cv) : -1;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(grid_for(p * c / ve)), dim3(256), 0, s, (const T*)r, p, c, scale,
                       shift, (T*)y, (long)y_ld, y_off, drop, base, lg);
  });
  return cnnitmo_check_launch("bn_apply");
}

// ----------------------------------------------------------------------------
// BN backward (thread layout and the shared device helpers: bn_rows.h).
// ----------------------------------------------------------------------------
static constexpr int BWD_BLOCKS = 1024;

static int bwd_blocks() { return BWD_BLOCKS; }

extern "C" int cnnitmo_bn_bwd_rows(long p, int c) {
  (void)c;
  return (int)std::max<long>(1, std::min<long>(bwd_blocks(), (p + 7) / 8));
}

template <typename T>
__global__ void bn_bwd_reduce_kernel(const T* __restrict__ dy, long dy_ld, int dy_off,
                                     const T* __restrict__ r, long r_ld, int r_off, long P, int C,
                                     const float* __restrict__ mean, const float* __restrict__ inv,
                                     int drop, uint64_t dbase, float* __restrict__ part) {
  constexpr int VE = Vec16<T>::N;
  const int tpp = C / VE, rows = 256 / tpp;
  const int tid = threadIdx.x;
  const int row = tid / tpp, cv = tid - row * tpp, c0 = cv * VE;
  float acc[2][VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) acc[0][e] = acc[1][e] = 0.f;
  float mu[VE], is[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    mu[e] = row < rows ? mean[c0 + e] : 0.f;
    is[e] = row < rows ? inv[c0 + e] : 0.f;
  }
  if (row < rows) {
    for (long p = (long)blockIdx.x * rows + row; p < P; p += (long)gridDim.x * rows) {
      float g[VE], rv[VE];
      load_dy<T>(dy, dy_ld, dy_off, p, C, c0, drop, dbase, g);
      Pack16<T>::load(r + (size_t)p * r_ld + r_off + c0, rv);
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        acc[0][e] += g[e];
        acc[1][e] += g[e] * (rv[e] - mu[e]) * is[e];
      }
    }
  }
  block_reduce_rows<VE, 2>(acc, C, part);
}

extern "C" int cnnitmo_bn_bwd_reduce(int dtype, const void* dy, int dy_ld, int dy_off,
                                     const void* r, int r_ld, int r_off, long p, int c, const float* mean,
                                     const float* invstd, int flags, uint64_t drop_seed,
                                     int drop_layer, float* part, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int G = cnnitmo_bn_bwd_rows(p, c);
  const int drop = (flags & CNNITMO_DROPOUT) ? 1 : 0;
  const uint64_t base = dropout_base(drop_seed, (uint64_t)drop_layer);
  const int VE = dtype == CNNITMO_BF16 ? 8 : 4;
  CNN_REQUIRE(c % VE == 0 && c / VE <= 256 && dy_ld % VE == 0 && dy_off % VE == 0 &&
              r_ld % VE == 0 && r_off % VE == 0, "bn_bwd_reduce: unsupported channel count %d", c);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<T>, dim3(G), dim3(256), 0, s, (const T*)dy, (long)dy_ld, dy_off,
                       (const T*)r, (long)r_ld, r_off, p, c, mean, invstd, drop, base, part);
  });
  return cnnitmo_check_launch("bn_bwd_reduce");
}

// coef [3][C]: dz = [r>0] * (a*dy - b*r + e)
__global__ void bn_bwd_final_kernel(const double* __restrict__ ws, int G, int C, double count,
                                    const float* __restrict__ gamma, const float* __restrict__ mean,
                                    const float* __restrict__ inv, float* dgamma, float* dbeta,
                                    float* coef) {
  const int c = wave_col();
  if (c >= C) return;
  const double sdy = fold(ws, G, 2 * C, c), sdyr = fold(ws, G, 2 * C, C + c);
  if ((threadIdx.x & 63) != 0) return;
  if (dgamma) dgamma[c] = (float)sdyr;
  if (dbeta) dbeta[c] = (float)sdy;
  const double a = (double)gamma[c] * inv[c];
  const double b = a * inv[c] * sdyr / count;
  const double e = b * mean[c] - a * sdy / count;
  coef[c] = (float)a;
  coef[C + c] = (float)b;
  coef[2 * C + c] = (float)e;
}

extern "C" int cnnitmo_bn_bwd_finalize(const float* part, long rows, int c, double count,
                                       const float* gamma, const float* mean, const float* invstd,
                                       float* dgamma, float* dbeta, float* coef, void* workspace,
                                       void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int G = colsum_stage1_launch(part, rows, 2 * c, workspace, s);
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(wave_grid(c)), dim3(256), 0, s,
                     (const double*)workspace, G, c, count, gamma, mean, invstd, dgamma, dbeta, coef);
  return cnnitmo_check_launch("bn_bwd_finalize");
}

// NP = 1: partial sums of dz per channel (bias gradient); NP = 4: split by the
// pixel's (h&1, w&1) parity, i.e. per Conv2DTranspose tap of the producer
// (needed by the folded-BN wgrad correction of the tconv; db = their sum).
// G3: dy is the rank-3 product dy[p][c] = sum_o g3[p][o] * wh[o][c] of the sigmoid
// head's per-pixel output gradient g3 and its [3][C] weights (cnnitmo_head_fwd_bwd_g3),
// formed in fp32 on the fly instead of being read as a C-channel tensor.
template <typename T, int NP, bool ROUTE, bool G3 = false>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ dy, long dy_ld, int dy_off,
                                    const T* __restrict__ r, long r_ld, int r_off, long P, int C,
                                    const float* __restrict__ coef, int nobn, int drop,
                                    uint64_t dbase, T* __restrict__ dz, float* __restrict__ part,
                                    int H, int W, const T* __restrict__ dyp,
                                    const uint8_t* __restrict__ pidx, const float* __restrict__ g3,
                                    const float* __restrict__ wh) {
  constexpr int VE = Vec16<T>::N;
  const int tpp = C / VE, rows = 256 / tpp;
  const int tid = threadIdx.x;
  const int row = tid / tpp, cv = tid - row * tpp, c0 = cv * VE;
  float acc[NP][VE];
  float ca[VE], cb[VE], ce[VE];
  float w3[G3 ? 3 : 1][VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) {
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k][e] = 0.f;
    if constexpr (G3) {
#pragma unroll
      for (int o = 0; o < 3; ++o) w3[o][e] = row < rows ? wh[o * C + c0 + e] : 0.f;
    }
    const bool ok = row < rows && !nobn;
    ca[e] = ok ? coef[c0 + e] : 1.f;
    cb[e] = ok ? coef[C + c0 + e] : 0.f;
    ce[e] = ok ? coef[2 * C + c0 + e] : 0.f;
  }
  if (row < rows) {
    const int hw = H * W;  // ROUTE / NP 4 index math in 32 bits (checked by the launchers)
    for (long p = (long)blockIdx.x * rows + row; p < P; p += (long)gridDim.x * rows) {
      float g[VE], rv[VE];
      if constexpr (G3) {
        const float q0 = g3[p * 3], q1 = g3[p * 3 + 1], q2 = g3[p * 3 + 2];
#pragma unroll
        for (int e = 0; e < VE; ++e) g[e] = q0 * w3[0][e] + q1 * w3[1][e] + q2 * w3[2][e];
      } else {
        load_dy<T>(dy, dy_ld, dy_off, p, C, c0, drop, dbase, g);
      }
      Pack16<T>::load(r + (size_t)p * r_ld + r_off + c0, rv);
      if constexpr (ROUTE) {  // + the MaxPooling2D gradient routed to this pixel
        const int pi = (int)p;
        const int n = pi / hw, rem = pi - n * hw;
        const int hh = rem / W, ww = rem - hh * W, Ho = H / 2, Wo = W / 2;
        if ((hh >> 1) < Ho && (ww >> 1) < Wo) {
          const long po = ((long)n * Ho + (hh >> 1)) * Wo + (ww >> 1);
          const int k = ((hh & 1) << 1) | (ww & 1);
          float gp[VE];
          Pack16<T>::load(dyp + (size_t)po * C + c0, gp);
          const uint8_t* ip = pidx + (size_t)po * C + c0;
          uint8_t arg[VE];
          if constexpr (VE == 8) {
            const uint2 a2 = *(const uint2*)ip;
            __builtin_memcpy(arg, &a2, 8);
          } else {
            const uint32_t a1 = *(const uint32_t*)ip;
            __builtin_memcpy(arg, &a1, 4);
          }
#pragma unroll
          for (int e = 0; e < VE; ++e) g[e] += arg[e] == k ? gp[e] : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const float d = rv[e] > 0.f ? (ca[e] * g[e] - cb[e] * rv[e] + ce[e]) : 0.f;
        g[e] = d;
      }
      Pack16<T>::store(dz + (size_t)p * C + c0, g);
      int k = 0;
      if constexpr (NP == 4) {
        const int rem = (int)p % hw;
        const int hh = rem / W, ww = rem - hh * W;
        k = ((hh & 1) << 1) | (ww & 1);
      }
      // bias gradient from the stored (rounded) dz, as the weight gradient sees it
#pragma unroll
      for (int kk = 0; kk < NP; ++kk)
        if (kk == k) {
#pragma unroll
          for (int e = 0; e < VE; ++e) acc[kk][e] += to_f32(from_f32<T>(g[e]));
        }
    }
  }
  block_reduce_rows<VE, NP>(acc, C, part);
}

// (A four-pixel form of this pass -- 2x2 windows, every load issued first, the
// pooled gradient read once per window -- measured no faster: 6.84 vs 6.82 ms/step
// for the routed applies, 4.6 vs 3.9 for the g3 one; profiles/r02e1_*.)

extern "C" int cnnitmo_bn_bwd_apply(int dtype, const void* dy, int dy_ld, int dy_off,
                                    const void* r, int r_ld, int r_off, long p, int c,
                                    const float* coef, int flags, uint64_t drop_seed, int drop_layer,
                                    int h, int w, void* dz, float* part, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int G = cnnitmo_bn_bwd_rows(p, c);
  const int drop = (flags & CNNITMO_DROPOUT) ? 1 : 0;
  const int nobn = (flags & CNNITMO_NO_BN) ? 1 : 0;
  const uint64_t base = dropout_base(drop_seed, (uint64_t)drop_layer);
  const int VE = dtype == CNNITMO_BF16 ? 8 : 4;
  CNN_REQUIRE(c % VE == 0 && c / VE <= 256 && dy_ld % VE == 0 && dy_off % VE == 0 &&
              r_ld % VE == 0 && r_off % VE == 0, "bn_bwd_apply: unsupported channel count %d", c);
  CNN_REQUIRE(nobn || coef, "bn_bwd_apply: missing coefficients");
  const bool par = flags & CNNITMO_PARITY;
  CNN_REQUIRE(!par || (h > 0 && w > 0), "bn_bwd_apply: PARITY needs h, w");
  CNN_REQUIRE(!par || p < (1L << 31), "bn_bwd_apply: too many pixels");
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
#define BNA(NP)                                                                                   \
  hipLaunchKernelGGL((bn_bwd_apply_kernel<T, NP, false>), dim3(G), dim3(256), 0, s, (const T*)dy, \
                     (long)dy_ld, dy_off, (const T*)r, (long)r_ld, r_off, p, c, coef, nobn, drop, \
                     base, (T*)dz, part, h, w, nullptr, nullptr, nullptr, nullptr)
    if (par) { BNA(4); } else { BNA(1); }
#undef BNA
  });
  return cnnitmo_check_launch("bn_bwd_apply");
}

extern "C" int cnnitmo_bn_bwd_apply_pooled(int dtype, const void* dy, int dy_ld, int dy_off, const void* r,
                                           int r_ld, int r_off, int n, int h, int w, int c,
                                           const float* coef, const void* dy_pool, const uint8_t* idx,
                                           void* dz, float* part, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const long p = (long)n * h * w;
  const int G = cnnitmo_bn_bwd_rows(p, c);
  const int VE = dtype == CNNITMO_BF16 ? 8 : 4;
  CNN_REQUIRE(c % 8 == 0 && c / VE <= 256 && dy_ld % 8 == 0 && dy_off % 8 == 0 && r_ld % 8 == 0 &&
              r_off % 8 == 0 && coef && dy_pool && idx, "bn_bwd_apply_pooled: unsupported arguments (c=%d)", c);
  CNN_REQUIRE(p < (1L << 31), "bn_bwd_apply_pooled: too many pixels");
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, 1, true>), dim3(G), dim3(256), 0, s, (const T*)dy, (long)dy_ld,
                       dy_off, (const T*)r, (long)r_ld, r_off, p, c, coef, 0, 0, (uint64_t)0, (T*)dz, part, h, w,
                       (const T*)dy_pool, idx, nullptr, nullptr);
  });
  return cnnitmo_check_launch("bn_bwd_apply_pooled");
}

extern "C" int cnnitmo_bn_bwd_apply_g3(int dtype, const float* g3, const float* wh, const void* r, int r_ld,
                                       int r_off, long p, int c, const float* coef, void* dz, float* part,
                                       void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int G = cnnitmo_bn_bwd_rows(p, c);
  const int VE = dtype == CNNITMO_BF16 ? 8 : 4;
  CNN_REQUIRE(c % VE == 0 && c / VE <= 256 && r_ld % VE == 0 && r_off % VE == 0 && coef && g3 && wh,
              "bn_bwd_apply_g3: unsupported arguments (c=%d)", c);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, 1, false, true>), dim3(G), dim3(256), 0, s, nullptr, 0L, 0,
                       (const T*)r, (long)r_ld, r_off, p, c, coef, 0, 0, (uint64_t)0, (T*)dz, part, 0, 0, nullptr,
                       nullptr, g3, wh);
  });
  return cnnitmo_check_launch("bn_bwd_apply_g3");
}

// Border sums of an output gradient dz [n][h][w][c] for the folded-BN conv
// weight-gradient correction: rows [n*BS_SEG][8][c] of partials (reduce with
// cnnitmo_colsum) = {row 0, row h-1, col 0, col w-1, (0,0), (0,w-1), (h-1,0), (h-1,w-1)}.
constexpr int BS_SEG = 16;
template <typename T>
__global__ void border_sums_kernel(const T* __restrict__ dz, int H, int W, int C,
                                   float* __restrict__ part) {
  const int img = blockIdx.x / BS_SEG, seg = blockIdx.x % BS_SEG;
  const T* base = dz + (size_t)img * H * W * C;
  float* out = part + (size_t)blockIdx.x * 8 * C;
  const int w0 = (int)((long)W * seg / BS_SEG), w1 = (int)((long)W * (seg + 1) / BS_SEG);
  const int h0 = (int)((long)H * seg / BS_SEG), h1 = (int)((long)H * (seg + 1) / BS_SEG);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float top = 0.f, bot = 0.f, lef = 0.f, rig = 0.f;
    for (int w = w0; w < w1; ++w) {
      top += to_f32(base[(size_t)w * C + c]);
      bot += to_f32(base[((size_t)(H - 1) * W + w) * C + c]);
    }
    for (int hh = h0; hh < h1; ++hh) {
      lef += to_f32(base[((size_t)hh * W) * C + c]);
      rig += to_f32(base[((size_t)hh * W + W - 1) * C + c]);
    }
    const bool s0 = seg == 0;
    out[0 * C + c] = top;
    out[1 * C + c] = bot;
    out[2 * C + c] = lef;
    out[3 * C + c] = rig;
    out[4 * C + c] = s0 ? to_f32(base[c]) : 0.f;
    out[5 * C + c] = s0 ? to_f32(base[(size_t)(W - 1) * C + c]) : 0.f;
    out[6 * C + c] = s0 ? to_f32(base[((size_t)(H - 1) * W) * C + c]) : 0.f;
    out[7 * C + c] = s0 ? to_f32(base[((size_t)(H - 1) * W + W - 1) * C + c]) : 0.f;
  }
}

extern "C" int cnnitmo_border_rows(int n) { return n * BS_SEG; }

extern "C" int cnnitmo_border_sums(int dtype, const void* dz, int n, int h, int w, int c, float* part,
                                   void* stream) {
  CNN_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, "border_sums: empty");
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(border_sums_kernel<T>, dim3(n * BS_SEG), dim3(256), 0, s, (const T*)dz, h, w, c, part);
  });
  return cnnitmo_check_launch("border_sums");
}

// ----------------------------------------------------------------------------
// BN-backward sums without a pass over the activations.  For a BN output v whose
// gradient is the input-gradient of a linear consumer (conv3x3 'same', tconv2x2,
// the 1x1 head), both sums the BN backward needs follow from quantities the
// consumer's weight gradient already produced:
//   sum_q dy[q][ci]             = sum_{co,t} W[co][t][ci] * V[co][t]
//   sum_q dy[q][ci] * rhat[q][ci] = inv[ci] * sum_{co,t} W[co][t][ci] * (raw[co][t][ci] - mean[ci] * V[co][t])
// raw = sum_p dz[p][co] * r[p + off_t][ci] (zero padded) and V[co][t] = the sum of dz
// over the pixels whose tap t lands inside the image (conv: db - border sums;
// tconv: the per-tap parity sums; head: db).  Exact in real arithmetic (the
// dgrad is the transpose of the same linear map), O(weights) work.
// part[0][c] = sum dy, part[1][c] = sum dy * rhat (one row for cnnitmo_bn_bwd_finalize).
// mode 1: conv3x3, w/raw [cout][9][cin_tot], V from db[cout] and border sums bs[8][cout]
// mode 2: tconv2x2, w/raw [4][cout][cin_tot], V = par[4*cout]
// mode 3: head 1x1, w/raw [3][cin_tot], V = db[3]
// ----------------------------------------------------------------------------
__device__ __forceinline__ double conv_v(const float* db, const float* bs, int C, int co, int t) {
  const int r = t / 3, q = t - 3 * r;
  double o = 0.0;
  if (r == 0) o += bs[0 * C + co];
  if (r == 2) o += bs[1 * C + co];
  if (q == 0) o += bs[2 * C + co];
  if (q == 2) o += bs[3 * C + co];
  if (r == 0 && q == 0) o -= bs[4 * C + co];
  if (r == 0 && q == 2) o -= bs[5 * C + co];
  if (r == 2 && q == 0) o -= bs[6 * C + co];
  if (r == 2 && q == 2) o -= bs[7 * C + co];
  return (double)db[co] - o;
}

// Grid (c/64, CNNITMO_CONSUMER_ROWS); a block's 4 waves split its slice of the
// K = cout*taps (co, tap) pairs (w/raw rows k*cin_tot, coalesced over ci) and
// reduce in LDS; every grid row writes one partial row (linear in the slices).
__global__ void bn_consumer_sums_kernel(int mode, const float* __restrict__ w, const float* __restrict__ raw,
                                        int cout, int cin_tot, int ci0, int c, const float* __restrict__ db,
                                        const float* __restrict__ vt, const float* __restrict__ mean,
                                        const float* __restrict__ inv, float* __restrict__ part) {
  const int cl = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + cl;
  const int K = cout * (mode == 1 ? 9 : (mode == 2 ? 4 : 1));
  const int slices = gridDim.y * 4, sl = blockIdx.y * 4 + sub;
  const int k0 = (int)((long)K * sl / slices), k1 = (int)((long)K * (sl + 1) / slices);
  double swv = 0.0, swr = 0.0;
  if (j < c) {
    const int ci = ci0 + j;
    for (int k = k0; k < k1; ++k) {
      const double v = mode == 1 ? conv_v(db, vt, cout, k / 9, k % 9) : (mode == 2 ? (double)vt[k] : (double)db[k]);
      const size_t idx = (size_t)k * cin_tot + ci;
      const double wv = w[idx];
      swv += wv * v;
      swr += wv * raw[idx];
    }
  }
  __shared__ double red[2][256];
  red[0][threadIdx.x] = swv;
  red[1][threadIdx.x] = swr;
  __syncthreads();
  if (sub == 0 && j < c) {
    swv = ((red[0][cl] + red[0][cl + 64]) + red[0][cl + 128]) + red[0][cl + 192];
    swr = ((red[1][cl] + red[1][cl + 64]) + red[1][cl + 128]) + red[1][cl + 192];
    float* o = part + (size_t)blockIdx.y * 2 * c;
    o[j] = (float)swv;
    o[c + j] = (float)(inv[j] * (swr - (double)mean[j] * swv));
  }
}

extern "C" int cnnitmo_bn_consumer_sums(int mode, const float* w, const float* raw, int cout, int cin_tot,
                                        int ci0, int c, const float* db, const float* vtab,
                                        const float* mean, const float* invstd, float* part,
                                        void* stream) {
  CNN_REQUIRE(mode >= 1 && mode <= 3 && ci0 >= 0 && ci0 + c <= cin_tot && (mode == 2 || db),
              "bn_consumer_sums: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_consumer_sums_kernel, dim3((c + 63) / 64, CNNITMO_CONSUMER_ROWS), dim3(256), 0, s,
                     mode, w, raw, cout, cin_tot, ci0, c, db, vtab, mean, invstd, part);
  return cnnitmo_check_launch("bn_consumer_sums");
}
