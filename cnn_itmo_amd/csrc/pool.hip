// MaxPooling2D forward and backward, and its share of the BN-backward sums of a folded pool
// input.  Conventions: colsum.h; the row-partial helpers: bn_rows.h.
#include <cstdlib>

#include "bn_rows.h"
#include "colsum.h"

// ----------------------------------------------------------------------------
// MaxPooling2D 2x2 s2 -- model.py:210,215,220,227.  Tie rule: first maximum in
// window order (0,0),(0,1),(1,0),(1,1) (strict '>' scan), shared with the oracle.
// ----------------------------------------------------------------------------
template <typename T>
__global__ void maxpool_fwd_kernel(const T* __restrict__ x, long x_ld, int x_off, int N, int H,
                                   int W, int C, T* __restrict__ y, uint8_t* __restrict__ idx,
                                   const float* __restrict__ sc, const float* __restrict__ sh) {
  constexpr int VE = Vec16<T>::N;
  const int Ho = H / 2, Wo = W / 2, cv = C / VE;
  const long total = (long)N * Ho * Wo * cv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int pi = (int)(i / cv);  // 32-bit index math from here (launcher: < 2^31 pixels)
    const long po = pi;
    const int c0 = (int)(i - po * cv) * VE;
    const int n = pi / (Ho * Wo);
    const int rem = pi - n * (Ho * Wo);
    const int ho = rem / Wo, wo = rem - ho * Wo;
    float best[VE], win[4][VE];
    uint8_t arg[VE];
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // the whole window's loads first
      const long pin = ((long)n * H + 2 * ho + (k >> 1)) * W + 2 * wo + (k & 1);
      Pack16<T>::load(x + (size_t)pin * x_ld + x_off + c0, win[k]);
    }
    if (sc) {  // folded BN: pool y = r*s + h (the max of y, whatever the sign of s); once per chunk
      float s8[VE], h8[VE];
      Pack16<float>::load(sc + c0, s8);
      Pack16<float>::load(sh + c0, h8);
      if constexpr (VE == 8) {
        Pack16<float>::load(sc + c0 + 4, s8 + 4);
        Pack16<float>::load(sh + c0 + 4, h8 + 4);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < VE; ++e) win[k][e] = win[k][e] * s8[e] + h8[e];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        if (k == 0 || win[k][e] > best[e]) {
          best[e] = win[k][e];
          arg[e] = (uint8_t)k;
        }
      }
    }
    Pack16<T>::store(y + (size_t)po * C + c0, best);
    if constexpr (VE == 8) {
      uint2 a;
      a.x = arg[0] | (arg[1] << 8) | (arg[2] << 16) | ((uint32_t)arg[3] << 24);
      a.y = arg[4] | (arg[5] << 8) | (arg[6] << 16) | ((uint32_t)arg[7] << 24);
      *reinterpret_cast<uint2*>(idx + (size_t)po * C + c0) = a;
    } else {
      *reinterpret_cast<uint32_t*>(idx + (size_t)po * C + c0) =
          arg[0] | (arg[1] << 8) | (arg[2] << 16) | ((uint32_t)arg[3] << 24);
    }
  }
}

// Rows of pooled pixels per 256-thread block: tpp = C/VE threads per pixel.
template <typename T>
__global__ void maxpool_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx, int H, int W,
                                   long Pp, int C, T* __restrict__ dx, long dx_ld, int dx_off) {
  constexpr int VE = Vec16<T>::N;
  const int tpp = C / VE, rows = 256 / tpp;
  const int row = threadIdx.x / tpp, cv = threadIdx.x - row * tpp, c0 = cv * VE;
  const int Ho = H / 2, Wo = W / 2;
  if (row >= rows) return;
  for (long po = (long)blockIdx.x * rows + row; po < Pp; po += (long)gridDim.x * rows) {
    const int n = (int)po / (Ho * Wo);  // 32-bit index math (launcher: < 2^31 pixels)
    const int rem = (int)po - n * (Ho * Wo);
    const int ho = rem / Wo, wo = rem - ho * Wo;
    float g[VE];
    Pack16<T>::load(dy + (size_t)po * C + c0, g);
    uint8_t arg[VE];
    load_args<VE>(idx + (size_t)po * C + c0, arg);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bool any = false;
#pragma unroll
      for (int e = 0; e < VE; ++e) any |= arg[e] == k;
      if (!any) continue;
      const long pin = ((long)n * H + 2 * ho + (k >> 1)) * W + 2 * wo + (k & 1);
      T* q = dx + (size_t)pin * dx_ld + dx_off + c0;
      float v[VE];
      Pack16<T>::load(q, v);
#pragma unroll
      for (int e = 0; e < VE; ++e)
        if (arg[e] == k) v[e] += g[e];
      Pack16<T>::store(q, v);
    }
  }
}

// The MaxPooling2D share of the BN-backward sums of a folded pool input (see
// cnnitmo_bn_consumer_sums): sum_p dyp[p] and sum_p dyp[p] * rhat[argmax(p)].
// The 2x2 window of r is read whole (two coalesced pixel pairs) and the argmax
// element selected per channel.
// PRE: r is the pooled r itself ([Pp][C] dense: the producer's epilogue wrote r at the
// window index, cnnitmo_conv3x3_fwd_pool), so no window is read and idx is not needed.
template <typename T, bool PRE = false>
__global__ void pool_bnsums_kernel(const T* __restrict__ dyp, const uint8_t* __restrict__ idx, int H, int W,
                                   long Pp, int C, const T* __restrict__ r, long r_ld, int r_off,
                                   const float* __restrict__ mean, const float* __restrict__ inv,
                                   float* __restrict__ part) {
  constexpr int VE = Vec16<T>::N;
  const int tpp = C / VE, rows = 256 / tpp;
  const int row = threadIdx.x / tpp, cv = threadIdx.x - row * tpp, c0 = cv * VE;
  const int Ho = H / 2, Wo = W / 2;
  float acc[2][VE], mu[VE], is[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    acc[0][e] = acc[1][e] = 0.f;
    mu[e] = row < rows ? mean[c0 + e] : 0.f;
    is[e] = row < rows ? inv[c0 + e] : 0.f;
  }
  if (row < rows) {
    for (long po = (long)blockIdx.x * rows + row; po < Pp; po += (long)gridDim.x * rows) {
      const int n = (int)po / (Ho * Wo);  // 32-bit index math (launcher: < 2^31 pixels)
      const int rem = (int)po - n * (Ho * Wo);
      const int ho = rem / Wo, wo = rem - ho * Wo;
      float g[VE], rw[4][VE];
      Pack16<T>::load(dyp + (size_t)po * C + c0, g);
      if constexpr (PRE) {
        Pack16<T>::load(r + (size_t)po * C + c0, rw[0]);
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          acc[0][e] += g[e];
          acc[1][e] += g[e] * (rw[0][e] - mu[e]) * is[e];
        }
        continue;
      }
      uint8_t arg[VE];
      load_args<VE>(idx + (size_t)po * C + c0, arg);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long pin = ((long)n * H + 2 * ho + (k >> 1)) * W + 2 * wo + (k & 1);
        Pack16<T>::load(r + (size_t)pin * r_ld + r_off + c0, rw[k]);
      }
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const int k = arg[e];
        const float rv = k == 0 ? rw[0][e] : (k == 1 ? rw[1][e] : (k == 2 ? rw[2][e] : rw[3][e]));
        acc[0][e] += g[e];
        acc[1][e] += g[e] * (rv - mu[e]) * is[e];
      }
    }
  }
  block_reduce_rows<VE, 2>(acc, C, part);
}

extern "C" int cnnitmo_pool_bnsums_pooled(int dtype, const void* dyp, const void* pr, int n, int h, int w, int c,
                                          const float* mean, const float* invstd, float* part, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int VE = dtype == CNNITMO_BF16 ? 8 : 4;
  CNN_REQUIRE(c % 8 == 0 && c / VE <= 256 && dyp && pr, "pool_bnsums_pooled: unsupported channel count %d", c);
  const long Pp = (long)n * (h / 2) * (w / 2);
  CNN_REQUIRE(Pp < (1L << 31), "pool_bnsums_pooled: too many pixels");
  const int G = cnnitmo_bn_bwd_rows(Pp, c);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((pool_bnsums_kernel<T, true>), dim3(G), dim3(256), 0, s, (const T*)dyp, nullptr, h, w, Pp, c,
                       (const T*)pr, (long)c, 0, mean, invstd, part);
  });
  return cnnitmo_check_launch("pool_bnsums_pooled");
}

extern "C" int cnnitmo_maxpool2x2_fwd(int dtype, const void* x, int x_ld, int x_off, int n, int h,
                                      int w, int c, void* y, uint8_t* idx, const float* scale,
                                      const float* shift, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  CNN_REQUIRE(c % 8 == 0 && x_ld % 8 == 0 && x_off % 8 == 0, "maxpool_fwd: channels must be multiples of 8");
  const long work = (long)n * (h / 2) * (w / 2) * c;
  CNN_REQUIRE((long)n * (h / 2) * (w / 2) < (1L << 31), "maxpool_fwd: too many pixels");
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(grid_for(work / Vec16<T>::N)), dim3(256), 0, s, (const T*)x,
                       (long)x_ld, x_off, n, h, w, c, (T*)y, idx, scale, shift);
  });
  return cnnitmo_check_launch("maxpool_fwd");
}

extern "C" int cnnitmo_maxpool2x2_bwd(int dtype, const void* dy, const uint8_t* idx, int n, int h, int w,
                                      int c, void* dx, int dx_ld, int dx_off, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int VE = dtype == CNNITMO_BF16 ? 8 : 4;
  CNN_REQUIRE(c % 8 == 0 && dx_ld % 8 == 0 && dx_off % 8 == 0 && c / VE <= 256,
              "maxpool_bwd: channels must be multiples of 8 (at most 1024/2048)");
  const long Pp = (long)n * (h / 2) * (w / 2);
  const int rows = 256 / (c / VE);
  const int G = (int)std::max<long>(1, std::min<long>((Pp + rows - 1) / rows, 8192));
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(G), dim3(256), 0, s, (const T*)dy, idx, h, w, Pp, c, (T*)dx,
                       (long)dx_ld, dx_off);
  });
  return cnnitmo_check_launch("maxpool_bwd");
}

extern "C" int cnnitmo_pool_bnsums(int dtype, const void* dyp, const uint8_t* idx, int n, int h, int w,
                                   int c, const void* r, int r_ld, int r_off, const float* mean,
                                   const float* invstd, float* part, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int VE = dtype == CNNITMO_BF16 ? 8 : 4;
  CNN_REQUIRE(c % 8 == 0 && r_ld % 8 == 0 && r_off % 8 == 0 && c / VE <= 256,
              "pool_bnsums: unsupported channel count %d", c);
  const long Pp = (long)n * (h / 2) * (w / 2);
  CNN_REQUIRE(Pp < (1L << 31), "pool_bnsums: too many pixels");
  const int G = cnnitmo_bn_bwd_rows(Pp, c);
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(pool_bnsums_kernel<T>, dim3(G), dim3(256), 0, s, (const T*)dyp, idx, h, w, Pp, c,
                       (const T*)r, (long)r_ld, r_off, mean, invstd, part);
  });
  return cnnitmo_check_launch("pool_bnsums");
}
