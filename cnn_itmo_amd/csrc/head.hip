// The sigmoid head: two kernel families (head2_kernel and its fallback head_kernel), the six
// training losses, the given-gradient form, and the finalize pass.  Conventions: colsum.h.
#include <cmath>
#include <cstdlib>

#include "colsum.h"

// ----------------------------------------------------------------------------
// Head: Conv2D(3, 1, activation='sigmoid') + the training loss (MSE, model.py:281, or
// another CNNITMO_LOSS_*: loss_term below) + categorical accuracy (model.py:276,281).
// LPP = cin/VE lanes share one pixel.
// part row layout: [loss, correct, db0..2, dW[3][cin]]
// ----------------------------------------------------------------------------
static constexpr int HEAD_BLOCKS = 1024;
#ifndef HEAD_U
#define HEAD_U 4
#endif
extern "C" int cnnitmo_head_rows(long p) {
  return (int)std::max<long>(1, std::min<long>(HEAD_BLOCKS, (p + 31) / 32));
}

// The training loss of one output element (cnn_itmo.h, CNNITMO_LOSS_*): its term l and
// g = dl/dz, z the head's logit, y = sigmoid(z), t the target; fp32, without the 1/numel
// of the mean.  Both head kernels call this and nothing else differs between the losses.
// CNNITMO_LOSS_GIVEN: dyv = dL/dy comes from outside, already normalised; no term of its own.
template <int LOSS>
__device__ __forceinline__ void loss_term(float z, float y, float t, float& l, float& g, float dyv = 0.f) {
  if constexpr (LOSS == CNNITMO_LOSS_MSE) {
    const float e = y - t;
    l = e * e;
    g = 2.f * e * y * (1.f - y);
  } else if constexpr (LOSS == CNNITMO_LOSS_MAE) {
    const float e = y - t;
    l = fabsf(e);
    g = (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) * y * (1.f - y);
  } else if constexpr (LOSS == CNNITMO_LOSS_LOGCOSH) {
    // ln cosh x = |x| + log1p(exp(-2|x|)) - ln 2 (Keras: x + softplus(-2x) - ln 2)
    const float e = y - t, a = fabsf(e);
    l = a + log1pf(expf(-2.f * a)) - 0.69314718055994531f;
    g = tanhf(e) * y * (1.f - y);
  } else if constexpr (LOSS == CNNITMO_LOSS_MSLE) {
    const float a = logf(fmaxf(y, 1e-7f) + 1.f), b = logf(fmaxf(t, 1e-7f) + 1.f);
    l = (a - b) * (a - b);
    g = y >= 1e-7f ? 2.f * (a - b) / (y + 1.f) * y * (1.f - y) : 0.f;
  } else if constexpr (LOSS == CNNITMO_LOSS_GIVEN) {
    l = 0.f;
    g = dyv * (y * (1.f - y));
  } else {
    // binary cross-entropy on the unclipped logit (Keras clips y to [1e-7, 1-1e-7] first)
    static_assert(LOSS == CNNITMO_LOSS_BCE, "unknown loss");
    l = fmaxf(z, 0.f) - z * t + log1pf(expf(-fabsf(z)));
    g = y - t;
  }
}

template <typename T, bool BWD, int LOSS = CNNITMO_LOSS_MSE>
__global__ void head_kernel(const T* __restrict__ x, int N, int H, int Hv, int W, int cin,
                            const float* __restrict__ wt, const float* __restrict__ bias,
                            const float* __restrict__ target, float* __restrict__ yhat,
                            T* __restrict__ dx, float inv_numel, float* __restrict__ part,
                            const float* __restrict__ fs, const float* __restrict__ fh,
                            float* __restrict__ g3) {
  constexpr int VE = Vec16<T>::N;
  const int lpp = cin / VE;             // lanes per pixel (power of two <= 64)
  const int ppb = 256 / lpp;            // pixels per block iteration
  const int tid = threadIdx.x, sub = tid % lpp, slot = tid / lpp;
  const int c0 = sub * VE;
  float w[3][VE], wf[3][VE];  // raw (for dx) and BN-folded (for z) weights
  float bfold[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      w[o][e] = wt[o * cin + c0 + e];
      wf[o][e] = fs ? w[o][e] * fs[c0 + e] : w[o][e];
      if (fh) bfold[o] += w[o][e] * fh[c0 + e];
    }
#pragma unroll
  for (int o = 0; o < 3; ++o)
    for (int off = lpp >> 1; off > 0; off >>= 1) bfold[o] += __shfl_xor(bfold[o], off, 64);
  const float b0 = bias[0] + bfold[0], b1 = bias[1] + bfold[1], b2 = bias[2] + bfold[2];
  float dwacc[3][VE];
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int e = 0; e < VE; ++e) dwacc[o][e] = 0.f;
  float lsum = 0.f, corr = 0.f, db[3] = {0.f, 0.f, 0.f};
  const long P = (long)N * H * W;
  const int hw = H * W;
  const bool rowal = W % ppb == 0;
  // HEAD_U pixel slots per lane group per iteration, all their loads issued first:
  // one 16-byte load in flight per lane left this HBM pass at ~2 TB/s
  for (long base0 = (long)blockIdx.x * ppb * HEAD_U; base0 < P; base0 += (long)gridDim.x * ppb * HEAD_U) {
    float v[HEAD_U][VE], tg[HEAD_U][3], gv[HEAD_U][3];  // gv: the given dy (CNNITMO_LOSS_GIVEN; yhat holds it)
    bool inb[HEAD_U], valid[HEAD_U];
    size_t tix[HEAD_U];
#pragma unroll
    for (int u = 0; u < HEAD_U; ++u) {
      const long base = base0 + (long)u * ppb, p = base + slot;
      inb[u] = p < P;
      if (inb[u]) Pack16<T>::load(x + (size_t)p * cin + c0, v[u]);
      else
#pragma unroll
        for (int e = 0; e < VE; ++e) v[u][e] = 0.f;
      // 32-bit index math (P < 2^31, checked by the launchers); when a block's ppb pixels
      // never straddle a row (W % ppb == 0) it is wave-uniform: one scalar division
      int n, h, wc;
      if (rowal) {
        const int b = (int)base, nb = b / hw, rb = b - nb * hw, hb = rb / W;
        n = nb;
        h = hb;
        wc = rb - hb * W + slot;
      } else {
        n = inb[u] ? (int)p / hw : 0;
        const int rem = inb[u] ? (int)p - n * hw : 0;
        h = rem / W;
        wc = rem - h * W;
      }
      valid[u] = inb[u] && h < Hv;
      tix[u] = (((size_t)n * Hv + h) * W + wc) * 3;
      if (BWD) {
#pragma unroll
        for (int o = 0; o < 3; ++o) tg[u][o] = valid[u] ? target[tix[u] + o] : 0.f;
      }
#pragma unroll
      for (int o = 0; o < 3; ++o) gv[u][o] = 0.f;
      if constexpr (BWD && LOSS == CNNITMO_LOSS_GIVEN) {
#pragma unroll
        for (int o = 0; o < 3; ++o) gv[u][o] = valid[u] ? yhat[tix[u] + o] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < HEAD_U; ++u) {
      const long p = base0 + (long)u * ppb + slot;
      float z[3];
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < VE; ++e) s += v[u][e] * wf[o][e];
        for (int off = lpp >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        z[o] = s;
      }
      z[0] += b0; z[1] += b1; z[2] += b2;
      float yh[3];
#pragma unroll
      for (int o = 0; o < 3; ++o) yh[o] = 1.f / (1.f + expf(-z[o]));
      if (!BWD) {
        if (valid[u] && sub == 0) {
          yhat[tix[u] + 0] = yh[0];
          yhat[tix[u] + 1] = yh[1];
          yhat[tix[u] + 2] = yh[2];
        }
        continue;
      }
      float dz[3] = {0.f, 0.f, 0.f};
      if (valid[u]) {
        const float t0 = tg[u][0], t1 = tg[u][1], t2 = tg[u][2];
        float l0, l1, l2, g0, g1, g2;
        loss_term<LOSS>(z[0], yh[0], t0, l0, g0, gv[u][0]);
        loss_term<LOSS>(z[1], yh[1], t1, l1, g1, gv[u][1]);
        loss_term<LOSS>(z[2], yh[2], t2, l2, g2, gv[u][2]);
        if (sub == 0) {
          lsum += l0 + l1 + l2;
          const int at = (t1 > t0) ? ((t2 > t1) ? 2 : 1) : ((t2 > t0) ? 2 : 0);
          const int ap = (yh[1] > yh[0]) ? ((yh[2] > yh[1]) ? 2 : 1) : ((yh[2] > yh[0]) ? 2 : 0);
          corr += (at == ap) ? 1.f : 0.f;
        }
        dz[0] = g0 * inv_numel;
        dz[1] = g1 * inv_numel;
        dz[2] = g2 * inv_numel;
      }
      if (sub == 0) {
        db[0] += dz[0]; db[1] += dz[1]; db[2] += dz[2];
      }
#pragma unroll
      for (int e = 0; e < VE; ++e)
#pragma unroll
        for (int o = 0; o < 3; ++o) dwacc[o][e] += dz[o] * v[u][e];
      if (g3) {  // rank-3 input gradient: the consumer forms dz . w itself
        if (inb[u] && sub == 0) {
          g3[p * 3] = dz[0];
          g3[p * 3 + 1] = dz[1];
          g3[p * 3 + 2] = dz[2];
        }
      } else {
        float g[VE];
#pragma unroll
        for (int e = 0; e < VE; ++e) g[e] = dz[0] * w[0][e] + dz[1] * w[1][e] + dz[2] * w[2][e];
        if (inb[u]) Pack16<T>::store(dx + (size_t)p * cin + c0, g);
      }
    }
  }
  if (!BWD) return;
  // reduce: lanes with equal `sub` hold the same channel slice
  __shared__ float red[256][3 * 8 + 5];
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int e = 0; e < VE; ++e) red[tid][o * VE + e] = dwacc[o][e];
  red[tid][3 * VE + 0] = lsum;
  red[tid][3 * VE + 1] = corr;
  red[tid][3 * VE + 2] = db[0];
  red[tid][3 * VE + 3] = db[1];
  red[tid][3 * VE + 4] = db[2];
  __syncthreads();
  const int ncol = 5 + 3 * cin;
  float* out = part + (size_t)blockIdx.x * ncol;
  for (int k = tid; k < ncol; k += 256) {
    float s = 0.f;
    if (k < 5) {
      for (int t = 0; t < 256; t += lpp) s += red[t][3 * VE + k];
    } else {
      const int q = k - 5, o = q / cin, c = q - o * cin;
      const int sb = c / VE, e = c - sb * VE;
      for (int t = sb; t < 256; t += lpp) s += red[t][o * VE + e];
    }
    out[k] = s;
  }
}

// The same head, one wave per 64 consecutive pixels per iteration, in two layouts:
//   * channel layout (loads, dot products, dW, dx): LPP = cin/VE lanes per pixel, each
//     lane issuing LPP 16-byte loads up front (pixel u*64/LPP + lane/LPP): 1 KB per
//     instruction, LPP KB in flight per wave; the dot products reduced over the LPP
//     lanes with DPP (quad_perm xor 1/2, half-row and row mirrors: VALU, no LDS);
//   * pixel layout (sigmoid, loss, accuracy, dz, target and g3/yhat): lane = pixel,
//     the per-pixel math done once (head_kernel did it on all LPP lanes of a pixel),
//     target / g3 / yhat as 12-byte runs of consecutive lanes.
// z and dz cross between the two through a 1 KB LDS slice per wave (no barrier: one
// wave owns the slice, LDS executes a wave's instructions in order).  Bench shape
// (32 x 1088 x 1920 x 64 bf16, g3 out; tools/probe_elem.py): head_kernel 4.85 ms
// (2.1 TB/s), head2_kernel 2.35 ms (4.3 TB/s; a torch copy of x runs at 4.9 TB/s).
template <int LPP>
__device__ __forceinline__ float lane_group_sum(float v) {
  if constexpr (LPP >= 2) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  if constexpr (LPP >= 4) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
  if constexpr (LPP >= 8) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
  if constexpr (LPP >= 16) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));
  return v;
}

template <typename T>
__device__ __forceinline__ void unpack16(const uint4& q, float* v) {
  if constexpr (Vec16<T>::N == 8) {
    const bf16x8 b = __builtin_bit_cast(bf16x8, q);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)b[i];
  } else {
    v[0] = __uint_as_float(q.x); v[1] = __uint_as_float(q.y); v[2] = __uint_as_float(q.z); v[3] = __uint_as_float(q.w);
  }
}

// BWD: loss + gradients; G3: the gradient leaves as g3 [P][3] (else dx = dz . W)
template <typename T, int LPP, bool BWD, bool G3, int LOSS = CNNITMO_LOSS_MSE>
__global__ __launch_bounds__(256) void head2_kernel(const T* __restrict__ x, int H, int Hv, int W, long P,
                                                    const float* __restrict__ wt, const float* __restrict__ bias,
                                                    const float* __restrict__ target, float* __restrict__ yhat,
                                                    T* __restrict__ dx, float inv_numel, float* __restrict__ part,
                                                    const float* __restrict__ fs, const float* __restrict__ fh,
                                                    float* __restrict__ g3) {
  constexpr int VE = Vec16<T>::N, CIN = LPP * VE, PPI = 64 / LPP;  // pixels per load instruction
  __shared__ float4 zs[4][64];
  __shared__ float red[4][3 * CIN + 5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPP, c0 = sub * VE, pq = lane / LPP;
  float w[3][VE], wf[3][VE], bf[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int o = 0; o < 3; ++o) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      w[o][e] = BWD && !G3 ? wt[o * CIN + c0 + e] : 0.f;  // (dx only)
      const float wo = wt[o * CIN + c0 + e];
      wf[o][e] = fs ? wo * fs[c0 + e] : wo;
      if (fh) bf[o] += wo * fh[c0 + e];
    }
    bf[o] = lane_group_sum<LPP>(bf[o]);
  }
  const float b0 = bias[0] + bf[0], b1 = bias[1] + bf[1], b2 = bias[2] + bf[2];
  float dwacc[3][VE];
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int e = 0; e < VE; ++e) dwacc[o][e] = 0.f;
  float lsum = 0.f, corr = 0.f, db0 = 0.f, db1 = 0.f, db2 = 0.f;
  const int hw = H * W;
  const long ngroups = (P + 63) / 64, nw = (long)gridDim.x * 4;
  // a group's x (channel layout) and target (pixel layout) loads, all issued first and
  // branch-free (buffer loads, out-of-range ones read 0).  (Issuing the next group's
  // loads before this group's math measured no faster: 2.35 vs 2.35 ms at the bench
  // shape, where a torch copy of the same bytes runs at 4.9 TB/s.)
  const __amdgpu_buffer_rsrc_t tr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(BWD ? target : nullptr), (short)0, BWD ? (int)(P / hw * Hv * W * 12) : 0, 0x00020000);
  auto fetch = [&](long g, uint4 (&xq)[LPP], float (&tq)[3]) {
    const long b = g * 64;
    const long np_ = P - b < 64 ? (P - b > 0 ? P - b : 0) : 64;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(x + (b < P ? b : 0) * CIN), (short)0, (int)np_ * CIN * (int)sizeof(T), 0x00020000);
#pragma unroll
    for (int u = 0; u < LPP; ++u)
      xq[u] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                            xr, (unsigned)(((u * PPI + pq) * CIN + c0) * sizeof(T)), 0, 0));
    if constexpr (BWD) {
      const int pp = (int)b + lane;
      const bool ok = lane < np_;
      const int n = ok ? pp / hw : 0, rem = ok ? pp - n * hw : 0, h = rem / W, wc = rem - h * W;
      const unsigned off = ok && h < Hv ? (((unsigned)n * Hv + h) * W + wc) * 12u : 0x80000000u;
#pragma unroll
      for (int o = 0; o < 3; ++o) tq[o] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(tr, off + 4 * o, 0, 0));
    }
  };
  uint4 xv[LPP];
  float tv[3] = {0.f, 0.f, 0.f};
  for (long grp = (long)blockIdx.x * 4 + wave; grp < ngroups; grp += nw) {
    fetch(grp, xv, tv);
    const long base = grp * 64;
    const int np = (int)(P - base < 64 ? P - base : 64);
    // pixel layout (32-bit index math: P < 2^31, checked by the launchers)
    const int p = (int)base + lane;
    const bool inb = lane < np;
    const int n = inb ? p / hw : 0, rem = inb ? p - n * hw : 0, h = rem / W, wc = rem - h * W;
    const bool valid = inb && h < Hv;
    const size_t tix = (((size_t)n * Hv + h) * W + wc) * 3;
    const float t0 = tv[0], t1 = tv[1], t2 = tv[2];
    float gv0 = 0.f, gv1 = 0.f, gv2 = 0.f;  // the given dy (CNNITMO_LOSS_GIVEN; yhat holds it)
    if constexpr (BWD && LOSS == CNNITMO_LOSS_GIVEN) {
      if (valid) {
        gv0 = yhat[tix];
        gv1 = yhat[tix + 1];
        gv2 = yhat[tix + 2];
      }
    }
#pragma unroll
    for (int u = 0; u < LPP; ++u) {
      float v[VE];
      unpack16<T>(xv[u], v);
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        s0 += v[e] * wf[0][e];
        s1 += v[e] * wf[1][e];
        s2 += v[e] * wf[2][e];
      }
      s0 = lane_group_sum<LPP>(s0);
      s1 = lane_group_sum<LPP>(s1);
      s2 = lane_group_sum<LPP>(s2);
      if (sub == 0) zs[wave][u * PPI + pq] = make_float4(s0, s1, s2, 0.f);
    }
    __builtin_amdgcn_wave_barrier();
    const float4 z = zs[wave][lane];
    const float y0 = 1.f / (1.f + expf(-(z.x + b0)));
    const float y1 = 1.f / (1.f + expf(-(z.y + b1)));
    const float y2 = 1.f / (1.f + expf(-(z.z + b2)));
    if (!BWD) {
      if (valid) {
        yhat[tix] = y0;
        yhat[tix + 1] = y1;
        yhat[tix + 2] = y2;
      }
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (valid) {
      float l0, l1, l2, g0, g1, g2;
      loss_term<LOSS>(z.x + b0, y0, t0, l0, g0, gv0);
      loss_term<LOSS>(z.y + b1, y1, t1, l1, g1, gv1);
      loss_term<LOSS>(z.z + b2, y2, t2, l2, g2, gv2);
      lsum += l0 + l1 + l2;
      const int at = (t1 > t0) ? ((t2 > t1) ? 2 : 1) : ((t2 > t0) ? 2 : 0);
      const int ap = (y1 > y0) ? ((y2 > y1) ? 2 : 1) : ((y2 > y0) ? 2 : 0);
      corr += (at == ap) ? 1.f : 0.f;
      d0 = g0 * inv_numel;
      d1 = g1 * inv_numel;
      d2 = g2 * inv_numel;
    }
    db0 += d0;
    db1 += d1;
    db2 += d2;
    if (G3 && inb) {
      g3[(size_t)p * 3] = d0;
      g3[(size_t)p * 3 + 1] = d1;
      g3[(size_t)p * 3 + 2] = d2;
    }
    zs[wave][lane] = make_float4(d0, d1, d2, 0.f);
    __builtin_amdgcn_wave_barrier();
    // back to the channel layout: dW (and dx = dz . W without g3)
#pragma unroll
    for (int u = 0; u < LPP; ++u) {
      const float4 d = zs[wave][u * PPI + pq];
      float v[VE];
      asm volatile("" : "+v"(xv[u].x), "+v"(xv[u].y), "+v"(xv[u].z), "+v"(xv[u].w));  // unpack again: keeping all LPP*VE floats live costs occupancy
      unpack16<T>(xv[u], v);
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        dwacc[0][e] += d.x * v[e];
        dwacc[1][e] += d.y * v[e];
        dwacc[2][e] += d.z * v[e];
      }
      if (!G3 && u * PPI + pq < np) {
        float g[VE];
#pragma unroll
        for (int e = 0; e < VE; ++e) g[e] = d.x * w[0][e] + d.y * w[1][e] + d.z * w[2][e];
        Pack16<T>::store(dx + (size_t)(base + u * PPI + pq) * CIN + c0, g);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (!BWD) return;
  // reduce: dW over the lanes of equal `sub`, the scalars over the wave, then the 4 waves
#pragma unroll
  for (int o = 0; o < 3; ++o)
#pragma unroll
    for (int e = 0; e < VE; ++e)
#pragma unroll
      for (int m = LPP; m < 64; m <<= 1) dwacc[o][e] += __shfl_xor(dwacc[o][e], m, 64);
  lsum = wave_sum(lsum);
  corr = wave_sum(corr);
  db0 = wave_sum(db0);
  db1 = wave_sum(db1);
  db2 = wave_sum(db2);
  if (lane < LPP) {
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
      for (int e = 0; e < VE; ++e) red[wave][5 + o * CIN + c0 + e] = dwacc[o][e];
  }
  if (lane == 0) {
    red[wave][0] = lsum;
    red[wave][1] = corr;
    red[wave][2] = db0;
    red[wave][3] = db1;
    red[wave][4] = db2;
  }
  __syncthreads();
  float* out = part + (size_t)blockIdx.x * (5 + 3 * CIN);
  for (int k = tid; k < 5 + 3 * CIN; k += 256) out[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
}

// head2_kernel for this dtype / width, or false (head_kernel then)
template <bool BWD, int LOSS = CNNITMO_LOSS_MSE>
static bool launch_head2(int dtype, const void* x, int n, int h, int h_valid, int w, int cin, const float* wt,
                         const float* b, const float* target, float* yhat, void* dx, float inv_numel,
                         float* part, const float* scale, const float* shift, float* g3, int G_, hipStream_t s) {
  const long P = (long)n * h * w;
  const int lpp = cin / (dtype == CNNITMO_BF16 ? 8 : 4);
  // 32-bit pixel and target-byte offsets inside the kernel
  if (P >= (1L << 30) || (long)n * h_valid * w * 12 >= (1L << 31)) return false;
#define H2K(L, G)                                                                                             \
  hipLaunchKernelGGL((head2_kernel<T, L, BWD, G, LOSS>), dim3(G_), dim3(256), 0, s, (const T*)x, h, h_valid, w, P, wt, \
                     b, target, yhat, (T*)dx, inv_numel, part, scale, shift, g3)
#define H2(L)                  \
  do {                         \
    if (BWD && g3) H2K(L, BWD); \
    else H2K(L, false);        \
  } while (0)
  return by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    switch (lpp) {
      case 2: H2(2); return true;
      case 4: H2(4); return true;
      case 8: H2(8); return true;
      case 16: H2(16); return true;
      default: return false;
    }
  });
#undef H2
#undef H2K
}

// The fallback for the widths head2_kernel does not cover.
template <bool BWD, int LOSS = CNNITMO_LOSS_MSE>
static void launch_head(int dtype, const void* x, int n, int h, int h_valid, int w, int cin, const float* wt,
                        const float* b, const float* target, float* yhat, void* dx, float inv_numel, float* part,
                        const float* scale, const float* shift, float* g3, int G, hipStream_t s) {
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((head_kernel<T, BWD, LOSS>), dim3(G), dim3(256), 0, s, (const T*)x, n, h, h_valid, w, cin, wt,
                       b, target, yhat, (T*)dx, inv_numel, part, scale, shift, g3);
  });
}

extern "C" int cnnitmo_head_fwd(int dtype, const void* x, int n, int h, int h_valid, int w, int cin,
                                const float* wt, const float* b, const float* scale,
                                const float* shift, float* yhat, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int VE = dtype == CNNITMO_BF16 ? 8 : 4;
  CNN_REQUIRE(cin % VE == 0 && (cin / VE) <= 64 && ((cin / VE) & (cin / VE - 1)) == 0,
              "head: cin/%d must be a power of two <= 64", VE);
  const long P = (long)n * h * w;
  CNN_REQUIRE(P < (1L << 31), "head: too many pixels");
  const int G = cnnitmo_head_rows(P);
  if (!launch_head2<false>(dtype, x, n, h, h_valid, w, cin, wt, b, nullptr, yhat, nullptr, 0.f, nullptr, scale,
                           shift, nullptr, G, s))
    launch_head<false>(dtype, x, n, h, h_valid, w, cin, wt, b, nullptr, yhat, nullptr, 0.f, nullptr, scale, shift,
                       nullptr, G, s);
  return cnnitmo_check_launch("head_fwd");
}

template <int LOSS>
static int head_fwd_bwd_t(int dtype, const void* x, int n, int h, int h_valid, int w, int cin, const float* wt,
                          const float* b, const float* scale, const float* shift, const float* target, void* dx,
                          float* g3, float* part, double grad_numel, void* stream, const float* given = nullptr) {
  hipStream_t s = (hipStream_t)stream;
  const int VE = dtype == CNNITMO_BF16 ? 8 : 4;
  CNN_REQUIRE(cin % VE == 0 && (cin / VE) <= 64 && ((cin / VE) & (cin / VE - 1)) == 0,
              "head: cin/%d must be a power of two <= 64", VE);
  const long P = (long)n * h * w;
  CNN_REQUIRE(P < (1L << 31), "head: too many pixels");
  const int G = cnnitmo_head_rows(P);
  const double numel = grad_numel > 0.0 ? grad_numel : (double)n * h_valid * w * 3;
  const float inv_numel = LOSS == CNNITMO_LOSS_GIVEN ? 1.f : (float)(1.0 / numel);
  float* gy = const_cast<float*>(given);  // CNNITMO_LOSS_GIVEN: read through the kernels' yhat argument
  if (!launch_head2<true, LOSS>(dtype, x, n, h, h_valid, w, cin, wt, b, target, gy, dx, inv_numel, part, scale,
                                shift, g3, G, s))
    launch_head<true, LOSS>(dtype, x, n, h, h_valid, w, cin, wt, b, target, gy, dx, inv_numel, part, scale, shift,
                            g3, G, s);
  return cnnitmo_check_launch("head_fwd_bwd");
}

extern "C" int cnnitmo_head_fwd_bwd_loss(int loss, int dtype, const void* x, int n, int h, int h_valid, int w, int cin,
                                         const float* wt, const float* b, const float* scale, const float* shift,
                                         const float* target, void* dx, float* g3, float* part, double grad_numel,
                                         void* stream) {
  CNN_REQUIRE(loss >= CNNITMO_LOSS_MSE && loss <= CNNITMO_LOSS_BCE, "head_fwd_bwd_loss: unknown loss %d", loss);
  CNN_REQUIRE((dx != nullptr) != (g3 != nullptr), "head_fwd_bwd_loss: exactly one of dx and g3 must be given");
#define HEAD_LOSS(L)                                                                                              \
  case L:                                                                                                         \
    return head_fwd_bwd_t<L>(dtype, x, n, h, h_valid, w, cin, wt, b, scale, shift, target, dx, g3, part, grad_numel, \
                             stream)
  switch (loss) {
    HEAD_LOSS(CNNITMO_LOSS_MAE);
    HEAD_LOSS(CNNITMO_LOSS_LOGCOSH);
    HEAD_LOSS(CNNITMO_LOSS_MSLE);
    HEAD_LOSS(CNNITMO_LOSS_BCE);
    default: break;
  }
#undef HEAD_LOSS
  return head_fwd_bwd_t<CNNITMO_LOSS_MSE>(dtype, x, n, h, h_valid, w, cin, wt, b, scale, shift, target, dx, g3, part,
                                          grad_numel, stream);
}

extern "C" int cnnitmo_head_fwd_bwd_given(int dtype, const void* x, int n, int h, int h_valid, int w, int cin,
                                          const float* wt, const float* b, const float* scale, const float* shift,
                                          const float* target, const float* dy, void* dx, float* g3, float* part,
                                          void* stream) {
  CNN_REQUIRE(dy, "head_fwd_bwd_given: null dy");
  CNN_REQUIRE((dx != nullptr) != (g3 != nullptr), "head_fwd_bwd_given: exactly one of dx and g3 must be given");
  return head_fwd_bwd_t<CNNITMO_LOSS_GIVEN>(dtype, x, n, h, h_valid, w, cin, wt, b, scale, shift, target, dx, g3, part,
                                            0.0, stream, dy);
}

extern "C" int cnnitmo_head_fwd_bwd(int dtype, const void* x, int n, int h, int h_valid, int w,
                                    int cin, const float* wt, const float* b, const float* scale,
                                    const float* shift, const float* target, void* dx, float* part,
                                    double grad_numel, void* stream) {
  CNN_REQUIRE(dx, "head_fwd_bwd: null dx");
  return cnnitmo_head_fwd_bwd_loss(CNNITMO_LOSS_MSE, dtype, x, n, h, h_valid, w, cin, wt, b, scale, shift, target, dx,
                                   nullptr, part, grad_numel, stream);
}

extern "C" int cnnitmo_head_fwd_bwd_g3(int dtype, const void* x, int n, int h, int h_valid, int w, int cin,
                                       const float* wt, const float* b, const float* scale, const float* shift,
                                       const float* target, float* g3, float* part, double grad_numel,
                                       void* stream) {
  CNN_REQUIRE(g3, "head_fwd_bwd_g3: null g3");
  return cnnitmo_head_fwd_bwd_loss(CNNITMO_LOSS_MSE, dtype, x, n, h, h_valid, w, cin, wt, b, scale, shift, target,
                                   nullptr, g3, part, grad_numel, stream);
}

// Folded input BN (x = r, y = r*s + h): dW[o][c] = s[c]*sum(dz*r) + h[c]*db[o].
__global__ void head_final_kernel(const double* __restrict__ ws, int G, int cin, double numel,
                                  float* loss_acc, float* dw, float* db, const float* fs,
                                  const float* fh, float* raw) {
  const int ncol = 5 + 3 * cin;
  const int k = wave_col();
  if (k < ncol) {
    const double s = fold(ws, G, ncol, k);
    double dbo = 0.0;
    if (k >= 5 && fh) dbo = fold(ws, G, ncol, 2 + (k - 5) / cin);
    if ((threadIdx.x & 63) != 0) return;
    if (k == 0) loss_acc[0] = (float)(s / numel);
    else if (k == 1) loss_acc[1] = (float)(s / (numel / 3.0));
    else if (k < 5) db[k - 2] = (float)s;
    else {
      const int c = (k - 5) % cin;
      dw[k - 5] = (float)((fs ? s * fs[c] : s) + (fh ? dbo * fh[c] : 0.0));
      if (raw) raw[k - 5] = (float)s;
    }
  }
}

extern "C" int cnnitmo_head_finalize(const float* part, long rows, int cin, double numel,
                                     const float* scale, const float* shift, float* loss_acc,
                                     float* dw, float* db, float* raw_out, void* workspace,
                                     void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int G = colsum_stage1_launch(part, rows, 5 + 3 * cin, workspace, s);
  hipLaunchKernelGGL(head_final_kernel, dim3(wave_grid(5 + 3 * cin)), dim3(256), 0, s, (const double*)workspace, G, cin,
                     numel, loss_acc, dw, db, scale, shift, raw_out);
  return cnnitmo_check_launch("head_finalize");
}
