#include <cstdio>
// Implicit-GEMM convolution on MFMA, "forward family" (K = taps x channels).
//
// One kernel template serves every GEMM of the U-Net whose reduction runs over
// (tap, channel) of an NHWC source:
//   conv3x3 fwd    (Conv2D 'same', model.py:196)      9 taps, scale 1
//   conv3x3 dgrad  (its input gradient)               9 taps on dz, flipped W
//   tconv2x2 fwd   (Conv2DTranspose s2, model.py:200) 1 tap, N = 4*cout, scatter store
//   tconv2x2 dgrad                                    4 taps, scale 2 gather
//   1-tap GEMM over im2col columns (conv2d_1, Cin=3)
//
// GEMM view: C[m][n] = sum_k A[m][k] * B[n][k]; m = output pixel (n,h,w),
// n = output channel, k = (tap, c).  A rows are gathered per tap from the
// source grid (zero outside = 'same' padding); B is the [N][K] weight matrix.
// Both operands are K-contiguous, so every global load is a 16-byte NHWC
// vector.  A K-step is 64 bytes of K per row (32 bf16 / 16 f32).  Tiles are
// staged through LDS (double buffered, one barrier per K-step) and consumed by
// v_mfma_f32_16x16x32_bf16 (bf16) or 4x v_mfma_f32_16x16x4_f32 (f32; lane
// group g owns channels 4g..4g+3 so each lane reads one 16-byte fragment per
// 4 MFMAs).  Epilogue: bias, ReLU, optional inference BN affine, BN partial
// sums (deterministic per-tile slabs), store (plain or tconv pixel-scatter).
#include "igemm_common.h"

// LDS image of a [rows][64 B] tile: 16-byte chunk c of row r stored at slot
// c ^ (((r >> 3) & 1) << 1).  With 16-row MFMA groups read by ds_read_b128
// (lane l: row l&15, chunk l>>4) every 16-lane bank group hits 16 distinct
// 16-byte slots (conflict-free); the staging ds_write_b128 stays conflict-free.
__device__ __forceinline__ int tile_off(int row, int chunk) {
  return (row << 6) + ((chunk ^ (((row >> 3) & 1) << 1)) << 4);
}

template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void igemm_fwd_kernel(const FwdArgs p) {
  constexpr int VE = Vec16<T>::N;
  constexpr int KE = 4 * VE;  // K elements per step (64 bytes)
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  constexpr int A_SEGS = BM * 4, B_SEGS = BN * 4;
  constexpr int SA = (A_SEGS + 255) / 256, SB = (B_SEGS + 255) / 256;
  constexpr int STAGE = (BM + BN) * 64;
  static_assert(WM * WN == 4, "4 waves");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lid = xcd_remap(blockIdx.x, p.mblocks * p.nblocks);
  const int mb = lid / p.nblocks, nb = lid - mb * p.nblocks;
  const long m0 = (long)mb * BM;
  const int n0 = nb * BN;
  const long K = (long)p.ntaps * p.cin;

  const T* __restrict__ A = (const T*)p.a;
  const T* __restrict__ B = (const T*)p.b;

  // Per-thread A rows (fixed over K): image index and base coordinates.
  int a_img[SA], a_h[SA], a_w[SA];
  const long hw = (long)p.ho * p.wo;
#pragma unroll
  for (int j = 0; j < SA; ++j) {
    const int seg = tid + j * 256;
    const long m = m0 + (seg >> 2);
    a_img[j] = -1;
    a_h[j] = 0;
    a_w[j] = 0;
    if (seg < A_SEGS && m < p.M) {
      const int img = (int)(m / hw);
      const int rem = (int)(m - (long)img * hw);
      const int oh = rem / p.wo;
      a_img[j] = img;
      a_h[j] = oh * p.scale;
      a_w[j] = (rem - oh * p.wo) * p.scale;
    }
  }
  const int chunk = tid & 3;

  uint4 ra[SA], rb[SB];
  const int steps_per_tap = p.cin / KE;
  const int nk = p.ntaps * steps_per_tap;

  auto load = [&](int tap, int c0) {
    const int ddy = ((p.dyc >> (2 * tap)) & 3) - 1, ddx = ((p.dxc >> (2 * tap)) & 3) - 1;
#pragma unroll
    for (int j = 0; j < SA; ++j) {
      const int hh = a_h[j] + ddy, ww = a_w[j] + ddx;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (a_img[j] >= 0 && hh >= 0 && hh < p.hs && ww >= 0 && ww < p.ws) {
        const size_t off = ((size_t)((long)a_img[j] * p.hs + hh) * p.ws + ww) * p.a_ld + p.a_off +
                           c0 + chunk * VE;
        v = *reinterpret_cast<const uint4*>(A + off);
      }
      ra[j] = v;
    }
#pragma unroll
    for (int j = 0; j < SB; ++j) {
      const int seg = tid + j * 256;
      if (seg < B_SEGS) {
        const size_t off = (size_t)(n0 + (seg >> 2)) * K + (long)tap * p.cin + c0 + chunk * VE;
        rb[j] = *reinterpret_cast<const uint4*>(B + off);
      }
    }
  };
  auto store = [&](int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + BM * 64;
#pragma unroll
    for (int j = 0; j < SA; ++j) {
      const int seg = tid + j * 256;
      if (seg < A_SEGS) *reinterpret_cast<uint4*>(As + tile_off(seg >> 2, chunk)) = ra[j];
    }
#pragma unroll
    for (int j = 0; j < SB; ++j) {
      const int seg = tid + j * 256;
      if (seg < B_SEGS) *reinterpret_cast<uint4*>(Bs + tile_off(seg >> 2, chunk)) = rb[j];
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int tap = 0, c0 = 0;
  load(0, 0);
  store(0);
  __syncthreads();
  int cur = 0;
  for (int ks = 0; ks < nk; ++ks) {
    const bool more = ks + 1 < nk;
    if (more) {
      c0 += KE;
      if (c0 == p.cin) { c0 = 0; ++tap; }
      load(tap, c0);
    }
    const char* As = smem + cur * STAGE;
    const char* Bs = As + BM * 64;
    uint4 af[FM], bfr[FN];
    const int frow = lane & 15, fch = lane >> 4;
#pragma unroll
    for (int i = 0; i < FM; ++i)
      af[i] = *reinterpret_cast<const uint4*>(As + tile_off(wm * TM + i * 16 + frow, fch));
#pragma unroll
    for (int j = 0; j < FN; ++j)
      bfr[j] = *reinterpret_cast<const uint4*>(Bs + tile_off(wn * TN + j * 16 + frow, fch));
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) Mma<T>::run(acc[i][j], af[i], bfr[j]);
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // ---------------- epilogue ----------------
  const bool relu = p.flags & CNNITMO_RELU, aff = p.flags & CNNITMO_AFFINE,
             stats = p.flags & CNNITMO_STATS;
  T* __restrict__ O = (T*)p.out;
  float bj[FN], sj[FN], hj[FN];
  int coj[FN], tapoff[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int n = n0 + wn * TN + j * 16 + (lane & 15);
    int co = n, tp = 0;
    if (p.scatter) {
      tp = n / p.cout;
      co = n - tp * p.cout;
    }
    coj[j] = co;
    tapoff[j] = (tp >> 1) * 2 * p.wo + (tp & 1);
    bj[j] = p.bias ? p.bias[(p.flags & CNNITMO_BIAS_PER_COL) ? n : co] : 0.f;
    sj[j] = aff ? p.aff_scale[co] : 1.f;
    hj[j] = aff ? p.aff_shift[co] : 0.f;
  }
  float s1[FN], s2[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) s1[j] = s2[j] = 0.f;

#pragma unroll
  for (int i = 0; i < FM; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long m = m0 + wm * TM + i * 16 + (lane >> 4) * 4 + r;
      if (m >= p.M) continue;
      int boh = 1, bow = 1;
      if (p.border) {
        const int rem = (int)(m % hw);
        boh = rem / p.wo;
        bow = rem - boh * p.wo;
      }
      long pixbase;
      if (p.scatter) {
        const int img = (int)(m / hw);
        const int rem = (int)(m - (long)img * hw);
        const int ii = rem / p.wo, jj = rem - ii * p.wo;
        pixbase = ((long)img * 2 * p.ho + 2 * ii) * 2 * p.wo + 2 * jj;
      } else {
        pixbase = m;
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        float v = acc[i][j][r] + bj[j];
        if (p.border) v -= border_corr(p.border + (size_t)coj[j] * 8, boh, bow, p.ho, p.wo);
        if (relu) v = fmaxf(v, 0.f);
        if (aff) v = v * sj[j] + hj[j];
        s1[j] += v;
        s2[j] += v * v;
        const size_t off = (size_t)(pixbase + (p.scatter ? tapoff[j] : 0)) * p.out_ld + p.out_off + coj[j];
        O[off] = from_f32<T>(v);
      }
    }
  }

  if (stats) {
    // rows beyond M contributed nothing (skipped above)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      s1[j] += __shfl_xor(s1[j], 16, 64);
      s1[j] += __shfl_xor(s1[j], 32, 64);
      s2[j] += __shfl_xor(s2[j], 16, 64);
      s2[j] += __shfl_xor(s2[j], 32, 64);
    }
    float* red = reinterpret_cast<float*>(smem);  // [WM][BN][2]; main loop ended with a barrier
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int col = wn * TN + j * 16 + lane;
        red[(wm * BN + col) * 2 + 0] = s1[j];
        red[(wm * BN + col) * 2 + 1] = s2[j];
      }
    }
    __syncthreads();
    if (tid < BN) {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int w = 0; w < WM; ++w) {
        t1 += red[(w * BN + tid) * 2 + 0];
        t2 += red[(w * BN + tid) * 2 + 1];
      }
      float* st = p.stats + (size_t)mb * 2 * p.N;
      st[n0 + tid] = t1;
      st[p.N + n0 + tid] = t2;
    }
  }
}

// ----------------------------------------------------------------------------
// Host side: this kernel's launch, sizes, rows and name (the routing between kernels is
// conv_dispatch.hip)
// ----------------------------------------------------------------------------
namespace {

struct Cfg {
  int bm, bn;
};
Cfg pick_cfg(int N) {
  if (N >= 128 && N % 128 == 0) return {128, 128};
  if (N % 64 == 0) return {256, 64};
  return {256, 32};
}

}  // namespace

// The sizes launch_fwd takes from dense views (its CNN_REQUIREs below; ve = Vec16<T>::N): the
// queries give a shape that fails them no rows and no kernel name.
bool fwd_sizes_ok(const FwdArgs& a, int ve) {
  return a.M > 0 && a.N > 0 && a.N % 32 == 0 && a.cin > 0 && a.cin % (4 * ve) == 0 && a.a_ld % ve == 0;
}

template <typename T>
int launch_fwd(FwdArgs a, hipStream_t s, const char* what) {
  CNN_REQUIRE(a.N % 32 == 0, "%s: output columns %d not a multiple of 32", what, a.N);
  CNN_REQUIRE(a.cin % (4 * Vec16<T>::N) == 0, "%s: channels per tap %d not a multiple of %d", what,
              a.cin, 4 * Vec16<T>::N);
  CNN_REQUIRE(a.a_ld % Vec16<T>::N == 0 && a.a_off % Vec16<T>::N == 0,
              "%s: source view ld/off must be multiples of %d", what, Vec16<T>::N);
  CNN_REQUIRE(a.M > 0 && a.ntaps >= 1 && a.ntaps <= 9, "%s: bad sizes", what);
  Cfg c = pick_cfg(a.N);
  a.mblocks = (int)((a.M + c.bm - 1) / c.bm);
  a.nblocks = a.N / c.bn;
  const long total = (long)a.mblocks * a.nblocks;
  CNN_REQUIRE(total < (1L << 31), "%s: grid too large", what);
  dim3 grid((unsigned)total), block(256);
  if (c.bm == 128)
    hipLaunchKernelGGL((igemm_fwd_kernel<T, 128, 128, 2, 2>), grid, block, 0, s, a);
  else if (c.bn == 64)
    hipLaunchKernelGGL((igemm_fwd_kernel<T, 256, 64, 4, 1>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((igemm_fwd_kernel<T, 256, 32, 4, 1>), grid, block, 0, s, a);
  return cnnitmo_check_launch(what);
}

template int launch_fwd<bf16>(FwdArgs, hipStream_t, const char*);
template int launch_fwd<float>(FwdArgs, hipStream_t, const char*);

// BN partial-sum rows: one per row tile.
int fwd_stat_rows(long m, int N) {
  const Cfg c = pick_cfg(N);
  return (int)((m + c.bm - 1) / c.bm);
}

const char* fwd_name(int N, bool bf16) {
  const Cfg c = pick_cfg(N);
  static thread_local char buf[96];
  snprintf(buf, sizeof(buf), "igemm_fwd_kernel<%s,%dx%d>", bf16 ? "bf16" : "f32", c.bm, c.bn);
  return buf;
}
