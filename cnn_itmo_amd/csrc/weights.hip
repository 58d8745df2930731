// Weight preparation (fp32 master -> the layouts the conv kernels read), BN folding into a
// consumer's weights, and the first-layer im2col.
#include "colsum.h"

// ----------------------------------------------------------------------------
// Weight preparation: fp32 master -> dtype copies in the layouts kernels read.
// ----------------------------------------------------------------------------
template <typename T>
__global__ void prep_conv_kernel(const float* __restrict__ w, int cout, int cin, T* __restrict__ wf,
                                 T* __restrict__ wflip) {
  const long total = (long)cout * 9 * cin;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % cin);
    const long t = i / cin;
    const int rs = (int)(t % 9), co = (int)(t / 9);
    const T v = from_f32<T>(w[i]);
    wf[i] = v;
    if (wflip) {  // wflip[ci][2-r][2-s][co] = w[co][r][s][ci]
      const int r = rs / 3, s = rs % 3;
      wflip[((long)ci * 9 + (2 - r) * 3 + (2 - s)) * cout + co] = v;
    }
  }
}

template <typename T>
__global__ void prep_tconv_kernel(const float* __restrict__ k, int cout, int cin, T* __restrict__ kf,
                                  T* __restrict__ kT) {
  const long total = 4L * cout * cin;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % cin);
    const long t = i / cin;
    const int co = (int)(t % cout), tap = (int)(t / cout);
    const T v = from_f32<T>(k[i]);
    kf[i] = v;
    kT[((long)ci * 4 + tap) * cout + co] = v;  // kT[ci][a][b][co]
  }
}

template <typename T>
__global__ void prep_c3_kernel(const float* __restrict__ w, int cout, T* __restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cout * 32) return;
  const int co = i / 32, k = i % 32;
  wp[i] = from_f32<T>(k < 27 ? w[co * 27 + k] : 0.f);
}

extern "C" int cnnitmo_prep_conv3x3_weights(int dtype, const float* w, int cout, int cin,
                                            void* w_fwd, void* w_flip, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)cout * 9 * cin;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(prep_conv_kernel<T>, dim3(grid_for(n)), dim3(256), 0, s, w, cout, cin, (T*)w_fwd,
                       (T*)w_flip);
  });
  return cnnitmo_check_launch("prep_conv3x3_weights");
}

extern "C" int cnnitmo_prep_tconv2x2_weights(int dtype, const float* k, int cout, int cin,
                                             void* k_fwd, void* kT, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const long n = 4L * cout * cin;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(prep_tconv_kernel<T>, dim3(grid_for(n)), dim3(256), 0, s, k, cout, cin, (T*)k_fwd, (T*)kT);
  });
  return cnnitmo_check_launch("prep_tconv2x2_weights");
}

extern "C" int cnnitmo_prep_c3_weights(int dtype, const float* w, int cout, void* w_packed,
                                       void* stream) {
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(prep_c3_kernel<T>, dim3((cout * 32 + 255) / 256), dim3(256), 0, s, w, cout, (T*)w_packed);
  });
  return cnnitmo_check_launch("prep_c3_weights");
}

// ----------------------------------------------------------------------------
// First-layer packing: x [n][h_valid][w][3] fp32 -> cols [n][h][w][32] dtype.
// ----------------------------------------------------------------------------
// One workgroup per 256-pixel segment of an output row: the three input rows it
// reads ((256+2) pixels x 3 channels each, fp32) are staged in LDS once (coalesced,
// zero outside the image / below h_valid), every thread assembles its pixel's 27
// (+5 zero) values, and the 256 x 32 tile leaves through LDS as lane-linear 16-byte
// stores (4.3 GB of bf16 columns per 1080p b32 step: a pure write stream).
template <typename T>
__global__ __launch_bounds__(256) void im2col_c3_kernel(const float* __restrict__ x, int Hv, int H, int W,
                                                        int segs, T* __restrict__ cols) {
  constexpr int SEG = 256, PW = SEG + 2;
  constexpr int VE = Vec16<T>::N;
  __shared__ float xs[3][PW * 3];
  __shared__ __attribute__((aligned(16))) T tile[SEG * 32];
  const int seg = blockIdx.x % segs;
  const long row = blockIdx.x / segs;  // n * H + h
  const int h = (int)(row % H);
  const long n = row / H;
  const int w0 = seg * SEG;
  for (int i = threadIdx.x; i < 3 * PW * 3; i += SEG) {
    const int r = i / (PW * 3), q = i - r * (PW * 3);
    const int ww = w0 - 1 + q / 3, hh = h + r - 1;
    float v = 0.f;
    if (hh >= 0 && hh < Hv && ww >= 0 && ww < W) v = x[((n * Hv + hh) * W + ww) * 3 + q % 3];
    xs[r][q] = v;
  }
  __syncthreads();
  const int t = threadIdx.x;
  float v[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const int tap = k / 3, c = k - tap * 3;
    v[k] = k < 27 ? xs[tap / 3][(t + tap % 3) * 3 + c] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < 32; j += VE) Pack16<T>::store(tile + t * 32 + j, v + j);
  __syncthreads();
  const int npx = min(SEG, W - w0);
  const uint4* src = reinterpret_cast<const uint4*>(tile);
  uint4* dst = reinterpret_cast<uint4*>(cols + ((size_t)row * W + w0) * 32);
  const int nv = npx * 32 / VE;
  for (int i = t; i < nv; i += SEG) dst[i] = src[i];
}

extern "C" int cnnitmo_im2col_c3(int dtype, const float* x, int n, int h_valid, int h, int w,
                                 void* cols, void* stream) {
  CNN_REQUIRE(h_valid <= h, "im2col_c3: h_valid > h");
  CNN_REQUIRE(n > 0 && h > 0 && w > 0, "im2col_c3: bad shape");
  hipStream_t s = (hipStream_t)stream;
  const int segs = (w + 255) / 256;
  const long blocks = (long)n * h * segs;
  CNN_REQUIRE(blocks < (1L << 31), "im2col_c3: too large");
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(im2col_c3_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, x, h_valid, h, w, segs,
                       (T*)cols);
  });
  return cnnitmo_check_launch("im2col_c3");
}

// ----------------------------------------------------------------------------
// BN folding (training): a consumer of a BN output y = r*s + h (per input
// channel) reads the stored r and folds the affine instead of materialising y.
//   conv3x3: W' = W*s, bias' = b + sum_t u_t, u_t[co] = sum_ci W[co][t][ci] h[ci];
//            zero padding applies to y, so the conv epilogue subtracts u_t for every
//            out-of-bounds tap t of a border pixel via the table
//            border[co] = {Utop, Ubot, Uleft, Uright, u0, u2, u6, u8}.
//   tconv:   K' = K*s, bias'[tap][co] = b[co] + sum_ci K[tap][co][ci] h[ci] (no padding).
// ----------------------------------------------------------------------------
__device__ float block_sum_det(float v, float* red) {
  // deterministic 256-thread tree sum; every thread returns the total
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const float s = red[0];
  __syncthreads();
  return s;
}

template <typename T>
__global__ void fold_conv_kernel(const float* __restrict__ w, const float* __restrict__ b,
                                 const float* __restrict__ s, const float* __restrict__ h, int cout,
                                 int cin, int ntaps, T* __restrict__ wout, float* __restrict__ bout,
                                 float* __restrict__ border) {
  __shared__ float red[256];
  const int co = blockIdx.x;
  float u[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {  // ntaps == 9
    float acc = 0.f;
    for (int ci = threadIdx.x; ci < cin; ci += blockDim.x) {
      const size_t i = ((size_t)co * ntaps + t) * cin + ci;
      const float wv = w[i];
      wout[i] = from_f32<T>(s ? wv * s[ci] : wv);
      if (h) acc += wv * h[ci];
    }
    u[t] = block_sum_det(acc, red);
  }
  if (threadIdx.x == 0) {
    float bsum = b ? b[co] : 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) bsum += u[t];
    bout[co] = bsum;
    if (border && ntaps == 9) {
      float* U = border + (size_t)co * 8;
      U[0] = u[0] + u[1] + u[2];
      U[1] = u[6] + u[7] + u[8];
      U[2] = u[0] + u[3] + u[6];
      U[3] = u[2] + u[5] + u[8];
      U[4] = u[0];
      U[5] = u[2];
      U[6] = u[6];
      U[7] = u[8];
    }
  }
}

extern "C" int cnnitmo_fold_conv3x3(int dtype, const float* w, const float* bias, const float* scale,
                                    const float* shift, int cout, int cin, void* w_out,
                                    float* bias_out, float* border, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(fold_conv_kernel<T>, dim3(cout), dim3(256), 0, s, w, bias, scale, shift, cout, cin, 9,
                       (T*)w_out, bias_out, border);
  });
  return cnnitmo_check_launch("fold_conv3x3");
}

// tconv: k [4][cout][cin] viewed as [4*cout rows][cin]: one block per (tap, co)
template <typename T>
__global__ void fold_tconv_kernel(const float* __restrict__ k, const float* __restrict__ b,
                                  const float* __restrict__ s, const float* __restrict__ h, int cout,
                                  int cin, T* __restrict__ kout, float* __restrict__ bout) {
  __shared__ float red[256];
  const int row = blockIdx.x, co = row % cout;
  float acc = 0.f;
  for (int ci = threadIdx.x; ci < cin; ci += blockDim.x) {
    const size_t i = (size_t)row * cin + ci;
    const float kv = k[i];
    kout[i] = from_f32<T>(s ? kv * s[ci] : kv);
    if (h) acc += kv * h[ci];
  }
  const float tot = block_sum_det(acc, red);
  if (threadIdx.x == 0) bout[row] = (b ? b[co] : 0.f) + tot;
}

extern "C" int cnnitmo_fold_tconv2x2(int dtype, const float* k, const float* bias, const float* scale,
                                     const float* shift, int cout, int cin, void* k_out,
                                     float* bias_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(fold_tconv_kernel<T>, dim3(4 * cout), dim3(256), 0, s, k, bias, scale, shift, cout, cin,
                       (T*)k_out, bias_out);
  });
  return cnnitmo_check_launch("fold_tconv2x2");
}
