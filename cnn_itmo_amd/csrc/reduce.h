// Fixed-order fp64 sums of a workgroup, shared by the image-level kernels (metrics, dssim, msssim,
// tonemap, gradclip; hlweight.hip and hdrpairs.hip write the same trees out and say why).  No
// atomics and nothing that depends on which wave or workgroup runs first: the order of every
// addition is a function of K, N and nblk alone, so two runs give the same bits.  Only additions
// happen here, so the caller's fp-contract setting does not matter.  N is the workgroup's thread
// count (blockDim.x), a power of two and a multiple of 64; the caller owns the LDS array and
// decides what it sums and where the result goes.
#pragma once
#include <hip/hip_runtime.h>

namespace reduce {

// LDS tree: sh[k][t] += sh[k][t + o] for o = N/2, N/4, .. 1.  Every thread passes its K values;
// the sums are in sh[k][0], readable by every thread (the tree ends on a barrier).
template <int K, int N>
__device__ __forceinline__ void tree_sum(const double (&v)[K], double (&sh)[K][N]) {
  static_assert(N >= 2 && (N & (N - 1)) == 0, "the tree halves N down to 1");
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][tid] = v[k];
  __syncthreads();
  for (int o = N / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][tid] += sh[k][tid + o];
    }
    __syncthreads();
  }
}

// Strided fold, then the tree: thread t adds rows t, t + N, ... of part [nblk][K] in that order
// to K zeros; the sums are in sh[k][0] as above.
template <int K, int N>
__device__ __forceinline__ void fold_tree_sum(const double* __restrict__ part, long nblk, double (&sh)[K][N]) {
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  for (long i = threadIdx.x; i < nblk; i += N) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += part[i * K + k];
  }
  tree_sum<K, N>(v, sh);
}

// xor butterfly over the 64 lanes (offsets 32, 16, .. 1): every lane ends with the same sum
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Wave butterfly, then LDS across the N / 64 waves: thread k < K returns the sum of v[k], the
// waves added in index order; every other thread returns 0.
template <int K, int N>
__device__ __forceinline__ double block_sum(const double (&v)[K], double (&red)[N / 64][K]) {
  static_assert(N % 64 == 0 && K <= N, "whole waves, one thread per sum");
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = wave_sum_f64(v[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = s;
  }
  __syncthreads();
  double s = 0.0;
  if (tid < K) {
    s = red[0][tid];
#pragma unroll
    for (int i = 1; i < N / 64; ++i) s += red[i][tid];
  }
  return s;
}

}  // namespace reduce
