// Device helpers of the row-partial passes: BN backward (bn.hip) and the MaxPooling2D BN sums
// (pool.hip).  Thread layout: TPP = C/VE threads per pixel row, ROWS = 256/TPP
// pixel rows per block iteration; each thread keeps VE channels of sums.  A pass over p pixels
// runs cnnitmo_bn_bwd_rows(p, c) blocks (bn.hip) and writes one partial row per block.
#pragma once
#include "common.h"

// VE argmax bytes of one channel chunk in ONE 8- (bf16) or 4-byte (fp32) load
template <int VE>
__device__ __forceinline__ void load_args(const uint8_t* p, uint8_t* arg) {
  if constexpr (VE == 8) {
    const uint2 a2 = *reinterpret_cast<const uint2*>(p);
    __builtin_memcpy(arg, &a2, 8);
  } else {
    const uint32_t a1 = *reinterpret_cast<const uint32_t*>(p);
    __builtin_memcpy(arg, &a1, 4);
  }
}

template <typename T>
__device__ __forceinline__ void load_dy(const T* dy, long dy_ld, int dy_off, long p, int C, int c0,
                                        int drop, uint64_t dbase, float* v) {
  constexpr int VE = Vec16<T>::N;
  Pack16<T>::load(dy + (size_t)p * dy_ld + dy_off + c0, v);
  if (drop) {
#pragma unroll
    for (int e = 0; e < VE; ++e)
      v[e] = dropout_keep(dbase, (uint64_t)p * C + c0 + e) ? v[e] * 2.f : 0.f;
  }
}

// Block-level reduction of per-thread [VE][NS] sums into part[blockIdx.x][NS][C].
template <int VE, int NS>
__device__ void block_reduce_rows(float (&acc)[NS][VE], int C, float* __restrict__ part) {
  __shared__ float red[256 * VE * NS];
  const int tpp = C / VE;
  const int rows = 256 / tpp;
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int e = 0; e < VE; ++e) red[(k * 256 + tid) * VE + e] = acc[k][e];
  __syncthreads();
  for (int idx = tid; idx < NS * C; idx += 256) {
    const int k = idx / C, c = idx - k * C;
    const int cv = c / VE, e = c - cv * VE;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += red[(k * 256 + r * tpp + cv) * VE + e];
    part[((size_t)blockIdx.x * NS + k) * C + c] = s;
  }
}
