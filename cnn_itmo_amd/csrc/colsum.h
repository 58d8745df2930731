// HBM-bound kernels of the U-Net step: BatchNormalization (train/infer, fwd/bwd) with the
// ReLU gradient and Dropout (bn.hip), MaxPooling2D fwd/bwd (pool.hip), the sigmoid head with
// its loss and 'accuracy' (head.hip), RMSprop and the other optimizers (optim.hip), weight
// preparation and first-layer packing (weights.hip) and the deterministic column reductions
// (colsum.hip).  All accesses are 16-byte NHWC vectors; every reduction writes per-block
// partial rows that a fixed-order fp64 pass folds, so results are bitwise reproducible run to
// run.  This header holds that pass's device side (fold, one wave per output column) and the
// launch arithmetic around it.  (reduce.h is something else: the image kernels' namespace
// reduce.)
#pragma once
#include <algorithm>

#include "common.h"

static inline int grid_for(long work, int per_block = 256, int cap = 8192) {
  long b = (work + per_block - 1) / per_block;
  return (int)std::max(1L, std::min<long>(b, cap));
}

// ----------------------------------------------------------------------------
// Column reduction: part [rows][cols] fp32 -> ws [G][cols] fp64 (stage 1).
// ----------------------------------------------------------------------------
static constexpr int RED_GMAX = 1024;  // stage-1 row groups (max)
static inline int red_groups(long rows) { return (int)std::max(1L, std::min<long>(RED_GMAX, rows / 16)); }

// Launches colsum_stage1 (colsum.hip) into ws and returns its G, the rows that fold reads.
int colsum_stage1_launch(const float* part, long rows, int cols, void* ws, hipStream_t s);

// Fold the G stage-1 rows of one column with a whole wave (fixed-order tree:
// deterministic).  Every lane returns the total.  Finalize kernels run one
// 64-lane wave per output column (256-thread blocks = 4 columns).
__device__ __forceinline__ double fold(const double* ws, int G, int cols, int col) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int g = lane; g < G; g += 64) s += ws[(size_t)g * cols + col];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}
__device__ __forceinline__ int wave_col() { return blockIdx.x * 4 + (threadIdx.x >> 6); }
static inline int wave_grid(int ncols) { return (ncols + 3) / 4; }
