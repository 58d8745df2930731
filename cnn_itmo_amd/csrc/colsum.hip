// The deterministic column reduction (conventions: colsum.h): stage 1 and the plain column sum.
#include "colsum.h"

// grid (ceil(cols/64), G); block = 64 columns x 4 row lanes; fixed-order fp64 sums.
__global__ void colsum_stage1(const float* __restrict__ part, long rows, int cols,
                              double* __restrict__ ws) {
  const int G = gridDim.y, g = blockIdx.y;
  const long per = (rows + G - 1) / G;
  const long r0 = (long)g * per, r1 = std::min(rows, r0 + per);
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s = 0.0;
  if (c < cols)
    for (long r = r0 + rl; r < r1; r += 4) s += part[(size_t)r * cols + c];
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0 && c < cols)
    ws[(size_t)g * cols + c] = ((red[cl] + red[cl + 64]) + red[cl + 128]) + red[cl + 192];
}

int colsum_stage1_launch(const float* part, long rows, int cols, void* ws, hipStream_t s) {
  const int G = red_groups(rows);
  hipLaunchKernelGGL(colsum_stage1, dim3((cols + 63) / 64, G), dim3(256), 0, s, part, rows, cols,
                     (double*)ws);
  return G;
}

extern "C" size_t cnnitmo_reduce_workspace_bytes(long rows, int cols) {
  return (size_t)red_groups(rows) * cols * sizeof(double);
}

__global__ void colsum_final(const double* __restrict__ ws, int G, int cols, int groups,
                             float* __restrict__ out) {
  const int c = wave_col();
  const int C = cols / groups;
  if (c >= C) return;
  double s = 0.0;
  for (int gr = 0; gr < groups; ++gr) s += fold(ws, G, cols, gr * C + c);
  if ((threadIdx.x & 63) == 0) out[c] = (float)s;
}

extern "C" int cnnitmo_colsum(const float* part, long rows, int cols, int groups, float* out,
                              void* workspace, void* stream) {
  CNN_REQUIRE(rows > 0 && cols > 0 && groups > 0 && cols % groups == 0, "colsum: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  const int G = colsum_stage1_launch(part, rows, cols, workspace, s);
  const int C = cols / groups;
  hipLaunchKernelGGL(colsum_final, dim3(wave_grid(C)), dim3(256), 0, s,
                     (const double*)workspace, G, cols, groups, out);
  return cnnitmo_check_launch("colsum");
}
