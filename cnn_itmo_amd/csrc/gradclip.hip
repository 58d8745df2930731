// Gradient clipping over the engine's flat fp32 gradient buffer (keras.optimizers clipnorm /
// clipvalue): cnnitmo_grad_sumsq / cnnitmo_grad_clip.
//
//   sumsq: out[0] = sum g[i]^2 in fp64.  (double)g * (double)g is exact (48 significant bits), so
//     only the additions round.  The order of the additions is a function of n alone:
//       * workgroup b owns the elements [b * SUM_SPAN, (b + 1) * SUM_SPAN); the grid is
//         ceil(n / SUM_SPAN) workgroups whatever the device;
//       * thread t of it adds, for it = 0 .. SUM_ITERS - 1 in turn, the four squares of the
//         elements b * SUM_SPAN + it * 4 * NT + 4 t + (0, 1, 2, 3), in that order, to one fp64
//         accumulator (elements past n add nothing);
//       * the 64 lanes of a wave are combined by an xor butterfly (offsets 32, 16, .. 1: every
//         lane ends with the same sum), the four waves through LDS in wave order by thread 0
//         (reduce.h's block_sum);
//       * the partial of workgroup b goes to ws[b]; a second launch of ONE workgroup has thread t
//         add ws[t], ws[t + NT], ... in ascending order and combines the threads the same way.
//     No atomics, no counter, nothing that depends on which workgroup finishes first: two calls
//     give the same bits, and so do an aligned and a misaligned buffer of the same values (the
//     element -> thread map is the same; only the width of the loads differs).
//   clip: g[i] <- clamp((float)((double)g[i] * f)), f from S = sumsq[0] read on the device (the
//     step never waits for the host); see cnn_itmo.h for the arithmetic.
//
// HBM-bound: 4 B per element read by sumsq, 4 B read + 4 B written by clip.  16-byte accesses when
// g is 16-byte aligned (a workgroup whose span lies inside n takes them without bounds tests, so the
// loads of an unrolled iteration are in flight together); the last workgroup tests each element; a
// buffer that is only 4-byte aligned takes dword accesses throughout.
#include <math.h>

#include "common.h"
#include "reduce.h"

namespace {

constexpr int NT = 256;
constexpr int SUM_ITERS = 8;
constexpr long SUM_SPAN = (long)NT * 4 * SUM_ITERS;  // 8192 elements per workgroup
constexpr int CLIP_ITERS = 4;
constexpr long CLIP_SPAN = (long)NT * 4 * CLIP_ITERS;  // 4096 elements per workgroup
constexpr long MAX_GRID = 0x7FFFFFFFL;

template <bool VEC>
__global__ __launch_bounds__(NT) void grad_sumsq_kernel(const float* __restrict__ g, long n,
                                                        double* __restrict__ part) {
  __shared__ double red[NT / 64][1];
  const long base = (long)blockIdx.x * SUM_SPAN + 4 * (long)threadIdx.x;
  double acc = 0.0;
  if (VEC && ((long)blockIdx.x + 1) * SUM_SPAN <= n) {
    float4 q[SUM_ITERS];
#pragma unroll
    for (int it = 0; it < SUM_ITERS; ++it) q[it] = *reinterpret_cast<const float4*>(g + base + (long)it * 4 * NT);
#pragma unroll
    for (int it = 0; it < SUM_ITERS; ++it) {
      const double x = q[it].x, y = q[it].y, z = q[it].z, w = q[it].w;
      acc += x * x;
      acc += y * y;
      acc += z * z;
      acc += w * w;
    }
  } else {
#pragma unroll
    for (int it = 0; it < SUM_ITERS; ++it) {
      const long e = base + (long)it * 4 * NT;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (VEC && e + 4 <= n) {
        const float4 q = *reinterpret_cast<const float4*>(g + e);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e + k < n) v[k] = g[e + k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // (+0 where the element is past n: the sum is unchanged)
        const double x = v[k];
        acc += x * x;
      }
    }
  }
  const double s = reduce::block_sum<1, NT>({acc}, red);  // valid in thread 0
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(NT) void grad_sumsq_final_kernel(const double* __restrict__ part, long nparts,
                                                              double* __restrict__ out) {
  __shared__ double red[NT / 64][1];
  double acc = 0.0;
  for (long i = threadIdx.x; i < nparts; i += NT) acc += part[i];
  const double s = reduce::block_sum<1, NT>({acc}, red);
  if (threadIdx.x == 0) out[0] = s;
}

struct ClipArgs {
  double grad_scale, clipnorm;
  float bound;  // (float)(clipvalue / grad_scale), 0 = no value clipping
};

__device__ __forceinline__ float clip_one(float g, double f, float bound) {
  float v = (float)((double)g * f);
  if (bound > 0.f) {  // comparisons, not fminf / fmaxf: a NaN stays a NaN
    if (v < -bound) v = -bound;
    if (v > bound) v = bound;
  }
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void grad_clip_kernel(float* __restrict__ g, long n,
                                                       const double* __restrict__ sumsq, ClipArgs a) {
  double f = 1.0;
  if (a.clipnorm > 0.0) {
    const double S = sumsq[0];
    const double N = a.grad_scale * sqrt(S);
    if (isfinite(S) && N >= a.clipnorm) f = a.clipnorm / N;
  }
  const long base = (long)blockIdx.x * CLIP_SPAN + 4 * (long)threadIdx.x;
#pragma unroll
  for (int it = 0; it < CLIP_ITERS; ++it) {
    const long e = base + (long)it * 4 * NT;
    if (VEC && e + 4 <= n) {
      float4 q = *reinterpret_cast<const float4*>(g + e);
      q.x = clip_one(q.x, f, a.bound);
      q.y = clip_one(q.y, f, a.bound);
      q.z = clip_one(q.z, f, a.bound);
      q.w = clip_one(q.w, f, a.bound);
      *reinterpret_cast<float4*>(g + e) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) g[e + k] = clip_one(g[e + k], f, a.bound);
    }
  }
}

long span_count(long n, long span) { return (n + span - 1) / span; }

}  // namespace

extern "C" long cnnitmo_grad_sumsq_workspace_bytes(long n) {
  return n <= 0 ? 0 : span_count(n, SUM_SPAN) * (long)sizeof(double);
}

extern "C" int cnnitmo_grad_sumsq(const float* g, long n, void* ws, double* out, void* stream) {
  CNN_REQUIRE(g && ws && out, "grad_sumsq: null pointer");
  CNN_REQUIRE(n > 0, "grad_sumsq: n %ld", n);
  CNN_REQUIRE(((uintptr_t)g & 3) == 0, "grad_sumsq: g is not 4-byte aligned");
  CNN_REQUIRE((((uintptr_t)ws | (uintptr_t)out) & 7) == 0, "grad_sumsq: ws and out must be 8-byte aligned");
  const long blocks = span_count(n, SUM_SPAN);
  CNN_REQUIRE(blocks <= MAX_GRID, "grad_sumsq: n %ld too large", n);
  hipStream_t s = (hipStream_t)stream;
  if (((uintptr_t)g & 15) == 0)
    hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3((unsigned)blocks), dim3(NT), 0, s, g, n, (double*)ws);
  else
    hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3((unsigned)blocks), dim3(NT), 0, s, g, n, (double*)ws);
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(NT), 0, s, (const double*)ws, blocks, out);
  return cnnitmo_check_launch("grad_sumsq");
}

extern "C" int cnnitmo_grad_clip(float* g, long n, const double* sumsq, double grad_scale, double clipnorm,
                                 double clipvalue, void* stream) {
  CNN_REQUIRE(g, "grad_clip: null pointer");
  CNN_REQUIRE(n > 0, "grad_clip: n %ld", n);
  CNN_REQUIRE(((uintptr_t)g & 3) == 0, "grad_clip: g is not 4-byte aligned");
  CNN_REQUIRE(grad_scale > 0.0 && isfinite(grad_scale), "grad_clip: grad_scale %g", grad_scale);
  CNN_REQUIRE(!isnan(clipnorm) && !isnan(clipvalue), "grad_clip: NaN clipnorm or clipvalue");
  CNN_REQUIRE(clipnorm > 0.0 || clipvalue > 0.0, "grad_clip: neither clipnorm nor clipvalue is set");
  CNN_REQUIRE(clipnorm <= 0.0 || (sumsq && ((uintptr_t)sumsq & 7) == 0),
              "grad_clip: clipnorm needs an 8-byte aligned sumsq");
  ClipArgs a;
  a.grad_scale = grad_scale;
  a.clipnorm = clipnorm > 0.0 ? clipnorm : 0.0;
  a.bound = clipvalue > 0.0 ? (float)(clipvalue / grad_scale) : 0.f;
  CNN_REQUIRE(clipvalue <= 0.0 || a.bound > 0.f, "grad_clip: clipvalue / grad_scale %g underflows fp32",
              clipvalue / grad_scale);
  const long blocks = span_count(n, CLIP_SPAN);
  CNN_REQUIRE(blocks <= MAX_GRID, "grad_clip: n %ld too large", n);
  hipStream_t s = (hipStream_t)stream;
  if (((uintptr_t)g & 15) == 0)
    hipLaunchKernelGGL(grad_clip_kernel<true>, dim3((unsigned)blocks), dim3(NT), 0, s, g, n, sumsq, a);
  else
    hipLaunchKernelGGL(grad_clip_kernel<false>, dim3((unsigned)blocks), dim3(NT), 0, s, g, n, sumsq, a);
  return cnnitmo_check_launch("grad_clip");
}
