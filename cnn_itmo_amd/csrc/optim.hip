// The optimizers: RMSprop, Adam and SGD, each one pass over flat fp32 buffers.
#include "colsum.h"

// ----------------------------------------------------------------------------
// RMSprop (Keras 2.2 defaults; eps outside the sqrt) over one flat buffer.
// ----------------------------------------------------------------------------
__global__ void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g,
                               float* __restrict__ a, long n, float lr, float rho, float eps,
                               float gs) {
  const long n4 = n / 4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 av = reinterpret_cast<float4*>(a)[i];
    float* pp = &pv.x;
    const float* gg = &gv.x;
    float* aa = &av.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = gg[e] * gs;
      aa[e] = rho * aa[e] + (1.f - rho) * gr * gr;
      pp[e] -= lr * gr / (sqrtf(aa[e]) + eps);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(a)[i] = av;
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float gr = g[i] * gs;
    a[i] = rho * a[i] + (1.f - rho) * gr * gr;
    p[i] -= lr * gr / (sqrtf(a[i]) + eps);
  }
}

extern "C" int cnnitmo_rmsprop(float* p, const float* g, float* a, long n, float lr, float rho,
                               float eps, float grad_scale, void* stream) {
  CNN_REQUIRE(((uintptr_t)p | (uintptr_t)g | (uintptr_t)a) % 16 == 0, "rmsprop: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(rmsprop_kernel, dim3(grid_for(n / 4 + 1, 256, 2048)), dim3(256), 0,
                     (hipStream_t)stream, p, g, a, n, lr, rho, eps, grad_scale);
  return cnnitmo_check_launch("rmsprop");
}

// ----------------------------------------------------------------------------
// Adam and SGD (Keras 2.2 arithmetic, cnn_itmo.h) over the same flat buffers: one pass,
// float4 body and scalar tail like rmsprop_kernel.
// ----------------------------------------------------------------------------
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float lr_t, float b1, float b2,
                                            float eps) {
  m = b1 * m + (1.f - b1) * g;
  v = b2 * v + (1.f - b2) * g * g;
  p -= lr_t * m / (sqrtf(v) + eps);
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long n, float lr_t, float b1, float b2, float eps, float gs) {
  const long n4 = n / 4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* pp = &pv.x;
    const float* gg = &gv.x;
    float* mm = &mv.x;
    float* vq = &vv.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) adam_update(pp[e], gg[e] * gs, mm[e], vq[e], lr_t, b1, b2, eps);
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    adam_update(p[i], g[i] * gs, m[i], v[i], lr_t, b1, b2, eps);
}

extern "C" int cnnitmo_adam(float* p, const float* g, float* m, float* v, long n, float lr_t, float beta1,
                            float beta2, float eps, float grad_scale, void* stream) {
  CNN_REQUIRE(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0,
              "adam: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n / 4 + 1, 256, 2048)), dim3(256), 0, (hipStream_t)stream, p, g, m,
                     v, n, lr_t, beta1, beta2, eps, grad_scale);
  return cnnitmo_check_launch("adam");
}

template <bool NESTEROV>
__device__ __forceinline__ void sgd_update(float& p, float g, float& mom, float lr, float mu) {
  mom = mu * mom - lr * g;
  if constexpr (NESTEROV) p = p + mu * mom - lr * g;
  else p = p + mom;
}

template <bool NESTEROV>
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mom, long n,
                           float lr, float mu, float gs) {
  const long n4 = n / 4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(mom)[i];
    float* pp = &pv.x;
    const float* gg = &gv.x;
    float* mm = &mv.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) sgd_update<NESTEROV>(pp[e], gg[e] * gs, mm[e], lr, mu);
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(mom)[i] = mv;
  }
  for (long i = n4 * 4 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    sgd_update<NESTEROV>(p[i], g[i] * gs, mom[i], lr, mu);
}

extern "C" int cnnitmo_sgd(float* p, const float* g, float* mom, long n, float lr, float momentum, int nesterov,
                           float grad_scale, void* stream) {
  CNN_REQUIRE(((uintptr_t)p | (uintptr_t)g | (uintptr_t)mom) % 16 == 0, "sgd: buffers must be 16-byte aligned");
  const dim3 grid(grid_for(n / 4 + 1, 256, 2048));
  if (nesterov)
    hipLaunchKernelGGL(sgd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p, g, mom, n, lr, momentum,
                       grad_scale);
  else
    hipLaunchKernelGGL(sgd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p, g, mom, n, lr, momentum,
                       grad_scale);
  return cnnitmo_check_launch("sgd");
}
