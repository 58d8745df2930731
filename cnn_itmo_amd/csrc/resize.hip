// Antialiased separable image resampling with Pillow's arithmetic: cnnitmo_resize_coeffs (host),
// cnnitmo_resize (device).
//
// The arithmetic is Pillow's Resample.c (box, bilinear, bicubic, lanczos), stated step by step in
// include/cnn_itmo.h and restated in numpy in tests/resize_ref.py; the three agree bit for bit
// (uint8: byte for byte).  Coefficients are C doubles made on the host by cnnitmo_resize_coeffs and
// uploaded by the caller; a pass accumulates `ss += (double)pixel * k[x]` in tap order (fp32) or
// `ss += pixel * ki[x]` in int32 (uint8), with no FMA contraction anywhere in this file, no atomics
// and one fixed order per output value: two runs give the same bits.
//
// One launch per pass, the horizontal pass first, its result stored in the picture's type:
//   resize_h  a workgroup (512 threads) takes TILE output columns x 64 rows.  The source span of the tile,
//             xmin(first) .. xmin(last) + n(last), is contiguous in every row: it is staged in LDS
//             as [64][pitch] dwords, interleaved RGB as in memory, pitch odd.  Staging: consecutive
//             lanes load and store consecutive dwords (coalesced, conflict-free).  Accumulating: a
//             lane is a ROW of the strip, a wave walks the (column, channel) items of the tile, so
//             the bounds and the coefficient row are uniform over the wave (scalar loads), and the
//             64 lanes read LDS addresses an odd pitch apart: 32 distinct banks per half wave.
//             Results go to a second LDS tile [64][3 TILE | 1] and leave as row segments of
//             consecutive dwords (bytes for uint8).  TILE comes from the scale on the host
//             (cnnitmo_resize_tile_cols): the largest tile whose span fits the LDS budget.
//             A span no tile of one column fits (a lanczos reduction beyond about 13x), or a
//             table whose span is wider than the host's bound, takes the direct path: a thread per
//             output value, reading global memory and its own coefficient row.
//   resize_v  consecutive lanes take consecutive values of an output row (3 w contiguous values),
//             each lane walks its n source rows; the output row, hence bounds and coefficients,
//             are uniform over the workgroup and come through scalar loads.
//   resize_copy  equal sizes on both axes: a copy (with the floor).
// The tables are device memory the caller filled; every index taken from them is clamped to the
// picture before use, so a bad table gives wrong pixels, never an access outside x / out.
#include "common.h"

#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int TB = 256;     // threads per workgroup of the vertical pass and the copy
constexpr int TBH = 512;    // of the horizontal pass: eight waves share a strip, four per SIMD at two workgroups per CU
constexpr int ROWS = 64;    // rows per horizontal strip: one per lane
constexpr int WAVES = TBH / 64;
constexpr int MAX_TILE = 64;            // output columns per horizontal tile, at most
constexpr int DIRECT_TILE = 32;         // the direct path's tile
constexpr int LDS_BUDGET = 64 * 1024;   // bytes per workgroup: two workgroups per CU (160 KiB)

constexpr double SUPPORT[4] = {0.5, 1.0, 2.0, 3.0};

// ---- Pillow's filters, in double ------------------------------------------------------------
inline double sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
inline double filter_value(int f, double x) {
  switch (f) {
    case CNNITMO_RESIZE_BOX:
      return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    case CNNITMO_RESIZE_BILINEAR:
      if (x < 0.0) x = -x;
      return x < 1.0 ? 1.0 - x : 0.0;
    case CNNITMO_RESIZE_BICUBIC: {
      const double a = -0.5;
      if (x < 0.0) x = -x;
      if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
      if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
      return 0.0;
    }
    default:
      return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0;
  }
}
inline int ksize_of(int in, int out, double support) {
  double fs = (double)in / out;
  if (fs < 1.0) fs = 1.0;
  return (int)ceil(support * fs) * 2 + 1;
}
inline bool ksize_ok(int in, int out, int ksize) {
  for (double s : SUPPORT)
    if (ksize == ksize_of(in, out, s)) return true;
  return false;
}

// Largest tile whose source span fits the LDS budget; 0 = none does.  span(tile) is bounded by
// (tile - 1) scale + 2 sup + 1 with sup <= (ksize - 1) / 2 (header: xmin > c - sup - 0.5,
// xmax <= c + sup + 0.5); the tile depends on the scale and ksize alone.
struct HPlan {
  int tile, cap_px, pitch_in, pitch_out;
  size_t lds;
};
HPlan plan_h(int w, int ow, int ksize) {
  const double scale = (double)w / ow;
  const int hs = (ksize - 1) / 2;
  for (int tile = MAX_TILE; tile >= 1; --tile) {
    HPlan p;
    p.tile = tile;
    const double cap = ceil((tile - 1) * scale) + 2.0 * hs + 1.0;
    if (cap > 65536.0) continue;
    p.cap_px = (int)cap;
    p.pitch_in = (3 * p.cap_px) | 1;
    p.pitch_out = (3 * tile) | 1;
    p.lds = (size_t)ROWS * ((size_t)p.pitch_in + p.pitch_out) * 4;
    if (p.lds <= (size_t)LDS_BUDGET) return p;
  }
  return HPlan{0, -1, 0, 0, 0};
}

// ---- per-type arithmetic ----------------------------------------------------------------------
template <typename T> struct Px;
template <> struct Px<float> {
  typedef float lds_t;   // a staged value
  typedef double acc_t;
  static __device__ __forceinline__ acc_t init() { return 0.0; }
  static __device__ __forceinline__ acc_t tap(acc_t a, float v, double k) { return a + (double)v * k; }
  static __device__ __forceinline__ lds_t finish(acc_t a, float lo) {
    const float v = (float)a;
    return v < lo ? lo : v;
  }
};
template <> struct Px<uint8_t> {
  typedef int lds_t;
  typedef int acc_t;
  static __device__ __forceinline__ acc_t init() { return 1 << 21; }
  static __device__ __forceinline__ acc_t tap(acc_t a, int v, double k) {
    const double s = k * 4194304.0;  // exact
    const int ki = k < 0 ? (int)(s - 0.5) : (int)(s + 0.5);
    return a + v * ki;
  }
  static __device__ __forceinline__ lds_t finish(acc_t a, float) {
    const int v = a >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
  }
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The taps of one output value, in tap order: p[t * stride] * k[t], t < nn.  Eight taps at a time: their
// coefficients (one scalar load when k is uniform) and their pixels are all requested before the first
// is used, so a wave waits for memory once per eight taps; the sum is still one chain in tap order.
// Taps beyond nn are never touched: a zero coefficient times an infinite pixel would be a NaN.
template <typename T, typename V>
__device__ __forceinline__ typename Px<T>::acc_t accumulate(const V* p, size_t stride, const double* k, int nn) {
  typename Px<T>::acc_t a = Px<T>::init();
  int t = 0;
  for (; t + 8 <= nn; t += 8) {
    double kv[8];
    V v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) kv[j] = k[t + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(t + j) * stride];
#pragma unroll
    for (int j = 0; j < 8; ++j) a = Px<T>::tap(a, v[j], kv[j]);
  }
  for (; t < nn; ++t) a = Px<T>::tap(a, p[(size_t)t * stride], k[t]);
  return a;
}

// ---- horizontal pass -------------------------------------------------------------------------
// x [rows][w][3] -> out [rows][ow][3].  cap_px < 0: every workgroup takes the direct path (no LDS).
template <typename T>
__global__ __launch_bounds__(TBH) void resize_h(const T* __restrict__ x, T* __restrict__ out,
                                               const int* __restrict__ bounds, const double* __restrict__ kk,
                                               int ksize, long rows, int w, int ow, int tile, int cap_px,
                                               int pitch_in, int pitch_out, float lo) {
  typedef typename Px<T>::lds_t S;
  typedef typename Px<T>::acc_t A;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tiles = (ow + tile - 1) / tile;
  const int bt = (int)(blockIdx.x % (unsigned)tiles);
  const long row0 = (long)(blockIdx.x / (unsigned)tiles) * ROWS;
  const int ox0 = bt * tile;
  const int tw = min(tile, ow - ox0);
  const int nr = (int)min((long)ROWS, rows - row0);
  // the tile's source span, inside the row whatever the table says
  const int x0 = clampi(bounds[2 * ox0], 0, w);
  const int xl = clampi(bounds[2 * (ox0 + tw - 1)], x0, w);
  const int x1 = xl + clampi(bounds[2 * (ox0 + tw - 1) + 1], 0, min(ksize, w - xl));
  const int span = x1 - x0;

  if (span > cap_px) {  // direct: one output value per thread and step, no LDS (uniform over the workgroup)
    const int items = 3 * tw;
    for (int idx = threadIdx.x; idx < nr * items; idx += TBH) {
      const int r = idx / items, it = idx - r * items;
      const int ox = ox0 + it / 3, c = it % 3;
      const int xm = clampi(bounds[2 * ox], 0, w);
      const int nn = clampi(bounds[2 * ox + 1], 0, min(ksize, w - xm));
      const double* k = kk + (size_t)ox * ksize;
      const T* p = x + ((size_t)(row0 + r) * w + xm) * 3 + c;
      out[((size_t)(row0 + r) * ow + ox) * 3 + c] = (T)Px<T>::finish(accumulate<T>(p, 3, k, nn), lo);
    }
    return;
  }

  S* sin = reinterpret_cast<S*>(smem);
  S* sout = sin + (size_t)ROWS * pitch_in;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int len = 3 * span;
  // a wave stages rows wv, wv + WAVES, ...: per 64-dword chunk its loads are in flight together
  const T* src = x + ((size_t)row0 * w + x0) * 3;
  for (int e = lane; e < len; e += 64) {
    S v[ROWS / WAVES];
#pragma unroll
    for (int j = 0; j < ROWS / WAVES; ++j) {
      const int r = wv + WAVES * j;
      v[j] = r < nr ? (S)src[(size_t)r * w * 3 + e] : (S)0;
    }
#pragma unroll
    for (int j = 0; j < ROWS / WAVES; ++j) {
      const int r = wv + WAVES * j;
      if (r < nr) sin[r * pitch_in + e] = v[j];
    }
  }
  __syncthreads();
  for (int it = wv; it < 3 * tw; it += WAVES) {  // (column, channel) items: uniform over the wave
    const int ox = ox0 + it / 3, c = it % 3;
    const int xm = clampi(bounds[2 * ox], x0, x1);
    const int nn = clampi(bounds[2 * ox + 1], 0, min(ksize, x1 - xm));
    const double* k = kk + (size_t)ox * ksize;
    // lanes past the strip's last row sum LDS words nobody staged and drop the result
    const A a = accumulate<T>(sin + lane * pitch_in + 3 * (xm - x0) + c, 3, k, nn);
    if (lane < nr) sout[lane * pitch_out + it] = Px<T>::finish(a, lo);
  }
  __syncthreads();
  const int olen = 3 * tw;
  T* dst = out + ((size_t)row0 * ow + ox0) * 3;
  for (int e = lane; e < olen; e += 64) {
#pragma unroll
    for (int j = 0; j < ROWS / WAVES; ++j) {
      const int r = wv + WAVES * j;
      if (r < nr) dst[(size_t)r * ow * 3 + e] = (T)sout[r * pitch_out + e];
    }
  }
}

// ---- vertical pass ---------------------------------------------------------------------------
// x [n][h][rowlen] -> out [n][oh][rowlen], rowlen = 3 * width.  A workgroup: TB consecutive values
// of one output row; blockIdx = (image * oh + oy) * chunks + chunk.
template <typename T>
__global__ __launch_bounds__(TB) void resize_v(const T* __restrict__ x, T* __restrict__ out,
                                               const int* __restrict__ bounds, const double* __restrict__ kk,
                                               int ksize, int h, int oh, long rowlen, int chunks, float lo) {
  typedef typename Px<T>::acc_t A;
  const unsigned b = blockIdx.x;
  const long e = (long)(b % (unsigned)chunks) * TB + threadIdx.x;
  const unsigned t = b / (unsigned)chunks;
  const int oy = (int)(t % (unsigned)oh);
  const size_t img = t / (unsigned)oh;
  if (e >= rowlen) return;
  const int ym = clampi(bounds[2 * oy], 0, h);
  const int nn = clampi(bounds[2 * oy + 1], 0, min(ksize, h - ym));
  const double* k = kk + (size_t)oy * ksize;
  const T* p = x + (img * h + ym) * rowlen + e;
  out[(img * oh + oy) * rowlen + e] = (T)Px<T>::finish(accumulate<T>(p, (size_t)rowlen, k, nn), lo);
}

__global__ __launch_bounds__(TB) void resize_copy_f32(const float* __restrict__ x, float* __restrict__ out, long total,
                                                      float lo) {
  const long i = (long)blockIdx.x * TB + threadIdx.x;
  if (i >= total) return;
  const float v = x[i];
  out[i] = v < lo ? lo : v;
}
__global__ __launch_bounds__(TB) void resize_copy_u8(const uint8_t* __restrict__ x, uint8_t* __restrict__ out,
                                                     long total) {
  const long i = (long)blockIdx.x * TB + threadIdx.x;
  if (i < total) out[i] = x[i];
}

template <typename T>
void launch_h(const T* x, T* out, const int* bounds, const double* kk, int ksize, long rows, int w, int ow, float lo,
              hipStream_t s) {
  HPlan p = plan_h(w, ow, ksize);
  if (p.tile == 0) p = HPlan{DIRECT_TILE, -1, 0, 0, 0};
  const long tiles = (ow + p.tile - 1) / p.tile, strips = (rows + ROWS - 1) / ROWS;
  hipLaunchKernelGGL(resize_h<T>, dim3((unsigned)(tiles * strips)), dim3(TBH), p.lds, s, x, out, bounds, kk, ksize,
                     rows, w, ow, p.tile, p.cap_px, p.pitch_in, p.pitch_out, lo);
}
template <typename T>
void launch_v(const T* x, T* out, const int* bounds, const double* kk, int ksize, int n, int h, int oh, int width,
              float lo, hipStream_t s) {
  const long rowlen = 3L * width;
  const int chunks = (int)((rowlen + TB - 1) / TB);
  hipLaunchKernelGGL(resize_v<T>, dim3((unsigned)((long)chunks * oh * n)), dim3(TB), 0, s, x, out, bounds, kk, ksize,
                     h, oh, rowlen, chunks, lo);
}

bool disjoint(uintptr_t a, uintptr_t alen, uintptr_t b, uintptr_t blen) { return a + alen <= b || b + blen <= a; }

}  // namespace

extern "C" {

int cnnitmo_resize_coeffs(int in, int out, int filter, int* bounds, double* kk) {
  CNN_REQUIRE(in > 0 && out > 0, "resize_coeffs: in %d, out %d", in, out);
  CNN_REQUIRE(filter >= 0 && filter <= CNNITMO_RESIZE_LANCZOS, "resize_coeffs: unknown filter %d", filter);
  CNN_REQUIRE((bounds == nullptr) == (kk == nullptr), "resize_coeffs: bounds and kk are given together or not at all");
  const double scale = (double)in / out;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = SUPPORT[filter] * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  if (!bounds) return ksize;
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double* k = kk + (size_t)xx * ksize;
    int x = 0;
    for (; x < xmax; ++x) {
      const double wgt = filter_value(filter, (x + xmin - center + 0.5) * ss);
      k[x] = wgt;
      ww += wgt;
    }
    if (ww != 0.0)
      for (x = 0; x < xmax; ++x) k[x] /= ww;
    for (x = xmax < 0 ? 0 : xmax; x < ksize; ++x) k[x] = 0.0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

int cnnitmo_resize_tile_cols(int w, int ow, int ksize_x) {
  if (w < 1 || ow < 1 || ksize_x < 1) return 0;
  return plan_h(w, ow, ksize_x).tile;
}

long cnnitmo_resize_workspace_bytes(int dtype, int n, int h, int w, int oh, int ow) {
  if ((dtype != 0 && dtype != 1) || n < 1 || h < 1 || w < 1 || oh < 1 || ow < 1) return 0;
  if (w == ow || h == oh) return 0;
  return (long)n * h * ow * 3 * (dtype == 0 ? 4 : 1);
}

int cnnitmo_resize(const void* x, int dtype, int n, int h, int w, void* out, int oh, int ow, const int* bounds_x,
                   const double* kk_x, int ksize_x, const int* bounds_y, const double* kk_y, int ksize_y, float lo,
                   void* workspace, void* stream) {
  CNN_REQUIRE(dtype == 0 || dtype == 1, "resize: dtype %d (0 fp32, 1 uint8)", dtype);
  CNN_REQUIRE(x && out, "resize: null picture");
  CNN_REQUIRE(n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "resize: n %d, %d x %d -> %d x %d", n, h, w, oh, ow);
  const bool do_h = w != ow, do_v = h != oh;
  const long es = dtype == 0 ? 4 : 1;
  const long wmax = w > ow ? w : ow, hmax = h > oh ? h : oh;
  CNN_REQUIRE((double)n * hmax * wmax * 3 < 2147483648.0, "resize: more than 2^31 values in a picture batch");
  if (dtype == 0)
    CNN_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)workspace % 4 == 0,
                "resize: fp32 pictures need 4-byte alignment");
  else
    CNN_REQUIRE(!(lo > -INFINITY), "resize: a floor is for fp32 pictures");
  CNN_REQUIRE(!(lo != lo), "resize: lo is NaN");
  const uintptr_t xlen = (uintptr_t)(es * n * h * w * 3), olen = (uintptr_t)(es * n * oh * ow * 3);
  CNN_REQUIRE(disjoint((uintptr_t)x, xlen, (uintptr_t)out, olen), "resize: out overlaps x");
  if (do_h) {
    CNN_REQUIRE(bounds_x && kk_x, "resize: null horizontal tables");
    CNN_REQUIRE(ksize_ok(w, ow, ksize_x), "resize: ksize_x %d does not belong to %d -> %d", ksize_x, w, ow);
  }
  if (do_v) {
    CNN_REQUIRE(bounds_y && kk_y, "resize: null vertical tables");
    CNN_REQUIRE(ksize_ok(h, oh, ksize_y), "resize: ksize_y %d does not belong to %d -> %d", ksize_y, h, oh);
  }
  if (do_h && do_v) {
    CNN_REQUIRE(workspace, "resize: two passes need a workspace");
    const uintptr_t wlen = (uintptr_t)(es * n * h * ow * 3);
    CNN_REQUIRE(disjoint((uintptr_t)workspace, wlen, (uintptr_t)x, xlen) &&
                    disjoint((uintptr_t)workspace, wlen, (uintptr_t)out, olen),
                "resize: the workspace overlaps a picture");
  }
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)n * h;
  if (dtype == 0) {
    const float* xf = (const float*)x;
    float* of = (float*)out;
    float* mid = do_v ? (float*)workspace : of;
    if (do_h) launch_h<float>(xf, mid, bounds_x, kk_x, ksize_x, rows, w, ow, do_v ? -INFINITY : lo, s);
    if (do_v) launch_v<float>(do_h ? mid : xf, of, bounds_y, kk_y, ksize_y, n, h, oh, ow, lo, s);
    if (!do_h && !do_v) {
      const long total = rows * w * 3;
      hipLaunchKernelGGL(resize_copy_f32, dim3((unsigned)((total + TB - 1) / TB)), dim3(TB), 0, s, xf, of, total, lo);
    }
  } else {
    const uint8_t* xb = (const uint8_t*)x;
    uint8_t* ob = (uint8_t*)out;
    uint8_t* mid = do_v ? (uint8_t*)workspace : ob;
    if (do_h) launch_h<uint8_t>(xb, mid, bounds_x, kk_x, ksize_x, rows, w, ow, 0.f, s);
    if (do_v) launch_v<uint8_t>(do_h ? mid : xb, ob, bounds_y, kk_y, ksize_y, n, h, oh, ow, 0.f, s);
    if (!do_h && !do_v) {
      const long total = rows * w * 3;
      hipLaunchKernelGGL(resize_copy_u8, dim3((unsigned)((total + TB - 1) / TB)), dim3(TB), 0, s, xb, ob, total);
    }
  }
  return cnnitmo_check_launch("resize");
}

}  // extern "C"
