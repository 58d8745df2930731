// A baseline-JPEG encode/decode round trip of 8-bit RGB frames: cnnitmo_jpeg_roundtrip.
//
// The arithmetic is the IJG library's pixel path (libjpeg 6b / libjpeg-turbo with their defaults),
// restated in int32 and stated step by step in include/cnn_itmo.h and tests/jpeg_ref.py: uint8(255 x),
// RGB -> YCbCr (jccolor.c), h2v2 box downsampling (jcsample.c), the slow-integer forward DCT
// (jfdctint.c), quantise / dequantise, the slow-integer inverse DCT (jidctint.c), triangle
// ("fancy") chroma upsampling (jdsample.c), YCbCr -> RGB (jdcolor.c).  No float after the load, no
// atomics, one code path whatever the alignment of x and out: bitwise reproducible.
//
// Two launches per group of GROUP images, the decoded planes held as uint8 in the workspace:
//   1. jpeg_codec   one workgroup per tile of TILE_W x 64 (4:2:0) or TILE_W x 32 (4:4:4) pixels = 96
//                   8x8 blocks in LDS (int32, rows padded to 9: the row pass and the column pass are
//                   both free of bank conflicts).  Load + colour transform (+ 2x2 average), then three
//                   passes of 768 one-dimensional tasks, three per thread: forward rows | forward
//                   columns, quantise, dequantise, inverse columns (all in the thread's registers) |
//                   inverse rows, clamp, 8 bytes stored.  Reads 12 B per pixel, writes 1.5 B (3 B).
//   2. jpeg_finish  one thread per pixel: Y, the chroma (4:2:0: the triangle filter over the decoded
//                   chroma samples, which is why they have to exist for the neighbouring blocks
//                   first), YCbCr -> RGB, the floats staged in LDS and stored by consecutive lanes
//                   to consecutive dwords as hdrpairs.hip does.  Reads 1.5 B (3 B), writes 12 B.
// The quantisation tables and the apply flags are host arrays: they are checked before any launch
// and travel as kernel arguments, GROUP images at a time (no copy, no allocation, nothing to keep
// alive after the call returns).
#include "common.h"
#include "tonemap_px.h"  // im2uint8

#include <limits.h>

namespace {

constexpr int TB = 256;     // threads per block
constexpr int GROUP = 8;    // images per launch
constexpr int TILE_W = 64;  // tile width in pixels; the height is 64 (4:2:0) or 32 (4:4:4)
constexpr int NBLK = 96;    // 8x8 blocks per tile: 64 + 16 + 16 or 32 + 32 + 32
constexpr int RS = 9;       // ints per block row in LDS
constexpr int BS = 8 * RS;  // ints per block

struct Tables {
  uint16_t q[GROUP][2][64];
  uint8_t apply[GROUP];
};
struct Flags {
  uint8_t apply[GROUP];
};

// the decoded planes of one image in the workspace: Y [hy][wy], Cb [hc][wc], Cr [hc][wc], uint8
struct Geom {
  int hy, wy, hc, wc;
  long bytes;  // per image, a multiple of 64
};

Geom geom_of(int h, int w, int sub) {
  const int m = sub ? 16 : 8;
  Geom g;
  g.hy = (int)(((long)h + m - 1) / m * m);
  g.wy = (int)(((long)w + m - 1) / m * m);
  g.hc = sub ? g.hy / 2 : g.hy;
  g.wc = sub ? g.wy / 2 : g.wy;
  g.bytes = (long)g.hy * g.wy + 2L * g.hc * g.wc;
  return g;
}

// jfdctint.c / jidctint.c: FIX(v) = round(v * 2^13)
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270;
constexpr int F_0_899976223 = 7373, F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137;
constexpr int F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;

__device__ __forceinline__ int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// one pass of jpeg_fdct_islow over d[0..7]; PASS2: the column pass's scaling
template <bool PASS2> __device__ __forceinline__ void fdct8(int* d) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int n = PASS2 ? CONST_BITS + PASS1_BITS : CONST_BITS - PASS1_BITS;
  if (PASS2) {
    d[0] = descale(t10 + t11, PASS1_BITS);
    d[4] = descale(t10 - t11, PASS1_BITS);
  } else {
    d[0] = (t10 + t11) << PASS1_BITS;
    d[4] = (t10 - t11) << PASS1_BITS;
  }
  int z1 = (t12 + t13) * F_0_541196100;
  d[2] = descale(z1 + t13 * F_0_765366865, n);
  d[6] = descale(z1 + t12 * -F_1_847759065, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * F_1_175875602;
  const int m4 = t4 * F_0_298631336, m5 = t5 * F_2_053119869, m6 = t6 * F_3_072711026, m7 = t7 * F_1_501321110;
  z1 *= -F_0_899976223;
  z2 *= -F_2_562915447;
  z3 = z3 * -F_1_961570560 + z5;
  z4 = z4 * -F_0_390180644 + z5;
  d[7] = descale(m4 + z1 + z3, n);
  d[5] = descale(m5 + z2 + z4, n);
  d[3] = descale(m6 + z2 + z3, n);
  d[1] = descale(m7 + z1 + z4, n);
}

// one pass of jpeg_idct_islow over d[0..7]; PASS2: the row pass's scaling (+ 128 and the clamp: the caller)
template <bool PASS2> __device__ __forceinline__ void idct8(int* d) {
  int z1 = (d[2] + d[6]) * F_0_541196100;
  int t2 = z1 + d[6] * -F_1_847759065;
  int t3 = z1 + d[2] * F_0_765366865;
  int t0 = (d[0] + d[4]) << CONST_BITS, t1 = (d[0] - d[4]) << CONST_BITS;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = d[7];
  t1 = d[5];
  t2 = d[3];
  t3 = d[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * F_1_175875602;
  t0 *= F_0_298631336;
  t1 *= F_2_053119869;
  t2 *= F_3_072711026;
  t3 *= F_1_501321110;
  z1 *= -F_0_899976223;
  z2 *= -F_2_562915447;
  z3 = z3 * -F_1_961570560 + z5;
  z4 = z4 * -F_0_390180644 + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  constexpr int n = PASS2 ? CONST_BITS + PASS1_BITS + 3 : CONST_BITS - PASS1_BITS;
  d[0] = descale(t10 + t3, n);
  d[7] = descale(t10 - t3, n);
  d[1] = descale(t11 + t2, n);
  d[6] = descale(t11 - t2, n);
  d[2] = descale(t12 + t1, n);
  d[5] = descale(t12 - t1, n);
  d[3] = descale(t13 + t0, n);
  d[4] = descale(t13 - t0, n);
}

struct Ycc {
  int y, cb, cr;
};

// pixel (r, c) of an h x w frame, inside it: 8-bit samples, then jccolor.c
__device__ __forceinline__ Ycc load_ycc(const float* __restrict__ img, int w, int r, int c) {
  const float* p = img + 3 * ((long)r * w + c);
  const int R = im2uint8((double)p[0]), G = im2uint8((double)p[1]), B = im2uint8((double)p[2]);
  Ycc v;
  v.y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
  v.cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
  v.cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
  return v;
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// SUB 1: 4:2:0, tile TILE_W x 64, LDS blocks Y 0..63 (8 x 8), Cb 64..79 (4 x 4), Cr 80..95
// SUB 0: 4:4:4, tile TILE_W x 32, LDS blocks Y 0..31 (4 rows of 8), Cb 32..63, Cr 64..95
template <int SUB>
__global__ __launch_bounds__(TB) void jpeg_codec(const float* __restrict__ x, int h, int w, Geom g, Tables tb,
                                                 int img0, uint8_t* __restrict__ planes) {
  constexpr int TH = SUB ? 64 : 32;
  constexpr int NY = SUB ? 64 : 32;  // luminance blocks
  constexpr int NC = SUB ? 16 : 32;  // blocks of one chroma plane
  constexpr int CBW = SUB ? 4 : 8;   // chroma blocks per tile row
  __shared__ int blk[NBLK * BS];
  __shared__ int qt[2][64];
  const int li = blockIdx.z, tid = threadIdx.x;
  if (!tb.apply[li]) return;
  if (tid < 128) qt[tid >> 6][tid & 63] = tb.q[li][tid >> 6][tid & 63];
  const long im = (long)img0 + li;
  const float* img = x + 3 * im * h * w;
  const int r_org = blockIdx.y * TH, c_org = blockIdx.x * TILE_W;

  if (SUB) {
    const int hct = (h + 1) >> 1;
    for (int q = tid; q < (TH / 2) * (TILE_W / 2); q += TB) {
      const int qy = q / (TILE_W / 2), qx = q % (TILE_W / 2);
      const int r0 = r_org + 2 * qy, c0 = c_org + 2 * qx;
      const int ca = min(c0, w - 1), cb = min(c0 + 1, w - 1);
      const int ra = min(r0, h - 1), rb = min(r0 + 1, h - 1);
      const Ycc p00 = load_ycc(img, w, ra, ca), p01 = load_ycc(img, w, ra, cb);
      const Ycc p10 = load_ycc(img, w, rb, ca), p11 = load_ycc(img, w, rb, cb);
      int* yb = blk + ((qy >> 2) * 8 + (qx >> 2)) * BS + ((2 * qy) & 7) * RS + ((2 * qx) & 7);
      yb[0] = p00.y - 128;
      yb[1] = p01.y - 128;
      yb[RS] = p10.y - 128;
      yb[RS + 1] = p11.y - 128;
      int scb = p00.cb + p01.cb + p10.cb + p11.cb, scr = p00.cr + p01.cr + p10.cr + p11.cr;
      const int ci = (r_org >> 1) + qy;
      if (ci >= hct) {  // a chroma row below the picture repeats the last chroma row, not the last pixel row
        const int sa = min(2 * hct - 2, h - 1), sb = min(2 * hct - 1, h - 1);
        const Ycc s00 = load_ycc(img, w, sa, ca), s01 = load_ycc(img, w, sa, cb);
        const Ycc s10 = load_ycc(img, w, sb, ca), s11 = load_ycc(img, w, sb, cb);
        scb = s00.cb + s01.cb + s10.cb + s11.cb;
        scr = s00.cr + s01.cr + s10.cr + s11.cr;
      }
      const int bias = (((c_org >> 1) + qx) & 1) ? 2 : 1;
      int* cp = blk + (NY + (qy >> 3) * CBW + (qx >> 3)) * BS + (qy & 7) * RS + (qx & 7);
      cp[0] = ((scb + bias) >> 2) - 128;
      cp[NC * BS] = ((scr + bias) >> 2) - 128;
    }
  } else {
    for (int p = tid; p < TH * TILE_W; p += TB) {
      const int ly = p / TILE_W, lx = p % TILE_W;
      const Ycc v = load_ycc(img, w, min(r_org + ly, h - 1), min(c_org + lx, w - 1));
      int* yb = blk + ((ly >> 3) * 8 + (lx >> 3)) * BS + (ly & 7) * RS + (lx & 7);
      yb[0] = v.y - 128;
      yb[NY * BS] = v.cb - 128;
      yb[(NY + NC) * BS] = v.cr - 128;
    }
  }
  __syncthreads();

  int d[8];
  // forward DCT, rows
  for (int t = tid; t < NBLK * 8; t += TB) {
    int* p = blk + (t >> 3) * BS + (t & 7) * RS;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = p[k];
    fdct8<false>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = d[k];
  }
  __syncthreads();
  // forward DCT columns, quantise, dequantise, inverse DCT columns
  for (int t = tid; t < NBLK * 8; t += TB) {
    const int b = t >> 3, c = t & 7;
    int* p = blk + b * BS + c;
    const int* q = qt[b < NY ? 0 : 1] + c;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = p[k * RS];
    fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned Q = (unsigned)q[8 * k], q8 = Q << 3;  // the forward DCT leaves 8 x the coefficient
      const unsigned a = ((unsigned)abs(d[k]) + (q8 >> 1)) / q8;
      const int v = (int)(a * Q);
      d[k] = d[k] < 0 ? -v : v;
    }
    idct8<false>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k * RS] = d[k];
  }
  __syncthreads();
  // inverse DCT rows, + 128, clamp, store 8 bytes
  uint8_t* base = planes + im * g.bytes;
  for (int t = tid; t < NBLK * 8; t += TB) {
    const int b = t >> 3, r = t & 7;
    const int* p = blk + b * BS + r * RS;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = p[k];
    idct8<true>(d);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (uint32_t)clamp255(d[k] + 128) << (8 * k);
      hi |= (uint32_t)clamp255(d[k + 4] + 128) << (8 * k);
    }
    uint8_t* plane;
    int ph, pw, gy, gx;
    if (b < NY) {
      plane = base;
      ph = g.hy;
      pw = g.wy;
      gy = r_org + (b >> 3) * 8 + r;
      gx = c_org + (b & 7) * 8;
    } else {
      const int cbk = (b - NY) % NC;
      plane = base + (long)g.hy * g.wy + (b - NY < NC ? 0L : (long)g.hc * g.wc);
      ph = g.hc;
      pw = g.wc;
      gy = (SUB ? r_org >> 1 : r_org) + (cbk / CBW) * 8 + r;
      gx = (SUB ? c_org >> 1 : c_org) + (cbk % CBW) * 8;
    }
    if (gy < ph && gx < pw)  // pw is a multiple of 8: the whole row of the block is inside
      *reinterpret_cast<uint2*>(plane + (long)gy * pw + gx) = make_uint2(lo, hi);
  }
}

// the first nfl floats of the block's staged tile to dst: lane j -> dword j
__device__ __forceinline__ void store_tile(float* __restrict__ dst, const float* tile, int nfl) {
  for (int j = threadIdx.x; j < nfl; j += TB) dst[j] = tile[j];
}

// x, out: the first image of the group; total = the group's pixels.  x is read only for images that
// are copied through, and then pixel i only by the block that writes pixel i: out may be x.
template <int SUB>
__global__ __launch_bounds__(TB) void jpeg_finish(const float* x, int h, int w, Geom g, Flags fl,
                                                  const uint8_t* __restrict__ planes, float* out, long total) {
  __shared__ float so[3 * TB];
  const long base = (long)blockIdx.x * TB;
  const long i = base + threadIdx.x;
  if (i < total) {
    const long hw = (long)h * w;
    const int li = (int)(i / hw);
    const long rem = i - (long)li * hw;
    const int r = (int)(rem / w), c = (int)(rem - (long)r * w);
    const int t = 3 * threadIdx.x;
    if (fl.apply[li]) {
      const uint8_t* py = planes + li * g.bytes;
      const uint8_t* pcb = py + (long)g.hy * g.wy;
      const uint8_t* pcr = pcb + (long)g.hc * g.wc;
      const int Y = py[(long)r * g.wy + c];
      int cb, cr;
      if (SUB) {
        const int hct = (h + 1) >> 1, wct = (w + 1) >> 1;
        const int ci = r >> 1, cj = c >> 1;
        const int ci2 = (r & 1) ? min(ci + 1, hct - 1) : max(ci - 1, 0);
        const int cj2 = (c & 1) ? min(cj + 1, wct - 1) : max(cj - 1, 0);
        const long a = (long)ci * g.wc, a2 = (long)ci2 * g.wc;
        const int rnd = (c & 1) ? 7 : 8;
        cb = (3 * (3 * pcb[a + cj] + pcb[a2 + cj]) + (3 * pcb[a + cj2] + pcb[a2 + cj2]) + rnd) >> 4;
        cr = (3 * (3 * pcr[a + cj] + pcr[a2 + cj]) + (3 * pcr[a + cj2] + pcr[a2 + cj2]) + rnd) >> 4;
      } else {
        cb = pcb[(long)r * g.wc + c];
        cr = pcr[(long)r * g.wc + c];
      }
      cb -= 128;
      cr -= 128;
      const int R = clamp255(Y + ((91881 * cr + 32768) >> 16));
      const int G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      const int B = clamp255(Y + ((116130 * cb + 32768) >> 16));
      so[t] = (float)R * (float)(1 / 255.);
      so[t + 1] = (float)G * (float)(1 / 255.);
      so[t + 2] = (float)B * (float)(1 / 255.);
    } else {
      const float* p = x + 3 * i;
      so[t] = p[0];
      so[t + 1] = p[1];
      so[t + 2] = p[2];
    }
  }
  __syncthreads();
  const long left = total - base;
  store_tile(out + 3 * base, so, 3 * (int)(left < TB ? left : TB));
}

bool shape_ok(int n, int h, int w, int sub) {
  return n >= 1 && h >= 1 && w >= 1 && (sub == 0 || sub == 1) && (long)h * w <= INT_MAX / 4 &&
         (long)n * h * w < (1L << 38) && h <= (1 << 21) - 64;  // (grid.y <= 65535 tiles of 32 rows)
}

}  // namespace

extern "C" long cnnitmo_jpeg_workspace_bytes(int n, int h, int w, int subsampling) {
  return shape_ok(n, h, w, subsampling) ? n * geom_of(h, w, subsampling).bytes : 0;
}

extern "C" int cnnitmo_jpeg_roundtrip(const float* x, int n, int h, int w, int subsampling,
                                      const unsigned short* qtabs, const unsigned char* apply, float* out,
                                      void* workspace, long workspace_bytes, void* stream) {
  CNN_REQUIRE(x && qtabs && out && workspace, "jpeg_roundtrip: null pointer");
  CNN_REQUIRE(n >= 1 && h >= 1 && w >= 1, "jpeg_roundtrip: bad shape %d x %d x %d", n, h, w);
  CNN_REQUIRE(subsampling == 0 || subsampling == 1, "jpeg_roundtrip: subsampling %d (0: 4:4:4, 1: 4:2:0)",
              subsampling);
  CNN_REQUIRE(shape_ok(n, h, w, subsampling), "jpeg_roundtrip: too large");
  CNN_REQUIRE(workspace_bytes >= cnnitmo_jpeg_workspace_bytes(n, h, w, subsampling),
              "jpeg_roundtrip: workspace too small");
  CNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "jpeg_roundtrip: workspace is not 8-byte aligned");
  CNN_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "jpeg_roundtrip: x or out is not 4-byte aligned");
  const long hw = (long)h * w;
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out, len = (uintptr_t)(12 * hw * n);
  CNN_REQUIRE(xa == oa || xa + len <= oa || oa + len <= xa, "jpeg_roundtrip: out overlaps x without being x");
  for (long k = 0; k < (long)n * 128; ++k)
    CNN_REQUIRE(qtabs[k] != 0, "jpeg_roundtrip: table entry %ld of image %ld is 0", k % 128, k / 128);
  hipStream_t s = (hipStream_t)stream;
  const Geom g = geom_of(h, w, subsampling);
  const int th = subsampling ? 64 : 32;
  const dim3 tiles((g.wy + TILE_W - 1) / TILE_W, (g.hy + th - 1) / th, 1);
  uint8_t* planes = (uint8_t*)workspace;
  for (int i0 = 0; i0 < n; i0 += GROUP) {
    const int cnt = n - i0 < GROUP ? n - i0 : GROUP;
    Tables tb;
    Flags fl;
    bool any = false;
    for (int i = 0; i < GROUP; ++i) {
      const bool on = i < cnt && (!apply || apply[i0 + i]);
      tb.apply[i] = fl.apply[i] = on;
      any |= on;
      for (int k = 0; k < 128; ++k) (&tb.q[i][0][0])[k] = i < cnt ? qtabs[(long)(i0 + i) * 128 + k] : 1;
    }
    const float* xg = x + 3 * hw * i0;
    float* og = out + 3 * hw * i0;
    if (!any && xg == og) continue;  // a group that is copied through onto itself
    const long total = hw * cnt;
    const dim3 grid1(tiles.x, tiles.y, cnt);
    const unsigned grid2 = (unsigned)((total + TB - 1) / TB);
    if (subsampling) {
      if (any) hipLaunchKernelGGL(jpeg_codec<1>, grid1, dim3(TB), 0, s, x, h, w, g, tb, i0, planes);
      hipLaunchKernelGGL(jpeg_finish<1>, dim3(grid2), dim3(TB), 0, s, xg, h, w, g, fl,
                         (const uint8_t*)(planes + i0 * g.bytes), og, total);
    } else {
      if (any) hipLaunchKernelGGL(jpeg_codec<0>, grid1, dim3(TB), 0, s, x, h, w, g, tb, i0, planes);
      hipLaunchKernelGGL(jpeg_finish<0>, dim3(grid2), dim3(TB), 0, s, xg, h, w, g, fl,
                         (const uint8_t*)(planes + i0 * g.bytes), og, total);
    }
  }
  return cnnitmo_check_launch("jpeg_roundtrip");
}
