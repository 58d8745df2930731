// OpenEXR scan-line pixel path: cnnitmo_exr_unpack / cnnitmo_exr_pack (the container and zlib stay on
// the host, cnn_itmo_amd/exr.py).
//
// A picture is h lines of line_bytes bytes; a line holds, channel after channel, that channel's w
// values (HALF 2 bytes, FLOAT / UINT 4, little-endian).  Chunks of L = lines_per_chunk lines (the last
// may be short) follow each other without gaps: chunk i starts at byte i * L * line_bytes and has
// n = lines * line_bytes bytes, so no offset is ever read from memory.  A "coded" chunk holds ZIP's
// form of its n record bytes r: t = (r[0], r[2], ..., r[1], r[3], ...) with the odd-indexed bytes from
// position half = (n + 1) / 2 on, then t[i] <- t[i] - t[i-1] + 128 (mod 256) from left to right, i >= 1.
//
// unpack (raw -> fp32 [h][w][3]):
//   1. exr_segsum_kernel: a coded chunk is cut into segments of SEG bytes, one workgroup each; the
//      segment's byte sum mod 256 goes to the workspace.
//   2. exr_scan_kernel: a workgroup adds the sums of the segments before it in its chunk, scans its
//      own segment (16 bytes per thread, a shuffle scan of the thread totals inside each wave and the
//      four wave totals through LDS, then a second walk over the thread's bytes) and writes
//      d[i] = (t[0] + ... + t[i] - 128 i) mod 256, the undone predictor, to the workspace at the
//      position i has in raw.  128 i mod 256 is 128 for odd i and 0 for even i.  No workgroup waits
//      for another: the two launches are the order.
//   3. exr_gather_kernel: record byte j of a chunk is d[(j >> 1) + (j & 1) * half] when coded and
//      raw[j] when not.  A workgroup takes 1024 pixels of one line, a thread four neighbouring pixels:
//      per channel 4 * size contiguous record bytes, i.e. two runs of 2 * size bytes of d (the even and
//      the odd half) or one run of raw, read with the widest access the address allows (16 / 8 / 4
//      bytes, else bytes).  The thread's 12 converted values are the 48 contiguous output bytes of
//      its pixels; they go through LDS (three 16-byte stores per thread, bank-conflict free: eight
//      neighbouring lanes start on banks 0, 12, 24, 4, 16, 28, 8, 20) so that store k of thread t is
//      float4 k * 256 + t of the tile: consecutive lanes write consecutive 16 bytes (dwords when
//      the tile does not start on a 16-byte boundary).
// pack (fp32 [h][w][3] -> the writer's record bytes, channels B, G, R of one type, coded per chunk or
//   plain): one pass, a thread makes four neighbouring output bytes from the (up to five) record
//   bytes t[i-1 .. i+3] they need, each computed from its pixel.
//
// Every conversion is done on the bit patterns, so no rounding, denormal or contraction mode of the
// float unit takes part: HALF -> fp32 is exact (denormals normalised, inf / NaN with the payload
// shifted left by 13); FLOAT is a copy; UINT -> fp32 and fp32 -> HALF round to nearest, ties to even
// (overflow -> inf, a NaN keeps its top payload bits and stays a NaN).
// No atomics anywhere: results are bitwise reproducible.  All addresses depend on the sizes alone,
// never on a byte read, so a wrong `coded` flag gives wrong pixels and no stray access.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int PER = 16;            // bytes per thread of a segment
constexpr int SEG = NT * PER;      // 4096
constexpr int TILE = 4 * NT;       // pixels of a gather tile
constexpr long MAX_GRID = 0x7FFFFFFFL;

struct Chan {
  int off[3];
  int type[3];
};

__host__ __device__ inline int type_size(int t) { return t == CNNITMO_EXR_HALF ? 2 : 4; }

// ---- conversions on bits ---------------------------------------------------------------------
__device__ __forceinline__ uint32_t half_to_f32_bits(uint32_t h) {
  const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
  if (e == 31u) return s | 0x7F800000u | (m << 13);
  if (e != 0u) return s | ((e + 112u) << 23) | (m << 13);
  if (m == 0u) return s;
  const uint32_t p = 31u - (uint32_t)__clz((int)m);  // 0..9: m * 2^-24 = 1.f * 2^(p - 24)
  return s | ((p + 103u) << 23) | ((m << (23u - p)) & 0x7FFFFFu);
}

__device__ __forceinline__ uint32_t uint_to_f32_bits(uint32_t u) {
  if (u == 0u) return 0u;
  const uint32_t p = 31u - (uint32_t)__clz((int)u);
  if (p <= 23u) return ((p + 127u) << 23) | ((u << (23u - p)) & 0x7FFFFFu);
  const uint32_t sh = p - 23u, m = u >> sh, rem = u & ((1u << sh) - 1u), mid = 1u << (sh - 1u);
  const uint32_t up = (rem > mid || (rem == mid && (m & 1u))) ? 1u : 0u;
  return (((p + 127u) << 23) | (m & 0x7FFFFFu)) + up;  // a carry out of the fraction raises the exponent
}

__device__ __forceinline__ uint32_t f32_bits_to_half(uint32_t u) {
  const uint32_t s = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) {  // NaN: the top ten payload bits, never all zero
    const uint32_t m = (a >> 13) & 0x3FFu;
    return s | 0x7C00u | (m ? m : 1u);
  }
  const uint32_t e = a >> 23;
  if (e >= 113u) {  // at least 2^-14: a normal half unless it overflows
    if (a >= 0x47800000u) return s | 0x7C00u;  // >= 65536, inf
    const uint32_t r = a - (112u << 23);
    const uint32_t h = (r + 0xFFFu + ((r >> 13) & 1u)) >> 13;
    return s | (h > 0x7C00u ? 0x7C00u : h);
  }
  const uint32_t sh = 126u - e;  // value = m * 2^(e - 150) = (m >> sh) units of 2^-24
  if (e == 0u || sh > 24u) return s;  // below half the smallest denormal (at sh = 25: < 2^-25)
  const uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
  uint32_t h = m >> sh;
  const uint32_t rem = m & ((1u << sh) - 1u), mid = 1u << (sh - 1u);
  if (rem > mid || (rem == mid && (h & 1u))) ++h;
  return s | h;
}

__device__ __forceinline__ uint32_t to_f32_bits(uint32_t v, int type) {
  if (type == CNNITMO_EXR_HALF) return half_to_f32_bits(v);
  if (type == CNNITMO_EXR_UINT) return uint_to_f32_bits(v);
  return v;
}

// ---- bounded byte-run access -----------------------------------------------------------------
// NB bytes from p into q (little-endian dwords); only the first `valid` exist, the rest read as 0
template <int NB>
__device__ __forceinline__ void load_run(const uint8_t* p, int valid, uint32_t* q) {
  const uintptr_t a = (uintptr_t)p;
  if (valid >= NB && (a & (NB >= 16 ? 15 : NB - 1)) == 0) {
    if constexpr (NB == 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    } else if constexpr (NB == 8) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      q[0] = v.x; q[1] = v.y;
    } else {
      q[0] = *reinterpret_cast<const uint32_t*>(p);
    }
    return;
  }
  if (valid >= NB && (a & 3) == 0) {
#pragma unroll
    for (int i = 0; i < NB / 4; ++i) q[i] = reinterpret_cast<const uint32_t*>(p)[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < NB / 4; ++i) {
    uint32_t v = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4 * i + b < valid) v |= (uint32_t)p[4 * i + b] << (8 * b);
    q[i] = v;
  }
}

__device__ __forceinline__ void store_run16(uint8_t* p, int valid, const uint32_t* q) {
  const uintptr_t a = (uintptr_t)p;
  if (valid >= 16 && (a & 15) == 0) {
    *reinterpret_cast<uint4*>(p) = make_uint4(q[0], q[1], q[2], q[3]);
    return;
  }
  if (valid >= 16 && (a & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) reinterpret_cast<uint32_t*>(p)[i] = q[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < valid) p[i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
}

__device__ __forceinline__ uint32_t byte_sum(const uint32_t* q) {
  uint32_t s = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += (q[i] & 0xFFu) + ((q[i] >> 8) & 0xFFu) + ((q[i] >> 16) & 0xFFu) + (q[i] >> 24);
  return s;
}

// the sum of v over the workgroup, in every thread (a fixed tree: shuffles, then four LDS slots)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* slots) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // slots may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
  __syncthreads();
  return slots[0] + slots[1] + slots[2] + slots[3];
}

// bytes of chunk c: its lines * line_bytes
__device__ __forceinline__ long chunk_bytes(int c, int h, int L, long line_bytes) {
  const int lines = min(L, h - c * L);
  return (long)lines * line_bytes;
}

// workgroup b = chunk * nseg + segment
__global__ __launch_bounds__(NT) void exr_segsum_kernel(const uint8_t* __restrict__ raw,
                                                        const uint8_t* __restrict__ coded, int h, int L,
                                                        long line_bytes, int nseg, uint8_t* __restrict__ sums) {
  __shared__ uint32_t slots[4];
  const int c = (int)(blockIdx.x / (unsigned)nseg), sg = (int)(blockIdx.x % (unsigned)nseg);
  if (!coded[c]) return;
  const long n = chunk_bytes(c, h, L, line_bytes);
  const long at = (long)sg * SEG + (long)threadIdx.x * PER;
  uint32_t q[4] = {0u, 0u, 0u, 0u};
  if (at < n) load_run<16>(raw + (long)c * L * line_bytes + at, (int)min((long)PER, n - at), q);
  const uint32_t s = block_sum(byte_sum(q), slots);
  if (threadIdx.x == 0) sums[blockIdx.x] = (uint8_t)s;
}

__global__ __launch_bounds__(NT) void exr_scan_kernel(const uint8_t* __restrict__ raw,
                                                      const uint8_t* __restrict__ coded, int h, int L,
                                                      long line_bytes, int nseg, const uint8_t* __restrict__ sums,
                                                      uint8_t* __restrict__ d) {
  __shared__ uint32_t slots[4];
  const int c = (int)(blockIdx.x / (unsigned)nseg), sg = (int)(blockIdx.x % (unsigned)nseg);
  if (!coded[c]) return;
  const long n = chunk_bytes(c, h, L, line_bytes);
  const long at = (long)sg * SEG + (long)threadIdx.x * PER;
  if ((long)sg * SEG >= n) return;  // a segment past the end of a short last chunk (whole workgroup)
  // the segments before this one
  uint32_t before = 0u;
  for (int k = (int)threadIdx.x; k < sg; k += NT) before += sums[(long)c * nseg + k];
  before = block_sum(before, slots);
  // this segment
  const long base = (long)c * L * line_bytes + at;
  const int valid = at < n ? (int)min((long)PER, n - at) : 0;
  uint32_t q[4] = {0u, 0u, 0u, 0u};
  if (valid > 0) load_run<16>(raw + base, valid, q);
  const uint32_t mine = byte_sum(q);
  uint32_t incl = mine;  // inclusive scan of the thread totals inside the wave
  const int lane = (int)(threadIdx.x & 63);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  __syncthreads();
  if (lane == 63) slots[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t run = before + incl - mine;
  for (int wv = 0; wv < (int)(threadIdx.x >> 6); ++wv) run += slots[wv];
  if (valid <= 0) return;
  uint32_t out[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t v = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      run += (q[i] >> (8 * b)) & 0xFFu;
      // position at + 4 i + b has the parity of b: at is a multiple of 16
      v |= ((run + ((b & 1) ? 128u : 0u)) & 0xFFu) << (8 * b);
    }
    out[i] = v;
  }
  store_run16(d + base, valid, out);
}

// one channel's four values of pixels x0 .. x0 + 3 (those below w), as fp32 bits
template <int SZ>
__device__ __forceinline__ void gather4(const uint8_t* __restrict__ chunk, bool is_coded, long j0, long half,
                                        int npx, int type, uint32_t* v) {
  if (!is_coded) {
    uint32_t q[SZ];
    load_run<4 * SZ>(chunk + j0, npx * SZ, q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t u = SZ == 2 ? (q[i >> 1] >> (16 * (i & 1))) & 0xFFFFu : q[i];
      v[i] = to_f32_bits(u, type);
    }
    return;
  }
  // record bytes j0 + 2k at d[j0/2 + k], j0 + 2k + 1 at d[half + j0/2 + k], k < 2 SZ (j0 is even)
  uint32_t ev[SZ / 2], od[SZ / 2];
  load_run<2 * SZ>(chunk + (j0 >> 1), npx * (SZ / 2), ev);
  load_run<2 * SZ>(chunk + half + (j0 >> 1), npx * (SZ / 2), od);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t u;
    if (SZ == 2) {
      u = ((ev[0] >> (8 * i)) & 0xFFu) | (((od[0] >> (8 * i)) & 0xFFu) << 8);
    } else {
      const uint32_t e2 = (ev[i >> 1] >> (16 * (i & 1))) & 0xFFFFu, o2 = (od[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
      u = (e2 & 0xFFu) | ((o2 & 0xFFu) << 8) | ((e2 >> 8) << 16) | ((o2 >> 8) << 24);
    }
    v[i] = to_f32_bits(u, type);
  }
}

// workgroup b = line * tiles + tile; src = d for the coded chunks, raw for the others
__global__ __launch_bounds__(NT) void exr_gather_kernel(const uint8_t* __restrict__ raw,
                                                        const uint8_t* __restrict__ d,
                                                        const uint8_t* __restrict__ coded, int h, int w, int L,
                                                        long line_bytes, Chan ch, int tiles,
                                                        uint32_t* __restrict__ rgb) {
  __shared__ __attribute__((aligned(16))) uint32_t stage[3 * TILE];
  const int row = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
  const int c = row / L, l = row - c * L;
  const bool is_coded = coded != nullptr && coded[c] != 0;
  const long n = chunk_bytes(c, h, L, line_bytes);
  const uint8_t* chunk = (is_coded ? d : raw) + (long)c * L * line_bytes;
  const int x0 = tile * TILE + 4 * (int)threadIdx.x;
  const int npx = min(4, w - x0);
  uint32_t v[3][4];
  if (npx > 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int type = ch.type[k];
      const long j0 = (long)l * line_bytes + ch.off[k] + (long)x0 * type_size(type);
      if (type == CNNITMO_EXR_HALF)
        gather4<2>(chunk, is_coded, j0, (n + 1) / 2, npx, type, v[k]);
      else
        gather4<4>(chunk, is_coded, j0, (n + 1) / 2, npx, type, v[k]);
    }
    uint4* st = reinterpret_cast<uint4*>(stage) + 3 * threadIdx.x;  // pixels 4t .. 4t+3, interleaved
    st[0] = make_uint4(v[0][0], v[1][0], v[2][0], v[0][1]);
    st[1] = make_uint4(v[1][1], v[2][1], v[0][2], v[1][2]);
    st[2] = make_uint4(v[2][2], v[0][3], v[1][3], v[2][3]);
  }
  __syncthreads();
  const int nd = 3 * min(TILE, w - tile * TILE);  // dwords of this tile
  uint32_t* out = rgb + ((long)row * w + (long)tile * TILE) * 3;
  if (((uintptr_t)out & 15) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int q = k * NT + (int)threadIdx.x;
      if (4 * q + 3 < nd) {
        reinterpret_cast<uint4*>(out)[q] = reinterpret_cast<const uint4*>(stage)[q];
      } else {
        for (int i = 4 * q; i < nd; ++i) out[i] = stage[i];  // at most three dwords, of one thread
      }
    }
  } else {
    for (int i = (int)threadIdx.x; i < nd; i += NT) out[i] = stage[i];
  }
}

// record byte j of a chunk of the writer's layout (channels B, G, R of 1 << lsz bytes): byte j % size of
// value j / size = (line, channel, x).  j < 2^31: a chunk is at most 16 lines of < 2^27 bytes.
__device__ __forceinline__ uint32_t record_byte(const uint32_t* __restrict__ rgb, long row0, uint32_t w, int lsz,
                                                uint32_t j) {
  const uint32_t vi = j >> lsz, b = j & ((1u << lsz) - 1u);
  const uint32_t lc = vi / w, x = vi - lc * w;  // lc = line * 3 + channel
  const uint32_t l = lc / 3u, cc = lc - l * 3u;  // 0 B, 1 G, 2 R
  const uint32_t u = rgb[((row0 + l) * w + x) * 3 + (2u - cc)];
  const uint32_t val = lsz == 1 ? f32_bits_to_half(u) : u;
  return (val >> (8u * b)) & 0xFFu;
}

// thread i of workgroup (chunk, part): output bytes 4i .. 4i+3 of the chunk
__global__ __launch_bounds__(NT) void exr_pack_kernel(const uint32_t* __restrict__ rgb, int h, int w, int is_half,
                                                      int L, int is_coded, int parts, uint8_t* __restrict__ out) {
  const int c = (int)(blockIdx.x / (unsigned)parts), part = (int)(blockIdx.x % (unsigned)parts);
  const int lsz = is_half ? 1 : 2;
  const long line_bytes = (3L * w) << lsz;
  const long n = chunk_bytes(c, h, L, line_bytes), half = (n + 1) / 2;
  const long i0 = ((long)part * NT + threadIdx.x) * 4;
  if (i0 >= n) return;
  const long row0 = (long)c * L;
  const int cnt = (int)min(4L, n - i0);
  uint32_t word = 0u;
  if (is_coded) {
    // t[i] = r[2i] for i < half, r[2(i - half) + 1] from there on
    uint32_t prev = 0u;
    if (i0 > 0) {
      const long k = i0 - 1;
      prev = record_byte(rgb, row0, (uint32_t)w, lsz, (uint32_t)(k < half ? 2 * k : 2 * (k - half) + 1));
    }
    for (int m = 0; m < cnt; ++m) {
      const long k = i0 + m;
      const uint32_t t = record_byte(rgb, row0, (uint32_t)w, lsz, (uint32_t)(k < half ? 2 * k : 2 * (k - half) + 1));
      const uint32_t o = k == 0 ? t : (t - prev + 128u) & 0xFFu;
      prev = t;
      word |= o << (8 * m);
    }
  } else {
    for (int m = 0; m < cnt; ++m) word |= record_byte(rgb, row0, (uint32_t)w, lsz, (uint32_t)(i0 + m)) << (8 * m);
  }
  uint8_t* p = out + row0 * line_bytes + i0;
  if (cnt == 4 && ((uintptr_t)p & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = word;
  } else {
    for (int m = 0; m < cnt; ++m) p[m] = (uint8_t)(word >> (8 * m));
  }
}

long seg_count(int L, long line_bytes) { return ((long)L * line_bytes + SEG - 1) / SEG; }
long round16(long v) { return (v + 15) & ~15L; }

bool sizes_ok(int h, int L, long line_bytes) {
  return h > 0 && (L == 1 || L == 16) && line_bytes > 0 && (line_bytes & 1) == 0 &&
         line_bytes <= 0x7FFFFFFFL / 16 && (long)h * line_bytes < (1L << 40);
}

}  // namespace

extern "C" int cnnitmo_exr_segment_bytes(void) { return SEG; }

// the undone predictor d, h * line_bytes bytes (rounded up to 16), then one byte per segment
extern "C" long cnnitmo_exr_workspace_bytes(int h, int rows, long cols) {
  const int L = rows;
  const long line_bytes = cols;
  if (!sizes_ok(h, L, line_bytes)) return 0;
  const long nchunks = (h + L - 1) / L;
  return round16((long)h * line_bytes) + nchunks * seg_count(L, line_bytes);
}

extern "C" int cnnitmo_exr_unpack(const uint8_t* raw, const uint8_t* coded, int h, int w, int lines_per_chunk,
                                  long line_bytes, const int* ch_off, const int* ch_type, float* rgb,
                                  void* workspace, long workspace_bytes, void* stream) {
  const int L = lines_per_chunk;
  CNN_REQUIRE(raw && rgb && ch_off && ch_type, "exr_unpack: null pointer");
  CNN_REQUIRE(h > 0 && w > 0, "exr_unpack: size %d x %d", h, w);
  CNN_REQUIRE(L == 1 || L == 16, "exr_unpack: lines_per_chunk %d (1 or 16)", L);
  CNN_REQUIRE(sizes_ok(h, L, line_bytes), "exr_unpack: line_bytes %ld (positive, even, %d lines)", line_bytes, h);
  CNN_REQUIRE(((uintptr_t)rgb & 3) == 0, "exr_unpack: rgb is not 4-byte aligned");
  Chan ch;
  for (int k = 0; k < 3; ++k) {
    const int t = ch_type[k];
    CNN_REQUIRE(t == CNNITMO_EXR_UINT || t == CNNITMO_EXR_HALF || t == CNNITMO_EXR_FLOAT,
                "exr_unpack: channel %d has the unknown pixel type %d", k, t);
    CNN_REQUIRE(ch_off[k] >= 0 && (ch_off[k] & 1) == 0, "exr_unpack: channel %d offset %d (even, >= 0)", k,
                ch_off[k]);
    CNN_REQUIRE((long)ch_off[k] + (long)w * type_size(t) <= line_bytes,
                "exr_unpack: channel %d (offset %d, %d values of %d bytes) runs past line_bytes %ld", k, ch_off[k],
                w, type_size(t), line_bytes);
    ch.off[k] = ch_off[k];
    ch.type[k] = t;
  }
  const long nchunks = (h + L - 1) / L, nseg = seg_count(L, line_bytes);
  const long tiles = ((long)w + TILE - 1) / TILE;
  CNN_REQUIRE(nchunks * nseg <= MAX_GRID && (long)h * tiles <= MAX_GRID, "exr_unpack: %d x %d is too large", h, w);
  uint8_t* d = nullptr;
  if (coded) {
    const long need = cnnitmo_exr_workspace_bytes(h, L, line_bytes);
    CNN_REQUIRE(workspace, "exr_unpack: coded chunks need a workspace");
    CNN_REQUIRE(workspace_bytes >= need, "exr_unpack: workspace of %ld bytes, %ld needed", workspace_bytes, need);
    d = (uint8_t*)workspace;
    uint8_t* sums = d + round16((long)h * line_bytes);
    hipLaunchKernelGGL(exr_segsum_kernel, dim3((unsigned)(nchunks * nseg)), dim3(NT), 0, (hipStream_t)stream, raw,
                       coded, h, L, line_bytes, (int)nseg, sums);
    hipLaunchKernelGGL(exr_scan_kernel, dim3((unsigned)(nchunks * nseg)), dim3(NT), 0, (hipStream_t)stream, raw,
                       coded, h, L, line_bytes, (int)nseg, sums, d);
  }
  hipLaunchKernelGGL(exr_gather_kernel, dim3((unsigned)((long)h * tiles)), dim3(NT), 0, (hipStream_t)stream, raw, d,
                     coded, h, w, L, line_bytes, ch, (int)tiles, reinterpret_cast<uint32_t*>(rgb));
  return cnnitmo_check_launch("exr_unpack");
}

extern "C" int cnnitmo_exr_pack(const float* rgb, int h, int w, int pixel_type, int lines_per_chunk, int coded,
                                uint8_t* out, void* stream) {
  const int L = lines_per_chunk;
  CNN_REQUIRE(rgb && out, "exr_pack: null pointer");
  CNN_REQUIRE(h > 0 && w > 0, "exr_pack: size %d x %d", h, w);
  CNN_REQUIRE(pixel_type == CNNITMO_EXR_HALF || pixel_type == CNNITMO_EXR_FLOAT,
              "exr_pack: pixel type %d (HALF or FLOAT)", pixel_type);
  CNN_REQUIRE(L == 1 || L == 16, "exr_pack: lines_per_chunk %d (1 or 16)", L);
  CNN_REQUIRE(coded == 0 || coded == 1, "exr_pack: coded %d (0 or 1)", coded);
  CNN_REQUIRE(((uintptr_t)rgb & 3) == 0, "exr_pack: rgb is not 4-byte aligned");
  const long line_bytes = 3L * w * type_size(pixel_type);
  CNN_REQUIRE(sizes_ok(h, L, line_bytes), "exr_pack: %d x %d is too large", h, w);
  const long nchunks = (h + L - 1) / L;
  const long parts = ((long)L * line_bytes + 4 * NT - 1) / (4 * NT);
  CNN_REQUIRE(nchunks * parts <= MAX_GRID, "exr_pack: %d x %d is too large", h, w);
  hipLaunchKernelGGL(exr_pack_kernel, dim3((unsigned)(nchunks * parts)), dim3(NT), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(rgb), h, w, pixel_type == CNNITMO_EXR_HALF ? 1 : 0, L, coded,
                     (int)parts, out);
  return cnnitmo_check_launch("exr_pack");
}
