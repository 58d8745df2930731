// Host dispatch of the forward family: which kernel runs an op for a shape.
//
// Every op asks one route function, and the launch entry point, the *_stat_rows query and the
// *_kernel_name query of that op all act on its answer: the ladders below exist once, so the
// BN partial-sum rows the engine allocates are the rows of the kernel the launch runs.
// (DESIGN.md section 3 has the two ladders as a table.)  No kernel lives in this file.
#include <cstring>

#include "igemm_common.h"

namespace {

// ----------------------------------------------------------------------------
// Argument builders: one per geometry, dense views.  Entry points add their pointers, views
// and flags; queries the flags and (dummy, never dereferenced) pointers they assume.
// ----------------------------------------------------------------------------
FwdArgs base_args() {
  FwdArgs a;
  memset(&a, 0, sizeof(a));
  a.scale = 1;
  a.ntaps = 1;
  a.dyc = a.dxc = 1;  // single tap at offset (0, 0)
  return a;
}

// conv3x3 'same' forward: x [n][h][w][cin] -> [n][h][w][cout]
FwdArgs conv3x3_args(int n, int h, int w, int cin, int cout) {
  FwdArgs a = base_args();
  a.nimg = n; a.hs = h; a.ws = w; a.ho = h; a.wo = w;
  a.ntaps = 9;
  a.dyc = a.dxc = 0;
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 3; ++s) {
      a.dyc |= r << (2 * (r * 3 + s));  // offset r-1 encoded as r
      a.dxc |= s << (2 * (r * 3 + s));
    }
  a.cin = cin; a.N = cout; a.M = (long)n * h * w;
  a.a_ld = cin; a.out_ld = cout; a.cout = cout;
  return a;
}

// its input gradient: the same walk over dz [..][cout] with the flipped weights -> dx [..][cin]
FwdArgs conv3x3_dgrad_args(int n, int h, int w, int cout, int cin) { return conv3x3_args(n, h, w, cout, cin); }

// Conv2DTranspose 2x2 stride 2 forward: one tap, column tap * cout + co scattered to the 2x grid
FwdArgs tconv_fwd_args(int n, int h, int w, int cin, int cout) {
  FwdArgs a = base_args();
  a.nimg = n; a.hs = h; a.ws = w; a.ho = h; a.wo = w;
  a.cin = cin; a.N = 4 * cout; a.M = (long)n * h * w;
  a.a_ld = cin; a.out_ld = cout; a.scatter = 1; a.cout = cout;
  return a;
}

// its input gradient: four taps gathered from dout [n][2h][2w][cout] -> dx [n][h][w][cin]
FwdArgs tconv_dgrad_args(int n, int h, int w, int cin, int cout) {
  FwdArgs a = base_args();
  a.nimg = n; a.hs = 2 * h; a.ws = 2 * w; a.ho = h; a.wo = w; a.scale = 2;
  a.ntaps = 4;
  a.dyc = a.dxc = 0;
  for (int t = 0; t < 4; ++t) {  // tap t = (a, b): offset (a, b) on the 2x grid
    a.dyc |= ((t >> 1) + 1) << (2 * t);
    a.dxc |= ((t & 1) + 1) << (2 * t);
  }
  a.cin = cout; a.N = cin; a.M = (long)n * h * w;
  a.a_ld = cout; a.out_ld = cin; a.cout = cin;
  return a;
}

// the conv3x3 forward entry points' common operands
FwdArgs conv3x3_fwd_args(const void* x, int x_ld, int x_off, int n, int h, int w, int cin, const void* wt,
                         const float* bias, int cout, void* out, int out_ld, int out_off, int flags,
                         const float* aff_scale, const float* aff_shift, float* stat_part, const float* border) {
  FwdArgs a = conv3x3_args(n, h, w, cin, cout);
  a.a = x; a.a_ld = x_ld; a.a_off = x_off; a.b = wt;
  a.bias = bias; a.out = out; a.out_ld = out_ld; a.out_off = out_off;
  a.flags = flags; a.aff_scale = aff_scale; a.aff_shift = aff_shift;
  a.stats = stat_part;
  a.border = border;
  return a;
}

// the fused BN-backward dgrads as their queries see them (cnnitmo_conv3x3_dgrad_bn / _pooled)
FwdArgs dgrad_bn_args(int n, int h, int w, int cout, int cin, int c0, int c1) {
  FwdArgs a = conv3x3_dgrad_args(n, h, w, cout, cin);
  a.bnb_c0 = c0; a.bnb_c1 = c1; a.bnb_out = (void*)1; a.bnb_r_ld = 8;
  return a;
}
FwdArgs dgrad_bn_pooled_args(int n, int h, int w, int cout, int cin) {
  FwdArgs a = dgrad_bn_args(n, h, w, cout, cin, 0, cin);
  a.bnb_r_ld = cin;
  a.pool_out = (void*)1; a.pool_ld = cin; a.pool_idx = (unsigned char*)1;
  return a;
}

// ----------------------------------------------------------------------------
// Routes
// ----------------------------------------------------------------------------
enum Kernel { K_NONE, K_HALO, K_FWD2, K_FWD, K_TSTREAM, K_TFWD2P, K_TWS };

// The kernel that runs an op and the BN partial-sum rows that kernel writes.  K_NONE: no kernel
// takes this dtype (or, for the halo-only and stream-only ops, these sizes).  rows = 0 with an
// implicit GEMM: its launch refuses these sizes with its own message, so the queries answer
// no rows and no name.
struct Route {
  Kernel kernel;
  long rows;
};

inline bool is_bf16(int dtype) { return dtype == CNNITMO_BF16; }
inline bool is_f32(int dtype) { return dtype == CNNITMO_F32; }

// the halo kernel or nothing: the ops that only it implements, and the first rung of conv_route
Route halo_route(int dtype, const FwdArgs& a) {
  if ((!is_bf16(dtype) && !is_f32(dtype)) || !halo_handles(a, is_f32(dtype))) return {K_NONE, 0};
  return {K_HALO, halo_stat_rows(a, is_f32(dtype))};
}

// the implicit GEMMs: v2 for every column count but 32
Route igemm_route(long m, int ncols) {
  if (fwd2_handles(ncols)) return {K_FWD2, fwd2_stat_rows(m)};
  return {K_FWD, fwd_stat_rows(m, ncols)};
}
Route igemm_route(int dtype, const FwdArgs& a) {
  if (!is_bf16(dtype) && !is_f32(dtype)) return {K_NONE, 0};
  Route r = igemm_route(a.M, a.N);
  const int ve = is_bf16(dtype) ? 8 : 4;  // Vec16<T>::N
  if (!(r.kernel == K_FWD2 ? fwd2_sizes_ok(a, ve) : fwd_sizes_ok(a, ve))) r.rows = 0;
  return r;
}

// conv3x3 forward and input gradient: halo -> igemm_fwd2 -> igemm_fwd
Route conv_route(int dtype, const FwdArgs& a) {
  const Route r = halo_route(dtype, a);
  return r.kernel ? r : igemm_route(dtype, a);
}

// Conv2DTranspose forward (mode 0) and input gradient (mode 1), cin / cout the layer's:
// tconv_stream -> tconv_fwd2p (forward) -> tconv_ws -> igemm_fwd2 -> igemm_fwd
Route tconv_route(int dtype, int mode, int cin, int cout, const FwdArgs& a) {
  if (is_bf16(dtype) && tconv_stream_handles(mode, a.ho, a.wo, cin, cout, false))
    return {K_TSTREAM, tconv_stream_rows(mode, a.nimg, a.ho, a.wo, cin, cout, false)};
  if (is_bf16(dtype) && mode == 0 && tfwd2p_handles(a, true)) return {K_TFWD2P, tfwd2p_stat_rows(a)};
  if ((is_bf16(dtype) || is_f32(dtype)) && tconv_ws_handles(mode, cin, cout, is_f32(dtype)))
    return {K_TWS, tconv_ws_rows(cin, cout, is_f32(dtype))};
  return igemm_route(dtype, a);
}

// the Conv2DTranspose input gradient with the BN backward fused: the stream kernel or nothing
Route tconv_bn_route(int dtype, int n, int h, int w, int cout, int cin) {
  if (!is_bf16(dtype) || !tconv_stream_handles(1, h, w, cin, cout, true)) return {K_NONE, 0};
  return {K_TSTREAM, tconv_stream_rows(1, n, h, w, cin, cout, true)};
}

// names of conv_route's kernels ("": none)
const char* route_name(const Route& r, int dtype, const FwdArgs& a) {
  if (r.kernel == K_HALO) return halo_name(a, is_f32(dtype));
  if (r.kernel == K_FWD2 && r.rows) return fwd2_name(a, is_bf16(dtype));
  if (r.kernel == K_FWD && r.rows) return fwd_name(a.N, is_bf16(dtype));
  return "";
}

// launches of conv_route's kernels
int launch_route(const Route& r, int dtype, const FwdArgs& a, void* stream, const char* what) {
  hipStream_t s = (hipStream_t)stream;
  CNN_REQUIRE(a.M > 0 && a.N > 0 && a.cin > 0, "%s: empty (%ld pixels, %d -> %d channels)", what, a.M, a.cin, a.N);
  switch (r.kernel) {
    case K_HALO: return launch_halo(a, s, what, is_f32(dtype));
    case K_FWD2: return is_bf16(dtype) ? launch_fwd2<bf16>(a, s, what) : launch_fwd2<float>(a, s, what);
    case K_FWD: return is_bf16(dtype) ? launch_fwd<bf16>(a, s, what) : launch_fwd<float>(a, s, what);
    default: break;
  }
  cnnitmo_set_error("%s: unsupported dtype %d", what, dtype);
  return CNNITMO_EUNSUPPORTED;
}

}  // namespace

// ----------------------------------------------------------------------------
// conv3x3 forward and input gradient
// ----------------------------------------------------------------------------
// conv3x3 forward: the halo kernel writes one row per (XCD stream, wave), the
// implicit GEMM one per 256 pixels.
extern "C" long cnnitmo_conv3x3_stat_rows(int dtype, int n, int h, int w, int cin, int cout) {
  return conv_route(dtype, conv3x3_args(n, h, w, cin, cout)).rows;
}

extern "C" int cnnitmo_fwd_stat_rows(int dtype, long m, int ncols) {
  (void)dtype;
  if (m <= 0 || ncols <= 0 || ncols % 32) return 0;  // (launch_fwd / launch_fwd2 refuse these)
  return (int)igemm_route(m, ncols).rows;
}

// Name of the kernel cnnitmo_conv3x3_fwd (dgrad = 0) or cnnitmo_conv3x3_dgrad
// (dgrad = 1; cin/cout as in the layer) launches for these sizes (for profiles).
extern "C" const char* cnnitmo_conv3x3_kernel_name(int dtype, int n, int h, int w, int cin, int cout,
                                                   int dgrad) {
  FwdArgs a = dgrad ? conv3x3_dgrad_args(n, h, w, cout, cin) : conv3x3_args(n, h, w, cin, cout);
  if (!dgrad) a.flags = CNNITMO_RELU;  // the forward epilogue variant (every U-Net conv has one)
  return route_name(conv_route(dtype, a), dtype, a);
}

extern "C" int cnnitmo_conv3x3_fwd(int dtype, const void* x, int x_ld, int x_off, int n, int h,
                                   int w, int cin, const void* wt, const float* bias, int cout,
                                   void* out, int out_ld, int out_off, int flags,
                                   const float* aff_scale, const float* aff_shift,
                                   float* stat_part, const float* border, void* stream) {
  const FwdArgs a = conv3x3_fwd_args(x, x_ld, x_off, n, h, w, cin, wt, bias, cout, out, out_ld, out_off, flags,
                                     aff_scale, aff_shift, stat_part, border);
  CNN_REQUIRE(!(flags & CNNITMO_STATS) || stat_part, "conv3x3_fwd: STATS without buffer");
  CNN_REQUIRE(!(flags & CNNITMO_AFFINE) || (aff_scale && aff_shift), "conv3x3_fwd: AFFINE without coefficients");
  return launch_route(conv_route(dtype, a), dtype, a, stream, "conv3x3_fwd");
}

extern "C" int cnnitmo_conv3x3_dgrad(int dtype, const void* dz, int n, int h, int w, int cout,
                                     const void* wt_flip, int cin, void* dx, int dx_ld,
                                     int dx_off, void* stream) {
  FwdArgs a = conv3x3_dgrad_args(n, h, w, cout, cin);
  a.a = dz; a.b = wt_flip;
  a.out = dx; a.out_ld = dx_ld; a.out_off = dx_off;
  return launch_route(conv_route(dtype, a), dtype, a, stream, "conv3x3_dgrad");
}

extern "C" int cnnitmo_conv1tap_fwd(int dtype, const void* cols, int k, long m, const void* wt,
                                    const float* bias, int cout, void* out, int out_ld,
                                    int out_off, int flags, const float* aff_scale,
                                    const float* aff_shift, float* stat_part, void* stream) {
  FwdArgs a = base_args();
  a.a = cols; a.a_ld = k; a.a_off = 0;
  a.nimg = 1; a.hs = 1; a.ws = (int)m; a.ho = 1; a.wo = (int)m;
  a.cin = k; a.b = wt; a.N = cout; a.M = m;
  a.bias = bias; a.out = out; a.out_ld = out_ld; a.out_off = out_off;
  a.cout = cout; a.flags = flags; a.aff_scale = aff_scale; a.aff_shift = aff_shift;
  a.stats = stat_part;
  CNN_REQUIRE(m < (1L << 31), "conv1tap_fwd: too many pixels");
  return launch_route(igemm_route(dtype, a), dtype, a, stream, "conv1tap_fwd");
}

// ----------------------------------------------------------------------------
// conv3x3 ops that only the halo kernel implements
// ----------------------------------------------------------------------------
extern "C" int cnnitmo_conv3x3_fwd_pool(int dtype, const void* x, int x_ld, int x_off, int n, int h, int w,
                                        int cin, const void* wt, const float* bias, int cout, void* out, int out_ld,
                                        int out_off, int flags, const float* aff_scale, const float* aff_shift,
                                        float* stat_part, const float* border, void* pool_out, int pool_ld,
                                        unsigned char* pool_idx, const float* pool_sign, void* stream) {
  FwdArgs a = conv3x3_fwd_args(x, x_ld, x_off, n, h, w, cin, wt, bias, cout, out, out_ld, out_off, flags, aff_scale,
                               aff_shift, stat_part, border);
  a.pool_out = pool_out; a.pool_ld = pool_ld; a.pool_idx = pool_idx; a.pool_sign = pool_sign;
  CNN_REQUIRE(pool_out && pool_idx, "conv3x3_fwd_pool: missing pool buffers");
  CNN_REQUIRE(!(flags & CNNITMO_STATS) || stat_part, "conv3x3_fwd_pool: STATS without buffer");
  CNN_REQUIRE(!(flags & CNNITMO_AFFINE) || (aff_scale && aff_shift), "conv3x3_fwd_pool: AFFINE without coefficients");
  if (!halo_route(dtype, a).kernel) {
    cnnitmo_set_error("conv3x3_fwd_pool: unsupported (halo kernel with an epilogue, even h/w, pool_ld >= cout)");
    return CNNITMO_EUNSUPPORTED;
  }
  return launch_halo(a, (hipStream_t)stream, "conv3x3_fwd_pool", is_f32(dtype));
}

extern "C" int cnnitmo_conv3x3_pool_supported(int dtype, int n, int h, int w, int cin, int cout) {
  FwdArgs a = conv3x3_args(n, h, w, cin, cout);
  a.a = (const void*)16;
  a.flags = CNNITMO_RELU;
  a.pool_out = (void*)16; a.pool_ld = cout; a.pool_idx = (unsigned char*)16;
  return halo_route(dtype, a).kernel ? 1 : 0;
}

extern "C" int cnnitmo_conv3x3_fwd_head(int dtype, const void* x, int x_ld, int x_off, int n, int h, int w,
                                        int cin, const void* wt, const float* bias, int cout, int flags,
                                        const float* aff_scale, const float* aff_shift, int h_valid,
                                        const float* head_w, const float* head_b, float* yhat, void* stream) {
  FwdArgs a = conv3x3_fwd_args(x, x_ld, x_off, n, h, w, cin, wt, bias, cout, nullptr, cout, 0, flags, aff_scale,
                               aff_shift, nullptr, nullptr);
  a.head_w = head_w; a.head_b = head_b; a.yhat = yhat; a.head_hv = h_valid;
  CNN_REQUIRE(head_w && head_b && yhat, "conv3x3_fwd_head: missing head buffers");
  CNN_REQUIRE(h_valid > 0 && h_valid <= h, "conv3x3_fwd_head: bad h_valid");
  CNN_REQUIRE((long)n * h_valid * w * 12 < (1L << 31), "conv3x3_fwd_head: yhat too large for 32-bit offsets");
  CNN_REQUIRE(!(flags & CNNITMO_STATS), "conv3x3_fwd_head: the inference forward has no BN sums");
  CNN_REQUIRE(!(flags & CNNITMO_AFFINE) || (aff_scale && aff_shift), "conv3x3_fwd_head: AFFINE without coefficients");
  if (!halo_route(dtype, a).kernel) {
    cnnitmo_set_error("conv3x3_fwd_head: unsupported (halo kernel, 64 output channels)");
    return CNNITMO_EUNSUPPORTED;
  }
  return launch_halo(a, (hipStream_t)stream, "conv3x3_fwd_head", is_f32(dtype));
}

extern "C" int cnnitmo_conv3x3_head_supported(int dtype, int n, int h, int w, int cin, int cout) {
  FwdArgs a = conv3x3_args(n, h, w, cin, cout);
  a.a = (const void*)16;
  a.flags = CNNITMO_RELU | CNNITMO_AFFINE;
  a.head_w = a.head_b = (const float*)16; a.yhat = (float*)16; a.head_hv = h;
  return halo_route(dtype, a).kernel ? 1 : 0;
}

extern "C" int cnnitmo_conv3x3_fwd_cat(int dtype, const void* x1, int x1_ld, int x1_off, int c1, const void* x2,
                                       int x2_ld, int x2_off, int n, int h, int w, int cin, const void* wt,
                                       const float* bias, int cout, void* out, int out_ld, int out_off, int flags,
                                       const float* aff_scale, const float* aff_shift, float* stat_part,
                                       const float* border, void* stream) {
  FwdArgs a = conv3x3_fwd_args(x1, x1_ld, x1_off, n, h, w, cin, wt, bias, cout, out, out_ld, out_off, flags, aff_scale,
                               aff_shift, stat_part, border);
  a.a2 = x2; a.a2_ld = x2_ld; a.a2_off = x2_off; a.cin1 = c1;
  CNN_REQUIRE(x1 && x2 && c1 > 0 && c1 < cin, "conv3x3_fwd_cat: needs two sources splitting cin");
  CNN_REQUIRE(!(flags & CNNITMO_STATS) || stat_part, "conv3x3_fwd_cat: STATS without buffer");
  CNN_REQUIRE(!(flags & CNNITMO_AFFINE) || (aff_scale && aff_shift), "conv3x3_fwd_cat: AFFINE without coefficients");
  if (!is_bf16(dtype) || !halo_route(dtype, a).kernel) {
    cnnitmo_set_error("conv3x3_fwd_cat: unsupported (bf16 halo kernel, 32-channel aligned split, with an epilogue)");
    return CNNITMO_EUNSUPPORTED;
  }
  return launch_halo(a, (hipStream_t)stream, "conv3x3_fwd_cat");
}

extern "C" int cnnitmo_conv3x3_fwd_cat_supported(int dtype, int n, int h, int w, int c1, int cin, int cout) {
  if (!is_bf16(dtype) || c1 <= 0 || c1 >= cin) return 0;
  FwdArgs a = conv3x3_args(n, h, w, cin, cout);
  a.a = (const void*)16; a.a_ld = c1;
  a.a2 = (const void*)16; a.a2_ld = cin - c1; a.cin1 = c1;
  a.flags = CNNITMO_RELU;  // every U-Net conv has the forward epilogue
  return halo_route(dtype, a).kernel ? 1 : 0;
}

// Partial-sum rows cnnitmo_conv3x3_dgrad_bn writes (0: the fused path is not
// available for these sizes / dtype).
extern "C" long cnnitmo_conv3x3_dgrad_bn_rows(int dtype, int n, int h, int w, int cout, int cin, int c0,
                                              int c1) {
  return halo_route(dtype, dgrad_bn_args(n, h, w, cout, cin, c0, c1)).rows;
}

// Name of the kernel cnnitmo_conv3x3_dgrad_bn launches for these sizes (for profiles).
extern "C" const char* cnnitmo_conv3x3_dgrad_bn_kernel_name(int dtype, int n, int h, int w, int cout, int cin,
                                                            int c0, int c1) {
  const FwdArgs a = dgrad_bn_args(n, h, w, cout, cin, c0, c1);
  return route_name(halo_route(dtype, a), dtype, a);
}

extern "C" int cnnitmo_conv3x3_dgrad_bn(int dtype, const void* dz, int n, int h, int w, int cout,
                                        const void* wt_flip, int cin, void* dx, int dx_ld, int dx_off,
                                        int c0, int c1, const float* coef, const void* r, int r_ld,
                                        int r_off, void* dz_out, float* part, int parity, void* stream) {
  FwdArgs a = conv3x3_dgrad_args(n, h, w, cout, cin);
  a.a = dz; a.b = wt_flip;
  a.out = dx; a.out_ld = dx ? dx_ld : cin; a.out_off = dx ? dx_off : 0;
  a.bnb_c0 = c0; a.bnb_c1 = c1; a.bnb_par = parity ? 1 : 0;
  a.bnb_coef = coef; a.bnb_r = r; a.bnb_r_ld = r_ld; a.bnb_r_off = r_off; a.bnb_out = dz_out;
  a.stats = part;
  CNN_REQUIRE(halo_route(dtype, a).kernel, "conv3x3_dgrad_bn: unsupported sizes (halo kernel only)");
  CNN_REQUIRE(coef && r && dz_out && part && (dx || (c0 == 0 && c1 == cin)),
              "conv3x3_dgrad_bn: missing buffers");
  return launch_halo(a, (hipStream_t)stream, "conv3x3_dgrad_bn", is_f32(dtype));
}

// Partial-sum rows cnnitmo_conv3x3_dgrad_bn_pooled writes (0: not available for these sizes).
extern "C" long cnnitmo_conv3x3_dgrad_bn_pooled_rows(int dtype, int n, int h, int w, int cout, int cin) {
  return halo_route(dtype, dgrad_bn_pooled_args(n, h, w, cout, cin)).rows;
}

extern "C" const char* cnnitmo_conv3x3_dgrad_bn_pooled_kernel_name(int dtype, int n, int h, int w, int cout,
                                                                   int cin) {
  const FwdArgs a = dgrad_bn_pooled_args(n, h, w, cout, cin);
  return route_name(halo_route(dtype, a), dtype, a);
}

extern "C" int cnnitmo_conv3x3_dgrad_bn_pooled(int dtype, const void* dz, int n, int h, int w, int cout,
                                               const void* wt_flip, int cin, const float* coef, const void* r,
                                               int r_ld, int r_off, const void* dy_pool, const unsigned char* idx,
                                               void* dz_out, float* part, void* stream) {
  FwdArgs a = dgrad_bn_pooled_args(n, h, w, cout, cin);
  a.a = dz; a.b = wt_flip;
  a.out = dz_out; a.out_ld = cin; a.out_off = 0;
  a.bnb_coef = coef; a.bnb_r = r; a.bnb_r_ld = r_ld; a.bnb_r_off = r_off; a.bnb_out = dz_out;
  a.pool_out = const_cast<void*>(dy_pool); a.pool_idx = const_cast<unsigned char*>(idx);
  a.stats = part;
  CNN_REQUIRE(halo_route(dtype, a).kernel, "conv3x3_dgrad_bn_pooled: unsupported sizes (halo kernel, even h and w)");
  CNN_REQUIRE(coef && r && dy_pool && idx && dz_out && part, "conv3x3_dgrad_bn_pooled: missing buffers");
  return launch_halo(a, (hipStream_t)stream, "conv3x3_dgrad_bn_pooled", is_f32(dtype));
}

// ----------------------------------------------------------------------------
// Conv2DTranspose 2x2 stride 2 forward and input gradient
// ----------------------------------------------------------------------------
extern "C" long cnnitmo_tconv2x2_stat_rows(int dtype, int n, int h, int w, int cin, int cout) {
  FwdArgs a = tconv_fwd_args(n, h, w, cin, cout);
  a.flags = CNNITMO_RELU | CNNITMO_STATS;  // the training forward
  return tconv_route(dtype, 0, cin, cout, a).rows;
}

extern "C" const char* cnnitmo_tconv2x2_kernel_name(int dtype, int n, int h, int w, int cin, int cout,
                                                    int dgrad) {
  const int mode = dgrad ? 1 : 0;
  FwdArgs a = mode ? tconv_dgrad_args(n, h, w, cin, cout) : tconv_fwd_args(n, h, w, cin, cout);
  if (!mode) a.flags = CNNITMO_RELU | CNNITMO_STATS;  // the training forward
  const Route r = tconv_route(dtype, mode, cin, cout, a);
  switch (r.kernel) {
    case K_TSTREAM: return tconv_stream_name(mode, h, w, cin, cout, false);
    case K_TFWD2P: return "tconv_fwd2p_kernel<bf16,256x256>";
    case K_TWS: return tconv_ws_name(mode, cin, cout, is_f32(dtype));
    default: return route_name(r, dtype, a);
  }
}

extern "C" int cnnitmo_tconv2x2_fwd(int dtype, const void* x, int n, int h, int w, int cin,
                                    const void* k, const float* bias, int cout, void* out,
                                    int out_ld, int out_off, int flags, const float* aff_scale,
                                    const float* aff_shift, float* stat_part, void* stream) {
  FwdArgs a = tconv_fwd_args(n, h, w, cin, cout);
  a.a = x; a.b = k;
  a.bias = bias; a.out = out; a.out_ld = out_ld; a.out_off = out_off; a.flags = flags;
  a.aff_scale = aff_scale; a.aff_shift = aff_shift; a.stats = stat_part;
  CNN_REQUIRE(!(flags & CNNITMO_STATS) || stat_part, "tconv2x2_fwd: STATS without buffer");
  const Route r = tconv_route(dtype, 0, cin, cout, a);
  switch (r.kernel) {
    case K_TSTREAM:
      return launch_tconv_stream(0, x, cin, 0, k, n, h, w, cin, cout, out, out_ld, out_off, bias, flags, aff_scale,
                                 aff_shift, stat_part, nullptr, nullptr, 0, 0, (hipStream_t)stream, "tconv2x2_fwd");
    case K_TFWD2P: return launch_tfwd2p(a, (hipStream_t)stream, "tconv2x2_fwd");
    case K_TWS:
      return launch_tconv_ws(0, x, cin, 0, k, n, h, w, cin, cout, out, out_ld, out_off, bias, flags, aff_scale,
                             aff_shift, stat_part, (hipStream_t)stream, "tconv2x2_fwd", is_f32(dtype));
    default: return launch_route(r, dtype, a, stream, "tconv2x2_fwd");
  }
}

extern "C" int cnnitmo_tconv2x2_dgrad(int dtype, const void* dout, int n, int h, int w, int cout,
                                      const void* kT, int cin, void* dx, void* stream) {
  FwdArgs a = tconv_dgrad_args(n, h, w, cin, cout);
  a.a = dout; a.b = kT; a.out = dx;
  const Route r = tconv_route(dtype, 1, cin, cout, a);
  switch (r.kernel) {
    case K_TSTREAM:
      return launch_tconv_stream(1, dout, cout, 0, kT, n, h, w, cin, cout, dx, cin, 0, nullptr, 0, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, 0, 0, (hipStream_t)stream, "tconv2x2_dgrad");
    case K_TWS:
      return launch_tconv_ws(1, dout, cout, 0, kT, n, h, w, cin, cout, dx, cin, 0, nullptr, 0, nullptr, nullptr,
                             nullptr, (hipStream_t)stream, "tconv2x2_dgrad", is_f32(dtype));
    default: return launch_route(r, dtype, a, stream, "tconv2x2_dgrad");
  }
}

extern "C" long cnnitmo_tconv2x2_dgrad_bn_rows(int dtype, int n, int h, int w, int cout, int cin) {
  return tconv_bn_route(dtype, n, h, w, cout, cin).rows;
}

// Name of the kernel cnnitmo_tconv2x2_dgrad_bn launches for these sizes (for profiles).
extern "C" const char* cnnitmo_tconv2x2_dgrad_bn_kernel_name(int dtype, int n, int h, int w, int cout, int cin) {
  if (!tconv_bn_route(dtype, n, h, w, cout, cin).kernel) return "";
  return tconv_stream_name(1, h, w, cin, cout, true);
}

extern "C" int cnnitmo_tconv2x2_dgrad_bn(int dtype, const void* dout, int n, int h, int w, int cout,
                                         const void* kT, int cin, const float* coef, const void* r, int r_ld,
                                         int r_off, void* dz_out, float* part, void* stream) {
  CNN_REQUIRE(tconv_bn_route(dtype, n, h, w, cout, cin).kernel,
              "tconv2x2_dgrad_bn: unsupported sizes (bf16 stream kernel only)");
  CNN_REQUIRE(coef && r && dz_out && part, "tconv2x2_dgrad_bn: missing buffers");
  return launch_tconv_stream(1, dout, cout, 0, kT, n, h, w, cin, cout, dz_out, cin, 0, nullptr, 0, nullptr,
                             nullptr, part, coef, r, r_ld, r_off, (hipStream_t)stream, "tconv2x2_dgrad_bn");
}
