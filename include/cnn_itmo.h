/*
 * cnn_itmo.h -- C ABI of libcnnitmo.so, the MI355X (gfx950) kernels behind the
 * CNN-ITMO U-Net hot path.
 *
 * The reference (LynxHack/CNN-ITMO) reaches its arithmetic through the Keras
 * functional Layer API (Conv2D, Conv2DTranspose, MaxPooling2D,
 * BatchNormalization, Activation, Dropout, concatenate) at
 * /root/reference/model.py:195-281; TensorFlow/cuDNN execute it.  Each entry
 * point below replaces one of those layer calls (forward or its gradient); the
 * Python host side (cnn_itmo_amd/) mirrors the Keras API and calls these.
 *
 * Conventions
 *   - Every function is stateless, never allocates, and enqueues work on the
 *     given HIP stream (hipStream_t passed as void*).  Scratch memory is
 *     caller-owned; size it with the *_workspace_bytes / *_rows queries.
 *   - Return value: 0 = ok, negative = error (CNNITMO_E*);
 *     cnnitmo_last_error() returns a thread-local message.
 *   - The size queries (*_rows, *_workspace_bytes, *_supported, *_kernel_name) run
 *     on the host and need no GPU.  For sizes no launch takes (a channel count of 0
 *     or one that is no multiple of what the kernels need, no pixels) they answer
 *     0 rows, 0 bytes, 0 or "" -- the launch itself then returns CNNITMO_EINVAL.
 *   - dtype: CNNITMO_F32 (fp32 storage) or CNNITMO_BF16 (bf16 storage).
 *     Accumulation is always fp32 (MFMA f32 accumulators).
 *   - Activations are NHWC.  A "view" of an activation is (ptr, ld, off):
 *     element (p, c) of a P-pixel, C-channel view lives at ptr[p*ld + off + c].
 *     This is how channel concatenation (model.py:246,251,256,261) is zero-copy:
 *     producers write channel slices of one buffer.
 *   - Weight layouts: Conv2D OHWI [Cout][kh][kw][Cin]; Conv2DTranspose
 *     [2][2][Cout][Cin] (Keras' own kernel layout, layers.txt:78).  Master
 *     weights are fp32; cnnitmo_prep_* produce the dtype copies kernels read.
 *   - Per-channel fp32 vectors (bias, BN gamma/beta/stats) are always fp32.
 */
#ifndef CNN_ITMO_H_
#define CNN_ITMO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNNITMO_F32 0
#define CNNITMO_BF16 1

#define CNNITMO_OK 0
#define CNNITMO_EINVAL (-1)
#define CNNITMO_EUNSUPPORTED (-2)
#define CNNITMO_ELAUNCH (-3)

/* Epilogue flags for the forward convolutions. */
#define CNNITMO_RELU 1   /* Activation('relu') after the conv (model.py:196,200) */
#define CNNITMO_STATS 2  /* write per-tile BN partial sums (sum, sum of squares) */
#define CNNITMO_AFFINE 4 /* y = v*scale[c] + shift[c] after ReLU (inference BN) */
#define CNNITMO_BIAS_PER_COL 8 /* bias indexed by GEMM column (tconv: [4*cout], folded BN) */

/* Flags for BN apply / backward. */
#define CNNITMO_DROPOUT 1 /* Dropout(0.5), model.py:226,239 (train only) */
#define CNNITMO_NO_BN 2   /* bwd: plain ReLU gradient, no BN (config-1 net)  */
#define CNNITMO_PARITY 4  /* bwd apply: bias partials split by (h&1, w&1) -> [4][c] */

/* ABI version: 2 since CNNITMO_CONSUMER_ROWS went from 16 to 64 (a caller built against the
 * old header under-allocates cnnitmo_bn_consumer_sums' part: check cnnitmo_consumer_rows()) and
 * cnnitmo_bn_apply started to require 16-byte aligned scale / shift.  Added since without a bump
 * (new entry points only, nothing existing changed): cnnitmo_rgbe_encode / cnnitmo_rgbe_decode,
 * cnnitmo_hdr_pairs / cnnitmo_hdr_pairs_workspace_bytes, cnnitmo_hdr_encode,
 * cnnitmo_lum_percentile / cnnitmo_lum_percentile_workspace_bytes,
 * cnnitmo_grad_sumsq / cnnitmo_grad_sumsq_workspace_bytes / cnnitmo_grad_clip,
 * cnnitmo_jpeg_roundtrip / cnnitmo_jpeg_workspace_bytes,
 * cnnitmo_resize / cnnitmo_resize_coeffs / cnnitmo_resize_workspace_bytes / cnnitmo_resize_tile_cols,
 * cnnitmo_exr_unpack / cnnitmo_exr_pack / cnnitmo_exr_workspace_bytes / cnnitmo_exr_segment_bytes,
 * cnnitmo_hdr_pairs_sensor / cnnitmo_sensor_noise (and CNNITMO_CURVE_PER_CHANNEL on curve 1 of
 * cnnitmo_tonemap_apply, a value refused before). */
int cnnitmo_version(void);
const char* cnnitmo_last_error(void);

/* ---------------------------------------------------------------------------
 * Conv2D(f, 3, padding='same') -- replaces Conv2D at model.py:196 (via ConvBN).
 * x view: [n, h, w, cin] (ld, off); wt: [cout][3][3][cin] in dtype.
 * out view: [n, h, w, cout] (ld, off).  flags: CNNITMO_RELU|STATS|AFFINE.
 * stat_part (STATS): [rows][2][cout] fp32, rows = cnnitmo_fwd_stat_rows(...).
 * aff_scale/aff_shift (AFFINE): [cout] fp32.
 * border (nullable): [cout][8] zero-padding correction of a folded input BN
 * (cnnitmo_fold_conv3x3): when x holds r and the conv's true input is
 * y = r*s + h, pass wt/bias/border from the fold.
 * Requires cin % 32 == 0 (bf16) or % 16 == 0 (f32), cout % 32 == 0.
 */
int cnnitmo_conv3x3_fwd(int dtype, const void* x, int x_ld, int x_off, int n, int h, int w,
                        int cin, const void* wt, const float* bias, int cout, void* out,
                        int out_ld, int out_off, int flags, const float* aff_scale,
                        const float* aff_shift, float* stat_part, const float* border,
                        void* stream);

/* conv3x3_fwd with the 2x2 MaxPooling2D of its output fused into the epilogue
 * (model.py:209-210, 214-215, 219-220: ConvBN -> MaxPooling2D).  pool_out
 * [n, h/2, w/2] x pool_ld (dtype) gets the pooled stored value, pool_idx (same layout,
 * bytes) its window index (first maximum in window order (0,0),(0,1),(1,0),(1,1), the
 * cnnitmo_maxpool2x2_fwd rule).  pool_sign [cout] (nullable): per channel, pool by the
 * maximum (> 0), the minimum (< 0) or take the first element (0) of the stored values:
 * with the output stored as r and the BN folded into the consumers, sign(gamma) makes
 * s * pooled + h the max-pool of y = r * s + h (s = gamma * invstd).  Requires even h, w
 * and the halo kernel (cnnitmo_conv3x3_pool_supported). */
int cnnitmo_conv3x3_fwd_pool(int dtype, const void* x, int x_ld, int x_off, int n, int h, int w, int cin,
                             const void* wt, const float* bias, int cout, void* out, int out_ld, int out_off,
                             int flags, const float* aff_scale, const float* aff_shift, float* stat_part,
                             const float* border, void* pool_out, int pool_ld, unsigned char* pool_idx,
                             const float* pool_sign, void* stream);
/* The last 3x3 ConvBN (conv9 = ConvBN(64, 3, merge9), model.py:262) with the sigmoid head
 * (model.py:276, Conv2D(3, 1, activation='sigmoid')) in its epilogue, for inference
 * (predict.py:62): yhat [n][h_valid][w][3] fp32 = sigmoid(y . head_w[3][cout] + head_b), y = the
 * conv's epilogue output (flags/aff as cnnitmo_conv3x3_fwd: ReLU, BN affine), never stored.
 * Replaces cnnitmo_conv3x3_fwd + cnnitmo_head_fwd.  cout = 64; no BN sums. */
int cnnitmo_conv3x3_fwd_head(int dtype, const void* x, int x_ld, int x_off, int n, int h, int w, int cin,
                             const void* wt, const float* bias, int cout, int flags, const float* aff_scale,
                             const float* aff_shift, int h_valid, const float* head_w, const float* head_b,
                             float* yhat, void* stream);
int cnnitmo_conv3x3_head_supported(int dtype, int n, int h, int w, int cin, int cout);
int cnnitmo_conv3x3_pool_supported(int dtype, int n, int h, int w, int cin, int cout);

/* conv3x3_fwd over concatenate([x1, x2]) (model.py:261, Keras axis=3) read from its
 * two members, without a concat buffer: input channels [0, c1) are x1's view
 * (x1_ld, x1_off), channels [c1, cin) are x2's (x2_ld, x2_off).  bf16 only, c1 % 32 == 0,
 * an epilogue (flags / bias / stats) required; CNNITMO_EUNSUPPORTED otherwise.  Used for
 * the level-0 concat [conv1 32 | up9 64], whose members each occupy partial 128-B lines
 * of a 192-B concat row. */
int cnnitmo_conv3x3_fwd_cat(int dtype, const void* x1, int x1_ld, int x1_off, int c1, const void* x2,
                            int x2_ld, int x2_off, int n, int h, int w, int cin, const void* wt,
                            const float* bias, int cout, void* out, int out_ld, int out_off, int flags,
                            const float* aff_scale, const float* aff_shift, float* stat_part,
                            const float* border, void* stream);
/* 1 if cnnitmo_conv3x3_fwd_cat runs for these sizes in this process (dtype, the
 * channel split, CNNITMO_HALO and the device's workgroup count decide), else 0: a
 * planner must not keep a concat split into members the forward cannot read. */
int cnnitmo_conv3x3_fwd_cat_supported(int dtype, int n, int h, int w, int c1, int cin, int cout);

/* Name of the kernel conv3x3_fwd (dgrad = 0) / conv3x3_dgrad (dgrad = 1, same
 * layer cin/cout) launches for these sizes (profiling labels; no GPU needed). */
const char* cnnitmo_conv3x3_kernel_name(int dtype, int n, int h, int w, int cin, int cout,
                                        int dgrad);
/* Same for tconv2x2_fwd / _dgrad over an n x h x w input grid. */
const char* cnnitmo_tconv2x2_kernel_name(int dtype, int n, int h, int w, int cin, int cout,
                                         int dgrad);

/* Rows of the BN partial-sum buffer written by a forward conv over m output
 * pixels with ncols GEMM columns (4*cout for tconv2x2; the 1-tap first layer).
 * conv3x3: use cnnitmo_conv3x3_stat_rows (the row count depends on the frame). */
int cnnitmo_fwd_stat_rows(int dtype, long m, int ncols);
long cnnitmo_conv3x3_stat_rows(int dtype, int n, int h, int w, int cin, int cout);
/* Same for cnnitmo_tconv2x2_fwd over an n x h x w input grid (columns 4*cout). */
long cnnitmo_tconv2x2_stat_rows(int dtype, int n, int h, int w, int cin, int cout);

/* Input-gradient of conv3x3 (TF Conv2DBackpropInput).  dz: [n,h,w,cout]
 * contiguous; wt_flip: [cin][3][3][cout] = W[co][2-r][2-s][ci] (from
 * cnnitmo_prep_conv3x3_weights).  dx view [n,h,w,cin] (ld, off) is OVERWRITTEN. */
int cnnitmo_conv3x3_dgrad(int dtype, const void* dz, int n, int h, int w, int cout,
                          const void* wt_flip, int cin, void* dx, int dx_ld, int dx_off,
                          void* stream);
/* conv3x3_dgrad with the PRODUCER's BN backward fused into its store (bf16):
 * input-gradient columns [c0, c1) are the gradient g of a folded BN output
 * whose backward coefficients coef [3][c1-c0] (cnnitmo_bn_bwd_finalize) are
 * already known (consumer-derived sums); they are written as the producer's
 * dz = [r>0]*(a*g - b*r + e) to dz_out [n*h*w][c1-c0] (r: the producer's saved
 * view, element (p, j) at r[p*r_ld + r_off + j]) together with column-sum
 * partials part [rows][parity ? 4 : 1][c1-c0] (rows =
 * cnnitmo_conv3x3_dgrad_bn_rows; parity splits by (h&1, w&1) like
 * CNNITMO_PARITY).  Columns outside [c0, c1) go to dx as in conv3x3_dgrad (dx
 * may be NULL when [c0, c1) = [0, cin)).  Replaces conv3x3_dgrad +
 * cnnitmo_bn_bwd_apply.  rows = 0: not available for these sizes. */
long cnnitmo_conv3x3_dgrad_bn_rows(int dtype, int n, int h, int w, int cout, int cin, int c0, int c1);
int cnnitmo_conv3x3_dgrad_bn(int dtype, const void* dz, int n, int h, int w, int cout,
                             const void* wt_flip, int cin, void* dx, int dx_ld, int dx_off, int c0,
                             int c1, const float* coef, const void* r, int r_ld, int r_off,
                             void* dz_out, float* part, int parity, void* stream);
/* Label of the kernel cnnitmo_conv3x3_dgrad_bn launches ("" = unavailable; profiling only). */
const char* cnnitmo_conv3x3_dgrad_bn_kernel_name(int dtype, int n, int h, int w, int cout, int cin,
                                                 int c0, int c1);
/* The skip path of a concatenate whose other reader is a MaxPooling2D(2) (model.py:209-211
 * + 261: conv1 feeds pool1 and merge9): the input-gradient of the concat-consuming conv
 * for the skip member's cin channels (wt_flip: its rows [cin][3][3][cout] of the flipped
 * weights), PLUS the pool's gradient dy_pool [n,h/2,w/2,cin] (dense) routed to the window
 * position idx [n,h/2,w/2,cin] (bytes, first-max index in window order, as
 * cnnitmo_maxpool2x2_fwd / _fwd_pool write them), through the producer's BN backward:
 * dz_out [n*h*w][cin] = [r>0]*(a*(bf16(g) + routed) - b*r + e), column-sum partials part
 * [rows][cin] (rows = cnnitmo_conv3x3_dgrad_bn_pooled_rows; 0: unavailable).  h, w even.
 * Replaces conv3x3_dgrad + cnnitmo_bn_bwd_apply_pooled (the skip gradient is never
 * stored). */
long cnnitmo_conv3x3_dgrad_bn_pooled_rows(int dtype, int n, int h, int w, int cout, int cin);
int cnnitmo_conv3x3_dgrad_bn_pooled(int dtype, const void* dz, int n, int h, int w, int cout,
                                    const void* wt_flip, int cin, const float* coef, const void* r, int r_ld,
                                    int r_off, const void* dy_pool, const unsigned char* idx, void* dz_out,
                                    float* part, void* stream);
const char* cnnitmo_conv3x3_dgrad_bn_pooled_kernel_name(int dtype, int n, int h, int w, int cout, int cin);

/* Weight-gradient of conv3x3 (TF Conv2DBackpropFilter).  x view [n,h,w,cin];
 * dz [n,h,w,cout] contiguous; dw: [cout][3][3][cin] fp32, OVERWRITTEN.
 * ntaps = 9 for the 3x3 conv, 1 for a 1x1 / pre-packed (im2col) input. */
size_t cnnitmo_wgrad_workspace_bytes(int dtype, int n, int h, int w, int cin, int cout,
                                     int ntaps);
/* Label of the main kernel a weight gradient launches for these sizes (ntaps 9 /
 * 1: conv, 4: tconv2x2; profiling only, no GPU needed). */
const char* cnnitmo_wgrad_kernel_name(int dtype, int ntaps, int n, int h, int w, int cin, int cout);
int cnnitmo_conv_wgrad(int dtype, int ntaps, const void* x, int x_ld, int x_off,
                       const void* dz, int n, int h, int w, int cin, int cout, float* dw,
                       int dw_cols, const float* fold_scale, const float* fold_shift,
                       const float* fold_db, const float* fold_border, float* raw_out,
                       void* workspace, size_t ws_bytes, void* stream);
/* Folded input BN (x holds r, the conv's input is y = r*s + h, see
 * cnnitmo_fold_conv3x3): pass fold_scale = s, fold_shift = h [cin], fold_db = the
 * bias gradient [cout] and fold_border = the reduced border sums [8][cout] of dz
 * (cnnitmo_border_sums + cnnitmo_colsum); dw is then the exact gradient w.r.t. W.
 * All four NULL: plain weight gradient.  raw_out (nullable, same layout as dw):
 * the uncorrected sum dz (x) r, input of cnnitmo_bn_consumer_sums. */

/* cnnitmo_conv_wgrad (ntaps 9, bf16) over concatenate([x1, x2]) read from its members
 * (see cnnitmo_conv3x3_fwd_cat): c1 == 32, cin == 96 (merge9 -> conv9, model.py:261-262).
 * workspace: cnnitmo_wgrad_cat_workspace_bytes (0 = unsupported sizes). */
size_t cnnitmo_wgrad_cat_workspace_bytes(int n, int h, int w, int c1, int cin, int cout);
const char* cnnitmo_wgrad_cat_kernel_name(int n, int h, int w, int c1, int cin, int cout);
int cnnitmo_conv_wgrad_cat(int dtype, const void* x1, int x1_ld, int x1_off, int c1, const void* x2, int x2_ld,
                           int x2_off, const void* dz, int n, int h, int w, int cin, int cout, float* dw,
                           const float* fold_scale, const float* fold_shift, const float* fold_db,
                           const float* fold_border, float* raw_out, void* workspace, size_t ws_bytes,
                           void* stream);

/* First layer (Cin=3): pack x [n,h_valid,w,3] fp32 into [n,h,w,32] dtype
 * columns k=(r*3+s)*3+c (k<27, zero pad; rows >= h_valid are zero), so that
 * conv2d_1 runs as a 1-tap GEMM with K=32.  Fuses the /255 input's cast and
 * the pad-to-multiple-of-16 of predict.py:59 / SURVEY 8a. */
int cnnitmo_im2col_c3(int dtype, const float* x, int n, int h_valid, int h, int w, void* cols,
                      void* stream);
/* 1-tap GEMM forward over packed columns: out = cols[m][k] * wt[cout][k]. */
int cnnitmo_conv1tap_fwd(int dtype, const void* cols, int k, long m, const void* wt,
                         const float* bias, int cout, void* out, int out_ld, int out_off,
                         int flags, const float* aff_scale, const float* aff_shift,
                         float* stat_part, void* stream);

/* First layer without im2col: x [n,h_valid,w,3] fp32 -> out view [n,h,w,32] in dtype
 * (bf16 or fp32; ld, off), rows >= h_valid of the input read as zero (pad-to-16).  wt:
 * [32][32] packed columns in dtype (cnnitmo_prep_c3_weights); flags/aff as conv3x3_fwd;
 * stat_part [rows][2][32] with rows = cnnitmo_conv_c3_stat_rows.  Replaces
 * cnnitmo_im2col_c3 + cnnitmo_conv1tap_fwd for model.py:208. */
long cnnitmo_conv_c3_stat_rows(int n, int h, int w);
int cnnitmo_conv_c3_fwd(int dtype, const float* x, int n, int h_valid, int h, int w, const void* wt,
                        const float* bias, void* out, int out_ld, int out_off, int flags,
                        const float* aff_scale, const float* aff_shift, float* stat_part, void* stream);
/* dw [32][27] fp32 (OVERWRITTEN; OHWI) = sum_p dz[p][co] * patch(x, p)[k], dz [n*h*w][32]
 * in dtype (bf16 or fp32) contiguous.  Replaces cnnitmo_conv_wgrad(ntaps = 1) over im2col
 * columns. */
size_t cnnitmo_conv_c3_wgrad_workspace_bytes(int n, int h, int w);
int cnnitmo_conv_c3_wgrad(int dtype, const float* x, int n, int h_valid, int h, int w, const void* dz,
                          float* dw, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Conv2DTranspose(f, 2, strides=2, 'valid') -- replaces model.py:200
 * (ConvBNTranspose).  x [n,h,w,cin] contiguous; k: [2][2][cout][cin] dtype;
 * out view [n,2h,2w,cout] (ld, off); flags/stat_part as conv3x3 (stat_part
 * columns are [4*cout] = (tap, channel) groups; only a channel's total over the
 * four groups is defined: cnnitmo_bn_fwd_finalize with groups = 4 folds them).
 */
int cnnitmo_tconv2x2_fwd(int dtype, const void* x, int n, int h, int w, int cin, const void* k,
                         const float* bias, int cout, void* out, int out_ld, int out_off,
                         int flags, const float* aff_scale, const float* aff_shift,
                         float* stat_part, void* stream);
/* dx [n,h,w,cin] (contiguous, OVERWRITTEN) from dout [n,2h,2w,cout] and
 * kT: [cin][2][2][cout] (from cnnitmo_prep_tconv2x2_weights). */
int cnnitmo_tconv2x2_dgrad(int dtype, const void* dout, int n, int h, int w, int cout,
                           const void* kT, int cin, void* dx, void* stream);
/* tconv2x2_dgrad with the PRODUCER's BN backward fused into its store (bf16;
 * the tconv input is a folded BN output whose coefficients coef [3][cin] are
 * known): dz_out [n*h*w][cin] = [r>0]*(a*g - b*r + e) of the input gradient g,
 * r the producer's saved view (element (p, c) at r[p*r_ld + r_off + c]), and
 * column-sum partials part [rows][cin] (rows = cnnitmo_tconv2x2_dgrad_bn_rows;
 * 0 = not available for these sizes).  Replaces tconv2x2_dgrad + bn_bwd_apply. */
long cnnitmo_tconv2x2_dgrad_bn_rows(int dtype, int n, int h, int w, int cout, int cin);
int cnnitmo_tconv2x2_dgrad_bn(int dtype, const void* dout, int n, int h, int w, int cout,
                              const void* kT, int cin, const float* coef, const void* r, int r_ld,
                              int r_off, void* dz_out, float* part, void* stream);
/* Label of the kernel cnnitmo_tconv2x2_dgrad_bn launches ("" = unavailable; profiling only). */
const char* cnnitmo_tconv2x2_dgrad_bn_kernel_name(int dtype, int n, int h, int w, int cout, int cin);
/* dk [2][2][cout][cin] fp32 (OVERWRITTEN) from x [n,h,w,cin], dout [n,2h,2w,cout]. */
int cnnitmo_tconv2x2_wgrad(int dtype, const void* x, const void* dout, int n, int h, int w,
                           int cin, int cout, float* dk, const float* fold_scale,
                           const float* fold_shift, const float* fold_par, float* raw_out,
                           void* workspace, size_t ws_bytes, void* stream);
/* fold_par: per-tap sums of dout [4][cout] (cnnitmo_bn_bwd_apply with
 * CNNITMO_PARITY, reduced by cnnitmo_colsum); NULL trio = plain gradient. */
size_t cnnitmo_tconv2x2_wgrad_workspace_bytes(int dtype, int n, int h, int w, int cin, int cout);

/* Weight preparation (after every optimizer step): fp32 master -> dtype copies.
 * conv3x3: w [cout][3][3][cin] -> w_fwd (same layout), w_flip [cin][3][3][cout].
 * w_flip may be NULL (first layer).  tconv: k [2][2][cout][cin] -> k_fwd (same),
 * kT [cin][2][2][cout].  pack_c3: w [32][3][3][3] -> [32][32] zero-padded. */
int cnnitmo_prep_conv3x3_weights(int dtype, const float* w, int cout, int cin, void* w_fwd,
                                 void* w_flip, void* stream);
int cnnitmo_prep_tconv2x2_weights(int dtype, const float* k, int cout, int cin, void* k_fwd,
                                  void* kT, void* stream);
int cnnitmo_prep_c3_weights(int dtype, const float* w, int cout, void* w_packed, void* stream);

/* BN folding (training): the consumer of a BN output y = r*s + h reads the
 * stored post-ReLU r and folds the affine into its own weights instead of
 * materialising y (removes one full read+write of every activation).
 * conv3x3: w_out = W*s (dtype), bias_out[cout] = b + sum_t u_t and border[cout][8]
 *   (u_t[co] = sum_ci W[co][t][ci]*h[ci]) for cnnitmo_conv3x3_fwd's border.
 * tconv2x2: k_out = K*s, bias_out[4*cout] per (tap, co) -> CNNITMO_BIAS_PER_COL.
 * scale/shift NULL = identity. */
int cnnitmo_fold_conv3x3(int dtype, const float* w, const float* bias, const float* scale,
                         const float* shift, int cout, int cin, void* w_out, float* bias_out,
                         float* border, void* stream);
int cnnitmo_fold_tconv2x2(int dtype, const float* k, const float* bias, const float* scale,
                          const float* shift, int cout, int cin, void* k_out, float* bias_out,
                          void* stream);
/* Border partial sums of dz [n,h,w,c] (contiguous): rows cnnitmo_border_rows(n)
 * of [8][c] = {row 0, row h-1, col 0, col w-1, 4 corners}; reduce with cnnitmo_colsum. */
int cnnitmo_border_rows(int n);
int cnnitmo_border_sums(int dtype, const void* dz, int n, int h, int w, int c, float* part,
                        void* stream);

/* ---------------------------------------------------------------------------
 * MaxPooling2D(pool_size=(2,2), strides=2) -- model.py:210,215,220,227.
 * fwd: x view [n,h,w,c] -> y [n,h/2,w/2,c] contiguous + argmax idx uint8 (0..3,
 * first maximum in row-major window order).
 * bwd: dx view [n,h,w,c] += scatter of dy to the argmax (other entries untouched).
 */
int cnnitmo_maxpool2x2_fwd(int dtype, const void* x, int x_ld, int x_off, int n, int h, int w,
                           int c, void* y, uint8_t* idx, const float* scale, const float* shift,
                           void* stream);
/* scale/shift (nullable, [c]): pool over x*scale + shift (a folded BN output). */
int cnnitmo_maxpool2x2_bwd(int dtype, const void* dy, const uint8_t* idx, int n, int h, int w,
                           int c, void* dx, int dx_ld, int dx_off, void* stream);

/* ---------------------------------------------------------------------------
 * BatchNormalization() (axis=-1, eps 1e-3, momentum 0.99) -- model.py:196,200.
 * Training forward: the conv epilogue writes r = relu(conv) and partial sums;
 * cnnitmo_bn_fwd_finalize reduces them (fp64) to batch mean / biased variance,
 * produces scale = gamma*invstd, shift = beta - mean*scale, saves mean/invstd for
 * backward and updates the moving statistics (Keras-2.2: var *= n/(n-(1+eps))).
 * groups: the stat_part columns are [groups][c] (4 for a tconv, else 1).
 * workspace: cnnitmo_reduce_workspace_bytes(rows, groups*c*2).
 */
size_t cnnitmo_reduce_workspace_bytes(long rows, int cols);
int cnnitmo_bn_fwd_finalize(const float* stat_part, long rows, int c, int groups, double count,
                            const float* gamma, const float* beta, float* moving_mean,
                            float* moving_var, float momentum, float eps, float* scale,
                            float* shift, float* save_mean, float* save_invstd,
                            void* workspace, void* stream);
/* Inference-mode coefficients from the moving statistics. */
int cnnitmo_bn_infer_coeffs(int c, const float* gamma, const float* beta, const float* mmean,
                            const float* mvar, float eps, float* scale, float* shift,
                            void* stream);
/* y view = r*scale + shift (optionally Dropout(0.5): element (p,c) kept iff the
 * counter hash of (seed, layer, p*c_total + c) says so, kept values x2).  scale and shift
 * must be 16-byte aligned (CNNITMO_EINVAL otherwise; since cnnitmo_version() 2). */
int cnnitmo_bn_apply(int dtype, const void* r, long p, int c, const float* scale,
                     const float* shift, void* y, int y_ld, int y_off, int flags,
                     uint64_t drop_seed, int drop_layer, void* stream);
/* Backward.  dy view (ld, off) is the gradient w.r.t. the BN (or dropout)
 * output; r is the saved post-ReLU tensor [p][c].
 * Step 1 (reduce+finalize): dgamma, dbeta (written, fp32) and the three dz
 * coefficients.  Step 2 (apply): dz = [r>0]*(a*dy' - b*r + e) -> dz [p][c] and
 * the bias gradient db (written).  With CNNITMO_NO_BN: dz = [r>0]*dy. */
int cnnitmo_bn_bwd_rows(long p, int c);
int cnnitmo_bn_bwd_reduce(int dtype, const void* dy, int dy_ld, int dy_off, const void* r,
                          int r_ld, int r_off, long p, int c, const float* mean,
                          const float* invstd, int flags,
                          uint64_t drop_seed, int drop_layer, float* part, void* stream);
int cnnitmo_bn_bwd_finalize(const float* part, long rows, int c, double count,
                            const float* gamma, const float* mean, const float* invstd,
                            float* dgamma, float* dbeta, float* coef, void* workspace,
                            void* stream);
int cnnitmo_bn_bwd_apply(int dtype, const void* dy, int dy_ld, int dy_off, const void* r,
                         int r_ld, int r_off, long p, int c, const float* coef, int flags,
                         uint64_t drop_seed, int drop_layer, int h, int w, void* dz, float* part,
                         void* stream);
/* r view: (r_ld, r_off).  part columns: [c], or [4][c] by pixel parity with
 * CNNITMO_PARITY (h, w = the spatial size, needed only then). */
/* The same for a BN output that also feeds a MaxPooling2D whose backward was
 * deferred: dy += the pool gradient dy_pool [n][h/2][w/2][c] routed by idx to
 * this pixel (replaces cnnitmo_maxpool2x2_bwd + the dy read-modify-write). */
int cnnitmo_bn_bwd_apply_pooled(int dtype, const void* dy, int dy_ld, int dy_off, const void* r,
                                int r_ld, int r_off, int n, int h, int w, int c, const float* coef,
                                const void* dy_pool, const uint8_t* idx, void* dz, float* part,
                                void* stream);
/* The same for the BN output consumed by the sigmoid head: dy is never stored;
 * dy[p][c] = sum_o g3[p][o] * wh[o][c] is formed in fp32 from the head's per-pixel
 * output gradient g3 [p][3] (cnnitmo_head_fwd_bwd_g3) and its weights wh [3][c]
 * (12 B per pixel read instead of 2*c). */
int cnnitmo_bn_bwd_apply_g3(int dtype, const float* g3, const float* wh, const void* r, int r_ld, int r_off,
                            long p, int c, const float* coef, void* dz, float* part, void* stream);
/* BN-backward sums WITHOUT a pass over dy: for a BN output whose gradient is the
 * input-gradient of a linear consumer (mode 1 conv3x3, 2 tconv2x2, 3 the 1x1
 * head), part[2][c] = {sum dy, sum dy*rhat} over the consumer's input channels
 * [ci0, ci0+c) from its weights w, its uncorrected weight-gradient raw (raw_out of
 * the *_wgrad / head_finalize call) and V (mode 1: db[cout] + border sums
 * vtab[8][cout]; mode 2: parity sums vtab[4*cout]; mode 3: db[3]).  Exact: the
 * dgrad is the transpose of the same map.  Feed to cnnitmo_bn_bwd_finalize.
 * part has CNNITMO_CONSUMER_ROWS rows [rows][2][c].  cnnitmo_pool_bnsums adds a
 * MaxPooling2D consumer's share (dyp: the pooled gradient; r: the pool input's
 * view; rows = cnnitmo_bn_bwd_rows(n*(h/2)*(w/2), c)). */
#define CNNITMO_CONSUMER_ROWS 64
/* The row count the library was built with (== CNNITMO_CONSUMER_ROWS of this header; 16 before
 * cnnitmo_version() 2): size part from this at run time. */
int cnnitmo_consumer_rows(void);
int cnnitmo_bn_consumer_sums(int mode, const float* w, const float* raw, int cout, int cin_tot, int ci0,
                             int c, const float* db, const float* vtab, const float* mean,
                             const float* invstd, float* part, void* stream);
int cnnitmo_pool_bnsums(int dtype, const void* dyp, const uint8_t* idx, int n, int h, int w, int c,
                        const void* r, int r_ld, int r_off, const float* mean, const float* invstd,
                        float* part, void* stream);
/* The same share when the pool was fused into the producer (cnnitmo_conv3x3_fwd_pool):
 * pr [n, h/2, w/2, c] dense is r at each window's index, so no window is read. */
int cnnitmo_pool_bnsums_pooled(int dtype, const void* dyp, const void* pr, int n, int h, int w, int c,
                               const float* mean, const float* invstd, float* part, void* stream);
/* Column sums of partial rows -> out[groups-folded c] (fp32, written). */
int cnnitmo_colsum(const float* part, long rows, int cols, int groups, float* out,
                   void* workspace, void* stream);

/* ---------------------------------------------------------------------------
 * Head: Conv2D(3, 1, activation='sigmoid') + MSE loss + 'accuracy'
 * (model.py:276,281).  x [p][64-ish cin] dtype; w [3][cin] fp32, b [3].
 * fwd: yhat [n,h,w,3] fp32 for rows < h_valid (predict.py:62).
 * fwd_bwd: target [n,h_valid,w,3] fp32; writes dx [p][cin] dtype
 * (= dz * W), and partials (loss sum, correct count, dW, db) into part;
 * cnnitmo_head_finalize reduces them into loss, acc, dw, db.
 * grad_numel: the element count the MSE gradient is normalised by (<= 0: this
 * batch's n*h_valid*w*3, i.e. the gradient of its mean).  Data parallel with
 * unequal shares: global_frames*h_valid*w*3/world, so that the all-reduced mean
 * of the ranks' gradients is the gradient of the GLOBAL batch mean (the loss
 * partials are unaffected). */
int cnnitmo_head_fwd(int dtype, const void* x, int n, int h, int h_valid, int w, int cin,
                     const float* wt, const float* b, const float* scale, const float* shift,
                     float* yhat, void* stream);
int cnnitmo_head_rows(long p);
int cnnitmo_head_fwd_bwd(int dtype, const void* x, int n, int h, int h_valid, int w, int cin,
                         const float* wt, const float* b, const float* scale,
                         const float* shift, const float* target, void* dx, float* part,
                         double grad_numel, void* stream);
/* As cnnitmo_head_fwd_bwd, but the input gradient leaves as its rank-3 factor
 * g3 [p][3] fp32 = dL/dz of the head (dx = g3 * W; see cnnitmo_bn_bwd_apply_g3). */
int cnnitmo_head_fwd_bwd_g3(int dtype, const void* x, int n, int h, int h_valid, int w, int cin,
                            const float* wt, const float* b, const float* scale, const float* shift,
                            const float* target, float* g3, float* part, double grad_numel, void* stream);
int cnnitmo_head_finalize(const float* part, long rows, int cin, double numel,
                          const float* scale, const float* shift, float* loss_acc, float* dw,
                          float* db, float* raw_out, void* workspace, void* stream);
/* scale/shift (nullable, [cin]): x holds r and the head's input is r*scale +
 * shift (folded BN); dx is then d/dy and dw the gradient w.r.t. the raw W. */

/* The training loss as a parameter: the mean over n*h_valid*w*3 elements of the term l,
 * with y = sigmoid(z), t the target, evaluated in fp32:
 *   CNNITMO_LOSS_MSE      l = (y-t)^2                                dl/dz = 2(y-t) y(1-y)
 *   CNNITMO_LOSS_MAE      l = |y-t|                                  sign(y-t) y(1-y), sign(0) = 0
 *   CNNITMO_LOSS_LOGCOSH  l = |x| + log1p(exp(-2|x|)) - ln 2, x=y-t  tanh(x) y(1-y)
 *                         (= ln cosh x; Keras' x + softplus(-2x) - ln 2)
 *   CNNITMO_LOSS_MSLE     l = (a-b)^2, a = ln(max(y,1e-7)+1),        2(a-b)/(y+1) y(1-y) for y >= 1e-7,
 *                         b = ln(max(t,1e-7)+1)                      else 0
 *   CNNITMO_LOSS_BCE      l = max(z,0) - z t + log1p(exp(-|z|))      y - t
 * BCE is computed from the logit z itself.  Keras clips y to [1e-7, 1-1e-7] and converts it
 * back to a logit first; the two agree for |z| < 16.1 and differ beyond (no clipping here).
 * Exactly one of dx (as cnnitmo_head_fwd_bwd) and g3 (as cnnitmo_head_fwd_bwd_g3) is non-null;
 * an unknown loss or a bad dx/g3 pair is CNNITMO_EINVAL before any launch.  'accuracy', db, dW,
 * the part layout and cnnitmo_head_finalize are the same for every loss;
 * cnnitmo_head_fwd_bwd[_g3] are this call with CNNITMO_LOSS_MSE. */
#define CNNITMO_LOSS_MSE 0
#define CNNITMO_LOSS_MAE 1
#define CNNITMO_LOSS_LOGCOSH 2
#define CNNITMO_LOSS_MSLE 3
#define CNNITMO_LOSS_BCE 4
int cnnitmo_head_fwd_bwd_loss(int loss, int dtype, const void* x, int n, int h, int h_valid, int w, int cin,
                              const float* wt, const float* b, const float* scale, const float* shift,
                              const float* target, void* dx /*nullable*/, float* g3 /*nullable*/,
                              float* part, double grad_numel, void* stream);
/* The same call with the loss gradient given from outside: dy [n][h_valid][w][3] fp32 =
 * dL/dyhat, already normalised (no grad_numel), e.g. cnnitmo_dssim_loss_grad's.
 * dl/dz = dy * y(1-y); the loss slot of part (and of cnnitmo_head_finalize) is 0, 'accuracy'
 * comes from target as for every other loss; dx / g3, dW, db and the part layout are the
 * same.  CNNITMO_LOSS_GIVEN is refused by cnnitmo_head_fwd_bwd_loss, which has no dy. */
#define CNNITMO_LOSS_GIVEN 5
int cnnitmo_head_fwd_bwd_given(int dtype, const void* x, int n, int h, int h_valid, int w, int cin,
                               const float* wt, const float* b, const float* scale, const float* shift,
                               const float* target, const float* dy, void* dx /*nullable*/,
                               float* g3 /*nullable*/, float* part, void* stream);

/* ---------------------------------------------------------------------------
 * RMSprop (keras.optimizers.RMSprop defaults via compile('rmsprop'), model.py:281):
 *   a <- rho*a + (1-rho)*g'^2 ; p <- p - lr*g'/(sqrt(a)+eps),  g' = g*grad_scale
 * over one flat fp32 buffer holding every trainable tensor (multi-tensor apply).
 */
int cnnitmo_rmsprop(float* p, const float* g, float* a, long n, float lr, float rho, float eps,
                    float grad_scale, void* stream);
/* Adam and SGD with Keras 2.2's arithmetic, over the same flat buffers (16-byte aligned,
 * g' = g*grad_scale):
 *   Adam: m <- beta1*m + (1-beta1)*g' ; v <- beta2*v + (1-beta2)*g'^2 ;
 *         p <- p - lr_t*m/(sqrt(v)+eps), the caller passing the bias-corrected
 *         lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t), t = applied updates so far + 1 (no amsgrad);
 *   SGD:  mom <- momentum*mom - lr*g' ; p <- p + mom, or with nesterov != 0
 *         p <- p + momentum*mom - lr*g'.
 * A `decay` is the caller's: lr/(1 + decay*iterations) before the call. */
int cnnitmo_adam(float* p, const float* g, float* m, float* v, long n, float lr_t, float beta1, float beta2,
                 float eps, float grad_scale, void* stream);
int cnnitmo_sgd(float* p, const float* g, float* mom, long n, float lr, float momentum, int nesterov,
                float grad_scale, void* stream);

/* ---------------------------------------------------------------------------
 * Gradient clipping (keras.optimizers clipnorm / clipvalue, Keras 2.2 get_gradients: by the
 * GLOBAL norm over all gradients, then by value), over the flat fp32 gradient buffer, before
 * the update kernels above.  Nothing here waits for the host.
 *
 * cnnitmo_grad_sumsq: out[0] (device double) = sum g[i]^2, accumulated in fp64 (each square is
 *   exact, only the additions round: relative error <= n * 2^-53).  Bitwise reproducible: the
 *   grid and every thread's element order depend on n alone, workgroup partials go to the
 *   workspace and a second one-workgroup launch adds them in a fixed order; no atomics.  An
 *   aligned and a misaligned buffer holding the same values give the same bits.
 *   workspace: cnnitmo_grad_sumsq_workspace_bytes(n) bytes of device memory, 8-byte aligned,
 *   contents irrelevant; the query needs no GPU, 0 for n <= 0.
 * cnnitmo_grad_clip: in place; S = sumsq[0] is read on the device.  grad_scale is the factor the
 *   update kernel will apply to g (1 / world under data parallelism), so that the clipped
 *   quantity is the averaged gradient g' = g * grad_scale:
 *     N = grad_scale * sqrt(S) in fp64;
 *     f = clipnorm / N  if clipnorm > 0, S is finite and N >= clipnorm;  f = 1 otherwise;
 *     v = (float)((double)g[i] * f);
 *     if clipvalue > 0:  b = (float)(clipvalue / grad_scale),  v = min(max(v, -b), b)
 *     (by comparisons: a NaN stays a NaN).
 *   clipnorm <= 0 switches norm clipping off (sumsq may then be NULL), clipvalue <= 0 value
 *   clipping; both off is an argument error.
 * g must be 4-byte aligned: 16-byte accesses when it is 16-byte aligned, dword accesses
 * otherwise and for the tail; the values are the same either way.  CNNITMO_EINVAL before any
 * device call: a null or misaligned pointer, n <= 0, grad_scale not positive and finite, a NaN
 * clipnorm / clipvalue, clipnorm > 0 without sumsq.
 */
long cnnitmo_grad_sumsq_workspace_bytes(long n);
int cnnitmo_grad_sumsq(const float* g, long n, void* workspace, double* out, void* stream);
int cnnitmo_grad_clip(float* g, long n, const double* sumsq, double grad_scale, double clipnorm, double clipvalue,
                      void* stream);

/* ---------------------------------------------------------------------------
 * Training-data augmentation -- replaces the paired keras ImageDataGenerator
 * (rescale, rotation_range, horizontal/vertical_flip, zoom_range;
 * /root/reference/main.py:71-77 -> keras_preprocessing apply_transform +
 * standardize).  src [n,h,w,c] uint8 (src_u8 = 1) or fp32; mats [n][6] fp64 =
 * (a00, a01, t0, a10, a11, t1) mapping an output (row, col) to the input
 * (row, col) (transform_matrix_offset_center(rotation @ zoom)); flips [n]
 * (bit 0 horizontal, bit 1 vertical, applied after the affine map); bilinear
 * with clamp-to-edge ('nearest' fill, scipy order 1); dst [n,h,w,c] fp32 =
 * float32(interpolated) * scale.  c = 1 or 3.
 */
int cnnitmo_augment_affine(int src_u8, const void* src, int n, int h, int w, int c, const double* mats,
                           const int* flips, float scale, float* dst, void* stream);

/* ---------------------------------------------------------------------------
 * Dataset generation / HDR reconstruction maps -- replace the reference's
 * MATLAB scripts m-files/Reinhard.m:10-24 (tone mapping of HDR crops into the
 * SDR training inputs), m-files/virtual_camera.m:10-31 (random exposure + camera
 * curve) and m-files/inverse_Reinhard.m:1-23 (SDR -> HDR), float64 arithmetic.
 * Images are NHWC RGB: HDR fp32, SDR uint8.  lum_coef: HOST pointer to the 3
 * luminance weights of RGB2Lum (not in the reference; NULL = Rec. 709).
 *   stats (device, [n][2]) = per image: sum of log(max(f, realmin)) over pixels,
 *   and the count of zero-luminance pixels; f = Y (mode 0, fp32 HDR input) or
 *   X = I/(I-1) (mode 1, uint8 SDR, inverse_Reinhard.m as written).  A NaN f
 *   makes the image's sum NaN.  n <= 65535.
 *   apply: curve 0 = Reinhard, 1 = virtual camera, 1 | CNNITMO_CURVE_PER_CHANNEL =
 *   virtual camera with a per-channel response (X_c = key*2^v/G * hdr_c, sdr_c =
 *   min(1, (1+n) X_c^y / (n + X_c^y)): every channel clips on its own, not in the
 *   reference; the flag goes with curve 1 alone, any other value is refused); params
 *   (device, [n][3]) =
 *   (key*2^v, n, y) -- Reinhard uses (0.18, -, -); out fp32 or, out_u8 = 1,
 *   imwrite's uint8(255*x).  inverse: a = the key (0.18); mode 1 = the script
 *   (uint8 sdr, stats of mode 1, g unused); mode 2 = the exact inverse of
 *   Reinhard.m for a linear fp32 sdr and the HDR log-average g (stats unused).
 */
#define CNNITMO_CURVE_PER_CHANNEL 16 /* flag on curve 1 of cnnitmo_tonemap_apply */
size_t cnnitmo_tonemap_workspace_bytes(int n);
int cnnitmo_tonemap_stats(int mode, const void* img, int n, int h, int w, const double* lum_coef,
                          double* stats, void* workspace, size_t ws_bytes, void* stream);
int cnnitmo_tonemap_apply(int curve, const float* hdr, int n, int h, int w, const double* lum_coef,
                          const double* params, const double* stats, int out_u8, void* out, void* stream);
int cnnitmo_inverse_reinhard_apply(int mode, const void* sdr, int n, int h, int w, const double* lum_coef,
                                   const double* stats, double a, double g, float* out, void* stream);

/* ---------------------------------------------------------------------------
 * Image-fidelity metrics of two NHWC RGB batches a, b (fp32 [n][h][w][3],
 * contiguous), per image, with dynamic range max_val:
 *   mse  = mean over h*w*3 of (a-b)^2;  psnr = 10*log10(max_val^2 / mse)
 *          (tf.image.psnr; mse == 0 gives +inf);
 *   ssim = tf.image.ssim defaults (Wang et al. 2004): 11x11 Gaussian window,
 *          sigma 1.5, valid positions only, K1 0.01, K2 0.03, biased weighted
 *          moments, mean over the (h-10)*(w-10) positions and the 3 channels.
 * what: bit 0 = MSE/PSNR, bit 1 = SSIM.  out (device): double [n][3] =
 * {mse, psnr_dB, ssim}; entries not asked for are left untouched.  One pass over
 * both images, moment sums in fp64, fixed-order two-level reduction (bitwise
 * reproducible, no atomics).  The SSIM bit needs h >= 11 and w >= 11.
 * workspace: cnnitmo_image_metrics_workspace_bytes(n, h, w) bytes of device
 * memory (<= 0 for a bad shape; needs no GPU).
 */
long cnnitmo_image_metrics_workspace_bytes(int n, int h, int w);
int cnnitmo_image_metrics(int what, const float* a, const float* b, int n, int h, int w, double max_val,
                          double* out, void* workspace, long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Structural-dissimilarity training loss of a prediction y against a target t
 * (fp32 [n][h][w][3], contiguous, max_val 1), per image i:
 *   L_i = alpha (1 - SSIM_i) + (1 - alpha) B_i
 *   B_i = mean over h*w*3 of |y-t| (CNNITMO_BASE_MAE), of (y-t)^2 (CNNITMO_BASE_MSE),
 *         0 with CNNITMO_BASE_NONE (alpha must then be 1); alpha in [0, 1].
 * SSIM_i is cnnitmo_image_metrics' (same window, constants and valid positions).
 * out (device): double [n][3] = {ssim, B, L}.  dy (nullable, fp32 [n][h][w][3]) =
 * d(sum_i L_i / F)/dy, F = grad_frames (<= 0: n), the frame count the gradient is
 * normalised by (the role grad_numel plays for the pointwise losses); every element
 * is written exactly once, sign(0) = 0 for the MAE base.  A null dy gives the loss
 * only: the same out bit for bit, no coefficient planes written.
 * fp64 after the loads, fixed-order reductions, no atomics: bitwise reproducible.
 * Requires h >= 11 and w >= 11.  workspace: cnnitmo_dssim_workspace_bytes(n, h, w,
 * with_grad) bytes of device memory, 8-byte aligned, its contents irrelevant
 * (<= 0 for a bad shape; the query needs no GPU); with_grad 0: loss only.
 * Stateless, never allocates; bad arguments are CNNITMO_EINVAL before any launch.
 */
#define CNNITMO_BASE_NONE 0
#define CNNITMO_BASE_MAE 1
#define CNNITMO_BASE_MSE 2
long cnnitmo_dssim_workspace_bytes(int n, int h, int w, int with_grad);
int cnnitmo_dssim_loss_grad(int base, double alpha, const float* y, const float* t, int n, int h, int w,
                            double grad_frames, double* out, float* dy, void* workspace, long workspace_bytes,
                            void* stream);
/* ---------------------------------------------------------------------------
 * Multi-scale SSIM (tf.image.ssim_multiscale) of a prediction y against a target t
 * (fp32 [n][h][w][3], contiguous), per image i, as a metric and as a training loss:
 *   level 0 = the image, level k+1 = the 2x2 mean of level k, an odd side first extended
 *   by a copy of its last row / column (h' = ceil(h / 2));
 *   F[k][c] = mean over the valid positions of level k, channel c, of cs (k < scales-1)
 *             or of l cs (the last level): cnnitmo_image_metrics' window and moments,
 *             C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2;
 *   MS_c = prod_k max(F[k][c], 0)^power_factors[k],  ms_ssim = (MS_0 + MS_1 + MS_2) / 3;
 *   L_i = alpha (1 - ms_ssim_i) + (1 - alpha) B_i, B_i and alpha as for the DSSIM loss.
 * power_factors: host pointer to `scales` weights (1..5 of them, finite, >= 0), used as
 * given.  The coarsest level must be at least 11 x 11: h, w >= 161 for five scales.
 * out (device): double [n][3 + 3 scales] = {ms_ssim, B, L, F[0][0..2], F[1][0..2], ...}.
 * dy (nullable, fp32 [n][h][w][3]) = d(sum_i L_i / F)/dy, F = grad_frames (<= 0: n); a
 * channel with any factor <= 0 has MS_c = 0 and contributes exactly 0.  Every element is
 * written exactly once.  A null dy gives the loss only: the same out bit for bit.
 * fp64 after the loads, fixed-order reductions, no atomics: bitwise reproducible; the
 * scalars of the gradient stay on the device (no host synchronisation).
 * workspace: cnnitmo_msssim_workspace_bytes(n, h, w, scales, with_grad) bytes of device
 * memory, 8-byte aligned, its contents irrelevant (0 for a bad shape; the query needs no
 * GPU): the fp64 levels >= 1 of y and t (48 B per level pixel), the per-tile sums, and
 * with_grad the coefficient planes of every level (72 B per map position) and the level
 * gradients (24 B per level pixel): 16 B per pixel of the image for the loss alone, up to
 * 120 B with the gradient.
 * Stateless, never allocates; bad arguments are CNNITMO_EINVAL before any launch.
 */
long cnnitmo_msssim_workspace_bytes(int n, int h, int w, int scales, int with_grad);
int cnnitmo_msssim_loss_grad(int base, double alpha, const double* power_factors, int scales, double max_val,
                             const float* y, const float* t, int n, int h, int w, double grad_frames, double* out,
                             float* dy, void* workspace, long workspace_bytes, void* stream);
/* ---------------------------------------------------------------------------
 * Highlight-weighted training loss of a prediction y against a target t, the mask taken
 * from a source image s (all fp32 [n][h][w][3], contiguous; s may be t).  Per pixel p
 *   m = max over the channels of s[p],  a = fmin(fmax((m - tau) / (1 - tau), 0), 1)
 *       (the soft saturation mask of Eilertsen et al. 2017; a NaN gives 0, m == tau exactly 0),
 *   wgt = 1 + gain a,  l = (y-t)^2 (CNNITMO_BASE_MSE) or |y-t| (CNNITMO_BASE_MAE),
 * and per image i, N = h*w*3:
 *   A_i = sum_p a / (h w)          the mean mask
 *   B_i = sum l / N                the unweighted base term
 *   L_i = sum wgt l / N            the loss: not divided by sum wgt, so gain 0 is the base
 *                                  loss and unmasked pixels keep the base loss's gradient
 *   H_i = sum a l / (3 sum_p a)    the base error inside the highlights, 0 if sum_p a == 0
 * tau in [0, 1), gain >= 0 and finite, base MAE or MSE (CNNITMO_BASE_NONE is refused).
 * out (device): double [n][4] = {A, B, L, H}.  dy (nullable, fp32 [n][h][w][3]) =
 * (float)((wgt l') / (F N)), l' = 2 (y-t) or sign(y-t) with sign(0) = 0, F = grad_frames
 * (<= 0: n); every element is written exactly once.  A null dy gives the same out bit for
 * bit.  fp64 after the loads, no FMA contraction, fixed-order reductions, no atomics:
 * bitwise reproducible, and the same bits whether the images are 16-byte aligned (16-byte
 * loads and stores, four pixels a thread) or not (one float at a time).
 * workspace: cnnitmo_highlight_workspace_bytes(n, h, w) bytes of device memory (32 per
 * 1024 pixels of an image), 8-byte aligned, its contents irrelevant (<= 0 for a bad
 * shape; the query needs no GPU).
 * Stateless, never allocates; bad arguments are CNNITMO_EINVAL before any launch.
 */
long cnnitmo_highlight_workspace_bytes(int n, int h, int w);
int cnnitmo_highlight_loss_grad(int base, double tau, double gain, const float* s, const float* y, const float* t,
                                int n, int h, int w, double grad_frames, double* out, float* dy, void* workspace,
                                long workspace_bytes, void* stream);
/* 'accuracy' of the head without a backward kernel: *count (device, zeroed by the caller) +=
 * the pixels out of npix whose argmax over RGB agrees between y and t [npix][3] fp32, with
 * the head kernels' tie rule (the first of equal channels). */
int cnnitmo_rgb_accuracy(const float* y, const float* t, long npix, unsigned long long* count, void* stream);

/* ---------------------------------------------------------------------------
 * Radiance RGBE (.hdr / .pic) pixel codec: [npix][3] fp32 <-> [npix][4] bytes
 * (red, green, blue mantissas, shared exponent), device pointers.
 *   encode: NaN -> 0, components clamped to [0, 255 * 2^119]; v = max(r, g, b);
 *           v < 1e-32f -> (0,0,0,0); else frexpf(v) = (m, e), mantissa =
 *           floor(ldexpf(c, 8 - e)) (truncation; the largest is in 128..255),
 *           exponent byte = e + 128.
 *   decode: exponent byte 0 -> (0,0,0) whatever the mantissas; else
 *           c = (float)mantissa * 2^(E - 136), no +0.5 (rgbe.c, MATLAB hdrread).
 *           Every result is exact in fp32; E = 1 gives denormals, not flushed.
 * rgb must be 4-byte aligned.  16-byte accesses (four pixels per thread) when
 * both pointers are 16-byte aligned, one pixel per thread otherwise and for the
 * npix % 4 tail; the bytes are the same either way.  A null pointer or
 * npix <= 0 is CNNITMO_EINVAL before any device call.
 */
int cnnitmo_rgbe_encode(const float* rgb, long npix, uint8_t* rgbe, void* stream);
int cnnitmo_rgbe_decode(const uint8_t* rgbe, long npix, float* rgb, void* stream);

/* ---------------------------------------------------------------------------
 * Training pairs straight from HDR pictures: for each of n output frames [h][w][3] a warped
 * window of a source picture, its Reinhard target y and its virtual-camera input x, in one call
 * (the offline route is make_dataset's PNGs, re-decoded and warped by the data generator).
 * srcs: DEVICE array of n descriptors; the pictures may differ in size and format.
 *   mats / flips (device, [n][6] fp64 / [n]) as the augmentation call's, except that a
 *   matrix maps an output (row, col), after the flips, to (row, col) of the SOURCE picture;
 *   bilinear in fp64, the four neighbours clamped to the window [r0, r1] x [c0, c1]; an RGBE
 *   tap is decoded by the RGBE codec's rule; the result rounded to fp32 is the warped HDR pixel
 *   (stored to `warped` when given).
 *   Y = lum of that pixel, fp64, no FMA contraction; logsum[i] = sum over the frame of
 *   log(max(Y, realmin)) (stored when given), fixed partition and fixed-order fold, no atomics;
 *   G = exp(logsum * (1 / (h*w))).
 *   y: X = key/G * Y, L = X/(1+X), y_c = hdr_c * (L/Y);  x: the virtual-camera curve of the
 *   tone-map call with cam (device, [n][3] = (key*2^v, n, y)).  Then NaN -> 0 (a black pixel has
 *   Y = 0) and a clamp to [0, 1]; stored as (float)v, or for the outputs named by quantize
 *   (bit 0: x, bit 1: y) as (float)uint8(255 v) * (float)(1/255) with imwrite's rounding.
 * lum_coef: HOST pointer, NULL = Rec. 709.  workspace: 8-byte aligned device memory of the
 * queried size, contents irrelevant.  The window must lie inside the picture and fmt be 0 or 1:
 * the descriptors live on the device, so the caller checks that (ops.hdr_descriptors does); the
 * kernels cut the window to the picture.  An RGBE picture that is not 4-byte aligned is read by
 * bytes.  CNNITMO_EINVAL before any device call: a null pointer (warped and logsum may be
 * null), n, h or w <= 0, n > 65535, h*w >= 2^31, quantize outside 0..3, a short or misaligned
 * workspace.
 */
typedef struct {
  const void* pix; /* source picture, row 0 = top (device) */
  int h, w;        /* its size */
  int fmt;         /* 0: fp32 RGB [h][w][3]   1: RGBE bytes [h][w][4] */
  int r0, c0, r1, c1; /* inclusive clamp window inside the picture */
} cnnitmo_hdr_src;

size_t cnnitmo_hdr_pairs_workspace_bytes(int n);
int cnnitmo_hdr_pairs(const cnnitmo_hdr_src* srcs, int n, int h, int w, const double* mats, const int* flips,
                      const double* lum_coef, double key, const double* cam, int quantize, float* x, float* y,
                      float* warped, double* logsum, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * The same call with a sensor in front of the camera curve.  Everything above holds (same
 * workspace, same launches, same y, warped and logsum); only x changes:
 *   response 0: the curve acts on the luminance and the channels share its factor.  With noise
 *     null this is the call above, bit for bit.
 *   response 1: every channel is exposed, clipped at full well and put through the curve on its
 *     own, so an overexposed colour goes to white as on a sensor:
 *       e_c  = cam[i][0]/G * hdr_c                      exposure in units of full well
 *       e'_c = max(0, noisy(e_c, a_i, b_i, z_c))        with noise, else e_c
 *       x_c  = min(1, (1+n) e'_c^y / (n + e'_c^y))      then the store rule above
 *     (min is fmin: a negative e_c without noise has a NaN power and gives 1.)
 *   noise: device, [n][2] fp64 = (a, b) per frame, nullable = none; needs response 1.
 *     noisy(e, a, b, z) = e + sqrt(a max(e, 0) + b^2) z, the Poisson-Gaussian model: a = the
 *     shot-noise factor, b = the read-noise standard deviation, both >= 0 (the caller checks:
 *     they live on the device).  A frame with a = b = 0 gets the bits of the call without noise.
 *   keys: device, [n][2] uint64, required with noise.  z of pixel p = row * w + col of frame i:
 *     (s0, s1, s2, s3) = Philox4x64-10 (Salmon et al. 2011; numpy's np.random.Philox) with
 *     counter (p + 1, 0, 0, 0) and key keys[i], i.e. row p of np.random.Philox(key=keys[i],
 *     counter=[0,0,0,0]).random_raw(4 h w).reshape(-1, 4).  u1 = ((s0 >> 11) + 1) 2^-53,
 *     u2 = (s1 >> 11) 2^-53;  z_R = sqrt(-2 ln u1) cos(2 pi u2), z_G = sqrt(-2 ln u1) sin(2 pi u2);
 *     z_B = the cosine branch on (s2, s3).  fp64, no FMA contraction.  The noise of a frame
 *     depends on its key and its pixels alone, not on n or on its place in the batch; no
 *     atomics, bitwise reproducible.
 * CNNITMO_EINVAL before any device call: as above, and response outside 0..1, noise with
 * response 0, noise without keys, noise or keys not 8-byte aligned.
 *
 * cnnitmo_sensor_noise: out = (float)noisy((double)e, a_i, b_i, z) for every channel value of
 * e [n][h][w][3] fp32 (device, contiguous; out the same shape, not overlapping e), UNCLAMPED, with
 * the z above; a frame with a = b = 0 is copied.  noise and keys as above, both required.
 * CNNITMO_EINVAL before any device call: a null pointer, n, h or w <= 0, h*w >= 2^31,
 * a misaligned pointer.
 */
int cnnitmo_hdr_pairs_sensor(const cnnitmo_hdr_src* srcs, int n, int h, int w, const double* mats, const int* flips,
                             const double* lum_coef, double key, const double* cam, int quantize, int response,
                             const double* noise, const uint64_t* keys, float* x, float* y, float* warped,
                             double* logsum, void* workspace, size_t ws_bytes, void* stream);
int cnnitmo_sensor_noise(const float* e, int n, int h, int w, const double* noise, const uint64_t* keys, float* out,
                         void* stream);

/* ---------------------------------------------------------------------------
 * HDR quality metrics: the maps that put two linear-radiance images (fp32 [n][h][w][3],
 * contiguous) in front of cnnitmo_image_metrics (max_val 1).  fp64, no FMA contraction.
 *
 * cnnitmo_hdr_encode: out = (float)E(x), x = (double)v * scale[i] for every channel value v of
 * image i; scale: DEVICE double [n], cd/m^2 per unit.
 *   CNNITMO_ENC_PQ  (SMPTE ST 2084): L = fmin(fmax(x, 0), 1e4), y = L / 1e4,
 *                   E = pow((c1 + c2 y^m1) / (1 + c3 y^m1), m2), m1 = 2610/16384,
 *                   m2 = 2523/4096*128, c1 = 3424/4096, c2 = 2413/4096*32, c3 = 2392/4096*32;
 *   CNNITMO_ENC_LOG L = fmin(fmax(x, 0.005), 1e4), E = (log10 L - log10 0.005) / (4 - log10 0.005).
 *   NaN and negative x encode like the bottom of the range, +inf like 1e4 (C fmax / fmin).
 * 16-byte accesses when 3*h*w % 4 == 0 and img, out are 16-byte aligned, one value per thread
 * otherwise: the same values.  Every element of out is written exactly once; out may not alias img.
 *
 * cnnitmo_lum_percentile: out[i] (device float [n]) = Q_q of the luminance Y of image i
 * (lum_coef: HOST pointer to 3 weights, NULL = Rec. 709), defined on the bits of (float)Y:
 *   bin = (bits >> 17) - (bits(2^-32f) >> 17), 4096 bins = 64 octaves x 64; below 2^-32, zero,
 *   negatives and NaN -> bin 0; >= 2^32 -> bin 4095; need = max(1, ceil(q*h*w)) in double;
 *   b = the first bin whose cumulative count reaches need; Q = the float with the bits
 *   (b + 1 + (bits(2^-32f) >> 17)) << 17, the upper edge of b.
 * So Q >= the order statistic of rank need, by less than a factor 1 + 1/64.  Integer counts
 * (LDS histogram per workgroup, integer atomics into the workspace): bitwise reproducible.
 * workspace: cnnitmo_lum_percentile_workspace_bytes(n) bytes of device memory, 4-byte aligned,
 * contents irrelevant (the call zeroes it); the query needs no GPU, <= 0 for n <= 0.
 *
 * CNNITMO_EINVAL before any device call: a null pointer (lum_coef may be null), an unknown
 * encoding, n, h or w <= 0, n > 65535 or h*w >= 2^31 (percentile), q outside (0, 1], a misaligned
 * pointer, a short workspace.
 */
#define CNNITMO_ENC_PQ 0
#define CNNITMO_ENC_LOG 1
int cnnitmo_hdr_encode(int encoding, const float* img, int n, int h, int w, const double* scale, float* out,
                       void* stream);
long cnnitmo_lum_percentile_workspace_bytes(int n);
int cnnitmo_lum_percentile(const float* img, int n, int h, int w, const double* lum_coef, double q, float* out,
                           void* workspace, long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Baseline-JPEG round trip (encode + decode, no entropy coding: it is lossless) of n frames
 * x [n][h][w][3] fp32 -> out, same shape: the degradation of an SDR input that went through a
 * JPEG file.  Integers end to end after the load, the pixel path of the IJG library (libjpeg 6b /
 * libjpeg-turbo, default settings) restated in int32; tests/jpeg_ref.py is the same in numpy and
 * the two agree bit for bit.  `>>` is the arithmetic shift, clamp is to 0..255.  Per image:
 *   1. u = uint8(255 x): round half away from zero, saturating, NaN -> 0 (the quantised store of
 *      cnnitmo_hdr_pairs; exact for an x already on 8-bit levels).
 *   2. Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16                       (jccolor.c)
 *      Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *      Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *   3. 4:2:0: chroma (i, j), i < ceil(h/2), = (the four full-resolution samples of rows
 *      min(2i, h-1), min(2i+1, h-1) and columns min(2j, w-1), min(2j+1, w-1), + 1 for an even j,
 *      + 2 for an odd j) >> 2, for every j up to a multiple of 8 (jcsample.c replicates the right
 *      edge before it averages); rows are then added by replication.  4:4:4 skips this.
 *   4. per plane: whole 8x8 blocks by edge replication, - 128, jfdctint.c's forward DCT (rows,
 *      then columns; 8 x the coefficient), q = sign(c) ((|c| + (8Q >> 1)) / (8Q)), c' = q Q,
 *      jidctint.c's inverse DCT (columns, then rows), + 128, clamp.  Q: qtabs[i][0] for Y,
 *      qtabs[i][1] for Cb and Cr, natural (row-major) order.
 *   5. 4:2:0: triangle upsampling over the ceil(h/2) x ceil(w/2) decoded chroma samples C,
 *      neighbours replicated at the edges (jdsample.c, h2v2 "fancy"): output (r, c), i = r >> 1,
 *      j = c >> 1, i' = i - 1 (r even) or i + 1 (r odd), j' likewise from c, both clamped;
 *      s(j) = 3 C[i][j] + C[i'][j];  value = (3 s(j) + s(j') + (c odd ? 7 : 8)) >> 4.
 *   6. cb = Cb - 128, cr = Cr - 128;  R = clamp(Y + ((91881 cr + 32768) >> 16)),       (jdcolor.c)
 *      G = clamp(Y + ((-22554 cb - 46802 cr + 32768) >> 16)), B = clamp(Y + ((116130 cb + 32768) >> 16));
 *      stored as (float)level * (float)(1/255.), cnnitmo_hdr_pairs' expression.
 * subsampling: 0 = 4:4:4, 1 = 4:2:0.  qtabs: HOST array [n][2][64] (entries 1..65535; a libjpeg
 * quality gives 1..255) and apply: HOST array [n], nullable = all 1; an image with apply 0 is
 * copied through bit for bit.  Both are read before the call returns (they travel as kernel
 * arguments, eight images per launch) and cost the same whether the images share a table or not.
 * x, out: device, 4-byte aligned; the bits of out do not depend on any further alignment.  In
 * place (out == x) is supported; any other overlap of the two is CNNITMO_EINVAL.  Every element
 * of out is written exactly once.  workspace: cnnitmo_jpeg_workspace_bytes(n, h, w, subsampling)
 * bytes of device memory, 8-byte aligned, contents irrelevant: the decoded planes as uint8, between
 * the two launches of a group (1.5 or 3 bytes per pixel, each plane padded to whole blocks); the
 * query needs no GPU and answers 0 for a shape the call refuses.  No atomics: bitwise reproducible.
 * Stateless, never allocates.  CNNITMO_EINVAL before any launch: a null pointer (apply may be
 * null), n, h or w < 1, h*w >= 2^29, h >= 2^21 - 64, subsampling outside 0..1, a table entry of 0,
 * a short or misaligned workspace, a misaligned or partly overlapping x / out.
 */
long cnnitmo_jpeg_workspace_bytes(int n, int h, int w, int c /* chroma layout: the call's subsampling, 0 or 1 */);
int cnnitmo_jpeg_roundtrip(const float* x, int n, int h, int w, int subsampling, const unsigned short* qtabs,
                           const unsigned char* apply, float* out, void* workspace, long workspace_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------
 * Antialiased separable resampling of n pictures x [n][h][w][3] -> out [n][oh][ow][3], fp32
 * (dtype 0) or uint8 (dtype 1), with the arithmetic of Pillow's Image.resize (Resample.c);
 * tests/resize_ref.py is the same in numpy, and the three agree bit for bit (uint8: byte for byte).
 *
 * Filters f(x), all in C double; `support` in brackets:
 *   CNNITMO_RESIZE_BOX      (0.5)  1 for -0.5 < x <= 0.5, else 0
 *   CNNITMO_RESIZE_BILINEAR (1)    1 - |x| for |x| < 1
 *   CNNITMO_RESIZE_BICUBIC  (2)    a = -0.5: ((a+2)|x| - (a+3)) |x| |x| + 1 for |x| < 1,
 *                                  (((|x| - 5)|x| + 8)|x| - 4) a for |x| < 2
 *   CNNITMO_RESIZE_LANCZOS  (3)    sinc(x) sinc(x/3) for -3 <= x < 3; sinc(0) = 1, else
 *                                  sin(t)/t with t = x * M_PI formed first (libm sin)
 * cnnitmo_resize_coeffs (host, needs no GPU): the tables of one axis, `in` -> `out` samples:
 *   scale = in/out; fs = max(scale, 1); sup = support fs; ksize = (int)ceil(sup) * 2 + 1;
 *   for output sample xx: c = (xx + 0.5) scale; xmin = max((int)(c - sup + 0.5), 0);
 *   xmax = min((int)(c + sup + 0.5), in); n = xmax - xmin;
 *   k[x] = f((x + xmin - c + 0.5) * (1/fs)) for x < n, ww their sum in that order, k[x] /= ww when
 *   ww != 0, the rest of the row 0.  bounds [out][2] = (xmin, n), kk [out][ksize].
 *   Returns ksize; with bounds == kk == NULL it only returns ksize.  CNNITMO_EINVAL: a size < 1,
 *   an unknown filter, exactly one of the two pointers null.
 * One pass per axis whose size changes, the horizontal first, its result stored in the picture's
 * type (fp32, or a clamped uint8) in the workspace; the vertical pass runs on that.
 *   fp32:  ss = 0.0 (double); ss += (double)pixel[xmin + x] * k[x] for x = 0..n-1 in that order, a
 *          multiply and then an add (no fused multiply-add); store (float)ss.
 *   uint8: ki[x] = (int)(k[x] 2^22 + 0.5) for k[x] >= 0, (int)(k[x] 2^22 - 0.5) otherwise (made on
 *          the device, exact in fp64); ss = 2^21 (int32); ss += pixel * ki[x];
 *          store clamp(ss >> 22, 0, 255), `>>` the arithmetic shift.
 * Equal sizes on both axes is a copy.  lo (fp32 only; pass -INFINITY with uint8): a floor applied
 * where a value is stored to out (also by the copy), `v < lo ? lo : v`, so a NaN stays a NaN;
 * -INFINITY is Pillow's behaviour.
 * bounds_x / kk_x (ksize_x) are the tables of w -> ow, bounds_y / kk_y (ksize_y) those of h -> oh:
 * DEVICE pointers, 4- and 8-byte aligned; those of an axis that keeps its size are not read and may
 * be null.  Every index read from a table is clamped to the picture before it is used.
 * x, out, workspace: device, 4-byte aligned for fp32, any alignment for uint8; the bits of out do
 * not depend on further alignment.  workspace: cnnitmo_resize_workspace_bytes bytes, the
 * intermediate [n][h][ow][3] picture; 0 (and the pointer unused) when fewer than two passes run, or
 * for a shape the call refuses.  The query needs no GPU.
 * cnnitmo_resize_tile_cols (host): the output columns per workgroup tile of the horizontal pass for
 * these sizes, 0 when it takes the direct (no LDS) path: the source span of one column does not
 * fit the staging buffer.  For tests and profiling labels.
 * Stateless, never allocates, no atomics: bitwise reproducible.  CNNITMO_EINVAL before any launch,
 * out untouched: an unknown dtype, a null x / out / table of a running pass / workspace of two
 * passes, a size < 1, n*max(h,oh)*max(w,ow)*3 >= 2^31, a misaligned fp32 pointer, out or the
 * workspace overlapping x or each other, a NaN lo or a floor with uint8, a ksize that is not
 * (int)ceil(support * max(in/out, 1)) * 2 + 1 for one of the four supports.
 */
#define CNNITMO_RESIZE_BOX 0
#define CNNITMO_RESIZE_BILINEAR 1
#define CNNITMO_RESIZE_BICUBIC 2
#define CNNITMO_RESIZE_LANCZOS 3
int cnnitmo_resize_coeffs(int in, int out, int filter, int* bounds, double* kk);
int cnnitmo_resize_tile_cols(int w, int ow, int ksize_x);
long cnnitmo_resize_workspace_bytes(int dtype, int n, int h, int w, int rows /* oh */, int cols /* ow */);
int cnnitmo_resize(const void* x, int dtype, int n, int h, int w, void* out, int oh, int ow, const int* bounds_x,
                   const double* kk_x, int ksize_x, const int* bounds_y, const double* kk_y, int ksize_y, float lo,
                   void* workspace, void* stream);

/* ---------------------------------------------------------------------------
 * OpenEXR scan-line pixels (the container and zlib are host work: cnn_itmo_amd/exr.py).
 * A picture is h lines of line_bytes bytes; a line holds, channel after channel in the file's
 * channel-list order, that channel's w values, little-endian: CNNITMO_EXR_UINT (4 bytes),
 * CNNITMO_EXR_HALF (2), CNNITMO_EXR_FLOAT (4) -- the format's own type numbers.  Chunks of
 * lines_per_chunk lines (1: NONE / ZIPS, 16: ZIP; the last chunk may be short) follow each other
 * without gaps, chunk i at byte i * lines_per_chunk * line_bytes, n = its lines * line_bytes bytes.
 * A coded chunk holds ZIP's form t of its record bytes r: t[k] = r[2k] for k < half = (n + 1) / 2,
 * t[half + k] = r[2k + 1], then t[i] <- t[i] - t[i-1] + 128 (mod 256) left to right for i >= 1;
 * a plain chunk holds r.
 *
 * cnnitmo_exr_unpack: raw (device, h * line_bytes bytes, any alignment) -> rgb [h][w][3] fp32
 * (device, 4-byte aligned).  coded: device bytes [ceil(h / lines_per_chunk)], non-zero = coded, or
 * null = every chunk plain.  ch_off / ch_type: HOST arrays of three: the byte offset of the red,
 * green and blue channel inside a line and its type (the three may be one channel, a lone Y);
 * they travel as kernel arguments.  Coded chunks are undone in the workspace (device,
 * cnnitmo_exr_workspace_bytes, needed only with coded != null; it may hold anything): byte sums of
 * segments of cnnitmo_exr_segment_bytes() bytes, then a scan per segment -- two launches, no
 * waiting between workgroups -- then one launch gathers, converts and stores.  Conversions are
 * done on the bits: HALF -> fp32 exact, denormals included, inf and NaN with the payload << 13;
 * FLOAT copied; UINT -> fp32 rounded to nearest even.  Accesses are 16, 8 or 4 bytes wide where an
 * address allows and single bytes otherwise: the same bits either way.  No address depends on a
 * byte read from memory: a wrong `coded` flag gives wrong pixels, never a stray access.
 *
 * cnnitmo_exr_pack: rgb [h][w][3] fp32 -> out, h * 3 * w * size bytes: lines of the channels B, G,
 * R (the file's name order) of pixel_type HALF or FLOAT, every chunk coded (coded = 1) or plain (0).
 * fp32 -> HALF rounds to nearest even: 65520 and above -> inf, 2^-25 and below -> 0 with the sign,
 * a NaN stays a NaN (its top ten payload bits, or 1 when those are zero).
 *
 * Stateless, never allocate, no atomics: bitwise reproducible.  CNNITMO_EINVAL before any launch,
 * rgb / out untouched: a null raw / rgb / out / ch_off / ch_type, a null or short workspace with
 * coded != null, h or w < 1, lines_per_chunk other than 1 or 16, a line_bytes that is odd, < 1 or
 * >= 2^27, an unknown type, a channel offset that is odd or negative, a channel that runs past
 * line_bytes, a coded flag other than 0 / 1, an rgb that is not 4-byte aligned.
 * cnnitmo_exr_workspace_bytes(h, lines_per_chunk, line_bytes) (host, needs no GPU): 0 for sizes
 * the launch refuses.
 */
#define CNNITMO_EXR_UINT 0
#define CNNITMO_EXR_HALF 1
#define CNNITMO_EXR_FLOAT 2
int cnnitmo_exr_segment_bytes(void);
long cnnitmo_exr_workspace_bytes(int h, int rows /* lines_per_chunk */, long cols /* line_bytes */);
int cnnitmo_exr_unpack(const uint8_t* raw, const uint8_t* coded, int h, int w, int lines_per_chunk, long line_bytes,
                       const int* ch_off, const int* ch_type, float* rgb, void* workspace, long workspace_bytes,
                       void* stream);
int cnnitmo_exr_pack(const float* rgb, int h, int w, int pixel_type, int lines_per_chunk, int coded, uint8_t* out,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNN_ITMO_H_ */
