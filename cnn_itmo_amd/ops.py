"""Thin typed wrappers over the C ABI (include/cnn_itmo.h).

Activations are passed as ``View`` objects: an NHWC channel window
(buffer, ld, off) of a device buffer -- the zero-copy concatenation of
model.py:246-261 is just two views of one buffer.  torch supplies device
memory and the current HIP stream; every FLOP runs in libcnnitmo.so.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from ._lib import call, query

DTYPES = {"float32": (L.F32, torch.float32), "bfloat16": (L.BF16, torch.bfloat16)}


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


@dataclass
class View:
    """Element (p, c) of an [n, h, w, c] activation is buf[p*ld + off + c]."""
    buf: torch.Tensor
    n: int
    h: int
    w: int
    c: int
    ld: int
    off: int = 0

    @property
    def p(self):
        return self.n * self.h * self.w

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def tensor(self):
        """[n, h, w, c] strided torch view (for tests / host copies)."""
        return self.buf.view(-1)[self.off:].as_strided((self.n, self.h, self.w, self.c),
                                                       (self.h * self.w * self.ld, self.w * self.ld, self.ld, 1))


def new_view(n, h, w, c, dtype, device="cuda"):
    return View(torch.empty(n * h * w * c, dtype=dtype, device=device), n, h, w, c, c, 0)


def workspace(nbytes, device="cuda"):
    return torch.empty(max(16, int(nbytes)), dtype=torch.uint8, device=device)


# ---------------------------------------------------------------- convolutions
def conv3x3_fwd(dt, x: View, wt, bias, out: View, flags=0, aff=None, stats=None, border=None):
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_conv3x3_fwd", dt, x.ptr, x.ld, x.off, x.n, x.h, x.w, x.c, ptr(wt), ptr(bias),
         out.c, out.ptr, out.ld, out.off, flags, ptr(sc), ptr(sh), ptr(stats), ptr(border),
         stream_ptr())


def conv3x3_fwd_pool(dt, x: View, wt, bias, out: View, pool_out, pool_idx, pool_sign=None, flags=0, aff=None,
                     stats=None, border=None):
    """conv3x3_fwd + the output's 2x2 MaxPooling2D in the epilogue (cnnitmo_conv3x3_fwd_pool):
    pool_out / pool_idx [n, h/2, w/2, cout] dense; pool_sign [cout] (None: max)."""
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_conv3x3_fwd_pool", dt, x.ptr, x.ld, x.off, x.n, x.h, x.w, x.c, ptr(wt), ptr(bias),
         out.c, out.ptr, out.ld, out.off, flags, ptr(sc), ptr(sh), ptr(stats), ptr(border),
         ptr(pool_out), out.c, ptr(pool_idx), ptr(pool_sign), stream_ptr())


def pool_supported(dt, n, h, w, cin, cout):
    return query("cnnitmo_conv3x3_pool_supported", dt, n, h, w, cin, cout) == 1


def conv3x3_fwd_head(dt, x: View, wt, bias, cout, flags, aff, h_valid, head_w, head_b, yhat):
    """The inference forward of the last 3x3 ConvBN with the sigmoid head in its epilogue
    (cnnitmo_conv3x3_fwd_head): yhat [n, h_valid, w, 3] fp32; the conv output is not stored."""
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_conv3x3_fwd_head", dt, x.ptr, x.ld, x.off, x.n, x.h, x.w, x.c, ptr(wt), ptr(bias), cout, flags,
         ptr(sc), ptr(sh), h_valid, ptr(head_w), ptr(head_b), ptr(yhat), stream_ptr())


def head_supported(dt, n, h, w, cin, cout):
    return query("cnnitmo_conv3x3_head_supported", dt, n, h, w, cin, cout) == 1


def conv3x3_fwd_cat(dt, x1: View, x2: View, wt, bias, out: View, flags=0, aff=None, stats=None, border=None):
    """conv3x3_fwd over concatenate([x1, x2]) read from its members (cnnitmo_conv3x3_fwd_cat)."""
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_conv3x3_fwd_cat", dt, x1.ptr, x1.ld, x1.off, x1.c, x2.ptr, x2.ld, x2.off, x1.n, x1.h, x1.w,
         x1.c + x2.c, ptr(wt), ptr(bias), out.c, out.ptr, out.ld, out.off, flags, ptr(sc), ptr(sh), ptr(stats),
         ptr(border), stream_ptr())


def conv1tap_fwd(dt, cols, k, m, wt, bias, out: View, flags=0, aff=None, stats=None):
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_conv1tap_fwd", dt, ptr(cols), k, m, ptr(wt), ptr(bias), out.c, out.ptr, out.ld,
         out.off, flags, ptr(sc), ptr(sh), ptr(stats), stream_ptr())


def fwd_stat_rows(dt, m, ncols):
    return query("cnnitmo_fwd_stat_rows", dt, m, ncols)


def conv3x3_stat_rows(dt, n, h, w, cin, cout):
    return query("cnnitmo_conv3x3_stat_rows", dt, n, h, w, cin, cout)


def tconv_stat_rows(dt, n, h, w, cin, cout):
    """BN partial rows of tconv_fwd over an n x h x w input grid."""
    return query("cnnitmo_tconv2x2_stat_rows", dt, n, h, w, cin, cout)


def conv3x3_dgrad(dt, dz, n, h, w, cout, wflip, cin, dx: View):
    call("cnnitmo_conv3x3_dgrad", dt, ptr(dz), n, h, w, cout, ptr(wflip), cin, dx.ptr, dx.ld, dx.off,
         stream_ptr())


def conv3x3_dgrad_bn_rows(dt, n, h, w, cout, cin, c0, c1):
    return query("cnnitmo_conv3x3_dgrad_bn_rows", dt, n, h, w, cout, cin, c0, c1)


def conv3x3_dgrad_bn(dt, dz, n, h, w, cout, wflip, cin, dx, c0, c1, coef, r, dz_out, part, parity):
    """conv3x3_dgrad with the producer's BN backward fused (see cnn_itmo.h); dx: View or None."""
    rp, rld, roff = _rview(r, c1 - c0)
    call("cnnitmo_conv3x3_dgrad_bn", dt, ptr(dz), n, h, w, cout, ptr(wflip), cin,
         dx.ptr if dx is not None else None, dx.ld if dx is not None else cin, dx.off if dx is not None else 0,
         c0, c1, ptr(coef), rp, rld, roff, ptr(dz_out), ptr(part), 1 if parity else 0, stream_ptr())


def conv3x3_dgrad_bn_pooled_rows(dt, n, h, w, cout, cin):
    return query("cnnitmo_conv3x3_dgrad_bn_pooled_rows", dt, n, h, w, cout, cin)


def conv3x3_dgrad_bn_pooled(dt, dz, n, h, w, cout, wflip, cin, coef, r, dyp, idx, dz_out, part):
    """The skip member's input gradient + its MaxPooling2D gradient routed by idx, through the
    producer's BN backward (cnnitmo_conv3x3_dgrad_bn_pooled): the skip gradient is never stored."""
    rp, rld, roff = _rview(r, cin)
    call("cnnitmo_conv3x3_dgrad_bn_pooled", dt, ptr(dz), n, h, w, cout, ptr(wflip), cin, ptr(coef), rp, rld, roff,
         ptr(dyp), ptr(idx), ptr(dz_out), ptr(part), stream_ptr())


def tconv_dgrad_bn_rows(dt, n, h, w, cout, cin):
    return query("cnnitmo_tconv2x2_dgrad_bn_rows", dt, n, h, w, cout, cin)


def tconv_dgrad_bn(dt, dout, n, h, w, cout, kT, cin, coef, r, dz_out, part):
    """tconv2x2_dgrad with the producer's BN backward fused (see cnn_itmo.h)."""
    rp, rld, roff = _rview(r, cin)
    call("cnnitmo_tconv2x2_dgrad_bn", dt, ptr(dout), n, h, w, cout, ptr(kT), cin, ptr(coef), rp, rld, roff,
         ptr(dz_out), ptr(part), stream_ptr())


def conv_wgrad(dt, ntaps, x: View, dz, cout, dw, dw_cols=0, fold=None, raw=None):
    """fold = (scale, shift, db, border_sums) for a folded input BN, else None;
    raw (optional, dw-shaped fp32): the uncorrected dz (x) r sum."""
    nbytes = query("cnnitmo_wgrad_workspace_bytes", dt, x.n, x.h, x.w, x.c, cout, ntaps)
    ws = workspace(nbytes, dz.device)
    fs, fh, fdb, fb = fold if fold is not None else (None,) * 4
    call("cnnitmo_conv_wgrad", dt, ntaps, x.ptr, x.ld, x.off, ptr(dz), x.n, x.h, x.w, x.c, cout,
         ptr(dw), dw_cols, ptr(fs), ptr(fh), ptr(fdb), ptr(fb), ptr(raw), ws.data_ptr(), ws.numel(),
         stream_ptr())


def conv_wgrad_cat(dt, x1: View, x2: View, dz, cout, dw, fold=None, raw=None):
    """conv_wgrad (9 taps) over concatenate([x1, x2]) read from its members (cnnitmo_conv_wgrad_cat)."""
    cin = x1.c + x2.c
    ws = workspace(query("cnnitmo_wgrad_cat_workspace_bytes", x1.n, x1.h, x1.w, x1.c, cin, cout), dz.device)
    fs, fh, fdb, fb = fold if fold is not None else (None,) * 4
    call("cnnitmo_conv_wgrad_cat", dt, x1.ptr, x1.ld, x1.off, x1.c, x2.ptr, x2.ld, x2.off, ptr(dz), x1.n, x1.h,
         x1.w, cin, cout, ptr(dw), ptr(fs), ptr(fh), ptr(fdb), ptr(fb), ptr(raw), ws.data_ptr(), ws.numel(),
         stream_ptr())


def fwd_cat_supported(dt, n, h, w, c1, cin, cout):
    return query("cnnitmo_conv3x3_fwd_cat_supported", dt, n, h, w, c1, cin, cout) == 1


def wgrad_cat_supported(n, h, w, c1, cin, cout):
    return query("cnnitmo_wgrad_cat_workspace_bytes", n, h, w, c1, cin, cout) > 0


def conv_c3_stat_rows(n, h, w):
    return query("cnnitmo_conv_c3_stat_rows", n, h, w)


def conv_c3_fwd(dt, x, n, h_valid, h, w, wt, bias, out: View, flags=0, aff=None, stats=None):
    """First layer (bf16 or fp32 output), operands built from the fp32 input image (no
    im2col buffer)."""
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_conv_c3_fwd", dt, ptr(x), n, h_valid, h, w, ptr(wt), ptr(bias), out.ptr, out.ld, out.off, flags,
         ptr(sc), ptr(sh), ptr(stats), stream_ptr())


def conv_c3_wgrad(dt, x, n, h_valid, h, w, dz, dw):
    ws = workspace(query("cnnitmo_conv_c3_wgrad_workspace_bytes", n, h, w), dz.device)
    call("cnnitmo_conv_c3_wgrad", dt, ptr(x), n, h_valid, h, w, ptr(dz), ptr(dw), ws.data_ptr(), ws.numel(),
         stream_ptr())


def im2col_c3(dt, x, n, h_valid, h, w, cols):
    call("cnnitmo_im2col_c3", dt, ptr(x), n, h_valid, h, w, ptr(cols), stream_ptr())


def tconv_fwd(dt, x: View, k, bias, out: View, flags=0, aff=None, stats=None):
    assert x.ld == x.c and x.off == 0
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_tconv2x2_fwd", dt, x.ptr, x.n, x.h, x.w, x.c, ptr(k), ptr(bias), out.c, out.ptr,
         out.ld, out.off, flags, ptr(sc), ptr(sh), ptr(stats), stream_ptr())


def tconv_dgrad(dt, dout, n, h, w, cout, kT, cin, dx):
    call("cnnitmo_tconv2x2_dgrad", dt, ptr(dout), n, h, w, cout, ptr(kT), cin, ptr(dx), stream_ptr())


def tconv_wgrad(dt, x: View, dout, cout, dk, fold=None, raw=None):
    """fold = (scale, shift, parity_sums[4*cout]) for a folded input BN, else None."""
    assert x.ld == x.c and x.off == 0
    nbytes = query("cnnitmo_tconv2x2_wgrad_workspace_bytes", dt, x.n, x.h, x.w, x.c, cout)
    ws = workspace(nbytes, dout.device)
    fs, fh, fp = fold if fold is not None else (None,) * 3
    call("cnnitmo_tconv2x2_wgrad", dt, x.ptr, ptr(dout), x.n, x.h, x.w, x.c, cout, ptr(dk),
         ptr(fs), ptr(fh), ptr(fp), ptr(raw), ws.data_ptr(), ws.numel(), stream_ptr())


def prep_conv3x3(dt, w32, cout, cin, wf, wflip):
    call("cnnitmo_prep_conv3x3_weights", dt, ptr(w32), cout, cin, ptr(wf), ptr(wflip), stream_ptr())


def prep_tconv(dt, k32, cout, cin, kf, kT):
    call("cnnitmo_prep_tconv2x2_weights", dt, ptr(k32), cout, cin, ptr(kf), ptr(kT), stream_ptr())


def prep_c3(dt, w32, cout, wp):
    call("cnnitmo_prep_c3_weights", dt, ptr(w32), cout, ptr(wp), stream_ptr())


def fold_conv3x3(dt, w32, b, scale, shift, cout, cin, wout, bout, border):
    call("cnnitmo_fold_conv3x3", dt, ptr(w32), ptr(b), ptr(scale), ptr(shift), cout, cin, ptr(wout),
         ptr(bout), ptr(border), stream_ptr())


def fold_tconv(dt, k32, b, scale, shift, cout, cin, kout, bout):
    call("cnnitmo_fold_tconv2x2", dt, ptr(k32), ptr(b), ptr(scale), ptr(shift), cout, cin, ptr(kout),
         ptr(bout), stream_ptr())


def border_rows(n):
    return query("cnnitmo_border_rows", n)


def border_sums(dt, dz, n, h, w, c, part):
    call("cnnitmo_border_sums", dt, ptr(dz), n, h, w, c, ptr(part), stream_ptr())


# ---------------------------------------------------------------- pooling
def maxpool_fwd(dt, x: View, y, idx, aff=None):
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_maxpool2x2_fwd", dt, x.ptr, x.ld, x.off, x.n, x.h, x.w, x.c, ptr(y), ptr(idx),
         ptr(sc), ptr(sh), stream_ptr())


def maxpool_bwd(dt, dy, idx, dx: View):
    call("cnnitmo_maxpool2x2_bwd", dt, ptr(dy), ptr(idx), dx.n, dx.h, dx.w, dx.c, dx.ptr, dx.ld,
         dx.off, stream_ptr())


# ---------------------------------------------------------------- batch norm
def reduce_ws(rows, cols, device):
    return workspace(query("cnnitmo_reduce_workspace_bytes", rows, cols), device)


def bn_fwd_finalize(stats, rows, c, groups, count, gamma, beta, mmean, mvar, momentum, eps,
                    scale, shift, smean, sinv):
    ws = reduce_ws(rows, 2 * groups * c, stats.device)
    call("cnnitmo_bn_fwd_finalize", ptr(stats), rows, c, groups, float(count), ptr(gamma), ptr(beta),
         ptr(mmean), ptr(mvar), momentum, eps, ptr(scale), ptr(shift), ptr(smean), ptr(sinv),
         ws.data_ptr(), stream_ptr())


def bn_infer_coeffs(c, gamma, beta, mmean, mvar, eps, scale, shift):
    call("cnnitmo_bn_infer_coeffs", c, ptr(gamma), ptr(beta), ptr(mmean), ptr(mvar), eps, ptr(scale),
         ptr(shift), stream_ptr())


def bn_apply(dt, r, p, c, scale, shift, y: View, flags=0, seed=0, layer=0):
    call("cnnitmo_bn_apply", dt, ptr(r), p, c, ptr(scale), ptr(shift), y.ptr, y.ld, y.off, flags,
         seed, layer, stream_ptr())


def bn_bwd_rows(p, c):
    return query("cnnitmo_bn_bwd_rows", p, c)


def _rview(r, c):
    """(ptr, ld, off) of a saved post-ReLU tensor given as a View or a contiguous [p][c] tensor."""
    if isinstance(r, View):
        return r.ptr, r.ld, r.off
    return ptr(r), c, 0


def bn_bwd_reduce(dt, dy: View, r, c, mean, inv, flags, seed, layer, part):
    rp, rld, roff = _rview(r, c)
    call("cnnitmo_bn_bwd_reduce", dt, dy.ptr, dy.ld, dy.off, rp, rld, roff, dy.p, c, ptr(mean),
         ptr(inv), flags, seed, layer, ptr(part), stream_ptr())


def bn_bwd_finalize(part, rows, c, count, gamma, mean, inv, dgamma, dbeta, coef):
    ws = reduce_ws(rows, 2 * c, part.device)
    call("cnnitmo_bn_bwd_finalize", ptr(part), rows, c, float(count), ptr(gamma), ptr(mean), ptr(inv),
         ptr(dgamma), ptr(dbeta), ptr(coef), ws.data_ptr(), stream_ptr())


def bn_bwd_apply(dt, dy: View, r, c, coef, flags, seed, layer, dz, part):
    """flags & L.PARITY: part columns are [4][c] split by (h&1, w&1) of dy's pixel."""
    rp, rld, roff = _rview(r, c)
    call("cnnitmo_bn_bwd_apply", dt, dy.ptr, dy.ld, dy.off, rp, rld, roff, dy.p, c, ptr(coef), flags,
         seed, layer, dy.h, dy.w, ptr(dz), ptr(part), stream_ptr())


def bn_bwd_apply_pooled(dt, dy: View, r, c, coef, dyp, idx, dz, part):
    """bn_bwd_apply with a deferred MaxPooling2D backward folded in: dy += dyp routed by idx."""
    rp, rld, roff = _rview(r, c)
    call("cnnitmo_bn_bwd_apply_pooled", dt, dy.ptr, dy.ld, dy.off, rp, rld, roff, dy.n, dy.h, dy.w, c,
         ptr(coef), ptr(dyp), ptr(idx), ptr(dz), ptr(part), stream_ptr())


def colsum(part, rows, cols, groups, out):
    ws = reduce_ws(rows, cols, part.device)
    call("cnnitmo_colsum", ptr(part), rows, cols, groups, ptr(out), ws.data_ptr(), stream_ptr())


# ---------------------------------------------------------------- head / optimizer
def head_fwd(dt, x: View, h_valid, wt, b, yhat, aff=None):
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_head_fwd", dt, x.ptr, x.n, x.h, h_valid, x.w, x.c, ptr(wt), ptr(b), ptr(sc),
         ptr(sh), ptr(yhat), stream_ptr())


def head_fwd_bwd(dt, x: View, h_valid, wt, b, target, dx, part, aff=None, grad_numel=0.0):
    """grad_numel: the MSE gradient's normaliser (0: this batch's element count; see cnn_itmo.h)."""
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_head_fwd_bwd", dt, x.ptr, x.n, x.h, h_valid, x.w, x.c, ptr(wt), ptr(b), ptr(sc),
         ptr(sh), ptr(target), ptr(dx), ptr(part), float(grad_numel), stream_ptr())


def head_fwd_bwd_g3(dt, x: View, h_valid, wt, b, target, g3, part, aff=None, grad_numel=0.0):
    """head_fwd_bwd whose input gradient leaves as g3 [p][3] (dx = g3 . W)."""
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_head_fwd_bwd_g3", dt, x.ptr, x.n, x.h, h_valid, x.w, x.c, ptr(wt), ptr(b), ptr(sc),
         ptr(sh), ptr(target), ptr(g3), ptr(part), float(grad_numel), stream_ptr())


def head_fwd_bwd_loss(loss, dt, x: View, h_valid, wt, b, target, part, dx=None, g3=None, aff=None, grad_numel=0.0):
    """head_fwd_bwd (dx) or head_fwd_bwd_g3 (g3) with the loss `loss` (an L.LOSSES id)."""
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_head_fwd_bwd_loss", loss, dt, x.ptr, x.n, x.h, h_valid, x.w, x.c, ptr(wt), ptr(b), ptr(sc),
         ptr(sh), ptr(target), ptr(dx), ptr(g3), ptr(part), float(grad_numel), stream_ptr())


def head_fwd_bwd_given(dt, x: View, h_valid, wt, b, target, dy, part, dx=None, g3=None, aff=None):
    """head_fwd_bwd (dx) or head_fwd_bwd_g3 (g3) with the loss gradient dy [n, h_valid, w, 3] given,
    already normalised; the loss slot of part is 0 (cnnitmo_head_fwd_bwd_given)."""
    sc, sh = aff if aff is not None else (None, None)
    call("cnnitmo_head_fwd_bwd_given", dt, x.ptr, x.n, x.h, h_valid, x.w, x.c, ptr(wt), ptr(b), ptr(sc),
         ptr(sh), ptr(target), ptr(dy), ptr(dx), ptr(g3), ptr(part), stream_ptr())


def bn_bwd_apply_g3(dt, g3, wh, r, c, p, coef, dz, part):
    rp, rld, roff = _rview(r, c)
    call("cnnitmo_bn_bwd_apply_g3", dt, ptr(g3), ptr(wh), rp, rld, roff, p, c, ptr(coef), ptr(dz), ptr(part),
         stream_ptr())


def head_rows(p):
    return query("cnnitmo_head_rows", p)


def head_finalize(part, rows, cin, numel, loss_acc, dw, db, aff=None, raw=None):
    sc, sh = aff if aff is not None else (None, None)
    ws = reduce_ws(rows, 5 + 3 * cin, part.device)
    call("cnnitmo_head_finalize", ptr(part), rows, cin, float(numel), ptr(sc), ptr(sh),
         ptr(loss_acc), ptr(dw), ptr(db), ptr(raw), ws.data_ptr(), stream_ptr())


def bn_consumer_sums(mode, w, raw, cout, cin_tot, ci0, c, db, vtab, mean, inv, part):
    """part[CONSUMER_ROWS][2][c] = (sum dy, sum dy*rhat) of a BN output from its consumer's weight
    gradient (mode 1 conv3x3, 2 tconv, 3 head); see cnn_itmo.h."""
    call("cnnitmo_bn_consumer_sums", mode, ptr(w), ptr(raw), cout, cin_tot, ci0, c, ptr(db), ptr(vtab),
         ptr(mean), ptr(inv), ptr(part), stream_ptr())


def pool_bnsums(dt, dyp, idx, r: View, mean, inv, part):
    """The MaxPooling2D share of a folded BN output's backward sums (rows =
    bn_bwd_rows(pooled pixels, c)); r is the pool input's view."""
    call("cnnitmo_pool_bnsums", dt, ptr(dyp), ptr(idx), r.n, r.h, r.w, r.c, r.ptr, r.ld, r.off, ptr(mean),
         ptr(inv), ptr(part), stream_ptr())


def pool_bnsums_pooled(dt, dyp, pr, n, h, w, c, mean, inv, part):
    """pool_bnsums when the producer pooled in its epilogue: pr = r at each window index
    [n, h/2, w/2, c] dense (h, w: the pool INPUT's size)."""
    call("cnnitmo_pool_bnsums_pooled", dt, ptr(dyp), ptr(pr), n, h, w, c, ptr(mean), ptr(inv), ptr(part),
         stream_ptr())


def rmsprop(p, g, a, lr, rho, eps, grad_scale=1.0):
    call("cnnitmo_rmsprop", ptr(p), ptr(g), ptr(a), p.numel(), lr, rho, eps, grad_scale, stream_ptr())


def adam(p, g, m, v, lr_t, beta1, beta2, eps, grad_scale=1.0):
    """lr_t: the bias-corrected rate lr*sqrt(1-beta2^t)/(1-beta1^t) (see cnn_itmo.h)."""
    call("cnnitmo_adam", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr_t, beta1, beta2, eps, grad_scale,
         stream_ptr())


def sgd(p, g, mom, lr, momentum=0.0, nesterov=False, grad_scale=1.0):
    call("cnnitmo_sgd", ptr(p), ptr(g), ptr(mom), p.numel(), lr, momentum, int(bool(nesterov)), grad_scale,
         stream_ptr())


def grad_sumsq_workspace_bytes(n):
    return int(query("cnnitmo_grad_sumsq_workspace_bytes", n))


def grad_sumsq(g, out=None, ws=None):
    """g: contiguous 1-D fp32 device tensor -> out (float64 [1], device) = sum g^2 in fp64, bitwise
    reproducible (cnnitmo_grad_sumsq).  ws: a uint8 workspace of grad_sumsq_workspace_bytes(n)."""
    assert g.dtype == torch.float32 and g.is_contiguous() and g.dim() == 1, (g.dtype, tuple(g.shape))
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=g.device)
    assert out.dtype == torch.float64 and out.numel() >= 1
    if ws is None:
        ws = workspace(grad_sumsq_workspace_bytes(g.numel()), g.device)
    assert ws.numel() * ws.element_size() >= grad_sumsq_workspace_bytes(g.numel())
    call("cnnitmo_grad_sumsq", ptr(g), g.numel(), ws.data_ptr(), ptr(out), stream_ptr())
    return out


def grad_clip(g, sumsq, grad_scale=1.0, clipnorm=0.0, clipvalue=0.0):
    """In place on g (contiguous 1-D fp32): Keras' clipnorm (global norm, from sumsq = grad_sumsq(g),
    read on the device) then clipvalue, of the gradient g * grad_scale (cnnitmo_grad_clip).  sumsq
    may be None without clipnorm."""
    assert g.dtype == torch.float32 and g.is_contiguous() and g.dim() == 1, (g.dtype, tuple(g.shape))
    assert sumsq is None or sumsq.dtype == torch.float64
    call("cnnitmo_grad_clip", ptr(g), g.numel(), ptr(sumsq), float(grad_scale), float(clipnorm or 0.0),
         float(clipvalue or 0.0), stream_ptr())
    return g


def augment_affine(src, mats, flips, scale, dst):
    """src [n,h,w,c] uint8/fp32 device tensor; mats [n,6] fp64 and flips [n] int32 device
    tensors; dst [n,h,w,c] fp32 (cnnitmo_augment_affine)."""
    n, h, w, c = src.shape
    assert src.is_contiguous() and dst.is_contiguous() and tuple(dst.shape) == (n, h, w, c)
    assert mats.dtype == torch.float64 and flips.dtype == torch.int32 and mats.numel() == 6 * n
    call("cnnitmo_augment_affine", 1 if src.dtype == torch.uint8 else 0, ptr(src), n, h, w, c, ptr(mats),
         ptr(flips), float(scale), ptr(dst), stream_ptr())


# ---------------------------------------------------------------- image metrics
MSE_PSNR = 1
SSIM = 2


def image_metrics_workspace_bytes(n, h, w):
    return query("cnnitmo_image_metrics_workspace_bytes", n, h, w)


def image_metrics(what, a, b, max_val=1.0, out=None):
    """a, b [n,h,w,3] contiguous fp32 device tensors -> out [n,3] fp64 = (mse, psnr dB, ssim) per
    image (cnnitmo_image_metrics); what = MSE_PSNR | SSIM, columns not asked for are left as they
    are (NaN in a fresh out)."""
    n, h, w, c = a.shape
    assert c == 3 and tuple(b.shape) == (n, h, w, 3), (tuple(a.shape), tuple(b.shape))
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.full((n, 3), float("nan"), dtype=torch.float64, device=a.device)
    ws = workspace(image_metrics_workspace_bytes(n, h, w), a.device)
    call("cnnitmo_image_metrics", what, ptr(a), ptr(b), n, h, w, float(max_val), ptr(out), ws.data_ptr(),
         ws.numel(), stream_ptr())
    return out


# ---------------------------------------------------------------- DSSIM loss
def dssim_workspace_bytes(n, h, w, with_grad):
    return query("cnnitmo_dssim_workspace_bytes", n, h, w, int(bool(with_grad)))


def dssim_loss_grad(base, alpha, y, t, dy=None, grad_frames=0.0, out=None):
    """y, t [n,h,w,3] contiguous fp32 device tensors -> out [n,3] fp64 = (ssim, base term, loss) per
    image; dy (optional, like y) = the gradient of the batch-mean loss, normalised by grad_frames
    (0: n) frames (cnnitmo_dssim_loss_grad).  base: an L.DSSIM_BASES id."""
    n, h, w, c = y.shape
    assert c == 3 and tuple(t.shape) == (n, h, w, 3), (tuple(y.shape), tuple(t.shape))
    assert y.dtype == torch.float32 and t.dtype == torch.float32 and y.is_contiguous() and t.is_contiguous()
    assert dy is None or (dy.dtype == torch.float32 and dy.is_contiguous() and tuple(dy.shape) == (n, h, w, 3))
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float64, device=y.device)
    ws = workspace(dssim_workspace_bytes(n, h, w, dy is not None), y.device)
    call("cnnitmo_dssim_loss_grad", base, float(alpha), ptr(y), ptr(t), n, h, w, float(grad_frames), ptr(out),
         ptr(dy), ws.data_ptr(), ws.numel(), stream_ptr())
    return out


# ---------------------------------------------------------------- MS-SSIM metric and loss
def msssim_workspace_bytes(n, h, w, scales, with_grad):
    return query("cnnitmo_msssim_workspace_bytes", n, h, w, scales, int(bool(with_grad)))


def msssim_loss_grad(base, alpha, power_factors, y, t, dy=None, grad_frames=0.0, max_val=1.0, out=None):
    """y, t [n,h,w,3] contiguous fp32 device tensors -> out [n, 3 + 3 scales] fp64 = (ms_ssim, base
    term, loss, the factors F[k][c]) per image; dy (optional, like y) = the gradient of the
    batch-mean loss, normalised by grad_frames (0: n) frames (cnnitmo_msssim_loss_grad).  base: an
    L.DSSIM_BASES id; power_factors: 1..5 host floats."""
    n, h, w, c = y.shape
    assert c == 3 and tuple(t.shape) == (n, h, w, 3), (tuple(y.shape), tuple(t.shape))
    assert y.dtype == torch.float32 and t.dtype == torch.float32 and y.is_contiguous() and t.is_contiguous()
    assert dy is None or (dy.dtype == torch.float32 and dy.is_contiguous() and tuple(dy.shape) == (n, h, w, 3))
    m = len(power_factors)
    pf = (ctypes.c_double * m)(*[float(v) for v in power_factors])
    if out is None:
        out = torch.empty((n, 3 + 3 * m), dtype=torch.float64, device=y.device)
    ws = workspace(msssim_workspace_bytes(n, h, w, m, dy is not None), y.device)
    call("cnnitmo_msssim_loss_grad", base, float(alpha), ctypes.addressof(pf), m, float(max_val), ptr(y), ptr(t), n, h,
         w, float(grad_frames), ptr(out), ptr(dy), ws.data_ptr(), ws.numel(), stream_ptr())
    return out


# ---------------------------------------------------------------- highlight-weighted loss
def highlight_workspace_bytes(n, h, w):
    return query("cnnitmo_highlight_workspace_bytes", n, h, w)


def highlight_loss_grad(base, tau, gain, s, y, t, dy=None, grad_frames=0.0, out=None):
    """s (the mask source; may be t), y, t [n,h,w,3] contiguous fp32 device tensors -> out [n,4] fp64 =
    (mean mask, base term, loss, base error inside the highlights) per image; dy (optional, like y) =
    the gradient of the batch-mean loss, normalised by grad_frames (0: n) frames
    (cnnitmo_highlight_loss_grad).  base: the L.DSSIM_BASES id of 'mae' or 'mse'."""
    n, h, w, c = y.shape
    assert c == 3 and tuple(t.shape) == (n, h, w, 3) and tuple(s.shape) == (n, h, w, 3), \
        (tuple(s.shape), tuple(y.shape), tuple(t.shape))
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in (s, y, t))
    assert dy is None or (dy.dtype == torch.float32 and dy.is_contiguous() and tuple(dy.shape) == (n, h, w, 3))
    if out is None:
        out = torch.empty((n, 4), dtype=torch.float64, device=y.device)
    ws = workspace(highlight_workspace_bytes(n, h, w), y.device)
    call("cnnitmo_highlight_loss_grad", base, float(tau), float(gain), ptr(s), ptr(y), ptr(t), n, h, w,
         float(grad_frames), ptr(out), ptr(dy), ws.data_ptr(), ws.numel(), stream_ptr())
    return out


def rgb_accuracy(y, t, count):
    """count (int64 [1], device) += the pixels of y, t [..., 3] whose argmax over RGB agrees."""
    assert y.dtype == torch.float32 and t.dtype == torch.float32 and y.is_contiguous() and t.is_contiguous()
    assert y.shape == t.shape and y.shape[-1] == 3 and count.dtype == torch.int64
    call("cnnitmo_rgb_accuracy", ptr(y), ptr(t), y.numel() // 3, ptr(count), stream_ptr())
    return count


# ---------------------------------------------------------------- RGBE codec
def _rgbe_pair(rgb, rgbe):
    assert rgb.dtype == torch.float32 and rgbe.dtype == torch.uint8 and rgb.is_contiguous() and rgbe.is_contiguous()
    assert rgb.shape[-1] == 3 and rgbe.shape[-1] == 4 and rgb.shape[:-1] == rgbe.shape[:-1], \
        (tuple(rgb.shape), tuple(rgbe.shape))
    return rgb.numel() // 3


def rgbe_encode(rgb, rgbe):
    """rgb [...,3] fp32 -> rgbe [...,4] uint8, contiguous device tensors (cnnitmo_rgbe_encode).  Views
    that do not start on a 16-byte boundary take the kernel's one-pixel path: same bytes."""
    call("cnnitmo_rgbe_encode", ptr(rgb), _rgbe_pair(rgb, rgbe), ptr(rgbe), stream_ptr())
    return rgbe


def rgbe_decode(rgbe, rgb):
    """rgbe [...,4] uint8 -> rgb [...,3] fp32, contiguous device tensors (cnnitmo_rgbe_decode)."""
    call("cnnitmo_rgbe_decode", ptr(rgbe), _rgbe_pair(rgb, rgbe), ptr(rgb), stream_ptr())
    return rgb


# ---------------------------------------------------------------- HDR pair generator
# cnnitmo_hdr_src: pointer, h, w, fmt, r0, c0, r1, c1 (+ 4 bytes of tail padding)
HDR_SRC = np.dtype({"names": ["pix", "h", "w", "fmt", "r0", "c0", "r1", "c1"],
                    "formats": ["<u8"] + ["<i4"] * 7, "offsets": [0, 8, 12, 16, 20, 24, 28, 32], "itemsize": 40})


def hdr_descriptors(sources, windows=None):
    """Host array (HDR_SRC, one per output frame) for cnnitmo_hdr_pairs.  sources: contiguous device
    tensors, fp32 [h,w,3] or RGBE uint8 [h,w,4] (the caller keeps them alive); windows: per frame the
    inclusive clamp window (r0, c0, r1, c1), None = the whole picture.  The descriptors are read on
    the device, so their contents are checked here."""
    d = np.zeros(len(sources), HDR_SRC)
    for i, t in enumerate(sources):
        if t.ndim != 3 or not t.is_contiguous() or (t.dtype, t.shape[2]) not in ((torch.float32, 3), (torch.uint8, 4)):
            raise ValueError(f"hdr source {i}: expected contiguous fp32 [h,w,3] or uint8 [h,w,4], got "
                             f"{t.dtype} {tuple(t.shape)}")
        h, w = int(t.shape[0]), int(t.shape[1])
        if h < 1 or w < 1:
            raise ValueError(f"hdr source {i}: empty picture {h} x {w}")
        win = None if windows is None else windows[i]
        r0, c0, r1, c1 = (0, 0, h - 1, w - 1) if win is None else (int(v) for v in win)
        if not (0 <= r0 <= r1 < h and 0 <= c0 <= c1 < w):
            raise ValueError(f"hdr source {i}: window rows {r0}..{r1}, columns {c0}..{c1} is not inside the "
                             f"{h} x {w} picture")
        d[i] = (t.data_ptr(), h, w, 0 if t.dtype == torch.float32 else 1, r0, c0, r1, c1)
    return d


def hdr_pairs_workspace_bytes(n):
    return int(query("cnnitmo_hdr_pairs_workspace_bytes", n))


def hdr_pairs(srcs, mats, flips, cam, x, y, key=0.18, lum=None, quantize=0, warped=None, logsum=None, ws=None):
    """srcs: device uint8 tensor holding n HDR_SRC descriptors (hdr_descriptors, uploaded); mats [n,6]
    fp64, flips [n] int32, cam [n,3] fp64 device tensors; x, y (and warped) [n,h,w,3] fp32, logsum [n]
    fp64 (cnnitmo_hdr_pairs).  lum: three host weights, None = Rec. 709."""
    import ctypes
    n, h, w, _ = x.shape
    assert srcs.dtype == torch.uint8 and srcs.numel() == n * HDR_SRC.itemsize and srcs.data_ptr() % 8 == 0
    assert mats.dtype == torch.float64 and mats.numel() == 6 * n and flips.dtype == torch.int32 and flips.numel() == n
    assert cam.dtype == torch.float64 and cam.numel() == 3 * n
    for t in (x, y, warped):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n, h, w, 3))
    assert logsum is None or (logsum.dtype == torch.float64 and logsum.numel() == n)
    if ws is None:
        ws = workspace(hdr_pairs_workspace_bytes(n), x.device)
    lc = None if lum is None else (ctypes.c_double * 3)(*[float(c) for c in lum])
    call("cnnitmo_hdr_pairs", ptr(srcs), n, h, w, ptr(mats), ptr(flips), None if lc is None else ctypes.addressof(lc),
         float(key), ptr(cam), int(quantize), ptr(x), ptr(y), ptr(warped), ptr(logsum), ptr(ws), ws.numel(),
         stream_ptr())
    return x, y


HDR_RESPONSES = {"luminance": 0, "channel": 1}


def _noise_pair(noise, keys, n):
    assert noise.dtype == torch.float64 and noise.is_contiguous() and noise.numel() == 2 * n, \
        (noise.dtype, tuple(noise.shape))
    assert keys is not None and keys.dtype in (torch.int64, torch.uint64) and keys.is_contiguous() and \
        keys.numel() == 2 * n, "keys: [n,2] 64-bit integers, one pair per frame"
    assert noise.data_ptr() % 8 == 0 and keys.data_ptr() % 8 == 0


def hdr_pairs_sensor(srcs, mats, flips, cam, x, y, key=0.18, lum=None, quantize=0, response=0, noise=None, keys=None,
                     warped=None, logsum=None, ws=None):
    """hdr_pairs with a sensor in front of the camera curve (cnnitmo_hdr_pairs_sensor).  response: 0 =
    the curve on the luminance (hdr_pairs' bits), 1 = on every channel's own exposure; noise [n,2] fp64
    = (shot factor a, read sigma b) per frame, both >= 0, None = no noise (needs response 1); keys
    [n,2] int64 / uint64 = the frames' Philox keys, as 64-bit patterns.  All device tensors."""
    import ctypes
    n, h, w, _ = x.shape
    assert srcs.dtype == torch.uint8 and srcs.numel() == n * HDR_SRC.itemsize and srcs.data_ptr() % 8 == 0
    assert mats.dtype == torch.float64 and mats.numel() == 6 * n and flips.dtype == torch.int32 and flips.numel() == n
    assert cam.dtype == torch.float64 and cam.numel() == 3 * n
    for t in (x, y, warped):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n, h, w, 3))
    assert logsum is None or (logsum.dtype == torch.float64 and logsum.numel() == n)
    if noise is not None:
        _noise_pair(noise, keys, n)
    if ws is None:
        ws = workspace(hdr_pairs_workspace_bytes(n), x.device)
    lc = None if lum is None else (ctypes.c_double * 3)(*[float(c) for c in lum])
    call("cnnitmo_hdr_pairs_sensor", ptr(srcs), n, h, w, ptr(mats), ptr(flips),
         None if lc is None else ctypes.addressof(lc), float(key), ptr(cam), int(quantize), int(response), ptr(noise),
         ptr(keys) if noise is not None else None, ptr(x), ptr(y), ptr(warped), ptr(logsum), ptr(ws), ws.numel(),
         stream_ptr())
    return x, y


def sensor_noise(e, noise, keys, out=None):
    """e [n,h,w,3] contiguous fp32 device tensor -> out like e (not e itself): e + sqrt(a max(e, 0) +
    b^2) z, unclamped (cnnitmo_sensor_noise).  noise [n,2] fp64 = (a, b) >= 0, keys [n,2] int64 / uint64:
    device tensors; z: the Philox normals of hdr_pairs_sensor."""
    n, h, w, c = e.shape
    assert c == 3 and e.dtype == torch.float32 and e.is_contiguous(), (e.dtype, tuple(e.shape))
    _noise_pair(noise, keys, n)
    if out is None:
        out = torch.empty_like(e)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, h, w, 3)
    assert out.data_ptr() != e.data_ptr()
    call("cnnitmo_sensor_noise", ptr(e), n, h, w, ptr(noise), ptr(keys), ptr(out), stream_ptr())
    return out


# ---------------------------------------------------------------- HDR quality metrics
HDR_ENCODINGS = {"pq": 0, "log": 1}  # CNNITMO_ENC_*


def hdr_encode(encoding, img, scale, out=None):
    """img [n,h,w,3] contiguous fp32, scale [n] fp64 device tensors -> out like img: the PQ / log
    encoding of img * scale (cnnitmo_hdr_encode).  encoding: an HDR_ENCODINGS id."""
    n, h, w, c = img.shape
    assert c == 3 and img.dtype == torch.float32 and img.is_contiguous(), (img.dtype, tuple(img.shape))
    assert scale.dtype == torch.float64 and scale.is_contiguous() and scale.numel() == n
    if out is None:
        out = torch.empty_like(img)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, h, w, 3)
    call("cnnitmo_hdr_encode", int(encoding), ptr(img), n, h, w, ptr(scale), ptr(out), stream_ptr())
    return out


def lum_percentile_workspace_bytes(n):
    return int(query("cnnitmo_lum_percentile_workspace_bytes", n))


def lum_percentile(img, q, lum=None, out=None):
    """img [n,h,w,3] contiguous fp32 device tensor -> out [n] fp32: the histogram percentile Q_q of
    each image's luminance (cnnitmo_lum_percentile).  lum: three host weights, None = Rec. 709."""
    import ctypes
    n, h, w, c = img.shape
    assert c == 3 and img.dtype == torch.float32 and img.is_contiguous(), (img.dtype, tuple(img.shape))
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=img.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n
    ws = workspace(lum_percentile_workspace_bytes(n), img.device)
    lc = None if lum is None else (ctypes.c_double * 3)(*[float(c) for c in lum])
    call("cnnitmo_lum_percentile", ptr(img), n, h, w, None if lc is None else ctypes.addressof(lc), float(q),
         ptr(out), ws.data_ptr(), ws.numel(), stream_ptr())
    return out


# ---------------------------------------------------------------- JPEG round trip
JPEG_SUBSAMPLINGS = {"4:4:4": 0, "4:2:0": 1}


def jpeg_workspace_bytes(n, h, w, subsampling):
    return int(query("cnnitmo_jpeg_workspace_bytes", n, h, w, JPEG_SUBSAMPLINGS[subsampling]))


def jpeg_roundtrip(x, qtabs, subsampling, apply=None, out=None, ws=None):
    """x [n,h,w,3] contiguous fp32 device tensor -> out like x (may be x): the baseline-JPEG round
    trip of uint8(255 x) (cnnitmo_jpeg_roundtrip).  qtabs: HOST uint16 [n,2,64] (numpy), natural order,
    no entry 0; apply: HOST [n] (numpy, nonzero = compress, 0 = copy through), None = all;
    subsampling: '4:4:4' or '4:2:0'."""
    n, h, w, c = x.shape
    assert c == 3 and x.dtype == torch.float32 and x.is_contiguous(), (x.dtype, tuple(x.shape))
    qt = np.ascontiguousarray(qtabs, dtype=np.uint16)
    assert qt.shape == (n, 2, 64), qt.shape
    ap = None if apply is None else np.ascontiguousarray(np.asarray(apply) != 0, dtype=np.uint8)
    assert ap is None or ap.shape == (n,), ap.shape
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, h, w, 3)
    if ws is None:
        ws = workspace(jpeg_workspace_bytes(n, h, w, subsampling), x.device)
    call("cnnitmo_jpeg_roundtrip", ptr(x), n, h, w, JPEG_SUBSAMPLINGS[subsampling], qt.ctypes.data,
         None if ap is None else ap.ctypes.data, ptr(out), ptr(ws), ws.numel(), stream_ptr())
    return out


# ---------------------------------------------------------------- antialiased resampling
RESIZE_FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2, "lanczos": 3}  # CNNITMO_RESIZE_*


def resize_coeffs(n_in, n_out, filt):
    """(bounds int32 [n_out,2] = (xmin, n), kk float64 [n_out,ksize]) of one axis, host arrays, from
    cnnitmo_resize_coeffs: the one source of coefficients (needs no GPU).  filt: a RESIZE_FILTERS id."""
    ksize = query("cnnitmo_resize_coeffs", int(n_in), int(n_out), int(filt), None, None)
    if ksize < 0:
        raise L.CnnItmoError(f"cnnitmo_resize_coeffs({n_in}, {n_out}, {filt}) failed ({ksize}): "
                             f"{query('cnnitmo_last_error').decode(errors='replace')}")
    bounds = np.empty((int(n_out), 2), np.int32)
    kk = np.empty((int(n_out), ksize), np.float64)
    rc = query("cnnitmo_resize_coeffs", int(n_in), int(n_out), int(filt), bounds.ctypes.data, kk.ctypes.data)
    assert rc == ksize, (rc, ksize)
    return bounds, kk


def resize_tile_cols(w, ow, ksize_x):
    """Output columns per tile of the horizontal pass; 0 = its direct (no LDS) path."""
    return int(query("cnnitmo_resize_tile_cols", int(w), int(ow), int(ksize_x)))


def resize_workspace_bytes(dtype, n, h, w, oh, ow):
    return int(query("cnnitmo_resize_workspace_bytes", 0 if dtype == torch.float32 else 1, n, h, w, oh, ow))


def resize(x, out, tab_x, tab_y, lo=float("-inf"), ws=None):
    """x [n,h,w,3] -> out [n,oh,ow,3], contiguous device tensors, both fp32 or both uint8
    (cnnitmo_resize).  tab_x / tab_y: (bounds int32 [o,2], kk float64 [o,ksize]) DEVICE tensors of
    w -> ow / h -> oh, None for an axis that keeps its size."""
    n, h, w, c = x.shape
    oh, ow = int(out.shape[1]), int(out.shape[2])
    assert c == 3 and x.dtype in (torch.float32, torch.uint8) and x.is_contiguous(), (x.dtype, tuple(x.shape))
    assert out.dtype == x.dtype and out.is_contiguous() and tuple(out.shape) == (n, oh, ow, 3), tuple(out.shape)
    args = []
    for tab, o in ((tab_x, ow), (tab_y, oh)):
        if tab is None:
            args += [None, None, 0]
            continue
        b, k = tab
        assert b.dtype == torch.int32 and b.is_contiguous() and tuple(b.shape) == (o, 2), (b.dtype, tuple(b.shape))
        assert k.dtype == torch.float64 and k.is_contiguous() and k.shape[0] == o and k.data_ptr() % 8 == 0
        args += [ptr(b), ptr(k), int(k.shape[1])]
    if ws is None and w != ow and h != oh:
        ws = workspace(resize_workspace_bytes(x.dtype, n, h, w, oh, ow), x.device)
    call("cnnitmo_resize", ptr(x), 0 if x.dtype == torch.float32 else 1, n, h, w, ptr(out), oh, ow, *args,
         float(lo), ptr(ws), stream_ptr())
    return out


# ---------------------------------------------------------------- OpenEXR pixels
EXR_UINT, EXR_HALF, EXR_FLOAT = 0, 1, 2


def exr_segment_bytes():
    """Bytes of a chunk one workgroup of cnnitmo_exr_unpack's scan takes."""
    return int(query("cnnitmo_exr_segment_bytes"))


def exr_workspace_bytes(h, lines_per_chunk, line_bytes):
    return int(query("cnnitmo_exr_workspace_bytes", int(h), int(lines_per_chunk), int(line_bytes)))


def exr_unpack(raw, coded, lines_per_chunk, line_bytes, ch_off, ch_type, rgb, ws=None):
    """raw uint8 [h * line_bytes] -> rgb [h,w,3] fp32, contiguous device tensors (cnnitmo_exr_unpack).
    coded: device uint8 [chunks] or None (every chunk plain); ch_off / ch_type: host triples for
    R, G, B.  ws: device uint8 workspace, allocated here when coded is given and ws is not."""
    h, w, c = rgb.shape
    assert c == 3 and rgb.dtype == torch.float32 and rgb.is_contiguous(), (rgb.dtype, tuple(rgb.shape))
    assert raw.dtype == torch.uint8 and raw.is_contiguous() and raw.numel() == h * int(line_bytes), \
        (raw.dtype, raw.numel(), h, line_bytes)
    if coded is not None:
        assert coded.dtype == torch.uint8 and coded.is_contiguous() and \
            coded.numel() * int(lines_per_chunk) >= h, (coded.dtype, coded.numel())
        if ws is None:
            ws = workspace(exr_workspace_bytes(h, lines_per_chunk, line_bytes), raw.device)
    off = (ctypes.c_int * 3)(*[int(v) for v in ch_off])
    typ = (ctypes.c_int * 3)(*[int(v) for v in ch_type])
    call("cnnitmo_exr_unpack", ptr(raw), ptr(coded), h, w, int(lines_per_chunk), int(line_bytes), off, typ,
         ptr(rgb), ptr(ws), 0 if ws is None else ws.numel(), stream_ptr())
    return rgb


def exr_pack(rgb, pixel_type, lines_per_chunk, coded, out):
    """rgb [h,w,3] fp32 -> out uint8 [h * 3 * w * size]: lines of B, G, R values of pixel_type
    (EXR_HALF / EXR_FLOAT), every chunk split and predicted when coded (cnnitmo_exr_pack)."""
    h, w, c = rgb.shape
    size = 2 if pixel_type == EXR_HALF else 4
    assert c == 3 and rgb.dtype == torch.float32 and rgb.is_contiguous(), (rgb.dtype, tuple(rgb.shape))
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == h * 3 * w * size, \
        (out.dtype, out.numel())
    call("cnnitmo_exr_pack", ptr(rgb), h, w, int(pixel_type), int(lines_per_chunk), int(bool(coded)), ptr(out),
         stream_ptr())
    return out
