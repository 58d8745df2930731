"""PSNR and SSIM of an HDR reconstruction against its HDR reference, on the GPU
(csrc/hdrmetrics.hip and csrc/metrics.hip behind the C ABI).

Linear radiance has an arbitrary overall scale and no perceptual meaning, so both images are
first aligned, anchored to display luminance (cd/m^2) and perceptually encoded; PSNR / SSIM are
then those of ``metrics.py`` on the encoded planes with ``max_val=1``.  Per image pair (P the
prediction, R the reference, Y the luminance with the ``lum`` weights, fp64 throughout):

  1. align P to R      ``align='logmean'``  s = G(R)/G(P), G = ``tonemap.log_average``
                       ``align='median'``   s = Q_0.5(R)/Q_0.5(P)  (for images with zeros, which
                                            wreck a log-average; granularity 1/64 octave)
                       ``align='none'``     s = 1
  2. anchor to cd/m^2  ``anchor='key'``         k = key * white_nits / G(R)   (0.18, 203.0: the
                                                Reinhard key on BT.2408 reference white)
                       ``anchor='percentile'``  k = peak_nits / Q_q(R)        (0.999, 1000.0)
                       ``anchor=<float>``       k = that value, for calibrated files
     scale_pred = s * k, scale_ref = k
  3. encode x = v * scale per channel value
                       ``'pq'``   SMPTE ST 2084 of min(max(x, 0), 1e4)
                       ``'log'``  (log10 L - log10 0.005) / (4 - log10 0.005), L = min(max(x, 0.005), 1e4)
  4. PSNR / SSIM of the two encoded fp32 planes, max_val 1.

Q_q is a histogram percentile on the float bits of the luminance (4096 bins: 64 octaves from
2^-32 to 2^32, 64 bins each); it is the upper edge of the bin that holds the order statistic of
rank max(1, ceil(q h w)), so it is at or above it by less than a factor 1 + 1/64.

  encode(img, encoding='pq', scale=1.0)             -> float32 like img
  luminance_percentile(img, q=0.999, lum=None)      -> float32 [n]
  hdr_scales(pred, ref, align=, anchor=, ...)       -> (scale_pred, scale_ref) float64 [n]
  hdr_psnr_ssim(pred, ref, encoding='pq', ...)      -> (psnr [n], ssim [n]) float64
  hdr_psnr, hdr_ssim                                -> one of them
  hdr_ms_ssim(pred, ref, encoding='pq', power_factors=None, ...)
                                                    -> metrics.ms_ssim of the encoded planes [n]

Inputs as in ``metrics.py``: numpy arrays or CUDA tensors, ``[h,w,3]`` or ``[n,h,w,3]``.  Every
result is a CUDA tensor; the scales are formed from the device-side statistics with torch ops and
nothing synchronises with the host.  SSIM needs images of at least 11 x 11 pixels, MS-SSIM with
its default five scales 161 x 161.
"""
from __future__ import annotations

from .metrics import WINDOW, _pair
from .tonemap import _dev

ENCODINGS = ("pq", "log")
ALIGNS = ("logmean", "median", "none")
ANCHORS = ("key", "percentile")


def _encoding_id(encoding):
    from . import ops
    if encoding not in ops.HDR_ENCODINGS:
        raise ValueError(f"encoding {encoding!r} (one of {', '.join(ENCODINGS)})")
    return ops.HDR_ENCODINGS[encoding]


def _scale_tensor(scale, n, device):
    import torch
    s = torch.as_tensor(scale, dtype=torch.float64).to(device).reshape(-1)
    if s.numel() == 1:
        s = s.expand(n)
    if s.numel() != n:
        raise ValueError(f"scale has {s.numel()} values for {n} images")
    return s.contiguous()


def encode(img, encoding="pq", scale=1.0):
    """The perceptual encoding of ``img * scale`` (cd/m^2), float32 like img.  ``scale``: one
    value, or one per image (array or tensor)."""
    import torch
    from . import ops
    enc = _encoding_id(encoding)
    x = _dev(img, torch.float32)
    return ops.hdr_encode(enc, x, _scale_tensor(scale, x.shape[0], x.device))


def luminance_percentile(img, q=0.999, lum=None):
    """The histogram percentile Q_q of each image's luminance, float32 [n]."""
    import torch
    from . import ops
    q = float(q)
    if not 0.0 < q <= 1.0:
        raise ValueError(f"percentile q {q!r} outside (0, 1]")
    return ops.lum_percentile(_dev(img, torch.float32), q, lum)


def _anchor(anchor):
    """'key', 'percentile' or a positive float (also as a string, for the command lines)."""
    if anchor in ANCHORS:
        return anchor
    try:
        k = float(anchor)
    except (TypeError, ValueError):
        k = float("nan")
    if not 0.0 < k < float("inf"):
        raise ValueError(f"anchor {anchor!r} ('key', 'percentile' or a positive number of cd/m^2 per unit)")
    return k


def _scales(p, r, align, anchor, key, white_nits, q, peak_nits, lum):
    import torch
    from . import tonemap
    if align not in ALIGNS:
        raise ValueError(f"align {align!r} (one of {', '.join(ALIGNS)})")
    anchor = _anchor(anchor)
    n = r.shape[0]
    g_ref = tonemap.log_average(r, lum) if align == "logmean" or anchor == "key" else None
    if align == "logmean":
        s = g_ref / tonemap.log_average(p, lum)
    elif align == "median":
        s = luminance_percentile(r, 0.5, lum).double() / luminance_percentile(p, 0.5, lum).double()
    else:
        s = torch.ones(n, dtype=torch.float64, device=r.device)
    if anchor == "key":
        k = (float(key) * float(white_nits)) / g_ref
    elif anchor == "percentile":
        k = float(peak_nits) / luminance_percentile(r, q, lum).double()
    else:
        k = torch.full((n,), anchor, dtype=torch.float64, device=r.device)
    return (s * k).contiguous(), k.contiguous()


def hdr_scales(pred, ref, align="logmean", anchor="key", key=0.18, white_nits=203.0, q=0.999, peak_nits=1000.0,
               lum=None):
    """(scale_pred, scale_ref): cd/m^2 per unit of the prediction and of the reference, float64 [n]."""
    p, r = _pair(pred, ref)
    return _scales(p, r, align, anchor, key, white_nits, q, peak_nits, lum)


def _score(what, pred, ref, encoding, align="logmean", anchor="key", key=0.18, white_nits=203.0, q=0.999,
           peak_nits=1000.0, lum=None):
    """(out [n,3] = (mse, psnr, ssim) of the encoded planes, scale_pred, scale_ref)"""
    from . import ops
    enc = _encoding_id(encoding)
    p, r = _pair(pred, ref)
    if what & ops.SSIM and (p.shape[1] < WINDOW or p.shape[2] < WINDOW):
        raise ValueError(f"ssim needs images of at least {WINDOW} x {WINDOW} pixels, got "
                         f"{p.shape[1]} x {p.shape[2]}")
    sp, sr = _scales(p, r, align, anchor, key, white_nits, q, peak_nits, lum)
    out = ops.image_metrics(what, ops.hdr_encode(enc, p, sp), ops.hdr_encode(enc, r, sr), 1.0)
    return out, sp, sr


def hdr_psnr_ssim(pred, ref, encoding="pq", **kw):
    """(psnr dB, ssim) per image of the aligned, anchored and encoded pair; the keywords are
    ``hdr_scales``'."""
    from . import ops
    out = _score(ops.MSE_PSNR | ops.SSIM, pred, ref, encoding, **kw)[0]
    return out[:, 1], out[:, 2]


def hdr_psnr(pred, ref, encoding="pq", **kw):
    """Peak signal-to-noise ratio per image in dB of the encoded pair, float64 [n]."""
    from . import ops
    return _score(ops.MSE_PSNR, pred, ref, encoding, **kw)[0][:, 1]


def hdr_ms_ssim(pred, ref, encoding="pq", power_factors=None, align="logmean", anchor="key", key=0.18,
                white_nits=203.0, q=0.999, peak_nits=1000.0, lum=None):
    """Multi-scale structural similarity per image of the encoded pair (metrics.ms_ssim with
    max_val 1: the same align / anchor / encode as hdr_ssim), float64 [n]."""
    from . import losses, metrics, ops
    enc = _encoding_id(encoding)
    p, r = _pair(pred, ref)
    need = losses.min_side(len(losses.check_power_factors(power_factors)))
    if p.shape[1] < need or p.shape[2] < need:  # (before any kernel runs, as for ssim)
        raise ValueError(f"ms_ssim needs images of at least {need} x {need} pixels, got {p.shape[1]} x {p.shape[2]}")
    sp, sr = _scales(p, r, align, anchor, key, white_nits, q, peak_nits, lum)
    return metrics.ms_ssim(ops.hdr_encode(enc, p, sp), ops.hdr_encode(enc, r, sr), 1.0, power_factors)


def hdr_ssim(pred, ref, encoding="pq", **kw):
    """Structural similarity per image of the encoded pair, float64 [n]."""
    from . import ops
    return _score(ops.SSIM, pred, ref, encoding, **kw)[0][:, 2]
