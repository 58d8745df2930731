"""PSNR and SSIM of image batches on the GPU (csrc/metrics.hip behind the C ABI).

  psnr(a, b, max_val=1.0)      -> [n] dB     tf.image.psnr: 10 log10(max_val^2 / mse), +inf for mse 0
  ssim(a, b, max_val=1.0)      -> [n]        tf.image.ssim defaults (Wang et al. 2004): 11x11 Gaussian
                                             window, sigma 1.5, valid positions, K1 0.01, K2 0.03
  psnr_ssim(a, b, max_val=1.0) -> ([n], [n]) both from one pass over the images
  ms_ssim(a, b, max_val=1.0, power_factors=None)
                               -> [n]        tf.image.ssim_multiscale (Wang et al. 2003): the product
                                             over up to five scales, each the 2x2 mean of the one
                                             before, of the per-channel contrast-structure means
                                             (SSIM at the coarsest) raised to the power factors, then
                                             the mean over channels; images of at least 161 x 161
                                             pixels for the default five scales (csrc/msssim.hip)

Inputs: numpy arrays or CUDA tensors, ``[h,w,3]`` or ``[n,h,w,3]``, float or uint8.
uint8 becomes fp32 0..255 and ``max_val`` is used as given (pass 255 for 8-bit
images).  Outputs: float64 CUDA tensors, one value per image, like
``tonemap.log_average``; nothing synchronises with the host.  SSIM needs images
of at least 11 x 11 pixels.

``Model.compile(metrics=[...])`` takes ``'psnr'`` / ``'ssim'`` / ``'ms_ssim'`` (or these functions)
for ``evaluate`` and the validation logs of ``fit`` / ``fit_generator``.
"""
from __future__ import annotations

from .tonemap import _dev

WINDOW = 11


def _pair(a, b):
    import torch
    a, b = _dev(a, torch.float32), _dev(b, torch.float32)
    if a.shape != b.shape:
        raise ValueError(f"image batches differ in shape: {tuple(a.shape)} vs {tuple(b.shape)}")
    return a, b


def _run(what, a, b, max_val):
    from . import ops
    a, b = _pair(a, b)
    if what & ops.SSIM and (a.shape[1] < WINDOW or a.shape[2] < WINDOW):
        raise ValueError(f"ssim needs images of at least {WINDOW} x {WINDOW} pixels, got "
                         f"{a.shape[1]} x {a.shape[2]}")
    return ops.image_metrics(what, a, b, max_val)


def mse(a, b):
    """Mean squared error per image, float64 [n]."""
    from . import ops
    return _run(ops.MSE_PSNR, a, b, 1.0)[:, 0]


def psnr(a, b, max_val=1.0):
    """Peak signal-to-noise ratio per image in dB, float64 [n]."""
    from . import ops
    return _run(ops.MSE_PSNR, a, b, max_val)[:, 1]


def ssim(a, b, max_val=1.0):
    """Structural similarity per image, float64 [n]."""
    from . import ops
    return _run(ops.SSIM, a, b, max_val)[:, 2]


def ms_ssim(a, b, max_val=1.0, power_factors=None):
    """Multi-scale structural similarity per image, float64 [n] (tf.image.ssim_multiscale):
    power_factors are the weights of 1..5 scales, used as given (None: TensorFlow's five).  Each
    scale is the 2x2 mean of the one before; the coarsest must hold the 11 x 11 window."""
    from . import losses, ops
    w = losses.check_power_factors(power_factors)
    a, b = _pair(a, b)
    need = losses.min_side(len(w))
    if a.shape[1] < need or a.shape[2] < need:
        raise ValueError(f"ms_ssim with {len(w)} scales needs images of at least {need} x {need} pixels, got "
                         f"{a.shape[1]} x {a.shape[2]}")
    return ops.msssim_loss_grad(0, 1.0, w, a, b, max_val=max_val)[:, 0]


def psnr_ssim(a, b, max_val=1.0):
    """(psnr, ssim) per image from one pass over the images."""
    from . import ops
    out = _run(ops.MSE_PSNR | ops.SSIM, a, b, max_val)
    return out[:, 1], out[:, 2]
