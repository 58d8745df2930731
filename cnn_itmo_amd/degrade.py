"""Degradations of SDR inputs on the GPU: the baseline-JPEG round trip.

The SDR pictures an inverse tone-mapping network meets have been through JPEG; a network trained on
clean quantised inputs expands their blocking and ringing into the highlights it invents.
``jpeg_roundtrip`` puts frames through the pixel path of a JPEG file -- colour transform, chroma
subsampling, 8x8 DCT, quantisation and the whole way back, the IJG library's integer arithmetic
(cnnitmo_jpeg_roundtrip, csrc/jpeg.hip; entropy coding is lossless and left out) -- without a pixel
touching the host:

    x = degrade.jpeg_roundtrip(x, quality=[30, 75, 90, 50])        # one quality per image
    x = degrade.jpeg_roundtrip(frame_u8, 60, subsampling="4:4:4")  # uint8 in, uint8 out

``HDRPairGenerator(jpeg_quality=...)`` applies it to the training inputs it makes.
"""
from __future__ import annotations

import numpy as np

SUBSAMPLINGS = ("4:4:4", "4:2:0")

# Annex K of ITU-T T.81, natural (row-major) order
LUMINANCE = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CHROMINANCE = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def check_quality(quality):
    """quality as an int in 1..100, ValueError otherwise."""
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"JPEG quality {quality!r}: an integer in 1..100")
    return q


def quant_tables(quality):
    """uint16 [2, 64]: the luminance and the chrominance table of a libjpeg quality (1..100), scaled as
    jpeg_quality_scaling does: s = 5000 // q below 50, else 200 - 2 q; clamp((base s + 50) // 100, 1, 255)."""
    q = check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([LUMINANCE, CHROMINANCE], np.int64)
    return np.clip((base * s + 50) // 100, 1, 255).astype(np.uint16)


def jpeg_roundtrip(x, quality=75, subsampling="4:2:0"):
    """x: numpy array or CUDA tensor, [h,w,3] or [n,h,w,3]; float in [0, 1] (returns an fp32 CUDA
    tensor on the 8-bit levels k/255) or uint8 (returns a uint8 CUDA tensor).  quality: an int or one per
    image.  Nothing synchronises with the host."""
    import torch
    from . import ops
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling {subsampling!r}: '4:4:4' or '4:2:0'")
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.ndim not in (3, 4) or t.shape[-1] != 3 or t.numel() == 0:
        raise ValueError(f"jpeg_roundtrip: expected [h,w,3] or [n,h,w,3], got {tuple(t.shape)}")
    if t.dtype != torch.uint8 and not t.dtype.is_floating_point:
        raise ValueError(f"jpeg_roundtrip: expected a float or uint8 image, got {t.dtype}")
    single, as_u8 = t.ndim == 3, t.dtype == torch.uint8
    t = t.cuda()
    if single:
        t = t[None]
    n = t.shape[0]
    qs = [quality] * n if np.ndim(quality) == 0 else list(quality)
    if len(qs) != n:
        raise ValueError(f"jpeg_roundtrip: {len(qs)} qualities for {n} images")
    qt = np.stack([quant_tables(q) for q in qs])
    # a uint8 level k is handed over as (float)k * (float)(1/255.), the kernel's own stored form: step 1 gives k back
    f = t.to(torch.float32)
    out = ops.jpeg_roundtrip((f * (1 / 255.) if as_u8 else f).contiguous(), qt, subsampling)
    if as_u8:
        out = torch.round(out * 255.0).to(torch.uint8)
    return out[0] if single else out
