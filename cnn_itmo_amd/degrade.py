"""Degradations of SDR inputs on the GPU: the baseline-JPEG round trip and sensor noise.

The SDR pictures an inverse tone-mapping network meets have been through JPEG; a network trained on
clean quantised inputs expands their blocking and ringing into the highlights it invents.
``jpeg_roundtrip`` puts frames through the pixel path of a JPEG file -- colour transform, chroma
subsampling, 8x8 DCT, quantisation and the whole way back, the IJG library's integer arithmetic
(cnnitmo_jpeg_roundtrip, csrc/jpeg.hip; entropy coding is lossless and left out) -- without a pixel
touching the host:

    x = degrade.jpeg_roundtrip(x, quality=[30, 75, 90, 50])        # one quality per image
    x = degrade.jpeg_roundtrip(frame_u8, 60, subsampling="4:4:4")  # uint8 in, uint8 out

``HDRPairGenerator(jpeg_quality=...)`` applies it to the training inputs it makes.

Real SDR material also carries signal-dependent sensor noise, strongest in the shadows, which a
network that has never seen it expands into its HDR output.  ``sensor_noise`` adds the
Poisson-Gaussian model ``e + sqrt(shot max(e, 0) + read^2) z`` to a linear image, with normals from a
counter-based generator inside the kernel (Philox4x64-10; cnnitmo_sensor_noise, csrc/sensor_px.h), so the
noise of an image depends on its key alone:

    noisy = degrade.sensor_noise(exposure, shot=1e-3, read=2e-3, key=[7, 8, 9, 10])   # one key per image

``HDRPairGenerator(response='channel', noise_shot=..., noise_read=...)`` applies the same arithmetic to
the channel exposures in front of its camera curve.
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


def noise_keys(key, n, single=False):
    """uint64 [n, 2]: the Philox keys of n images.  key: an int in [0, 2^64) (the key is (key, 0), for
    every image), one int per image, or [n, 2] pairs; for a single unbatched image also one pair."""
    k = np.asarray(key, dtype=object)
    if k.ndim == 1 and single and k.shape[0] == 2:
        k = k[None]
    if k.ndim == 0:
        k = np.array([[key, 0]] * n, dtype=object)
    elif k.ndim == 1:
        k = np.array([[v, 0] for v in k], dtype=object).reshape(-1, 2)
    if k.shape != (n, 2):
        raise ValueError(f"sensor_noise: key of shape {np.shape(key)} for {n} image(s): an int, one per image or "
                         f"[n, 2] pairs")
    out = np.empty((n, 2), np.uint64)
    for i in range(n):
        for j in range(2):
            v = k[i, j]
            if int(v) != v or not 0 <= int(v) < 1 << 64:
                raise ValueError(f"sensor_noise: key word {v!r}: an integer in [0, 2^64)")
            out[i, j] = int(v)
    return out


def noise_levels(shot, read, n):
    """float64 [n, 2] = (a, b) per image from scalars or one value per image; both finite and >= 0."""
    ab = np.empty((n, 2), np.float64)
    for j, (name, v) in enumerate((("shot", shot), ("read", read))):
        v = np.asarray(v, np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != n):
            raise ValueError(f"sensor_noise: {v.shape[0] if v.ndim == 1 else v.shape} {name} values for {n} image(s)")
        if not (np.isfinite(v).all() and (v >= 0).all()):
            raise ValueError(f"sensor_noise: {name} {v.tolist()!r}: finite and >= 0")
        ab[:, j] = v
    return ab


def sensor_noise(e, shot, read, key):
    """Poisson-Gaussian sensor noise on a linear image: e + sqrt(shot max(e, 0) + read^2) z, unclamped,
    with e in units of full well, ``shot`` the shot-noise factor (1 / full-well electrons) and
    ``read`` the read-noise standard deviation.  e: fp32 [h,w,3] or [n,h,w,3], numpy array or tensor;
    shot, read: scalars or one per image; key: see ``noise_keys``.  z are standard normals from
    Philox4x64-10 (numpy's ``np.random.Philox``) keyed per image and counted by the pixel's index in
    its image (cnnitmo_sensor_noise, csrc/sensor_px.h), so an image and a key give the same noise in any
    batch, on any rank.  Returns an fp32 CUDA tensor; nothing synchronises with the host."""
    import torch
    from . import ops
    t = e if isinstance(e, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(e))
    if t.ndim not in (3, 4) or t.shape[-1] != 3 or t.numel() == 0:
        raise ValueError(f"sensor_noise: expected [h,w,3] or [n,h,w,3], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"sensor_noise: expected an fp32 image, got {t.dtype}")
    single = t.ndim == 3
    t = t.cuda().contiguous()
    if single:
        t = t[None]
    n = t.shape[0]
    ab, keys = noise_levels(shot, read, n), noise_keys(key, n, single)
    # one upload: the levels, then the keys (8-byte items)
    dev = torch.from_numpy(np.concatenate([ab.view(np.uint8).reshape(-1), keys.view(np.uint8).reshape(-1)])).cuda()
    out = ops.sensor_noise(t, dev[:16 * n].view(torch.float64), dev[16 * n:].view(torch.int64))
    return out[0] if single else out


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
