"""numpy float64 reference of the image metrics (tf.image.psnr / tf.image.ssim defaults).

Inputs [n,h,w,3] (or [h,w,3]); every result is per image, float64 [n].
SSIM: 11x11 Gaussian window (sigma 1.5, 1-D taps exp(-x^2/4.5) normalised to sum 1,
2-D window their outer product), valid positions only, K1 0.01, K2 0.03, biased
weighted moments, mean over the (h-10)(w-10) positions and the 3 channels.
"""
import numpy as np

SIZE, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03


def taps():
    x = np.arange(SIZE, dtype=np.float64) - SIZE // 2
    g = np.exp(-(x * x) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def _batch(a):
    a = np.asarray(a, dtype=np.float64)
    return a[None] if a.ndim == 3 else a


def _filter_valid(x, g):
    """Separable valid filtering of [n,h,w,c] along h then w."""
    n, h, w, c = x.shape
    k = len(g)
    v = sum(g[i] * x[:, i:h - k + 1 + i] for i in range(k))
    return sum(g[j] * v[:, :, j:w - k + 1 + j] for j in range(k))


def mse(a, b):
    a, b = _batch(a), _batch(b)
    return ((a - b) ** 2).mean(axis=(1, 2, 3))


def psnr(a, b, max_val=1.0):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(float(max_val) ** 2 / mse(a, b))


def ssim_map(a, b, max_val=1.0, filt=_filter_valid):
    a, b = _batch(a), _batch(b)
    if a.shape[1] < SIZE or a.shape[2] < SIZE:
        raise ValueError(f"ssim needs at least {SIZE} x {SIZE} pixels, got {a.shape[1]} x {a.shape[2]}")
    g = taps()
    c1, c2 = (K1 * max_val) ** 2, (K2 * max_val) ** 2
    mx, my = filt(a, g), filt(b, g)
    vx = filt(a * a, g) - mx * mx
    vy = filt(b * b, g) - my * my
    cxy = filt(a * b, g) - mx * my
    return ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def ssim(a, b, max_val=1.0):
    return ssim_map(a, b, max_val).mean(axis=(1, 2, 3))


def make_pair(shape, seed, noise=0.03):
    """The GPU tests' images: target = smooth sinusoid + N(0, 0.05) quantised to /255,
    prediction = target + N(0, noise) clipped to [0, 1]; fp32 [n,h,w,3].  ``noise`` may be
    one level or one per image."""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    yy, xx, cc = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    base = 0.5 + 0.35 * np.sin(0.11 * yy + 0.07 * xx + 1.3 * cc) * np.cos(0.05 * xx - 0.03 * yy)
    t = base[None] + rng.normal(0.0, 0.05, (n, h, w, 3))
    t = np.round(np.clip(t, 0.0, 1.0) * 255.0) / 255.0
    lv = np.broadcast_to(np.asarray(noise, np.float64), (n,)).reshape(n, 1, 1, 1)
    p = np.clip(t + rng.normal(0.0, 1.0, (n, h, w, 3)) * lv, 0.0, 1.0)
    return p.astype(np.float32), t.astype(np.float32)
