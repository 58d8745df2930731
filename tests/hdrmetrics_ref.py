"""numpy float64 reference of the HDR quality metrics (cnn_itmo_amd/hdrmetrics.py).

A restatement of the definition: align the prediction P to the reference R, anchor both to
cd/m^2, encode every channel value (float64, then one cast to float32), PSNR / SSIM of the
encoded planes with max_val 1 (tests/metrics_ref.py).  Luminance and the log-average are
oracle.tonemap_ref's.  The clamps are np.fmax / np.fmin (NaN -> the bound), not np.clip.
"""
import numpy as np

import metrics_ref as MR
from oracle import tonemap_ref as TR

M1, M2 = 2610 / 16384, 2523 / 4096 * 128
C1, C2, C3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
PEAK, LOG_FLOOR = 1e4, 0.005
BINS = 4096
BASE = int(np.float32(2.0 ** -32).view(np.uint32)) >> 17


def _batch(a):
    """[n,h,w,3]; the images are fp32 by definition, float64 input is taken as it is (for checks of
    the reference itself that need products no fp32 image holds)."""
    a = np.asarray(a)
    if a.dtype != np.float64:
        a = a.astype(np.float32)
    return a[None] if a.ndim == 3 else a


def pq(x):
    """SMPTE ST 2084 of cd/m^2 (float64 in, float64 out)."""
    with np.errstate(invalid="ignore"):
        y = np.fmin(np.fmax(np.asarray(x, np.float64), 0.0), PEAK) / PEAK
    yp = y ** M1
    return ((C1 + C2 * yp) / (1.0 + C3 * yp)) ** M2


def log_encoding(x):
    with np.errstate(invalid="ignore"):
        L = np.fmin(np.fmax(np.asarray(x, np.float64), LOG_FLOOR), PEAK)
    return (np.log10(L) - np.log10(LOG_FLOOR)) / (4.0 - np.log10(LOG_FLOOR))


ENCODINGS = {"pq": pq, "log": log_encoding}


def encode(img, encoding="pq", scale=1.0):
    """float32 [n,h,w,3]: the encoding of (double)v * scale, scale one value or one per image."""
    img = _batch(img)
    s = np.broadcast_to(np.asarray(scale, np.float64).reshape(-1), (img.shape[0],)).reshape(-1, 1, 1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return ENCODINGS[encoding](img.astype(np.float64) * s).astype(np.float32)


def lum_bins(img, lum=TR.REC709):
    """Histogram bin of every pixel's luminance, on the bits of (float)Y."""
    with np.errstate(invalid="ignore", over="ignore"):
        Y = TR.rgb2lum(np.asarray(img).astype(np.float64), lum)
        Yf = Y.astype(np.float32)
    u = Yf.view(np.uint32).astype(np.int64)
    b = np.clip((u >> 17) - BASE, 0, BINS - 1)
    b[np.isnan(Yf) | (u >> 31 != 0)] = 0  # NaN of either sign, negatives, -0
    return b


def percentile(img, q=0.999, lum=TR.REC709):
    """Q_q per image, float32 [n]: the upper edge of the first bin whose cumulative count reaches
    max(1, ceil(q h w))."""
    img = _batch(img)
    n, h, w, _ = img.shape
    need = max(1, int(np.ceil(q * h * w)))
    out = np.empty(n, np.float32)
    for i in range(n):
        cum = np.cumsum(np.bincount(lum_bins(img[i], lum).reshape(-1), minlength=BINS))
        b = int(np.searchsorted(cum, need, side="left"))
        out[i] = np.uint32((b + 1 + BASE) << 17).view(np.float32)
    return out


def log_average(img, lum=TR.REC709):
    img = _batch(img)
    return np.array([TR.log_average(TR.rgb2lum(im, lum)) for im in img])


def scales(pred, ref, align="logmean", anchor="key", key=0.18, white_nits=203.0, q=0.999, peak_nits=1000.0,
           lum=TR.REC709):
    """(scale_pred, scale_ref), float64 [n]."""
    p, r = _batch(pred), _batch(ref)
    if align == "logmean":
        s = log_average(r, lum) / log_average(p, lum)
    elif align == "median":
        s = percentile(r, 0.5, lum).astype(np.float64) / percentile(p, 0.5, lum).astype(np.float64)
    else:
        assert align == "none"
        s = np.ones(r.shape[0])
    if anchor == "key":
        k = (key * white_nits) / log_average(r, lum)
    elif anchor == "percentile":
        k = peak_nits / percentile(r, q, lum).astype(np.float64)
    else:
        k = np.full(r.shape[0], float(anchor))
    return s * k, k


def psnr_ssim(pred, ref, encoding="pq", **kw):
    sp, sr = scales(pred, ref, **kw)
    ep, er = encode(pred, encoding, sp), encode(ref, encoding, sr)
    return MR.psnr(ep, er), MR.ssim(ep, er)


def make_pair(shape, seed, level=0.1):
    """(prediction, reference) fp32 [n,h,w,3]: the reference spans +-7 stops (2^(7 * smooth
    sinusoid + N(0, 0.3))), the prediction is the reference x 2^(N(0, 1) * level) x 3.7.  ``level``
    may be one value or one per image."""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    yy, xx, cc = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    base = np.sin(0.11 * yy + 0.07 * xx + 0.4 * cc) * np.cos(0.05 * xx - 0.03 * yy)
    r = 2.0 ** (7.0 * base[None] + rng.normal(0.0, 0.3, (n, h, w, 3)))
    lv = np.broadcast_to(np.asarray(level, np.float64), (n,)).reshape(n, 1, 1, 1)
    p = r * 2.0 ** (rng.normal(0.0, 1.0, (n, h, w, 3)) * lv) * 3.7
    return p.astype(np.float32), r.astype(np.float32)
