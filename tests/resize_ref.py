"""Numpy restatement of Pillow's antialiased resampling (src/libImaging/Resample.c): the reference
of cnnitmo_resize / cnnitmo_resize_coeffs (include/cnn_itmo.h) and cnn_itmo_amd.resize.

``coeffs`` is precompute_coeffs, ``pass_f`` the 32-bit float pass (mode F), ``pass_u8`` the 8-bit
pass with normalize_coeffs_8bpc's fixed-point taps, ``resize`` ImagingResample's order of the two.
tests/test_resize_host.py holds this file against ``PIL.Image.resize`` itself: byte for byte for
uint8 RGB, bit for bit for float32 (channel by channel, mode F).

Everything is a C double: Python floats for the taps (``math.sin`` is libm's, as in Pillow), numpy
float64 for the sums, one multiply and one add per tap, in tap order.
"""
import math

import numpy as np

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
FILTER_IDS = {f: i for i, f in enumerate(FILTERS)}  # CNNITMO_RESIZE_*
SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
PRECISION_BITS = 32 - 8 - 2


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FUNCS = {"box": _box, "bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos}


def coeffs(n_in, n_out, filt):
    """(ksize, bounds int32 [n_out,2] = (xmin, n), kk float64 [n_out,ksize])."""
    f, support = FUNCS[filt], SUPPORT[filt]
    scale = filterscale = float(n_in) / n_out
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.float64)
    ss = 1.0 / filterscale
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        ww = 0.0
        xmin = max(int(center - support + 0.5), 0)  # int(): towards zero, as C's (int)
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        k = []
        for x in range(n):
            w = f((x + xmin - center + 0.5) * ss)
            k.append(w)
            ww += w
        if ww != 0.0:
            k = [v / ww for v in k]
        kk[xx, :n] = k
        bounds[xx] = (xmin, n)
    return ksize, bounds, kk


def pass_f(a, axis, bounds, kk):
    """float32 array, filtered along `axis` (0 or 1 of [h,w,...]; leading batch axes excluded by the
    caller): ss = 0.0; ss += (double)pixel * k in tap order; (float)ss."""
    a = np.moveaxis(np.asarray(a, np.float32), axis, 0)
    out = np.empty((len(bounds),) + a.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for xx, (xmin, n) in enumerate(bounds):
            ss = np.zeros(a.shape[1:], np.float64)
            for x in range(n):
                ss = ss + a[xmin + x].astype(np.float64) * kk[xx, x]
            out[xx] = ss.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def fixed_taps(kk):
    """normalize_coeffs_8bpc: (int)(k 2^22 + 0.5) for k >= 0, (int)(k 2^22 - 0.5) otherwise."""
    s = kk * float(1 << PRECISION_BITS)
    return np.where(kk < 0, np.trunc(s - 0.5), np.trunc(s + 0.5)).astype(np.int64)


def pass_u8(a, axis, bounds, kk):
    """uint8 array: ss = 2^21; ss += pixel * ki; clamp(ss >> 22, 0, 255).  Every partial sum is
    checked to stay inside int32."""
    a = np.moveaxis(np.asarray(a, np.uint8), axis, 0)
    ki = fixed_taps(kk)
    out = np.empty((len(bounds),) + a.shape[1:], np.uint8)
    for xx, (xmin, n) in enumerate(bounds):
        ss = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(n):
            ss = ss + a[xmin + x].astype(np.int64) * ki[xx, x]
            assert np.abs(ss).max(initial=0) < 2 ** 31, "int32 overflow in the 8-bit pass"
        out[xx] = np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, size, filt):
    """img [h,w,(3)] or [n,h,w,3], float32 or uint8 -> the same with (oh, ow): the horizontal pass
    first where the width changes, then the vertical one on its stored result; a copy otherwise."""
    img = np.asarray(img)
    assert img.dtype in (np.float32, np.uint8), img.dtype
    if img.ndim == 4:
        return np.stack([resize(i, size, filt) for i in img])
    oh, ow = size
    h, w = img.shape[:2]
    one = pass_u8 if img.dtype == np.uint8 else pass_f
    out = img.copy()
    if ow != w:
        _, b, k = coeffs(w, ow, filt)
        out = one(out, 1, b, k)
    if oh != h:
        _, b, k = coeffs(h, oh, filt)
        out = one(out, 0, b, k)
    return out
