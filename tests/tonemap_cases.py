"""Inputs and float64 references of tests/test_gpu_tonemap.py (test infrastructure, numpy only).

The reference is oracle/tonemap_ref.py, one image at a time; this file only builds the images, plants
the special pixels and states the two comparisons the oracle does not have: the exactly rounded sum of
the logs (math.fsum) and the tie rule of the uint8 outputs.  References are computed once per key and
handed out read-only.
"""
import math

import numpy as np

from oracle import tonemap_ref as T

PARTITION = 256 * 256  # pixels one sweep of stats_partial_kernel's grid takes (BLK_PER_IMG * TB)
LUM601 = (0.299, 0.587, 0.114)
TIE_EPS = 1e-6  # |255 x - (k + .5)| below which the two sides may round a uint8 differently
_CACHE = {}


def shape_of(case):
    return tuple(int(v) for v in case.split("x"))


def hdr_image(seed, h, w):
    """Log-normal HDR, as test_tonemap._hdr."""
    return np.exp(np.random.default_rng(seed).normal(-1.0, 1.5, (h, w, 3))).astype(np.float32)


def hdr_batch(case, seed=100):
    """fp32 [n,h,w,3], image i from seed + i (read-only, cached)."""
    key = ("hdr", case, seed)
    if key not in _CACHE:
        n, h, w = shape_of(case)
        a = np.stack([hdr_image(seed + i, h, w) for i in range(n)])
        a.setflags(write=False)
        _CACHE[key] = a
    return _CACHE[key]


def sdr_batch(case, seed=200):
    """uint8 [n,h,w,3] noise without an all-0 and without an all-255 pixel (0 < I < 1 everywhere)."""
    key = ("sdr", case, seed)
    if key not in _CACHE:
        n, h, w = shape_of(case)
        a = np.stack([np.random.default_rng(seed + i).integers(0, 256, (h, w, 3), dtype=np.uint8) for i in range(n)])
        a[..., 1] = np.clip(a[..., 1], 1, 254)
        a.setflags(write=False)
        _CACHE[key] = a
    return _CACHE[key]


def zero_positions(hw, k, seed):
    """k distinct pixel indices (at most hw); where the image has pixels past the first sweep of the
    statistics grid, the larger half of them lies there."""
    rng = np.random.default_rng(seed)
    k = min(k, hw)
    far = min((k + 1) // 2, max(hw - PARTITION, 0))
    near = rng.choice(min(hw, PARTITION), k - far, replace=False)
    return np.concatenate([near, PARTITION + rng.choice(max(hw - PARTITION, 1), far, replace=False)]).astype(np.int64)


ZERO_COUNTS = (0, 1, 7)


def plant_zeros(batch, rot):
    """A copy of batch in which image i has ZERO_COUNTS[(i + rot) % 3] all-zero pixels; the counts."""
    out = np.array(batch)
    n, h, w, _ = out.shape
    counts = []
    for i in range(n):
        pos = zero_positions(h * w, ZERO_COUNTS[(i + rot) % 3], 7000 + 31 * i + rot)
        out[i].reshape(h * w, 3)[pos] = 0
        counts.append(len(pos))
    return out, counts


def logs_of(img, lum=T.REC709):
    """log(max(Y, realmin)) of one fp32 HDR image, float64, flat."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.maximum(T.rgb2lum(img, lum), T.REALMIN)).reshape(-1)


def log_sum_exact(img, lum=T.REC709):
    """(the exactly rounded sum of the logs, max |log|)."""
    lg = logs_of(img, lum)
    return math.fsum(lg), float(np.abs(lg).max())


def g_refs(img, lum=T.REC709):
    """The log-average two ways: exp(fsum / hw) and the oracle's sequential sum."""
    lg = logs_of(img, lum)
    return math.exp(math.fsum(lg) / lg.size), float(T.log_average(T.rgb2lum(img, lum)))


def near_tie(ref64):
    """Elements of a float64 reference whose 255 x lies within TIE_EPS of a .5 tie inside (0, 255)."""
    with np.errstate(invalid="ignore"):
        v = 255.0 * np.asarray(ref64, np.float64)
        return (np.abs(v - np.floor(v) - 0.5) <= TIE_EPS) & (v > 0) & (v < 255)


def check_u8(got, ref64):
    """got equals im2uint8(ref64) exactly, except by 1 at a near tie; near ties are < 0.1 % of the image."""
    want = T.im2uint8(ref64)
    assert got.dtype == np.uint8 and got.shape == want.shape
    tie = near_tie(ref64)
    assert tie.mean() < 1e-3, f"{int(tie.sum())} of {tie.size} reference elements sit on a tie"
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert not (d[~tie] != 0).any(), f"{int((d[~tie] != 0).sum())} elements away from a tie differ, max {int(d.max())}"
    assert d.max(initial=0) <= 1


MAP_SHAPES = ["2x257x259", "3x37x61"]
EXTREME_CAMERA = (4.0, 0.05, 1.3)  # exposure 2^4 and a steep curve: many pixels reach min(1, .)


def map_hdr(case):
    """The HDR batch of the map tests: image 0 has one zero-luminance pixel (0/0 -> NaN, as in MATLAB)."""
    def make():
        a = np.array(hdr_batch(case, seed=300))
        a[0, 0, 0] = 0.0
        return a
    return cached(("map_hdr", case), make)


def camera_params(n, seed=3):
    """Per-image (v, n, y) as virtual_camera.m draws them; the last image gets EXTREME_CAMERA."""
    from cnn_itmo_amd.tonemap import virtual_camera_params
    v, cn, cy = virtual_camera_params(n, np.random.default_rng(seed))
    v[-1], cn[-1], cy[-1] = EXTREME_CAMERA
    return v, cn, cy


SCRIPT_KINDS = {"2x257x259": ("none", "some"), "2x257x259b": ("all", "some"), "3x37x61": ("none", "some", "all")}


def script_sdr(case, white):
    """uint8 batch for inverse_Reinhard.m: per image no / some / only zero-luminance pixels (PB1 == 0,
    0 < PB1 < P, PB1 == P); white plants an all-255 pixel (I = 1: X = inf, E clamps to 2^32) in each."""
    def make():
        a = np.array(sdr_batch(case.rstrip("b"), seed=400))
        for i, kind in enumerate(SCRIPT_KINDS[case]):
            if kind == "some":
                a[i, :2] = 0
                a[i, -1, -3:] = 0
            elif kind == "all":
                a[i] = 0
            if white:
                a[i, a.shape[1] // 2, a.shape[2] // 3] = 255
        return a
    return cached(("script_sdr", case, white), make)


EXACT_G = 0.37


def exact_sdr(case):
    """Linear fp32 SDR for the exact inverse: the oracle's Reinhard of an HDR batch, with a pixel of
    exactly 1.0 (E clamps to 2^32), one of 1.5 (I > 1: negative output) and a zero pixel (0/0) per image."""
    def make():
        hdr = hdr_batch(case, seed=450)
        a = np.stack([T.reinhard(h) for h in hdr]).astype(np.float32)
        a[:, 1, 1] = 1.0
        a[:, 2, 0] = 1.5
        a[:, 0, 2] = 0.0
        return a
    return cached(("exact_sdr", case), make)


SPECIAL_CASE = "3x37x61"
SPECIAL_IMAGE = 1


def special_hdr(kind):
    """A batch of three whose image 1 holds special pixels.  'finite': a negative pixel, an fp32 denormal
    and a zero pixel; 'inf': those and a +inf channel (G = inf); 'nan': a NaN pixel (G = NaN)."""
    def make():
        a = np.array(hdr_batch(SPECIAL_CASE, seed=500))
        s = a[SPECIAL_IMAGE]
        if kind in ("finite", "inf"):
            s[0, 0] = (-0.5, -0.25, -1.0)
            s[1, 1] = (1e-40, 2e-41, 5e-42)
            s[2, 2] = 0.0
        if kind == "inf":
            s[3, 3] = (1.0, np.inf, 2.0)
        if kind == "nan":
            s[4, 4] = (np.nan, 1.0, 1.0)
        return a
    return cached(("special", kind), make)


def cached(key, fn):
    if key not in _CACHE:
        r = fn()
        if isinstance(r, np.ndarray):
            r.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def same_bits(got, want):
    """Equal bits, whatever the type (fp32, fp64 or uint8)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = got.view(u) != want.view(u)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} elements differ, the first at {np.argwhere(bad)[0]}"
