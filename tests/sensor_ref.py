"""Reference for the sensor model of the HDR pair generator (csrc/sensor_px.h, csrc/hdrpairs.hip):
numpy float64.  The block table comes from numpy's own Philox; a pure-Python Philox4x64-10 pins the
counter convention the kernel is held to.  The per-channel camera is built from hdrgen_ref's and
the tone-mapping oracle's pieces."""
import numpy as np

import hdrgen_ref as R
from oracle import tonemap_ref as TR

M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
MASK = (1 << 64) - 1

# the four frames of the GPU tests: test_gpu_hdrgen.py's cameras (v, n, y), and per frame (a, b, key):
# both terms, shot noise alone, read noise alone; keys below 2^32, above 2^63 and with a second word
CAMERAS = [(0.5, 0.6, 0.9), (-2.0, 0.3, 1.1), (3.0, 0.9, 0.7), (-3.5, 1.2, 0.5)]
FRAME_NOISE = [(1e-3, 2e-3, (12345, 0)), (1e-2, 1e-3, (2 ** 63 + 77, 5)), (0.0, 5e-3, (2 ** 32 + 1, 0)),
               (4e-3, 0.0, (99, 2 ** 64 - 1))]


def scene(h=24, w=40):
    """The four frames of test_gpu_hdrgen.py's case (float and RGBE sources; identity, quarter turn,
    flips; windows of target size and resized) from pictures with two black pixels instead of a
    2 % share: a black pixel adds log(realmin) = -708 to the log sum, and a 2 % share sinks the
    log-average so far that 98 % of the exposures clip, where noise shows nothing.  Returns (srcs,
    pics = what the sources hold as float32, windows (top, left, ch, cw), transform draws)."""
    import rgbe_ref as RR
    from cnn_itmo_amd import datagen as D
    rng = np.random.default_rng(12)
    f0, f1, f2, f3 = (R.radiance(rng, *s, zeros=0.0) for s in ((37, 53), (41, 29), (24, 40), (64, 64)))
    f0[20, 20] = 0.0  # inside frame 0's window, which is copied through
    f2[5, 7] = 0.0
    q1, q2 = RR.encode(f1), RR.encode(f2)
    windows = [(13, 13, h, w), (0, 0, 41, 29), (0, 0, 24, 40), (5, 9, 48, 50)]
    g = D.ImageDataGenerator(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2)
    rs = np.random.RandomState(5)
    params = [g.get_random_transform((h, w, 3), rs) for _ in range(4)]
    params[0].update(theta=0, zx=1, zy=1, flip_horizontal=False, flip_vertical=False)
    params[1].update(theta=90.0, zx=1, zy=1, flip_horizontal=False, flip_vertical=False)
    params[2].update(flip_horizontal=True, flip_vertical=False)
    params[3].update(flip_horizontal=True, flip_vertical=True)
    return [f0, q1, q2, f3], [f0, RR.decode(q1), RR.decode(q2), f3], windows, params


def philox4x64_10(counter, key):
    """One block: counter = (c0, c1, c2, c3), key = (k0, k1), Python ints -> four Python ints."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & MASK, (p0 >> 64) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def blocks(key, count):
    """uint64 [count, 4]: row p is the block of pixel p, i.e. of counter (p + 1, 0, 0, 0)."""
    k0, k1 = (int(key), 0) if np.ndim(key) == 0 else (int(key[0]), int(key[1]))
    bg = np.random.Philox(key=np.array([k0, k1], np.uint64), counter=np.zeros(4, np.uint64))
    return bg.random_raw(4 * count).reshape(count, 4)


def normals(key, h, w):
    """float64 [h, w, 3]: the standard normals (R, G, B) of every pixel of an h x w frame."""
    b = blocks(key, h * w)
    u1 = ((b[:, 0] >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = (b[:, 1] >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    u3 = ((b[:, 2] >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    u4 = (b[:, 3] >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    ra, rb = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(u3))
    z = np.stack([ra * np.cos(2 * np.pi * u2), ra * np.sin(2 * np.pi * u2), rb * np.cos(2 * np.pi * u4)], axis=-1)
    return z.reshape(h, w, 3)


def sigma(e, a, b):
    return np.sqrt(a * np.maximum(np.asarray(e, np.float64), 0.0) + b * b)


def noisy(e, a, b, z):
    return np.asarray(e, np.float64) + sigma(e, a, b) * z


def exposure(warped, camera, key=0.18, lum=TR.REC709):
    """float64 [h, w, 3]: e_c = key 2^v / G * hdr_c, G the log-average of the luminance."""
    G = TR.log_average(TR.rgb2lum(warped, lum))
    return (key * 2.0 ** camera[0] / G) * np.asarray(warped, np.float64)


def curve(e, camera):
    """The camera curve min(1, (1+n) e^y / (n + e^y)) on every element."""
    _, n, y = camera
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ey = np.asarray(e, np.float64) ** y
        return np.fmin(1.0, (1 + n) * (ey / (n + ey)))


def channel_camera(warped, camera, key=0.18, quantize=0, noise=None, shift=0.0, lum=TR.REC709):
    """The input x of response 1 as the kernel stores it, float32 [h, w, 3], and the raw float64 curve.
    noise = (a, b, frame key); shift: e' is moved by shift * 16 * 2^-53 * (e + sigma |z|) before the
    clamp at 0 (-1 / +1: the ends of the interval the fp64 library functions' last bits leave)."""
    e = exposure(warped, camera, key, lum)
    if noise is not None and (noise[0] != 0 or noise[1] != 0):
        a, b, k = noise
        h, w, _ = e.shape
        z = normals(k, h, w)
        s = sigma(e, a, b)
        e = np.maximum(0.0, noisy(e, a, b, z) + shift * 16 * 2.0 ** -53 * (e + s * np.abs(z)))
    raw = curve(e, camera)
    return R.store(raw, quantize & 1), raw
