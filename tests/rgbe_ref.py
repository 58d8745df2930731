"""Reference for cnn_itmo_amd/hdrio.py: a numpy restatement of the RGBE pixel codec and
deliberately simple, independent Radiance .hdr and PFM readers / writers (per-byte Python loops,
no code shared with the package)."""
import numpy as np

RGBE_MAX = np.float32(255 * 2.0 ** 119)  # the largest value RGBE holds: (255, ., ., 255)
RGBE_TINY = np.float32(1e-32)


# ---------------------------------------------------------------------------------- pixel codec
def encode(x):
    """float32 [...,3] -> uint8 [...,4]: NaN -> 0, clamp to [0, 255 * 2^119], v = max(r,g,b);
    v < 1e-32f -> 0,0,0,0; else frexp(v) = (m, e), mantissa = floor(ldexp(c, 8 - e)), byte e + 128."""
    x = np.array(x, np.float32)
    x[np.isnan(x)] = 0
    x = np.minimum(np.maximum(x, np.float32(0)), RGBE_MAX)
    v = x.max(-1)
    _, e = np.frexp(v)
    mant = np.floor(np.ldexp(x, (8 - e)[..., None].astype(np.int32)))
    assert mant.dtype == np.float32 and mant.min() >= 0 and mant.max() <= 255
    out = np.empty(x.shape[:-1] + (4,), np.uint8)
    out[..., :3] = mant.astype(np.uint8)
    out[..., 3] = (e + 128).astype(np.uint8)
    out[v < RGBE_TINY] = 0
    return out


def decode(q):
    """uint8 [...,4] -> float32 [...,3]: E = 0 -> 0; else mantissa * 2^(E - 136), no +0.5.  Formed in
    float64 and narrowed: every value (the E = 1 denormals included) is exact in float32."""
    q = np.asarray(q, np.uint8)
    E = q[..., 3].astype(np.int32)
    out = np.ldexp(q[..., :3].astype(np.float64), (E - 136)[..., None])
    out[E == 0] = 0
    f = out.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), out)
    return f


# ---------------------------------------------------------------------------------- .hdr
def _rle_channel(vals, out):
    """Ward's scheme, simply: a run of >= 4 equal bytes is a run packet (<= 127), everything else
    is gathered into literal packets (<= 128)."""
    n, i = len(vals), 0
    lit = []

    def flush():
        j = 0
        while j < len(lit):
            chunk = lit[j:j + 128]
            out.append(len(chunk))
            out.extend(chunk)
            j += 128
        del lit[:]

    while i < n:
        r = 1
        while i + r < n and r < 127 and vals[i + r] == vals[i]:
            r += 1
        if r >= 4:
            flush()
            out.append(128 + r)
            out.append(vals[i])
            i += r
        else:
            lit.append(vals[i])
            i += 1
    flush()


def write_hdr(rgbe, rle=False, magic="#?RADIANCE", lines=(), orientation="-Y", fmt="32-bit_rle_rgbe"):
    """uint8 [h,w,4] (row 0 = top) -> file bytes.  orientation '+Y' stores the rows bottom to top."""
    q = np.asarray(rgbe, np.uint8)
    h, w = q.shape[:2]
    out = bytearray()
    out += magic.encode() + b"\n"
    out += b"FORMAT=" + fmt.encode() + b"\n"
    for s in lines:
        out += s.encode() + b"\n"
    out += b"\n"
    out += f"{orientation} {h} +X {w}\n".encode()
    rows = range(h) if orientation == "-Y" else range(h - 1, -1, -1)
    for y in rows:
        if rle:
            assert 8 <= w <= 32767
            out += bytes([2, 2, w >> 8, w & 255])
            for c in range(4):
                _rle_channel(q[y, :, c].tolist(), out)
        else:
            for xx in range(w):
                out += bytes(q[y, xx].tolist())
    return bytes(out)


def read_hdr(data, packets=None):
    """file bytes -> (exposure product, uint8 [h,w,4], row 0 = top).  ``packets``: a list that
    receives ('run' | 'lit', count, first byte) for every run-length packet read."""
    data = bytes(data)
    head, _, rest = data.partition(b"\n\n")
    hl = head.split(b"\n")
    assert hl[0] in (b"#?RADIANCE", b"#?RGBE"), hl[0]
    exposure = 1.0
    for s in hl[1:]:
        if s.startswith(b"EXPOSURE="):
            exposure *= float(s[9:])
    res, _, body = rest.partition(b"\n")
    t = res.split()
    assert t[0] in (b"-Y", b"+Y") and t[2] == b"+X", res
    h, w = int(t[1]), int(t[3])
    img = np.zeros((h, w, 4), np.uint8)
    p = 0
    for y in range(h):
        if 8 <= w <= 32767 and body[p] == 2 and body[p + 1] == 2 and body[p + 2] * 256 + body[p + 3] == w:
            p += 4
            for c in range(4):
                xx = 0
                while xx < w:
                    cnt = body[p]
                    p += 1
                    assert cnt != 0
                    if cnt > 128:
                        cnt -= 128
                        assert xx + cnt <= w
                        if packets is not None:
                            packets.append(("run", cnt, body[p]))
                        for _ in range(cnt):
                            img[y, xx, c] = body[p]
                            xx += 1
                        p += 1
                    else:
                        assert xx + cnt <= w
                        if packets is not None:
                            packets.append(("lit", cnt, body[p]))
                        for _ in range(cnt):
                            img[y, xx, c] = body[p]
                            xx += 1
                            p += 1
        else:
            for xx in range(w):
                for c in range(4):
                    img[y, xx, c] = body[p]
                    p += 1
    assert p == len(body), (p, len(body))
    if t[0] == b"+Y":
        img = img[::-1].copy()
    return exposure, img


# ---------------------------------------------------------------------------------- PFM
def write_pfm(img, big_endian=False, magic="PF"):
    a = np.asarray(img, np.float32)
    h, w = a.shape[:2]
    out = bytearray(f"{magic}\n{w} {h}\n{'1.0' if big_endian else '-1.0'}\n".encode())
    for y in range(h - 1, -1, -1):  # bottom row first
        out += a[y].astype(">f4" if big_endian else "<f4").tobytes()
    return bytes(out)


def read_pfm(data):
    data = bytes(data)
    t = data.split(b"\n", 3)
    assert t[0] == b"PF", t[0]
    w, h = (int(v) for v in t[1].split())
    dt = "<f4" if float(t[2]) < 0 else ">f4"
    a = np.frombuffer(t[3], dt, h * w * 3).reshape(h, w, 3)
    return a[::-1].astype(np.float32)


# ---------------------------------------------------------------------------------- test data
def random_hdr(shape, seed, lo=-100, hi=126):
    """float32 [...,3]: random mantissas in [1, 2) times 2^U(lo, hi) per pixel; every fourth pixel
    has one channel 1000x smaller than the others."""
    rng = np.random.default_rng(seed)
    shape = tuple(shape)
    mant = 1 + rng.random(shape + (3,))
    ex = rng.integers(lo, hi + 1, shape)
    x = (mant * 2.0 ** ex[..., None]).astype(np.float32)
    flat = x.reshape(-1, 3)
    idx = np.arange(0, flat.shape[0], 4)
    flat[idx, rng.integers(0, 3, idx.shape[0])] *= np.float32(1e-3)
    return x


def specials():
    """float32 [k,3]: zeros, negatives, -0, NaN, +-inf, the 1e-32 threshold, exact powers of two,
    the largest RGBE value and FLT_MAX, alone and mixed with ordinary components."""
    inf, nan, fmax = np.inf, np.nan, np.finfo(np.float32).max
    rows = [(0, 0, 0), (-1, -1, -1), (-0.0, -0.0, -0.0), (nan, nan, nan), (inf, inf, inf), (-inf, -inf, -inf),
            (1e-33, 1e-33, 1e-33), (1e-32, 1e-32, 1e-32), (1e-33, 1e-32, 0), (9.9999e-33, 0, 0),
            (1.0000001e-32, 0, 0), (1e-40, 1e-45, 1e-38), (1, 1, 1), (0.5, 0.25, 0.125), (2, 4, 8), (1, 0, 0),
            (2.0 ** -100, 2.0 ** -101, 2.0 ** -109), (2.0 ** 126, 2.0 ** 119, 2.0 ** 118),
            (255 * 2.0 ** 119, 255 * 2.0 ** 119, 1), (255 * 2.0 ** 119, 0, 254 * 2.0 ** 119), (fmax, fmax, fmax),
            (fmax, 1, 0), (inf, 1, 2.0 ** 120), (nan, 1, 2), (-1, 3, nan), (1, -0.0, -inf), (255, 256, 257),
            (0.999999, 1, 1.000001), (1e-45, 1, 1e-38), (3e38, 1e38, 1e30), (nan, -1, 1e-33), (-nan, inf, 7)]
    return np.array(rows, np.float32)
