"""The baseline-JPEG round trip of cnnitmo_jpeg_roundtrip (csrc/jpeg.hip), defined in integers.

This file is the definition: plain numpy on int64, every intermediate asserted to fit int32 (so the
kernel may use int32), no float after the 8-bit load.  It restates the pixel path of the IJG
library (libjpeg 6b / libjpeg-turbo, the defaults every writer and reader uses: JDCT_ISLOW on both
sides, h2v2 box downsampling, "fancy" triangle upsampling); entropy coding is lossless and left out.

Per image, u8 [h][w][3]:

1. samples      u = uint8(255 x): round half away from zero, saturating, NaN -> 0 (tonemap_px.h).
2. RGB -> YCbCr (jccolor.c), 16-bit fixed point, F(v) = floor(v * 65536 + 0.5):
       Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
       Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
       Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
3. 4:2:0        the full-resolution chroma planes are extended by edge replication to an even number
                of rows and, as the library does it (jcsample.c expands the right edge before it
                averages), to a multiple of 16 columns; then chroma (i, j) = (the four samples of
                rows 2i, 2i+1 and columns 2j, 2j+1, + 1 for an even j, + 2 for an odd j) >> 2
                (h2v2_downsample).  Chroma size: ceil(h/2) x ceil(w/2), already a multiple of 8 wide.
                In clamped form: rows min(2i, h-1), min(2i+1, h-1), columns min(2j, w-1), min(2j+1, w-1).
4. per plane    extended to whole 8 x 8 blocks by edge replication (for the chroma of 4:2:0 only
                rows are left to add), - 128, forward DCT `fdct` rows then columns (jfdctint.c: the
                result is 8 x the DCT), quantised q = sign(c) ((|c| + (8Q >> 1)) / (8Q)) (round
                half away from zero), dequantised q Q, inverse DCT `idct` columns then rows
                (jidctint.c), + 128, clamped to 0..255.
5. 4:2:0        triangle upsampling (jdsample.c, h2v2 fancy) of the ceil(h/2) x ceil(w/2) decoded
                chroma samples, neighbours replicated at that size's edges: for output (r, c),
                i = r >> 1, j = c >> 1, i' = i - 1 (r even) or i + 1 (r odd), j' likewise, clamped;
                s(j) = 3 C[i][j] + C[i'][j];  out = (3 s(j) + s(j') + (8 for an even c, 7 for an
                odd c)) >> 4.
6. YCbCr -> RGB (jdcolor.c), cb = Cb - 128, cr = Cr - 128, >> is the arithmetic shift:
       R = clamp(Y + ((91881 cr + 32768) >> 16))
       G = clamp(Y + ((-22554 cb - 46802 cr + 32768) >> 16))
       B = clamp(Y + ((116130 cb + 32768) >> 16))
   stored as float32(level) * float32(1 / 255.).

Quantisation tables: Annex K of ITU-T T.81 scaled as jpeg_quality_scaling / jpeg_add_quant_table do,
natural (row-major) order, [0] luminance, [1] chrominance.
"""
import numpy as np

I32 = (-(1 << 31), (1 << 31) - 1)

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)

# jfdctint.c / jidctint.c: FIX(v) = round(v * 2^13)
CONST_BITS, PASS1_BITS = 13, 2
F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865 = 2446, 3196, 4433, 6270
F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065 = 7373, 9633, 12299, 15137
F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 16069, 16819, 20995, 25172


def _c(a):
    """a, asserted to fit int32."""
    a = np.asarray(a, np.int64)
    assert a.size == 0 or (a.min() >= I32[0] and a.max() <= I32[1]), "an intermediate leaves int32"
    return a


def _descale(a, n):
    return _c(_c(a + (1 << (n - 1))) >> n)


def quant_tables(quality):
    """uint16 [2][64] of a libjpeg quality 1..100."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {quality!r}: 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * s + 50) // 100, 1, 255) for t in (LUMA, CHROMA)]).astype(np.uint16)


def im2uint8(x):
    """uint8(255 x) of a float array with imwrite's rounding (a uint8 array passes through)."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x
    v = 255.0 * x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        u = np.where(v > 0.0, np.floor(np.minimum(v, 255.0) + 0.5), 0.0)  # a NaN compares false
    return u.astype(np.uint8)


def fdct(d, pass2):
    """jfdctint.c's 1-D pass along the last axis ([..., 8] int64); pass2: the column pass's scaling."""
    d = [_c(d[..., k]) for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = _c(t0 + t3), _c(t0 - t3), _c(t1 + t2), _c(t1 - t2)
    o = [None] * 8
    if pass2:
        o[0], o[4] = _descale(t10 + t11, PASS1_BITS), _descale(t10 - t11, PASS1_BITS)
        n = CONST_BITS + PASS1_BITS
    else:
        o[0], o[4] = _c((t10 + t11) << PASS1_BITS), _c((t10 - t11) << PASS1_BITS)
        n = CONST_BITS - PASS1_BITS
    z1 = _c(_c(t12 + t13) * F_0_541196100)
    o[2] = _descale(z1 + _c(t13 * F_0_765366865), n)
    o[6] = _descale(z1 + _c(t12 * -F_1_847759065), n)
    z1, z2, z3, z4 = _c(t4 + t7), _c(t5 + t6), _c(t4 + t6), _c(t5 + t7)
    z5 = _c(_c(z3 + z4) * F_1_175875602)
    t4, t5, t6, t7 = _c(t4 * F_0_298631336), _c(t5 * F_2_053119869), _c(t6 * F_3_072711026), _c(t7 * F_1_501321110)
    z1, z2 = _c(z1 * -F_0_899976223), _c(z2 * -F_2_562915447)
    z3, z4 = _c(_c(z3 * -F_1_961570560) + z5), _c(_c(z4 * -F_0_390180644) + z5)
    o[7] = _descale(_c(t4 + z1) + z3, n)
    o[5] = _descale(_c(t5 + z2) + z4, n)
    o[3] = _descale(_c(t6 + z2) + z3, n)
    o[1] = _descale(_c(t7 + z1) + z4, n)
    return np.stack(o, axis=-1)


def idct(d, pass2):
    """jidctint.c's 1-D pass along the last axis; pass2: the row pass's scaling (the + 128 and the
    clamp are the caller's)."""
    d = [_c(d[..., k]) for k in range(8)]
    z1 = _c(_c(d[2] + d[6]) * F_0_541196100)
    t2 = _c(z1 + _c(d[6] * -F_1_847759065))
    t3 = _c(z1 + _c(d[2] * F_0_765366865))
    t0, t1 = _c(_c(d[0] + d[4]) << CONST_BITS), _c(_c(d[0] - d[4]) << CONST_BITS)
    t10, t13, t11, t12 = _c(t0 + t3), _c(t0 - t3), _c(t1 + t2), _c(t1 - t2)
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = _c(t0 + t3), _c(t1 + t2), _c(t0 + t2), _c(t1 + t3)
    z5 = _c(_c(z3 + z4) * F_1_175875602)
    t0, t1, t2, t3 = _c(t0 * F_0_298631336), _c(t1 * F_2_053119869), _c(t2 * F_3_072711026), _c(t3 * F_1_501321110)
    z1, z2 = _c(z1 * -F_0_899976223), _c(z2 * -F_2_562915447)
    z3, z4 = _c(_c(z3 * -F_1_961570560) + z5), _c(_c(z4 * -F_0_390180644) + z5)
    t0, t1 = _c(_c(t0 + z1) + z3), _c(_c(t1 + z2) + z4)
    t2, t3 = _c(_c(t2 + z2) + z3), _c(_c(t3 + z1) + z4)
    n = CONST_BITS + PASS1_BITS + 3 if pass2 else CONST_BITS - PASS1_BITS
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(v, n) for v in o], axis=-1)


def codec_plane(p, q):
    """Step 4: p int64 [H][W], H and W multiples of 8, samples 0..255; q [64] -> decoded plane."""
    hb, wb = p.shape[0] // 8, p.shape[1] // 8
    b = p.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3) - 128  # [hb][wb][row][col]
    c = fdct(b, False)                                        # rows
    c = fdct(c.swapaxes(-1, -2), True).swapaxes(-1, -2)       # columns
    q8 = (np.asarray(q, np.int64).reshape(8, 8)) << 3
    a = _c(np.abs(c) + (q8 >> 1)) // q8
    c = _c(np.sign(c) * a * (q8 >> 3))
    c = idct(c.swapaxes(-1, -2), False).swapaxes(-1, -2)      # columns
    c = idct(c, True)                                         # rows
    return np.clip(c + 128, 0, 255).transpose(0, 2, 1, 3).reshape(p.shape)


def _extend(p, mh, mw):
    h, w = p.shape
    return np.pad(p, ((0, -h % mh), (0, -w % mw)), mode="edge")


def upsample(c, h, w):
    """Step 5: decoded chroma c [ceil(h/2)][ceil(w/2)] -> [h][w]."""
    hc, wc = c.shape
    r, col = np.arange(h), np.arange(w)
    i, j = r >> 1, col >> 1
    i2 = np.clip(np.where(r & 1, i + 1, i - 1), 0, hc - 1)
    j2 = np.clip(np.where(col & 1, j + 1, j - 1), 0, wc - 1)
    s = 3 * c[i] + c[i2]  # [h][wc]
    return _c(3 * s[:, j] + s[:, j2] + np.where(col & 1, 7, 8)[None, :]) >> 4


def roundtrip_u8(u, qtabs, subsampling="4:2:0"):
    """u uint8 [h][w][3], qtabs [2][64] -> uint8 [h][w][3]."""
    if subsampling not in ("4:4:4", "4:2:0"):
        raise ValueError(f"subsampling {subsampling!r}: '4:4:4' or '4:2:0'")
    qtabs = np.asarray(qtabs, np.int64).reshape(2, 64)
    assert qtabs.min() >= 1
    h, w, _ = u.shape
    R, G, B = (u[..., k].astype(np.int64) for k in range(3))
    Y = _c(19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = _c(-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = _c(32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    Yd = codec_plane(_extend(Y, 8, 8), qtabs[0])[:h, :w]
    ch = []
    for P in (Cb, Cr):
        if subsampling == "4:2:0":
            P = _extend(P, 2, 16)
            bias = np.where(np.arange(P.shape[1] // 2) & 1, 2, 1)[None, :]
            P = _extend((P[0::2, 0::2] + P[0::2, 1::2] + P[1::2, 0::2] + P[1::2, 1::2] + bias) >> 2, 8, 8)
            ch.append(upsample(codec_plane(P, qtabs[1])[:(h + 1) // 2, :(w + 1) // 2], h, w))
        else:
            ch.append(codec_plane(_extend(P, 8, 8), qtabs[1])[:h, :w])
    cb, cr = ch[0] - 128, ch[1] - 128
    out = np.stack([Yd + (_c(91881 * cr + 32768) >> 16),
                    Yd + (_c(-22554 * cb - 46802 * cr + 32768) >> 16),
                    Yd + (_c(116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def to_float(u):
    """The stored value of a level: float32(level) * float32(1 / 255.)."""
    return u.astype(np.float32) * np.float32(1 / 255.)


def roundtrip(x, qtabs, subsampling="4:2:0", apply=None):
    """x [n][h][w][3] float (or uint8), qtabs [n][2][64] (or [2][64] for all), apply [n] or None ->
    float32 [n][h][w][3]: what cnnitmo_jpeg_roundtrip stores; an image with apply 0 is copied."""
    x = np.asarray(x)
    qtabs = np.broadcast_to(np.asarray(qtabs), (x.shape[0], 2, 64))
    out = np.empty(x.shape, np.float32)
    for i in range(x.shape[0]):
        if apply is not None and not apply[i]:
            out[i] = x[i]
        else:
            out[i] = to_float(roundtrip_u8(im2uint8(x[i]), qtabs[i], subsampling))
    return out
