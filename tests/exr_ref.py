"""numpy + zlib restatement of the OpenEXR scan-line layout that cnn_itmo_amd/exr.py and
csrc/exr.hip implement (see exr.py's docstring for the layout); written plainly, sharing no code
with them.  The reference of tests/test_exr_host.py and tests/test_gpu_exr.py.

  code_chunk / decode_chunk     ZIP's split + predictor on one chunk's bytes, and its inverse
  build(channels, ...)          a file from per-channel arrays
  take_apart(data)              (header, {name: array [h,w]}, raw, coded) of a file
  rgb(channels)                 float32 [h,w,3] of R, G, B or a lone Y; half through np.float16
  record_bytes / payload        the writer's B, G, R record bytes of a picture, plain or coded
"""
import struct
import zlib

import numpy as np

MAGIC = bytes([0x76, 0x2F, 0x31, 0x01])
DTYPES = {0: np.dtype("<u4"), 1: np.dtype("<f2"), 2: np.dtype("<f4")}
LINES = {0: 1, 2: 1, 3: 16}


def code_chunk(r):
    """uint8 [n] record bytes -> split (even-indexed bytes, then odd-indexed) and predicted."""
    r = np.asarray(r, np.uint8)
    t = np.concatenate([r[0::2], r[1::2]])
    out = t.copy()
    for i in range(1, t.size):
        out[i] = (int(t[i]) - int(t[i - 1]) + 128) & 255
    return out


def decode_chunk(t):
    """The inverse of code_chunk, with np.cumsum: d[i] = t[0] + ... + t[i] - 128 i (mod 256)."""
    t = np.asarray(t, np.uint8)
    n = t.size
    d = ((np.cumsum(t.astype(np.int64)) - 128 * np.arange(n)) & 255).astype(np.uint8)
    out = np.empty(n, np.uint8)
    half = (n + 1) // 2
    out[0::2] = d[:half]
    out[1::2] = d[half:]
    return out


def code_chunk_fast(r):
    """code_chunk without the Python loop (pinned against it by the host tests)."""
    r = np.asarray(r, np.uint8)
    t = np.concatenate([r[0::2], r[1::2]]).astype(np.int64)
    out = t.copy()
    out[1:] = t[1:] - t[:-1] + 128
    return (out & 255).astype(np.uint8)


def attr(name, typ, val):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(val)) + val


def build(channels, compression=3, line_order=0, origin=(0, 0), flags=0, extra=(), level=6, table_in_file_order=False,
          display=None, sampling=None, omit=()):
    """channels: {name: array [h,w] of uint32 / float16 / float32}.  origin: (xMin, yMin) of the data
    window.  line_order 1: the chunks are written from the bottom up; the offset table is in
    increasing y unless table_in_file_order.  extra: further (name, type, bytes) attributes.
    sampling: {name: (xs, ys)} written into the channel list (the data stay full size).  omit:
    names of required attributes to leave out.  Returns (bytes, coded flags per chunk)."""
    names = sorted(channels)
    arrs = {}
    for n in names:
        a = np.asarray(channels[n])
        t = {np.dtype(np.uint32): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}[a.dtype]
        arrs[n] = (t, np.ascontiguousarray(a.astype(DTYPES[t], copy=False)))
    h, w = arrs[names[0]][1].shape
    chlist = b""
    for n in names:
        xs, ys = (sampling or {}).get(n, (1, 1))
        chlist += n.encode() + b"\0" + struct.pack("<i", arrs[n][0]) + bytes([0, 0, 0, 0]) + struct.pack("<ii", xs, ys)
    chlist += b"\0"
    x0, y0 = origin
    box = struct.pack("<4i", x0, y0, x0 + w - 1, y0 + h - 1)
    attrs = {"channels": attr("channels", "chlist", chlist),
             "compression": attr("compression", "compression", bytes([compression])),
             "dataWindow": attr("dataWindow", "box2i", box),
             "displayWindow": attr("displayWindow", "box2i", box if display is None else struct.pack("<4i", *display)),
             "lineOrder": attr("lineOrder", "lineOrder", bytes([line_order])),
             "pixelAspectRatio": attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)),
             "screenWindowCenter": attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0)),
             "screenWindowWidth": attr("screenWindowWidth", "float", struct.pack("<f", 1.0))}
    head = MAGIC + struct.pack("<i", 2 | flags)
    for k, v in attrs.items():
        if k not in omit:
            head += v
    for n, t, v in extra:
        head += attr(n, t, v)
    head += b"\0"
    lines = LINES[compression]
    nchunks = (h + lines - 1) // lines
    datas, coded = [], []
    for i in range(nchunks):
        rec = b""
        for y in range(i * lines, min(h, (i + 1) * lines)):
            for n in names:
                rec += arrs[n][1][y].tobytes()
        if compression == 0:
            datas.append(rec)
            coded.append(0)
            continue
        z = zlib.compress(code_chunk_fast(np.frombuffer(rec, np.uint8)).tobytes(), level)
        if len(z) < len(rec):
            datas.append(z)
            coded.append(1)
        else:
            datas.append(rec)
            coded.append(0)
    order = list(range(nchunks)) if line_order == 0 else list(range(nchunks - 1, -1, -1))
    pos = len(head) + 8 * nchunks
    offsets = {}
    body = b""
    for i in order:
        offsets[i] = pos + len(body)
        body += struct.pack("<ii", y0 + i * lines, len(datas[i])) + datas[i]
    table = b"".join(struct.pack("<Q", offsets[i]) for i in (order if table_in_file_order else range(nchunks)))
    return head + table + body, np.array(coded, np.uint8)


def cstr(buf, pos):
    end = buf.index(b"\0", pos)
    return buf[pos:end].decode("latin-1"), end + 1


def take_apart(data):
    """bytes -> (header, {name: array [h,w]}, raw uint8 [h * line_bytes], coded uint8 [nchunks]).
    header has the shape exr.parse_exr returns.  For well-formed files only."""
    buf = bytes(data)
    assert buf[:4] == MAGIC
    version = struct.unpack_from("<i", buf, 4)[0]
    header = {"version": version & 255, "flags": version & ~255, "other": {}}
    pos = 8
    while buf[pos] != 0:
        name, pos = cstr(buf, pos)
        typ, pos = cstr(buf, pos)
        size = struct.unpack_from("<i", buf, pos)[0]
        val = buf[pos + 4:pos + 4 + size]
        pos += 4 + size
        if name == "channels":
            chans, p = [], 0
            while val[p] != 0:
                cn, p = cstr(val, p)
                t, pl, xs, ys = struct.unpack_from("<iB3xii", val, p)
                p += 16
                chans.append({"name": cn, "type": t, "pLinear": pl, "xSampling": xs, "ySampling": ys})
            header[name] = chans
        elif name in ("compression", "lineOrder"):
            header[name] = val[0]
        elif name in ("dataWindow", "displayWindow"):
            header[name] = struct.unpack("<4i", val)
        elif name in ("pixelAspectRatio", "screenWindowWidth"):
            header[name] = struct.unpack("<f", val)[0]
        elif name == "screenWindowCenter":
            header[name] = struct.unpack("<2f", val)
        else:
            header["other"][name] = (typ, val)
    pos += 1
    x0, y0, x1, y1 = header["dataWindow"]
    w, h = x1 - x0 + 1, y1 - y0 + 1
    lines = LINES[header["compression"]]
    nchunks = (h + lines - 1) // lines
    line_bytes = sum(w * DTYPES[c["type"]].itemsize for c in header["channels"])
    raw = np.zeros(h * line_bytes, np.uint8)
    coded = np.zeros(nchunks, np.uint8)
    rec = np.zeros(h * line_bytes, np.uint8)
    for k in range(nchunks):
        off = struct.unpack_from("<Q", buf, pos + 8 * k)[0]
        y, size = struct.unpack_from("<ii", buf, off)
        i = (y - y0) // lines
        n = min(lines, h - i * lines) * line_bytes
        part = buf[off + 8:off + 8 + size]
        if header["compression"] != 0 and size < n:
            part = zlib.decompress(part)
            coded[i] = 1
        assert len(part) == n
        at = i * lines * line_bytes
        raw[at:at + n] = np.frombuffer(part, np.uint8)
        rec[at:at + n] = decode_chunk(raw[at:at + n]) if coded[i] else raw[at:at + n]
    rows = rec.reshape(h, line_bytes)
    out, at = {}, 0
    for c in header["channels"]:
        dt = DTYPES[c["type"]]
        out[c["name"]] = np.ascontiguousarray(rows[:, at:at + w * dt.itemsize]).view(dt).reshape(h, w)
        at += w * dt.itemsize
    return header, out, raw, coded


def to_f32(a):
    """One channel -> float32: half exactly (np.float16), uint rounded to nearest even, float as is."""
    return np.asarray(a).astype(np.float32)


def rgb(channels):
    """{name: array} -> float32 [h,w,3]: R, G, B, else a lone Y replicated."""
    if all(k in channels for k in "RGB"):
        return np.stack([to_f32(channels[k]) for k in "RGB"], axis=-1)
    return np.repeat(to_f32(channels["Y"])[..., None], 3, axis=-1)


def record_bytes(img, pixel_type):
    """float32 [h,w,3] -> uint8 [h, 3 * w * size]: the lines of a B, G, R file of pixel_type (1 half,
    2 float); half by np.float16 (round to nearest even, overflow to inf)."""
    img = np.asarray(img, np.float32)
    with np.errstate(over="ignore"):
        planes = [img[..., c].astype(DTYPES[pixel_type]) for c in (2, 1, 0)]
    h = img.shape[0]
    return np.concatenate([p.view(np.uint8).reshape(h, -1) for p in planes], axis=1)


def payload(img, pixel_type, lines, coded):
    """The bytes cnnitmo_exr_pack writes: record_bytes, each chunk of `lines` lines coded or not."""
    rows = record_bytes(img, pixel_type)
    if not coded:
        return rows.reshape(-1)
    h = rows.shape[0]
    return np.concatenate([code_chunk_fast(rows[y:y + lines].reshape(-1)) for y in range(0, h, lines)])
