"""OpenEXR files (``.exr``): single-part, scan-line, flat images.

No OpenEXR library is used or available here: this module is a restatement of the published
file layout (the "OpenEXR File Layout" document of the OpenEXR project), and
tests/exr_ref.py restates it a second time for the tests.

The layout, as far as it is used:

  magic 76 2F 31 01, then an int32 version field: low byte 2; flag 0x200 = tiled, 0x800 = deep
  ("non-image"), 0x1000 = multi-part (all three refused), 0x400 = long names (accepted).
  Header: attributes ``name\\0 type\\0 int32 size, value``, ended by a single ``\\0``.
    channels (chlist)    entries ``name\\0, int32 type (0 UINT, 1 HALF, 2 FLOAT), uint8 pLinear,
                         3 reserved bytes, int32 xSampling, int32 ySampling``, ended by ``\\0``; the
                         channels are stored, and laid out in the data, in this order (sorted by name)
    compression (uint8)  0 NONE, 1 RLE, 2 ZIPS, 3 ZIP, 4 PIZ, 5 PXR24, 6 B44, 7 B44A, 8 DWAA, 9 DWAB
    dataWindow, displayWindow (box2i: xMin, yMin, xMax, yMax, inclusive, may be negative)
    lineOrder (uint8: 0 increasing y, 1 decreasing y)
    pixelAspectRatio (float), screenWindowCenter (v2f), screenWindowWidth (float)
    Every other attribute is kept as raw bytes: header['other'][name] = (type, bytes).
  Then the offset table, one uint64 per chunk, then the chunks: ``int32 y, int32 size, data``.  A
  chunk holds L scan lines from y on: 1 for NONE and ZIPS, 16 for ZIP; the last may be short.
  Uncompressed chunk bytes: for each line, for each channel in list order, that channel's w values,
  little-endian; line_bytes = sum over the channels of w * sizeof(type).
  ZIP / ZIPS encoding of a chunk of n bytes: (1) split: even-indexed bytes to t[0 .. (n+1)/2),
  odd-indexed to the rest; (2) predict, left to right: t[i] <- t[i] - t_old[i-1] + 128 (mod 256),
  i >= 1; (3) deflate; (4) if the result is not smaller than n the chunk is stored raw: size == n,
  neither split nor predicted.  Decoding: inflate, t[i] <- t[i-1] + t[i] - 128 (mod 256), then
  out[2k] = t[k], out[2k+1] = t[(n+1)/2 + k].  Example: 00 3C 00 40 (halves 1.0, 2.0) splits to
  00 00 3C 40 and predicts to 00 80 BC 84.

Supported: compression NONE, ZIPS, ZIP; channel types UINT, HALF, FLOAT with xSampling =
ySampling = 1; both line orders.  NotImplementedError (naming what was found): tiled, deep or
multi-part files, the other compressions, subsampled channels, a file without R, G, B or Y.
Malformed input is a ValueError, raised before anything of the claimed size is allocated: a data
window whose raw size the file's bytes cannot hold (NONE: h * line_bytes plus the tables; ZIP / ZIPS:
more than 1032 x the file size, deflate's best ratio) is refused, and a chunk is inflated with
``zlib.decompressobj().decompress(data, expected + 1)`` so that it cannot expand past its size.

Which channels become RGB: R, G, B at the top level; otherwise a lone Y, replicated; any further
channel (A, Z, names with a dot) is skipped.  The picture is the data window, row 0 = top; values
are returned as stored (no chromaticities / whiteLuminance conversion).

The host does the container and zlib (a thread pool over chunks: zlib releases the GIL); the pixels
are GPU work (csrc/exr.hip): the inflated chunks go to the device as they are, 6 B per pixel for half
RGB, and cnnitmo_exr_unpack undoes the predictor and the split, picks the channels and converts;
cnnitmo_exr_pack makes the split and predicted record bytes of a picture for the writer.

  parse_exr(bytes) -> Parsed(header, layout, raw)
      raw: uint8 [h * line_bytes], the inflated chunks in increasing y; layout: dict with h, w,
      line_bytes, lines_per_chunk, nchunks, compression, channels [(name, type, offset)], ch_off,
      ch_type (of R, G, B) and coded: uint8 [nchunks], 1 = split and predicted, 0 = plain
  format_exr(payload, coded, h, w, pixel_type, compression, level=6, workers=8) -> bytes
      payload: uint8 [h * line_bytes] record bytes, channels B G R of one type, chunk i in the form
      coded[i] says; HALF / FLOAT; ZIP / ZIPS / NONE; increasing line order; data window =
      display window = (0, 0) - (w-1, h-1); the eight required attributes
  exr_size(path) -> (h, w) from the header alone
  unpack(parsed) -> CUDA float32 [h,w,3]
  read_exr(path, return_header=False) -> CUDA float32 [h,w,3]
  write_exr(path, img, pixel_type='half', compression='zip')
"""
from __future__ import annotations

import collections
import concurrent.futures as cf
import struct
import zlib

import numpy as np

MAGIC = b"\x76\x2f\x31\x01"
TILED, LONG_NAMES, DEEP, MULTIPART = 0x200, 0x400, 0x800, 0x1000
UINT, HALF, FLOAT = 0, 1, 2
TYPE_SIZE = {UINT: 4, HALF: 2, FLOAT: 4}
TYPE_NAMES = {"uint": UINT, "half": HALF, "float": FLOAT}
COMPRESSIONS = ("NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB")
NONE, ZIPS, ZIP = 0, 2, 3
LINES = {NONE: 1, ZIPS: 1, ZIP: 16}
COMPRESSION_NAMES = {"none": NONE, "zips": ZIPS, "zip": ZIP}
REQUIRED = ("channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio",
            "screenWindowCenter", "screenWindowWidth")
MAX_RATIO = 1032  # deflate cannot expand by more
WORKERS = 8

Parsed = collections.namedtuple("Parsed", "header layout raw")
Parsed.shape = property(lambda self: (self.layout["h"], self.layout["w"], 3))


# ------------------------------------------------------------------------------ header
def _cstr(buf, pos, what):
    end = buf.find(b"\0", pos)
    if end < 0:
        raise ValueError(f"exr: header is truncated (in {what})")
    return buf[pos:end], end + 1


def _fixed(name, typ, val, want, fmt):
    if typ != want or len(val) != struct.calcsize(fmt):
        raise ValueError(f"exr: attribute {name} is {typ!r} of {len(val)} bytes, expected {want}")
    out = struct.unpack(fmt, val)
    return out[0] if len(out) == 1 else out


def _chlist(val):
    chans, pos = [], 0
    while True:
        if pos >= len(val):
            raise ValueError("exr: channel list is truncated")
        if val[pos] == 0:
            break
        name, pos = _cstr(val, pos, "the channel list")
        if pos + 16 > len(val):
            raise ValueError("exr: channel list is truncated")
        typ, plinear, xs, ys = struct.unpack_from("<iB3xii", val, pos)
        pos += 16
        chans.append({"name": name.decode("latin-1"), "type": typ, "pLinear": plinear, "xSampling": xs,
                      "ySampling": ys})
    if not chans:
        raise ValueError("exr: empty channel list")
    return chans


def parse_header(data):
    """bytes (at least the header's) -> (header dict, position of the offset table)."""
    buf = bytes(data)
    if len(buf) < 8:
        raise ValueError("exr: file is truncated (no magic and version)")
    if buf[:4] != MAGIC:
        raise ValueError("exr: wrong magic (not an OpenEXR file)")
    version, = struct.unpack_from("<i", buf, 4)
    if version & 0xFF != 2:
        raise ValueError(f"exr: file format version {version & 0xFF}, expected 2")
    flags = version & ~0xFF
    for bit, what in ((TILED, "tiled"), (DEEP, "deep"), (MULTIPART, "multi-part")):
        if flags & bit:
            raise NotImplementedError(f"exr: {what} files are not supported (version flag 0x{bit:x})")
    if flags & ~LONG_NAMES:
        raise ValueError(f"exr: unknown version flags 0x{flags:x}")
    header = {"version": 2, "flags": flags, "other": {}}
    pos = 8
    while True:
        if pos >= len(buf):
            raise ValueError("exr: header is truncated (no end of header)")
        if buf[pos] == 0:
            pos += 1
            break
        name, pos = _cstr(buf, pos, "an attribute name")
        typ, pos = _cstr(buf, pos, "an attribute type")
        if pos + 4 > len(buf):
            raise ValueError("exr: header is truncated (in an attribute size)")
        size, = struct.unpack_from("<i", buf, pos)
        pos += 4
        if size < 0 or pos + size > len(buf):
            raise ValueError(f"exr: header is truncated or corrupt: attribute {name.decode('latin-1')} of {size} bytes "
                             "runs past the end of the file")
        val = buf[pos:pos + size]
        pos += size
        name, typ = name.decode("latin-1"), typ.decode("latin-1")
        if name == "channels":
            if typ != "chlist":
                raise ValueError(f"exr: attribute channels is {typ!r}, expected chlist")
            header[name] = _chlist(val)
        elif name in ("compression", "lineOrder"):
            header[name] = _fixed(name, typ, val, name, "<B")
        elif name in ("dataWindow", "displayWindow"):
            header[name] = _fixed(name, typ, val, "box2i", "<4i")
        elif name in ("pixelAspectRatio", "screenWindowWidth"):
            header[name] = _fixed(name, typ, val, "float", "<f")
        elif name == "screenWindowCenter":
            header[name] = _fixed(name, typ, val, "v2f", "<2f")
        else:
            header["other"][name] = (typ, val)
    for name in REQUIRED:
        if name not in header:
            raise ValueError(f"exr: required attribute {name} is missing")
    return header, pos


def _layout(header):
    """Sizes and the RGB channels of a parsed header; refuses what is not supported."""
    comp = header["compression"]
    if comp >= len(COMPRESSIONS):
        raise ValueError(f"exr: unknown compression {comp}")
    if comp not in LINES:
        raise NotImplementedError(f"exr: compression {COMPRESSIONS[comp]} is not supported (NONE, ZIPS, ZIP)")
    if header["lineOrder"] not in (0, 1):
        raise ValueError(f"exr: lineOrder {header['lineOrder']} (0 or 1; tiles' random order is not for scan lines)")
    x0, y0, x1, y1 = header["dataWindow"]
    w, h = x1 - x0 + 1, y1 - y0 + 1
    if w < 1 or h < 1:
        raise ValueError(f"exr: empty data window {header['dataWindow']}")
    chans, off = [], 0
    for c in header["channels"]:
        if c["type"] not in TYPE_SIZE:
            raise ValueError(f"exr: channel {c['name']} has the unknown pixel type {c['type']}")
        if c["xSampling"] != 1 or c["ySampling"] != 1:
            raise NotImplementedError(f"exr: channel {c['name']} is subsampled {c['xSampling']} x {c['ySampling']}: "
                                      "not supported")
        chans.append((c["name"], c["type"], off))
        off += w * TYPE_SIZE[c["type"]]
    by_name = {n: (t, o) for n, t, o in chans}
    if all(k in by_name for k in "RGB"):
        pick = [by_name[k] for k in "RGB"]
    elif "Y" in by_name and not any(k in by_name for k in "RGB"):
        pick = [by_name["Y"]] * 3
    else:
        raise NotImplementedError(f"exr: no R, G, B and no lone Y among the channels {[n for n, _, _ in chans]}")
    lines = LINES[comp]
    return {"h": h, "w": w, "line_bytes": off, "lines_per_chunk": lines, "nchunks": -(-h // lines),
            "compression": comp, "channels": chans, "ch_type": tuple(t for t, _ in pick),
            "ch_off": tuple(o for _, o in pick)}


def _inflate(data, n):
    """One ZIP / ZIPS chunk of n raw bytes -> (bytes, coded)."""
    if len(data) == n:
        return data, 0
    if len(data) > n:
        raise ValueError(f"exr: a chunk of {n} bytes is stored as {len(data)}")
    try:
        out = zlib.decompressobj().decompress(data, n + 1)
    except zlib.error as e:
        raise ValueError(f"exr: bad deflate stream ({e})") from None
    if len(out) != n:
        raise ValueError(f"exr: a chunk inflates to {'more than ' if len(out) > n else ''}{len(out)} bytes, "
                         f"expected {n}")
    return out, 1


def parse_exr(data, workers=WORKERS):
    """bytes of an OpenEXR file -> Parsed(header, layout, raw): see the module's docstring."""
    buf = bytes(data)
    header, pos = parse_header(buf)
    lay = _layout(header)
    h, lb, lines, nchunks, comp = lay["h"], lay["line_bytes"], lay["lines_per_chunk"], lay["nchunks"], \
        lay["compression"]
    table_end = pos + 8 * nchunks
    if table_end + 8 * nchunks > len(buf):
        raise ValueError(f"exr: a file of {len(buf)} bytes cannot hold {nchunks} chunks (offset table truncated)")
    if comp == NONE and table_end + 8 * nchunks + h * lb > len(buf):
        raise ValueError(f"exr: a file of {len(buf)} bytes cannot hold {h} uncompressed lines of {lb} bytes")
    if h * lb > MAX_RATIO * len(buf):
        raise ValueError(f"exr: a file of {len(buf)} bytes cannot hold a picture of {h * lb} bytes")
    offsets = struct.unpack_from(f"<{nchunks}Q", buf, pos)
    y0 = header["dataWindow"][1]
    jobs = [None] * nchunks
    for off in offsets:
        if off < table_end or off + 8 > len(buf):
            raise ValueError(f"exr: chunk offset {off} is outside the file's data")
        y, size = struct.unpack_from("<ii", buf, off)
        if size < 0 or off + 8 + size > len(buf):
            raise ValueError(f"exr: the chunk at {off} ({size} bytes) runs past the end of the file")
        i, rem = divmod(y - y0, lines)
        if rem or not 0 <= i < nchunks:
            raise ValueError(f"exr: the chunk at {off} starts at y = {y}: not a chunk start of the data window")
        if jobs[i] is not None:
            raise ValueError(f"exr: two chunks start at y = {y}")
        n = min(lines, h - i * lines) * lb
        if comp == NONE and size != n:
            raise ValueError(f"exr: an uncompressed chunk of {n} bytes is stored as {size}")
        jobs[i] = (off + 8, size, n)
    view = memoryview(buf)

    def one(job):
        at, size, n = job
        return (view[at:at + size], 0) if comp == NONE else _inflate(view[at:at + size], n)

    if comp == NONE or workers <= 1 or nchunks == 1:
        parts = [one(j) for j in jobs]
    else:
        with cf.ThreadPoolExecutor(max_workers=workers) as ex:
            parts = list(ex.map(one, jobs))
    raw = np.empty(h * lb, np.uint8)
    coded = np.zeros(nchunks, np.uint8)
    for i, (part, c) in enumerate(parts):
        at = i * lines * lb
        raw[at:at + len(part)] = np.frombuffer(part, np.uint8)
        coded[i] = c
    lay["coded"] = coded
    return Parsed(header, lay, raw)


def exr_size(path):
    """(h, w) of the data window from the header alone."""
    with open(path, "rb") as fh:
        buf = fh.read(1 << 16)
        try:
            header, _ = parse_header(buf)
        except ValueError:
            rest = fh.read()
            if not rest:
                raise
            header, _ = parse_header(buf + rest)
    x0, y0, x1, y1 = header["dataWindow"]
    if x1 < x0 or y1 < y0:
        raise ValueError(f"{path}: empty data window {header['dataWindow']}")
    return y1 - y0 + 1, x1 - x0 + 1


# ------------------------------------------------------------------------------ writer
def _attr(name, typ, val):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(val)) + val


def _unpredict(t):
    """uint8 [n], split and predicted -> the record bytes (the chunk the GPU coded did not shrink)."""
    n = t.size
    d = (np.cumsum(t, dtype=np.uint64) - 128 * np.arange(n, dtype=np.uint64)).astype(np.uint8)
    out = np.empty(n, np.uint8)
    out[0::2] = d[:(n + 1) // 2]
    out[1::2] = d[(n + 1) // 2:]
    return out


def format_exr(payload, coded, h, w, pixel_type=HALF, compression=ZIP, level=6, workers=WORKERS):
    """Record bytes -> the bytes of an OpenEXR file: see the module's docstring."""
    if pixel_type not in (HALF, FLOAT):
        raise ValueError(f"format_exr: pixel type {pixel_type} (HALF = 1 or FLOAT = 2)")
    if compression not in LINES:
        raise ValueError(f"format_exr: compression {compression} (NONE = 0, ZIPS = 2, ZIP = 3)")
    if h < 1 or w < 1:
        raise ValueError(f"format_exr: empty picture {h} x {w}")
    lines, lb = LINES[compression], 3 * w * TYPE_SIZE[pixel_type]
    nchunks = -(-h // lines)
    payload = np.ascontiguousarray(payload, np.uint8).reshape(-1)
    coded = np.asarray(coded, np.uint8).reshape(-1)
    if payload.size != h * lb or coded.size != nchunks:
        raise ValueError(f"format_exr: {payload.size} payload bytes and {coded.size} flags for a {h} x {w} picture "
                         f"of {h * lb} bytes in {nchunks} chunks")
    if compression == NONE and coded.any():
        raise ValueError("format_exr: compression NONE takes plain chunks only")

    def one(i):
        part = payload[i * lines * lb:(i + 1) * lines * lb]
        if not coded[i]:
            return part.tobytes()
        z = zlib.compress(part.tobytes(), level)
        return z if len(z) < part.size else _unpredict(part).tobytes()

    if compression == NONE or workers <= 1 or nchunks == 1:
        parts = [one(i) for i in range(nchunks)]
    else:
        with cf.ThreadPoolExecutor(max_workers=workers) as ex:
            parts = list(ex.map(one, range(nchunks)))
    chlist = b"".join(n + b"\0" + struct.pack("<iB3xii", pixel_type, 0, 1, 1) for n in (b"B", b"G", b"R")) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    out = bytearray(MAGIC + struct.pack("<i", 2))
    out += _attr("channels", "chlist", chlist)
    out += _attr("compression", "compression", struct.pack("<B", compression))
    out += _attr("dataWindow", "box2i", box)
    out += _attr("displayWindow", "box2i", box)
    out += _attr("lineOrder", "lineOrder", b"\0")
    out += _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    out += _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
    out += _attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
    out += b"\0"
    at = len(out) + 8 * nchunks
    for p in parts:
        out += struct.pack("<Q", at)
        at += 8 + len(p)
    for i, p in enumerate(parts):
        out += struct.pack("<ii", i * lines, len(p)) + p
    return bytes(out)


# ------------------------------------------------------------------------------ files (GPU)
def unpack(parsed):
    """Parsed -> CUDA float32 [h,w,3] (cnnitmo_exr_unpack; raw crosses PCIe as it is in the file)."""
    import torch
    from . import ops
    lay = parsed.layout
    raw = torch.from_numpy(parsed.raw).cuda()
    coded = torch.from_numpy(lay["coded"]).cuda() if lay["coded"].any() else None
    rgb = torch.empty((lay["h"], lay["w"], 3), dtype=torch.float32, device=raw.device)
    return ops.exr_unpack(raw, coded, lay["lines_per_chunk"], lay["line_bytes"], lay["ch_off"], lay["ch_type"], rgb)


def read_exr(path, return_header=False):
    """An OpenEXR file -> CUDA float32 [h,w,3], row 0 = top; with ``return_header`` also the header."""
    with open(path, "rb") as fh:
        parsed = parse_exr(fh.read())
    img = unpack(parsed)
    return (img, parsed.header) if return_header else img


def _code(name, table, what):
    key = name.lower() if isinstance(name, str) else name
    if key in table:
        return table[key]
    if key in table.values():
        return key
    raise ValueError(f"write_exr: {what} {name!r} ({', '.join(table)})")


def write_exr(path, img, pixel_type="half", compression="zip", level=6, workers=WORKERS):
    """numpy array or CUDA tensor [h,w,3] -> an OpenEXR file with the channels B, G, R
    (cnnitmo_exr_pack makes the record bytes on the GPU; the host deflates them)."""
    import torch
    from . import hdrio, ops
    ptype = _code(pixel_type, {"half": HALF, "float": FLOAT}, "pixel type")
    comp = _code(compression, COMPRESSION_NAMES, "compression")
    t = torch.as_tensor(hdrio._hw3(img, "write_exr"))
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    t = (t if t.is_cuda else t.cuda()).contiguous()
    h, w = int(t.shape[0]), int(t.shape[1])
    is_coded = comp != NONE
    out = torch.empty(h * 3 * w * TYPE_SIZE[ptype], dtype=torch.uint8, device=t.device)
    ops.exr_pack(t, ptype, LINES[comp], is_coded, out)
    coded = np.full(-(-h // LINES[comp]), int(is_coded), np.uint8)
    data = format_exr(out.cpu().numpy(), coded, h, w, ptype, comp, level, workers)
    with open(path, "wb") as fh:
        fh.write(data)
