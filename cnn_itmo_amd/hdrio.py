"""HDR image files: Radiance RGBE (``.hdr`` / ``.pic``) and PFM (``.pfm``).

Pixel codec (csrc/hdrio.hip behind the C ABI, on the GPU):

  rgbe_encode(x) -> uint8 [...,4]     fp32 RGB -> red, green, blue mantissas + shared exponent
  rgbe_decode(q) -> float32 [...,3]   the inverse map

  x, q: numpy arrays or CUDA tensors, ``[h,w,c]`` or ``[n,h,w,c]``; the results are CUDA tensors.
  Encode: NaN -> 0, components clamped to [0, 255 * 2^119]; v = max(r,g,b); v < 1e-32 ->
  (0,0,0,0); else frexp(v) = (m, e), mantissa = floor(ldexp(c, 8 - e)), exponent byte e + 128.
  Decode: exponent byte 0 -> black whatever the mantissas; else mantissa * 2^(E - 136), no +0.5
  (rgbe.c and MATLAB's hdrread).  Both are exact, so decode(encode(x)) <= x, short of x by less
  than 2^-7 of the pixel's largest component, and encode(decode(q)) == q for encoder output.

Container (host numpy, no GPU):

  parse_hdr(bytes) -> (header, rgbe uint8 [h,w,4])
  format_hdr(rgbe, rle=True, header=None) -> bytes

  The parser takes the ``#?RADIANCE`` / ``#?RGBE`` magic, ``FORMAT=32-bit_rle_rgbe`` (xyze raises
  NotImplementedError), ``EXPOSURE=`` lines (their product is header['exposure']), ``#`` comments
  (header['comments']) and any other line (``KEY=value`` into header['fields'], the rest into
  header['lines']); resolutions ``-Y h +X w`` and ``+Y h +X w`` (flipped: row 0 is always the top;
  other orientations raise NotImplementedError); flat scanlines and new-style run-length encoded
  ones (marker 2, 2, w >> 8, w & 255, then each of the four channels as packets: a count > 128 =
  count - 128 copies of the next byte, a count 1..128 = that many literal bytes).  Old-style
  run-length pixels (1, 1, 1, n) are not supported: such a file is read as flat pixels.
  The writer emits ``#?RADIANCE``, the format line, a blank line and ``-Y h +X w``, run-length
  encoded when ``rle`` and 8 <= w <= 32767, flat otherwise.  Malformed input is a ValueError.

Files:

  read_hdr(path, apply_exposure=False, return_header=False) -> CUDA float32 [h,w,3]
  write_hdr(path, img, rle=True)          img: numpy array or CUDA tensor [h,w,3]
  read_pfm(path) -> numpy float32 [h,w,3]; write_pfm(path, img)       colour 'PF', bit-exact
  read_image(path) -> CUDA float32 [h,w,3]; write_image(path, img)    by extension
  load_image(path) / save_image(path, img, **opts)    the same, and ``.exr`` through exr.py
      (opts: write_exr's pixel_type / compression); the front ends use this pair

  Only the 4 bytes/pixel RGBE form crosses PCIe for ``.hdr``.  ``apply_exposure`` divides the
  decoded pixels by the header's EXPOSURE product (the file holds radiance * EXPOSURE).
"""
from __future__ import annotations

import os
import re

import numpy as np

MAGICS = (b"#?RADIANCE", b"#?RGBE")
FORMAT_RGBE = "32-bit_rle_rgbe"
FORMAT_XYZE = "32-bit_rle_xyze"
MIN_RLE, MAX_RLE = 8, 32767


# ------------------------------------------------------------------------------ GPU codec
def _codec(x, cin, dtype, name):
    import torch
    from . import ops
    t = torch.as_tensor(x)
    if t.ndim not in (3, 4) or t.shape[-1] != cin or t.numel() == 0:
        raise ValueError(f"{name}: expected [h,w,{cin}] or [n,h,w,{cin}], got shape {tuple(t.shape)}")
    if t.dtype != dtype:
        t = t.to(dtype)
    t = (t if t.is_cuda else t.cuda()).contiguous()
    cout = 4 if cin == 3 else 3
    out = torch.empty(t.shape[:-1] + (cout,), dtype=torch.uint8 if cout == 4 else torch.float32, device=t.device)
    (ops.rgbe_encode if cin == 3 else ops.rgbe_decode)(t, out)
    return out


def rgbe_encode(x):
    """fp32 RGB [h,w,3] / [n,h,w,3] (numpy or CUDA tensor) -> CUDA uint8 [...,4]."""
    import torch
    return _codec(x, 3, torch.float32, "rgbe_encode")


def rgbe_decode(q):
    """uint8 RGBE [h,w,4] / [n,h,w,4] (numpy or CUDA tensor) -> CUDA float32 [...,3]."""
    import torch
    return _codec(q, 4, torch.uint8, "rgbe_decode")


# ------------------------------------------------------------------------------ .hdr container
def _line(buf, pos):
    """(line without its newline, position after it); the header must end inside the buffer."""
    end = buf.find(b"\n", pos)
    if end < 0:
        raise ValueError("hdr: header is truncated (no resolution line)")
    return buf[pos:end].rstrip(b"\r"), end + 1


def _unpack_channel(buf, pos, w, out):
    """One run-length encoded channel of a scanline into out[:w]; returns the new position."""
    n, x = len(buf), 0
    while x < w:
        if pos >= n:
            raise ValueError("hdr: run-length data is truncated")
        count = buf[pos]
        pos += 1
        if count == 0:
            raise ValueError("hdr: run-length packet with a zero count")
        if count > 128:
            count -= 128
            if pos >= n:
                raise ValueError("hdr: run-length data is truncated")
            if x + count > w:
                raise ValueError("hdr: run-length packet overruns its scanline")
            out[x:x + count] = buf[pos]
            pos += 1
        else:
            if x + count > w:
                raise ValueError("hdr: run-length packet overruns its scanline")
            if pos + count > n:
                raise ValueError("hdr: run-length data is truncated")
            out[x:x + count] = np.frombuffer(buf, np.uint8, count, pos)
            pos += count
        x += count
    return pos


def parse_hdr(data):
    """bytes of a Radiance picture -> (header dict, uint8 [h,w,4], row 0 = top)."""
    buf = bytes(data)
    first, pos = _line(buf, 0)
    if not first.startswith(MAGICS):
        raise ValueError("hdr: missing #?RADIANCE / #?RGBE magic line")
    header = {"magic": first.decode("latin-1"), "format": None, "exposure": 1.0, "comments": [], "fields": {},
              "lines": []}
    while True:
        raw, pos = _line(buf, pos)
        if not raw:
            break
        s = raw.decode("latin-1").strip()
        if s.startswith("#"):
            header["comments"].append(s)
        elif s.startswith("FORMAT="):
            header["format"] = s[7:].strip()
        elif s.startswith("EXPOSURE="):
            try:
                header["exposure"] *= float(s[9:])
            except ValueError:
                raise ValueError(f"hdr: bad header line {s!r}") from None
        elif "=" in s:
            k, v = s.split("=", 1)
            header["fields"][k.strip()] = v.strip()
        else:
            header["lines"].append(s)
    if header["format"] == FORMAT_XYZE:
        raise NotImplementedError("hdr: FORMAT=32-bit_rle_xyze (CIE XYZ pictures) is not supported")
    if header["format"] not in (None, FORMAT_RGBE):
        raise ValueError(f"hdr: unknown FORMAT={header['format']}")
    res, pos = _line(buf, pos)
    m = re.fullmatch(r"([-+][XY]) +(\d+) +([-+][XY]) +(\d+)", res.decode("latin-1").strip())
    if not m:
        raise ValueError(f"hdr: bad resolution line {res!r}")
    if (m.group(1), m.group(3)) not in (("-Y", "+X"), ("+Y", "+X")):
        raise NotImplementedError(f"hdr: orientation {m.group(1)} {m.group(3)} is not supported")
    h, w = int(m.group(2)), int(m.group(4))
    if h <= 0 or w <= 0:
        raise ValueError(f"hdr: empty picture {h} x {w}")
    header.update(orientation=f"{m.group(1)} {m.group(3)}", height=h, width=w)
    if len(buf) - pos < h * min(4 * w, 4 + 8):  # (a run-length scanline is at least 4 + 4*2 bytes)
        raise ValueError("hdr: pixel data is truncated")
    img = np.empty((h, w, 4), np.uint8)
    line = np.empty((4, w), np.uint8)
    n = len(buf)
    for y in range(h):
        if MIN_RLE <= w <= MAX_RLE and pos + 4 <= n and buf[pos] == 2 and buf[pos + 1] == 2 and \
                (buf[pos + 2] << 8 | buf[pos + 3]) == w:
            pos += 4
            for c in range(4):
                pos = _unpack_channel(buf, pos, w, line[c])
            img[y] = line.T
        else:
            if pos + 4 * w > n:
                raise ValueError("hdr: pixel data is truncated")
            img[y] = np.frombuffer(buf, np.uint8, 4 * w, pos).reshape(w, 4)
            pos += 4 * w
    if m.group(1) == "+Y":
        img = img[::-1].copy()
    return header, img


def _pack_channel(a, out):
    """Append the packets of one channel of a scanline (uint8 [w]) to the bytearray out: runs of
    three or more equal bytes as run packets (at most 127 each), the rest as literals (at most 128)."""
    w = a.shape[0]
    starts = np.concatenate(([0], np.flatnonzero(a[1:] != a[:-1]) + 1))
    lens = np.diff(np.concatenate((starts, [w])))

    def literals(lo, hi):
        while lo < hi:
            k = min(128, hi - lo)
            out.append(k)
            out.extend(a[lo:lo + k].tobytes())
            lo += k

    pos = 0
    for k in np.flatnonzero(lens >= 3):
        s, l = int(starts[k]), int(lens[k])
        literals(pos, s)
        pos = s + l
        while l > 0:
            r = min(127, l)
            out.append(128 + r)
            out.append(int(a[s]))
            l -= r
    literals(pos, w)


def format_hdr(rgbe, rle=True, header=None):
    """uint8 [h,w,4] (row 0 = top) -> the bytes of a Radiance picture.  ``header``: optional dict
    with 'exposure' (an EXPOSURE= line when not 1), 'comments', 'fields' and 'lines' as parse_hdr
    returns them."""
    q = np.ascontiguousarray(rgbe, np.uint8)
    if q.ndim != 3 or q.shape[2] != 4 or q.size == 0:
        raise ValueError(f"format_hdr: expected uint8 [h,w,4], got shape {q.shape}")
    h, w = q.shape[:2]
    header = header or {}
    out = bytearray(b"#?RADIANCE\n")
    for c in header.get("comments", ()):
        out += (c if c.startswith("#") else "# " + c).encode("latin-1") + b"\n"
    out += b"FORMAT=" + FORMAT_RGBE.encode() + b"\n"
    if float(header.get("exposure", 1.0)) != 1.0:
        out += b"EXPOSURE=" + repr(float(header["exposure"])).encode() + b"\n"
    for k, v in header.get("fields", {}).items():
        out += f"{k}={v}\n".encode("latin-1")
    for s in header.get("lines", ()):
        out += s.encode("latin-1") + b"\n"
    out += b"\n" + f"-Y {h} +X {w}\n".encode()
    if rle and MIN_RLE <= w <= MAX_RLE:
        for y in range(h):
            out += bytes((2, 2, w >> 8, w & 255))
            ch = np.ascontiguousarray(q[y].T)
            for c in range(4):
                _pack_channel(ch[c], out)
    else:
        out += q.tobytes()
    return bytes(out)


# ------------------------------------------------------------------------------ files
def _hw3(img, name):
    """numpy array or tensor, [h,w,3] or [1,h,w,3] -> the same object as [h,w,3]."""
    shape = tuple(img.shape)
    if len(shape) == 4 and shape[0] == 1:
        img, shape = img[0], shape[1:]
    if len(shape) != 3 or shape[2] != 3 or 0 in shape:
        raise ValueError(f"{name}: expected one [h,w,3] image, got shape {shape}")
    return img


def read_hdr(path, apply_exposure=False, return_header=False):
    """A Radiance picture -> CUDA float32 [h,w,3] (decoded on the GPU); with ``return_header``
    also the header dict.  ``apply_exposure``: divide by the EXPOSURE product."""
    with open(path, "rb") as fh:
        header, q = parse_hdr(fh.read())
    img = rgbe_decode(q)
    if apply_exposure and header["exposure"] != 1.0:
        img = img / float(header["exposure"])
    return (img, header) if return_header else img


def write_hdr(path, img, rle=True):
    """numpy array or CUDA tensor [h,w,3] -> a Radiance picture (encoded on the GPU)."""
    q = rgbe_encode(_hw3(img, "write_hdr")).cpu().numpy()
    with open(path, "wb") as fh:
        fh.write(format_hdr(q, rle=rle))


def read_pfm(path):
    """Colour PFM ('PF') -> numpy float32 [h,w,3], row 0 = top (the file stores bottom to top);
    either byte order (a negative scale = little-endian).  Grey 'Pf' raises ValueError."""
    with open(path, "rb") as fh:
        buf = fh.read()
    m = re.match(rb"(P[Ff])\s+(\d+)\s+(\d+)\s+([-+0-9.eE]+)[ \t\r]?\n", buf)
    if not m:
        raise ValueError(f"{path}: not a PFM file")
    if m.group(1) != b"PF":
        raise ValueError(f"{path}: grey-scale PFM ('Pf') is not supported")
    w, h, scale = int(m.group(2)), int(m.group(3)), float(m.group(4))
    if w <= 0 or h <= 0 or scale == 0.0:
        raise ValueError(f"{path}: bad PFM header {m.group(0)!r}")
    if len(buf) - m.end() < 12 * w * h:
        raise ValueError(f"{path}: pixel data is truncated")
    a = np.frombuffer(buf, "<f4" if scale < 0 else ">f4", 3 * w * h, m.end()).reshape(h, w, 3)
    return a[::-1].astype(np.float32)  # (a byte swap for '>f4': no value changes)


def write_pfm(path, img):
    """numpy array or tensor [h,w,3] -> colour PFM, little-endian (scale -1.0), rows bottom to top."""
    img = _hw3(img, "write_pfm")
    a = img.detach().cpu().numpy() if hasattr(img, "detach") else np.asarray(img)
    a = np.ascontiguousarray(a, np.float32)
    with open(path, "wb") as fh:
        fh.write(f"PF\n{a.shape[1]} {a.shape[0]}\n-1.0\n".encode())
        fh.write(a[::-1].astype("<f4", copy=False).tobytes())


def _ext(path):
    return os.path.splitext(str(path))[1].lower()


def read_image(path):
    """``.hdr`` / ``.pic`` / ``.pfm`` -> CUDA float32 [h,w,3]."""
    import torch
    e = _ext(path)
    if e in (".hdr", ".pic"):
        return read_hdr(path)
    if e == ".pfm":
        return torch.from_numpy(read_pfm(path)).cuda()
    raise ValueError(f"{path}: unknown HDR image extension {e!r} (.hdr, .pic, .pfm)")


def write_image(path, img):
    """numpy array or CUDA tensor [h,w,3] -> ``.hdr`` / ``.pic`` (run-length encoded) or ``.pfm``."""
    e = _ext(path)
    if e in (".hdr", ".pic"):
        return write_hdr(path, img)
    if e == ".pfm":
        return write_pfm(path, img)
    raise ValueError(f"{path}: unknown HDR image extension {e!r} (.hdr, .pic, .pfm)")


def load_image(path):
    """``.exr`` (exr.read_exr) or what read_image takes -> CUDA float32 [h,w,3]."""
    if _ext(path) == ".exr":
        from . import exr
        return exr.read_exr(path)
    return read_image(path)


def save_image(path, img, **opts):
    """numpy array or CUDA tensor [h,w,3] -> ``.exr`` (exr.write_exr with ``opts``: half ZIP by
    default) or what write_image takes (no options)."""
    if _ext(path) == ".exr":
        from . import exr
        return exr.write_exr(path, img, **opts)
    if opts:
        raise TypeError(f"{path}: options {sorted(opts)} are for .exr files")
    return write_image(path, img)
