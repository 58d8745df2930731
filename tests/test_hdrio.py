"""Host side of cnn_itmo_amd/hdrio.py without a GPU: the Radiance .hdr container (flat and
run-length encoded) and PFM against the independent readers / writers of tests/rgbe_ref.py, the
error behaviour of the parser, and the argument checks of the two RGBE entry points of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

from cnn_itmo_amd import hdrio as H
import rgbe_ref as RR

HEAD = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"


def _random(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _structured(seed=0):
    """[3, 640, 4]: per channel (shifted by the channel index) runs of 2, 3 and 4 equal bytes, a run
    of 300, 200 distinct bytes in a row, a short random rest."""
    rng = np.random.default_rng(seed)
    img = np.zeros((3, 640, 4), np.uint8)
    for y in range(3):
        for c in range(4):
            line = np.concatenate([np.full(2, 11), np.full(3, 22), np.full(4, 33), np.full(300, 44 + y),
                                   (np.arange(200) + 50) % 256, rng.integers(0, 256, 131)]).astype(np.uint8)
            img[y, :, c] = np.roll(line, 7 * c)
    return img


IMAGES = {
    "7x3": lambda: _random(3, 7, 1),        # below the run-length minimum: flat even with rle=True
    "8x2": lambda: _random(2, 8, 2),
    "53x5": lambda: _random(5, 53, 3),
    "smooth53": lambda: (_random(5, 53, 4) // 64) * 64,  # short runs everywhere
    "32767x1": lambda: (_random(1, 32767, 5) // 32) * 32,
    "32768x1": lambda: _random(1, 32768, 6),  # above the run-length maximum: flat
    "structured": _structured,
}


@pytest.mark.parametrize("rle", [False, True], ids=["flat", "rle"])
@pytest.mark.parametrize("name", list(IMAGES))
def test_container_round_trips_against_reference(name, rle):
    img = IMAGES[name]()
    h, w = img.shape[:2]
    data = H.format_hdr(img, rle=rle)
    assert data.startswith(HEAD + f"-Y {h} +X {w}\n".encode())
    body = len(data) - len(HEAD) - len(f"-Y {h} +X {w}\n")
    is_rle = rle and 8 <= w <= 32767
    assert is_rle or body == 4 * w * h  # flat: exactly the pixels
    if is_rle:
        assert data[len(data) - body:][:4] == bytes([2, 2, w >> 8, w & 255])
    # ours -> ours, ours -> reference reader, reference writer -> ours
    header, back = H.parse_hdr(data)
    assert back.dtype == np.uint8 and np.array_equal(back, img)
    assert (header["height"], header["width"], header["exposure"], header["format"]) == (h, w, 1.0, "32-bit_rle_rgbe")
    packets = []
    exposure, ref_back = RR.read_hdr(data, packets)
    assert exposure == 1.0 and np.array_equal(ref_back, img)
    assert bool(packets) == is_rle
    assert all(1 <= n <= (127 if kind == "run" else 128) for kind, n, _ in packets)
    _, from_ref = H.parse_hdr(RR.write_hdr(img, rle=is_rle))
    assert np.array_equal(from_ref, img)


def test_long_runs_and_long_literals_split():
    img = _structured()
    packets = []
    RR.read_hdr(H.format_hdr(img[:1], rle=True), packets)
    per_channel = len(packets) // 4
    assert sum(n for _, n, _ in packets) == 4 * 640
    runs44 = [n for kind, n, b in packets if kind == "run" and b == 44]
    assert len(runs44) >= 4 * 3 and sum(runs44) == 4 * 300 and max(runs44) <= 127  # 300 = 127 + 127 + 46
    lits = [n for kind, n, _ in packets if kind == "lit"]
    assert max(lits) <= 128 and sum(lits) >= 4 * 200 and len(lits) >= 4 * 2
    assert per_channel < 40  # runs and literals are merged into few packets, not one per byte


def test_constant_image_compresses():
    img = np.full((4, 100, 4), 77, np.uint8)
    rle, flat = H.format_hdr(img, rle=True), H.format_hdr(img, rle=False)
    assert len(rle) < len(flat) // 10
    assert np.array_equal(H.parse_hdr(rle)[1], img) and np.array_equal(RR.read_hdr(rle)[1], img)


def test_header_forms():
    img = _random(4, 9, 7)
    lines = ["# made by a test", "EXPOSURE=2.0", "SOFTWARE=none", "EXPOSURE=0.25", "VIEW= -vtv -vp 0 0 0",
             "# second comment"]
    for rle in (False, True):
        data = RR.write_hdr(img, rle=rle, magic="#?RGBE", lines=lines, orientation="+Y")
        header, back = H.parse_hdr(data)
        assert np.array_equal(back, img)  # +Y: stored bottom to top, returned top first
        assert header["exposure"] == 0.5 and header["orientation"] == "+Y +X" and header["magic"] == "#?RGBE"
        assert header["comments"] == ["# made by a test", "# second comment"]
        assert header["fields"] == {"SOFTWARE": "none", "VIEW": "-vtv -vp 0 0 0"}
    # the +Y body by hand: the first stored row is the bottom one
    data = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+Y 4 +X 9\n" + img[::-1].tobytes()
    assert np.array_equal(H.parse_hdr(data)[1], img)
    # no FORMAT line, CRLF-free spare spaces in the resolution line
    data = b"#?RADIANCE\n\n-Y  4  +X  9\n" + img.tobytes()
    assert np.array_equal(H.parse_hdr(data)[1], img)
    # a header written back: EXPOSURE survives
    again, _ = H.parse_hdr(H.format_hdr(img, header=header))
    assert again["exposure"] == 0.5 and again["fields"] == header["fields"] and again["comments"] == header["comments"]


def _rle_file(w, channels):
    return HEAD + f"-Y 1 +X {w}\n".encode() + bytes([2, 2, w >> 8, w & 255]) + bytes(channels)


def test_malformed_input_raises():
    img = (_random(2, 12, 8) // 128) * 128
    flat, rle = H.format_hdr(img, rle=False), H.format_hdr(img, rle=True)
    with pytest.raises(ValueError, match="magic"):
        H.parse_hdr(flat[2:])
    with pytest.raises(ValueError, match="magic"):
        H.parse_hdr(b"P6\n12 2\n255\n" + bytes(72))
    with pytest.raises(ValueError, match="truncated"):
        H.parse_hdr(flat[:-1])
    with pytest.raises(ValueError, match="truncated"):
        H.parse_hdr(rle[:-1])
    # every proper prefix of either file is an error: no IndexError, no endless loop
    for data in (flat, rle):
        for n in range(len(data)):
            with pytest.raises(ValueError):
                H.parse_hdr(data[:n])
    good = [128 + 8, 5] * 4
    assert np.array_equal(H.parse_hdr(_rle_file(8, good))[1], np.full((1, 8, 4), 5, np.uint8))
    with pytest.raises(ValueError, match="overruns"):
        H.parse_hdr(_rle_file(8, [128 + 9, 5] + good))  # a run of 9 in a scanline of 8
    with pytest.raises(ValueError, match="overruns"):
        H.parse_hdr(_rle_file(8, [128 + 5, 5, 4, 1, 2, 3, 4] + good))  # 5 + 4 literals
    with pytest.raises(ValueError, match="zero count"):
        H.parse_hdr(_rle_file(8, [128 + 4, 5, 0, 128 + 4, 5] + good))
    with pytest.raises(ValueError, match="truncated"):
        H.parse_hdr(_rle_file(8, [128 + 8, 5] * 3 + [128 + 8]))
    with pytest.raises(NotImplementedError, match="xyze"):
        H.parse_hdr(RR.write_hdr(img, fmt="32-bit_rle_xyze"))
    with pytest.raises(NotImplementedError, match="orientation"):
        H.parse_hdr(HEAD + b"-Y 2 -X 12\n" + img.tobytes())
    with pytest.raises(NotImplementedError, match="orientation"):
        H.parse_hdr(HEAD + b"+X 12 -Y 2\n" + img.tobytes())
    with pytest.raises(ValueError, match="truncated"):
        H.parse_hdr(HEAD + b"-Y 2000000000 +X 2000000000\n" + img.tobytes())  # no giant allocation either
    with pytest.raises(ValueError):
        H.format_hdr(img[..., :3])


def test_pfm_bit_exact(tmp_path):
    rng = np.random.default_rng(9)
    img = rng.standard_normal((5, 7, 3)).astype(np.float32)
    img[0, 0] = [np.inf, -np.inf, -0.0]
    img[1, 1] = [1e-45, -1e-40, np.finfo(np.float32).max]
    img[4, 6] = [np.finfo(np.float32).tiny, -3.5, 0.0]
    p = str(tmp_path / "a.pfm")
    H.write_pfm(p, img)
    raw = open(p, "rb").read()
    assert raw.startswith(b"PF\n7 5\n-1.0\n") and len(raw) == len(b"PF\n7 5\n-1.0\n") + 5 * 7 * 12
    assert raw[-7 * 12:] == img[0].astype("<f4").tobytes()  # the top row is stored last
    back = H.read_pfm(p)
    assert back.dtype == np.float32 and back.tobytes() == img.tobytes()
    assert RR.read_pfm(raw).tobytes() == img.tobytes()
    # reference-written files, either byte order
    for big in (False, True):
        with open(p, "wb") as fh:
            fh.write(RR.write_pfm(img, big_endian=big))
        assert H.read_pfm(p).tobytes() == img.tobytes()
    with open(p, "wb") as fh:
        fh.write(RR.write_pfm(img[..., :1].repeat(3, 2), magic="Pf"))
    with pytest.raises(ValueError, match="Pf"):
        H.read_pfm(p)
    with open(p, "wb") as fh:
        fh.write(RR.write_pfm(img)[:-1])
    with pytest.raises(ValueError, match="truncated"):
        H.read_pfm(p)
    for bad in ("x.exr", "x.png"):
        with pytest.raises(ValueError, match="extension"):
            H.write_image(str(tmp_path / bad), img)
        with pytest.raises(ValueError, match="extension"):
            H.read_image(str(tmp_path / bad))


def test_reference_codec_known_values():
    """The numpy restatement the GPU tests compare with, pinned on values worked out by hand."""
    x = np.float32([[1, 1, 1], [0.5, 0.25, 0.125], [1, 0, 0], [255 * 2.0 ** 119, 0, 2.0 ** 119], [1e-33, 0, 0],
                    [3, 1.5, 0.01], [np.inf, np.nan, -1]])
    want = np.uint8([[128, 128, 128, 129], [128, 64, 32, 128], [128, 0, 0, 129], [255, 0, 1, 255], [0, 0, 0, 0],
                     [192, 96, 0, 130], [255, 0, 0, 255]])
    assert np.array_equal(RR.encode(x), want)
    q = np.uint8([[128, 64, 32, 128], [255, 255, 255, 0], [1, 0, 255, 1], [255, 255, 255, 255], [3, 0, 0, 136]])
    got = RR.decode(q)
    want = np.float64([[0.5, 0.25, 0.125], [0, 0, 0], [2.0 ** -135, 0, 255 * 2.0 ** -135],
                       [255 * 2.0 ** 119] * 3, [3, 0, 0]])
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    x = RR.random_hdr((4000,), 1, hi=125)
    d = RR.decode(RR.encode(x)).astype(np.float64)
    assert (d <= x).all() and ((x - d) < 2.0 ** -7 * x.max(-1, keepdims=True)).all()
    assert np.array_equal(RR.encode(d.astype(np.float32)), RR.encode(x))


def test_abi_argument_checks():
    from cnn_itmo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    for name in ("cnnitmo_rgbe_encode", "cnnitmo_rgbe_decode"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    host = ctypes.create_string_buffer(64)  # never dereferenced: the checks come first
    p = ctypes.addressof(host)
    for fn in (lib.cnnitmo_rgbe_encode, lib.cnnitmo_rgbe_decode):
        for args, word in (((None, 4, p, None), b"null"), ((p, 4, None, None), b"null"), ((p, 0, p, None), b"npix"),
                           ((p, -3, p, None), b"npix")):
            assert fn(*args) == -1  # CNNITMO_EINVAL
            assert word in lib.cnnitmo_last_error(), lib.cnnitmo_last_error()
