"""cnn_itmo_amd/exr.py on the CPU: the container parser and writer against tests/exr_ref.py (byte
for byte, bit for bit), every refusal, and the front ends' host side.  The pixel kernels are
tests/test_gpu_exr.py's."""
import contextlib
import io
import os
import struct
import zlib

import numpy as np
import pytest

import exr_ref as ER
from cnn_itmo_amd import evaluate_hdr, exr, hdrgen, hdrio, make_dataset

SIZES = [(1, 1), (3, 5), (17, 23), (16, 40)]  # ZIP: 17 = one full chunk + one line, 16 = exactly one chunk
COMPRESSIONS = [exr.NONE, exr.ZIPS, exr.ZIP]


def picture(h, w, seed=0):
    rng = np.random.default_rng(seed)
    return (np.exp(rng.uniform(-8, 8, (h, w, 3))) * rng.choice([1, 1, 1, -1], (h, w, 3))).astype(np.float32)


def smooth(h, w):
    """A picture that deflates well in every chunk."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x + y, x * 0.5 + 1, y + 2.0], -1).astype(np.float32)


def rgb_channels(img, dtype):
    with np.errstate(over="ignore"):
        return {"R": img[..., 0].astype(dtype), "G": img[..., 1].astype(dtype), "B": img[..., 2].astype(dtype)}


def host_pixels(parsed):
    """parse_exr's result -> float32 [h,w,3] through the reference's chunk decoder (what the GPU
    does in exr.unpack)."""
    lay = parsed.layout
    h, w, lb, lines = lay["h"], lay["w"], lay["line_bytes"], lay["lines_per_chunk"]
    rec = parsed.raw.copy()
    for i in range(lay["nchunks"]):
        lo, hi = i * lines * lb, min(h, (i + 1) * lines) * lb
        if lay["coded"][i]:
            rec[lo:hi] = ER.decode_chunk(parsed.raw[lo:hi])
    rows = rec.reshape(h, lb)
    planes = []
    for off, typ in zip(lay["ch_off"], lay["ch_type"]):
        dt = ER.DTYPES[typ]
        planes.append(np.ascontiguousarray(rows[:, off:off + w * dt.itemsize]).view(dt).reshape(h, w)
                      .astype(np.float32))
    return np.stack(planes, -1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------ the chunk coding
def test_worked_example():
    r = np.array([0x00, 0x3C, 0x00, 0x40], np.uint8)
    assert r.view("<f2").tolist() == [1.0, 2.0]
    split = np.concatenate([r[0::2], r[1::2]])
    assert split.tolist() == [0x00, 0x00, 0x3C, 0x40]
    coded = ER.code_chunk(r)
    assert coded.tolist() == [0x00, 0x80, 0xBC, 0x84]
    assert ER.decode_chunk(coded).tolist() == r.tolist()
    assert exr._unpredict(coded).tolist() == r.tolist()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 1001])
def test_reference_chunk_coding(n):
    r = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    t = ER.code_chunk(r)
    assert np.array_equal(ER.code_chunk_fast(r), t)
    assert np.array_equal(ER.decode_chunk(t), r)
    assert np.array_equal(exr._unpredict(t), r)


# ------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("comp", COMPRESSIONS)
@pytest.mark.parametrize("hw", SIZES)
def test_parse_reference_files(hw, comp, dtype):
    img = picture(*hw, seed=hw[0]) if hw[0] % 2 else smooth(*hw)
    chans = rgb_channels(img, dtype)
    data, coded = ER.build(chans, compression=comp)
    header, got, raw, coded2 = ER.take_apart(data)
    assert np.array_equal(coded, coded2)
    for k in "RGB":  # the reference reads what it wrote
        assert np.array_equal(got[k].view(np.uint8), chans[k].view(np.uint8))
    p = exr.parse_exr(data)
    assert p.header == header
    assert np.array_equal(p.raw, raw) and np.array_equal(p.layout["coded"], coded)
    lay = p.layout
    size = np.dtype(dtype).itemsize
    assert (lay["h"], lay["w"], lay["line_bytes"]) == (hw[0], hw[1], 3 * hw[1] * size)
    assert lay["lines_per_chunk"] == (16 if comp == exr.ZIP else 1) and lay["nchunks"] == len(coded)
    assert lay["ch_off"] == (2 * hw[1] * size, hw[1] * size, 0)  # B, G, R in the file
    assert lay["ch_type"] == (1 if dtype == np.float16 else 2,) * 3
    assert np.array_equal(bits(host_pixels(p)), bits(ER.rgb(chans)))
    assert p.shape == hw + (3,)


@pytest.mark.parametrize("ptype", [exr.HALF, exr.FLOAT])
@pytest.mark.parametrize("comp", COMPRESSIONS)
@pytest.mark.parametrize("hw", SIZES)
def test_format_exr_read_by_the_reference(hw, comp, ptype):
    img = picture(*hw, seed=7) if hw[0] % 2 else smooth(*hw)
    lines = exr.LINES[comp]
    is_coded = comp != exr.NONE
    pay = ER.payload(img, ptype, lines, is_coded)
    nchunks = -(-hw[0] // lines)
    data = exr.format_exr(pay, np.full(nchunks, int(is_coded), np.uint8), hw[0], hw[1], ptype, comp)
    header, got, raw, coded = ER.take_apart(data)
    want = ER.record_bytes(img, ptype)
    dt = ER.DTYPES[ptype]
    for k, name in enumerate("BGR"):
        plane = np.ascontiguousarray(want[:, k * hw[1] * dt.itemsize:(k + 1) * hw[1] * dt.itemsize]).view(dt)
        assert np.array_equal(got[name].view(np.uint8), plane.view(np.uint8))
    assert header["compression"] == comp and header["lineOrder"] == 0
    assert header["dataWindow"] == header["displayWindow"] == (0, 0, hw[1] - 1, hw[0] - 1)
    assert [c["name"] for c in header["channels"]] == ["B", "G", "R"] and header["other"] == {}
    assert (header["pixelAspectRatio"], header["screenWindowCenter"], header["screenWindowWidth"]) == \
        (1.0, (0.0, 0.0), 1.0)
    # the same file as the reference builds from the same picture, and the parser agrees with its reader
    ref_file, ref_coded = ER.build({n: got[n] for n in "BGR"}, compression=comp)
    assert data == ref_file and np.array_equal(coded, ref_coded)
    p = exr.parse_exr(data)
    assert p.header == header and np.array_equal(p.raw, raw) and np.array_equal(p.layout["coded"], coded)


def test_store_raw_rule_both_kinds():
    """Noise chunks do not deflate and are stored raw, neither split nor predicted, next to flat chunks
    that are coded: in the reference's files and in format_exr's."""
    h, w = 48, 40
    img = smooth(h, w)
    img[16:32] = np.random.default_rng(0).integers(0, 2 ** 32, (16, w, 3), dtype=np.uint64).astype(np.uint32) \
        .view(np.float32)
    img = np.where(np.isfinite(img), img, 1.0).astype(np.float32)
    data, coded = ER.build(rgb_channels(img, np.float32), compression=exr.ZIP)
    assert coded.tolist() == [1, 0, 1]
    p = exr.parse_exr(data)
    assert p.layout["coded"].tolist() == [1, 0, 1]
    assert np.array_equal(bits(host_pixels(p)), bits(img))
    ours = exr.format_exr(ER.payload(img, exr.FLOAT, 16, True), np.ones(3, np.uint8), h, w, exr.FLOAT, exr.ZIP)
    assert ours == data
    for workers in (1, 8):
        assert exr.format_exr(ER.payload(img, exr.FLOAT, 16, True), np.ones(3, np.uint8), h, w, exr.FLOAT, exr.ZIP,
                              workers=workers) == data
        assert np.array_equal(exr.parse_exr(data, workers=workers).raw, p.raw)


# ------------------------------------------------------------------------------ layouts
def test_mixed_types_and_skipped_channels():
    h, w = 17, 23
    rng = np.random.default_rng(3)
    img = picture(h, w, 3)
    chans = {"B": img[..., 2].astype(np.float16), "G": img[..., 1].copy(),
             "R": rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32),
             "A": np.ones((h, w), np.float16), "Z": rng.random((h, w)).astype(np.float32),
             "diffuse.R": rng.random((h, w)).astype(np.float16)}
    for comp in COMPRESSIONS:
        data, _ = ER.build(chans, compression=comp)
        p = exr.parse_exr(data)
        assert [c[0] for c in p.layout["channels"]] == ["A", "B", "G", "R", "Z", "diffuse.R"]
        assert p.layout["ch_type"] == (0, 2, 1)
        assert p.layout["ch_off"] == (2 * w + 2 * w + 4 * w, 2 * w + 2 * w, 2 * w)
        assert p.layout["line_bytes"] == w * (2 + 2 + 4 + 4 + 4 + 2)
        assert np.array_equal(bits(host_pixels(p)), bits(ER.rgb(chans)))


def test_lone_y_and_channel_sets():
    y = picture(3, 5)[..., 0].astype(np.float16)
    p = exr.parse_exr(ER.build({"Y": y, "A": np.ones((3, 5), np.float16)})[0])
    assert p.layout["ch_off"] == (10, 10, 10) and p.layout["ch_type"] == (1, 1, 1)
    assert np.array_equal(bits(host_pixels(p)), bits(ER.rgb({"Y": y})))
    with pytest.raises(NotImplementedError, match="RY"):
        exr.parse_exr(ER.build({"RY": y, "BY": y, "A": y})[0])
    with pytest.raises(NotImplementedError, match="'R', 'Y'"):
        exr.parse_exr(ER.build({"R": y, "Y": y})[0])
    with pytest.raises(NotImplementedError, match="diffuse.R"):
        exr.parse_exr(ER.build({"diffuse.R": y, "diffuse.G": y, "diffuse.B": y})[0])


@pytest.mark.parametrize("comp", COMPRESSIONS)
def test_line_order_window_and_long_names(comp):
    img = smooth(37, 11)
    chans = rgb_channels(img, np.float16)
    want = bits(ER.rgb(chans))
    for table_in_file_order in (False, True):
        data, _ = ER.build(chans, compression=comp, line_order=1, table_in_file_order=table_in_file_order)
        p = exr.parse_exr(data)
        assert p.header["lineOrder"] == 1 and np.array_equal(bits(host_pixels(p)), want)
    data, _ = ER.build(chans, compression=comp, origin=(-3, 7), display=(0, 0, 99, 99))
    p = exr.parse_exr(data)
    assert p.header["dataWindow"] == (-3, 7, 7, 43) and p.header["displayWindow"] == (0, 0, 99, 99)
    assert np.array_equal(bits(host_pixels(p)), want)
    long_name = "a_layer_name_of_more_than_thirty_one_characters.R"
    data, _ = ER.build(dict(chans, **{long_name: chans["R"]}), compression=comp, flags=0x400,
                       extra=[("owner", "string", b"somebody"), ("chromaticities", "chromaticities", bytes(32))])
    p = exr.parse_exr(data)
    assert p.header["flags"] == 0x400 and np.array_equal(bits(host_pixels(p)), want)
    assert p.header["other"] == {"owner": ("string", b"somebody"), "chromaticities": ("chromaticities", bytes(32))}
    assert p.header == ER.take_apart(data)[0]


# ------------------------------------------------------------------------------ refusals
def small_file(comp=exr.ZIP, **kw):
    return ER.build(rgb_channels(smooth(20, 6), np.float16), compression=comp, **kw)[0]


def set_version(data, version):
    return data[:4] + struct.pack("<i", version) + data[8:]


def test_not_implemented():
    data = small_file()
    for flag, word in ((0x200, "tiled"), (0x800, "deep"), (0x1000, "multi-part")):
        with pytest.raises(NotImplementedError, match=word):
            exr.parse_exr(set_version(data, 2 | flag))
    at = data.index(b"compression\0compression\0") + 24 + 4
    assert data[at] == exr.ZIP
    for code, name in ((1, "RLE"), (4, "PIZ"), (5, "PXR24"), (6, "B44"), (7, "B44A"), (8, "DWAA"), (9, "DWAB")):
        with pytest.raises(NotImplementedError, match=name):
            exr.parse_exr(data[:at] + bytes([code]) + data[at + 1:])
    with pytest.raises(ValueError, match="compression"):
        exr.parse_exr(data[:at] + bytes([10]) + data[at + 1:])
    for sampling in ((2, 1), (1, 2), (2, 2)):
        with pytest.raises(NotImplementedError, match="subsampled"):
            exr.parse_exr(small_file(sampling={"B": sampling}))


def test_malformed_headers():
    data = small_file()
    with pytest.raises(ValueError, match="magic"):
        exr.parse_exr(b"\x76\x2f\x31\x02" + data[4:])
    with pytest.raises(ValueError, match="magic"):
        exr.parse_exr(b"#?RADIANCE\n" + data)
    with pytest.raises(ValueError, match="version"):
        exr.parse_exr(set_version(data, 3))
    with pytest.raises(ValueError, match="flags"):
        exr.parse_exr(set_version(data, 2 | 0x2000))
    header_end = ER.take_apart(data) and data.index(b"screenWindowWidth\0float\0") + 24 + 4 + 4 + 1
    table_end = header_end + 8 * 2
    # every prefix of the header and the offset table, cut at each byte: always a ValueError
    for cut in range(0, table_end):
        with pytest.raises(ValueError):
            exr.parse_exr(data[:cut])
    # the structural boundaries by name: after the magic, inside the version, an attribute name, its
    # type, its size, its value, before the end-of-header byte, inside the offset table
    name_at = data.index(b"dataWindow\0")
    for cut, word in ((0, "truncated"), (4, "truncated"), (6, "truncated"), (8, "truncated"),
                      (name_at + 4, "truncated"), (name_at + 13, "truncated"), (name_at + 19, "truncated"),
                      (name_at + 30, "past the end"), (header_end - 1, "truncated"), (header_end + 3, "offset table")):
        with pytest.raises(ValueError, match=word):
            exr.parse_exr(data[:cut])
    for name in exr.REQUIRED:
        with pytest.raises(ValueError, match=name):
            exr.parse_exr(ER.build(rgb_channels(smooth(4, 6), np.float16), omit=(name,))[0])
    # a negative attribute size, an attribute of the wrong type, an empty window, an unknown pixel type
    size_at = name_at + len(b"dataWindow\0box2i\0")
    with pytest.raises(ValueError, match="past the end"):
        exr.parse_exr(data[:size_at] + struct.pack("<i", -1) + data[size_at + 4:])
    with pytest.raises(ValueError, match="dataWindow"):
        exr.parse_exr(data.replace(b"dataWindow\0box2i\0", b"dataWindow\0box2f\0"))
    with pytest.raises(ValueError, match="empty data window"):
        exr.parse_exr(data[:size_at + 4] + struct.pack("<4i", 0, 0, -1, 5) + data[size_at + 20:])
    type_at = data.index(b"channels\0chlist\0") + 16 + 4 + 2
    assert struct.unpack_from("<i", data, type_at)[0] == 1
    with pytest.raises(ValueError, match="pixel type"):
        exr.parse_exr(data[:type_at] + struct.pack("<i", 3) + data[type_at + 4:])


@pytest.mark.parametrize("comp", COMPRESSIONS)
def test_malformed_chunks(comp):
    data = small_file(comp)
    header, _, _, _ = ER.take_apart(data)
    lines = exr.LINES[comp]
    nchunks = -(-20 // lines)
    table = len(data) - len(data.split(b"screenWindowWidth\0float\0", 1)[1]) + 4 + 4 + 1
    offsets = list(struct.unpack_from(f"<{nchunks}Q", data, table))
    assert offsets[0] == table + 8 * nchunks

    def with_offset(k, value):
        return data[:table + 8 * k] + struct.pack("<Q", value) + data[table + 8 * (k + 1):]

    for value in (len(data), len(data) - 7, 2 ** 63, 0, table):  # past the end, and inside the header / table
        with pytest.raises(ValueError, match="offset"):
            exr.parse_exr(with_offset(nchunks - 1, value))
    with pytest.raises(ValueError, match="two chunks"):
        exr.parse_exr(with_offset(nchunks - 1, offsets[0]))
    for cut in (1, 9):  # the last chunk loses its tail
        with pytest.raises(ValueError, match="cannot hold" if comp == exr.NONE else "past the end"):
            exr.parse_exr(data[:-cut])
    at = offsets[-1]
    y, size = struct.unpack_from("<ii", data, at)
    for bad_y in (y + 1 if lines > 1 else 20, -lines, y + lines, 2 ** 31 - 1, -2 ** 31):
        with pytest.raises(ValueError, match="chunk start"):
            exr.parse_exr(data[:at] + struct.pack("<i", bad_y) + data[at + 4:])
    for bad_size in (-1, size + 1, 2 ** 31 - 1):
        with pytest.raises(ValueError, match="past the end"):
            exr.parse_exr(data[:at + 4] + struct.pack("<i", bad_size) + data[at + 8:])


@pytest.mark.parametrize("comp", [exr.ZIPS, exr.ZIP])
def test_chunks_inflating_to_the_wrong_size(comp):
    img = smooth(20, 64)  # a line of 384 bytes deflates to fewer
    good, coded = ER.build(rgb_channels(img, np.float16), compression=comp)
    assert coded.all()
    table = len(good) - len(good.split(b"screenWindowWidth\0float\0", 1)[1]) + 4 + 4 + 1
    nchunks = -(-20 // exr.LINES[comp])
    at = struct.unpack_from("<Q", good, table + 8 * (nchunks - 1))[0]  # the last chunk: the file's tail
    y, size = struct.unpack_from("<ii", good, at)
    rec = zlib.decompress(good[at + 8:])
    for change, word in ((rec + b"\0", "more than"), (rec[:-1], "inflates to"), (rec + bytes(5000), "more than")):
        z = zlib.compress(change, 6)
        assert len(z) < len(rec)
        with pytest.raises(ValueError, match=word):
            exr.parse_exr(good[:at] + struct.pack("<ii", y, len(z)) + z)
    for junk in (b"\x78\x9c" + b"\xff" * (size - 2), good[at + 8:-3] + b"\xff\xff\xff", bytes(size)):
        assert len(junk) == size
        with pytest.raises(ValueError):  # a zlib.error, or a stream that ends early
            exr.parse_exr(good[:at + 8] + junk)
    with pytest.raises(ValueError, match="stored as"):  # larger than its raw size
        exr.parse_exr(good[:at] + struct.pack("<ii", y, len(rec) + 1) + rec + b"\0")


def test_huge_data_window_is_refused_without_allocating():
    """A 2^30-wide (or -high, or 2^32-square) data window in a file of a few hundred bytes.  The
    eight required attributes alone take more than 200 bytes, so the file cut to 200 bytes is a
    truncated header; the whole header with a short tail is refused for its size.  Neither
    allocates anything of the claimed size."""
    import tracemalloc
    data = small_file(exr.ZIP)
    at = data.index(b"dataWindow\0box2i\0") + 17 + 4
    cat = data.index(b"compression\0compression\0") + 24 + 4
    header_end = data.index(b"screenWindowWidth\0float\0") + 24 + 4 + 4 + 1
    for comp in COMPRESSIONS:
        for box in ((0, 0, 2 ** 30 - 1, 0), (0, 0, 0, 2 ** 30 - 1), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)):
            bad = data[:cat] + bytes([comp]) + data[cat + 1:at] + struct.pack("<4i", *box) + data[at + 16:]
            for size, word in ((200, "truncated"), (header_end + 40, "cannot hold")):
                tracemalloc.start()
                with pytest.raises(ValueError, match=word):
                    exr.parse_exr(bad[:size])
                peak = tracemalloc.get_traced_memory()[1]
                tracemalloc.stop()
                assert peak < 1 << 20, peak


def test_format_exr_arguments():
    pay = ER.payload(smooth(3, 5), exr.HALF, 16, True)
    for args in ((pay, [1], 3, 5, 0, exr.ZIP), (pay, [1], 3, 5, exr.HALF, 1), (pay, [1, 1], 3, 5, exr.HALF, exr.ZIP),
                 (pay[:-1], [1], 3, 5, exr.HALF, exr.ZIP), (pay, [1, 1, 1], 3, 5, exr.HALF, exr.NONE),
                 (pay, [1], 0, 5, exr.HALF, exr.ZIP)):
        with pytest.raises(ValueError):
            exr.format_exr(*args)


# ------------------------------------------------------------------------------ front ends (host side)
def test_exr_size_and_sources(tmp_path):
    img = picture(19, 31)
    for name, comp, kw in (("a.exr", exr.ZIP, {}), ("b.EXR", exr.NONE, {"origin": (-3, 7)}),
                           ("c.exr", exr.ZIPS, {"extra": [("preview", "bytes", bytes(100000))]})):
        path = str(tmp_path / name)
        data, _ = ER.build(rgb_channels(img, np.float16), compression=comp, **kw)
        open(path, "wb").write(data)
        assert exr.exr_size(path) == (19, 31) and hdrgen.image_size(path) == (19, 31)
        src = hdrgen.read_source(path)
        assert isinstance(src, exr.Parsed) and src.shape == (19, 31, 3)
        assert np.array_equal(src.raw, exr.parse_exr(data).raw)
        open(path, "wb").write(data[:40])
        with pytest.raises(ValueError, match="truncated"):
            exr.exr_size(path)
    assert ".exr" in make_dataset.EXTENSIONS and ".exr" in evaluate_hdr.EXTENSIONS
    assert hdrgen.EXTENSIONS is make_dataset.EXTENSIONS
    open(str(tmp_path / "a.exr"), "wb").write(b"x")
    open(str(tmp_path / "a.hdr"), "wb").write(b"x")
    assert evaluate_hdr.find_reference(str(tmp_path), "a") == str(tmp_path / "a.hdr")  # the old order first
    assert evaluate_hdr.find_reference(str(tmp_path), "c") == str(tmp_path / "c.exr")
    assert [os.path.basename(f) for f in evaluate_hdr.hdr_files(str(tmp_path))] == ["a.exr", "a.hdr", "b.EXR", "c.exr"]


def test_load_and_save_dispatch(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(exr, "read_exr", lambda path: calls.append(("read_exr", path)) or "exr picture")
    monkeypatch.setattr(exr, "write_exr", lambda path, img, **kw: calls.append(("write_exr", path, img, kw)))
    monkeypatch.setattr(hdrio, "read_image", lambda path: calls.append(("read_image", path)) or "old picture")
    monkeypatch.setattr(hdrio, "write_image", lambda path, img: calls.append(("write_image", path, img)))
    assert hdrio.load_image("x.exr") == "exr picture" and hdrio.load_image("x.EXR") == "exr picture"
    assert hdrio.load_image("x.hdr") == "old picture" and hdrio.load_image("x.png") == "old picture"
    hdrio.save_image("y.exr", 1)
    hdrio.save_image("y.exr", 2, pixel_type="float", compression="zips")
    hdrio.save_image("y.pfm", 3)
    with pytest.raises(TypeError, match="pixel_type"):
        hdrio.save_image("y.pfm", 4, pixel_type="float")
    assert calls == [("read_exr", "x.exr"), ("read_exr", "x.EXR"), ("read_image", "x.hdr"), ("read_image", "x.png"),
                     ("write_exr", "y.exr", 1, {}),
                     ("write_exr", "y.exr", 2, {"pixel_type": "float", "compression": "zips"}),
                     ("write_image", "y.pfm", 3)]
    monkeypatch.undo()
    for bad in ("x.png", "x.tif"):  # the old pair's refusal comes through
        with pytest.raises(ValueError, match="extension"):
            hdrio.load_image(bad)
        with pytest.raises(ValueError, match="extension"):
            hdrio.save_image(bad, np.zeros((2, 2, 3), np.float32))


def test_generator_draws_over_exr_equal_those_over_pfm(tmp_path):
    sizes = [(37, 53), (41, 47), (30, 64), (64, 64), (25, 41)]
    for kind in ("pfm", "exr"):
        os.makedirs(str(tmp_path / kind))
    for k, (h, w) in enumerate(sizes):
        img = picture(h, w, k)
        hdrio.write_pfm(str(tmp_path / "pfm" / f"{k:02d}.pfm"), img)
        comp = COMPRESSIONS[k % 3]
        open(str(tmp_path / "exr" / f"{k:02d}.exr"), "wb").write(ER.build(rgb_channels(img, np.float16),
                                                                           compression=comp)[0])
    args = dict(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2)
    with contextlib.redirect_stdout(io.StringIO()):
        a, b = [hdrgen.HDRPairGenerator(**args).flow_from_directory(str(tmp_path / kind), target_size=(24, 40),
                                                                     batch_size=2, seed=5) for kind in ("pfm", "exr")]
    assert a.sizes == b.sizes == sizes
    for _ in range(7):
        da, db = a.next_draws(), b.next_draws()
        assert len(da) == len(db) == 2 or len(da) == len(db) == 1
        for p, q in zip(da, db):
            assert p.keys() == q.keys()
            for key in p:
                assert repr(p[key]) == repr(q[key]), key
