"""cnnitmo_exr_unpack / cnnitmo_exr_pack (csrc/exr.hip) and the .exr front ends against
tests/exr_ref.py.  Every conversion is exact or a single rounding to nearest even, and the
predictor is integer arithmetic, so every comparison is on bits or bytes, with no tolerance."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import _lib as L  # noqa: E402
from cnn_itmo_amd import exr, hdrio, ops  # noqa: E402
import exr_ref as ER  # noqa: E402
from arena import Arena, poison_count  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1
COMPRESSIONS = [exr.NONE, exr.ZIPS, exr.ZIP]
SIZES = [(1, 1), (3, 5), (17, 23)]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def picture(h, w, seed=0, smooth=False):
    if smooth:  # deflates in every chunk
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([x + y, x * 0.5 + 1, y + 2.0], -1).astype(np.float32)
    rng = np.random.default_rng(seed)
    return (np.exp(rng.uniform(-8, 8, (h, w, 3))) * rng.choice([1, 1, 1, -1], (h, w, 3))).astype(np.float32)


def rgb_channels(img, dtype):
    with np.errstate(over="ignore"):
        return {"R": img[..., 0].astype(dtype), "G": img[..., 1].astype(dtype), "B": img[..., 2].astype(dtype)}


def unpack(parsed, coded="own", raw_off=0, rgb_off=0):
    """ops.exr_unpack of a parsed file -> uint32 bits [h,w,3].  raw_off / rgb_off: bytes / elements by
    which raw and rgb sit off a 16-byte boundary; what lies around rgb must stay as it was."""
    lay = parsed.layout
    h, w = lay["h"], lay["w"]
    c = lay["coded"] if isinstance(coded, str) else coded
    src = torch.zeros(parsed.raw.size + raw_off, dtype=torch.uint8, device="cuda")
    src[raw_off:] = torch.from_numpy(parsed.raw)
    dst = torch.full((h * w * 3 + rgb_off + 4,), -7.0, dtype=torch.float32, device="cuda")
    out = dst[rgb_off:rgb_off + h * w * 3].view(h, w, 3)
    assert src[raw_off:].data_ptr() % 16 == raw_off % 16 and out.data_ptr() % 16 == 4 * rgb_off % 16
    ops.exr_unpack(src[raw_off:], None if c is None else torch.from_numpy(c).cuda(), lay["lines_per_chunk"],
                   lay["line_bytes"], lay["ch_off"], lay["ch_type"], out)
    got = dst.cpu().numpy()
    assert (got[:rgb_off] == -7).all() and (got[rgb_off + h * w * 3:] == -7).all()
    return got[rgb_off:rgb_off + h * w * 3].view(np.uint32).reshape(h, w, 3)


def pack(img, ptype, lines, coded, rgb_off=0, out_off=0):
    img = np.ascontiguousarray(img, np.float32)
    h, w = img.shape[:2]
    n = h * 3 * w * (2 if ptype == exr.HALF else 4)
    src = torch.zeros(h * w * 3 + rgb_off, dtype=torch.float32, device="cuda")
    src[rgb_off:] = torch.from_numpy(img.reshape(-1))
    dst = torch.full((n + out_off + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    ops.exr_pack(src[rgb_off:].view(h, w, 3), ptype, lines, coded, dst[out_off:out_off + n])
    got = dst.cpu().numpy()
    assert (got[:out_off] == 0xA5).all() and (got[out_off + n:] == 0xA5).all()
    return got[out_off:out_off + n]


# ------------------------------------------------------------------------------ unpack
def test_unpack_every_half_pattern():
    y = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(256, 256)
    chans = {"R": y, "G": y.T.copy(), "B": y[::-1].copy()}
    want = bits(ER.rgb(chans))
    assert np.isnan(ER.rgb(chans)).sum() == 3 * 2046
    for comp in COMPRESSIONS:
        data, _ = ER.build(chans, compression=comp)
        assert np.array_equal(unpack(exr.parse_exr(data)), want)


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.uint32])
@pytest.mark.parametrize("comp", COMPRESSIONS)
@pytest.mark.parametrize("hw", SIZES)
def test_unpack_small_shapes(hw, comp, dtype):
    for smooth in (False, True):
        img = picture(*hw, seed=hw[1], smooth=smooth)
        chans = rgb_channels(np.abs(img) * 1000 if dtype == np.uint32 else img, dtype)
        data, _ = ER.build(chans, compression=comp)
        assert np.array_equal(unpack(exr.parse_exr(data)), bits(ER.rgb(chans)))


@pytest.mark.parametrize("comp", COMPRESSIONS)
def test_unpack_mixed_types_skipped_channels_and_lone_y(comp):
    h, w = 17, 23
    rng = np.random.default_rng(3)
    img = picture(h, w, 3, smooth=True)
    chans = {"B": img[..., 2].astype(np.float16), "G": img[..., 1].copy(),
             "R": rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32),
             "A": np.ones((h, w), np.float16), "Z": rng.random((h, w)).astype(np.float32),
             "diffuse.R": rng.random((h, w)).astype(np.float16)}
    data, _ = ER.build(chans, compression=comp, origin=(-3, 7), line_order=1)
    assert np.array_equal(unpack(exr.parse_exr(data)), bits(ER.rgb(chans)))
    # uint -> float rounds to nearest even: the values around 2^24 and 2^32 by hand
    u = np.array([[2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 32 - 1, 2 ** 32 - 129, 2 ** 32 - 128, 0]],
                 np.uint32)
    data, _ = ER.build({"Y": u}, compression=comp)
    got = unpack(exr.parse_exr(data)).view(np.float32)
    assert got[0, :, 0].tolist() == [2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 25, 2.0 ** 25 + 8, 2.0 ** 32, 2.0 ** 32 - 256,
                                     2.0 ** 32, 0.0]
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    y = img[..., 0].astype(np.float16)
    data, _ = ER.build({"Y": y, "A": y}, compression=comp)
    assert np.array_equal(unpack(exr.parse_exr(data)), bits(ER.rgb({"Y": y})))


def test_unpack_on_the_segment_edges():
    """ZIP chunks of SEG - 2, SEG, SEG + 2 and 3 SEG + 2 bytes: a full chunk is 16 lines, so these are
    the short last chunk (one line of a half channel) behind a full one of 16 times the size; and
    full chunks of SEG - 32, SEG, SEG + 32 and 3 SEG + 32 bytes with a short chunk of five lines."""
    seg = ops.exr_segment_bytes()
    assert seg >= 64 and seg % 32 == 0
    for nbytes in (seg - 2, seg, seg + 2, 3 * seg + 2):
        w = nbytes // 2
        y = (np.arange(17 * w, dtype=np.float32).reshape(17, w) % 2048).astype(np.float16)
        data, coded = ER.build({"Y": y}, compression=exr.ZIP)
        p = exr.parse_exr(data)
        assert coded.tolist() == [1, 1] and p.layout["line_bytes"] == nbytes
        assert np.array_equal(unpack(p), bits(ER.rgb({"Y": y})))
    for nbytes in (seg - 32, seg, seg + 32, 3 * seg + 32):
        w = nbytes // 32
        y = (np.arange(21 * w, dtype=np.float32).reshape(21, w) % 2048).astype(np.float16)
        data, coded = ER.build({"Y": y}, compression=exr.ZIP)
        p = exr.parse_exr(data)
        assert coded.tolist() == [1, 1] and 16 * p.layout["line_bytes"] == nbytes
        assert np.array_equal(unpack(p), bits(ER.rgb({"Y": y})))


def test_unpack_mixed_and_null_coded():
    h, w = 48, 40
    img = picture(h, w, smooth=True)
    img[16:32] = picture(16, w, seed=1) * 1.2345  # noise: stored raw
    chans = rgb_channels(img, np.float32)
    data, coded = ER.build(chans, compression=exr.ZIP)
    assert coded.tolist() == [1, 0, 1]
    p = exr.parse_exr(data)
    want = bits(img)
    assert np.array_equal(unpack(p), want)
    # wrong flags: wrong pixels in those chunks only, and nothing outside rgb (checked in unpack)
    got = unpack(p, coded=np.array([1, 1, 1], np.uint8))
    assert np.array_equal(got[:16], want[:16]) and np.array_equal(got[32:], want[32:])
    assert not np.array_equal(got[16:32], want[16:32])
    unpack(p, coded=np.array([0, 255, 0], np.uint8))
    data, coded = ER.build(chans, compression=exr.NONE)
    p = exr.parse_exr(data)
    assert np.array_equal(unpack(p, coded=None), want) and np.array_equal(unpack(p, coded=np.zeros(h, np.uint8)), want)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_alignment_does_not_change_the_bits(dtype):
    img = picture(33, 1030, seed=4, smooth=True)  # two tiles a line, three segments a ZIP chunk
    chans = rgb_channels(img, dtype)
    for comp in COMPRESSIONS:
        p = exr.parse_exr(ER.build(chans, compression=comp)[0])
        want = bits(ER.rgb(chans))
        for raw_off, rgb_off in ((0, 0), (1, 1), (3, 3), (2, 0), (0, 2)):
            assert np.array_equal(unpack(p, raw_off=raw_off, rgb_off=rgb_off), want), (comp, raw_off, rgb_off)
    ptype = exr.HALF if dtype == np.float16 else exr.FLOAT
    for lines in (1, 16):
        for coded in (0, 1):
            want = ER.payload(img, ptype, lines, coded)
            for rgb_off, out_off in ((0, 0), (1, 1), (3, 3)):
                assert np.array_equal(pack(img, ptype, lines, coded, rgb_off, out_off), want)


# ------------------------------------------------------------------------------ pack
def half_rounding_cases():
    """For every finite half a and its successor b: the fp32 midpoint and its two fp32 neighbours;
    +-0, fp32 denormals, +-65504, +-65520 and their neighbours, +-inf."""
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)  # 0 .. 65504, increasing
    mid = ((h[:-1] + h[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (h[:-1] + h[1:]) / 2)  # exact in fp32
    up, inf = np.float32(np.inf), np.float32(np.inf)
    special = np.array([0.0, 65504.0, 65520.0, np.inf, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 2.0 ** -126], np.float32)
    denormals = np.array([1, 2, 0x3FFFFF, 0x400000, 0x7FFFFF], np.uint32).view(np.float32)
    x = np.concatenate([mid, np.nextafter(mid, up), np.nextafter(mid, -inf), h.astype(np.float32), special,
                        np.nextafter(special[:3], up), np.nextafter(special[1:], -inf), denormals])
    return np.concatenate([x, -x])


def test_pack_half_rounding():
    x = half_rounding_cases()
    w = 3 * 251
    x = np.concatenate([x, np.zeros(-x.size % w, np.float32)])
    img = x.reshape(-1, w // 3, 3)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    got = pack(img, exr.HALF, 1, 0).view(np.float16).reshape(img.shape[0], 3, -1)  # lines of B, G, R planes
    got = np.stack([got[:, 2], got[:, 1], got[:, 0]], -1).reshape(-1)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert (want.view(np.uint16) == 0x7C00).sum() > 2 and (want.view(np.uint16) == 0x8000).sum() > 2
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0x7F802000], np.uint32).view(np.float32)
    got = pack(nan.reshape(1, 2, 3), exr.HALF, 1, 0).view(np.float16)
    assert np.isnan(got).all()


@pytest.mark.parametrize("ptype", [exr.HALF, exr.FLOAT])
@pytest.mark.parametrize("hw", SIZES + [(33, 700)])
def test_pack_payload_and_round_trip(hw, ptype):
    img = picture(*hw, seed=hw[0])
    img.reshape(-1)[::7] *= 1e4  # some overflow half
    size = 2 if ptype == exr.HALF else 4
    lay = {"h": hw[0], "w": hw[1], "line_bytes": 3 * hw[1] * size, "ch_off": (2 * hw[1] * size, hw[1] * size, 0),
           "ch_type": (ptype,) * 3}
    with np.errstate(over="ignore"):
        back = bits(img if ptype == exr.FLOAT else img.astype(np.float16).astype(np.float32))
    for lines in (1, 16):
        nchunks = -(-hw[0] // lines)
        for coded in (0, 1):
            got = pack(img, ptype, lines, coded)
            assert np.array_equal(got, ER.payload(img, ptype, lines, coded))
            p = exr.Parsed({}, dict(lay, lines_per_chunk=lines, nchunks=nchunks,
                                    coded=np.full(nchunks, coded, np.uint8)), got)
            assert np.array_equal(unpack(p), back)


# ------------------------------------------------------------------------------ arena, determinism, arguments
def test_arena_and_two_runs_equal():
    h, w = 37, 1100
    img = picture(h, w, seed=5, smooth=True)
    chans = rgb_channels(img, np.float16)
    p = exr.parse_exr(ER.build(chans, compression=exr.ZIP)[0])
    lay = p.layout
    assert lay["coded"].all()
    ar = Arena(16 << 20, fill="nan", device="cuda")
    raw = ar.take(p.raw.size, torch.uint8, data=p.raw, name="raw")
    coded = ar.take(lay["nchunks"], torch.uint8, data=lay["coded"], name="coded")
    ws = ar.take(ops.exr_workspace_bytes(h, 16, lay["line_bytes"]), torch.uint8, name="workspace")
    rgb = ar.take(h * w * 3, torch.float32, name="rgb").view(h, w, 3)
    out = ar.take(h * w * 6, torch.uint8, name="out")
    ops.exr_unpack(raw, coded, 16, lay["line_bytes"], lay["ch_off"], lay["ch_type"], rgb, ws=ws)
    want = bits(ER.rgb(chans))
    first = rgb.cpu().numpy().view(np.uint32)
    assert np.array_equal(first, want) and poison_count(rgb) == 0
    ops.exr_pack(rgb, exr.HALF, 16, 1, out)
    packed = out.cpu().numpy()
    assert np.array_equal(packed, ER.payload(ER.rgb(chans), exr.HALF, 16, 1))
    ar.check_untouched()
    ws.fill_(0)  # another workspace content, a second run: the same bits
    ops.exr_unpack(raw, coded, 16, lay["line_bytes"], lay["ch_off"], lay["ch_type"], rgb, ws=ws)
    ops.exr_pack(rgb, exr.HALF, 16, 1, out)
    assert np.array_equal(rgb.cpu().numpy().view(np.uint32), first) and np.array_equal(out.cpu().numpy(), packed)
    ar.check_untouched()


def test_bad_arguments_are_einval_and_touch_nothing():
    lib = L.load()
    h, w, lb = 4, 6, 36
    raw = torch.zeros(h * lb, dtype=torch.uint8, device="cuda")
    coded = torch.ones(h, dtype=torch.uint8, device="cuda")
    rgb = torch.full((h, w, 3), -7.0, device="cuda")
    out = torch.full((h * lb,), 0xA5, dtype=torch.uint8, device="cuda")
    need = ops.exr_workspace_bytes(h, 1, lb)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    assert need > 0 and ops.exr_workspace_bytes(h, 2, lb) == 0 and ops.exr_workspace_bytes(0, 1, lb) == 0
    assert ops.exr_workspace_bytes(h, 1, lb + 1) == 0

    def triple(v):
        return (ctypes.c_int * 3)(*v)

    def unpack_rc(raw=raw.data_ptr(), coded=coded.data_ptr(), h=h, w=w, lines=1, lb=lb, off=(24, 12, 0),
                  typ=(1, 1, 1), rgb=rgb.data_ptr(), ws=ws.data_ptr(), ws_bytes=need):
        return lib.cnnitmo_exr_unpack(raw, coded, h, w, lines, lb, None if off is None else triple(off),
                                      None if typ is None else triple(typ), rgb, ws, ws_bytes, None)

    assert unpack_rc() == 0
    torch.cuda.synchronize()
    rgb.fill_(-7.0)
    bad = [dict(raw=None), dict(rgb=None), dict(off=None), dict(typ=None), dict(ws=None), dict(h=0), dict(w=0),
           dict(h=-1), dict(w=-1), dict(lines=2), dict(lines=0), dict(lines=32), dict(off=(26, 12, 0)),
           dict(off=(24, 12, 0), typ=(2, 1, 1)), dict(off=(24, 13, 0)), dict(off=(24, 12, -2)), dict(typ=(1, 3, 1)),
           dict(typ=(-1, 1, 1)), dict(ws_bytes=need - 1), dict(lb=35), dict(lb=0), dict(rgb=rgb.data_ptr() + 2)]
    for kw in bad:
        assert unpack_rc(**kw) == EINVAL, kw
        assert lib.cnnitmo_last_error()
    assert unpack_rc(coded=None, ws=None, ws_bytes=0) == 0  # no workspace needed without coded chunks
    torch.cuda.synchronize()
    rgb.fill_(-7.0)

    def pack_rc(rgb=rgb.data_ptr(), h=h, w=w, ptype=1, lines=1, coded=1, out=out.data_ptr()):
        return lib.cnnitmo_exr_pack(rgb, h, w, ptype, lines, coded, out, None)

    for kw in (dict(rgb=None), dict(out=None), dict(h=0), dict(w=0), dict(ptype=0), dict(ptype=3), dict(lines=2),
               dict(coded=2), dict(coded=-1), dict(rgb=rgb.data_ptr() + 1)):
        assert pack_rc(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (rgb == -7).all() and (out == 0xA5).all()
    assert pack_rc() == 0
    with pytest.raises(L.CnnItmoError, match="runs past line_bytes"):
        ops.exr_unpack(raw, None, 1, lb, (26, 12, 0), (1, 1, 1), rgb)


# ------------------------------------------------------------------------------ front ends
@pytest.mark.parametrize("compression", ["zip", "zips", "none"])
@pytest.mark.parametrize("pixel_type", ["half", "float"])
def test_read_write_round_trip(tmp_path, pixel_type, compression):
    img = picture(40, 64, seed=2)
    img[16:32] = picture(16, 64, smooth=True)  # chunks that deflate next to chunks that may not
    path = str(tmp_path / "a.exr")
    exr.write_exr(path, img, pixel_type=pixel_type, compression=compression)
    header, chans, _, coded = ER.take_apart(open(path, "rb").read())
    dt = np.float16 if pixel_type == "half" else np.float32
    with np.errstate(over="ignore"):
        want = img.astype(dt)
    for k, name in enumerate("RGB"):
        assert chans[name].dtype == dt
        assert np.array_equal(chans[name].view(np.uint8), want[..., k].copy().view(np.uint8))
    assert header["compression"] == exr.COMPRESSION_NAMES[compression]
    # the file the reference builds from the same values
    assert open(path, "rb").read() == ER.build(chans, compression=header["compression"])[0]
    got, hd = exr.read_exr(path, return_header=True)
    assert hd == header and got.is_cuda and got.dtype == torch.float32
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.astype(np.float32)))
    assert np.array_equal(bits(hdrio.load_image(path).cpu().numpy()), bits(want.astype(np.float32)))
    hdrio.save_image(str(tmp_path / "b.exr"), torch.from_numpy(img).cuda(), pixel_type=pixel_type,
                     compression=compression)
    assert open(str(tmp_path / "b.exr"), "rb").read() == open(path, "rb").read()
    with pytest.raises(ValueError, match="pixel type"):
        exr.write_exr(path, img, pixel_type="uint")
    with pytest.raises(ValueError, match="compression"):
        exr.write_exr(path, img, compression="piz")


def test_generator_over_exr_equals_pfm(tmp_path):
    from cnn_itmo_amd import hdrgen as G
    img = picture(40, 64, seed=8).astype(np.float16).astype(np.float32)
    batches = {}
    for kind in ("pfm", "exr", "exr_half"):
        d = tmp_path / kind
        os.makedirs(str(d))
        if kind == "pfm":
            hdrio.write_pfm(str(d / "a.pfm"), img)
        elif kind == "exr":
            open(str(d / "a.exr"), "wb").write(ER.build(rgb_channels(img, np.float32), compression=exr.ZIP)[0])
        else:
            exr.write_exr(str(d / "a.exr"), img)
        gen = G.HDRPairGenerator(rotation_range=90, horizontal_flip=True, zoom_range=0.2)
        with contextlib.redirect_stdout(io.StringIO()):
            it = gen.flow_from_directory(str(d), target_size=(24, 40), batch_size=3, seed=4)
        x, y = next(it)
        batches[kind] = (x.cpu().numpy(), y.cpu().numpy())
    for kind in ("exr", "exr_half"):
        for a, b in zip(batches[kind], batches["pfm"]):
            assert np.array_equal(bits(a), bits(b))


def test_make_dataset_over_exr(tmp_path):
    from PIL import Image
    from cnn_itmo_amd import make_dataset as MD
    outs = {}
    for kind in ("pfm", "exr"):
        src = tmp_path / kind
        os.makedirs(str(src))
        for i, name in enumerate(("b_scene", "a_scene")):
            img = np.abs(picture(40, 56, seed=20 + i)).astype(np.float16).astype(np.float32)
            if kind == "pfm":
                hdrio.write_pfm(str(src / f"{name}.pfm"), img)
            else:
                exr.write_exr(str(src / f"{name}.exr"), img, compression=("zip", "zips")[i])
        out = tmp_path / f"train_{kind}"
        with contextlib.redirect_stdout(io.StringIO()):
            assert MD.main(["--hdr-dir", str(src), "--out", str(out), "--cameras", "2", "--seed", "3"]) == 0
        names = sorted(os.listdir(str(out / "input1" / "0")))
        assert names == ["a_scene_0.png", "a_scene_1.png", "b_scene_0.png", "b_scene_1.png"]
        outs[kind] = [np.array(Image.open(str(out / sub / "0" / n))) for sub in ("input1", "output1") for n in names]
        outs[kind].append(open(str(out / "params.csv")).read())
    assert outs["exr"][-1] == outs["pfm"][-1]
    for a, b in zip(outs["exr"][:-1], outs["pfm"][:-1]):
        assert np.array_equal(a, b)


def test_evaluate_hdr_pairs_exr_with_hdr(tmp_path):
    from cnn_itmo_amd import evaluate_hdr as EH
    pred, ref = tmp_path / "pred", tmp_path / "ref"
    os.makedirs(str(pred))
    os.makedirs(str(ref))
    r = np.abs(picture(24, 37, seed=1)) + 0.01
    p = (r * 1.1).astype(np.float32)
    exr.write_exr(str(pred / "a.exr"), p, pixel_type="float")
    hdrio.write_hdr(str(ref / "a.hdr"), r)
    hdrio.write_pfm(str(pred / "b.pfm"), p)
    exr.write_exr(str(ref / "b.exr"), r, pixel_type="float")
    hdrio.write_pfm(str(tmp_path / "a.pfm"), p)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rows = EH.evaluate_dir(str(pred), str(ref))
    assert [row[0] for row in rows] == ["a.exr", "b.pfm"]
    assert rows[0][1:] == EH.score_files(str(tmp_path / "a.pfm"), str(ref / "a.hdr"))  # as the same pixels from a .pfm
    assert "mean of 2 scored HDR files" in buf.getvalue()


def test_predict_hdr_format_exr(tmp_path):
    from PIL import Image
    from cnn_itmo_amd import predict as PR
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(32, 32, 3), seed=5, verbose=False)
    rng = np.random.default_rng(2)
    m.set_named_weights({k: rng.uniform(0.5, 1.5, v.shape) for k, v in m.named_weights().items()
                         if k.endswith("/moving_variance")})
    ck = str(tmp_path / "tiny.hdf5")
    m.save(ck)
    os.makedirs(str(tmp_path / "in"))
    for name in ("first", "second"):
        Image.fromarray(rng.integers(0, 256, (32, 48, 3), dtype=np.uint8)).save(str(tmp_path / "in" / f"{name}.png"))
    refs = tmp_path / "refs"
    os.makedirs(str(refs))
    exr.write_exr(str(refs / "first.exr"), np.abs(picture(32, 48, seed=3)) + 0.5, pixel_type="float")
    exr.write_exr(str(refs / "second.exr"), np.abs(picture(32, 48, seed=4)) + 0.5)
    flags = ["--hdr-mode", "exact", "--hdr-log-average", "reference", "--hdr-reference", str(refs)]
    for fmt in ("pfm", "exr"):
        with contextlib.redirect_stdout(io.StringIO()):
            assert PR.main(["--model", ck, "--input", str(tmp_path / "in"), "--output", str(tmp_path / f"out_{fmt}"),
                            "--hdr", str(tmp_path / f"hdr_{fmt}"), "--hdr-format", fmt] + flags) == 0
    assert sorted(os.listdir(str(tmp_path / "hdr_exr"))) == ["first.exr", "second.exr"]
    for name in ("first", "second"):
        want = hdrio.read_pfm(str(tmp_path / "hdr_pfm" / f"{name}.pfm"))
        header, chans, _, _ = ER.take_apart(open(str(tmp_path / "hdr_exr" / f"{name}.exr"), "rb").read())
        assert header["compression"] == exr.ZIP and all(chans[k].dtype == np.float16 for k in "RGB")
        with np.errstate(over="ignore"):
            assert np.array_equal(bits(ER.rgb(chans)), bits(want.astype(np.float16).astype(np.float32)))
        assert open(str(tmp_path / "out_exr" / f"{name}.png"), "rb").read() == \
            open(str(tmp_path / "out_pfm" / f"{name}.png"), "rb").read()
