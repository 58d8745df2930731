"""The antialiased resampler on the GPU (csrc/resize.hip, ops, resize, HDRPairGenerator, make_dataset,
predict) against the numpy restatement of Pillow (tests/resize_ref.py).  The contract is identity:
float results are compared as bits, uint8 results as bytes, never with a tolerance; where the
reference has a NaN only its position must match.

The horizontal pass has two paths, chosen on the host from (w, ow, ksize) and exposed as
cnnitmo_resize_tile_cols: the LDS path (a tile of that many output columns per workgroup, 64 rows) and,
for 0, the direct path.  The shapes below are picked on each side of that switch with the query itself
(test_both_horizontal_paths_are_reached asserts it): 16x300 -> 16x19 is direct for lanczos (97 taps) and
LDS for the other filters; every upscale is LDS.  BOUNDARY: w = 4 ow, whose bilinear tile is 16 columns:
ow = 16 is one full tile, ow = 17 a second tile of one column; its 65 rows are a second strip of one row.
"""
import contextlib
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cnn_itmo_amd as C  # noqa: E402
import resize_ref as R  # noqa: E402
from arena import Arena  # noqa: E402
from cnn_itmo_amd import hdrio, ops  # noqa: E402
from cnn_itmo_amd import resize as Z  # noqa: E402

# n x h x w -> oh x ow
CASES = ["1x1x1-5x3", "1x8x8-1x1", "2x17x23-64x100", "1x52x76-17x23", "1x33x47-33x20", "1x40x40-7x40",
         "1x16x300-16x19", "3x97x61-31x32", "1x9x11-9x11",
         "1x65x64-65x16", "1x65x68-65x17"]  # BOUNDARY: tile and tile + 1 output columns, 64 + 1 rows
DTYPES = ["f32", "u8"]
_X, _REF = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_itmo_amd import _lib as L
    return L.load()


def parse(case):
    a, b = case.split("-")
    return tuple(int(v) for v in a.split("x")), tuple(int(v) for v in b.split("x"))


def hdr_like(shape, seed=0):
    """float32 [n,h,w,3]: rand^8 * 1000, a patch of zeros and one 1e4 spike per image (where there is room)."""
    n, h, w = shape
    rng = np.random.default_rng(seed + 1000 * h + w)
    x = (rng.random((n, h, w, 3)) ** 8 * 1000).astype(np.float32)
    if h >= 7 and w >= 5:
        x[:, 1:1 + h // 3, 1:1 + w // 3] = 0
        x[:, h // 2, w // 2] = 1e4
    return x


def levels(shape, seed=0):
    """uint8 [n,h,w,3]: random, with a patch of 0 and one of 255 (where there is room)."""
    n, h, w = shape
    rng = np.random.default_rng(seed + 1000 * h + w + 7)
    u = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    if h >= 7 and w >= 5:
        u[:, 1:1 + h // 3, 1:1 + w // 3] = 0
        u[:, h - 1 - h // 3:h - 1, w - 1 - w // 3:w - 1] = 255
    return u


def _x(case, dt):
    if (case, dt) not in _X:
        _X[case, dt] = (hdr_like if dt == "f32" else levels)(parse(case)[0])
        _X[case, dt].setflags(write=False)
    return _X[case, dt]


def _ref(case, dt, filt):
    """The reference's result for a case, computed once and read only."""
    if (case, dt, filt) not in _REF:
        _REF[case, dt, filt] = R.resize(_x(case, dt), parse(case)[1], filt)
        _REF[case, dt, filt].setflags(write=False)
    return _REF[case, dt, filt]


def same(got, want):
    """Bits (float32) or bytes (uint8); a NaN of the reference must be a NaN, whatever its payload."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype == np.uint8:
        bad = got != want
    else:
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all(), "NaN positions differ"
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values differ, the first at {np.argwhere(bad)[0]}"


def tables(n_in, n_out, filt):
    """Device tables of one axis (None when the size stays), from the library's coefficients."""
    if n_in == n_out:
        return None
    b, k = Z.coefficients(n_in, n_out, filt)
    return torch.from_numpy(b).cuda(), torch.from_numpy(k).cuda()


def run_kernel(x, size, filt, lo=float("-inf")):
    xd = torch.from_numpy(np.array(x)).cuda()
    n, h, w, _ = x.shape
    out = torch.empty((n,) + tuple(size) + (3,), dtype=xd.dtype, device="cuda")
    ops.resize(xd, out, tables(w, size[1], filt), tables(h, size[0], filt), lo=lo)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------- the kernel equals the reference
@pytest.mark.parametrize("filt", R.FILTERS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_kernel_equals_reference(case, dt, filt):
    same(run_kernel(_x(case, dt), parse(case)[1], filt), _ref(case, dt, filt))


def test_both_horizontal_paths_are_reached(_lib):
    """The cases above take the direct path (tile 0), the LDS path with one tile, with several tiles,
    and the BOUNDARY pair sits on a tile edge."""
    tiles = {}
    for case in CASES:
        (_, _, w), (_, ow) = parse(case)
        for f in R.FILTERS:
            if w != ow:
                tiles[case, f] = ops.resize_tile_cols(w, ow, R.coeffs(w, ow, f)[0])
    assert tiles["1x16x300-16x19", "lanczos"] == 0  # direct
    assert all(tiles["1x16x300-16x19", f] > 0 for f in ("box", "bilinear", "bicubic"))
    assert all(tiles["2x17x23-64x100", f] > 0 for f in R.FILTERS)  # the upscale: LDS, two tiles
    assert all(0 < tiles["2x17x23-64x100", f] < 100 for f in R.FILTERS)
    assert tiles["1x65x64-65x16", "bilinear"] == 16 and tiles["1x65x68-65x17", "bilinear"] == 16


def test_nan_and_infinities():
    x = hdr_like((1, 33, 47), seed=3).copy()
    x[0, 4, 5, 0], x[0, 20, 30, 1], x[0, 28, 9, 2] = np.nan, np.inf, -np.inf
    for filt in ("bilinear", "lanczos"):
        want = R.resize(x, (12, 20), filt)
        assert np.isnan(want).any() and np.isinf(want).any()
        same(run_kernel(x, (12, 20), filt), want)


def test_floor():
    """lo = 0 on a lanczos case whose reference does go negative; a NaN stays a NaN."""
    case = "1x52x76-17x23"
    ref = _ref(case, "f32", "lanczos")
    assert (ref < 0).any()
    same(run_kernel(_x(case, "f32"), parse(case)[1], "lanczos", lo=0.0), np.where(ref < 0, np.float32(0), ref))
    x = _x(case, "f32").copy()
    x[0, 10, 10, 1] = np.nan
    want = R.resize(x, (52, 23), "lanczos")  # one pass: the floor is on the horizontal store
    assert (want < 0).any() and np.isnan(want).any()
    same(run_kernel(x, (52, 23), "lanczos", lo=0.0), np.where(want < 0, np.float32(0), want))
    same(run_kernel(x, (52, 76), "lanczos", lo=50.0), np.where(x < 50, np.float32(50), x))  # the copy


def test_repeatable():
    case = "3x97x61-31x32"
    for dt in DTYPES:
        a = run_kernel(_x(case, dt), parse(case)[1], "bicubic")
        b = run_kernel(_x(case, dt), parse(case)[1], "bicubic")
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- poisoned arena
def _carve(arena, numel, dtype, off, name, data=None):
    """`numel` elements `off` elements past a 16-byte boundary; only they are payload."""
    t = arena.take(numel + off, dtype, name=name, payload=False)
    es = t.element_size()
    start = arena.carves[-1][1]
    arena.payload[start + off * es:start + (off + numel) * es] = True
    v = t[off:]
    assert v.data_ptr() % 16 == (off * es) % 16
    if data is not None:
        v.copy_(torch.from_numpy(np.array(data)).reshape(-1))
    return v


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case,filt", [("2x17x23-64x100", "bicubic"), ("1x16x300-16x19", "lanczos"),
                                       ("1x52x76-17x23", "bilinear")])
def test_poisoned_arena(case, filt, dt):
    """x one and out three elements off a 16-byte boundary, out and the workspace poisoned first: out
    equals the reference under both poisons (so every element is written), x is unchanged, and no byte
    outside out and the workspace changes."""
    (n, h, w), (oh, ow) = parse(case)
    x, want = _x(case, dt), _ref(case, dt, filt)
    tdt = torch.float32 if dt == "f32" else torch.uint8
    for fill in ("nan", "zero"):
        arena = Arena(12 << 20, fill=fill, device="cuda")
        xd = _carve(arena, x.size, tdt, 1, "x", x)
        out = _carve(arena, want.size, tdt, 3, "out")
        nws = ops.resize_workspace_bytes(tdt, n, h, w, oh, ow)
        assert nws == (n * h * ow * 3 * xd.element_size() if (h != oh and w != ow) else 0)
        ws = arena.take(max(nws, 4), torch.uint8, name="workspace")
        tx, ty = tables(w, ow, filt), tables(h, oh, filt)
        ops.resize(xd.view(n, h, w, 3), out.view(n, oh, ow, 3), tx, ty, ws=ws)
        arena.check_untouched()
        same(out.view(n, oh, ow, 3).cpu().numpy(), want)
        assert xd.cpu().numpy().tobytes() == x.tobytes()


# ---------------------------------------------------------------- bad arguments
def test_bad_arguments(_lib):
    """Every bad argument is CNNITMO_EINVAL before any launch: out keeps its poison."""
    lib = _lib
    n, h, w, oh, ow = 1, 12, 20, 5, 7
    x = torch.zeros(n * h * w * 3 + 8, dtype=torch.float32, device="cuda")
    out = torch.full((n * oh * ow * 3 + 8,), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.zeros(n * h * ow * 3, dtype=torch.float32, device="cuda")
    (bx, kx), (by, ky) = tables(w, ow, "bilinear"), tables(h, oh, "bilinear")
    ksx, ksy = kx.shape[1], ky.shape[1]
    ninf = float("-inf")
    X, O, W_ = x.data_ptr(), out.data_ptr(), ws.data_ptr()
    BX, KX, BY, KY = bx.data_ptr(), kx.data_ptr(), by.data_ptr(), ky.data_ptr()
    good = [X, 0, n, h, w, O, oh, ow, BX, KX, ksx, BY, KY, ksy, ninf, W_, None]
    names = ["x", "dtype", "n", "h", "w", "out", "oh", "ow", "bounds_x", "kk_x", "ksize_x", "bounds_y", "kk_y",
             "ksize_y", "lo", "workspace", "stream"]
    bad = [("x", None), ("out", None), ("dtype", 2), ("dtype", -1), ("n", 0), ("h", 0), ("w", -1), ("oh", 0),
           ("ow", 0), ("bounds_x", None), ("kk_x", None), ("bounds_y", None), ("kk_y", None), ("workspace", None),
           ("ksize_x", ksx + 1), ("ksize_x", 0), ("ksize_y", ksy + 1), ("lo", float("nan")),
           ("x", X + 2), ("out", O + 1), ("out", X + 16), ("out", X - 16), ("workspace", O + 4), ("workspace", X)]
    for name, value in bad:
        args = list(good)
        args[names.index(name)] = value
        assert lib.cnnitmo_resize(*args) == -1, (name, value)
        assert lib.cnnitmo_last_error()
    u8 = list(good)
    u8[1], u8[14] = 1, 0.0  # a floor with uint8
    assert lib.cnnitmo_resize(*u8) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote to out"
    assert lib.cnnitmo_resize(*good) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:n * oh * ow * 3]).any()) and bool(torch.isnan(out[n * oh * ow * 3:]).all())
    assert lib.cnnitmo_resize_workspace_bytes(0, n, h, w, oh, ow) == n * h * ow * 12
    assert lib.cnnitmo_resize_workspace_bytes(1, n, h, w, oh, ow) == n * h * ow * 3
    assert lib.cnnitmo_resize_workspace_bytes(0, n, h, w, h, ow) == 0
    assert lib.cnnitmo_resize_workspace_bytes(0, n, h, w, oh, w) == 0
    assert lib.cnnitmo_resize_workspace_bytes(2, n, h, w, oh, ow) == 0
    assert lib.cnnitmo_resize_workspace_bytes(0, 0, h, w, oh, ow) == 0


# ---------------------------------------------------------------- front ends
def test_resize_front_end():
    xf, xu = _x("2x17x23-64x100", "f32"), _x("2x17x23-64x100", "u8")
    got = Z.resize(xf, (64, 100), "bicubic")  # numpy, 4-D, float32
    assert got.is_cuda and got.dtype == torch.float32
    same(got.cpu().numpy(), _ref("2x17x23-64x100", "f32", "bicubic"))
    got = Z.resize(xf[1].astype(np.float64), (64, 100), "bicubic")  # numpy, 3-D, float64 -> float32
    assert got.dtype == torch.float32 and tuple(got.shape) == (64, 100, 3)
    same(got.cpu().numpy(), _ref("2x17x23-64x100", "f32", "bicubic")[1])
    got = Z.resize(torch.from_numpy(xu.copy()).cuda(), (64, 100), "lanczos")  # tensor, 4-D, uint8
    assert got.is_cuda and got.dtype == torch.uint8
    same(got.cpu().numpy(), _ref("2x17x23-64x100", "u8", "lanczos"))
    got = Z.resize(torch.from_numpy(xu[0].copy()).cuda(), (64, 100))  # tensor, 3-D, the default filter
    same(got.cpu().numpy(), _ref("2x17x23-64x100", "u8", "bilinear")[0])
    ref = _ref("1x52x76-17x23", "f32", "lanczos")
    same(Z.resize(_x("1x52x76-17x23", "f32"), (17, 23), "lanczos", floor=0).cpu().numpy(),
         np.where(ref < 0, np.float32(0), ref))
    same(Z.resize(xu, (17, 23), "box").cpu().numpy(), xu)  # equal sizes: a copy
    with pytest.raises(ValueError):
        Z.resize(torch.zeros(4, 4, 3), (2, 2))  # a host tensor


def _pictures():
    rng = np.random.default_rng(11)
    pics = {}
    for name, (h, w) in (("a.hdr", (40, 64)), ("b.pfm", (33, 47)), ("c.pfm", (64, 64))):
        img = (rng.random((h, w, 3)) ** 6 * 50 + 0.01).astype(np.float32)
        img[h // 3, w // 2] = 3e3  # a highlight
        pics[name] = img
    return pics


@pytest.mark.parametrize("resample", ["bilinear", "lanczos"])
def test_pair_generator_max_side(tmp_path, resample):
    """max_side = 32 over a 40x64 .hdr, a 33x47 .pfm and a 64x64 .pfm equals, bit for bit, a generator
    without max_side over .pfm files of the reference-resized pictures (lanczos: floored at 0)."""
    src, small = tmp_path / "src", tmp_path / "small"
    os.makedirs(src), os.makedirs(small)
    sizes = []
    for name, img in _pictures().items():
        hdrio.write_image(str(src / name), img)
        img = hdrio.read_image(str(src / name)).cpu().numpy()  # what the file holds (RGBE rounds)
        size = Z.fit_within(img.shape[0], img.shape[1], 32)
        ref = R.resize(img, size, resample)
        if resample == "lanczos":
            ref = np.where(ref < 0, np.float32(0), ref)
        hdrio.write_pfm(str(small / (name[:-4] + ".pfm")), ref)
        sizes.append(size)
    assert sizes == [(20, 32), (22, 32), (32, 32)]
    gen = C.HDRPairGenerator(rotation_range=20, zoom_range=0.2, horizontal_flip=True)
    with contextlib.redirect_stdout(io.StringIO()):
        a = gen.flow_from_directory(str(src), (16, 16), batch_size=3, seed=4, max_side=32, resample=resample)
        b = gen.flow_from_directory(str(small), (16, 16), batch_size=3, seed=4)
    assert a.sizes == sizes == b.sizes
    for _ in range(2):
        (xa, ya), (xb, yb) = next(a), next(b)
        same(xa.cpu().numpy(), xb.cpu().numpy())
        same(ya.cpu().numpy(), yb.cpu().numpy())
        assert np.isfinite(ya.cpu().numpy()).all()


def test_pair_generator_without_max_side_is_unchanged(tmp_path):
    """max_side=None, and a max_side no picture exceeds: the pairs of a generator built without it."""
    for name, img in _pictures().items():
        hdrio.write_image(str(tmp_path / name), img)
    gen = C.HDRPairGenerator(rotation_range=20, zoom_range=0.2, horizontal_flip=True)
    with contextlib.redirect_stdout(io.StringIO()):
        its = [gen.flow_from_directory(str(tmp_path), (16, 16), batch_size=3, seed=4, **kw)
               for kw in ({}, {"max_side": None}, {"max_side": 64, "resample": "lanczos"})]
    (x0, y0), (x1, y1), (x2, y2) = (next(it) for it in its)
    assert its[2]._sources[0].dtype == torch.uint8  # still in file format: nothing was resized
    for x, y in ((x1, y1), (x2, y2)):
        same(x.cpu().numpy(), x0.cpu().numpy())
        same(y.cpu().numpy(), y0.cpu().numpy())


def test_make_dataset_max_side(tmp_path):
    from PIL import Image
    from cnn_itmo_amd import make_dataset as MD, tonemap
    img = _pictures()["a.hdr"]
    os.makedirs(tmp_path / "hdr")
    hdrio.write_pfm(str(tmp_path / "hdr" / "a.pfm"), img)
    out = str(tmp_path / "data")
    assert MD.main(["--hdr-dir", str(tmp_path / "hdr"), "--out", out, "--max-side", "32", "--resample",
                    "bicubic"]) == 0
    ref = R.resize(img, (20, 32), "bicubic")
    ref = np.where(ref < 0, np.float32(0), ref)
    v, cn, cy = tonemap.virtual_camera_params(1, np.random.default_rng(0))
    want_t = tonemap.reinhard(ref, out_u8=True)[0].cpu().numpy()
    want_i = tonemap.virtual_camera(ref, v[0], cn[0], cy[0], out_u8=True)[0].cpu().numpy()
    got_t = np.asarray(Image.open(os.path.join(out, "output1", "0", "a_0.png")))
    got_i = np.asarray(Image.open(os.path.join(out, "input1", "0", "a_0.png")))
    assert got_t.shape == (20, 32, 3)
    same(got_t, want_t)
    same(got_i, want_i)


def test_predict_max_side(tmp_path):
    """A 48x80 PNG with --max-side 32 gives a 19x32 output (fit_within), equal to a run given the
    PIL-resized PNG."""
    from PIL import Image
    from cnn_itmo_amd import predict as PR
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(32, 32, 3), seed=5, verbose=False)
    ck = str(tmp_path / "model.hdf5")
    m.save(ck)
    u8 = levels((1, 48, 80), seed=2)[0]
    assert Z.fit_within(48, 80, 32) == (19, 32)
    for d in ("big", "small"):
        os.makedirs(tmp_path / d)
    Image.fromarray(u8).save(str(tmp_path / "big" / "f.png"))
    Image.fromarray(u8).resize((32, 19), Image.BILINEAR).save(str(tmp_path / "small" / "f.png"))
    with contextlib.redirect_stdout(io.StringIO()):
        assert PR.main(["--model", ck, "--input", str(tmp_path / "big"), "--output", str(tmp_path / "o1"),
                        "--max-side", "32", "--hdr", str(tmp_path / "h1")]) == 0
        assert PR.main(["--model", ck, "--input", str(tmp_path / "small"), "--output", str(tmp_path / "o2"),
                        "--hdr", str(tmp_path / "h2")]) == 0
    a = np.asarray(Image.open(str(tmp_path / "o1" / "f.png")))
    b = np.asarray(Image.open(str(tmp_path / "o2" / "f.png")))
    assert a.shape == (19, 32, 3)
    same(a, b)
    ha, hb = hdrio.read_image(str(tmp_path / "h1" / "f.hdr")), hdrio.read_image(str(tmp_path / "h2" / "f.hdr"))
    assert tuple(ha.shape) == (19, 32, 3)
    same(ha.cpu().numpy(), hb.cpu().numpy())
