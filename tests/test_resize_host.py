"""CPU checks of the antialiased resampler: the numpy restatement (tests/resize_ref.py) against
PIL.Image.resize itself, the library's host coefficients (cnnitmo_resize_coeffs) against the
restatement, fit_within, the front end's argument errors and HDRPairGenerator's draw stream with
max_side.  No pixels are produced on a GPU here."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest

import resize_ref as R

# h x w -> oh x ow: down, up, one axis untouched (either), to one pixel, from one pixel, odd sizes, a
# 15.8x reduction (97 lanczos taps)
SHAPES = [(52, 76, 17, 23), (51, 75, 64, 100), (33, 47, 33, 20), (40, 40, 7, 40), (8, 8, 1, 1), (1, 1, 5, 3),
          (97, 61, 31, 32), (16, 300, 16, 19)]
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from cnn_itmo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def pil_filter(name):
    from PIL import Image
    return {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]


def u8_inputs(h, w):
    rng = np.random.default_rng(100 * h + w)
    u = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if h >= 7 and w >= 5:
        u[1:1 + h // 3, 1:1 + w // 3] = 0
        u[h - 1 - h // 3:h - 1, w - 1 - w // 3:w - 1] = 255
    return {"random": u, "zeros": np.zeros((h, w, 3), np.uint8), "full": np.full((h, w, 3), 255, np.uint8)}


def f32_inputs(h, w):
    rng = np.random.default_rng(100 * h + w + 1)
    spike = np.full((h, w, 3), 1e-2, np.float32)
    spike[h // 2, w // 2] = 1e4
    return {"hdr": (rng.random((h, w, 3)) ** 8 * 1000).astype(np.float32), "spike": spike}


def ulp_distance(a, b):
    """Distance in float32 steps between finite values of equal sign or zero."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


# ---------------------------------------------------------------- the reference against PIL
@pytest.mark.parametrize("filt", R.FILTERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_reference_equals_pil_uint8(shape, filt):
    from PIL import Image
    h, w, oh, ow = shape
    for name, u in u8_inputs(h, w).items():
        want = np.asarray(Image.fromarray(u).resize((ow, oh), pil_filter(filt)))
        got = R.resize(u, (oh, ow), filt)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, int((got != want).sum()))


@pytest.mark.parametrize("filt", R.FILTERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_reference_equals_pil_float32(shape, filt):
    """Mode F, channel by channel.  The 1-ulp bound stands beside the identity, so that a Pillow build
    that rounds a tap differently is told apart from a wrong reference."""
    from PIL import Image
    h, w, oh, ow = shape
    for name, x in f32_inputs(h, w).items():
        want = np.stack([np.asarray(Image.fromarray(x[..., c]).resize((ow, oh), pil_filter(filt)))
                         for c in range(3)], -1)
        got = R.resize(x, (oh, ow), filt)
        assert got.dtype == np.float32 and want.dtype == np.float32
        assert ulp_distance(got, want).max() <= 1, (name, int(ulp_distance(got, want).max()))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            (name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


# ---------------------------------------------------------------- the library's coefficients
def axes():
    """(in, out) of every axis of SHAPES, both directions, and in == out."""
    s = set()
    for h, w, oh, ow in SHAPES:
        s |= {(h, oh), (oh, h), (w, ow), (ow, w), (h, h), (w, w)}
    return sorted(s)


@pytest.mark.parametrize("filt", R.FILTERS)
def test_library_coefficients_equal_reference(lib, filt):
    fid = R.FILTER_IDS[filt]
    for n_in, n_out in axes():
        ksize, bounds, kk = R.coeffs(n_in, n_out, filt)
        assert lib.cnnitmo_resize_coeffs(n_in, n_out, fid, None, None) == ksize
        b = np.full((n_out, 2), -7, np.int32)
        k = np.full((n_out, ksize), np.nan, np.float64)
        assert lib.cnnitmo_resize_coeffs(n_in, n_out, fid, b.ctypes.data, k.ctypes.data) == ksize
        assert np.array_equal(b, bounds), (n_in, n_out)
        assert np.array_equal(k.view(np.uint64), kk.view(np.uint64)), (n_in, n_out)
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= ksize).all()


def test_front_end_coefficients(lib):
    from cnn_itmo_amd import resize as Z
    ksize, bounds, kk = R.coeffs(300, 19, "lanczos")
    b, k = Z.coefficients(300, 19, "lanczos")
    assert ksize == 97 and b.dtype == np.int32 and k.dtype == np.float64
    assert np.array_equal(b, bounds) and np.array_equal(k.view(np.uint64), kk.view(np.uint64))
    assert np.array_equal(Z.coefficients(8, 3)[1].view(np.uint64), R.coeffs(8, 3, "bilinear")[2].view(np.uint64))
    for bad in [(0, 3, "box"), (3, -1, "box"), (3, 3, "hamming"), (3.5, 3, "box"), (3, True, "box")]:
        with pytest.raises(ValueError):
            Z.coefficients(*bad)


def test_library_coefficients_einval(lib):
    b = np.zeros((4, 2), np.int32)
    k = np.zeros((4, 9), np.float64)
    for n_in, n_out, fid in [(0, 4, 1), (-3, 4, 1), (8, 0, 1), (8, -1, 1), (8, 4, -1), (8, 4, 4), (8, 4, 99)]:
        assert lib.cnnitmo_resize_coeffs(n_in, n_out, fid, None, None) == EINVAL
        assert lib.cnnitmo_resize_coeffs(n_in, n_out, fid, b.ctypes.data, k.ctypes.data) == EINVAL
        assert lib.cnnitmo_last_error()
    assert lib.cnnitmo_resize_coeffs(8, 4, 1, b.ctypes.data, None) == EINVAL  # one table without the other
    assert lib.cnnitmo_resize_coeffs(8, 4, 1, None, k.ctypes.data) == EINVAL
    assert not b.any() and not k.any()
    assert lib.cnnitmo_version() == 2


def test_host_queries(lib):
    """The workspace is the intermediate picture, 0 when fewer than two passes run; the tile query
    needs no GPU: 0 (the direct path) for the 97-tap case, a tile for an upscale."""
    assert lib.cnnitmo_resize_workspace_bytes(0, 2, 10, 20, 5, 7) == 2 * 10 * 7 * 3 * 4
    assert lib.cnnitmo_resize_workspace_bytes(1, 2, 10, 20, 5, 7) == 2 * 10 * 7 * 3
    assert lib.cnnitmo_resize_workspace_bytes(0, 2, 10, 20, 10, 7) == 0
    assert lib.cnnitmo_resize_workspace_bytes(0, 2, 10, 20, 5, 20) == 0
    assert lib.cnnitmo_resize_workspace_bytes(0, 2, 10, 20, 10, 20) == 0
    assert lib.cnnitmo_resize_workspace_bytes(3, 2, 10, 20, 5, 7) == 0
    assert lib.cnnitmo_resize_workspace_bytes(0, 2, 10, 0, 5, 7) == 0
    assert lib.cnnitmo_resize_tile_cols(300, 19, 97) == 0
    assert lib.cnnitmo_resize_tile_cols(300, 19, 33) > 0
    assert lib.cnnitmo_resize_tile_cols(23, 100, 3) > 1
    assert lib.cnnitmo_resize_tile_cols(0, 19, 97) == 0


# ---------------------------------------------------------------- fit_within and argument errors
def test_fit_within():
    from cnn_itmo_amd.resize import fit_within
    assert fit_within(48, 80, 32) == (19, 32)  # 19.2
    assert fit_within(80, 48, 32) == (32, 19)
    assert fit_within(40, 64, 32) == (20, 32) and fit_within(33, 47, 32) == (22, 32)  # 22.47
    assert fit_within(64, 64, 32) == (32, 32)
    assert fit_within(4096, 8192, 1024) == (512, 1024) and fit_within(2160, 3840, 960) == (540, 960)
    assert fit_within(3, 4, 2) == (2, 2)  # 1.5: halves round up
    assert fit_within(5, 4, 2) == (2, 2)  # 1.6
    assert fit_within(1, 1000, 10) == (1, 10)  # never below one pixel
    assert fit_within(30, 32, 32) == (30, 32) and fit_within(7, 5, 100) == (7, 5)  # fits: unchanged
    for bad in [(0, 5, 3), (5, 5, 0), (5, -1, 3), (5.0, 5, 3)]:
        with pytest.raises(ValueError):
            fit_within(*bad)


def test_resize_argument_errors():
    """Checked before anything touches a GPU."""
    pytest.importorskip("torch")
    from cnn_itmo_amd.resize import resize
    x = np.zeros((4, 5, 3), np.float32)
    u = np.zeros((4, 5, 3), np.uint8)
    for args, kw in [((x, (2, 2), "hamming"), {}), ((x, (2, 2), "nearest"), {}), ((x, (0, 2)), {}),
                     ((x, (2, -1)), {}), ((x, (2.5, 2)), {}), ((x, 2), {}), ((x, (2, 2, 2)), {}),
                     ((x[..., :2], (2, 2)), {}), ((x[0], (2, 2)), {}), ((np.zeros((1, 1, 4, 5, 3)), (2, 2)), {}),
                     ((np.zeros((0, 5, 3), np.float32), (2, 2)), {}), ((u.astype(np.int32), (2, 2)), {}),
                     ((u, (2, 2)), {"floor": 0}), ((x, (2, 2)), {"floor": float("nan")}), (([[1, 2, 3]], (2, 2)), {})]:
        with pytest.raises(ValueError):
            resize(*args, **kw)


# ---------------------------------------------------------------- HDRPairGenerator's draw stream
def test_pair_generator_draw_stream(tmp_path):
    """With max_side the window draws use the resized sizes: the stream equals that of a generator over
    files that have those sizes; with max_side=None it equals the stream of a generator built without
    the argument.  next_draws() produces no pixels."""
    import cnn_itmo_amd as C
    from cnn_itmo_amd import hdrio
    big, small = tmp_path / "big", tmp_path / "small"
    os.makedirs(big), os.makedirs(small)
    sizes = {"a.pfm": (40, 64), "b.pfm": (33, 47), "c.pfm": (64, 64), "d.pfm": (20, 30)}
    fitted = [(20, 32), (22, 32), (32, 32), (20, 30)]
    for (name, (h, w)), (fh, fw) in zip(sizes.items(), fitted):
        hdrio.write_pfm(str(big / name), np.ones((h, w, 3), np.float32))
        hdrio.write_pfm(str(small / name), np.ones((fh, fw, 3), np.float32))
    gen = C.HDRPairGenerator(rotation_range=30, zoom_range=0.2, horizontal_flip=True)

    def flow(d, **kw):
        with contextlib.redirect_stdout(io.StringIO()):
            return gen.flow_from_directory(str(d), (16, 16), batch_size=3, seed=9, **kw)

    def stream(it, batches=4):
        return [[(d["j"], d["top"], d["left"], d["ch"], d["cw"], d["camera"], d["jpeg"],
                  sorted((k, float(v)) for k, v in d["params"].items() if np.isscalar(v)))
                 for d in it.next_draws()] for _ in range(batches)]

    a, b = flow(big, max_side=32, resample="lanczos"), flow(small)
    assert a.sizes == fitted == b.sizes and a.file_sizes == list(sizes.values())
    sa = stream(a)
    assert sa == stream(b)
    assert not a._sources and not b._sources  # nothing was loaded
    for blk in sa:
        for j, top, left, ch, cw, *_ in blk:
            assert 0 <= top <= fitted[j][0] - ch and 0 <= left <= fitted[j][1] - cw
    plain = stream(flow(big))
    assert stream(flow(big, max_side=None)) == plain
    assert stream(flow(big, max_side=64)) == plain  # no picture exceeds it
    assert sa != plain
    with pytest.raises(ValueError):  # 20 x 30 after the resize: smaller than the window
        with contextlib.redirect_stdout(io.StringIO()):
            gen.flow_from_directory(str(big), (24, 24), max_side=30)
    with pytest.raises(ValueError):
        flow(big, max_side=32, resample="hamming")
    with pytest.raises(ValueError):
        flow(big, max_side=0)
