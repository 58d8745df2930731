"""Host side of the JPEG round trip: the quantisation tables, the integer reference (tests/jpeg_ref.py)
against libjpeg through PIL, its properties and int32 range, and the generator's random stream.  No GPU.

The reference restates the IJG library's pixel path, and on the Pillow this was written against
(12.2.0, libjpeg-turbo) it equals PIL's own save + load byte for byte, for both subsamplings and
every quality tried: test_reference_equals_pil asserts that identity, which implies the issue's
condition PSNR(reference, PIL) >= PSNR(PIL, source) + 6 dB with room to spare; the condition is
asserted on its own as well, so that a libjpeg build with another DCT still has to meet it.
"""
import io

import numpy as np
import pytest

import jpeg_ref as J
from cnn_itmo_amd import degrade
from cnn_itmo_amd import hdrgen as G
from cnn_itmo_amd import hdrio

SUBS = ["4:4:4", "4:2:0"]
PIL_SUB = {"4:4:4": 0, "4:2:0": 2}


# ---------------------------------------------------------------- C1: tables
@pytest.mark.parametrize("q", [1, 10, 49, 50, 51, 75, 95, 100])
def test_tables_equal_the_reference(q):
    t = degrade.quant_tables(q)
    assert t.dtype == np.uint16 and t.shape == (2, 64)
    np.testing.assert_array_equal(t, J.quant_tables(q))
    assert t.min() >= 1 and t.max() <= 255


def test_tables_known_values():
    np.testing.assert_array_equal(degrade.quant_tables(50), np.stack([J.LUMA, J.CHROMA]))
    assert (degrade.quant_tables(100) == 1).all()
    assert list(degrade.quant_tables(75)[0][:8]) == [8, 6, 5, 8, 12, 20, 26, 31]
    for bad in (0, 101, -3, 50.5):
        with pytest.raises(ValueError):
            degrade.quant_tables(bad)


def _pil():
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check("jpg"):
        pytest.skip("Pillow without libjpeg")
    return Image


@pytest.mark.parametrize("q", [30, 75, 90])
def test_tables_are_the_ones_pil_writes(q):
    Image = _pil()
    b = io.BytesIO()
    Image.fromarray(_image(16, 16)).save(b, "JPEG", quality=q)
    b.seek(0)
    theirs = Image.open(b).quantization
    ours = degrade.quant_tables(q)
    for k in (0, 1):  # sorted: the order of PIL's lists differs between versions
        assert sorted(int(v) for v in theirs[k]) == sorted(int(v) for v in ours[k])


# ---------------------------------------------------------------- C2: the reference against libjpeg
def _image(h, w):
    """A smooth sinusoid per channel plus sigma = 12 Gaussian noise, seed 0."""
    rng = np.random.RandomState(0)
    r, c = np.mgrid[0:h, 0:w]
    img = np.stack([127.5 + 100 * np.sin(r / (5.0 + 2 * k) + c / (9.0 - 2 * k) + k) for k in range(3)], -1)
    return np.clip(np.round(img + rng.normal(0, 12, img.shape)), 0, 255).astype(np.uint8)


def _pil_roundtrip(img, q, sub):
    Image = _pil()
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=PIL_SUB[sub])
    b.seek(0)
    return np.array(Image.open(b).convert("RGB"))


def _psnr(a, b):
    m = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return np.inf if m == 0 else 10 * np.log10(255.0 ** 2 / m)


@pytest.mark.parametrize("shape", [(52, 76), (51, 75)], ids=["52x76", "51x75"])
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("q", [30, 50, 75, 90])
def test_reference_is_close_to_libjpeg(q, sub, shape):
    img = _image(*shape)
    theirs = _pil_roundtrip(img, q, sub)
    ours = J.roundtrip_u8(img, J.quant_tables(q), sub)
    ab, bs = _psnr(ours, theirs), _psnr(theirs, img)
    print(f"{shape} {sub} q{q}: reference vs PIL {ab:.2f} dB, PIL vs source {bs:.2f} dB")
    assert ab >= bs + 6.0


@pytest.mark.parametrize("shape", [(52, 76), (51, 75), (8, 8), (7, 5), (1, 1), (17, 23)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sub", SUBS)
def test_reference_equals_pil(sub, shape):
    """Byte identity with PIL's save + load (libjpeg-turbo's defaults), q = 95 and the extremes included."""
    img = _image(*shape)
    for q in (1, 10, 30, 50, 75, 90, 95, 100):
        np.testing.assert_array_equal(J.roundtrip_u8(img, J.quant_tables(q), sub), _pil_roundtrip(img, q, sub),
                                      err_msg=f"q{q}")


# ---------------------------------------------------------------- C3: properties
@pytest.mark.parametrize("level", [0, 1, 37, 127, 128, 200, 254, 255])
def test_grey_is_a_fixed_point_at_q100(level):
    img = np.full((11, 13, 3), level, np.uint8)
    np.testing.assert_array_equal(J.roundtrip_u8(img, J.quant_tables(100), "4:4:4"), img)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (8, 8), (9, 17), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_output_size(shape, sub):
    out = J.roundtrip_u8(_image(*shape), J.quant_tables(60), sub)
    assert out.shape == shape + (3,) and out.dtype == np.uint8


@pytest.mark.parametrize("sub", SUBS)
def test_int32_range_at_the_extremes(sub):
    """The reference asserts that every intermediate fits int32; these are the inputs that push it."""
    r, c = np.mgrid[0:32, 0:48]
    images = [np.zeros((32, 48), np.uint8), np.full((32, 48), 255, np.uint8),
              (((r + c) & 1) * 255).astype(np.uint8), ((((r >> 3) + (c >> 3)) & 1) * 255).astype(np.uint8)]
    for g in images:
        for q in (100, 1):
            for img in (np.stack([g] * 3, -1), np.stack([g, 255 - g, g], -1)):
                out = J.roundtrip_u8(img, J.quant_tables(q), sub)
                assert out.shape == img.shape
    for g in images[:2]:  # flat: unchanged at q = 100
        img = np.stack([g] * 3, -1)
        np.testing.assert_array_equal(J.roundtrip_u8(img, J.quant_tables(100), sub), img)


def test_float_form_and_pass_through():
    """roundtrip: step 1's rounding, the stored float of a level, apply = 0 copies the bits."""
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.1, 1.1, (2, 9, 10, 3)).astype(np.float32)
    x[0, 0, 0] = [np.nan, 0.5 / 255, 1.5 / 255]
    u = J.im2uint8(x)
    assert list(u[0, 0, 0]) == [0, 1, 2] and u.min() == 0 and u.max() == 255
    out = J.roundtrip(x, J.quant_tables(80), "4:2:0", apply=[1, 0])
    np.testing.assert_array_equal(out[1].view(np.uint32), x[1].view(np.uint32))
    want = J.roundtrip_u8(u[0], J.quant_tables(80), "4:2:0")
    np.testing.assert_array_equal(out[0], want.astype(np.float32) * np.float32(1 / 255.))
    levels = J.to_float(np.arange(256, dtype=np.uint8))
    np.testing.assert_array_equal(J.im2uint8(levels), np.arange(256))


# ---------------------------------------------------------------- C4: the stream
@pytest.fixture()
def pfm_dir(tmp_path):
    rng = np.random.default_rng(1)
    for k in range(2):
        hdrio.write_pfm(str(tmp_path / f"{k}.pfm"), rng.lognormal(0.0, 1.0, (20, 24, 3)).astype(np.float32))
    return str(tmp_path)


def _flow(root, seed=3, **kw):
    gen = G.HDRPairGenerator(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2, **kw)
    return gen.flow_from_directory(root, target_size=(8, 12), batch_size=2, seed=seed)


EARLIER = ("j", "params", "top", "left", "ch", "cw", "camera")


def test_stream_is_unchanged_when_off(pfm_dir):
    """Steps 1-3 restated from the RandomState: the second frame starts where step 3 of the first ended."""
    it = _flow(pfm_dir)
    d = it.next_draws()
    assert len(d) == 2 and all(f.get("jpeg", 0) == 0 for f in d)
    rs = np.random.RandomState(3)
    rs.permutation(2)
    for frame in d:
        theta = rs.uniform(-90, 90)
        zx, zy = rs.uniform(0.8, 1.2, 2)
        fh, fv = rs.random_sample() < 0.5, rs.random_sample() < 0.5
        assert (frame["params"]["theta"], frame["params"]["zx"], frame["params"]["zy"]) == (theta, zx, zy)
        assert (bool(frame["params"]["flip_horizontal"]), bool(frame["params"]["flip_vertical"])) == (fh, fv)
        assert frame["top"] == rs.randint(0, 20 - 8 + 1) and frame["left"] == rs.randint(0, 24 - 12 + 1)
        v = 8 * rs.random_sample() - 4
        n = rs.normal(0.6, np.sqrt(0.1))
        while n <= 0:
            n = rs.normal(0.6, np.sqrt(0.1))
        y = rs.normal(0.9, np.sqrt(0.1))
        while y <= 0:
            y = rs.normal(0.9, np.sqrt(0.1))
        assert frame["camera"] == (v, n, y)


def test_stream_with_a_quality_range(pfm_dir):
    off, on = _flow(pfm_dir), _flow(pfm_dir, jpeg_quality=(30, 90), jpeg_prob=0.5)
    seen = []
    for b in range(20):
        d0, d1 = off.next_draws(), on.next_draws()
        # the generator reseeds before every batch: the first frame of each batch has drawn nothing of step 4 yet
        assert all(d0[0][k] == d1[0][k] for k in EARLIER)
        seen += [d["jpeg"] for d in d1]
    assert len(seen) == 40 and all(q == 0 or 30 <= q <= 90 for q in seen)
    assert any(q == 0 for q in seen) and any(q > 0 for q in seen)
    # step 4 restated for the first batch: u, then q whether or not it is used
    on = _flow(pfm_dir, jpeg_quality=(30, 90), jpeg_prob=0.5)
    d = on.next_draws()
    rs = np.random.RandomState(3)
    rs.permutation(2)
    for frame in d:
        rs.uniform(-90, 90), rs.uniform(0.8, 1.2, 2), rs.random_sample(), rs.random_sample()
        rs.randint(0, 13), rs.randint(0, 13), rs.random_sample()
        for mean in (0.6, 0.9):
            while rs.normal(mean, np.sqrt(0.1)) <= 0:
                pass
        u = rs.random_sample()
        q = int(rs.randint(30, 91))
        assert frame["jpeg"] == (q if u < 0.5 else 0)


def test_fixed_quality_draws_only_the_gate(pfm_dir):
    on = _flow(pfm_dir, jpeg_quality=60, jpeg_prob=0.5)
    seen = [d["jpeg"] for _ in range(20) for d in on.next_draws()]
    assert set(seen) == {0, 60}
    assert all(d["jpeg"] == 60 for d in _flow(pfm_dir, jpeg_quality=60).next_draws())
    assert all(d["jpeg"] == 0 for d in _flow(pfm_dir, jpeg_quality=60, jpeg_prob=0.0).next_draws())


def test_fixed_cameras_repeat_the_jpeg_draw_every_epoch(pfm_dir):
    it = _flow(pfm_dir, cameras="fixed", jpeg_quality=(30, 90), jpeg_prob=0.5)
    first = {d["j"]: d["jpeg"] for d in it.next_draws()}
    second = {d["j"]: d["jpeg"] for d in it.next_draws()}
    assert len(first) == 2 and first == second
    for j, q in first.items():
        own = np.random.default_rng(3 + j)
        from cnn_itmo_amd.tonemap import virtual_camera_params
        virtual_camera_params(1, own)
        u = own.random()
        assert q == (int(own.integers(30, 91)) if u < 0.5 else 0)
    # the geometry's stream is the one of a generator without JPEG
    plain = _flow(pfm_dir, cameras="fixed")
    again = _flow(pfm_dir, cameras="fixed", jpeg_quality=(30, 90), jpeg_prob=0.5)
    for _ in range(3):
        for a, b in zip(plain.next_draws(), again.next_draws()):
            assert all(a[k] == b[k] for k in EARLIER)


@pytest.mark.parametrize("kw", [dict(jpeg_quality=0), dict(jpeg_quality=101), dict(jpeg_quality=(60, 40)),
                                dict(jpeg_quality=(0, 40)), dict(jpeg_quality=50, jpeg_prob=-0.1),
                                dict(jpeg_quality=50, jpeg_prob=1.5), dict(jpeg_quality=50, jpeg_subsampling="4:2:2"),
                                dict(jpeg_quality=50, quantize=None)],
                         ids=["q0", "q101", "lo>hi", "lo0", "p<0", "p>1", "subsampling", "quantize-none"])
def test_bad_arguments(kw):
    with pytest.raises(ValueError):
        G.HDRPairGenerator(**kw)


def test_workspace_query_needs_no_gpu():
    from cnn_itmo_amd import ops
    assert ops.jpeg_workspace_bytes(1, 1, 1, "4:4:4") == 3 * 64
    assert ops.jpeg_workspace_bytes(1, 1, 1, "4:2:0") == 256 + 2 * 64
    assert ops.jpeg_workspace_bytes(2, 17, 23, "4:2:0") == 2 * (32 * 32 + 2 * 16 * 16)
    assert ops.jpeg_workspace_bytes(3, 40, 72, "4:4:4") == 3 * 3 * 40 * 72
    assert ops.jpeg_workspace_bytes(0, 8, 8, "4:4:4") == 0 and ops.jpeg_workspace_bytes(1, 0, 8, "4:2:0") == 0
