"""The JPEG round trip on the GPU (csrc/jpeg.hip, ops, degrade, HDRPairGenerator) against the integer
reference (tests/jpeg_ref.py).  The contract is identity: every comparison is of the float bits, none
has a tolerance.

TILE = 64: the width of the tile one workgroup of jpeg_codec takes; its height is 64 for 4:2:0 and 32
for 4:4:4, so TILE + 1 in both dimensions is more than one tile either way.
"""
import contextlib
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cnn_itmo_amd as C  # noqa: E402
import jpeg_ref as J  # noqa: E402
from arena import Arena, poison_count  # noqa: E402
from cnn_itmo_amd import degrade  # noqa: E402
from cnn_itmo_amd import hdrgen as G  # noqa: E402
from cnn_itmo_amd import hdrio  # noqa: E402

TILE = 64
SUBS = ["4:4:4", "4:2:0"]
QUALITIES = [10, 50, 75, 100]
# 1x7x5: less than a block; 2x17x23: part blocks and odd sizes (4:2:0) both ways; TILE + 1: a second tile
# of one pixel both ways
SHAPES = ["1x1x1", "1x7x5", "1x8x8", "1x16x16", "2x17x23", f"1x{TILE + 1}x{TILE + 1}"]
_X, _REF = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_itmo_amd import _lib as L
    L.load()


def levels(shape, seed=0):
    """uint8 [n,h,w,3]: smooth plus noise, with a patch of 0 and one of 255 (where there is room)."""
    n, h, w = shape
    rng = np.random.RandomState(seed + 1000 * h + w)
    r, c = np.mgrid[0:h, 0:w]
    img = np.stack([np.stack([127.5 + 90 * np.sin(r / (4.0 + k + i) + c / (7.0 - k) + i) for k in range(3)], -1)
                    for i in range(n)])
    u = np.clip(np.round(img + rng.normal(0, 10, img.shape)), 0, 255).astype(np.uint8)
    if h >= 7 and w >= 5:
        u[:, 1:1 + h // 3, 1:1 + w // 3] = 0
        u[:, h - 1 - h // 3:h - 1, w - 1 - w // 3:w - 1] = 255
    return u


def _x(case):
    if case not in _X:
        _X[case] = J.to_float(levels(tuple(int(v) for v in case.split("x"))))
    return _X[case]


def _ref(case, sub, quals, apply=None):
    """The reference's floats for a case, computed once and read only."""
    key = (case, sub, tuple(quals), None if apply is None else tuple(apply))
    if key not in _REF:
        _REF[key] = J.roundtrip(_x(case), np.stack([J.quant_tables(q) for q in quals]), sub, apply)
    return _REF[key]


def _dev(a, off=0):
    """a on the device, `off` floats past a 16-byte boundary."""
    buf = torch.empty(a.size + off, dtype=torch.float32, device="cuda")
    v = buf[off:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _run(x, quals, sub, apply=None, off=0, inplace=False):
    from cnn_itmo_amd import ops
    xd = _dev(x, off)
    out = xd if inplace else _dev(np.full(x.shape, np.nan, np.float32), off)
    ops.jpeg_roundtrip(xd, np.stack([degrade.quant_tables(q) for q in quals]), sub, apply=apply, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(got, want):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} floats differ, the first at {np.argwhere(bad)[0]}"


# ---------------------------------------------------------------- G1: the kernel equals the reference
@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("case", SHAPES)
def test_kernel_equals_reference(case, sub, q):
    n = int(case.split("x")[0])
    same_bits(_run(_x(case), [q] * n, sub), _ref(case, sub, [q] * n))


@pytest.mark.parametrize("sub", SUBS)
def test_per_image_quality_and_pass_through(sub):
    """3x40x72: qualities 10 and 75 and an image that is copied through, in one call."""
    x = _x("3x40x72")
    got = _run(x, [10, 75, 50], sub, apply=[1, 1, 0])
    same_bits(got, _ref("3x40x72", sub, [10, 75, 50], [1, 1, 0]))
    same_bits(got[2], x[2])
    assert (got[0] != got[1]).any() and (got[0] != x[0]).any()


@pytest.mark.parametrize("sub", SUBS)
def test_more_images_than_one_launch_takes(sub):
    """11 images: the tables travel eight images at a time; image 9 is copied through."""
    x = np.concatenate([_x("2x17x23")] * 6)[:11]
    quals = [10, 50, 75, 100, 20, 30, 40, 60, 70, 80, 90]
    apply = [1] * 9 + [0, 1]
    want = J.roundtrip(x, np.stack([J.quant_tables(q) for q in quals]), sub, apply)
    same_bits(_run(x, quals, sub, apply=apply), want)


@pytest.mark.parametrize("sub", SUBS)
def test_unaligned_and_in_place(sub):
    """x and out one float off a 16-byte boundary, and out = x: the same bits."""
    want = _ref("2x17x23", sub, [75, 75])
    same_bits(_run(_x("2x17x23"), [75, 75], sub, off=1), want)
    same_bits(_run(_x("2x17x23"), [75, 75], sub, inplace=True), want)
    got = _run(_x("3x40x72"), [10, 75, 50], sub, apply=[1, 1, 0], inplace=True, off=3)
    same_bits(got, _ref("3x40x72", sub, [10, 75, 50], [1, 1, 0]))


@pytest.mark.parametrize("sub", SUBS)
def test_inputs_off_the_8_bit_levels(sub):
    """Step 1: uint8(255 x), half away from zero, saturating, NaN -> 0."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.05, 1.05, (1, 19, 21, 3)).astype(np.float32)
    k = np.arange(19 * 21 * 3).reshape(1, 19, 21, 3)
    x = np.where(k % 5 == 0, ((k % 255) + 0.5) / 255.0, x).astype(np.float32)  # ties, up to fp32's rounding
    x[0, 0, 0] = [np.nan, np.inf, -np.inf]
    x[0, 0, 1] = [0.5 / 255, 254.5 / 255, 1.0]
    same_bits(_run(x, [90], sub), J.roundtrip(x, J.quant_tables(90), sub))


# ---------------------------------------------------------------- G2: poisoned arena
def _raw(x, n, h, w, sub, qt, apply, out, ws, nbytes):
    from cnn_itmo_amd import _lib as L, ops
    p = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    q = None if qt is None else qt.ctypes.data
    a = None if apply is None else apply.ctypes.data
    return L.load().cnnitmo_jpeg_roundtrip(p(x), n, h, w, sub, q, a, p(out), p(ws), nbytes, ops.stream_ptr())


@pytest.mark.parametrize("sub", SUBS)
def test_poisoned_arena(sub):
    """x, out and the workspace carved from a NaN-poisoned arena: out fully written, the reference's
    bits, nothing outside out and the workspace touched, x unchanged.  2 x (TILE + 3) x (TILE + 9):
    several tiles, part blocks, odd sizes."""
    from cnn_itmo_amd import ops
    n, h, w = 2, TILE + 3, TILE + 9
    u = levels((n, h, w), seed=2)
    x = J.to_float(u)
    qt = np.stack([degrade.quant_tables(q) for q in (35, 85)])
    ar = Arena(16 << 20, "nan", "cuda")
    xd = ar.take(x.size, torch.float32, x, "x")
    out = ar.take(x.size, torch.float32, name="out")
    nb = ops.jpeg_workspace_bytes(n, h, w, sub)
    ws = ar.take(nb, torch.uint8, name="workspace", align=16)
    assert _raw(xd, n, h, w, ops.JPEG_SUBSAMPLINGS[sub], qt, None, out, ws, nb) == 0
    ar.check_untouched()
    assert poison_count(out) == 0
    same_bits(xd.cpu().numpy().reshape(x.shape), x)
    same_bits(out.cpu().numpy().reshape(x.shape), J.roundtrip(x, qt, sub))


# ---------------------------------------------------------------- G3: repeatability and errors
@pytest.mark.parametrize("sub", SUBS)
def test_two_runs_give_equal_bits(sub):
    x = _x("3x40x72")
    same_bits(_run(x, [10, 75, 50], sub), _run(x, [10, 75, 50], sub))


def test_bad_arguments_write_nothing():
    from cnn_itmo_amd import ops
    n, h, w = 2, 16, 16
    x = torch.rand(n, h, w, 3, device="cuda")
    out = torch.full((n, h, w, 3), float("nan"), device="cuda")
    nb = ops.jpeg_workspace_bytes(n, h, w, "4:2:0")
    ws = ops.workspace(nb)
    qt = np.stack([degrade.quant_tables(50)] * n)
    zero = qt.copy()
    zero[1, 1, 63] = 0
    bad = [dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(sub=2), dict(sub=-1), dict(qt=zero), dict(nb=nb - 1),
           dict(x=None), dict(out=None), dict(ws=None), dict(qt=None), dict(out=x.view(-1)[3:])]
    for ch in bad:
        a = dict(dict(x=x, n=n, h=h, w=w, sub=1, qt=qt, out=out, ws=ws, nb=nb), **ch)
        assert _raw(a["x"], a["n"], a["h"], a["w"], a["sub"], a["qt"], None, a["out"], a["ws"], a["nb"]) == -1, ch
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert _raw(x, n, h, w, 1, qt, None, out, ws, nb) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


# ---------------------------------------------------------------- G4: the front end
@pytest.mark.parametrize("sub", SUBS)
def test_degrade_front_end(sub):
    u = levels((2, 17, 23))
    x = J.to_float(u)
    want = J.roundtrip(x, np.stack([J.quant_tables(q) for q in (40, 80)]), sub)
    got = degrade.jpeg_roundtrip(x, [40, 80], sub)  # float numpy, a batch
    assert got.is_cuda and got.dtype == torch.float32
    same_bits(got.cpu().numpy(), want)
    got = degrade.jpeg_roundtrip(torch.from_numpy(u).cuda(), [40, 80], sub)  # uint8 tensor, a batch
    assert got.is_cuda and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), J.im2uint8(want))
    one = degrade.jpeg_roundtrip(u[1], 80, sub)  # uint8 numpy, one image
    assert one.dtype == torch.uint8 and tuple(one.shape) == (17, 23, 3)
    np.testing.assert_array_equal(one.cpu().numpy(), J.roundtrip_u8(u[1], J.quant_tables(80), sub))
    one = degrade.jpeg_roundtrip(torch.from_numpy(x[0]).cuda(), 40, sub)  # float tensor, one image
    same_bits(one.cpu().numpy(), want[0])
    for bad in (dict(quality=0), dict(quality=[40]), dict(subsampling="4:2:2")):
        with pytest.raises(ValueError):
            degrade.jpeg_roundtrip(x, **{"quality": 75, "subsampling": sub, **bad})
    with pytest.raises(ValueError):
        degrade.jpeg_roundtrip(x[..., :2], 75, sub)


@pytest.fixture()
def pfm_dir(tmp_path):
    rng = np.random.default_rng(2)
    for k in range(2):
        hdrio.write_pfm(str(tmp_path / f"{k}.pfm"), rng.lognormal(-1.0, 1.2, (40, 56, 3)).astype(np.float32))
    return str(tmp_path)


def _flow(root, gen_kw=None, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return G.HDRPairGenerator(**(gen_kw or {})).flow_from_directory(root, (32, 48), seed=4, **kw)


@pytest.mark.parametrize("sub", SUBS)
def test_generator_fixed_quality(pfm_dir, sub):
    """No geometry, a centre window, fixed cameras: nothing is drawn from the stream, so the frames of
    the generator with and without JPEG are the same frames."""
    kw = dict(window="center", batch_size=2, shuffle=False)
    x0, y0 = next(_flow(pfm_dir, dict(cameras="fixed"), **kw))
    it = _flow(pfm_dir, dict(cameras="fixed", jpeg_quality=70, jpeg_subsampling=sub), **kw)
    x1, y1 = next(it)
    assert [d["jpeg"] for d in it.last_draws] == [70, 70]
    assert torch.equal(y1, y0)
    same_bits(x1.cpu().numpy(), J.roundtrip(x0.cpu().numpy(), J.quant_tables(70), sub))
    assert not torch.equal(x1, x0)
    xp, yp = next(_flow(pfm_dir, dict(cameras="fixed", jpeg_quality=70, jpeg_prob=0.0, jpeg_subsampling=sub), **kw))
    assert torch.equal(xp, x0) and torch.equal(yp, y0)
    xn, yn = next(_flow(pfm_dir, dict(cameras="fixed", jpeg_quality=70, jpeg_subsampling=sub), output="numpy", **kw))
    assert isinstance(xn, np.ndarray) and isinstance(yn, np.ndarray)
    same_bits(xn, x1.cpu().numpy())
    same_bits(yn, y0.cpu().numpy())


def test_generator_range_compresses_the_drawn_frames(pfm_dir):
    """Batches of one frame (the stream is reseeded before every batch, so the frame before step 4 is
    the feature-off frame): compressed exactly when the draw says so, at the drawn quality."""
    geo = dict(rotation_range=90, horizontal_flip=True, zoom_range=0.2)
    off = _flow(pfm_dir, geo, batch_size=1)
    on = _flow(pfm_dir, dict(jpeg_quality=(30, 90), jpeg_prob=0.5, **geo), batch_size=1)
    seen = []
    for _ in range(8):
        (x0, y0), (x1, y1) = next(off), next(on)
        q = on.last_draws[0]["jpeg"]
        seen.append(q)
        assert q == 0 or 30 <= q <= 90
        assert torch.equal(y1, y0)
        if q:
            same_bits(x1.cpu().numpy(), J.roundtrip(x0.cpu().numpy(), J.quant_tables(q), "4:2:0"))
        else:
            assert torch.equal(x1, x0)
    assert 0 in seen and any(seen), seen


# ---------------------------------------------------------------- G5: one training step
def test_one_training_step_from_a_jpeg_generator(pfm_dir):
    with contextlib.redirect_stdout(io.StringIO()):
        gen = G.HDRPairGenerator(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2,
                                 jpeg_quality=(30, 90)) \
            .flow_from_directory(pfm_dir, (32, 32), batch_size=2, seed=1)
        C.clear_session()
        m = C.U_net(input_size=(32, 32, 3), verbose=False)
    hist = m.fit_generator(gen, steps_per_epoch=1, epochs=1, verbose=0)
    assert np.isfinite(hist.history["loss"][0])
    assert all(30 <= d["jpeg"] <= 90 for d in gen.last_draws)
