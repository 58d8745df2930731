"""cnnitmo_hdr_pairs (csrc/hdrpairs.hip) and HDRPairGenerator on the GPU against tests/hdrgen_ref.py:
scipy's warp, the tone-mapping oracle, the sanitise and quantise rules.

Tolerances.  (a) warped: 2e-6 * max|source window| per frame, test_gpu_warp_matches_scipy's bound
(2e-6 of a full scale of 1) rescaled to the frame's own full scale.  (b) logsum: rtol 1e-12 against
the sequential sum over the GPU's own warped pixels (the pictures' mean log is about -1 per pixel, so
the sum does not cancel).  (c) unquantised x, y: rtol 2e-6 against the oracle curves of the GPU's own
warped pixels (test_tonemap.py's header: the last bits of log / exp / pow differ); values the
reference sanitised (0 where Y = 0, 1 where clipped) are exact.  (d) quantised: at most one level
apart on a share below 1e-3 (a .5 tie of 255 v), bit-equal elsewhere."""
import contextlib
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import datagen as D  # noqa: E402
from cnn_itmo_amd import hdrgen as G  # noqa: E402
from cnn_itmo_amd import hdrio  # noqa: E402
import hdrgen_ref as R  # noqa: E402
import rgbe_ref as RR  # noqa: E402
from arena import Arena, poison_count  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 24, 40
CAMERAS = [(0.5, 0.6, 0.9), (-2.0, 0.3, 1.1), (3.0, 0.9, 0.7), (-3.5, 1.2, 0.5)]
KEY = 0.18


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def source_matrix(p, window, h=H, w=W):
    """M_src = T(top, left) . S . M_keras of the package, as [6] float64, and the flip bits."""
    top, left, ch, cw = window
    m6, flips = D.ImageDataGenerator.affine(p, h, w)
    m = np.vstack([m6.reshape(2, 3), [0.0, 0.0, 1.0]])
    t = np.array([[1, 0, top], [0, 1, left], [0, 0, 1]], np.float64)
    return np.dot(t, np.dot(G.resize_matrix(ch, cw, h, w), m))[:2].reshape(-1), flips


def launch(srcs, windows, mats, flips, cams, quantize=0, extras=True, h=H, w=W, arena=None):
    """One cnnitmo_hdr_pairs call.  srcs: numpy pictures (uint8 [h,w,4] or float32 [h,w,3]) or device
    tensors; windows (top, left, ch, cw); returns numpy x, y, warped, logsum (None without extras).
    With an arena every operand is carved from it."""
    from cnn_itmo_amd import ops
    n = len(srcs)
    cam = np.array([[KEY * 2.0 ** v, cn, cy] for v, cn, cy in cams], np.float64)
    mats = np.ascontiguousarray(mats, np.float64)
    flips = np.asarray(flips, np.int32)
    win = [(t, l, t + ch - 1, l + cw - 1) for t, l, ch, cw in windows]

    def dev(a, dtype, name):
        a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if arena is None:
            return a.cuda()
        return arena.take(a.numel(), dtype, a, name).view(a.shape)

    def out(shape, dtype, name):
        if arena is None:
            return torch.empty(shape, dtype=dtype, device="cuda")
        return arena.take(int(np.prod(shape)), dtype, name=name).view(shape)

    pics = [dev(s, torch.uint8 if str(s.dtype).endswith("uint8") else torch.float32, f"src{i}")
            for i, s in enumerate(srcs)]
    desc = dev(ops.hdr_descriptors(pics, win).view(np.uint8).reshape(-1), torch.uint8, "descriptors")
    dm, df, dc = dev(mats, torch.float64, "mats"), dev(flips, torch.int32, "flips"), dev(cam, torch.float64, "cam")
    x, y = out((n, h, w, 3), torch.float32, "x"), out((n, h, w, 3), torch.float32, "y")
    warped = out((n, h, w, 3), torch.float32, "warped") if extras else None
    logsum = out((n,), torch.float64, "logsum") if extras else None
    ws = out((ops.hdr_pairs_workspace_bytes(n),), torch.uint8, "workspace")
    ops.hdr_pairs(desc, dm, df, dc, x, y, key=KEY, quantize=quantize, warped=warped, logsum=logsum, ws=ws)
    torch.cuda.synchronize()
    res = [t if t is None else t.cpu().numpy() for t in (x, y, warped, logsum)]
    return res, (x, y, warped, logsum)


@pytest.fixture(scope="module")
def case():
    """Four frames of 24 x 40 from four pictures; the reference warp of each, computed once."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(11)
    f0, f3 = R.radiance(rng, 37, 53), R.radiance(rng, 64, 64)
    q1, q2 = RR.encode(R.radiance(rng, 41, 29)), RR.encode(R.radiance(rng, 24, 40))
    srcs = [f0, q1, q2, f3]
    pics = [f0, RR.decode(q1), RR.decode(q2), f3]  # what the sources hold, as float32
    windows = [(13, 13, H, W),   # a corner window of target size
               (0, 0, 41, 29),   # the whole picture, resized
               (0, 0, 24, 40),   # the whole picture = the target size
               (5, 9, 48, 50)]   # a resized window
    g = D.ImageDataGenerator(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2)
    rs = np.random.RandomState(5)
    params = [g.get_random_transform((H, W, 3), rs) for _ in range(4)]
    params[0].update(theta=0, zx=1, zy=1, flip_horizontal=False, flip_vertical=False)  # identity
    params[1].update(theta=90.0, zx=1, zy=1, flip_horizontal=False, flip_vertical=False)  # exact quarter turn
    params[2].update(flip_horizontal=True, flip_vertical=False)
    params[3].update(flip_horizontal=True, flip_vertical=True)
    mats, flips = zip(*[source_matrix(p, wd) for p, wd in zip(params, windows)])
    ref_warp = [R.warp(pic, wd, p, H, W) for pic, wd, p in zip(pics, windows, params)]
    args = (srcs, windows, np.stack(mats), flips, CAMERAS)
    (x, y, warped, logsum), _ = launch(*args)
    return dict(args=args, pics=pics, windows=windows, ref_warp=ref_warp, x=x, y=y, warped=warped, logsum=logsum)


def test_warped_matches_scipy(case):
    zeros = 0
    for i, (pic, (t, l, ch, cw)) in enumerate(zip(case["pics"], case["windows"])):
        scale = float(np.abs(pic[t:t + ch, l:l + cw]).max())
        err = float(np.abs(case["warped"][i] - case["ref_warp"][i]).max())
        print(f"frame {i}: warp max-abs error {err:.3e}, bound {2e-6 * scale:.3e}")
        assert err <= 2e-6 * scale, (i, err, scale)
        zeros += int((case["warped"][i].max(-1) == 0).sum())
    assert zeros > 0  # black pixels reach the tone curves
    # the identity frame returns its window bit for bit
    np.testing.assert_array_equal(case["warped"][0], case["pics"][0][13:13 + H, 13:13 + W])


def test_logsum_matches_sequential_sum(case):
    for i in range(4):
        ref = R.logsum(case["warped"][i])
        print(f"frame {i}: logsum {case['logsum'][i]!r}, reference {ref!r}")
        np.testing.assert_allclose(case["logsum"][i], ref, rtol=1e-12)


def test_pairs_match_oracle_curves(case):
    clipped = black = 0
    for i in range(4):
        xr, yr, xc, yc = R.pair(case["warped"][i], CAMERAS[i], KEY)
        for got, ref, raw in ((case["x"][i], xr, xc), (case["y"][i], yr, yc)):
            assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
            np.testing.assert_allclose(got, ref, rtol=2e-6, atol=1e-37)
            fixed = np.isnan(raw) | (raw >= 1) | (raw <= 0)
            np.testing.assert_array_equal(got[fixed], ref[fixed])
            clipped += int((raw >= 1).sum())
            black += int(np.isnan(raw).sum())
    assert clipped > 0 and black > 0  # both sanitise rules were exercised


@pytest.mark.parametrize("quantize", [1, 2, 3])
def test_quantised_pairs(case, quantize):
    (x, y, warped, _), _ = launch(*case["args"], quantize=quantize)
    np.testing.assert_array_equal(warped, case["warped"])
    for i in range(4):
        xr, yr, _, _ = R.pair(warped[i], CAMERAS[i], KEY, quantize)
        for got, ref, bit, plain in ((x[i], xr, 1, case["x"][i]), (y[i], yr, 2, case["y"][i])):
            if not quantize & bit:  # the other output is the unquantised one
                np.testing.assert_array_equal(got, plain)
                continue
            lv = np.rint(got.astype(np.float64) * 255).astype(int)
            np.testing.assert_array_equal(got, lv.astype(np.float32) * np.float32(1 / 255.))
            d = np.abs(lv - np.rint(ref.astype(np.float64) * 255).astype(int))
            print(f"frame {i} bit {bit}: {int((d > 0).sum())} of {d.size} levels differ, max {d.max()}")
            assert d.max() <= 1 and (d > 0).mean() < 1e-3
            np.testing.assert_array_equal(got[d == 0], ref[d == 0])


def test_two_calls_are_bit_identical(case):
    (x, y, warped, logsum), _ = launch(*case["args"])
    for a, b in ((x, case["x"]), (y, case["y"]), (warped, case["warped"]), (logsum, case["logsum"])):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    # the optional outputs do not change the others
    (x2, y2, w2, l2), _ = launch(*case["args"], extras=False)
    assert w2 is None and l2 is None
    np.testing.assert_array_equal(x2, x)
    np.testing.assert_array_equal(y2, y)


@pytest.mark.parametrize("fmt", ["fp32", "rgbe"])
def test_taps_stay_inside_the_clamp_window(fmt):
    """A window surrounded by 1e30: the call equals the call on a copy of just the window, bit for
    bit.  The matrix entries, offsets and pixel indices are dyadic rationals of a few bits, so every
    coordinate is exact in float64 whichever translation is added; the map (a shear-zoom with
    offsets of several pixels, both flips) sends taps beyond every side of the window."""
    rng = np.random.default_rng(2)
    top, left = 10, 12
    inner = R.radiance(rng, H, W)
    big = np.full((50, 60, 3), 1e30, np.float32)
    big[top:top + H, left:left + W] = inner
    if fmt == "rgbe":
        big, inner = RR.encode(big), RR.encode(inner)
        np.testing.assert_array_equal(big[top:top + H, left:left + W], inner)
    m = np.array([0.75, 0.25, -3.5, -0.25, 1.25, -6.25])
    shift = np.array([0, 0, top, 0, 0, left], np.float64)
    cams = CAMERAS[:1]
    (a, _) = launch([big], [(top, left, H, W)], [m + shift], [3], cams)
    (b, _) = launch([inner], [(0, 0, H, W)], [m], [3], cams)
    limit = float((RR.decode(inner) if fmt == "rgbe" else inner).max())
    assert float(a[2].max()) <= limit and np.isfinite(a[3]).all()
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p.view(np.uint8), q.view(np.uint8))
    # the map does leave the window: without the clamp window the surrounding 1e30 is sampled
    (c, _) = launch([big], [(0, 0, big.shape[0], big.shape[1])], [m + shift], [3], cams)
    assert float(c[2].max()) > limit


def test_unaligned_rgbe_picture(case):
    """An RGBE picture that does not start on a 4-byte boundary is read by bytes: same result."""
    srcs, windows, mats, flips, cams = case["args"]
    q = srcs[1]
    buf = torch.zeros(q.size + 8, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + q.size].view(q.shape)
    view.copy_(torch.from_numpy(q))
    assert view.data_ptr() % 4 == 1
    (res, _) = launch([view], windows[1:2], mats[1:2], flips[1:2], cams[1:2])
    np.testing.assert_array_equal(res[0][0], case["x"][1])
    np.testing.assert_array_equal(res[2][0], case["warped"][1])
    assert res[3][0] == case["logsum"][1]


@pytest.mark.parametrize("extras", [True, False])
def test_operands_only(case, extras):
    """Every operand carved from a NaN-poisoned arena: the outputs are written completely, nothing
    else is, and the results are those of ordinary allocations."""
    ar = Arena(40 << 20, "nan", "cuda")
    (x, y, warped, logsum), dev = launch(*case["args"], extras=extras, arena=ar)
    ar.check_untouched()
    assert poison_count(dev[0]) == 0 and poison_count(dev[1]) == 0
    np.testing.assert_array_equal(x, case["x"])
    np.testing.assert_array_equal(y, case["y"])
    if extras:
        assert poison_count(dev[2]) == 0 and poison_count(dev[3]) == 0
        np.testing.assert_array_equal(warped, case["warped"])
        np.testing.assert_array_equal(logsum, case["logsum"])


def test_indices_past_2_31():
    """3 x 16384 x 16384: each output holds 2.4e9 floats, so the third frame's float indices pass
    2^31 (and byte offsets 2^32 in the first).  Frames 0 and 2 have the same arguments and must be
    equal bit for bit; every element is written (the outputs start as NaN)."""
    from cnn_itmo_amd import ops
    n, s = 3, 16384
    pic = torch.from_numpy(R.radiance(np.random.default_rng(6), 64, 64)).cuda()
    m = G.resize_matrix(64, 64, s, s)[:2].reshape(-1)
    cams = [CAMERAS[0], CAMERAS[1], CAMERAS[0]]
    desc = torch.from_numpy(ops.hdr_descriptors([pic] * n).view(np.uint8).reshape(-1)).cuda()
    mats = torch.from_numpy(np.stack([m] * n)).cuda()
    flips = torch.zeros(n, dtype=torch.int32, device="cuda")
    cam = torch.tensor([[KEY * 2.0 ** v, cn, cy] for v, cn, cy in cams], dtype=torch.float64, device="cuda")
    x = torch.full((n, s, s, 3), float("nan"), dtype=torch.float32, device="cuda")
    y = torch.full_like(x, float("nan"))
    assert x.numel() > 2 ** 31
    logsum = torch.empty(n, dtype=torch.float64, device="cuda")
    ops.hdr_pairs(desc, mats, flips, cam, x, y, key=KEY, logsum=logsum)
    assert not bool(torch.isnan(x).any()) and not bool(torch.isnan(y).any())
    assert torch.equal(x[2], x[0]) and torch.equal(y[2], y[0]) and torch.equal(y[1], y[0])
    assert not torch.equal(x[1], x[0])  # another camera
    assert float(logsum[0]) == float(logsum[1]) == float(logsum[2]) and np.isfinite(float(logsum[0]))
    del x, y
    torch.cuda.empty_cache()


def write_hdr_files(root, count, h, w, seed):
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    for k in range(count):
        with open(os.path.join(root, f"pic{k}.hdr"), "wb") as fh:
            fh.write(hdrio.format_hdr(RR.encode(R.radiance(rng, h, w))))


def test_equals_the_offline_path(tmp_path):
    """make_dataset's PNGs through two flow_from_directory streams against the generator with
    quantize='both', cameras='fixed' on the same files: one level apart on a share below 1e-3 (the
    two log-averages are folded over different partitions, so a .5 tie can fall either way)."""
    from cnn_itmo_amd.make_dataset import make_dataset
    hdr_dir, out = str(tmp_path / "hdr"), str(tmp_path / "data")
    write_hdr_files(hdr_dir, 3, 32, 48, seed=3)
    make_dataset(hdr_dir, out, cameras=1, seed=7, log=lambda *a: None)
    kw = dict(target_size=(32, 48), class_mode=None, batch_size=3, shuffle=False)
    with contextlib.redirect_stdout(io.StringIO()):
        xo = next(D.ImageDataGenerator(rescale=1 / 255).flow_from_directory(os.path.join(out, "input1"), **kw))
        yo = next(D.ImageDataGenerator(rescale=1 / 255).flow_from_directory(os.path.join(out, "output1"), **kw))
        it = G.HDRPairGenerator(quantize="both", cameras="fixed").flow_from_directory(
            hdr_dir, (32, 48), window="full", shuffle=False, seed=7, batch_size=3)
    x, y = next(it)
    assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (3, 32, 48, 3) == tuple(y.shape)
    for got, ref in ((x, xo), (y, yo)):
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        d = np.abs(np.rint(got.astype(np.float64) * 255) - np.rint(ref.astype(np.float64) * 255))
        print(f"{int((d > 0).sum())} of {d.size} levels differ, max {d.max()}")
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
        np.testing.assert_array_equal(got[d == 0], ref[d == 0])


def test_feeds_fit_generator(tmp_path):
    write_hdr_files(str(tmp_path), 4, 48, 64, seed=4)
    with contextlib.redirect_stdout(io.StringIO()):
        gen = G.HDRPairGenerator(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2) \
            .flow_from_directory(str(tmp_path), (32, 32), batch_size=2, seed=1)
        val = G.HDRPairGenerator(cameras="fixed").flow_from_directory(
            str(tmp_path), (32, 32), window="center", batch_size=4, shuffle=False, seed=1)
        cold = G.HDRPairGenerator(cameras="fixed").flow_from_directory(
            str(tmp_path), (32, 32), window="center", batch_size=4, shuffle=False, seed=1, cache=False,
            output="numpy")
    # two epochs of the fixed, unshuffled validation stream: the same batch, bit for bit
    (x1, y1), (x2, y2) = next(val), next(val)
    assert torch.equal(x1, x2) and torch.equal(y1, y2)
    assert len(val._sources) == 4
    xc, yc = next(cold)  # files re-read each batch, host arrays out
    assert not cold._sources
    np.testing.assert_array_equal(xc, x1.cpu().numpy())
    np.testing.assert_array_equal(yc, y1.cpu().numpy())
    xb, yb = next(gen)
    assert xb.is_cuda and tuple(xb.shape) == (2, 32, 32, 3) == tuple(yb.shape)
    lv = xb * 255  # the input is quantised by default, the target is not
    assert torch.equal(torch.round(lv).float() * np.float32(1 / 255.), xb) and not torch.equal(torch.round(yb * 255) / 255, yb)
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(32, 32, 3), verbose=False)
    hist = m.fit_generator(gen, steps_per_epoch=2, epochs=1, verbose=0, validation_data=val, validation_steps=1)
    assert np.isfinite(hist.history["loss"][0]) and np.isfinite(hist.history["val_loss"][0])
