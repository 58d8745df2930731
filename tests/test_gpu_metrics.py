"""GPU PSNR / SSIM (csrc/metrics.hip) against the numpy float64 reference (tests/metrics_ref.py).

Bounds: epoch logs print 4 decimals and checkpoint names 2, so the kernel has to sit well inside
0.5e-4: |ssim - ref64| <= 1e-6 per image (fp64 moment sums meet it with orders of margin; plain
fp32 misses it by 100x on flat images) and |psnr - ref64| <= 1e-4 dB (2.3e-5 relative in the MSE).
"""
import contextlib
import csv
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import metrics as M  # noqa: E402
import metrics_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-6
PSNR_TOL = 1e-4

# (2,11,11): a single window; the others give partial tiles in both directions for any tile up to 128
SHAPES = [(2, 11, 11), (1, 12, 27), (5, 45, 83), (1, 16, 200), (1, 200, 16), (1, 139, 261)]
_CASES = {}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(shape):
    """(prediction, target, reference psnr, reference ssim), computed once per shape."""
    if shape not in _CASES:
        noise = [0.01, 0.02, 0.03, 0.05, 0.08] if shape[0] == 5 else 0.03
        p, t = MR.make_pair(shape, seed=shape[1] * 1000 + shape[2], noise=noise)
        _CASES[shape] = (p, t, MR.psnr(p, t), MR.ssim(p, t))
    return _CASES[shape]


def _metrics(what, a, b, max_val=1.0):
    from cnn_itmo_amd import ops
    a, b = (torch.from_numpy(np.array(v, np.float32)).cuda() for v in (a, b))
    return ops.image_metrics(what, a, b, max_val).cpu().numpy()


@pytest.mark.parametrize("what", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_reference(shape, what):
    p, t, rp, rs = _case(shape)
    out = _metrics(what, p, t)
    assert out.shape == (shape[0], 3)
    if what & 1:
        print("psnr err", np.abs(out[:, 1] - rp).max())
        np.testing.assert_allclose(out[:, 0], MR.mse(p, t), rtol=2.3e-5, atol=0)
        assert np.abs(out[:, 1] - rp).max() <= PSNR_TOL, (out[:, 1], rp)
    else:
        assert np.isnan(out[:, :2]).all()  # not asked for: left untouched
    if what & 2:
        print("ssim err", np.abs(out[:, 2] - rs).max())
        assert np.abs(out[:, 2] - rs).max() <= SSIM_TOL, (out[:, 2], rs)
    else:
        assert np.isnan(out[:, 2]).all()
    if shape[0] == 5:  # five noise levels: five different values, each its own image's
        assert len(set(np.round(rp, 2))) == 5 and len(set(np.round(rs, 3))) == 5


def test_public_functions_and_input_forms():
    p, t, rp, rs = _case((5, 45, 83))
    ps, ss = M.psnr_ssim(p, t)
    assert ps.is_cuda and ps.dtype == torch.float64 and tuple(ps.shape) == (5,) and tuple(ss.shape) == (5,)
    assert np.abs(ps.cpu().numpy() - rp).max() <= PSNR_TOL and np.abs(ss.cpu().numpy() - rs).max() <= SSIM_TOL
    assert torch.equal(M.psnr(torch.as_tensor(p).cuda(), t), ps) and torch.equal(M.ssim(p, t), ss)
    one = M.ssim(p[2], t[2])  # [h,w,3]
    assert tuple(one.shape) == (1,) and one.item() == ss[2].item()
    # uint8: 0..255 values, max_val as given
    pu, tu = np.round(p * 255).astype(np.uint8), np.round(t * 255).astype(np.uint8)
    ps8, ss8 = M.psnr_ssim(pu, tu, max_val=255)
    assert np.abs(ps8.cpu().numpy() - MR.psnr(pu, tu, 255)).max() <= PSNR_TOL
    assert np.abs(ss8.cpu().numpy() - MR.ssim(pu, tu, 255)).max() <= SSIM_TOL


def test_closed_forms():
    a, b = np.full((1, 13, 14, 3), 0.25, np.float32), np.full((1, 13, 14, 3), 0.75, np.float32)
    want = (2 * 0.25 * 0.75 + 1e-4) / (0.25 ** 2 + 0.75 ** 2 + 1e-4)
    assert abs(want - 0.6000640) < 1e-7
    out = _metrics(3, a, b)
    assert abs(out[0, 2] - want) <= SSIM_TOL, out
    assert abs(out[0, 1] - 10 * np.log10(1 / 0.25)) <= PSNR_TOL
    x = np.random.default_rng(3).random((2, 20, 31, 3), dtype=np.float32)
    out = _metrics(3, x, x.copy())
    assert (np.abs(1 - out[:, 2]) <= SSIM_TOL).all() and np.isposinf(out[:, 1]).all() and (out[:, 0] == 0).all()
    z = np.zeros((1, 11, 12, 3), np.float32)
    out = _metrics(3, z, z)
    assert out[0, 2] == 1.0 and np.isposinf(out[0, 1])


def test_max_val_scaling():
    p, t, rp, rs = _case((1, 139, 261))
    lo, hi = _metrics(3, p, t, 1.0), _metrics(3, p * np.float32(255), t * np.float32(255), 255.0)
    assert np.abs(lo[:, 2] - hi[:, 2]).max() <= SSIM_TOL
    assert np.abs(lo[:, 1] - hi[:, 1]).max() <= PSNR_TOL


def test_bitwise_deterministic():
    p, t, _, _ = _case((5, 45, 83))
    a, b = _metrics(3, p, t), _metrics(3, p, t)
    assert a.tobytes() == b.tobytes()


def test_small_image_errors():
    from cnn_itmo_amd._lib import CnnItmoError
    x = np.random.default_rng(4).random((1, 10, 20, 3), dtype=np.float32)
    y = np.random.default_rng(5).random((1, 10, 20, 3), dtype=np.float32)
    for what in (2, 3):
        with pytest.raises(CnnItmoError, match="SSIM needs"):
            _metrics(what, x, y)
    with pytest.raises(ValueError, match="at least 11"):
        M.ssim(x, y)
    out = _metrics(1, x, y)
    assert abs(out[0, 1] - MR.psnr(x, y)[0]) <= PSNR_TOL
    assert abs(M.psnr(x, y).item() - MR.psnr(x, y)[0]) <= PSNR_TOL


def test_workspace_too_small_is_an_error():
    from cnn_itmo_amd import _lib, ops
    a = torch.zeros(1, 32, 32, 3, device="cuda")
    out = torch.zeros(1, 3, dtype=torch.float64, device="cuda")
    ws = ops.workspace(64)
    with pytest.raises(_lib.CnnItmoError, match="workspace too small"):
        _lib.call("cnnitmo_image_metrics", 3, a.data_ptr(), a.data_ptr(), 1, 32, 32, 1.0, out.data_ptr(),
                  ws.data_ptr(), 64, ops.stream_ptr())


# ---------------------------------------------------------------- model level
def _unet(input_size, dtype, pad=False, seed=4):
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=input_size, dtype=dtype, seed=seed, verbose=False, pad=pad)
    rng = np.random.default_rng(seed)
    m.set_named_weights({k: rng.uniform(0.5, 1.5, v.shape) for k, v in m.named_weights().items()
                         if k.endswith("/moving_variance")})
    return m


def _xy(n, h, w, seed):
    t, x = MR.make_pair((n, h, w), seed, noise=0.1)
    return x, t


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("size,pad", [((32, 32, 3), False), ((40, 48, 3), True)], ids=["32x32", "40x48pad"])
def test_evaluate_image_metrics(size, pad, dtype):
    x, y = _xy(3, size[0], size[1], 7)
    m = _unet(size, dtype, pad)
    base = m.evaluate(x, y)
    m.compile(m.optimizer, "mse", metrics=["accuracy", "psnr", "ssim"])
    assert m.metrics_names == ["loss", "acc", "psnr", "ssim"]
    got = m.evaluate(x, y)
    assert len(base) == 2 and len(got) == 4
    assert np.float64(got[:2]).tobytes() == np.float64(base).tobytes()  # loss, acc: bitwise the same
    pred = m.predict(x)
    assert pred.shape == y.shape
    rp, rs = MR.psnr(pred, y).mean(), MR.ssim(pred, y).mean()
    print("model psnr err", abs(got[2] - rp), "ssim err", abs(got[3] - rs))
    assert abs(got[2] - rp) <= PSNR_TOL and abs(got[3] - rs) <= SSIM_TOL, (got, rp, rs)
    # batches of 2 + 1: still the mean of the per-image values
    got2 = m.evaluate(x, y, batch_size=2)
    assert abs(got2[2] - rp) <= PSNR_TOL and abs(got2[3] - rs) <= SSIM_TOL
    m.compile(m.optimizer, "mse", metrics=["ssim"])
    only = m.evaluate(x, y)
    assert len(only) == 2 and only[0] == got[0] and only[1] == got[3]


def test_fit_generator_validation_checkpoint_and_reload(tmp_path):
    x, y = _xy(4, 32, 32, 11)
    xv, yv = _xy(3, 32, 32, 12)
    m = _unet((32, 32, 3), "float32")
    m.compile(m.optimizer, "mse", metrics=["accuracy", "psnr", "ssim"])

    def gen():
        while True:
            yield x[:2], y[:2]
            yield x[2:], y[2:]

    h = m.fit_generator(gen(), steps_per_epoch=2, epochs=1, verbose=0, validation_data=(xv, yv))
    assert sorted(h.history) == ["acc", "loss", "val_acc", "val_loss", "val_psnr", "val_ssim"]  # no training psnr/ssim
    ev = m.evaluate(xv, yv)
    for k, v in zip(m.metrics_names, ev):
        assert h.history["val_" + k] == [pytest.approx(v, rel=1e-14)]
    pred = m.predict(xv)
    assert abs(h.history["val_psnr"][0] - MR.psnr(pred, yv).mean()) <= PSNR_TOL
    assert abs(h.history["val_ssim"][0] - MR.ssim(pred, yv).mean()) <= SSIM_TOL

    pat = str(tmp_path / "m-{epoch:02d}-{val_psnr:.2f}.hdf5")
    ck = C.ModelCheckpoint(pat, monitor="val_psnr", save_best_only=True)
    h = m.fit_generator(gen(), steps_per_epoch=2, epochs=3, verbose=0, validation_data=(xv, yv), callbacks=[ck])
    vp = h.history["val_psnr"]
    assert len(vp) == 3
    want = [pat.format(epoch=e + 1, val_psnr=v) for e, v in enumerate(vp) if e == 0 or v > max(vp[:e])]
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in want)
    m2 = C.load_model(want[-1])
    assert m2.metrics_names == ["loss", "acc", "psnr", "ssim"] and m2.image_metrics == ["psnr", "ssim"]


def test_predict_cli_scores_written_pngs(tmp_path):
    from PIL import Image
    from cnn_itmo_amd import predict as PR
    m = _unet((32, 32, 3), "float32", seed=5)
    ck = str(tmp_path / "tiny.hdf5")
    m.save(ck)
    rng = np.random.default_rng(6)
    ind, refd, outd = tmp_path / "in", tmp_path / "ref", tmp_path / "out"
    for d in (ind, refd):
        os.makedirs(d)
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(str(ind / f"{i:04d}.png"))
        if i != 1:  # 0001.png has no reference: reported and skipped
            Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(str(refd / f"{i:04d}.png"))
    csvp = str(tmp_path / "scores.csv")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert PR.main(["--model", ck, "--input", str(ind), "--output", str(outd), "--reference", str(refd),
                        "--metrics-csv", csvp]) == 0
    with open(csvp, newline="") as fh:
        rows = list(csv.reader(fh, delimiter=";"))
    assert rows[0] == ["name", "psnr", "ssim"] and [r[0] for r in rows[1:]] == ["0000.png", "0002.png"]
    for name, ps, ss in rows[1:]:
        a, b = np.asarray(Image.open(str(outd / name))), np.asarray(Image.open(str(refd / name)))
        assert abs(float(ps) - MR.psnr(a, b, 255)[0]) <= PSNR_TOL and abs(float(ss) - MR.ssim(a, b, 255)[0]) <= SSIM_TOL
    log = buf.getvalue()
    assert "0001.png: no reference" in log and "mean of 2 scored files" in log
    assert sorted(os.listdir(outd)) == ["0000.png", "0001.png", "0002.png"]
    # a reference of another size is an error
    Image.fromarray(np.zeros((16, 32, 3), np.uint8)).save(str(refd / "0001.png"))
    with pytest.raises(ValueError, match="0001.png"), contextlib.redirect_stdout(io.StringIO()):
        PR.main(["--model", ck, "--input", str(ind), "--output", str(outd), "--reference", str(refd)])
