"""Host side of the PSNR / SSIM metrics: the numpy reference itself (tests/metrics_ref.py),
the C ABI's size query, compile()'s metric names, ModelCheckpoint's best/mode logic, the
metric names in a Keras HDF5 training_config, and the validation logs over DP ranks."""
import contextlib
import io
import json
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import metrics as M  # noqa: E402
import metrics_ref as MR  # noqa: E402


def _unet(**kw):
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        return C.U_net(input_size=(32, 32, 3), seed=2, verbose=False, **kw)


# ---------------------------------------------------------------- reference
def test_reference_taps_and_closed_form():
    g = MR.taps()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.allclose(g, g[::-1], rtol=0, atol=0)
    assert abs(g[5] / g[4] - np.exp(1 / 4.5)) < 1e-14
    a, b = np.full((13, 14, 3), 0.25), np.full((13, 14, 3), 0.75)
    assert abs(MR.ssim(a, b)[0] - (2 * 0.25 * 0.75 + 1e-4) / (0.25 ** 2 + 0.75 ** 2 + 1e-4)) < 1e-12
    assert abs(MR.psnr(a, b)[0] - 10 * np.log10(4.0)) < 1e-12
    assert np.isposinf(MR.psnr(a, a)[0]) and abs(MR.ssim(a, a)[0] - 1) < 1e-12
    with pytest.raises(ValueError):
        MR.ssim(np.zeros((10, 20, 3)), np.zeros((10, 20, 3)))


def test_reference_matches_conv2d_of_the_2d_window():
    """Separable valid filtering == a float64 grouped conv2d with the 11x11 outer-product window."""
    import torch.nn.functional as F
    g = torch.as_tensor(MR.taps())
    win = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)

    def conv(x, _g):
        t = torch.as_tensor(np.ascontiguousarray(x)).permute(0, 3, 1, 2)
        return F.conv2d(t, win, groups=3).permute(0, 2, 3, 1).numpy()

    for shape, seed in (((2, 11, 11), 1), ((3, 29, 41), 2)):
        p, t = MR.make_pair(shape, seed, noise=0.04)
        sep = MR.ssim_map(p, t)
        full = MR.ssim_map(p, t, filt=conv)
        assert sep.shape == (shape[0], shape[1] - 10, shape[2] - 10, 3)
        assert np.abs(sep - full).max() <= 1e-12
        assert np.abs(MR.ssim(p, t) - full.mean(axis=(1, 2, 3))).max() <= 1e-12


# ---------------------------------------------------------------- C ABI (no GPU)
def test_workspace_bytes_without_gpu():
    from cnn_itmo_amd import _lib, ops
    assert "cnnitmo_image_metrics" in _lib.SIGNATURES
    small, big = ops.image_metrics_workspace_bytes(1, 11, 11), ops.image_metrics_workspace_bytes(8, 1080, 1920)
    assert small > 0 and big > small
    assert ops.image_metrics_workspace_bytes(1, 5, 5) > 0  # PSNR alone has no size limit
    assert ops.image_metrics_workspace_bytes(3, 64, 64) == 3 * ops.image_metrics_workspace_bytes(1, 64, 64)
    assert ops.image_metrics_workspace_bytes(0, 64, 64) <= 0


# ---------------------------------------------------------------- compile
def test_compile_metric_names():
    m = _unet()
    assert m.metrics_names == ["loss", "acc"] and m.image_metrics == []
    m.compile("rmsprop", "mse", metrics=None)
    assert m.metrics_names == ["loss"] and m.image_metrics == []
    m.compile("rmsprop", "mse", metrics=["accuracy"])
    assert m.metrics_names == ["loss", "acc"]
    m.compile("rmsprop", "mse", metrics=["accuracy", "psnr", "ssim"])
    assert m.metrics_names == ["loss", "acc", "psnr", "ssim"] and m.image_metrics == ["psnr", "ssim"]
    m.compile("rmsprop", "mse", metrics=[M.ssim, "acc", M.psnr])
    assert m.metrics_names == ["loss", "ssim", "acc", "psnr"] and m.image_metrics == ["ssim", "psnr"]
    m.compile("rmsprop", "mse", metrics=["psnr"])
    assert m.metrics_names == ["loss", "psnr"]


@pytest.mark.parametrize("bad", ["mae", "ms-ssim", M.psnr_ssim, len, 3])
def test_compile_unknown_metric_raises(bad):
    m = _unet()
    with pytest.raises(NotImplementedError):
        m.compile("rmsprop", "mse", metrics=["accuracy", bad])
    assert m.metrics_names == ["loss", "acc"]  # a failed compile changes nothing


# ---------------------------------------------------------------- ModelCheckpoint
class _StubModel:
    def __init__(self):
        self.saved = []

    def save(self, path):
        self.saved.append(("model", path))

    def save_weights(self, path):
        self.saved.append(("weights", path))


def _run_ckpt(cb, series, key):
    stub = _StubModel()
    cb.set_model(stub)
    for e, v in enumerate(series):
        cb.on_epoch_end(e, {key: v, "lr": 1.0})
    return [p for _, p in stub.saved]


def test_checkpoint_default_saves_every_epoch():
    got = _run_ckpt(C.ModelCheckpoint("m-{epoch:02d}-{val_psnr:.2f}.hdf5"), [20.0, 19.0, 21.0], "val_psnr")
    assert got == ["m-01-20.00.hdf5", "m-02-19.00.hdf5", "m-03-21.00.hdf5"]


def test_checkpoint_best_only_auto_modes():
    for key in ("val_psnr", "val_ssim", "val_acc", "acc"):  # auto -> max
        cb = C.ModelCheckpoint("e{epoch}", monitor=key, save_best_only=True)
        assert cb.mode == "max"
        assert _run_ckpt(cb, [0.5, 0.4, 0.5, 0.7, 0.6, 0.8], key) == ["e1", "e4", "e6"]
    for key in ("val_loss", "loss"):  # auto -> min
        cb = C.ModelCheckpoint("e{epoch}", monitor=key, save_best_only=True)
        assert cb.mode == "min"
        assert _run_ckpt(cb, [0.5, 0.6, 0.5, 0.3, 0.4, 0.1], key) == ["e1", "e4", "e6"]


def test_checkpoint_explicit_mode_and_weights_only():
    cb = C.ModelCheckpoint("e{epoch}", monitor="val_psnr", save_best_only=True, mode="min", save_weights_only=True)
    stub = _StubModel()
    cb.set_model(stub)
    for e, v in enumerate([30.0, 31.0, 29.0]):
        cb.on_epoch_end(e, {"val_psnr": v})
    assert stub.saved == [("weights", "e1"), ("weights", "e3")]
    cb = C.ModelCheckpoint("e{epoch}", monitor="val_loss", save_best_only=True, mode="max")
    assert _run_ckpt(cb, [0.5, 0.6, 0.4], "val_loss") == ["e1", "e2"]


def test_checkpoint_missing_monitor_warns_and_skips():
    cb = C.ModelCheckpoint("e{epoch}", monitor="val_psnr", save_best_only=True)
    with pytest.warns(RuntimeWarning, match="val_psnr"):
        assert _run_ckpt(cb, [1.0], "val_loss") == []
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # without save_best_only the monitor is not consulted
        assert _run_ckpt(C.ModelCheckpoint("e{epoch}", monitor="val_psnr"), [1.0], "val_loss") == ["e1"]


# ---------------------------------------------------------------- Keras HDF5 training_config
def test_training_config_round_trip(tmp_path):
    from cnn_itmo_amd import keras_h5
    m = _unet()
    assert keras_h5.training_config(m)["metrics"] == ["accuracy"]
    m.compile("rmsprop", "mse", metrics=None)
    assert keras_h5.training_config(m)["metrics"] == []
    m.compile("rmsprop", "mse", metrics=["accuracy", M.psnr, "ssim"])
    assert keras_h5.training_config(m)["metrics"] == ["accuracy", "psnr", "ssim"]
    json.dumps(keras_h5.training_config(m))
    p = str(tmp_path / "m.hdf5")
    m.save(p)
    assert C.load_model(p).metrics_names == ["loss", "acc", "psnr", "ssim"]
    m.compile("rmsprop", "mse", metrics=["ssim"])
    m.save(p)
    assert C.load_model(p).metrics_names == ["loss", "ssim"]
    m.compile("rmsprop", "mse", metrics=None)  # no metrics in the file: the fallback of before
    m.save(p)
    assert C.load_model(p).metrics_names == ["loss", "acc"]


# ---------------------------------------------------------------- validation logs over ranks
def test_validation_logs_weight_ranks_by_their_frames(monkeypatch):
    """Two ranks with 3 and 5 validation frames: every log is the mean over the 8 frames."""
    m = _unet()
    m.compile("rmsprop", "mse", metrics=["accuracy", "psnr", "ssim"])
    mine = {"loss": 0.25, "acc": 0.5, "psnr": 30.0, "ssim": 0.9}
    other = {"loss": 0.125, "acc": 0.75, "psnr": 20.0, "ssim": 0.5}
    keys = ["loss", "acc", "psnr", "ssim"]
    seen = []

    def means(x, y, batch_size):
        assert batch_size == len(x) == 3
        return dict(mine), len(x)

    def allreduce(vals):
        vals = np.asarray(vals, np.float64)
        seen.append(vals.copy())
        return vals + np.array([other[k] * 5 for k in keys] + [5.0])

    monkeypatch.setattr(m, "_evaluate_means", means)
    monkeypatch.setattr(m, "_allreduce_sum", allreduce)
    logs = m._validation_logs((np.zeros((3, 32, 32, 3)), np.zeros((3, 32, 32, 3))))
    assert list(logs) == ["val_loss", "val_acc", "val_psnr", "val_ssim"]
    assert len(seen) == 1 and seen[0].shape == (5,) and seen[0][-1] == 3
    for k in keys:
        assert logs["val_" + k] == pytest.approx((mine[k] * 3 + other[k] * 5) / 8, rel=1e-15)
    # two validation steps from an iterator, one rank
    monkeypatch.setattr(m, "_allreduce_sum", lambda v: np.asarray(v, np.float64))
    it = iter([(np.zeros((3, 32, 32, 3)),) * 2] * 2)
    logs = m._validation_logs(it, 2)
    assert logs["val_psnr"] == pytest.approx(30.0) and logs["val_ssim"] == pytest.approx(0.9)
    # compiled without image metrics: the two keys of before
    m.compile("rmsprop", "mse", metrics=["accuracy"])
    assert list(m._validation_logs((np.zeros((3, 32, 32, 3)),) * 2)) == ["val_loss", "val_acc"]
