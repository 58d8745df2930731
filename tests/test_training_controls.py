"""Gradient clipping arguments and the training-control callbacks without a GPU: the optimizers'
clipnorm / clipvalue (Keras 2.2.4 base Optimizer) and their persistence, every callback driven
by a fake model over a hand-written log sequence with the expected state worked out by hand, the
C ABI's argument checks, and tests/gradclip_ref.py pinned on hand-worked vectors."""
import json
import math

import numpy as np
import pytest

import cnn_itmo_amd as C
from cnn_itmo_amd import callbacks as CB
from cnn_itmo_amd import hdf5
import gradclip_ref as GR


def _tiny():
    C.clear_session()
    return C.TinyNet(seed=3)


# ---- optimizer arguments -----------------------------------------------------------------------
@pytest.mark.parametrize("cls", [C.RMSprop, C.Adam, C.SGD])
def test_clip_arguments(cls):
    o = cls()
    assert o.clipnorm is None and o.clipvalue is None
    assert "clipnorm" not in o.get_config() and "clipvalue" not in o.get_config()
    o = cls(clipnorm=1.0)
    assert o.clipnorm == 1.0 and o.clipvalue is None
    assert o.get_config()["clipnorm"] == 1.0 and "clipvalue" not in o.get_config()
    o = cls(clipvalue=0.5)
    assert o.get_config()["clipvalue"] == 0.5 and "clipnorm" not in o.get_config()
    o = cls(clipnorm=2, clipvalue=0.25)
    assert (o.clipnorm, o.clipvalue) == (2.0, 0.25) and isinstance(o.clipnorm, float)
    for off in (0, 0.0, None):  # 0 / None: off, and not written
        o = cls(clipnorm=off, clipvalue=off)
        assert o.clipnorm is None and o.clipvalue is None and o.get_config() == cls().get_config()
    for kw in ({"clipnorm": -1.0}, {"clipvalue": -0.5}, {"clipnorm": float("nan")}):
        with pytest.raises(ValueError):
            cls(**kw)
    with pytest.raises(TypeError):
        cls(clipnorms=1.0)
    with pytest.raises(NotImplementedError):
        C.Adam(amsgrad=True, clipnorm=1.0)


def test_unclipped_optimizer_launches_nothing(monkeypatch):
    """_clip with neither option set returns before touching ops (no kernel, no allocation)."""
    from cnn_itmo_amd import ops
    monkeypatch.setattr(ops, "grad_sumsq", lambda *a, **k: pytest.fail("grad_sumsq launched"))
    monkeypatch.setattr(ops, "grad_clip", lambda *a, **k: pytest.fail("grad_clip launched"))
    for o in (C.RMSprop(), C.Adam(), C.SGD(momentum=0.9)):
        assert o._clip(object(), 0.5) is None


def test_clip_order_and_arguments(monkeypatch):
    """_clip: the norm is taken only with clipnorm; one grad_clip call carries both (norm, then value)."""
    from cnn_itmo_amd import ops
    calls = []
    monkeypatch.setattr(ops, "grad_sumsq", lambda g: calls.append(("sumsq", g)) or "S")
    monkeypatch.setattr(ops, "grad_clip", lambda *a: calls.append(("clip",) + a))
    C.Adam(clipnorm=2.0, clipvalue=0.5)._clip("G", 0.25)
    assert calls == [("sumsq", "G"), ("clip", "G", "S", 0.25, 2.0, 0.5)]
    del calls[:]
    C.SGD(clipvalue=0.5)._clip("G")
    assert calls == [("clip", "G", None, 1.0, 0.0, 0.5)]
    del calls[:]
    C.RMSprop(clipnorm=3.0)._clip("G")
    assert calls == [("sumsq", "G"), ("clip", "G", "S", 1.0, 3.0, 0.0)]


@pytest.mark.parametrize("opt", [C.Adam(lr=0.002, clipnorm=1.5), C.SGD(momentum=0.9, clipvalue=0.25),
                                 C.RMSprop(lr=0.003, clipnorm=2.0, clipvalue=0.5)], ids=["adam", "sgd", "rmsprop"])
@pytest.mark.parametrize("ext", ["h5", "npz"])
def test_clip_arguments_roundtrip_before_any_step(tmp_path, opt, ext):
    m = _tiny()
    m.compile(opt, "mse", ["accuracy"])
    p = str(tmp_path / f"m.{ext}")
    m.save(p)
    if ext == "h5":  # what a Keras reader sees
        tc = json.loads(bytes(hdf5.File(p).attrs["training_config"]).decode())
        assert tc["optimizer_config"] == {"class_name": type(opt).__name__, "config": opt.get_config()}
    C.clear_session()
    o2 = C.load_model(p).optimizer
    assert type(o2) is type(opt) and o2.get_config() == opt.get_config()
    assert (o2.clipnorm, o2.clipvalue) == (opt.clipnorm, opt.clipvalue)


def test_compile_from_config_dict():
    m = _tiny()
    m.compile({"class_name": "Adam", "config": {"lr": 0.01, "clipnorm": 1.0, "name": "ignored"}}, "mse")
    assert type(m.optimizer) is C.Adam and m.optimizer.clipnorm == 1.0 and m.optimizer.clipvalue is None
    m.compile({"class_name": "SGD", "config": {"clipvalue": 0.5, "clipnorm": 0.0}}, "mse")
    assert m.optimizer.clipvalue == 0.5 and m.optimizer.clipnorm is None
    with pytest.raises(ValueError):
        m.compile({"class_name": "SGD", "config": {"clipvalue": -0.5}}, "mse")
    with pytest.raises(NotImplementedError):
        m.compile({"class_name": "Nadam", "config": {"clipnorm": 1.0}}, "mse")


def test_exports():
    for name in ("ReduceLROnPlateau", "EarlyStopping", "LearningRateScheduler", "TerminateOnNaN"):
        assert getattr(C, name) is getattr(CB, name) and name in C.__all__


# ---- the C ABI without a GPU ---------------------------------------------------------------------
def test_gradclip_abi_argument_checks():
    """The sizing query and every CNNITMO_EINVAL of cnn_itmo.h, all refused before a device call."""
    import ctypes
    from cnn_itmo_amd import _lib
    lib = _lib.load()
    q = lib.cnnitmo_grad_sumsq_workspace_bytes
    assert q(0) == 0 and q(-5) == 0
    assert q(1) == 8 and q(8192) == 8 and q(8193) == 16 and q(11159011) == 8 * 1363
    buf = (ctypes.c_double * 8)()
    a = ctypes.addressof(buf)
    assert a % 8 == 0
    bad_sumsq = [(None, 4, a, a), (a, 0, a, a), (a + 2, 4, a, a), (a, 4, None, a), (a, 4, a, None),
                 (a, 4, a + 4, a), (a, 4, a, a + 4)]
    for g, n, ws, out in bad_sumsq:
        assert lib.cnnitmo_grad_sumsq(g, n, ws, out, None) != 0, (g, n, ws, out)
        assert lib.cnnitmo_last_error()
    bad_clip = [(None, 4, a, 1.0, 1.0, 0.0), (a, 0, a, 1.0, 1.0, 0.0), (a + 1, 4, a, 1.0, 1.0, 0.0),
                (a, 4, a, 1.0, 0.0, 0.0),            # both off
                (a, 4, a, 1.0, -1.0, -1.0),
                (a, 4, None, 1.0, 1.0, 0.0),         # clipnorm without sumsq
                (a, 4, a + 4, 1.0, 1.0, 0.0),
                (a, 4, a, 0.0, 1.0, 0.0), (a, 4, a, -0.5, 1.0, 0.0), (a, 4, a, math.inf, 1.0, 0.0),
                (a, 4, a, math.nan, 1.0, 0.0), (a, 4, a, 1.0, math.nan, 0.5), (a, 4, a, 1.0, 1.0, math.nan)]
    for g, n, s, gs, cn, cv in bad_clip:
        assert lib.cnnitmo_grad_clip(g, n, s, gs, cn, cv, None) != 0, (g, n, s, gs, cn, cv)
    with pytest.raises(_lib.CnnItmoError, match="neither clipnorm nor clipvalue"):
        _lib.call("cnnitmo_grad_clip", a, 4, a, 1.0, 0.0, 0.0, None)


# ---- the reference of the GPU tests ----------------------------------------------------------------
def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_gradclip_ref_hand_worked():
    f32 = np.float32
    assert GR.sumsq([3, 4]) == 25.0
    assert GR.sumsq([1e-20, 1.0]) == 1.0 + float(np.float64(f32(1e-20)) ** 2) == 1.0  # below half an ulp of 1
    assert GR.sumsq([2.0 ** -30] * 4 + [1.0]) == 1.0 + 2.0 ** -58  # exact in fp64
    # ||(3, 4)|| = 5 >= 1: scaled by 1/5 in fp64, rounded to fp32 once
    assert np.array_equal(_bits(GR.clip([3, 4], 25.0, clipnorm=1.0)),
                          _bits([f32(3 * (1.0 / 5.0)), f32(4 * (1.0 / 5.0))]))
    np.testing.assert_allclose(GR.clip([3, 4], 25.0, clipnorm=1.0), [0.6, 0.8], rtol=1e-7)
    # below the norm (5 < 6) and exactly at it (f = 5/5 = 1): unchanged, bit for bit
    for cn in (6.0, 5.0):
        assert np.array_equal(_bits(GR.clip([3, 4], 25.0, clipnorm=cn)), _bits([3, 4]))
    # value clipping alone; -0.0 and values inside stay
    assert np.array_equal(_bits(GR.clip([3, -4, 0.25, -0.0], None, clipvalue=0.5)), _bits([0.5, -0.5, 0.25, -0.0]))
    # norm first, then value: (3, 4) -> (0.6, 0.8) -> (0.6, 0.7); the other order would give (0.42.., 0.56..)
    assert np.array_equal(_bits(GR.clip([3, 4], 25.0, clipnorm=1.0, clipvalue=0.7)),
                          _bits([f32(3 * (1.0 / 5.0)), f32(0.7)]))
    # grad_scale 0.5: the averaged gradient is (1.5, 2), norm 2.5 -> f = 1/2.5; the buffer holds g*f =
    # (1.2, 1.6), which the update kernel halves to (0.6, 0.8), norm 1
    v = GR.clip([3, 4], 25.0, grad_scale=0.5, clipnorm=1.0)
    assert np.array_equal(_bits(v), _bits([f32(3 * (1.0 / 2.5)), f32(4 * (1.0 / 2.5))]))
    assert GR.clip([3, 4], 25.0, grad_scale=0.5, clipnorm=2.6).tolist() == [3.0, 4.0]  # 2.5 < 2.6
    # the value bound is on the averaged gradient too: |g * 0.5| <= 0.5 <=> |g| <= 1
    assert GR.clip([3, -4, 0.5], None, grad_scale=0.5, clipvalue=0.5).tolist() == [1.0, -1.0, 0.5]
    # a sum that is not finite switches norm clipping off; value clipping still applies; NaN stays NaN
    for S in (math.inf, math.nan):
        assert GR.clip([3, 4], S, clipnorm=1.0).tolist() == [3.0, 4.0]
        v = GR.clip([3, math.nan, -math.inf], S, clipnorm=1.0, clipvalue=2.0)
        assert v[0] == 2.0 and math.isnan(v[1]) and v[2] == -2.0


# ---- callbacks: a fake model and hand-written logs ---------------------------------------------------
class FakeOptimizer:
    def __init__(self, lr):
        self.lr = lr


class FakeModel:
    def __init__(self, lr=1.0):
        self.optimizer = FakeOptimizer(lr)
        self.stop_training = False
        self.weights = [np.zeros(2)]

    def get_weights(self):
        return [w.copy() for w in self.weights]

    def set_weights(self, ws):
        self.weights = [np.array(w) for w in ws]


def _run(cb, key, values, model=None, epoch_hook=None):
    """Drive cb over one log value per epoch; -> the model and per epoch (lr after, wait, logs)."""
    m = model or FakeModel()
    cb.set_model(m)
    cb.on_train_begin({})
    trace = []
    for e, v in enumerate(values):
        if epoch_hook:
            epoch_hook(m, e)
        cb.on_epoch_begin(e, {})
        logs = {} if v is None else {key: v}
        cb.on_epoch_end(e, logs)
        trace.append((m.optimizer.lr, getattr(cb, "wait", None), logs))
        if m.stop_training:
            break
    cb.on_train_end({})
    return m, trace


def test_reduce_lr_plateau_with_cooldown():
    """patience 2, cooldown 1, factor 0.5, min_delta 0, lr 1.0, val_loss 1.0 every epoch after the first
    improvement.  By hand (Keras 2.2.4: the cooldown epoch's counter is decremented BEFORE the test
    `in_cooldown`, so with cooldown = 1 the epoch after a reduction already counts):
      e0 1.0 improves (best 1.0)                   wait 0  lr 1
      e1 wait 1                                            lr 1
      e2 wait 2 >= 2 -> lr 0.5, cooldown_counter 1, wait 0
      e3 in cooldown: counter 0, wait 0; then not in cooldown: wait 1     lr 0.5
      e4 wait 2 -> lr 0.25, counter 1, wait 0
      e5 counter 0, wait 1                                 lr 0.25
      e6 0.5 improves: best 0.5, wait 0                    lr 0.25"""
    cb = C.ReduceLROnPlateau(factor=0.5, patience=2, cooldown=1, min_delta=0)
    m, tr = _run(cb, "val_loss", [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5])
    assert [t[0] for t in tr] == [1.0, 1.0, 0.5, 0.5, 0.25, 0.25, 0.25]
    assert [t[1] for t in tr] == [0, 1, 0, 1, 0, 1, 0]
    # logs['lr'] is the rate the epoch ran with (read before the reduction)
    assert [t[2]["lr"] for t in tr] == [1.0, 1.0, 1.0, 0.5, 0.5, 0.25, 0.25]
    assert cb.best == 0.5 and cb.cooldown_counter == 0


def test_reduce_lr_longer_cooldown_does_not_count():
    """cooldown 2, patience 1: after the reduction at e1 the counter is 2; e2 decrements to 1 (still
    in cooldown: wait stays 0), e3 decrements to 0 and counts (wait 1 >= 1 -> reduce again)."""
    cb = C.ReduceLROnPlateau(factor=0.5, patience=1, cooldown=2, min_delta=0)
    m, tr = _run(cb, "val_loss", [1.0, 1.0, 1.0, 1.0])
    assert [t[0] for t in tr] == [1.0, 0.5, 0.5, 0.25]


def test_reduce_lr_min_lr_then_no_change():
    """factor 0.1, patience 1, min_lr 0.05, lr 1: e1 -> 0.1, e2 -> max(0.01, 0.05) = 0.05, then lr is
    not above min_lr: nothing changes and (Keras) wait keeps counting: 1, 2."""
    cb = C.ReduceLROnPlateau(factor=0.1, patience=1, min_lr=0.05, min_delta=0)
    m, tr = _run(cb, "val_loss", [1.0] * 5)
    assert [t[0] for t in tr] == pytest.approx([1.0, 0.1, 0.05, 0.05, 0.05])
    assert tr[2][0] == 0.05
    assert [t[1] for t in tr] == [0, 0, 0, 1, 2]


def test_reduce_lr_min_delta_both_sides():
    """min mode, min_delta 0.1, patience 1, best 1.0 after e0: 0.95 (not below 0.9) is no improvement
    -> reduced; 0.85 (< 0.9) is: best 0.85; 0.75 = best - 0.1 exactly is not (strict)."""
    cb = C.ReduceLROnPlateau(factor=0.5, patience=1, min_delta=0.1)
    m, tr = _run(cb, "val_loss", [1.0, 0.95, 0.85, 0.75])
    assert [t[0] for t in tr] == [1.0, 0.5, 0.5, 0.25]
    assert cb.best == 0.85
    # max mode, the mirror image: 1.05 is not above 1.1; 1.15 is
    cb = C.ReduceLROnPlateau(monitor="score", mode="max", factor=0.5, patience=1, min_delta=0.1)
    m, tr = _run(cb, "score", [1.0, 1.05, 1.15])
    assert [t[0] for t in tr] == [1.0, 0.5, 0.5] and cb.best == 1.15


def test_auto_mode_is_the_projects_rule():
    for name, mode in [("val_psnr", "max"), ("val_ssim", "max"), ("acc", "max"), ("val_acc", "max"),
                       ("val_loss", "min"), ("loss", "min"), ("lr", "min")]:
        assert C.ReduceLROnPlateau(monitor=name).mode == mode
        assert C.EarlyStopping(monitor=name).mode == mode
        assert C.ModelCheckpoint("x", monitor=name).mode == mode
        assert CB.monitor_mode(name, "auto") == mode
    assert C.EarlyStopping(monitor="val_psnr", mode="min").mode == "min"
    for cls in (C.ReduceLROnPlateau, C.EarlyStopping):
        with pytest.warns(RuntimeWarning, match="fallback to auto"):
            assert cls(monitor="val_psnr", mode="best").mode == "max"
    with pytest.warns(RuntimeWarning, match="ModelCheckpoint mode 'best' is unknown"):  # as before
        assert C.ModelCheckpoint("x", monitor="val_loss", mode="best").mode == "min"
    # val_psnr rising is an improvement: no reduction; falling is a plateau
    cb = C.ReduceLROnPlateau(monitor="val_psnr", factor=0.5, patience=1, min_delta=0)
    m, tr = _run(cb, "val_psnr", [20.0, 21.0, 22.0, 21.5, 21.0])
    assert [t[0] for t in tr] == [1.0, 1.0, 1.0, 0.5, 0.25] and cb.best == 22.0


def test_reduce_lr_missing_key_and_arguments():
    cb = C.ReduceLROnPlateau(factor=0.5, patience=1, min_delta=0)
    m = FakeModel()
    cb.set_model(m)
    cb.on_train_begin({})
    for e in range(3):
        logs = {"loss": 1.0}
        with pytest.warns(RuntimeWarning, match="val_loss"):
            cb.on_epoch_end(e, logs)
        assert logs == {"loss": 1.0, "lr": 1.0}
    assert (m.optimizer.lr, cb.wait, cb.best, cb.cooldown_counter) == (1.0, 0, math.inf, 0)
    for f in (1.0, 1.5):
        with pytest.raises(ValueError):
            C.ReduceLROnPlateau(factor=f)
    assert C.ReduceLROnPlateau().__dict__.items() >= dict(monitor="val_loss", factor=0.1, patience=10, mode="min",
                                                          min_delta=1e-4, cooldown=0, min_lr=0).items()
    # on_train_begin resets the state of an earlier run
    cb.best, cb.wait, cb.cooldown_counter = 0.1, 5, 3
    cb.on_train_begin({})
    assert (cb.best, cb.wait, cb.cooldown_counter) == (math.inf, 0, 0)


def test_early_stopping_patience_and_min_delta():
    """patience 2, min_delta 0.1 (given negative: Keras takes |.|): 1.0 best; 0.95 no (needs < 0.9):
    wait 1; 0.85 improves: wait 0; 0.8, 0.79: wait 1, 2 -> stop at epoch 4."""
    cb = C.EarlyStopping(patience=2, min_delta=-0.1)
    m, tr = _run(cb, "val_loss", [1.0, 0.95, 0.85, 0.8, 0.79, 0.1])
    assert [t[1] for t in tr] == [0, 1, 0, 1, 2]
    assert m.stop_training and cb.stopped_epoch == 4 and cb.best == 0.85
    # patience 0 (the default): the first epoch without an improvement stops
    cb = C.EarlyStopping()
    m, tr = _run(cb, "val_loss", [1.0, 0.5, 0.5, 0.1])
    assert cb.stopped_epoch == 2 and len(tr) == 3
    assert (cb.monitor, cb.min_delta, cb.patience, cb.baseline, cb.restore_best_weights) == ("val_loss", 0, 0, None,
                                                                                             False)


def test_early_stopping_baseline():
    """baseline 0.5, patience 2, min mode: 0.7, 0.6 never beat the baseline -> stop at epoch 1; with
    0.7, 0.4 the second epoch does: best 0.4, training goes on."""
    cb = C.EarlyStopping(baseline=0.5, patience=2)
    m, tr = _run(cb, "val_loss", [0.7, 0.6, 0.1])
    assert m.stop_training and cb.stopped_epoch == 1 and cb.best == 0.5 and len(tr) == 2
    cb = C.EarlyStopping(baseline=0.5, patience=2)
    m, tr = _run(cb, "val_loss", [0.7, 0.4, 0.45])
    assert not m.stop_training and cb.best == 0.4 and [t[1] for t in tr] == [1, 0, 1]
    # max mode on val_psnr via auto: the baseline 30 dB is the value to beat
    cb = C.EarlyStopping(monitor="val_psnr", baseline=30.0, patience=1)
    m, tr = _run(cb, "val_psnr", [29.0, 31.0])
    assert m.stop_training and cb.stopped_epoch == 0


def test_early_stopping_restores_best_weights():
    """The weights are [epoch] during epoch `epoch`; val_loss 3, 1, 2, 2.5 with patience 2: best at
    epoch 1, stop at epoch 3, weights back to epoch 1's."""
    def hook(m, e):
        m.weights = [np.full(2, float(e))]

    cb = C.EarlyStopping(patience=2, restore_best_weights=True)
    m, tr = _run(cb, "val_loss", [3.0, 1.0, 2.0, 2.5, 0.0], epoch_hook=hook)
    assert m.stop_training and cb.stopped_epoch == 3 and m.weights[0].tolist() == [1.0, 1.0]
    cb = C.EarlyStopping(patience=2)  # without the option the last weights stay
    m, tr = _run(cb, "val_loss", [3.0, 1.0, 2.0, 2.5, 0.0], epoch_hook=hook)
    assert cb.stopped_epoch == 3 and m.weights[0].tolist() == [3.0, 3.0]
    # no epoch beat the baseline: nothing was kept, nothing is restored
    cb = C.EarlyStopping(patience=1, baseline=0.5, restore_best_weights=True)
    m, tr = _run(cb, "val_loss", [3.0], epoch_hook=hook)
    assert m.stop_training and m.weights[0].tolist() == [0.0, 0.0]


def test_early_stopping_missing_key():
    cb = C.EarlyStopping(patience=0)
    m = FakeModel()
    cb.set_model(m)
    cb.on_train_begin({})
    with pytest.warns(RuntimeWarning, match="val_loss"):
        cb.on_epoch_end(0, {"loss": 1.0})
    assert not m.stop_training and cb.wait == 0 and cb.best == math.inf


def test_learning_rate_scheduler():
    seen = []

    def two(epoch, lr):
        seen.append((epoch, lr))
        return lr * 0.5

    m, tr = _run(C.LearningRateScheduler(two), "loss", [1.0, 1.0, 1.0], model=FakeModel(0.8))
    assert seen == [(0, 0.8), (1, 0.4), (2, 0.2)]
    assert [t[0] for t in tr] == [0.4, 0.2, 0.1] and [t[2]["lr"] for t in tr] == [0.4, 0.2, 0.1]
    m, tr = _run(C.LearningRateScheduler(lambda epoch: 0.1 / (epoch + 1)), "loss", [1.0, 1.0])
    assert [t[0] for t in tr] == [0.1, 0.05]
    m, tr = _run(C.LearningRateScheduler(lambda epoch: np.float32(0.25)), "loss", [1.0])
    assert tr[0][0] == 0.25 and type(m.optimizer.lr) is float
    for bad in (lambda e: 1, lambda e: "0.1", lambda e: None, lambda e, lr: np.array([0.1])):
        cb = C.LearningRateScheduler(bad)
        cb.set_model(FakeModel())
        with pytest.raises(ValueError, match="should be float"):
            cb.on_epoch_begin(0, {})

    class NoLr:
        optimizer = object()

    cb = C.LearningRateScheduler(lambda e: 0.1)
    cb.set_model(NoLr())
    with pytest.raises(ValueError, match="lr"):
        cb.on_epoch_begin(0, {})


def test_terminate_on_nan(capsys):
    for bad in (math.nan, math.inf, -math.inf, np.float32("nan")):
        for hook in ("on_batch_end", "on_epoch_end"):
            cb = C.TerminateOnNaN()
            m = FakeModel()
            cb.set_model(m)
            getattr(cb, hook)(0, {"loss": 0.5})
            getattr(cb, hook)(1, {"batch": 1, "size": 2})  # this project's batch logs: no loss
            getattr(cb, hook)(1, None)
            assert not m.stop_training
            getattr(cb, hook)(2, {"loss": bad})
            assert m.stop_training
    assert "Invalid loss" in capsys.readouterr().out


def test_lr_callbacks_feed_csvlogger_and_order(tmp_path):
    """An LR callback listed before CSVLogger gives it an `lr` column (CSVLogger writes what is in logs)."""
    m = FakeModel(1.0)
    path = str(tmp_path / "log.csv")
    cbs = CB.CallbackList([C.ReduceLROnPlateau(monitor="loss", factor=0.5, patience=1, min_delta=0),
                           C.CSVLogger(path)], m)
    cbs.call("on_train_begin", {})
    for e, v in enumerate([1.0, 1.0, 1.0]):
        cbs.call("on_epoch_end", e, {"loss": v})
    with open(path) as f:
        rows = [ln.split(",") for ln in f.read().split()]
    assert rows[0] == ["epoch", "loss", "lr"]
    assert [float(r[2]) for r in rows[1:]] == [1.0, 1.0, 0.5] and m.optimizer.lr == 0.25
