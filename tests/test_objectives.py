"""Selectable losses and optimizers without a GPU: compile()'s parsing and failure
behaviour, persistence of an Adam / SGD model before any step, the C ABI's argument checks
of cnnitmo_head_fwd_bwd_loss, and the reference module's own consistency
(tests/ref_objectives.py: derivatives against finite differences, ln cosh, the BCE forms)."""
import json
import os

import numpy as np
import pytest

import cnn_itmo_amd as C
from cnn_itmo_amd import hdf5
import ref_objectives as RO

ALIASES = {"mse": "mse", "MSE": "mse", "mean_squared_error": "mse",
           "mae": "mae", "MAE": "mae", "mean_absolute_error": "mae",
           "logcosh": "logcosh",
           "msle": "msle", "MSLE": "msle", "mean_squared_logarithmic_error": "msle",
           "binary_crossentropy": "binary_crossentropy"}


def _tiny():
    C.clear_session()
    return C.TinyNet(seed=3)


@pytest.mark.parametrize("name,canon", sorted(ALIASES.items()))
def test_loss_aliases(name, canon):
    m = _tiny()
    m.compile("rmsprop", name, ["accuracy"])
    assert m.loss == canon
    from cnn_itmo_amd import _lib
    assert _lib.LOSSES[canon] == RO.LOSS_IDS[canon]


@pytest.mark.parametrize("name,cls", [("rmsprop", C.RMSprop), ("RMSprop", C.RMSprop), ("adam", C.Adam),
                                      ("Adam", C.Adam), ("sgd", C.SGD), ("SGD", C.SGD)])
def test_optimizer_strings(name, cls):
    m = _tiny()
    m.compile(name, "mse")
    assert type(m.optimizer) is cls


def test_optimizer_defaults_and_learning_rate():
    a = C.Adam()
    assert (a.lr, a.beta_1, a.beta_2, a.epsilon, a.decay, a.slots) == (0.001, 0.9, 0.999, 1e-7, 0.0, 2)
    s = C.SGD()
    assert (s.lr, s.momentum, s.decay, s.nesterov, s.slots) == (0.01, 0.0, 0.0, False, 1)
    assert C.Adam(learning_rate=0.5).lr == 0.5 and C.SGD(learning_rate=0.25).lr == 0.25
    r = C.RMSprop(decay=0.1)  # no longer refused
    assert r.decay == 0.1 and r.lr_at(0) == r.lr and r.lr_at(10) == pytest.approx(r.lr / 2)
    # Keras' bias correction, t = iterations + 1
    assert a.lr_t(0) == pytest.approx(0.001 * np.sqrt(1 - 0.999) / (1 - 0.9))
    assert C.Adam(decay=1.0).lr_t(3) == pytest.approx(0.001 / 4 * np.sqrt(1 - 0.999 ** 4) / (1 - 0.9 ** 4))


def test_refused_arguments_leave_the_model_as_it_was():
    with pytest.raises(NotImplementedError):
        C.Adam(amsgrad=True)
    m = _tiny()
    m.compile(C.SGD(lr=0.5, momentum=0.9), "mae", ["accuracy", "psnr"])
    before = (m.optimizer, m.loss, list(m.metrics_names), list(m.image_metrics), m.dtype)
    for args in [("adagrad", "mse"), ("adam", "huber"), ("adam", "kullback_leibler_divergence"),
                 ("adam", None), ("adam", "mse", ["mae"]), ({"class_name": "Nadam", "config": {}}, "mse")]:
        with pytest.raises(NotImplementedError):
            m.compile(*args)
        assert (m.optimizer, m.loss, m.metrics_names, m.image_metrics, m.dtype) == before
    with pytest.raises(ValueError):
        m.compile("adam", "mse", dtype="float16")
    assert (m.optimizer, m.loss, m.metrics_names, m.image_metrics, m.dtype) == before


@pytest.mark.parametrize("opt", [C.Adam(lr=0.002, beta_1=0.8, beta_2=0.99, epsilon=1e-6, decay=0.01),
                                 C.SGD(lr=0.05, momentum=0.9, decay=0.02, nesterov=True),
                                 C.RMSprop(lr=0.003, rho=0.8, decay=0.1)], ids=["adam", "sgd", "rmsprop"])
@pytest.mark.parametrize("ext", ["h5", "npz"])
def test_compiled_model_roundtrip_before_any_step(tmp_path, opt, ext):
    m = _tiny()
    m.compile(opt, "mean_absolute_error", ["accuracy"])
    p = str(tmp_path / f"m.{ext}")
    m.save(p)
    if ext == "h5":  # what a Keras reader sees
        tc = json.loads(bytes(hdf5.File(p).attrs["training_config"]).decode())
        assert tc["optimizer_config"] == {"class_name": type(opt).__name__, "config": opt.get_config()}
        assert tc["loss"] == "mae" and tc["metrics"] == ["accuracy"]
        assert "optimizer_weights" not in hdf5.File(p)  # no state before the first step
    C.clear_session()
    m2 = C.load_model(p)
    assert type(m2.optimizer) is type(opt) and m2.optimizer.get_config() == opt.get_config()
    assert m2.loss == "mae" and m2.metrics_names == ["loss", "acc"] and m2.iterations == 0


def _write_state(tmp_path, cls, with_vhats=True):
    """An .h5 with optimizer state, written without an engine (the pending-state path)."""
    m = _tiny()
    m.compile(cls(), "logcosh")
    rng = np.random.default_rng(5)
    slots = [{k: rng.uniform(size=v.shape).astype(np.float32) for k, v in m.named_weights().items()}
             for _ in range(m.optimizer.slots)]
    m._pending_accum = ("named", slots[0], 7)
    m._pending_slots = slots[1:]
    m._pending_iterations = 7
    p = str(tmp_path / "state.h5")
    m.save(p)
    return m, slots, p


@pytest.mark.parametrize("cls", [C.Adam, C.SGD, C.RMSprop])
def test_optimizer_weights_follow_keras_order(tmp_path, cls):
    m, slots, p = _write_state(tmp_path, cls)
    og = hdf5.File(p)["optimizer_weights"]
    names = [bytes(n).decode() for n in og.attrs["weight_names"]]
    vals = [og[n].read() for n in names]
    nt = len(m.named_weights())
    keras = m.get_weights()  # Keras layouts, model order (TinyNet: every weight trainable)
    lead = 0 if cls is C.RMSprop else 1
    assert len(vals) == lead + nt * m.optimizer.slots + (nt if cls is C.Adam else 0)
    if lead:
        assert np.asarray(vals[0]).size == 1 and int(np.asarray(vals[0]).reshape(-1)[0]) == 7
    for s in range(m.optimizer.slots):
        for v, w in zip(vals[lead + s * nt:lead + (s + 1) * nt], keras):
            assert v.shape == w.shape and v.dtype == np.float32
    if cls is C.Adam:  # the non-amsgrad vhats
        assert all(v.shape == (1,) and not v.any() for v in vals[lead + 2 * nt:])
    C.clear_session()
    m2 = C.load_model(p)
    assert m2.iterations == (0 if cls is C.RMSprop else 7) and m2.loss == "logcosh"
    got = m2.named_slots()
    assert len(got) == len(slots)
    for a, b in zip(slots, got):
        assert a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(m2.named_accumulators()["conv2d_1/kernel"], slots[0]["conv2d_1/kernel"])


def test_adam_file_without_vhat_placeholders_loads(tmp_path):
    """The reader goes by order and shape: an Adam file that carries [iterations] + ms + vs
    alone (no placeholders) and other variable names restores the same state."""
    m, slots, p = _write_state(tmp_path, C.Adam)
    f = hdf5.File(p)
    w = hdf5.Writer()
    for k in ("keras_version", "backend", "model_config", "training_config"):
        w.attrs[k] = bytes(f.attrs[k]).decode()
    mw = w.create_group("model_weights")
    src = f["model_weights"]
    for k in ("layer_names", "backend", "keras_version"):
        v = src.attrs[k]
        mw.attrs[k] = [bytes(x).decode() for x in v] if k == "layer_names" else bytes(v).decode()
    for ln in [bytes(x).decode() for x in src.attrs["layer_names"]]:
        g = mw.create_group(ln)
        wn = [bytes(x).decode() for x in src[ln].attrs["weight_names"]]
        g.attrs["weight_names"] = wn if wn else np.zeros((0,), dtype="S1")
        for n in wn:
            g.create_dataset(n, src[ln][n].read())
    og = f["optimizer_weights"]
    names = [bytes(n).decode() for n in og.attrs["weight_names"]]
    nt = len(m.named_weights())
    keep = names[:1 + 2 * nt]
    og2 = w.create_group("optimizer_weights")
    new = [f"some/other/name_{i}:0" for i in range(len(keep))]
    for n, nn in zip(keep, new):
        og2.create_dataset(nn, og[n].read())
    og2.attrs["weight_names"] = new
    p2 = str(tmp_path / "bare.h5")
    w.save(p2)
    C.clear_session()
    m2 = C.load_model(p2)
    assert m2.iterations == 7
    for a, b in zip(slots, m2.named_slots()):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_npz_from_before_the_selectable_optimizers_loads(tmp_path):
    """Today's .npz files: opt/accum, opt/step and a 3-value opt/hyper, no class or loss."""
    m = _tiny()
    arrays = {"__config__": np.frombuffer(json.dumps(m.get_config()).encode(), np.uint8)}
    for k, v in m.named_weights().items():
        arrays["w/" + k] = v
    arrays["opt/accum"] = np.arange(8, dtype=np.float32)
    arrays["opt/step"] = np.array([4])
    arrays["opt/hyper"] = np.array([0.002, 0.8, 1e-6])
    p = str(tmp_path / "old.npz")
    np.savez(p, **arrays)
    C.clear_session()
    m2 = C.load_model(p)
    o = m2.optimizer
    assert type(o) is C.RMSprop and (o.lr, o.rho, o.epsilon, o.decay) == (0.002, 0.8, 1e-6, 0.0)
    assert m2.loss == "mse" and m2.iterations == 4 and m2._pending_slots == []


# ---- C ABI argument checks (no launch is reached) -------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from cnn_itmo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _head_call(lib, loss, dx, g3):
    import ctypes
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    return lib.cnnitmo_head_fwd_bwd_loss(loss, 0, a, 1, 1, 1, 1, 16, a, a, None, None, a, a if dx else None,
                                         a if g3 else None, a, 0.0, None)


@pytest.mark.parametrize("loss", [5, -1])
def test_unknown_loss_is_einval(lib, loss):
    assert _head_call(lib, loss, True, False) < 0
    assert b"unknown loss" in lib.cnnitmo_last_error()


@pytest.mark.parametrize("dx,g3", [(True, True), (False, False)])
def test_dx_g3_pair_is_einval(lib, dx, g3):
    assert _head_call(lib, 1, dx, g3) < 0
    assert b"exactly one of dx and g3" in lib.cnnitmo_last_error()


# ---- the reference module's own consistency ----------------------------------------------------
@pytest.mark.parametrize("name", RO.LOSSES)
def test_reference_derivative_matches_finite_difference(name):
    rng = np.random.default_rng(11)
    z = rng.uniform(-6, 6, 4000)
    t = rng.uniform(0, 1, 4000)
    if name == "mae":  # away from the kink of |y - t|
        t = RO.mae_safe_target(RO.sigmoid(z), t)
    # central difference in fp64: truncation h^2 |l'''| / 6 ~ 1e-11; rounding, worst for
    # ln(1 - y) at z = 6 (1 - y = 2.5e-3): 2 * ulp(1) / 2.5e-3 / (2 h) ~ 4e-9 -- both below 1e-8
    h = 1e-5
    fd =(RO.term(name, RO.sigmoid(z + h), t) - RO.term(name, RO.sigmoid(z - h), t)) / (2 * h)
    np.testing.assert_allclose(RO.dterm_dz(name, RO.sigmoid(z), t), fd, rtol=0, atol=1e-8)
    y = RO.sigmoid(z)
    assert RO.loss(name, y, t) == pytest.approx(float(RO.term(name, y, t).mean()))
    np.testing.assert_array_equal(RO.grad_z(name, y, t), RO.dterm_dz(name, y, t) / y.size)


def test_reference_logcosh_and_bce_forms():
    x = np.linspace(-1, 1, 2001)
    np.testing.assert_allclose(RO.term("logcosh", x, np.zeros_like(x)), np.log(np.cosh(x)), rtol=0, atol=1e-15)
    rng = np.random.default_rng(12)
    z = rng.uniform(-10, 10, 4000)
    t = rng.uniform(0, 1, 4000)
    # the logit form the kernel uses == -(t ln y + (1-t) ln(1-y)) == Keras' clipped form on |z| < 10
    # (fp64 rounding of 1 - y at z = 10, where 1 - y = 4.5e-5: ulp(1) / 4.5e-5 = 2.4e-12 per logarithm)
    np.testing.assert_allclose(RO.bce_logit(z, t), RO.term("binary_crossentropy", RO.sigmoid(z), t), rtol=0, atol=1e-11)
    np.testing.assert_allclose(RO.bce_logit(z, t), RO.bce_keras(z, t), rtol=0, atol=1e-9)


@pytest.mark.parametrize("C_,H,W", [(64, 8, 16), (16, 5, 13), (128, 6, 11), (256, 4, 9)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mae_target_construction_holds_for_the_gpu_cases(dt, C_, H, W):
    """The condition tests/test_gpu_losses.py puts on its MAE targets, checked here for the
    same seeds: no |y_ref - t| below 1e-3 after the float32 rounding of the target."""
    import test_gpu_losses as G
    case = G.head_case(dt, C_, H, W, "mae")
    assert float(np.abs(case["yref"] - case["t"]).min()) >= 1e-3
    assert case["t"].min() >= 0.0 and case["t"].max() <= 1.0
    np.testing.assert_array_equal(case["t"], case["t"].astype(np.float32).astype(np.float64))
