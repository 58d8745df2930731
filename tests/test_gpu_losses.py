"""The selectable training objectives on the GPU: cnnitmo_head_fwd_bwd_loss per loss against
the fp64 reference (tests/ref_objectives.py) under test_gpu_ops.test_head's rules, the whole
U-Net's 74 gradients per loss against the oracle with its loss patched, the Adam / SGD
kernels, the engine's `iterations` wiring and the front end (compile, fit, evaluate,
save / load_model, set_dtype)."""
import contextlib
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import unet_ref as R  # noqa: E402
import ref_objectives as RO  # noqa: E402
from tests.test_gpu_ops import DT, TDT, close, dev, host, rnd  # noqa: E402

NEW_LOSSES = ("mae", "logcosh", "msle", "binary_crossentropy")
HEAD_SHAPES = [(64, 8, 16),
               # head2_kernel at 2 and 16 lanes per pixel, ragged 64-pixel groups
               (16, 5, 13), (128, 6, 11),
               # head_kernel (the fallback)
               (256, 4, 9)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_itmo_amd import _lib as L
    L.load()


def cu(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def head_case(dt, C, H, W, loss, folded=False):
    """Seeded inputs of one head case (host only): x rounded through the device dtype, the
    fp64 prediction of those values and the float32-exact target; for 'mae' the target keeps
    1e-3 away from the reference prediction (RO.mae_safe_target)."""
    rng = np.random.default_rng(6 + C)
    N, Hv = 2, H - 1
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    if folded:  # x holds r = relu(conv); the head's input is r*s + h
        x = np.maximum(x, 0)
    w = (rng.standard_normal((3, C)) * 0.2).astype(np.float32)
    b = rng.standard_normal(3).astype(np.float32)
    t = rng.uniform(size=(N, Hv, W, 3)).astype(np.float32).astype(np.float64)
    s = h = None
    xin = rnd(x, dt)
    if folded:
        s = rng.uniform(0.3, 2.0, C).astype(np.float32)
        h = rng.standard_normal(C).astype(np.float32)
        xin = xin * s + h
    xin = xin[:, :Hv]
    yref = RO.sigmoid(xin @ w.T.astype(np.float64) + b)
    if loss == "mae":
        t = RO.mae_safe_target(yref, t)
    return dict(N=N, Hv=Hv, x=x, w=w, b=b, t=t, s=s, h=h, xin=xin, yref=yref)


def _check_head(dt, C, H, W, loss, folded):
    from cnn_itmo_amd import ops
    c = head_case(dt, C, H, W, loss, folded)
    N, Hv, w, t, yref, xin = c["N"], c["Hv"], c["w"], c["t"], c["yref"], c["xin"]
    if loss == "mae":  # a condition on the inputs, not a tolerance
        assert float(np.abs(yref - t).min()) >= 1e-3
    d, lid = DT[dt], RO.LOSS_IDS[loss]
    aff = (cu(c["s"]), cu(c["h"])) if folded else None
    xv = ops.View(dev(c["x"], dt).reshape(-1), N, H, W, C, C)
    rows = ops.head_rows(N * H * W)
    numel = N * Hv * W * 3
    dz = RO.grad_z(loss, yref, t)
    dx_ref = np.zeros((N, H, W, C))
    dx_ref[:, :Hv] = dz @ w.astype(np.float64)
    g3_ref = np.zeros((N, H, W, 3))
    g3_ref[:, :Hv] = dz
    # dx form
    part = torch.empty(rows, 5 + 3 * C, device="cuda")
    dx = torch.empty(N * H * W * C, dtype=TDT[dt], device="cuda")
    ops.head_fwd_bwd_loss(lid, d, xv, Hv, cu(w), cu(c["b"]), cu(t), part, dx=dx, aff=aff)
    la, dw, db = torch.empty(2, device="cuda"), torch.empty(3, C, device="cuda"), torch.empty(3, device="cuda")
    ops.head_finalize(part, rows, C, numel, la, dw, db, aff=aff)
    # g3 form: every row, the zero rows at and beyond Hv included
    g3 = torch.full((N * H * W * 3,), 7.0, device="cuda")
    part3 = torch.empty(rows, 5 + 3 * C, device="cuda")
    ops.head_fwd_bwd_loss(lid, d, xv, Hv, cu(w), cu(c["b"]), cu(t), part3, g3=g3, aff=aff)
    la3, dw3, db3 = torch.empty(2, device="cuda"), torch.empty(3, C, device="cuda"), torch.empty(3, device="cuda")
    ops.head_finalize(part3, rows, C, numel, la3, dw3, db3, aff=aff)
    torch.cuda.synchronize()
    print(f"{loss} {dt} C={C}: loss {la[0].item():.8f} ref {RO.loss(loss, yref, t):.8f} "
          f"dx max-abs {np.abs(host(dx).reshape(dx_ref.shape) - dx_ref).max():.3e}")
    assert abs(la[0].item() - RO.loss(loss, yref, t)) < 1e-5
    assert abs(la[1].item() - R.categorical_accuracy(t, yref)) < 1e-6
    k = 1e3 if folded else 1.0  # (test_head_folded scales dw and db, test_head does not)
    close(host(dw) * k, dz.reshape(-1, 3).T @ xin.reshape(-1, C) * k, "f32", "head dw")
    close(host(db) * k, dz.reshape(-1, 3).sum(0) * k, "f32", "head db")
    close(host(dx).reshape(dx_ref.shape) * 1e3, dx_ref * 1e3, dt, "head dx")
    close(g3.cpu().numpy().reshape(g3_ref.shape) * 1e3, g3_ref * 1e3, "f32", "head g3")
    assert np.array_equal(la3.cpu().numpy(), la.cpu().numpy())
    assert np.array_equal(host(dw3), host(dw)) and np.array_equal(host(db3), host(db))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,H,W", HEAD_SHAPES)
@pytest.mark.parametrize("loss", NEW_LOSSES)
def test_head_loss(loss, C, H, W, dt):
    _check_head(dt, C, H, W, loss, folded=False)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("loss", NEW_LOSSES)
def test_head_loss_folded(loss, dt):
    """The folded-BN input (x holds r, the head sees r*s + h), as test_head_folded: (2,7,8,16,64)."""
    _check_head(dt, 64, 8, 16, loss, folded=True)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,H,W", [(64, 8, 16), (256, 4, 9)])
def test_head_loss_mse_is_head_fwd_bwd(dt, C, H, W):
    """cnnitmo_head_fwd_bwd_loss(MSE) == cnnitmo_head_fwd_bwd bit for bit (dx and part)."""
    from cnn_itmo_amd import ops
    c = head_case(dt, C, H, W, "mse")
    N, Hv = c["N"], c["Hv"]
    xv = ops.View(dev(c["x"], dt).reshape(-1), N, H, W, C, C)
    rows = ops.head_rows(N * H * W)
    out = []
    for new in (False, True):
        part = torch.zeros(rows, 5 + 3 * C, device="cuda")
        dx = torch.zeros(N * H * W * C, dtype=TDT[dt], device="cuda")
        if new:
            ops.head_fwd_bwd_loss(RO.LOSS_IDS["mse"], DT[dt], xv, Hv, cu(c["w"]), cu(c["b"]), cu(c["t"]), part, dx=dx)
        else:
            ops.head_fwd_bwd(DT[dt], xv, Hv, cu(c["w"]), cu(c["b"]), cu(c["t"]), dx, part)
        torch.cuda.synchronize()
        out.append((dx, part))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- whole network ---------------------------------------------------------------------------
def build_unet(size, dtype, seed=1):
    import cnn_itmo_amd as C
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=size, dtype=dtype, seed=seed)
    return m


def _rel_l2(g, r):
    return float(np.linalg.norm(g - r)) / max(1e-12, float(np.linalg.norm(r)))


_NET_REF = {}  # loss -> the fp64 reference of the case (computed once, read only)


def _net_reference(loss, P, x, seed):
    """(target, loss, gradients) of the fp64 oracle for `loss`; R's loss is patched by the caller."""
    if loss not in _NET_REF:
        net = R.UNetRef(P)
        y = net.forward(x, training=True, seed=seed)
        t = np.clip(x ** 2.2 * 1.2, 0, 1).astype(np.float32).astype(np.float64)
        if loss == "mae":
            t = RO.mae_safe_target(y, t)
        ref_loss, _, rg = net.backward(t)
        _NET_REF[loss] = (t, ref_loss, rg, {k: v.copy() for k, v in P.items()})
    t, ref_loss, rg, P0 = _NET_REF[loss]
    assert all(np.array_equal(P0[k], P[k]) for k in P0)  # the same weights for both dtypes
    return t, ref_loss, rg


@pytest.mark.parametrize("dtype,loss", [("float32", k) for k in NEW_LOSSES] +
                         [("bfloat16", "logcosh"), ("bfloat16", "binary_crossentropy")])
def test_unet_all_74_grads_per_loss(dtype, loss, monkeypatch):
    """U-Net (64,64,3) b2, train_step(apply=False): the loss and all 74 gradients against
    UNetRef with its loss patched, under test_unet_train_step_all_74_grads_128's rule:
      fp32: rel-L2 <= max(1e-4, 3x the deviation of numpy's own float32 run of the oracle);
      bf16: rel-L2 <= max(3x the deviation of the bf16-storage run, 2e-3);
      loss: rel <= max(3x the same floor run's loss deviation, 1e-6 fp32 / 5e-3 bf16).
    MAE runs in fp32 only, on a target kept 1e-3 away from the reference prediction: bf16
    activation rounding moves y by far more than any usable margin (kernel-level there)."""
    from test_gpu_model import randomize_bn
    RO.patch_oracle(monkeypatch, R, loss)
    rng = np.random.default_rng(21)
    m = build_unet((64, 64, 3), dtype, seed=7)
    P = randomize_bn(m, rng)
    x = rng.integers(0, 256, size=(2, 64, 64, 3)) / 255.0
    seed = 9
    t, ref_loss, rg = _net_reference(loss, P, x, seed)
    m.compile(m.optimizer, loss, ["accuracy"])
    eng = m._engine()
    la = eng.train_step(torch.tensor(x, dtype=torch.float32).cuda(), torch.tensor(t, dtype=torch.float32).cuda(),
                        seed=seed, apply=False).cpu().numpy()
    grads = eng.get_grads()
    assert eng.iterations == 0 and eng.step == 1
    assert len(rg) == 74 and set(rg) == set(grads)
    if dtype == "float32":
        em = R.UNetRef(P, np.float32)
        em.forward(x.astype(np.float32), training=True, seed=seed)
        eloss, _, eg = em.backward(t.astype(np.float32))
    else:
        em = R.UNetRef(P, store=R.round_bf16)
        em.forward(x, training=True, seed=seed)
        eloss, _, eg = em.backward(t)
    err = {k: _rel_l2(grads[k].reshape(rg[k].shape), rg[k]) for k in rg}
    floor = {k: _rel_l2(eg[k], rg[k]) for k in rg}
    lerr, lfloor = abs(la[0] - ref_loss) / ref_loss, abs(eloss - ref_loss) / ref_loss
    worst = max(rg, key=lambda k: err[k] / max(floor[k], 1e-12))
    print(f"{dtype} {loss}: loss rel {lerr:.2e} (floor {lfloor:.2e}); worst gradient {worst} "
          f"gpu {err[worst]:.2e} floor {floor[worst]:.2e}; max gpu rel-L2 {max(err.values()):.2e}")
    if dtype == "float32":
        assert lerr <= max(3 * lfloor, 1e-6), (lerr, lfloor)
        bad = {k: (err[k], floor[k]) for k in rg if err[k] > max(1e-4, 3 * floor[k])}
    else:
        assert lerr <= max(3 * lfloor, 5e-3), (lerr, lfloor)
        bad = {k: (err[k], floor[k]) for k in rg if err[k] > max(3 * floor[k], 2e-3)}
    assert not bad, bad


# ---- optimizer kernels -------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["adam", "sgd", "sgd_momentum", "sgd_nesterov"])
def test_adam_sgd_kernels(case):
    """As test_rmsprop: n = 1003 (scalar tail), grad_scale 0.5, three consecutive steps; p and
    every slot against fp64 numpy at atol 1e-6."""
    from cnn_itmo_amd import ops
    rng = np.random.default_rng(7)
    n = 1003
    p = rng.standard_normal(n)
    slots = [rng.standard_normal(n) * 0.1, rng.uniform(size=n)] if case == "adam" else [rng.standard_normal(n) * 0.1]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).cuda()  # noqa: E731
    pt, st = f32(p), [f32(s) for s in slots]
    p, slots = pt.double().cpu().numpy(), [s.double().cpu().numpy() for s in st]
    kw = {"sgd": {}, "sgd_momentum": {"momentum": 0.9}, "sgd_nesterov": {"momentum": 0.9, "nesterov": True}}
    for it in range(3):
        gt = f32(rng.standard_normal(n))
        g = gt.double().cpu().numpy() * 0.5
        if case == "adam":
            lr_t = 1e-3 * np.sqrt(1 - 0.999 ** (it + 1)) / (1 - 0.9 ** (it + 1))
            ops.adam(pt, gt, st[0], st[1], lr_t, 0.9, 0.999, 1e-7, grad_scale=0.5)
            p, slots[0], slots[1] = RO.adam(p, g, slots[0], slots[1], it)
        else:
            ops.sgd(pt, gt, st[0], 1e-2, grad_scale=0.5, **kw[case])
            p, slots[0] = RO.sgd(p, g, slots[0], **kw[case])
        torch.cuda.synchronize()
        np.testing.assert_allclose(pt.cpu().numpy(), p, atol=1e-6, err_msg=f"p, step {it}")
        for i, (a, b) in enumerate(zip(st, slots)):
            np.testing.assert_allclose(a.cpu().numpy(), b, atol=1e-6, err_msg=f"slot {i}, step {it}")


# ---- engine wiring ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["adam", "sgd_momentum", "rmsprop_decay"])
def test_engine_updates_follow_iterations(case):
    """TinyNet (no BN, no Dropout): twice, the gradients from train_step(apply=False), then a
    step on the same batch; the parameters equal the fp64 rule applied to those gradients
    (atol 1e-6).  The apply=False calls advance `step` but not `iterations`, so an lr_t or a
    decay taken from `step` shows."""
    import cnn_itmo_amd as C
    opt = {"adam": C.Adam(), "sgd_momentum": C.SGD(momentum=0.9), "rmsprop_decay": C.RMSprop(decay=0.1)}[case]
    C.clear_session()
    m = C.TinyNet(seed=2)
    m.compile(opt, "mse", ["accuracy"])
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.uniform(size=(2, 64, 64, 3)), dtype=torch.float32).cuda()
    t = torch.tensor(rng.uniform(size=(2, 64, 64, 3)), dtype=torch.float32).cuda()
    eng = m._engine()
    P = {k: v.astype(np.float64) for k, v in m.named_weights().items()}
    S = [{k: np.zeros_like(v) for k, v in P.items()} for _ in range(opt.slots)]
    for it in range(2):
        eng.train_step(x, t, optimizer=opt, apply=False)
        assert eng.iterations == it and eng.step == 2 * it + 1
        g = {k: v.astype(np.float64) for k, v in eng.get_grads().items()}
        eng.train_step(x, t, optimizer=opt)
        assert eng.iterations == it + 1 and eng.step == 2 * it + 2
        after = m.named_weights()
        for k in P:
            gk = g[k].reshape(P[k].shape)
            if case == "adam":
                exp, S[0][k], S[1][k] = RO.adam(P[k], gk, S[0][k], S[1][k], it)
            elif case == "sgd_momentum":
                exp, S[0][k] = RO.sgd(P[k], gk, S[0][k], momentum=0.9)
            else:
                exp, S[0][k] = RO.rmsprop(P[k], gk, S[0][k], it, decay=0.1)
            np.testing.assert_allclose(after[k], exp, atol=1e-6, err_msg=f"{k}, update {it}")
        P = {k: v.astype(np.float64) for k, v in after.items()}
        for s, got in zip(S, m.named_slots()):
            for k in s:
                np.testing.assert_allclose(got[k], s[k], atol=1e-6, err_msg=f"slot of {k}, update {it}")


def test_recompile_with_another_optimizer_starts_fresh():
    """Slots and iterations belong to the optimizer: compiling another class zeroes them (a
    new Keras optimizer starts from nothing), compiling the same class keeps them."""
    import cnn_itmo_amd as C
    C.clear_session()
    m = C.TinyNet(seed=2)
    x, t = np.full((1, 64, 64, 3), 0.25), np.full((1, 64, 64, 3), 0.5)
    m.train_on_batch(x, t)
    m.compile(C.RMSprop(lr=1e-4), "mse", ["accuracy"])
    assert m.iterations == 1 and float(m.engine.accum.abs().max()) > 0
    m.compile("adam", "mse", ["accuracy"])
    assert m.iterations == 0 and all(float(s.abs().max()) == 0 for s in m.engine.slots)
    m.train_on_batch(x, t)
    assert m.iterations == 1 and len(m.engine.slots) == 2 and float(m.engine.slots[1].abs().max()) > 0


# ---- front end -------------------------------------------------------------------------------
def _pairs(seed, n=4):
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, 64, 64, 3))
    return x, np.clip(x * 0.8 + 0.1, 0, 1)


def test_compile_adam_mae_fit_and_evaluate():
    m = build_unet((64, 64, 3), "float32", seed=10)
    m.compile("adam", "mae", ["accuracy"])
    x, t = _pairs(9)

    def gen():
        while True:
            yield x[:2], t[:2]
            yield x[2:], t[2:]
    h = m.fit_generator(gen(), steps_per_epoch=10, epochs=3, verbose=0)
    losses = h.history["loss"]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert m.iterations == 30
    ev = m.evaluate(x, t, batch_size=2)
    assert abs(ev[0] - float(np.abs(m.predict(x).astype(np.float64) - t).mean())) < 1e-5


@pytest.mark.parametrize("ext", ["h5", "npz"])
def test_save_load_continues_bitwise(tmp_path, ext):
    """Two Adam/MAE steps, save, load_model: one more step from the loaded model equals one
    more step from the original bit for bit (slots, iterations, loss, hyper-parameters and
    the Dropout seed all restored)."""
    import cnn_itmo_amd as C
    m = build_unet((64, 64, 3), "float32", seed=11)
    m.compile(C.Adam(lr=2e-3, beta_1=0.8), "mae", ["accuracy"])
    x, t = _pairs(13, 2)
    for _ in range(2):
        m.train_on_batch(x, t)
    p = str(tmp_path / f"ck.{ext}")
    m.save(p)
    la = m.train_on_batch(x, t)
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m2 = C.load_model(p)
    assert type(m2.optimizer) is C.Adam and m2.optimizer.get_config() == m.optimizer.get_config()
    assert m2.loss == "mae" and m2.iterations == 2
    la2 = m2.train_on_batch(x, t)
    assert la2 == la and m2.iterations == 3 and m2.engine.step == 3
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    for sa, sb in zip(m.named_slots(), m2.named_slots()):
        assert all(np.array_equal(v, w) for v, w in zip(sa.values(), sb.values()))


def test_set_dtype_keeps_slots_and_iterations():
    m = build_unet((64, 64, 3), "float32", seed=12)
    m.compile("adam", "logcosh", ["accuracy"])
    x, t = _pairs(14, 2)
    for _ in range(2):
        m.train_on_batch(x, t)
    before = [s.clone() for s in m.engine.slots]
    assert len(before) == 2 and all(float(s.abs().max()) > 0 for s in before)
    m.set_dtype("bfloat16")
    eng = m._engine()
    assert eng.dtype_name == "bfloat16" and eng.iterations == 2 and eng.step == 2
    assert len(eng.slots) == 2 and all(torch.equal(a, b) for a, b in zip(eng.slots, before))
    la = m.train_on_batch(x, t)
    assert np.isfinite(la[0]) and m.iterations == 3
