"""The DSSIM training loss on the GPU (csrc/dssim.hip, cnnitmo_head_fwd_bwd_given, the engine
and the front end) against the numpy float64 reference (tests/dssim_ref.py).

Kernel bounds, per image:
  |ssim - ref| <= 1e-6, the project's metric bound (tests/test_gpu_metrics.py);
  B and L: relative error <= 1e-9 (fp64 sums of <= 2e5 terms);
  |dy - ref| <= 1e-6 * max|ref dy|: 16x the 2^-24 rounding of the fp32 output.
"""
import contextlib
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cnn_itmo_amd as C  # noqa: E402
from oracle import unet_ref as R  # noqa: E402
import dssim_ref as DR  # noqa: E402
import metrics_ref as MR  # noqa: E402
import ref_objectives as RO  # noqa: E402
from arena import Arena, poison_count  # noqa: E402
from tests.test_gpu_ops import DT, TDT, close, dev, host  # noqa: E402
from tests.test_gpu_losses import HEAD_SHAPES, _rel_l2, build_unet, cu, head_case  # noqa: E402

LOSSES = [(None, 1.0), ("mae", 0.84), ("mse", 0.84)]
LOSS_IDS = ["none", "mae", "mse"]
SSIM_TOL, SUM_RTOL, DY_TOL = 1e-6, 1e-9, 1e-6

# (2,11,11): one window; (1,12,27): 3w % 4 != 0, the scalar path; (1,26,26) / (1,27,27): exactly
# one 16 x 48 map tile and one element past it both ways; (1,43,60): the vector path, several
# tiles; (3,45,83): one noise level per image; two long thin ones; a nearly flat pair (1/B2 ~ 1e3);
# (1,12,28) on a view one float off a 16-byte boundary (3w % 4 == 0, still the scalar path)
KERNEL_CASES = ["2x11x11", "1x12x27", "1x26x26", "1x27x27", "1x43x60", "3x45x83", "1x16x200", "1x200x16", "flat",
                "unaligned"]
_PAIRS, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_itmo_amd import _lib as L
    L.load()


def _pair(case):
    if case not in _PAIRS:
        if case == "flat":
            _PAIRS[case] = DR.flat_pair((1, 45, 84))
        else:
            shape = (1, 12, 28) if case == "unaligned" else tuple(int(v) for v in case.split("x"))
            noise = [0.03, 0.1, 0.005] if shape[0] == 3 else 0.03
            _PAIRS[case] = MR.make_pair(shape, seed=shape[1] * 1000 + shape[2], noise=noise)
    return _PAIRS[case]


def _ref(case, base, alpha):
    """(ssim, B, L, dy) of the reference for the fp32 inputs, computed once and read only."""
    if (case, base) not in _REFS:
        p, t = _pair(case)
        _REFS[case, base] = DR.loss_grad(p.astype(np.float64), t.astype(np.float64), base, alpha)
    return _REFS[case, base]


def _dev(a, off=0):
    """a on the device, `off` floats past a 16-byte boundary."""
    buf = torch.empty(a.size + off, dtype=torch.float32, device="cuda")
    v = buf[off:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _run(case, base, alpha, grad=True, frames=0.0):
    from cnn_itmo_amd import ops
    p, t = _pair(case)
    off = 1 if case == "unaligned" else 0
    y, tt = _dev(p, off), _dev(t, off)
    dy = _dev(np.full(p.shape, np.nan, np.float32), off) if grad else None
    out = ops.dssim_loss_grad(DR.BASE_IDS[base], alpha, y, tt, dy, frames,
                              out=torch.full((p.shape[0], 3), float("nan"), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    return out, dy


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("base,alpha", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("case", KERNEL_CASES)
def test_kernel_matches_reference(case, base, alpha):
    rs, rb, rl, rdy = _ref(case, base, alpha)
    out, dy = _run(case, base, alpha)
    out, dy = out.cpu().numpy(), dy.cpu().numpy().astype(np.float64)
    es = np.abs(out[:, 0] - rs).max()
    eb = np.abs(out[:, 1] - rb).max() / max(np.abs(rb).max(), 1e-300)
    el = (np.abs(out[:, 2] - rl) / np.abs(rl)).max()
    scale = np.abs(rdy).max(axis=(1, 2, 3))
    ed = (np.abs(dy - rdy).max(axis=(1, 2, 3)) / scale).max()
    print(f"dssim {case} base {base}: ssim err {es:.2e}  B rel {eb:.2e}  L rel {el:.2e}  "
          f"dy err {ed:.2e} of max|dy| ({scale.max():.3e})")
    assert not np.isnan(dy).any() and not np.isnan(out).any()
    assert es <= SSIM_TOL, (out[:, 0], rs)
    if base is None:
        assert (out[:, 1] == 0).all()
    else:
        assert eb <= SUM_RTOL, (out[:, 1], rb)
    assert el <= SUM_RTOL, (out[:, 2], rl)
    assert ed <= DY_TOL, ed
    if case == "3x45x83":  # three noise levels: three different values, each its own image's
        assert len(set(np.round(rs, 3))) == 3


@pytest.mark.parametrize("base,alpha", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("case", ["1x12x27", "3x45x83"])
def test_loss_only_determinism_and_grad_frames(case, base, alpha):
    """dy = null gives the same out bit for bit; two runs are bitwise equal; grad_frames = 2n
    gives exactly 0.5 * dy."""
    out, dy = _run(case, base, alpha)
    out0, _ = _run(case, base, alpha, grad=False)
    assert torch.equal(out0, out)
    out1, dy1 = _run(case, base, alpha)
    assert torch.equal(out1, out) and torch.equal(dy1, dy)
    n = _pair(case)[0].shape[0]
    out2, dy2 = _run(case, base, alpha, frames=2.0 * n)
    assert torch.equal(out2, out) and torch.equal(dy2, 0.5 * dy)
    out3, dy3 = _run(case, base, alpha, frames=float(n))
    assert torch.equal(dy3, dy)  # grad_frames <= 0 means n


def _raw(base, alpha, y, t, n, h, w, out, dy, ws, nbytes, frames=0.0):
    from cnn_itmo_amd import _lib as L, ops
    p = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    return L.load().cnnitmo_dssim_loss_grad(base, alpha, p(y), p(t), n, h, w, frames, p(out), p(dy), p(ws), nbytes,
                                            ops.stream_ptr())


@pytest.mark.parametrize("shape", [(2, 27, 28), (1, 27, 27)], ids=["vec", "scalar"])
@pytest.mark.parametrize("grad", [True, False], ids=["grad", "loss"])
def test_poisoned_arena(shape, grad):
    """Every operand carved from a NaN-poisoned arena, the workspace handed over poisoned: dy and
    out fully written, the results those of torch's allocator, nothing outside a payload touched."""
    from cnn_itmo_amd import ops
    n, h, w = shape
    p, t = MR.make_pair(shape, seed=31)
    ar = Arena(16 << 20, "nan", "cuda")
    y = ar.take(p.size, torch.float32, p, "y")
    tt = ar.take(t.size, torch.float32, t, "t")
    out = ar.take(n * 3, torch.float64, name="out")
    dy = ar.take(p.size, torch.float32, name="dy") if grad else None
    nb = ops.dssim_workspace_bytes(n, h, w, grad)
    ws = ar.take(nb, torch.uint8, name="workspace")
    assert _raw(1, 0.84, y, tt, n, h, w, out, dy, ws, nb) == 0
    ar.check_untouched()
    assert poison_count(out) == 0 and (dy is None or poison_count(dy) == 0)
    dy0 = torch.empty(shape + (3,), device="cuda") if grad else None
    out0 = ops.dssim_loss_grad(1, 0.84, torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda(), dy0)
    assert torch.equal(out0.view(-1), out) and (dy is None or torch.equal(dy0.view(-1), dy))


def test_bad_arguments_write_nothing():
    from cnn_itmo_amd import ops
    y = torch.rand(1, 16, 16, 3, device="cuda")
    nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt, device="cuda")  # noqa: E731
    out, dy = nan(1, 3, dt=torch.float64), nan(1, 16, 16, 3)
    ws = ops.workspace(ops.dssim_workspace_bytes(1, 16, 16, 1))
    nb = ws.numel()
    bad = [dict(h=10), dict(w=10), dict(nb=nb - 8), dict(y=None), dict(t=None), dict(out=None), dict(ws=None),
           dict(base=7), dict(alpha=1.5)]
    for ch in bad:
        a = dict(dict(base=1, alpha=0.84, y=y, t=y, n=1, h=16, w=16, out=out, dy=dy, ws=ws, nb=nb), **ch)
        assert _raw(a["base"], a["alpha"], a["y"], a["t"], a["n"], a["h"], a["w"], a["out"], a["dy"], a["ws"],
                    a["nb"]) < 0, ch
    # a loss-only workspace is too small for the gradient
    assert _raw(1, 0.84, y, y, 1, 16, 16, out, dy, ws, ops.dssim_workspace_bytes(1, 16, 16, 0)) < 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dy).all())
    assert _raw(1, 0.84, y, y, 1, 16, 16, out, dy, ws, nb) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dy).any())


# ---------------------------------------------------------------- head with a given gradient
def _check_head_given(dt, Cc, H, W, folded):
    from cnn_itmo_amd import ops
    c = head_case(dt, Cc, H, W, "mse", folded)
    N, Hv, w, t, yref, xin = c["N"], c["Hv"], c["w"], c["t"], c["yref"], c["xin"]
    dyg = (np.random.default_rng(40 + Cc).standard_normal((N, Hv, W, 3)) * 1e-3).astype(np.float32)
    d = DT[dt]
    aff = (cu(c["s"]), cu(c["h"])) if folded else None
    xv = ops.View(dev(c["x"], dt).reshape(-1), N, H, W, Cc, Cc)
    rows = ops.head_rows(N * H * W)
    numel = N * Hv * W * 3
    dz = dyg.astype(np.float64) * yref * (1.0 - yref)
    dx_ref = np.zeros((N, H, W, Cc))
    dx_ref[:, :Hv] = dz @ w.astype(np.float64)
    g3_ref = np.zeros((N, H, W, 3))
    g3_ref[:, :Hv] = dz
    part = torch.empty(rows, 5 + 3 * Cc, device="cuda")
    dx = torch.empty(N * H * W * Cc, dtype=TDT[dt], device="cuda")
    ops.head_fwd_bwd_given(d, xv, Hv, cu(w), cu(c["b"]), cu(t), cu(dyg), part, dx=dx, aff=aff)
    la, dw, db = torch.empty(2, device="cuda"), torch.empty(3, Cc, device="cuda"), torch.empty(3, device="cuda")
    ops.head_finalize(part, rows, Cc, numel, la, dw, db, aff=aff)
    g3 = torch.full((N * H * W * 3,), 7.0, device="cuda")
    part3 = torch.empty(rows, 5 + 3 * Cc, device="cuda")
    ops.head_fwd_bwd_given(d, xv, Hv, cu(w), cu(c["b"]), cu(t), cu(dyg), part3, g3=g3, aff=aff)
    la3, dw3, db3 = torch.empty(2, device="cuda"), torch.empty(3, Cc, device="cuda"), torch.empty(3, device="cuda")
    ops.head_finalize(part3, rows, Cc, numel, la3, dw3, db3, aff=aff)
    torch.cuda.synchronize()
    assert la[0].item() == 0.0 and la3[0].item() == 0.0  # the loss slot
    assert abs(la[1].item() - R.categorical_accuracy(t, yref)) < 1e-6
    k = 1e3 if folded else 1.0
    close(host(dw) * k, dz.reshape(-1, 3).T @ xin.reshape(-1, Cc) * k, "f32", "head dw")
    close(host(db) * k, dz.reshape(-1, 3).sum(0) * k, "f32", "head db")
    close(host(dx).reshape(dx_ref.shape) * 1e3, dx_ref * 1e3, dt, "head dx")
    close(g3.cpu().numpy().reshape(g3_ref.shape) * 1e3, g3_ref * 1e3, "f32", "head g3")
    assert np.array_equal(la3.cpu().numpy(), la.cpu().numpy())
    assert np.array_equal(host(dw3), host(dw)) and np.array_equal(host(db3), host(db))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Cc,H,W", HEAD_SHAPES)
def test_head_given(Cc, H, W, dt):
    _check_head_given(dt, Cc, H, W, folded=False)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_head_given_folded(dt):
    _check_head_given(dt, 64, 8, 16, folded=True)


# ---------------------------------------------------------------- whole network
_NET_REF = {}


def _net_reference(key, base, P, xin, x, seed, valid_rows=None):
    """(target, loss, gradients) of the fp64 oracle; R's loss is patched by the caller.  xin: the
    (zero-padded) input of the oracle, x: its valid rows."""
    if key not in _NET_REF:
        net = R.UNetRef(P)
        y = net.forward(xin, training=True, seed=seed)
        y = y if valid_rows is None else y[:, :valid_rows]
        t = np.clip(x ** 2.2 * 1.2, 0, 1).astype(np.float32).astype(np.float64)
        if base == "mae":
            t = RO.mae_safe_target(y, t)
        ref_loss, _, rg = net.backward(t, valid_rows=valid_rows)
        _NET_REF[key] = (t, y, ref_loss, rg, {k: v.copy() for k, v in P.items()})
    t, y, ref_loss, rg, P0 = _NET_REF[key]
    assert all(np.array_equal(P0[k], P[k]) for k in P0)
    return t, y, ref_loss, rg


def _check_net(m, dtype, loss, key, x, xin, seed, monkeypatch, valid_rows=None):
    d = loss if isinstance(loss, C.DSSIM) else C.DSSIM()
    DR.patch_oracle(monkeypatch, R, d.base, d.alpha)
    from test_gpu_model import randomize_bn
    P = randomize_bn(m, np.random.default_rng(21))
    t, y, ref_loss, rg = _net_reference(key, d.base, P, xin, x, seed, valid_rows)
    if d.base == "mae":  # a condition on the inputs, not a tolerance
        assert float(np.abs(y - t).min()) >= 1e-3
    m.compile(m.optimizer, loss, ["accuracy"])
    eng = m._engine()
    la = eng.train_step(torch.tensor(x, dtype=torch.float32).cuda(), torch.tensor(t, dtype=torch.float32).cuda(),
                        seed=seed, apply=False).cpu().numpy()
    grads = eng.get_grads()
    assert len(rg) == 74 and set(rg) == set(grads)
    if dtype == "float32":
        em = R.UNetRef(P, np.float32)
        em.forward(xin.astype(np.float32), training=True, seed=seed)
        eloss, _, eg = em.backward(t.astype(np.float32), valid_rows=valid_rows)
    else:
        em = R.UNetRef(P, store=R.round_bf16)
        em.forward(xin, training=True, seed=seed)
        eloss, _, eg = em.backward(t, valid_rows=valid_rows)
    err = {k: _rel_l2(grads[k].reshape(rg[k].shape), rg[k]) for k in rg}
    floor = {k: _rel_l2(eg[k], rg[k]) for k in rg}
    lerr, lfloor = abs(la[0] - ref_loss) / ref_loss, abs(eloss - ref_loss) / ref_loss
    worst = max(rg, key=lambda k: err[k] / max(floor[k], 1e-12))
    print(f"{dtype} {d!r}: loss {la[0]:.7f} rel {lerr:.2e} (floor {lfloor:.2e}); worst gradient {worst} "
          f"gpu {err[worst]:.2e} floor {floor[worst]:.2e}; max gpu rel-L2 {max(err.values()):.2e}")
    if dtype == "float32":
        assert lerr <= max(3 * lfloor, 1e-6), (lerr, lfloor)
        bad = {k: (err[k], floor[k]) for k in rg if err[k] > max(1e-4, 3 * floor[k])}
    else:
        assert lerr <= max(3 * lfloor, 5e-3), (lerr, lfloor)
        bad = {k: (err[k], floor[k]) for k in rg if err[k] > max(3 * floor[k], 2e-3)}
    assert not bad, bad
    return t


@pytest.mark.parametrize("dtype,loss", [("float32", "dssim"), ("float32", C.DSSIM("mae")), ("float32", C.DSSIM("mse")),
                                        ("bfloat16", "dssim")], ids=["f32-dssim", "f32-mae", "f32-mse", "bf16-dssim"])
def test_unet_all_74_grads(dtype, loss, monkeypatch):
    """U-Net (64,64,3) b2, train_step(apply=False): the loss and all 74 gradients against UNetRef
    with its loss patched to the DSSIM reference (grad_z = dy * y(1-y)), under
    test_gpu_losses.test_unet_all_74_grads_per_loss's rule and floor runs.  The MAE base runs on
    a target kept 1e-3 away from the reference prediction."""
    m = build_unet((64, 64, 3), dtype, seed=7)
    x = np.random.default_rng(22).integers(0, 256, size=(2, 64, 64, 3)) / 255.0
    base = loss.base if isinstance(loss, C.DSSIM) else None
    _check_net(m, dtype, loss, base, x, x, 9, monkeypatch)
    assert m._engine().iterations == 0 and m._engine().step == 1


def test_padded_frame(monkeypatch):
    """A (40,48,3) model padded to 48 rows: evaluate's loss is 1 - mean SSIM of the prediction's
    40 valid rows and leaves the gradients alone; the training gradients equal the reference's
    on the valid rows."""
    from cnn_itmo_amd import metrics as M
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(40, 48, 3), pad=True, dtype="float32", seed=5, verbose=False)
    x = np.random.default_rng(23).integers(0, 256, size=(2, 40, 48, 3)) / 255.0
    xin = np.concatenate([x, np.zeros((2, 8, 48, 3))], 1)
    t = _check_net(m, "float32", "dssim", "padded", x, xin, 4, monkeypatch, valid_rows=40)
    eng = m._engine()
    eng.grads.fill_(3.0)
    ev = m.evaluate(x, t, batch_size=2)
    assert bool((eng.grads == 3.0).all())
    want = 1.0 - float(M.ssim(m.predict(x), t.astype(np.float32)).mean())
    print(f"padded evaluate loss {ev[0]:.7f}, 1 - mean ssim {want:.7f}")
    assert abs(ev[0] - want) <= 1e-5
    pred = m.predict(x)
    assert abs(ev[1] - R.categorical_accuracy(t, pred)) < 1e-6
    m.compile(m.optimizer, "dssim", ["accuracy", "ssim"])
    ev2 = m.evaluate(x, t, batch_size=2)
    assert ev2[0] == ev[0] and abs((1.0 - ev2[2]) - ev2[0]) <= 1e-6


def test_small_frame_is_an_error_naming_the_size():
    C.clear_session()
    m = C.TinyNet(input_size=(16, 16, 3), seed=5)
    m.compile("adam", "dssim")
    x = np.random.default_rng(2).uniform(size=(1, 10, 16, 3))
    with pytest.raises(ValueError, match="10 x 16"):
        m.train_on_batch(x, x)
    with pytest.raises(ValueError, match="10 x 16"):
        m.evaluate(x, x)


def test_train_step_grad_frames():
    """grad_frames = 2n halves dy exactly, and every gradient with it (fp32, powers of two)."""
    C.clear_session()
    m = C.TinyNet(seed=2)
    m.compile("adam", C.DSSIM("mse"))
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.uniform(size=(2, 64, 64, 3)), dtype=torch.float32).cuda()
    t = torch.tensor(rng.uniform(size=(2, 64, 64, 3)), dtype=torch.float32).cuda()
    eng = m._engine()
    la = eng.train_step(x, t, apply=False).cpu().numpy()
    g = eng.grads.clone()
    la2 = eng.train_step(x, t, apply=False, grad_frames=4).cpu().numpy()
    assert np.array_equal(la, la2) and float(g.abs().max()) > 0 and torch.equal(eng.grads, 0.5 * g)


# ---------------------------------------------------------------- front end
def _pairs(seed, n=4):
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, 64, 64, 3))
    return x, np.clip(x * 0.8 + 0.1, 0, 1)


def test_fit_lowers_the_loss_and_set_dtype_keeps_it():
    m = build_unet((64, 64, 3), "float32", seed=10)
    m.compile("adam", C.DSSIM("mae"), ["accuracy"])
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
    pred = m.predict(x).astype(np.float64)
    want = DR.loss(pred, t, "mae", 0.84)[2].mean()
    assert abs(ev[0] - want) < 1e-5, (ev, want)
    m.set_dtype("bfloat16")
    assert m.loss == C.DSSIM("mae") and m.loss.alpha == 0.84
    la = m.train_on_batch(x[:2], t[:2])
    assert np.isfinite(la[0]) and m.iterations == 31 and la[0] < losses[0]  # still the trained DSSIM model


@pytest.mark.parametrize("ext", ["h5", "npz"])
def test_save_load_continues_bitwise(tmp_path, ext):
    """Two Adam / DSSIM('mse', 0.7) steps, save, load_model: one more step from the loaded model
    equals one more step from the original bit for bit."""
    m = build_unet((64, 64, 3), "float32", seed=11)
    m.compile(C.Adam(lr=2e-3, beta_1=0.8), C.DSSIM("mse", 0.7), ["accuracy"])
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
    assert m2.loss == C.DSSIM("mse", 0.7) and m2.iterations == 2
    la2 = m2.train_on_batch(x, t)
    assert la2 == la and m2.iterations == 3 and m2.engine.step == 3
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    for sa, sb in zip(m.named_slots(), m2.named_slots()):
        assert all(np.array_equal(v, w) for v, w in zip(sa.values(), sb.values()))
