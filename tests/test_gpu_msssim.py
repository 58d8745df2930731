"""Multi-scale SSIM on the GPU (csrc/msssim.hip, the engine and the front end) against the numpy
float64 reference (tests/msssim_ref.py).

Kernel bounds, per image, those of tests/test_gpu_dssim.py:
  |ms_ssim - ref| and |each factor - ref| <= 1e-6, the project's metric bound;
  B and L: relative error <= 1e-9 (fp64 sums);
  |dy - ref| <= 1e-6 * max|ref dy|: 16x the 2^-24 rounding of the fp32 output.
"""
import contextlib
import csv
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cnn_itmo_amd as C  # noqa: E402
from oracle import unet_ref as R  # noqa: E402
import dssim_ref as DR  # noqa: E402
import hdrmetrics_ref as HR  # noqa: E402
import msssim_ref as MS  # noqa: E402
from arena import Arena, poison_count  # noqa: E402
from tests.test_gpu_losses import _rel_l2, build_unet  # noqa: E402

LOSSES = [(None, 1.0), ("mae", 0.84), ("mse", 0.84)]
LOSS_IDS = ["none", "mae", "mse"]
MS_TOL, SUM_RTOL, DY_TOL = 1e-6, 1e-9, 1e-6
W3 = MS.WEIGHTS[:3]

# name -> (shape, power factors, sigma per image; None: dssim_ref's nearly flat pair, 1/B2 ~ 1e3)
#   176:     TF's minimum for five scales; 3w % 4 == 0, the 16-byte path; every side even; the
#            coarsest map is 1 x 1
#   183x205: the scalar path; 183 -> 92 -> 46 -> 23 -> 12 and 205 -> 103 -> 52 -> 26 -> 13: odd at
#            levels 0, 3 and at 0, 1; partial tiles at every level
#   44:      the exact minimum for three scales (44 -> 22 -> 11)
#   flat:    (1,45,84), odd at level 0 / 1 (45 -> 23 -> 12)
KERNEL_CASES = {"176": ((2, 176, 176), MS.WEIGHTS, [0.02, 0.1]),
                "183x205": ((1, 183, 205), MS.WEIGHTS, 0.1),
                "183x205fine": ((1, 183, 205), MS.WEIGHTS, 0.02),
                "44": ((2, 44, 44), W3, [0.02, 0.1]),
                "flat": ((1, 45, 84), W3, None)}
_PAIRS, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_itmo_amd import _lib as L
    L.load()


def _pair(case):
    if case not in _PAIRS:
        shape, _, sigma = KERNEL_CASES[case]
        _PAIRS[case] = DR.flat_pair(shape) if sigma is None else MS.blocky_pair(shape, shape[1] * 1000 + shape[2], sigma)
    return _PAIRS[case]


def _ref(case, base, alpha, frames=None):
    """(ms_ssim, B, L, F, dy) of the reference for the fp32 inputs, computed once and read only."""
    if (case, base, frames) not in _REFS:
        p, t = _pair(case)
        _REFS[case, base, frames] = MS.loss_grad(p.astype(np.float64), t.astype(np.float64), base, alpha,
                                                 KERNEL_CASES[case][1], frames)
    return _REFS[case, base, frames]


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _run(p, t, w, base, alpha, grad=True, frames=0.0, max_val=1.0):
    from cnn_itmo_amd import ops
    y, tt = _cu(p), _cu(t)
    dy = torch.full(p.shape, float("nan"), dtype=torch.float32, device="cuda") if grad else None
    out = ops.msssim_loss_grad(DR.BASE_IDS[base], alpha, w, y, tt, dy, frames, max_val,
                               out=torch.full((p.shape[0], 3 + 3 * len(w)), float("nan"), dtype=torch.float64,
                                              device="cuda"))
    torch.cuda.synchronize()
    return out, dy


def _run_case(case, base, alpha, **kw):
    p, t = _pair(case)
    return _run(p, t, KERNEL_CASES[case][1], base, alpha, **kw)


# ---------------------------------------------------------------- kernels
def _check(case, base, alpha, frames=None):
    rms, rb, rl, rf, rdy = _ref(case, base, alpha, frames)
    assert rf.min() >= 0.1, rf.min()  # no factor near the clamp: the power's derivative is well conditioned
    out, dy = _run_case(case, base, alpha, frames=0.0 if frames is None else frames)
    out, dy = out.cpu().numpy(), dy.cpu().numpy().astype(np.float64)
    n, m = rf.shape[:2]
    em = np.abs(out[:, 0] - rms).max()
    ef = np.abs(out[:, 3:].reshape(n, m, 3) - rf).max()
    eb = np.abs(out[:, 1] - rb).max() / max(np.abs(rb).max(), 1e-300)
    el = (np.abs(out[:, 2] - rl) / np.abs(rl)).max()
    scale = np.abs(rdy).max(axis=(1, 2, 3))
    ed = (np.abs(dy - rdy).max(axis=(1, 2, 3)) / scale).max()
    print(f"msssim {case} base {base} frames {frames}: ms_ssim {rms} err {em:.2e}  factors min {rf.min():.3f} err "
          f"{ef:.2e}  B rel {eb:.2e}  L rel {el:.2e}  dy err {ed:.2e} of max|dy| ({scale.max():.3e})")
    assert not np.isnan(dy).any() and not np.isnan(out).any()
    assert em <= MS_TOL and ef <= MS_TOL, (out, rms, rf)
    if base is None:
        assert (out[:, 1] == 0).all()
    else:
        assert eb <= SUM_RTOL, (out[:, 1], rb)
    assert el <= SUM_RTOL, (out[:, 2], rl)
    assert ed <= DY_TOL, ed


@pytest.mark.parametrize("base,alpha", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernel_matches_reference(case, base, alpha):
    _check(case, base, alpha)


def test_kernel_matches_reference_with_grad_frames():
    """grad_frames = 3 on a batch of 2: dy is normalised by 3 frames, out is the same."""
    _check("176", "mae", 0.84, frames=3.0)
    assert torch.equal(_run_case("176", "mae", 0.84, frames=3.0)[0], _run_case("176", "mae", 0.84)[0])


@pytest.mark.parametrize("base,alpha", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("case", ["176", "183x205"])
def test_loss_only_with_max_val_255(case, base, alpha):
    """The metric's form: 0..255 images with max_val 255, no gradient."""
    p, t = _pair(case)
    w = KERNEL_CASES[case][1]
    p, t = np.round(p * 255.0).astype(np.float32), np.round(t * 255.0).astype(np.float32)
    rf = MS.factors(p, t, w, 255.0)
    rms, rb, rl = MS.loss(p, t, base, alpha, w, 255.0)
    assert rf.min() >= 0.1
    out = _run(p, t, w, base, alpha, grad=False, max_val=255.0)[0].cpu().numpy()
    em, ef = np.abs(out[:, 0] - rms).max(), np.abs(out[:, 3:].reshape(rf.shape) - rf).max()
    print(f"msssim {case} base {base} max_val 255: ms_ssim {rms} err {em:.2e}, factors err {ef:.2e}")
    assert em <= MS_TOL and ef <= MS_TOL
    if base is not None:
        assert np.abs(out[:, 1] - rb).max() / np.abs(rb).max() <= SUM_RTOL
    assert (np.abs(out[:, 2] - rl) / np.abs(rl)).max() <= SUM_RTOL


@pytest.mark.parametrize("case", ["183x205", "44"])
def test_clamped_channels(case):
    """y = 1 - t: every cs mean is about -0.9 in the reference, so ms_ssim is exactly 0; without a
    base dy is exactly zero everywhere (and finite), with 'mae' it is the base term's alone."""
    _, t = _pair(case)
    w = KERNEL_CASES[case][1]
    y = (1.0 - t.astype(np.float64)).astype(np.float32)
    rf = MS.factors(y, t, w)
    assert rf[:, :-1].max() < -0.5, rf
    out, dy = _run(y, t, w, None, 1.0)
    assert bool((out[:, 0] == 0).all()) and bool((out[:, 2] == 1).all())
    assert np.abs(out[:, 3:].cpu().numpy().reshape(rf.shape) - rf).max() <= MS_TOL
    assert bool(torch.isfinite(dy).all()) and not bool(dy.any())
    out, dy = _run(y, t, w, "mae", 0.84)
    assert bool((out[:, 0] == 0).all())
    d = y.astype(np.float64) - t.astype(np.float64)
    want = (1.0 - 0.84) / (y.shape[0] * d[0].size) * np.sign(d)
    assert np.array_equal(dy.cpu().numpy(), want.astype(np.float32))


@pytest.mark.parametrize("case", ["176", "183x205", "44"])
def test_identity(case):
    _, t = _pair(case)
    w = KERNEL_CASES[case][1]
    out, dy = _run(t, t, w, "mse", 0.84)
    out = out.cpu().numpy()
    assert np.abs(out[:, 0] - 1.0).max() <= 1e-12 and np.abs(out[:, 3:] - 1.0).max() <= 1e-12
    assert (out[:, 1] == 0).all() and np.abs(out[:, 2]).max() <= 1e-12 and bool(torch.isfinite(dy).all())


@pytest.mark.parametrize("base,alpha", LOSSES, ids=LOSS_IDS)
@pytest.mark.parametrize("case", ["183x205", "44"])
def test_loss_only_determinism_and_grad_frames(case, base, alpha):
    """dy = null gives the same out bit for bit; two runs are bitwise equal, loss-only and with
    the gradient; grad_frames = 2n gives exactly 0.5 * dy."""
    out, dy = _run_case(case, base, alpha)
    out0, _ = _run_case(case, base, alpha, grad=False)
    assert torch.equal(out0, out) and torch.equal(_run_case(case, base, alpha, grad=False)[0], out0)
    out1, dy1 = _run_case(case, base, alpha)
    assert torch.equal(out1, out) and torch.equal(dy1, dy)
    n = _pair(case)[0].shape[0]
    out2, dy2 = _run_case(case, base, alpha, frames=2.0 * n)
    assert torch.equal(out2, out) and torch.equal(dy2, 0.5 * dy) and float(dy.abs().max()) > 0
    assert torch.equal(_run_case(case, base, alpha, frames=float(n))[1], dy)  # grad_frames <= 0 means n


def _raw(base, alpha, pf, max_val, y, t, n, h, w, out, dy, ws, nbytes, frames=0.0, scales=None):
    import ctypes
    from cnn_itmo_amd import _lib as L, ops
    p = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    arr = (ctypes.c_double * max(1, len(pf)))(*pf)
    return L.load().cnnitmo_msssim_loss_grad(base, alpha, ctypes.addressof(arr), len(pf) if scales is None else scales,
                                             max_val, p(y), p(t), n, h, w, frames, p(out), p(dy), p(ws), nbytes,
                                             ops.stream_ptr())


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "loss"])
def test_poisoned_arena(grad):
    """Every operand carved from a NaN-poisoned arena, the workspace handed over poisoned: dy and
    out fully written, the results those of torch's allocator, nothing outside a payload touched."""
    from cnn_itmo_amd import ops
    p, t = _pair("183x205")
    n, h, w = p.shape[:3]
    ar = Arena(24 << 20, "nan", "cuda")
    y = ar.take(p.size, torch.float32, p, "y")
    tt = ar.take(t.size, torch.float32, t, "t")
    out = ar.take(n * 18, torch.float64, name="out")
    dy = ar.take(p.size, torch.float32, name="dy") if grad else None
    nb = ops.msssim_workspace_bytes(n, h, w, 5, grad)
    ws = ar.take(nb, torch.uint8, name="workspace")
    assert _raw(1, 0.84, MS.WEIGHTS, 1.0, y, tt, n, h, w, out, dy, ws, nb) == 0
    torch.cuda.synchronize()
    ar.check_untouched()
    assert poison_count(out) == 0 and (dy is None or poison_count(dy) == 0)
    out0, dy0 = _run(p, t, MS.WEIGHTS, "mae", 0.84, grad=grad)
    assert torch.equal(out0.view(-1), out) and (dy is None or torch.equal(dy0.view(-1), dy))


def test_bad_arguments_write_nothing():
    from cnn_itmo_amd import ops
    y = torch.rand(1, 48, 48, 3, device="cuda")
    nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt, device="cuda")  # noqa: E731
    out, dy = nan(1, 12, dt=torch.float64), nan(1, 48, 48, 3)
    ws = ops.workspace(ops.msssim_workspace_bytes(1, 48, 48, 3, 1) + 8)
    nb = ws.numel() - 8
    inf, qnan = float("inf"), float("nan")
    ok = dict(base=1, alpha=0.84, pf=W3, max_val=1.0, y=y, t=y, n=1, h=48, w=48, out=out, dy=dy, ws=ws, nb=nb, scales=None)
    bad = [dict(base=7), dict(base=-1), dict(alpha=1.5), dict(alpha=-0.5), dict(base=0, alpha=0.5), dict(scales=0),
           dict(scales=6), dict(pf=(0.1, -0.2, 0.3)), dict(pf=(0.1, inf, 0.3)), dict(pf=(qnan, 0.2, 0.3)),
           dict(max_val=0.0), dict(max_val=-2.0), dict(h=40), dict(w=40), dict(pf=MS.WEIGHTS[:4]),
           dict(nb=nb - 8), dict(ws=ws[4:]), dict(y=None), dict(t=None), dict(out=None), dict(ws=None)]
    for ch in bad:
        a = dict(ok, **ch)
        assert _raw(a["base"], a["alpha"], a["pf"], a["max_val"], a["y"], a["t"], a["n"], a["h"], a["w"], a["out"],
                    a["dy"], a["ws"], a["nb"], scales=a["scales"]) < 0, ch
    # a loss-only workspace is too small for the gradient
    assert _raw(1, 0.84, W3, 1.0, y, y, 1, 48, 48, out, dy, ws, ops.msssim_workspace_bytes(1, 48, 48, 3, 0)) < 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dy).all())
    a = ok
    assert _raw(a["base"], a["alpha"], a["pf"], a["max_val"], y, y, 1, 48, 48, out, dy, ws, nb) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dy).any())


# ---------------------------------------------------------------- whole network
_NET_REF = {}


def _net_reference(key, P, x, seed):
    """(target, prediction, loss, gradients) of the fp64 oracle; R's loss is patched by the caller.
    The target is the reference prediction + N(0, 0.2), clipped, in fp32: a random network's
    output is uncorrelated with any fixed target, which would put every factor at the clamp
    (MS-SSIM here 0.87, every factor >= 0.76)."""
    if key not in _NET_REF:
        net = R.UNetRef(P)
        y = net.forward(x, training=True, seed=seed)
        t = np.clip(y + np.random.default_rng(5).normal(0.0, 0.2, y.shape), 0, 1).astype(np.float32).astype(np.float64)
        ref_loss, _, rg = net.backward(t)
        _NET_REF[key] = (t, y, ref_loss, rg, {k: v.copy() for k, v in P.items()})
    t, y, ref_loss, rg, P0 = _NET_REF[key]
    assert all(np.array_equal(P0[k], P[k]) for k in P0)
    return t, y, ref_loss, rg


@pytest.mark.parametrize("dtype,loss", [("float32", C.MSSSIM(power_factors=W3)),
                                        ("float32", C.MSSSIM("mse", power_factors=W3)),
                                        ("bfloat16", C.MSSSIM(power_factors=W3))], ids=["f32-none", "f32-mse", "bf16-none"])
def test_unet_all_74_grads(dtype, loss, monkeypatch):
    """U-Net (128,128,3) b1, three scales, train_step(apply=False): the loss and all 74 gradients
    against UNetRef with its loss patched to the MS-SSIM reference (grad_z = dy * y(1-y)), under
    test_gpu_dssim.test_unet_all_74_grads's rule, bounds and floor runs."""
    from test_gpu_model import randomize_bn
    m = build_unet((128, 128, 3), dtype, seed=7)
    x = np.random.default_rng(22).integers(0, 256, size=(1, 128, 128, 3)) / 255.0
    seed = 9
    MS.patch_oracle(monkeypatch, R, loss.base, loss.alpha, loss.power_factors)
    P = randomize_bn(m, np.random.default_rng(21))
    t, y, ref_loss, rg = _net_reference(loss.base, P, x, seed)
    assert MS.factors(y, t, W3).min() >= 0.1  # a condition on the inputs, not a tolerance
    m.compile(m.optimizer, loss, ["accuracy"])
    eng = m._engine()
    la = eng.train_step(torch.tensor(x, dtype=torch.float32).cuda(), torch.tensor(t, dtype=torch.float32).cuda(),
                        seed=seed, apply=False).cpu().numpy()
    grads = eng.get_grads()
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
    print(f"{dtype} {loss!r}: loss {la[0]:.7f} rel {lerr:.2e} (floor {lfloor:.2e}); worst gradient {worst} "
          f"gpu {err[worst]:.2e} floor {floor[worst]:.2e}; max gpu rel-L2 {max(err.values()):.2e}")
    if dtype == "float32":
        assert lerr <= max(3 * lfloor, 1e-6), (lerr, lfloor)
        bad = {k: (err[k], floor[k]) for k in rg if err[k] > max(1e-4, 3 * floor[k])}
    else:
        assert lerr <= max(3 * lfloor, 5e-3), (lerr, lfloor)
        bad = {k: (err[k], floor[k]) for k in rg if err[k] > max(3 * floor[k], 2e-3)}
    assert not bad, bad
    assert eng.iterations == 0 and eng.step == 1


def _blocky_xy(n, h, w, seed):
    t, x = MS.blocky_pair((n, h, w), seed, 0.1)
    return x.astype(np.float64), t.astype(np.float64)


@pytest.mark.parametrize("size,pad", [((176, 176, 3), False), ((168, 176, 3), True)], ids=["176", "168pad"])
def test_evaluate_five_scales(size, pad):
    """evaluate's loss with the default five scales is the reference's on predict's output (1e-5,
    test_gpu_dssim.test_padded_frame's bound); a pad=True model of 168 valid rows (not a multiple
    of 16) scores those rows; the compiled metric is 1 - that loss."""
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=size, pad=pad, dtype="float32", seed=5, verbose=False)
    x, t = _blocky_xy(2, size[0], size[1], 23)
    m.compile(m.optimizer, C.MSSSIM("mae"), ["accuracy", "ms_ssim"])
    eng = m._engine()
    eng.grads.fill_(3.0)
    ev = m.evaluate(x, t, batch_size=2)
    assert bool((eng.grads == 3.0).all())
    pred = m.predict(x)
    assert pred.shape == t.shape
    rms, _, rl = MS.loss(pred.astype(np.float64), t, "mae", 0.84)
    print(f"{size} evaluate loss {ev[0]:.7f} (reference {rl.mean():.7f}), ms_ssim {ev[2]:.7f} ({rms.mean():.7f})")
    assert m.metrics_names == ["loss", "acc", "ms_ssim"]
    assert abs(ev[0] - rl.mean()) <= 1e-5 and abs(ev[2] - rms.mean()) <= 1e-5
    assert abs(ev[1] - R.categorical_accuracy(t, pred)) < 1e-6


def test_small_frame_is_an_error_naming_the_sizes():
    C.clear_session()
    m = C.TinyNet(input_size=(48, 48, 3), seed=5)
    m.compile("adam", C.MSSSIM(power_factors=W3))
    x = np.random.default_rng(2).uniform(size=(1, 40, 48, 3))
    with pytest.raises(ValueError, match="40 x 48.*41 x 41"):
        m.train_on_batch(x, x)
    with pytest.raises(ValueError, match="40 x 48.*41 x 41"):
        m.evaluate(x, x)
    m.compile("adam", "mse", ["ms_ssim"])  # the metric has five scales
    with pytest.raises(ValueError, match="40 x 48"):
        m.evaluate(x, x)


def test_train_step_grad_frames():
    """grad_frames = 2n halves dy exactly, and every gradient with it (fp32, powers of two)."""
    C.clear_session()
    m = C.TinyNet(seed=2)
    m.compile("adam", C.MSSSIM("mse", power_factors=W3))
    x, t = _blocky_xy(2, 64, 64, 3)
    x, t = torch.tensor(x, dtype=torch.float32).cuda(), torch.tensor(t, dtype=torch.float32).cuda()
    eng = m._engine()
    la = eng.train_step(x, t, apply=False).cpu().numpy()
    g = eng.grads.clone()
    la2 = eng.train_step(x, t, apply=False, grad_frames=4).cpu().numpy()
    assert np.array_equal(la, la2) and float(g.abs().max()) > 0 and torch.equal(eng.grads, 0.5 * g)


# ---------------------------------------------------------------- front end
def test_fit_lowers_the_loss():
    m = build_unet((64, 64, 3), "float32", seed=10)
    loss = C.MSSSIM("mae", power_factors=W3)
    m.compile("adam", loss, ["accuracy"])
    x, t = _blocky_xy(4, 64, 64, 9)

    def gen():
        while True:
            yield x[:2], t[:2]
            yield x[2:], t[2:]
    h = m.fit_generator(gen(), steps_per_epoch=10, epochs=3, verbose=0)
    losses = h.history["loss"]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    ev = m.evaluate(x, t, batch_size=2)
    want = MS.loss(m.predict(x).astype(np.float64), t, "mae", 0.84, W3)[2].mean()
    assert abs(ev[0] - want) < 1e-5, (ev, want)
    m.set_dtype("bfloat16")
    assert m.loss == loss
    la = m.train_on_batch(x[:2], t[:2])
    assert np.isfinite(la[0]) and m.iterations == 31 and la[0] < losses[0]


@pytest.mark.parametrize("ext", ["hdf5", "npz"])
def test_save_load_continues_bitwise(tmp_path, ext):
    """Two Adam / MSSSIM('mse', 0.7, three scales) steps, save, load_model: one more step from the
    loaded model equals one more step from the original bit for bit."""
    m = build_unet((64, 64, 3), "float32", seed=11)
    loss = C.MSSSIM("mse", 0.7, (0.2, 0.1 + 0.2, 0.5))
    m.compile(C.Adam(lr=2e-3, beta_1=0.8), loss, ["accuracy"])
    x, t = _blocky_xy(2, 64, 64, 13)
    for _ in range(2):
        m.train_on_batch(x, t)
    p = str(tmp_path / f"ck.{ext}")
    m.save(p)
    la = m.train_on_batch(x, t)
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m2 = C.load_model(p)
    assert type(m2.optimizer) is C.Adam and m2.optimizer.get_config() == m.optimizer.get_config()
    assert m2.loss == loss and m2.loss.power_factors == loss.power_factors and m2.iterations == 2
    la2 = m2.train_on_batch(x, t)
    assert la2 == la and m2.iterations == 3 and m2.engine.step == 3
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    for sa, sb in zip(m.named_slots(), m2.named_slots()):
        assert all(np.array_equal(v, w) for v, w in zip(sa.values(), sb.values()))


def test_compiled_metric_in_history_and_checkpoint(tmp_path):
    """compile(metrics=['ms_ssim']): val_ms_ssim in History, equal to evaluate's and to the
    reference on predict's output; ModelCheckpoint(monitor='val_ms_ssim') keeps the best (max)."""
    C.clear_session()
    m = C.TinyNet(input_size=(176, 176, 3), seed=4)
    m.compile("adam", "mae", ["accuracy", "ms_ssim"])
    x, t = _blocky_xy(4, 176, 176, 31)
    xv, tv = _blocky_xy(3, 176, 176, 32)

    def gen():
        while True:
            yield x[:2], t[:2]
            yield x[2:], t[2:]
    pat = str(tmp_path / "m-{epoch:02d}.npz")
    ck = C.ModelCheckpoint(pat, monitor="val_ms_ssim", save_best_only=True)
    h = m.fit_generator(gen(), steps_per_epoch=2, epochs=3, verbose=0, validation_data=(xv, tv), callbacks=[ck])
    assert sorted(h.history) == ["acc", "loss", "val_acc", "val_loss", "val_ms_ssim"]
    vm = h.history["val_ms_ssim"]
    ev = m.evaluate(xv, tv)
    assert m.metrics_names == ["loss", "acc", "ms_ssim"] and vm[-1] == pytest.approx(ev[2], rel=1e-14)
    assert abs(vm[-1] - MS.ms_ssim(m.predict(xv).astype(np.float64), tv).mean()) <= 1e-5
    assert ck.mode == "max"
    want = [pat.format(epoch=e + 1) for e, v in enumerate(vm) if e == 0 or v > max(vm[:e])]
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in want)
    m2 = C.load_model(want[-1])
    assert m2.metrics_names == ["loss", "acc", "ms_ssim"] and m2.image_metrics == ["ms_ssim"]


def test_metric_functions_and_command_lines(tmp_path):
    """metrics.ms_ssim (fp32, uint8, three scales), hdrmetrics.hdr_ms_ssim and the two --ms-ssim
    flags agree with the reference within 1e-6 on written file pairs."""
    from PIL import Image
    from cnn_itmo_amd import evaluate_hdr as EH, hdrio as H, hdrmetrics as HM, metrics as M, predict as PR
    p, t = _pair("183x205")
    assert abs(M.ms_ssim(p, t).item() - _ref("183x205", None, 1.0)[0][0]) <= MS_TOL
    assert abs(M.ms_ssim(_cu(p), _cu(t), power_factors=W3).item() - MS.ms_ssim(p, t, 1.0, W3)[0]) <= MS_TOL
    a, b = np.round(p * 255).astype(np.uint8), np.round(t * 255).astype(np.uint8)
    got = M.ms_ssim(a[0], b[0], max_val=255)
    assert got.dtype == torch.float64 and tuple(got.shape) == (1,) and got.is_cuda
    assert abs(got.item() - MS.ms_ssim(a, b, 255.0)[0]) <= MS_TOL
    with pytest.raises(ValueError, match="5 scales.*161 x 161.*160 x 205"):
        M.ms_ssim(p[:, :160], t[:, :160])
    with pytest.raises(ValueError):
        M.ms_ssim(p, t, power_factors=(0.5, -0.5))

    # predict --reference --ms-ssim: the written PNG against the reference PNG, max_val 255
    C.clear_session()
    m = C.TinyNet(input_size=(176, 176, 3), seed=5)
    ck = str(tmp_path / "tiny.hdf5")
    m.save(ck)
    ind, refd, outd = tmp_path / "in", tmp_path / "ref", tmp_path / "out"
    for d in (ind, refd):
        os.makedirs(d)
    x8, t8 = MS.blocky_pair((1, 176, 176), 6, 0.1)
    Image.fromarray(np.round(x8[0] * 255).astype(np.uint8)).save(str(ind / "0000.png"))
    Image.fromarray(np.round(t8[0] * 255).astype(np.uint8)).save(str(refd / "0000.png"))
    csvp = str(tmp_path / "scores.csv")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert PR.main(["--model", ck, "--input", str(ind), "--output", str(outd), "--reference", str(refd),
                        "--metrics-csv", csvp, "--ms-ssim"]) == 0
    with open(csvp, newline="") as fh:
        rows = list(csv.reader(fh, delimiter=";"))
    assert rows[0] == ["name", "psnr", "ssim", "ms_ssim"] and len(rows) == 2
    wa, wb = np.asarray(Image.open(str(outd / "0000.png"))), np.asarray(Image.open(str(refd / "0000.png")))
    want = MS.ms_ssim(wa, wb, 255.0)[0]
    assert abs(float(rows[1][3]) - want) <= MS_TOL and f"ms_ssim {want:.6f}" in buf.getvalue()
    with contextlib.redirect_stdout(io.StringIO()):  # without the flag the CSV is what it was
        PR.main(["--model", ck, "--input", str(ind), "--output", str(outd), "--reference", str(refd), "--metrics-csv", csvp])
    with open(csvp, newline="") as fh:
        assert next(csv.reader(fh, delimiter=";")) == ["name", "psnr", "ssim"]

    # hdr_ms_ssim and evaluate_hdr --ms-ssim: the files read back, aligned, anchored, PQ-encoded
    hp, hr = HR.make_pair((1, 176, 180), seed=9, level=0.1)
    pred, ref = tmp_path / "pred", tmp_path / "hdrref"
    os.makedirs(pred)
    os.makedirs(ref)
    H.write_image(str(pred / "a.hdr"), hp[0])
    H.write_image(str(ref / "a.pfm"), hr[0])
    fa, fb = H.read_image(str(pred / "a.hdr")), H.read_image(str(ref / "a.pfm"))
    ha, hb = fa.cpu().numpy()[None].astype(np.float32), fb.cpu().numpy()[None].astype(np.float32)
    for enc, kw in (("pq", {}), ("log", dict(align="median", anchor="percentile", q=0.99))):
        sp, sr = HR.scales(ha, hb, **kw)
        want = MS.ms_ssim(HR.encode(ha, enc, sp), HR.encode(hb, enc, sr))[0]
        got = HM.hdr_ms_ssim(fa, fb, enc, **kw).item()
        print(f"hdr_ms_ssim {enc}: {got:.7f}, reference {want:.7f}")
        assert abs(got - want) <= MS_TOL
    want = MS.ms_ssim(HR.encode(ha, "pq", HR.scales(ha, hb)[0]), HR.encode(hb, "pq", HR.scales(ha, hb)[1]))[0]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert EH.main(["--pred", str(pred), "--reference", str(ref), "--csv", csvp, "--ms-ssim"]) == 0
    with open(csvp, newline="") as fh:
        rows = list(csv.reader(fh, delimiter=";"))
    assert rows[0] == ["name", "psnr", "ssim", "scale_pred", "scale_ref", "ms_ssim"] and rows[1][0] == "a.hdr"
    assert abs(float(rows[1][5]) - want) <= MS_TOL and f"ms_ssim {float(rows[1][5]):.6f}" in buf.getvalue()
    with contextlib.redirect_stdout(io.StringIO()):
        EH.main(["--pred", str(pred), "--reference", str(ref), "--csv", csvp])
    with open(csvp, newline="") as fh:
        assert next(csv.reader(fh, delimiter=";")) == ["name", "psnr", "ssim", "scale_pred", "scale_ref"]
