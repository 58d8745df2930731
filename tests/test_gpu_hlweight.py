"""The highlight-weighted training loss on the GPU (csrc/hlweight.hip, the engine's given-gradient
head and the front end) against the numpy float64 reference (tests/hlweight_ref.py).

Kernel bounds, per image:
  out {A, B, L, H}: relative error <= 1e-10.  Every sum has at most 1e5 non-negative fp64 terms
    here, so any summation order is within terms * 2^-53 ~ 1.1e-11 of exact, for the kernel and
    for numpy alike; a sum that is exactly 0 (no masked pixel) must be exactly 0.
  dy: within 1 fp32 ulp of the reference's fp64 value cast to fp32 (two correctly rounded casts of
    fp64 values a few fp64 ulps apart cannot differ by more).  Identity is expected: kernel and
    reference do the same fp64 operations in the same order; the count of non-identical elements
    is printed.

B4 = 1024: the pixels one workgroup of the kernel takes (256 threads x 4 pixels).
"""
import contextlib
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import cnn_itmo_amd as C  # noqa: E402
from oracle import unet_ref as R  # noqa: E402
import hlweight_ref as HR  # noqa: E402
import ref_objectives as RO  # noqa: E402
from arena import Arena, poison_count  # noqa: E402
from tests.test_gpu_losses import _rel_l2, build_unet  # noqa: E402

B4 = 1024
TAU, GAIN = 0.75, 3.0  # (tau is an fp32 value: m == tau happens)
OUT_RTOL = 1e-10
BASES = ["mse", "mae"]
SOURCES = ["input", "target"]

# 1x1x1; 3x5x7: images 2 and 3 start off a 16-byte boundary (the one-pixel path), image 2 has no masked
# pixel, image 3 only saturated ones; one pixel less than a workgroup, exactly one, one more (x2 images: the
# second of the odd sizes is off alignment); 3 rows of 2 B4 / 3 + 1 pixels: two workgroups and one pixel;
# 2x33x65: several workgroups, a % 4 tail, image 2 off alignment; 1x12x28 on a view one float off a 16-byte
# boundary
KERNEL_CASES = ["1x1x1", "3x5x7", f"2x1x{B4 - 1}", f"2x1x{B4}", f"2x1x{B4 + 1}", f"1x3x{2 * B4 // 3 + 1}", "2x33x65",
                "unaligned"]
_DATA, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_itmo_amd import _lib as L
    L.load()


def _shape(case):
    return (1, 12, 28) if case == "unaligned" else tuple(int(v) for v in case.split("x"))


def _data(case, source):
    """(s, y, t) fp32 of a case, made once; source 'target': s is t."""
    if (case, source) not in _DATA:
        shape = _shape(case)
        three = shape[0] == 3
        s, y, t = HR.make_case(shape, TAU, seed=shape[1] * 1000 + shape[2], source=source,
                               flat_image=1 if three else None, full_image=2 if three else None)
        if shape[1] * shape[2] >= 10:  # a condition on the inputs: every image mixes the kinds of pixel
            m = s.max(axis=-1).reshape(shape[0], -1)
            kinds = [(m < TAU), (m == TAU), (m > TAU) & (m < 1.0), (m == 1.0)]
            for i in range(shape[0]):
                want = [True, True, i != 1, i != 1] if three and i < 2 else [False, False, False, True] if three \
                    else [True] * 4
                assert [bool(k[i].any()) for k in kinds] == want, (case, i)
            assert (y == t).any() and (y != t).any()
        _DATA[case, source] = (s, y, t)
    return _DATA[case, source]


def _ref(case, base, source):
    """(out, dy) of the reference for the fp32 inputs, computed once and read only."""
    if (case, base, source) not in _REFS:
        s, y, t = _data(case, source)
        _REFS[case, base, source] = HR.loss_grad(s, y, t, base, TAU, GAIN)
    return _REFS[case, base, source]


def _dev(a, off=0):
    """a on the device, `off` floats past a 16-byte boundary."""
    buf = torch.empty(a.size + off, dtype=torch.float32, device="cuda")
    v = buf[off:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _run(case, base, source, grad=True, frames=0.0, off=None):
    from cnn_itmo_amd import ops
    s, y, t = _data(case, source)
    off = (1 if case == "unaligned" else 0) if off is None else off
    yd, td = _dev(y, off), _dev(t, off)
    sd = td if source == "target" else _dev(s, off)  # 'target': the same memory
    dy = _dev(np.full(y.shape, np.nan, np.float32), off) if grad else None
    out = ops.highlight_loss_grad(HR.BASE_IDS[base], TAU, GAIN, sd, yd, td, dy, frames,
                                  out=torch.full((y.shape[0], 4), float("nan"), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    return out, dy


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("case", KERNEL_CASES)
def test_kernel_matches_reference(case, base, source):
    rout, rdy = _ref(case, base, source)
    out, dy = _run(case, base, source)
    out, dy = out.cpu().numpy(), dy.cpu().numpy()
    assert not np.isnan(dy).any() and not np.isnan(out).any()
    eo = np.abs(out - rout) / np.where(rout == 0, 1.0, np.abs(rout))
    r32 = rdy.astype(np.float32)
    differ = int((dy != r32).sum())
    ulps = np.abs(dy.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
    print(f"highlight {case} {base}/{source}: out rel err {eo.max(axis=0)}  dy: {differ} of {dy.size} elements "
          f"not identical, max {ulps.max():.1f} ulp")
    assert (out[rout == 0] == 0).all()
    assert eo.max() <= OUT_RTOL, (out, rout)
    assert ulps.max() <= 1.0, ulps.max()
    if base == "mae":
        s, y, t = _data(case, source)
        assert (dy[y == t] == 0).all()  # sign(0) = 0
    if case == "3x5x7":
        assert out[1, 0] == 0 and out[1, 3] == 0 and out[1, 2] == out[1, 1]  # no masked pixel
        assert out[2, 0] == 1.0 and out[2, 3] > 0  # every pixel saturated


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("case", ["3x5x7", "2x33x65"])
def test_loss_only_determinism_and_grad_frames(case, base, source):
    """dy = null gives the same out bit for bit; two runs are bitwise equal; grad_frames = 2n
    gives exactly 0.5 * dy."""
    out, dy = _run(case, base, source)
    out0, _ = _run(case, base, source, grad=False)
    assert torch.equal(out0, out)
    out1, dy1 = _run(case, base, source)
    assert torch.equal(out1, out) and torch.equal(dy1, dy)
    n = _shape(case)[0]
    out2, dy2 = _run(case, base, source, frames=2.0 * n)
    assert torch.equal(out2, out) and torch.equal(dy2, 0.5 * dy) and float(dy.abs().max()) > 0
    out3, dy3 = _run(case, base, source, frames=float(n))
    assert torch.equal(dy3, dy)  # grad_frames <= 0 means n


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("base", BASES)
def test_unaligned_view_equals_aligned(base, source):
    """The one-pixel path (a view one float off a 16-byte boundary) gives the bits of the 16-byte path."""
    out_a, dy_a = _run("unaligned", base, source, off=0)
    out_u, dy_u = _run("unaligned", base, source, off=1)
    assert torch.equal(out_u, out_a) and torch.equal(dy_u, dy_a)
    out_l, _ = _run("unaligned", base, source, grad=False, off=1)
    assert torch.equal(out_l, out_a)


def test_functional_form_takes_numpy_and_single_images():
    s, y, t = _data("2x33x65", "input")
    rout, _ = HR.loss_grad(s, y, t, "mae", 0.5, 2.0)
    out = C.losses.highlight_weighted(s, y, t, base="mae", threshold=0.5, gain=2.0)
    assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == (2, 4)
    assert np.abs(out.cpu().numpy() - rout).max() <= OUT_RTOL * np.abs(rout).max()
    one = C.losses.highlight_weighted(torch.from_numpy(s[1]).cuda(), y[1], t[1], "mae", 0.5, 2.0)
    assert tuple(one.shape) == (1, 4) and torch.equal(one[0], out[1])  # (image 2 of the batch was off alignment)
    rt, _ = HR.loss_grad(t, y, t, "mse", 0.5, 2.0)
    ot = C.losses.highlight_weighted(None, y, t, "mse", 0.5, 2.0, source="target")
    assert np.abs(ot.cpu().numpy() - rt).max() <= OUT_RTOL * np.abs(rt).max()
    with pytest.raises(ValueError):
        C.losses.highlight_weighted(s[:, :8], y, t)
    with pytest.raises(ValueError):
        C.losses.highlight_weighted(s, y, t, gain=-1.0)


def _raw(base, tau, gain, s, y, t, n, h, w, out, dy, ws, nbytes, frames=0.0):
    from cnn_itmo_amd import _lib as L, ops
    p = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    return L.load().cnnitmo_highlight_loss_grad(base, tau, gain, p(s), p(y), p(t), n, h, w, frames, p(out), p(dy),
                                                p(ws), nbytes, ops.stream_ptr())


@pytest.mark.parametrize("shape,alias", [((2, 33, 64), False), ((3, 5, 7), True)], ids=["vec", "scalar-alias"])
@pytest.mark.parametrize("grad", [True, False], ids=["grad", "loss"])
def test_poisoned_arena(shape, alias, grad):
    """Every operand carved from a NaN-poisoned arena, the workspace handed over poisoned: dy and
    out fully written, the results those of torch's allocator, nothing outside a payload touched.
    (2,33,64): both images aligned, three workgroups each, the last one part full; (3,5,7): images 2
    and 3 off alignment, s the same memory as t."""
    from cnn_itmo_amd import ops
    n, h, w = shape
    s, y, t = HR.make_case(shape, TAU, seed=31, source="target" if alias else "input")
    ar = Arena(16 << 20, "nan", "cuda")
    yd = ar.take(y.size, torch.float32, y, "y")
    td = ar.take(t.size, torch.float32, t, "t")
    sd = td if alias else ar.take(s.size, torch.float32, s, "s")
    out = ar.take(n * 4, torch.float64, name="out")
    dy = ar.take(y.size, torch.float32, name="dy") if grad else None
    nb = ops.highlight_workspace_bytes(n, h, w)
    ws = ar.take(nb, torch.uint8, name="workspace")
    assert _raw(2, TAU, GAIN, sd, yd, td, n, h, w, out, dy, ws, nb) == 0
    ar.check_untouched()
    assert poison_count(out) == 0 and (dy is None or poison_count(dy) == 0)
    dy0 = torch.empty(shape + (3,), device="cuda") if grad else None
    t0 = torch.from_numpy(t).cuda()
    s0 = t0 if alias else torch.from_numpy(s).cuda()
    out0 = ops.highlight_loss_grad(2, TAU, GAIN, s0, torch.from_numpy(y).cuda(), t0, dy0)
    assert torch.equal(out0.view(-1), out) and (dy is None or torch.equal(dy0.view(-1), dy))


def test_bad_arguments_write_nothing():
    from cnn_itmo_amd import ops
    y = torch.rand(1, 16, 16, 3, device="cuda")
    nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt, device="cuda")  # noqa: E731
    out, dy = nan(1, 4, dt=torch.float64), nan(1, 16, 16, 3)
    ws = ops.workspace(ops.highlight_workspace_bytes(1, 16, 16))
    nb = ops.highlight_workspace_bytes(1, 16, 16)
    bad = [dict(h=0), dict(n=0), dict(nb=nb - 8), dict(s=None), dict(y=None), dict(t=None), dict(out=None),
           dict(ws=None), dict(base=0), dict(base=7), dict(tau=1.0), dict(tau=float("nan")), dict(gain=-1.0),
           dict(gain=float("inf"))]
    for ch in bad:
        a = dict(dict(base=1, tau=0.5, gain=1.0, s=y, y=y, t=y, n=1, h=16, w=16, out=out, dy=dy, ws=ws, nb=nb), **ch)
        assert _raw(a["base"], a["tau"], a["gain"], a["s"], a["y"], a["t"], a["n"], a["h"], a["w"], a["out"], a["dy"],
                    a["ws"], a["nb"]) < 0, ch
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dy).all())
    assert _raw(1, 0.5, 1.0, y, y, y, 1, 16, 16, out, dy, ws, nb) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dy).any())


# ---------------------------------------------------------------- whole network
_NET_REF = {}
NET_GAIN = 4.0


def _net_input(shape, seed):
    """uint8-valued frames in [0, 1] (float32-exact) of which about 10 % of the pixels have max_c x >= 0.95."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 243, size=shape)  # 242 / 255 < 0.95
    hot = rng.uniform(size=shape[:3]) < 0.10
    ch = rng.integers(0, 3, size=shape[:3])
    val = rng.integers(243, 256, size=shape[:3])
    for c in range(3):
        sel = hot & (ch == c)
        x[..., c][sel] = val[sel]
    x = (x / 255.0).astype(np.float32).astype(np.float64)
    share = float((x.max(axis=-1) >= 0.95).mean())
    assert 0.05 <= share <= 0.20, share  # a condition on the inputs
    return x


def _net_reference(key, hw, P, xin, x, seed, valid_rows=None):
    """(target, prediction, loss, gradients) of the fp64 oracle; R's loss is patched by the caller's
    first patch (source 'input') or here (source 'target': the target is made from the prediction).
    xin: the (zero-padded) input of the oracle, x: its valid rows."""
    if key not in _NET_REF:
        net = R.UNetRef(P)
        y = net.forward(xin, training=True, seed=seed)
        y = y if valid_rows is None else y[:, :valid_rows]
        t = np.clip(x ** 2.2 * 1.2, 0, 1).astype(np.float32).astype(np.float64)
        if hw.base == "mae":
            t = RO.mae_safe_target(y, t)
        ref_loss, _, rg = net.backward(t, valid_rows=valid_rows)
        _NET_REF[key] = (t, y, ref_loss, rg, {k: v.copy() for k, v in P.items()})
    t, y, ref_loss, rg, P0 = _NET_REF[key]
    assert all(np.array_equal(P0[k], P[k]) for k in P0)
    return t, y, ref_loss, rg


def _check_net(m, dtype, hw, key, x, xin, seed, monkeypatch, valid_rows=None):
    """test_gpu_dssim._check_net's rule, floor runs and bounds with the oracle's loss patched to this one."""
    HR.patch_oracle(monkeypatch, R, x if hw.source == "input" else None, hw.base, hw.threshold, hw.gain)
    from test_gpu_model import randomize_bn
    P = randomize_bn(m, np.random.default_rng(21))
    t, y, ref_loss, rg = _net_reference(key, hw, P, xin, x, seed, valid_rows)
    if hw.base == "mae":  # a condition on the inputs, not a tolerance
        assert float(np.abs(y - t).min()) >= 1e-3
    if hw.source == "target":
        share = float((t.max(axis=-1) > hw.threshold).mean())
        assert 0.05 <= share, share  # the mask is not empty
    m.compile(m.optimizer, hw, ["accuracy"])
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
    print(f"{dtype} {hw!r}: loss {la[0]:.7f} rel {lerr:.2e} (floor {lfloor:.2e}); worst gradient {worst} "
          f"gpu {err[worst]:.2e} floor {floor[worst]:.2e}; max gpu rel-L2 {max(err.values()):.2e}")
    if dtype == "float32":
        assert lerr <= max(3 * lfloor, 1e-6), (lerr, lfloor)
        bad = {k: (err[k], floor[k]) for k in rg if err[k] > max(1e-4, 3 * floor[k])}
    else:
        assert lerr <= max(3 * lfloor, 5e-3), (lerr, lfloor)
        bad = {k: (err[k], floor[k]) for k in rg if err[k] > max(3 * floor[k], 2e-3)}
    assert not bad, bad
    return t


@pytest.mark.parametrize("dtype,base,source", [("float32", "mse", "input"), ("float32", "mae", "target"),
                                               ("bfloat16", "mse", "input")],
                         ids=["f32-mse-input", "f32-mae-target", "bf16-mse-input"])
def test_unet_all_74_grads(dtype, base, source, monkeypatch):
    """U-Net (64,64,3) b2, train_step(apply=False): the loss and all 74 gradients against UNetRef
    with its loss patched to the reference (grad_z = dy * y(1-y)).  The MAE base runs on a target
    kept 1e-3 away from the reference prediction."""
    m = build_unet((64, 64, 3), dtype, seed=7)
    x = _net_input((2, 64, 64, 3), 22)
    hw = C.HighlightWeighted(base, 0.95, NET_GAIN, source)
    _check_net(m, dtype, hw, (base, source), x, x, 9, monkeypatch)
    assert m._engine().iterations == 0 and m._engine().step == 1


def test_padded_frame(monkeypatch):
    """A (40,48,3) model padded to 48 rows: the training gradients equal the reference's on the 40
    valid rows (the mask from the input's valid rows), evaluate gives the reference's loss of the
    prediction and leaves the gradients alone."""
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(40, 48, 3), pad=True, dtype="float32", seed=5, verbose=False)
    x = _net_input((2, 40, 48, 3), 23)
    xin = np.concatenate([x, np.zeros((2, 8, 48, 3))], 1)
    hw = C.HighlightWeighted("mse", 0.95, NET_GAIN, "input")
    t = _check_net(m, "float32", hw, "padded", x, xin, 4, monkeypatch, valid_rows=40)
    eng = m._engine()
    eng.grads.fill_(3.0)
    ev = m.evaluate(x, t, batch_size=2)
    assert bool((eng.grads == 3.0).all())
    pred = m.predict(x)
    want = HR.loss_grad(x, pred, t, "mse", 0.95, NET_GAIN)[0][:, 2].mean()
    print(f"padded evaluate loss {ev[0]:.7f}, reference of the prediction {want:.7f}")
    assert abs(ev[0] - want) <= 1e-5
    assert abs(ev[1] - R.categorical_accuracy(t, pred)) < 1e-6


def test_gain_zero_evaluates_to_mse():
    """gain = 0: evaluate's loss is the 'mse' model's on the same weights (test_gpu_dssim.test_padded_frame's
    1e-5 absolute bound)."""
    m = build_unet((64, 64, 3), "float32", seed=12)
    x = _net_input((2, 64, 64, 3), 5)
    t = np.clip(x ** 2.2 * 1.2, 0, 1)
    m.compile("adam", C.HighlightWeighted("mse", gain=0.0), ["accuracy"])
    ev = m.evaluate(x, t, batch_size=2)
    m.compile("adam", "mse", ["accuracy"])
    ev0 = m.evaluate(x, t, batch_size=2)
    print(f"gain 0: evaluate {ev[0]:.8f}, 'mse' {ev0[0]:.8f}")
    assert abs(ev[0] - ev0[0]) <= 1e-5 and abs(ev[1] - ev0[1]) < 1e-6


def test_target_shape_mismatch_is_a_value_error():
    C.clear_session()
    m = C.TinyNet(seed=5)
    m.compile("adam", C.HighlightWeighted())
    x = torch.rand(2, 64, 64, 3, device="cuda")
    with pytest.raises(ValueError, match="HighlightWeighted loss: target of shape"):
        m._engine().train_step(x, x[:, :32], apply=False)


def test_train_step_grad_frames():
    """grad_frames = 4 with n = 2 halves dy exactly, and every gradient with it (fp32, powers of two)."""
    C.clear_session()
    m = C.TinyNet(seed=2)
    m.compile("adam", C.HighlightWeighted("mse", 0.9, 2.0))
    rng = np.random.default_rng(3)
    x = torch.tensor(rng.uniform(size=(2, 64, 64, 3)), dtype=torch.float32).cuda()
    t = torch.tensor(rng.uniform(size=(2, 64, 64, 3)), dtype=torch.float32).cuda()
    eng = m._engine()
    la = eng.train_step(x, t, apply=False).cpu().numpy()
    g = eng.grads.clone()
    la2 = eng.train_step(x, t, apply=False, grad_frames=4).cpu().numpy()
    assert np.array_equal(la, la2) and float(g.abs().max()) > 0 and torch.equal(eng.grads, 0.5 * g)


def test_other_losses_do_not_reach_the_new_kernel(monkeypatch):
    """With ops.highlight_loss_grad made to raise, models compiled with 'mse' and DSSIM('mse') train a step."""
    from cnn_itmo_amd import ops

    def boom(*a, **k):
        raise AssertionError("highlight_loss_grad on another loss's path")
    monkeypatch.setattr(ops, "highlight_loss_grad", boom)
    rng = np.random.default_rng(8)
    x, t = rng.uniform(size=(2, 64, 64, 3)), rng.uniform(size=(2, 64, 64, 3))
    for loss in ("mse", C.DSSIM("mse")):
        C.clear_session()
        m = C.TinyNet(seed=2)
        m.compile("adam", loss, ["accuracy"])
        la = m.train_on_batch(x, t)
        assert np.isfinite(la[0]) and m.iterations == 1
        assert np.isfinite(m.evaluate(x, t, batch_size=2)[0])
    C.clear_session()
    m = C.TinyNet(seed=2)
    m.compile("adam", C.HighlightWeighted())
    with pytest.raises(AssertionError, match="another loss"):
        m.train_on_batch(x, t)


# ---------------------------------------------------------------- front end
def _pairs(seed, n=4):
    x = _net_input((n, 64, 64, 3), seed)
    return x, np.clip(x ** 2.2 * 1.2, 0, 1)


def test_fit_lowers_the_loss_and_the_highlight_error():
    m = build_unet((64, 64, 3), "float32", seed=10)
    hw = C.HighlightWeighted("mae", gain=4)
    m.compile("adam", hw, ["accuracy"])
    x, t = _pairs(9)
    before = C.losses.highlight_weighted(x, m.predict(x), t, "mae", 0.95, 4.0).cpu().numpy()

    def gen():
        while True:
            yield x[:2], t[:2]
            yield x[2:], t[2:]
    h = m.fit_generator(gen(), steps_per_epoch=10, epochs=3, verbose=0)
    losses = h.history["loss"]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert m.iterations == 30
    pred = m.predict(x)
    after = C.losses.highlight_weighted(x, pred, t, "mae", 0.95, 4.0).cpu().numpy()
    print(f"H before {before[:, 3].mean():.5f} after {after[:, 3].mean():.5f}; L {before[:, 2].mean():.5f} -> "
          f"{after[:, 2].mean():.5f}; saturated share {after[:, 0].mean():.3f}")
    assert after[:, 3].mean() < before[:, 3].mean() and np.array_equal(after[:, 0], before[:, 0])
    ev = m.evaluate(x, t, batch_size=2)
    want = HR.loss_grad(x, pred.astype(np.float64), t, "mae", 0.95, 4.0)[0][:, 2].mean()
    assert abs(ev[0] - want) < 1e-5, (ev, want)
    m.set_dtype("bfloat16")
    assert m.loss is hw
    la = m.train_on_batch(x[:2], t[:2])
    assert np.isfinite(la[0]) and m.iterations == 31 and la[0] < losses[0]  # still the trained model


@pytest.mark.parametrize("ext", ["h5", "npz"])
def test_save_load_continues_bitwise(tmp_path, ext):
    """Two Adam / HighlightWeighted steps, save, load_model: one more step from the loaded model
    equals one more step from the original bit for bit."""
    m = build_unet((64, 64, 3), "float32", seed=11)
    hw = C.HighlightWeighted("mae", 0.9, 2.5, "target")
    m.compile(C.Adam(lr=2e-3, beta_1=0.8), hw, ["accuracy"])
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
    assert m2.loss == hw and m2.iterations == 2
    la2 = m2.train_on_batch(x, t)
    assert la2 == la and m2.iterations == 3 and m2.engine.step == 3
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    for sa, sb in zip(m.named_slots(), m2.named_slots()):
        assert all(np.array_equal(v, w) for v, w in zip(sa.values(), sb.values()))
