"""Gradient clipping on the GPU (cnnitmo_grad_sumsq / cnnitmo_grad_clip, csrc/gradclip.hip) against
tests/gradclip_ref.py, the clipped optimizers end to end, the training-control callbacks through
fit_generator, and both under data parallelism (tools/dp_controls.py).

Operands come from a poisoned arena (tests/arena.py): guards before and after every buffer, the
gradient once 16-byte aligned and once one float further (the dword path)."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gradclip_ref as GR  # noqa: E402
import ref_objectives as RO  # noqa: E402
from arena import Arena, poison_count  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNET_PARAMS = 11159011
# 1 .. 1025: the issue's list; 4095 .. 4097 and 8191 .. 8193: one workgroup's span of grad_clip (4096) and of
# grad_sumsq (8192), where the unchecked 16-byte path hands over to the checked one; 12388: ends inside the
# second workgroup's span; 300001: 37 / 74 workgroups and a ragged tail
SMALL = [1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12388, 300001]

_CASES = {}  # n -> (values, reference sum): computed once, read only


def case(n):
    """n fp32 values of both signs spread over 60 binades (2^-40 .. 2^20), and their exact sum of squares."""
    if n not in _CASES:
        rng = np.random.default_rng(1000 + n % 997)
        v = (np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-40, 20, n)) * rng.choice([-1.0, 1.0], n))
        v = v.astype(np.float32)
        v.setflags(write=False)
        _CASES[n] = (v, GR.sumsq(v))
    return _CASES[n]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Placed:
    """A gradient vector inside an arena, `off` floats past a 16-byte boundary, with the sumsq workspace, its
    output and a sumsq input next to it."""

    def __init__(self, vals, off):
        from cnn_itmo_amd import ops
        n = len(vals)
        self.n, self.off = n, off
        wsb = ops.grad_sumsq_workspace_bytes(n)
        self.arena = A = Arena(4 * (n + off) + wsb + 5 * (1 << 20) + 4096, device="cuda")
        self.whole = A.take(n + off, torch.float32, name="g")
        self.whole[off:].copy_(torch.tensor(vals))
        self.g = self.whole[off:]
        assert self.g.data_ptr() % 16 == 4 * off
        self.ws = A.take(wsb, torch.uint8, name="ws")
        self.out = A.take(1, torch.float64, name="out")
        self.S = A.take(1, torch.float64, data=np.zeros(1), name="S")

    def check(self):
        self.arena.check_untouched()
        assert poison_count(self.whole[:self.off]) == self.off  # the floats before a misaligned start


# ---- grad_sumsq ------------------------------------------------------------------------------------
def _check_sumsq(n):
    from cnn_itmo_amd import ops
    vals, ref = case(n)
    got = []
    for off in (0, 1):
        P = Placed(vals, off)
        assert poison_count(P.out) == 1
        r = ops.grad_sumsq(P.g, out=P.out, ws=P.ws)
        assert r is P.out
        a = float(P.out.cpu()[0])
        P.ws.fill_(0xFF)  # the workspace's contents are irrelevant: poison it again and repeat
        ops.grad_sumsq(P.g, out=P.out, ws=P.ws)
        b = float(P.out.cpu()[0])
        P.check()
        assert np.array_equal(P.g.cpu().numpy(), vals)  # the input is read only
        rel = abs(a - ref) / ref
        print(f"n {n} off {off}: sumsq {a!r} reference {ref!r} rel {rel:.3e} (bound {n * 2.0 ** -53:.3e})")
        # every square is exact in fp64; n - 1 additions each round by <= 2^-53 relative, and the reference is the
        # exact sum rounded once: n * 2^-53 in all
        assert rel <= n * 2.0 ** -53, (n, off, a, ref, rel)
        assert a == b, (n, off, a, b)  # bit for bit: two runs
        got.append(a)
    assert got[0] == got[1], (n, got)  # and the aligned and the dword path (same element -> thread map)
    # the default workspace / output path
    assert float(ops.grad_sumsq(torch.tensor(vals).cuda()).cpu()[0]) == got[0]


@pytest.mark.parametrize("n", SMALL)
def test_grad_sumsq(n):
    _check_sumsq(n)


def test_grad_sumsq_unet_size():
    _check_sumsq(UNET_PARAMS)


def test_grad_sumsq_nonfinite_and_zero():
    from cnn_itmo_amd import ops
    z = torch.zeros(9000, device="cuda")
    assert float(ops.grad_sumsq(z).cpu()[0]) == 0.0
    z[8999] = float("inf")
    assert float(ops.grad_sumsq(z).cpu()[0]) == float("inf")
    z[17] = float("nan")
    assert np.isnan(float(ops.grad_sumsq(z).cpu()[0]))
    big = torch.full((5,), 3e38, device="cuda")  # squares beyond fp32, far inside fp64
    assert float(ops.grad_sumsq(big).cpu()[0]) == 5 * float(np.float64(np.float32(3e38)) ** 2)


# ---- grad_clip -------------------------------------------------------------------------------------
def _clip_cases(vals, S):
    """name -> (S fed, grad_scale, clipnorm, clipvalue); N = grad_scale * sqrt(S) in fp64."""
    N = float(np.sqrt(np.float64(S)))
    med = float(np.median(np.abs(vals)))
    third = 1.0 / 3.0
    N3 = float(np.float64(third) * np.sqrt(np.float64(S)))
    return {
        "norm": (S, 1.0, 0.5 * N, 0.0),
        "value": (None, 1.0, 0.0, med),
        "both": (S, 1.0, 0.37 * N, 0.37 * med),       # value after norm: bites on the scaled values
        "norm_just_below": (S, 1.0, float(np.nextafter(N, np.inf)), 0.0),   # N < clipnorm: unchanged
        "norm_equal": (S, 1.0, N, 0.0),                                     # N >= clipnorm, f = 1
        "norm_just_above": (S, 1.0, float(np.nextafter(N, 0.0)), 0.0),      # N > clipnorm by one ulp
        "grad_scale_half": (S, 0.5, 0.25 * N, 0.3 * med),
        "grad_scale_third": (S, third, 0.5 * N3, 2.0 * med),
        "grad_scale_third_below": (S, third, float(np.nextafter(N3, np.inf)), 0.0),
        "S_inf": (float("inf"), 1.0, 0.5 * N, med),   # no norm clipping; the value clip still applies
        "S_nan": (float("nan"), 1.0, 0.5 * N, 0.0),
    }


def _check_clip(n, names=None):
    from cnn_itmo_amd import ops
    vals, S = case(n)
    for name, (Sfed, gs, cn, cv) in _clip_cases(vals, S).items():
        if names and name not in names:
            continue
        ref = GR.clip(vals, Sfed, gs, cn, cv)
        if name in ("norm_just_below", "grad_scale_third_below", "S_nan"):
            assert np.array_equal(bits(ref), bits(vals))
        if name == "norm":
            assert not np.array_equal(bits(ref), bits(vals))
        for off in (0, 1):
            P = Placed(vals, off)
            sumsq = None
            if Sfed is not None:
                P.S.fill_(Sfed)
                sumsq = P.S
            assert ops.grad_clip(P.g, sumsq, gs, cn, cv) is P.g
            P.check()
            got = P.g.cpu().numpy()
            bad = np.flatnonzero(bits(got) != bits(ref))
            assert bad.size == 0, (n, name, off, bad[:5], got[bad[:5]], ref[bad[:5]], vals[bad[:5]])
            if Sfed is not None:
                assert float(P.S.cpu()[0]) == Sfed or np.isnan(Sfed)  # read only


@pytest.mark.parametrize("n", SMALL)
def test_grad_clip_bit_for_bit(n):
    _check_clip(n)


def test_grad_clip_unet_size():
    _check_clip(UNET_PARAMS, names=("both",))


def test_grad_clip_keeps_nan_and_clamps_inf():
    from cnn_itmo_amd import ops
    v = np.array([3.0, np.nan, -np.inf, np.inf, -0.0, 0.25, -7.0], np.float32)
    for off in (0, 1):
        P = Placed(v, off)
        ops.grad_clip(P.g, None, 1.0, 0.0, 2.0)
        P.check()
        got = P.g.cpu().numpy()
        assert np.isnan(got[1])
        assert np.array_equal(bits(np.delete(got, 1)), bits([2.0, -2.0, 2.0, -0.0, 0.25, -2.0]))
        ref = GR.clip(v, None, 1.0, 0.0, 2.0)
        assert np.isnan(ref[1]) and np.array_equal(bits(np.delete(ref, 1)), bits(np.delete(got, 1)))


def test_sumsq_then_clip_gives_the_norm():
    """The two kernels chained as the optimizers chain them: afterwards the norm is clipnorm."""
    from cnn_itmo_amd import ops
    vals, S = case(300001)
    g = torch.tensor(vals).cuda()
    cn = 0.25 * float(np.sqrt(S))
    ops.grad_clip(g, ops.grad_sumsq(g), 1.0, cn, 0.0)
    after = float(np.sqrt(float(ops.grad_sumsq(g).cpu()[0])))
    assert abs(after - cn) <= 1e-6 * cn, (after, cn)  # each element rounded to fp32 once: 2^-24 relative


# ---- end to end: a clipped optimizer step ------------------------------------------------------------
def _net(kind, dtype):
    import cnn_itmo_amd as C
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "tiny":
            return C.TinyNet(dtype=dtype, seed=2), 64
        return C.U_net(input_size=(32, 32, 3), dtype=dtype, seed=4), 32


def _one_step(kind, dtype, opt, x, t, apply=True):
    """A fresh model: one train_step -> (params before, params after, gradient buffer after), fp32 host copies."""
    m, _ = _net(kind, dtype)
    m.compile(opt, "mse", ["accuracy"])
    eng = m._engine()
    p0 = eng.params.cpu().numpy().copy()
    eng.train_step(x, t, optimizer=opt, apply=apply)
    torch.cuda.synchronize()
    assert eng.iterations == int(apply)
    return p0, eng.params.cpu().numpy().copy(), eng.grads.cpu().numpy().copy()


@pytest.mark.parametrize("kind,dtype", [("tiny", "float32"), ("tiny", "bfloat16"), ("unet", "float32"),
                                        ("unet", "bfloat16")])
def test_clipped_optimizer_step(kind, dtype):
    """The raw gradients G of one batch (train_step(apply=False)), then fresh identical models take one step
    with RMSprop / Adam / SGD(momentum) clipping at half of ||G|| and at a value that still bites afterwards:
    the parameters equal ref_objectives' fp64 update of the clipped G (atol 1e-6, test_gpu_losses' bound for
    optimizer steps).  A clipnorm above ||G|| leaves the step bit-identical to the unclipped optimizer's."""
    import cnn_itmo_amd as C
    size = 64 if kind == "tiny" else 32
    rng = np.random.default_rng(31)
    x = torch.tensor(rng.uniform(size=(2, size, size, 3)), dtype=torch.float32).cuda()
    t = torch.tensor(rng.uniform(size=(2, size, size, 3)), dtype=torch.float32).cuda()
    p0, p_same, G = _one_step(kind, dtype, C.RMSprop(), x, t, apply=False)
    assert np.array_equal(p0, p_same)
    norm = float(np.sqrt(GR.sumsq(G)))
    assert np.isfinite(norm) and norm > 0
    cn = 0.5 * norm
    cv = 0.25 * float(np.abs(G).max()) * 0.5  # a quarter of the largest entry after the norm clip
    Gc = GR.clip(G, GR.sumsq(G), 1.0, cn, cv)
    assert np.count_nonzero(np.abs(Gc) == np.float32(cv)) > 0 and np.count_nonzero(np.abs(Gc) < np.float32(cv)) > 0
    P, g = p0.astype(np.float64), Gc.astype(np.float64)
    zero = np.zeros_like(P)
    expect = {"rmsprop": (C.RMSprop(clipnorm=cn, clipvalue=cv), RO.rmsprop(P, g, zero)[0]),
              "adam": (C.Adam(clipnorm=cn, clipvalue=cv), RO.adam(P, g, zero, zero, 0)[0]),
              "sgd": (C.SGD(momentum=0.9, clipnorm=cn, clipvalue=cv), RO.sgd(P, g, zero, momentum=0.9)[0])}
    for name, (opt, exp) in expect.items():
        q0, q, gbuf = _one_step(kind, dtype, opt, x, t)
        assert np.array_equal(q0, p0)
        # the buffer the update read: the clipped gradient (the device's own sum differs from the reference's
        # in the last bits of fp64, far below fp32's)
        np.testing.assert_allclose(gbuf, Gc, rtol=1e-6, atol=0, err_msg=name)
        err = float(np.abs(q - exp).max())
        print(f"{kind} {dtype} {name}: ||G|| {norm:.4e} clipnorm {cn:.4e} clipvalue {cv:.4e} max |p - ref| {err:.3e}")
        np.testing.assert_allclose(q, exp, atol=1e-6, rtol=0, err_msg=name)
        assert float(np.abs(q - p0).max()) > 0
    # above the norm: f = 1, every element passes through (float)((double)g * 1.0) unchanged
    _, plain, _ = _one_step(kind, dtype, C.RMSprop(), x, t)
    _, above, gbuf = _one_step(kind, dtype, C.RMSprop(clipnorm=2.0 * norm), x, t)
    assert np.array_equal(bits(gbuf), bits(G))
    assert np.array_equal(bits(above), bits(plain))
    _, clipped, _ = _one_step(kind, dtype, C.RMSprop(clipnorm=cn), x, t)
    assert not np.array_equal(bits(clipped), bits(plain))


# ---- fit_generator with the callbacks -----------------------------------------------------------------
def test_fit_generator_reduce_lr_csv_early_stopping(tmp_path):
    """min_delta = 10 on a loss below 1: after epoch 0 (which improves on inf) no epoch improves, whatever the
    data.  By hand, ReduceLROnPlateau(factor 0.5, patience 1): epoch 1, 2, 3 halve lr = 1e-3; the epochs ran
    with 1e-3, 1e-3, 5e-4, 2.5e-4 (logs['lr']); EarlyStopping(patience 3): wait 1, 2, 3 -> stops at epoch 3 of
    6 with lr = 1.25e-4, which the checkpoint of that epoch carries."""
    import cnn_itmo_amd as C
    m, size = _net("unet", "float32")
    m.compile(C.RMSprop(lr=1e-3, clipnorm=1.0), "mse", ["accuracy"])
    rng = np.random.default_rng(5)
    x = rng.uniform(size=(4, size, size, 3)).astype(np.float32)
    y = rng.uniform(size=(4, size, size, 3)).astype(np.float32)

    def gen():
        while True:
            yield x[:2], y[:2]
            yield x[2:], y[2:]

    trace = []
    log = str(tmp_path / "log.csv")
    ck = str(tmp_path / "ck{epoch}.h5")
    rl = C.ReduceLROnPlateau(monitor="loss", factor=0.5, patience=1, min_delta=10.0)
    es = C.EarlyStopping(monitor="loss", min_delta=10.0, patience=3)
    h = m.fit_generator(gen(), steps_per_epoch=2, epochs=6, verbose=0, validation_data=(x, y),
                        callbacks=[rl, C.LambdaCallback(on_epoch_end=lambda e, logs: trace.append(logs["lr"])),
                                   C.CSVLogger(log), es, C.ModelCheckpoint(ck)])
    ran = [1e-3, 1e-3, 5e-4, 2.5e-4]
    assert trace == ran and h.history["lr"] == ran and h.epoch == [0, 1, 2, 3]
    assert sorted(h.history) == ["acc", "loss", "lr", "val_acc", "val_loss"]
    assert all(len(v) == 4 for v in h.history.values()) and np.isfinite(h.history["loss"]).all()
    assert m.stop_training and es.stopped_epoch == 3 and es.wait == 3
    assert m.optimizer.lr == 1.25e-4 and m.iterations == 8
    with open(log) as f:
        rows = [ln.split(",") for ln in f.read().split()]
    assert rows[0] == ["epoch", "acc", "loss", "lr", "val_acc", "val_loss"]
    assert [float(r[3]) for r in rows[1:]] == ran
    assert [float(r[2]) for r in rows[1:]] == h.history["loss"]
    assert sorted(os.listdir(tmp_path)) == ["ck1.h5", "ck2.h5", "ck3.h5", "ck4.h5", "log.csv"]
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        m2 = C.load_model(str(tmp_path / "ck4.h5"))
    assert m2.optimizer.lr == 1.25e-4 and m2.optimizer.clipnorm == 1.0
    assert m2.optimizer.get_config() == m.optimizer.get_config()


def test_fit_generator_scheduler_and_terminate_on_nan():
    """LearningRateScheduler sets the rate before each epoch; a rate of inf makes the parameters, hence the
    next epoch's loss, non-finite, and TerminateOnNaN stops there (its epoch-end check)."""
    import cnn_itmo_amd as C
    m, size = _net("tiny", "float32")
    m.compile(C.SGD(lr=0.01), "mse", ["accuracy"])
    rng = np.random.default_rng(6)
    x = rng.uniform(size=(2, size, size, 3)).astype(np.float32)
    sched = [0.01, 0.005, float("inf"), 0.01, 0.01]
    h = m.fit_generator(iter(lambda: (x, x), None), steps_per_epoch=1, epochs=5, verbose=0,
                        callbacks=[C.LearningRateScheduler(lambda e: sched[e]), C.TerminateOnNaN()])
    assert h.history["lr"] == sched[:len(h.history["lr"])]
    assert m.stop_training and 3 <= len(h.epoch) <= 4 and not np.isfinite(h.history["loss"][-1])
    assert np.isfinite(h.history["loss"][:2]).all()


# ---- data parallel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_dp_two_ranks_lr_sync_and_clipnorm(dtype):
    """tools/dp_controls.py, launched as test_gpu_dist launches dp_rehearsal: two ranks on one GPU over gloo."""
    port = str(30400 + (os.getpid() % 200) + (300 if dtype == "bfloat16" else 0))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.join(ROOT, "tools", "dp_controls.py")]
    env = dict(os.environ, CNNITMO_DEVICE="0", CNNITMO_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0",
               DTYPE=dtype)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "scheduler: ranks identical" in r.stdout and "restore: ranks identical" in r.stdout, r.stdout
    print("\n".join(r.stdout.strip().splitlines()[-2:]))
