"""bench.py's command line: a plain run does the headline steps only, ``--full`` adds the
rest, ``--steps`` sets the number of timed steps and ``--dump-outputs`` writes what the last
of them computed.

The GPU tests call ``bench.main`` in this process on two 48x80 frames (3x5 at the U-Net's
deepest level; the command line's logic does not depend on the frame size) and replay the same
seeded inputs and step seeds through the engine by hand: the library is bitwise
deterministic (test_gpu_determinism.py), so the dumped arrays must equal the replay exactly,
and a run of one step more or fewer would not."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, B = 48, 80, 2
SHAPE = ["--height", str(H), "--width", str(W), "--batch", str(B)]
FULL_ONLY = ("roofline", "cpu_baseline", "fp32_infer", "fp32_infer_b32", "k4_train", "fp32_train",
             "replicas", "allreduce_exposed")


def test_options():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "some/dir"])
    assert a.full is True and a.dump_outputs == "some/dir"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    # a whole output may be dumped only while the dump stays under 64 MB
    assert 4 * bench.DUMP_SAMPLE < 64e6


def _run(argv, capsys):
    import bench
    import cnn_itmo_amd as C
    C.clear_session()
    capsys.readouterr()
    bench.main(argv)
    C.clear_session()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _inputs(torch):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    x = torch.randint(0, 256, (B, H, W, 3), generator=g, device="cuda", dtype=torch.uint8).float() / 255.0
    t = torch.randint(0, 256, (B, H, W, 3), generator=g, device="cuda", dtype=torch.uint8).float() / 255.0
    return x, t


def _model(dtype):
    import cnn_itmo_amd as C
    C.clear_session()
    with contextlib.redirect_stdout(io.StringIO()):
        return C.U_net(input_size=(H, W, 3), pad=True, dtype=dtype, seed=0, verbose=False)


@pytest.mark.gpu
def test_plain_run_dumps_last_timed_step(tmp_path, capsys):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    steps, warmup = 3, 2
    outs = []
    for d in ("a", "b"):
        res = _run(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs",
                    str(tmp_path / d)] + SHAPE, capsys)
        assert res["steps"] == steps and res["warmup"] == warmup and res["dtype"] == "bf16"
        assert res["unit"] == "frames/s" and res["higher_is_better"] is True
        assert res["metric"] == f"{W}x{H} SDR->HDR frames/sec (fwd+bwd)"
        assert res["ms_per_step"] > 0
        # value and ms_per_step describe the same timed steps (each is rounded on its own)
        assert res["value"] == pytest.approx(B / (res["ms_per_step"] * 1e-3), rel=0.05)
        assert not [k for k in FULL_ONLY if k in res]
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["bufs.npy", "loss_acc.npy", "params.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= 64e6
        outs.append({f[:-4]: np.load(tmp_path / d / f) for f in files})
    for k, v in outs[0].items():
        assert v.dtype == np.float32 and np.isfinite(v).all()
        assert np.array_equal(v, outs[1][k]), k  # same arguments: same inputs, same outputs
    # the replay: warmup + steps training steps with bench.py's seeds
    m = _model("bfloat16")
    e, opt = m._engine(), m.optimizer
    x, t = _inputs(torch)
    p_before = None
    for i in range(warmup + steps):
        if i == warmup + steps - 1:
            p_before = e.params.clone()
        la = e.train_step(x, t, seed=i, lr=opt.lr, rho=opt.rho, eps=opt.epsilon)
    assert np.array_equal(outs[0]["loss_acc"], la.cpu().numpy())
    assert np.array_equal(outs[0]["params"], e.params.cpu().numpy())
    assert np.array_equal(outs[0]["bufs"], e.bufs.cpu().numpy())
    assert not torch.equal(p_before, e.params)  # (one step fewer would have been told apart)
    import cnn_itmo_amd as C
    C.clear_session()


@pytest.mark.gpu
def test_infer_dump_is_a_fixed_sample(tmp_path, capsys, monkeypatch):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bench
    n = B * H * W * 3
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)  # the output (23040 values) is above it: sampled
    argv = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--mode", "infer", "--dtype", "float32"] + SHAPE
    res = _run(argv + ["--dump-outputs", str(tmp_path / "s")], capsys)
    assert res["metric"] == f"{W}x{H} SDR->HDR frames/sec (fwd)" and res["dtype"] == "f32"
    assert not [k for k in FULL_ONLY if k in res]
    monkeypatch.setattr(bench, "DUMP_SAMPLE", n)  # at the limit: dumped whole
    _run(argv + ["--dump-outputs", str(tmp_path / "w")], capsys)
    ys, yw = np.load(tmp_path / "s" / "yhat.npy"), np.load(tmp_path / "w" / "yhat.npy")
    assert ys.dtype == yw.dtype == np.float32 and ys.shape == (1000,) and yw.shape == (B, H, W, 3)
    idx = np.sort(np.random.default_rng(0).integers(0, n, size=1000))
    assert np.array_equal(ys, yw.reshape(-1)[idx])
    e = _model("float32")._engine()
    x, _ = _inputs(torch)
    y = torch.empty(B, H, W, 3, device="cuda", dtype=torch.float32)
    e.predict_into(x, y)
    assert np.array_equal(yw, y.cpu().numpy())
    import cnn_itmo_amd as C
    C.clear_session()


@pytest.mark.gpu
def test_full_run_keeps_the_other_figures(capsys):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cnn_itmo_amd import ops
    saved = {k: v for k, v in vars(ops).items() if callable(v)}
    try:  # --full wraps the ops' entry points for its instrumented pass: undo that for later tests
        res = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu", "--infer-batch", "1",
                    "--ns-batch", "0", "--k4-batch", "0", "--f32-train-batch", "1", "--f32-train-steps", "1",
                    "--f32-train-warmup", "1"] + SHAPE, capsys)
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["roofline"]["kernel"] and res["config"]["gflop_per_frame"] > 0
    assert res["cpu_baseline"] is None  # --no-cpu
    for leg in ("fp32_infer", "fp32_train"):
        assert "roofline" in res[leg] and "error" not in res[leg], res[leg]
    assert "k4_train" not in res and "fp32_infer_b32" not in res
