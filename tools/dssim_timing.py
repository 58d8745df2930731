"""Time the DSSIM loss (csrc/dssim.hip) and the training step that uses it.

    python tools/dssim_timing.py [--shape 8,1080,1920] [--runs 30] [--warmup 5] [--base mae]
                                 [--step-batch 8] [--step-runs 10] [--json FILE]

Kernels: cnnitmo_dssim_loss_grad in its loss-only form (the coefficient pass without planes)
and in its full form (coefficient pass storing the fp64 planes, then the gradient pass), each
timed with device events around one call: warm-up runs first, then the median and the spread
of --runs runs, the two alternating.  Their difference is what the gradient costs.

Step (--step-batch > 0): U_net(1080, 1920) pad=True in bf16, one train_step compiled with
the DSSIM loss against one compiled with 'mae' on the same model, inputs and box, the two
alternating, with the peak memory of each.  Prints one JSON line.  Needs a GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import _lib as L, ops  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "p10_p90_ms": [round(float(np.percentile(v, 10)), 4), round(float(np.percentile(v, 90)), 4)]}


def kernels(n, h, w, base, alpha, runs, warmup):
    gen = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(n, h, w, 3, device="cuda", generator=gen)
    y = (t + 0.03 * torch.randn(n, h, w, 3, device="cuda", generator=gen)).clamp_(0, 1)
    dy = torch.empty_like(y)
    out = torch.empty(n, 3, dtype=torch.float64, device="cuda")
    ws = ops.workspace(ops.dssim_workspace_bytes(n, h, w, 1))

    def call(grad):
        ops.call("cnnitmo_dssim_loss_grad", L.DSSIM_BASES[base], alpha, y.data_ptr(), t.data_ptr(), n, h, w, 0.0,
                 out.data_ptr(), dy.data_ptr() if grad else None, ws.data_ptr(), ws.numel(), ops.stream_ptr())

    for _ in range(warmup):
        call(False)
        call(True)
    torch.cuda.synchronize()
    tl, tg = [], []
    for _ in range(runs):
        tl.append(timed(lambda: call(False)))
        tg.append(timed(lambda: call(True)))
    planes = n * 3 * (h - 10) * 3 * (w - 10) * 8
    res = {"shape": [n, h, w, 3], "base": base, "alpha": alpha, "runs": runs, "warmup": warmup,
           "loss_only": stats(tl), "loss_and_grad": stats(tg), "plane_bytes": planes,
           "workspace_bytes": ws.numel()}
    print(f"cnnitmo_dssim_loss_grad on [{n},{h},{w},3] base {base}: loss only {res['loss_only']['median_ms']:.3f} ms, "
          f"with gradient {res['loss_and_grad']['median_ms']:.3f} ms (medians of {runs}); planes "
          f"{planes / 1e9:.2f} GB written and read")
    return res


def step(batch, base, alpha, runs, warmup):
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(1080, 1920, 3), pad=True, dtype="bfloat16", seed=0, verbose=False)
    eng = m._engine()
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randint(0, 256, (batch, 1080, 1920, 3), generator=g, device="cuda", dtype=torch.uint8).float() / 255.0
    t = torch.randint(0, 256, (batch, 1080, 1920, 3), generator=g, device="cuda", dtype=torch.uint8).float() / 255.0
    losses = {"mae": "mae", "dssim": C.DSSIM(base, alpha) if base else "dssim"}
    times, peak = {k: [] for k in losses}, {}
    for i in range(warmup + runs):
        for k, loss in losses.items():  # alternating, one step each
            m.compile(m.optimizer, loss, ["accuracy"])
            torch.cuda.reset_peak_memory_stats()
            ms = timed(lambda: eng.train_step(x, t, seed=i, optimizer=m.optimizer))
            if i >= warmup:
                times[k].append(ms)
                peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
    res = {"batch": batch, "dtype": "bfloat16", "runs": runs, "warmup": warmup,
           "mae_step": stats(times["mae"]), "dssim_step": stats(times["dssim"]),
           "peak_mem_gib": {k: round(v / 2 ** 30, 2) for k, v in peak.items()}}
    print(f"1080p bf16 step, batch {batch}: mae {res['mae_step']['median_ms']:.2f} ms, "
          f"DSSIM({base!r}) {res['dssim_step']['median_ms']:.2f} ms; peak memory {res['peak_mem_gib']} GiB")
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", default="8,1080,1920", help="n,h,w of the kernel timing")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--base", default="mae", choices=["none", "mae", "mse"])
    ap.add_argument("--alpha", type=float, default=0.84)
    ap.add_argument("--step-batch", type=int, default=0, help="also time the 1080p bf16 step at this batch (0: no)")
    ap.add_argument("--step-runs", type=int, default=10)
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args(argv)
    n, h, w = (int(v) for v in a.shape.split(","))
    if a.runs < 20:
        ap.error("--runs: at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("dssim_timing: needs a GPU")
    base = None if a.base == "none" else a.base
    alpha = 1.0 if base is None else a.alpha
    res = {"kernels": kernels(n, h, w, base, alpha, a.runs, a.warmup)}
    if a.step_batch > 0:
        res["step"] = step(a.step_batch, base, alpha, a.step_runs, a.step_warmup)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
