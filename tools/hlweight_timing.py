"""Time the training step compiled with the highlight-weighted loss (csrc/hlweight.hip).

    python tools/hlweight_timing.py [--batch 32] [--runs 10] [--warmup 2] [--only-highlight] [--json FILE]

U_net(1080, 1920) pad=True in bf16: one train_step compiled with HighlightWeighted('mse') against
one compiled with DSSIM('mse') and one with 'mse' on the same model and inputs, alternating, each
timed with device events; the inputs are uint8-valued frames of which about 10 % of the pixels are
saturated.  Prints the bytes the loss kernel has to move (36 B read + 12 B written per pixel) and
one JSON line.  --only-highlight runs the HighlightWeighted steps alone: the form to put under
`rocprofv3 --kernel-trace --stats`, whose highlight_kernel row over those bytes is the kernel's
achieved bandwidth.  Needs a GPU.
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

BYTES_PER_PIXEL = 48  # s, y, t read (3 x 12 B), dy written (12 B)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def frames(batch, g):
    x = torch.randint(0, 243, (batch, 1080, 1920, 3), generator=g, device="cuda", dtype=torch.uint8)
    hot = torch.rand(batch, 1080, 1920, generator=g, device="cuda") < 0.10
    x[..., 0][hot] = 255
    return x.float() / 255.0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only-highlight", action="store_true")
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("hlweight_timing: needs a GPU")
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(1080, 1920, 3), pad=True, dtype="bfloat16", seed=0, verbose=False)
    eng = m._engine()
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = frames(a.batch, g)
    t = (x ** 2.2 * 1.2).clamp_(0, 1)
    losses = {"highlight": C.HighlightWeighted("mse")}
    if not a.only_highlight:
        losses.update({"dssim": C.DSSIM("mse"), "mse": "mse"})
    times = {k: [] for k in losses}
    for i in range(a.warmup + a.runs):
        for k, loss in losses.items():  # alternating, one step each
            m.compile(m.optimizer, loss, ["accuracy"])
            ms = timed(lambda: eng.train_step(x, t, seed=i, optimizer=m.optimizer))
            if i >= a.warmup:
                times[k].append(ms)
    nbytes = a.batch * 1080 * 1920 * BYTES_PER_PIXEL
    res = {"batch": a.batch, "dtype": "bfloat16", "runs": a.runs, "warmup": a.warmup, "loss_kernel_bytes": nbytes,
           "saturated_share": round(float((x.amax(dim=-1) >= 0.95).float().mean()), 4),
           "step": {k: stats(v) for k, v in times.items()}}
    print(f"1080p bf16 step, batch {a.batch}: " + ", ".join(f"{k} {v['median_ms']:.2f} ms" for k, v in res["step"].items())
          + f"; the highlight kernel moves {nbytes / 1e9:.2f} GB")
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
