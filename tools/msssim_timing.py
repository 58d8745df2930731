"""Time the multi-scale SSIM loss (csrc/msssim.hip) against the single-scale DSSIM loss
(csrc/dssim.hip), and the training steps that use them.

    python tools/msssim_timing.py [--shape 32,1080,1920] [--runs 30] [--warmup 5] [--base mae]
                                  [--scales 5] [--step-batch 8] [--step-runs 10] [--json FILE]

Kernels: cnnitmo_msssim_loss_grad (loss and gradient, and the loss-only form) and
cnnitmo_dssim_loss_grad with the same arguments on the same images, each timed with device events
around one call: warm-up runs first, then the median and the spread of --runs runs, the entries
alternating.  The coarser levels hold a third of level 0's pixels, so 4/3 of DSSIM's time plus the
pyramid passes is what to expect; the printed ratio says how far off that is.

Step (--step-batch > 0): U_net(1080, 1920) pad=True in bf16, one train_step compiled with
MSSSIM(base) against one compiled with DSSIM(base) on the same model, inputs and box, the two
alternating, with the peak memory of each.  Prints one JSON line.  Needs a GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import _lib as L, losses, ops  # noqa: E402
from dssim_timing import stats, timed  # noqa: E402


def kernels(n, h, w, base, alpha, scales, runs, warmup):
    gen = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(n, h, w, 3, device="cuda", generator=gen)
    y = (t + 0.03 * torch.randn(n, h, w, 3, device="cuda", generator=gen)).clamp_(0, 1)
    dy = torch.empty_like(y)
    wts = losses.MSSSIM_WEIGHTS[:scales]
    out = torch.empty(n, 3 + 3 * scales, dtype=torch.float64, device="cuda")
    out3 = torch.empty(n, 3, dtype=torch.float64, device="cuda")
    nb = {"msssim": ops.msssim_workspace_bytes(n, h, w, scales, 1), "dssim": ops.dssim_workspace_bytes(n, h, w, 1)}
    calls = {"msssim": lambda: ops.msssim_loss_grad(L.DSSIM_BASES[base], alpha, wts, y, t, dy, out=out),
             "msssim_loss_only": lambda: ops.msssim_loss_grad(L.DSSIM_BASES[base], alpha, wts, y, t, out=out),
             "dssim": lambda: ops.dssim_loss_grad(L.DSSIM_BASES[base], alpha, y, t, dy, out=out3)}
    # (the wrappers take their workspace from torch's caching allocator: warm after the first call)
    for _ in range(warmup):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(runs):
        for k, f in calls.items():
            times[k].append(timed(f))
    res = {"shape": [n, h, w, 3], "base": base, "alpha": alpha, "scales": scales, "runs": runs, "warmup": warmup,
           "workspace_bytes": nb, "workspace_bytes_per_pixel": {k: round(v / (n * h * w), 2) for k, v in nb.items()}}
    res.update({k: stats(v) for k, v in times.items()})
    ratio = res["msssim"]["median_ms"] / res["dssim"]["median_ms"]
    res["msssim_over_dssim"] = round(ratio, 3)
    print(f"[{n},{h},{w},3] base {base}: cnnitmo_msssim_loss_grad ({scales} scales) {res['msssim']['median_ms']:.3f} ms "
          f"(loss only {res['msssim_loss_only']['median_ms']:.3f} ms), cnnitmo_dssim_loss_grad "
          f"{res['dssim']['median_ms']:.3f} ms: x{ratio:.2f} (4/3 expected); workspace "
          f"{nb['msssim'] / 2 ** 30:.2f} GiB against {nb['dssim'] / 2 ** 30:.2f} GiB")
    return res


def step(batch, base, alpha, scales, runs, warmup):
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(1080, 1920, 3), pad=True, dtype="bfloat16", seed=0, verbose=False)
    eng = m._engine()
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randint(0, 256, (batch, 1080, 1920, 3), generator=g, device="cuda", dtype=torch.uint8).float() / 255.0
    t = torch.randint(0, 256, (batch, 1080, 1920, 3), generator=g, device="cuda", dtype=torch.uint8).float() / 255.0
    compiled = {"dssim": C.DSSIM(base, alpha), "msssim": C.MSSSIM(base, alpha, losses.MSSSIM_WEIGHTS[:scales])}
    times, peak = {k: [] for k in compiled}, {}
    for i in range(warmup + runs):
        for k, loss in compiled.items():  # alternating, one step each
            m.compile(m.optimizer, loss, ["accuracy"])
            torch.cuda.reset_peak_memory_stats()
            ms = timed(lambda: eng.train_step(x, t, seed=i, optimizer=m.optimizer))
            if i >= warmup:
                times[k].append(ms)
                peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
    res = {"batch": batch, "dtype": "bfloat16", "runs": runs, "warmup": warmup,
           "dssim_step": stats(times["dssim"]), "msssim_step": stats(times["msssim"]),
           "peak_mem_gib": {k: round(v / 2 ** 30, 2) for k, v in peak.items()}}
    print(f"1080p bf16 step, batch {batch}: DSSIM({base!r}) {res['dssim_step']['median_ms']:.2f} ms, "
          f"MSSSIM({base!r}) {res['msssim_step']['median_ms']:.2f} ms; peak memory {res['peak_mem_gib']} GiB")
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", default="32,1080,1920", help="n,h,w of the kernel timing")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--base", default="mae", choices=["none", "mae", "mse"])
    ap.add_argument("--alpha", type=float, default=0.84)
    ap.add_argument("--scales", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=0, help="also time the 1080p bf16 step at this batch (0: no)")
    ap.add_argument("--step-runs", type=int, default=10)
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args(argv)
    n, h, w = (int(v) for v in a.shape.split(","))
    if a.runs < 20:
        ap.error("--runs: at least 20")
    if not 1 <= a.scales <= 5:
        ap.error("--scales: 1..5")
    if not torch.cuda.is_available():
        raise SystemExit("msssim_timing: needs a GPU")
    base = None if a.base == "none" else a.base
    alpha = 1.0 if base is None else a.alpha
    res = {"kernels": kernels(n, h, w, base, alpha, a.scales, a.runs, a.warmup)}
    if a.step_batch > 0:
        res["step"] = step(a.step_batch, base, alpha, a.scales, a.step_runs, a.step_warmup)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
