"""Cost of gradient clipping on the GPU: the two kernels alone, and a training step with and without it.

  python tools/gradclip_time.py [--n 11159011] [--runs 50] [--height 1080 --width 1920 --batch 32
                                 --dtype bfloat16 --steps 8 --rounds 3] [--no-step]

Kernels: cnnitmo_grad_sumsq (both launches) and cnnitmo_grad_clip (norm and value) on n fp32, timed one
call at a time with device events after a warm-up; the median, minimum and maximum of `runs` calls.
Twice: on one buffer (44.6 MB at the U-Net's n: it stays in the 256 MiB last-level cache, as the
gradients a backward pass has just written partly do), and rotating over enough buffers to exceed that
cache (every call reads from HBM).  GB/s counts 4 B per element for sumsq and 8 B for clip.

Step: Engine.train_step on random frames, RMSprop without and with clipnorm (set far above the norm, so
that the parameters stay the same and only the two extra kernels differ), in alternating blocks of
`steps` steps, `rounds` times; per variant the median over blocks of the block's mean step time, and
the spread of the unclipped blocks, which is the noise a difference has to exceed.
Prints one JSON line.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cnn_itmo_amd as C  # noqa: E402
from cnn_itmo_amd import ops  # noqa: E402


def timed(fn, bufs, runs, warmup=10):
    """fn(buffer) over the buffers in turn -> sorted per-call times in microseconds."""
    for i in range(warmup):
        fn(bufs[i % len(bufs)])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(bufs[i % len(bufs)])
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)


def stats(us, nbytes):
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2),
            "gb_per_s": round(nbytes / med / 1e3, 1)}


def kernels(n, runs):
    out = {"n": n, "runs": runs}
    ws = ops.workspace(ops.grad_sumsq_workspace_bytes(n))
    S = torch.empty(1, dtype=torch.float64, device="cuda")
    nbuf = max(2, -(-(320 << 20) // (4 * n)))  # > 256 MiB in all
    for label, count in (("one_buffer", 1), ("rotating", nbuf)):
        bufs = [torch.randn(n, device="cuda") for _ in range(count)]
        ops.grad_sumsq(bufs[0], out=S, ws=ws)
        # clipnorm below the norm and a value bound: the multiply and both compares run; the data shrink by at
        # most 2^-30 per call, so they stay normal numbers over the runs
        norm = float(S.cpu()[0]) ** 0.5
        out[label] = {
            "buffers": count,
            "grad_sumsq": stats(timed(lambda g: ops.grad_sumsq(g, out=S, ws=ws), bufs, runs), 4 * n),
            "grad_clip": stats(timed(lambda g: ops.grad_clip(g, S, 1.0, norm * (1 - 2.0 ** -30), 1e30), bufs, runs),
                               8 * n),
        }
        del bufs
    return out


def step(args):
    with contextlib.redirect_stdout(io.StringIO()):
        m = C.U_net(input_size=(args.height, args.width, 3), pad=True, dtype=args.dtype, seed=0, verbose=False)
    eng = m._engine()
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    x = torch.rand(args.batch, args.height, args.width, 3, device="cuda", generator=g)
    t = torch.rand(args.batch, args.height, args.width, 3, device="cuda", generator=g)
    opts = {"unclipped": C.RMSprop(), "clipnorm": C.RMSprop(clipnorm=1e30)}

    def block(opt, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            eng.train_step(x, t, optimizer=opt)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    for opt in opts.values():  # warm-up of both variants
        block(opt, 2)
    ms = {k: [] for k in opts}
    for _ in range(args.rounds):
        for k, opt in opts.items():
            ms[k].append(block(opt, args.steps))
    res = {"shape": [args.batch, args.height, args.width], "dtype": args.dtype, "steps_per_block": args.steps,
           "blocks": args.rounds}
    for k, v in ms.items():
        res[k] = {"median_ms": round(statistics.median(v), 3), "blocks_ms": [round(u, 3) for u in v]}
    res["unclipped_spread_ms"] = round(max(ms["unclipped"]) - min(ms["unclipped"]), 3)
    res["clipnorm_minus_unclipped_ms"] = round(res["clipnorm"]["median_ms"] - res["unclipped"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=11159011)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gradclip_time: needs a GPU (a timing taken elsewhere says nothing)")
    res = {"kernels": kernels(args.n, args.runs)}
    if not args.no_step:
        res["step"] = step(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
