"""Time cnnitmo_image_metrics (PSNR + SSIM in one pass, csrc/metrics.hip) against a torch-ops
composition of the same metric on the same GPU.

    python tools/metrics_timing.py [--shape 8,1080,1920] [--runs 30] [--warmup 5] [--json FILE]

Both are timed with device events around one call: warm-up runs first, then the median of
--runs runs, the two alternating.  The composition is what a user would write with torch: five
grouped fp32 conv2d calls with the 11x11 window (x, y, x^2, y^2, xy) plus elementwise work and
the means; it makes at least five passes over the data and cancels in fp32, so its values are
compared with the kernel's only loosely (1e-3).  Prints the times, the kernel's achieved GB/s
over the algorithmic read 2*n*h*w*12 B and the share of the 8 TB/s HBM peak, and one JSON line.
Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnn_itmo_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12  # B/s


def torch_composition(a, b, max_val=1.0):
    """(psnr, ssim) per image with torch ops; a, b [n,h,w,3] fp32."""
    import torch.nn.functional as F
    x = torch.arange(11, device=a.device, dtype=torch.float32) - 5
    g = torch.exp(-(x * x) / 4.5)
    g = g / g.sum()
    win = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)
    xa, xb = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mx, my = F.conv2d(xa, win, groups=3), F.conv2d(xb, win, groups=3)
    vx = F.conv2d(xa * xa, win, groups=3) - mx * mx
    vy = F.conv2d(xb * xb, win, groups=3) - my * my
    cxy = F.conv2d(xa * xb, win, groups=3) - mx * my
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    mse = ((a - b) ** 2).mean(dim=(1, 2, 3))
    return 10 * torch.log10(max_val ** 2 / mse), s.mean(dim=(1, 2, 3))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", default="8,1080,1920", help="n,h,w")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args(argv)
    n, h, w = (int(v) for v in a.shape.split(","))
    if a.runs < 20:
        ap.error("--runs: at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("metrics_timing: needs a GPU")
    gen = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(n, h, w, 3, device="cuda", generator=gen)
    p = (t + 0.03 * torch.randn(n, h, w, 3, device="cuda", generator=gen)).clamp_(0, 1)
    out = torch.empty(n, 3, dtype=torch.float64, device="cuda")
    ws = ops.workspace(ops.image_metrics_workspace_bytes(n, h, w))

    def kernel():
        ops.call("cnnitmo_image_metrics", 3, p.data_ptr(), t.data_ptr(), n, h, w, 1.0, out.data_ptr(),
                 ws.data_ptr(), ws.numel(), ops.stream_ptr())

    ref = [None]

    def composition():
        ref[0] = torch_composition(p, t)

    for _ in range(a.warmup):
        kernel()
        composition()
    torch.cuda.synchronize()
    tk, tc = [], []
    for _ in range(a.runs):
        tk.append(timed(kernel))
        tc.append(timed(composition))
    got = out.cpu().numpy()
    rp, rs = (v.double().cpu().numpy() for v in ref[0])
    if not (np.abs(got[:, 1] - rp).max() <= 1e-3 and np.abs(got[:, 2] - rs).max() <= 1e-3):
        raise SystemExit(f"metrics_timing: kernel {got[:, 1:]} and composition {rp} {rs} disagree")
    ms_k, ms_c = float(np.median(tk)), float(np.median(tc))
    nbytes = 2 * n * h * w * 12
    gbs = nbytes / (ms_k * 1e-3) / 1e9
    res = {"shape": [n, h, w, 3], "runs": a.runs, "warmup": a.warmup, "kernel_ms": round(ms_k, 4),
           "kernel_ms_min_max": [round(min(tk), 4), round(max(tk), 4)], "torch_composition_ms": round(ms_c, 4),
           "speedup": round(ms_c / ms_k, 2), "algorithmic_bytes": nbytes, "kernel_GBps": round(gbs, 1),
           "hbm_peak_fraction": round(gbs * 1e9 / HBM_PEAK, 4),
           "max_abs_diff_vs_composition": {"psnr_dB": float(np.abs(got[:, 1] - rp).max()),
                                           "ssim": float(np.abs(got[:, 2] - rs).max())}}
    print(f"cnnitmo_image_metrics(what=3) on [{n},{h},{w},3]: {ms_k:.3f} ms (median of {a.runs}), "
          f"{gbs:.0f} GB/s of the {nbytes / 1e6:.0f} MB algorithmic read = {100 * gbs * 1e9 / HBM_PEAK:.1f}% "
          f"of the HBM peak; torch composition {ms_c:.3f} ms ({ms_c / ms_k:.1f}x)")
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0 if ms_k < ms_c else 1


if __name__ == "__main__":
    sys.exit(main())
