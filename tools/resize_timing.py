"""Time the antialiased resampler (csrc/resize.hip) at the sizes HDR sources and video frames come in.

    python tools/resize_timing.py [--runs 10] [--warmup 2] [--seed 0] [--pil-runs 3] [--out FILE]

Two workloads, each for 'bilinear' and 'lanczos', tables and workspace already on the device, device
events around one cnnitmo_resize call, the legs alternating in one process:

  fp32   [1,4096,8192,3] -> fit_within(.., 1024) = 512 x 1024      an HDR panorama made a training source
  uint8  [8,2160,3840,3] -> 540 x 960                             a batch of 4K frames for predict --max-side

and, per workload and filter, the horizontal pass alone (the same call with the height kept).  Reported:
median and min..max of --runs after --warmup, the bytes of the traffic model (the input read once, the
intermediate [n,h,ow,3] written and read once, the output written once) and the rate they imply, to hold
against the achievable HBM rate; and, for scale, PIL's Image.resize on the host
over the same uint8 frames.  Prints a text report, --out also writes it to a file.  Needs a GPU.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnn_itmo_amd import ops  # noqa: E402
from cnn_itmo_amd import resize as Z  # noqa: E402

FILTERS = ("bilinear", "lanczos")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def tables(n_in, n_out, filt):
    if n_in == n_out:
        return None
    b, k = Z.coefficients(n_in, n_out, filt)
    return torch.from_numpy(b).cuda(), torch.from_numpy(k).cuda()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pil-runs", type=int, default=3, help="0: skip the host comparison")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("resize_timing: needs a GPU")

    g = torch.Generator(device="cuda").manual_seed(a.seed)
    hdr = torch.rand(1, 4096, 8192, 3, device="cuda", generator=g) ** 8 * 1000
    frames = torch.randint(0, 256, (8, 2160, 3840, 3), device="cuda", generator=g, dtype=torch.uint8)
    work = {"fp32": (hdr, Z.fit_within(4096, 8192, 1024)), "uint8": (frames, (540, 960))}

    legs, model = {}, {}
    for name, (x, (oh, ow)) in work.items():
        n, h, w, _ = x.shape
        es = x.element_size()
        for filt in FILTERS:
            tx, ty = tables(w, ow, filt), tables(h, oh, filt)
            out = torch.empty(n, oh, ow, 3, dtype=x.dtype, device="cuda")
            mid = torch.empty(n, h, ow, 3, dtype=x.dtype, device="cuda")
            ws = ops.workspace(ops.resize_workspace_bytes(x.dtype, n, h, w, oh, ow))
            legs[f"{name} {filt}"] = lambda x=x, out=out, tx=tx, ty=ty, ws=ws: ops.resize(x, out, tx, ty, ws=ws)
            legs[f"{name} {filt} horizontal only"] = lambda x=x, mid=mid, tx=tx: ops.resize(x, mid, tx, None)
            model[f"{name} {filt}"] = 3 * es * n * (h * w + 2 * h * ow + oh * ow)
            model[f"{name} {filt} horizontal only"] = 3 * es * n * (h * w + h * ow)
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, fn in legs.items():  # alternating, one call each
            times[k].append(timed(fn))

    lines = [f"cnnitmo_resize: fp32 [1,4096,8192,3] -> 512 x 1024 and uint8 [8,2160,3840,3] -> 540 x 960; medians of "
             f"{a.runs} runs after {a.warmup} warm-ups, ms per call; traffic model: input read once, intermediate "
             f"written and read once, output written once"]
    for k, t in times.items():
        med = float(np.median(t))
        lines.append(f"  {k:36s} median {med:8.3f}  min {min(t):8.3f}  max {max(t):8.3f}   model "
                     f"{model[k] / 1e6:8.1f} MB -> {model[k] / med / 1e9:6.3f} TB/s")
    if a.pil_runs > 0:
        from PIL import Image
        host = frames.cpu().numpy()
        for filt, f in (("bilinear", Image.BILINEAR), ("lanczos", Image.LANCZOS)):
            ts = []
            for _ in range(a.pil_runs):
                t0 = time.perf_counter()
                for u in host:
                    Image.fromarray(u).resize((960, 540), f)
                ts.append(1e3 * (time.perf_counter() - t0))
            lines.append(f"  PIL on the host, uint8 {filt:9s}          median {float(np.median(ts)):8.1f}  min "
                         f"{min(ts):8.1f}  max {max(ts):8.1f}   (8 frames, one thread)")
    report = "\n".join(lines)
    print(report)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(report + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
