"""Time the JPEG round trip (csrc/jpeg.hip) beside the HDR pair generator's kernel call it follows.

    python tools/jpeg_timing.py [--batch 32] [--size 512] [--sources 16] [--source-shape 1024,2048]
                                [--runs 10] [--warmup 2] [--seed 0] [--step-ms MS] [--out FILE]

The batch is tools/hdrgen_timing.py's: synthetic log-normal RGBE pictures resident on the device,
--batch frames of --size x --size, the reference augmentation, random cameras, x quantised to 8 bits
(what the JPEG step needs).  In one run, the legs alternating, with device events around one batch:

  pairs        one cnnitmo_hdr_pairs call, its arguments already on the device
  pairs+jpeg   the same call followed by cnnitmo_jpeg_roundtrip on x, in place, one quality per frame
               drawn from 30..90, for '4:2:0' and for '4:4:4'

Reported per subsampling: the medians, the round trip's own time (the difference of the medians), its
ratio to the pairs call of the same run, its HBM traffic model (12 B read + 12 B written per pixel,
plus the uint8 planes written and read once: 1.5 B each way for 4:2:0, 3 B for 4:4:4) and, with
--step-ms (the ms_per_step of `bench.py --gpus 1`, a 1080p training step), its share of that step.
Prints a text report, --out also writes it to a file.  Needs a GPU.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnn_itmo_amd import degrade, hdrio, ops  # noqa: E402
from cnn_itmo_amd.datagen import ImageDataGenerator  # noqa: E402

REF_ARGS = dict(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2)
KEY = 0.18
PLANE_BYTES = {"4:2:0": 1.5, "4:4:4": 3.0}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sources", type=int, default=16)
    ap.add_argument("--source-shape", default="1024,2048")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-ms", type=float, default=None, help="ms_per_step of bench.py --gpus 1")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    hs, ws = (int(v) for v in a.source_shape.split(","))
    n, s = a.batch, a.size
    if hs < s or ws < s:
        ap.error("--source-shape: smaller than the window")
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_timing: needs a GPU")

    g = torch.Generator(device="cuda").manual_seed(a.seed)
    sources = []
    for _ in range(a.sources):
        base = torch.exp(np.log(10.0) * (0.85 * torch.randn(hs, ws, 1, device="cuda", generator=g) - 0.5))
        sources.append(hdrio.rgbe_encode(base * (0.5 + 0.5 * torch.rand(hs, ws, 3, device="cuda", generator=g))))
    gen = ImageDataGenerator(**REF_ARGS)
    rs = np.random.RandomState(a.seed)
    params = [gen.get_random_transform((s, s, 3), rs) for _ in range(n)]
    tops = [int(rs.randint(0, hs - s + 1)) for _ in range(n)]
    lefts = [int(rs.randint(0, ws - s + 1)) for _ in range(n)]
    v, cn, cy = 8 * rs.random_sample(n) - 4, np.abs(rs.normal(0.6, np.sqrt(0.1), n)) + 0.05, \
        np.abs(rs.normal(0.9, np.sqrt(0.1), n)) + 0.05
    qtabs = np.stack([degrade.quant_tables(int(q)) for q in rs.randint(30, 91, n)])
    frames = [sources[i % a.sources] for i in range(n)]
    desc = ops.hdr_descriptors(frames, [(t, l, t + s - 1, l + s - 1) for t, l in zip(tops, lefts)])
    mats, flips = [], []
    for p, t, l in zip(params, tops, lefts):
        m6, f = ImageDataGenerator.affine(p, s, s)
        m = np.vstack([m6.reshape(2, 3), [0.0, 0.0, 1.0]])
        mats.append(np.dot(np.array([[1, 0, t], [0, 1, l], [0, 0, 1]], np.float64), m)[:2].reshape(-1))
        flips.append(f)
    dev = (torch.from_numpy(desc.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(np.stack(mats)).cuda(),
           torch.from_numpy(np.asarray(flips, np.int32)).cuda(),
           torch.from_numpy(np.stack([KEY * 2.0 ** v, cn, cy], axis=1)).cuda())
    x, y = (torch.empty(n, s, s, 3, device="cuda") for _ in range(2))
    wsp = ops.workspace(ops.hdr_pairs_workspace_bytes(n))
    wsj = {sub: ops.workspace(ops.jpeg_workspace_bytes(n, s, s, sub)) for sub in PLANE_BYTES}

    def pairs():
        ops.hdr_pairs(*dev, x, y, key=KEY, quantize=1, ws=wsp)

    def with_jpeg(sub):
        pairs()
        ops.jpeg_roundtrip(x, qtabs, sub, out=x, ws=wsj[sub])

    legs = {"pairs": pairs, **{f"pairs+jpeg {sub}": (lambda sub=sub: with_jpeg(sub)) for sub in PLANE_BYTES}}
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, fn in legs.items():  # alternating, one batch each
            times[k].append(timed(fn))

    med = {k: float(np.median(t)) for k, t in times.items()}
    px = n * s * s
    lines = [f"jpeg round trip after cnnitmo_hdr_pairs, [{n},{s},{s},3] from {a.sources} RGBE pictures of {hs} x {ws}, "
             f"qualities 30..90 per frame; medians of {a.runs} runs after {a.warmup} warm-ups, ms per batch"]
    for k, t in times.items():
        lines.append(f"  {k:18s} median {med[k]:8.3f}  min {min(t):8.3f}  max {max(t):8.3f}")
    for sub, pb in PLANE_BYTES.items():
        own = med[f"pairs+jpeg {sub}"] - med["pairs"]
        line = (f"  round trip {sub}: {own:.3f} ms = {own / med['pairs']:.2f} x the pairs call; traffic model "
                f"{24 + 2 * pb:.0f} B/pixel -> {(24 + 2 * pb) * px / own / 1e6:.0f} GB/s")
        if a.step_ms:
            line += f"; {100 * own / a.step_ms:.2f} % of a {a.step_ms:.2f} ms 1080p training step"
        lines.append(line)
    report = "\n".join(lines)
    print(report)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(report + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
