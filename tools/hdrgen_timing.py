"""Time the HDR pair generator's kernel call (csrc/hdrpairs.hip) against the same batch composed
from the ops that existed before it.

    python tools/hdrgen_timing.py [--batch 32] [--size 512] [--sources 16] [--source-shape 1024,2048]
                                  [--runs 30] [--warmup 5] [--seed 0] [--json FILE]

Sources: synthetic log-normal pictures, RGBE bytes resident on the device.  Batch: --batch frames of
--size x --size, frame i from source i % --sources, a random window of the target size, the
reference augmentation (rotation 90, both flips, zoom 0.2), random cameras, nothing quantised.

  fused      one cnnitmo_hdr_pairs call, its arguments already on the device
  fused+host the same call with the descriptors, matrices and cameras built and uploaded first
             (what HDRPairIterator does per batch)
  composed   the batch from the earlier ops: the windows cut out of the RGBE pictures,
             hdrio.rgbe_decode, ImageDataGenerator.transform_batch, tonemap.reinhard and
             tonemap.virtual_camera, through their public Python entry points

Each leg is timed with device events around one batch: warm-up first, then the median and the
spread of --runs runs, the legs alternating.  The two results are compared after the sanitise rule
(NaN -> 0, clamp to [0, 1]), which only the fused call applies itself.  Prints one JSON line.
Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnn_itmo_amd import hdrio, ops, tonemap  # noqa: E402
from cnn_itmo_amd.datagen import ImageDataGenerator  # noqa: E402

REF_ARGS = dict(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2)
KEY = 0.18


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v, batch):
    med = float(np.median(v))
    return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "p10_p90_ms": [round(float(np.percentile(v, 10)), 4), round(float(np.percentile(v, 90)), 4)],
            "pairs_per_s": round(batch / med * 1e3, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sources", type=int, default=16)
    ap.add_argument("--source-shape", default="1024,2048")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args(argv)
    hs, ws = (int(v) for v in a.source_shape.split(","))
    n, s = a.batch, a.size
    if a.runs < 20:
        ap.error("--runs: at least 20")
    if hs < s or ws < s:
        ap.error("--source-shape: smaller than the window")
    if not torch.cuda.is_available():
        raise SystemExit("hdrgen_timing: needs a GPU")

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
    frames = [sources[i % a.sources] for i in range(n)]

    def host_args():
        desc = ops.hdr_descriptors(frames, [(t, l, t + s - 1, l + s - 1) for t, l in zip(tops, lefts)])
        mats, flips = [], []
        for p, t, l in zip(params, tops, lefts):
            m6, f = ImageDataGenerator.affine(p, s, s)
            m = np.vstack([m6.reshape(2, 3), [0.0, 0.0, 1.0]])
            m = np.dot(np.array([[1, 0, t], [0, 1, l], [0, 0, 1]], np.float64), m)
            mats.append(m[:2].reshape(-1))
            flips.append(f)
        cam = np.stack([KEY * 2.0 ** v, cn, cy], axis=1)
        return (torch.from_numpy(desc.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(np.stack(mats)).cuda(),
                torch.from_numpy(np.asarray(flips, np.int32)).cuda(), torch.from_numpy(cam).cuda())

    x, y = (torch.empty(n, s, s, 3, device="cuda") for _ in range(2))
    wsp = ops.workspace(ops.hdr_pairs_workspace_bytes(n))
    dev = host_args()

    def fused(args=None):
        d, m, f, c = args or dev
        ops.hdr_pairs(d, m, f, c, x, y, key=KEY, quantize=0, ws=wsp)

    def composed():
        crops = torch.stack([src[t:t + s, l:l + s] for src, t, l in zip(frames, tops, lefts)])
        warped = gen.transform_batch(hdrio.rgbe_decode(crops), params)
        return tonemap.virtual_camera(warped, v, cn, cy, key=KEY), tonemap.reinhard(warped, key=KEY)

    legs = {"fused": fused, "fused_with_host": lambda: fused(host_args()), "composed": composed}
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, fn in legs.items():  # alternating, one batch each
            times[k].append(timed(fn))

    fused()
    xc, yc = composed()
    torch.cuda.synchronize()
    diff = {k: float((p - torch.nan_to_num(q, nan=0.0).clamp_(0, 1)).abs().max())
            for k, p, q in (("x", x, xc), ("y", y, yc))}
    px = n * s * s
    res = {"batch": [n, s, s, 3], "sources": [a.sources, hs, ws], "format": "rgbe", "runs": a.runs,
           "warmup": a.warmup, **{k: stats(t, n) for k, t in times.items()},
           "fused_over_composed": round(float(np.median(times["composed"]) / np.median(times["fused"])), 3),
           # fused: x, y written + two 4-byte gathers; composed: crop copy 8, decode 16, warp 24, two
           # statistics passes 24, two curve passes 48
           "model_bytes_per_pixel": {"fused": 32, "composed": 120},
           "fused_model_gb_per_s": round(32 * px / np.median(times["fused"]) / 1e6, 1),
           "max_abs_difference": diff}
    print(f"hdr pairs [{n},{s},{s},3] from {a.sources} RGBE pictures of {hs} x {ws}: fused "
          f"{res['fused']['median_ms']:.3f} ms ({res['fused']['pairs_per_s']:.0f} pairs/s), with host arguments "
          f"{res['fused_with_host']['median_ms']:.3f} ms, composed {res['composed']['median_ms']:.3f} ms "
          f"({res['composed']['pairs_per_s']:.0f} pairs/s); medians of {a.runs}; max |difference| {diff}")
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
