"""Time the sensor paths of the HDR pair generator (csrc/hdrpairs.hip) against cnnitmo_hdr_pairs.

    python tools/sensor_timing.py [--batch 32] [--size 512] [--sources 16] [--source-shape 1024,2048]
                                  [--runs 30] [--warmup 5] [--seed 0] [--baseline-lib FILE] [--json FILE]

The batch is tools/hdrgen_timing.py's: --batch frames of --size x --size from RGBE pictures resident
on the device, a random window of the target size, the reference augmentation, random cameras,
nothing quantised, every argument already on the device.  Legs, one call each:

  pairs          cnnitmo_hdr_pairs
  luminance      cnnitmo_hdr_pairs_sensor, response 0 (the same kernel instantiation as `pairs`)
  channel        cnnitmo_hdr_pairs_sensor, response 1, no noise
  channel_noise  cnnitmo_hdr_pairs_sensor, response 1, noise (a, b) = (1e-3, 2e-3) on every frame
  noise_alone    cnnitmo_sensor_noise on the batch x
  baseline       with --baseline-lib: cnnitmo_hdr_pairs of that build of the library (an earlier
                 commit's, say), loaded beside this one and called with the same arguments

Device events around one call: warm-up first, then the median and the spread of --runs runs, the
legs alternating in one process.  Prints one JSON line.  Needs a GPU.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdrgen_timing import KEY, REF_ARGS, stats, timed  # noqa: E402
from cnn_itmo_amd import _lib, hdrio, ops  # noqa: E402
from cnn_itmo_amd.datagen import ImageDataGenerator  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sources", type=int, default=16)
    ap.add_argument("--source-shape", default="1024,2048")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--baseline-lib", default=None, help="another build of libcnnitmo.so to time cnnitmo_hdr_pairs of")
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    a = ap.parse_args(argv)
    hs, ws = (int(v) for v in a.source_shape.split(","))
    n, s = a.batch, a.size
    if a.runs < 20:
        ap.error("--runs: at least 20")
    if hs < s or ws < s:
        ap.error("--source-shape: smaller than the window")
    if not torch.cuda.is_available():
        raise SystemExit("sensor_timing: needs a GPU")

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
    desc = ops.hdr_descriptors(frames, [(t, l, t + s - 1, l + s - 1) for t, l in zip(tops, lefts)])
    mats, flips = [], []
    for p, t, l in zip(params, tops, lefts):
        m6, f = ImageDataGenerator.affine(p, s, s)
        m = np.vstack([m6.reshape(2, 3), [0.0, 0.0, 1.0]])
        mats.append(np.dot(np.array([[1, 0, t], [0, 1, l], [0, 0, 1]], np.float64), m)[:2].reshape(-1))
        flips.append(f)
    d = torch.from_numpy(desc.view(np.uint8).reshape(-1)).cuda()
    m = torch.from_numpy(np.stack(mats)).cuda()
    f = torch.from_numpy(np.asarray(flips, np.int32)).cuda()
    c = torch.from_numpy(np.stack([KEY * 2.0 ** v, cn, cy], axis=1)).cuda()
    noise = torch.tensor([[1e-3, 2e-3]] * n, dtype=torch.float64, device="cuda")
    keys = torch.from_numpy(np.stack([rs.randint(0, 2 ** 62, n), np.zeros(n, np.int64)], axis=1)).cuda()

    x, y, xl, xn = (torch.empty(n, s, s, 3, device="cuda") for _ in range(4))
    wsp = ops.workspace(ops.hdr_pairs_workspace_bytes(n))

    def sensor(out, response, ab=None):
        ops.hdr_pairs_sensor(d, m, f, c, out, y, key=KEY, response=response, noise=ab, keys=keys, ws=wsp)

    legs = {"pairs": lambda: ops.hdr_pairs(d, m, f, c, x, y, key=KEY, quantize=0, ws=wsp),
            "luminance": lambda: sensor(xl, 0),
            "channel": lambda: sensor(xn, 1),
            "channel_noise": lambda: sensor(xn, 1, noise),
            "noise_alone": lambda: ops.sensor_noise(x, noise, keys, out=xn)}
    if a.baseline_lib:
        base = ctypes.CDLL(os.path.abspath(a.baseline_lib))
        base.cnnitmo_hdr_pairs.restype, base.cnnitmo_hdr_pairs.argtypes = _lib.SIGNATURES["cnnitmo_hdr_pairs"]
        xb, yb = torch.empty_like(x), torch.empty_like(x)

        def baseline():
            rc = base.cnnitmo_hdr_pairs(d.data_ptr(), n, s, s, m.data_ptr(), f.data_ptr(), None, KEY, c.data_ptr(), 0,
                                        xb.data_ptr(), yb.data_ptr(), None, None, wsp.data_ptr(), wsp.numel(),
                                        ops.stream_ptr())
            assert rc == 0, rc
        legs["baseline"] = baseline
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, fn in legs.items():  # alternating, one call each
            times[k].append(timed(fn))

    legs["pairs"]()
    legs["luminance"]()
    res = {"batch": [n, s, s, 3], "sources": [a.sources, hs, ws], "format": "rgbe", "runs": a.runs,
           "warmup": a.warmup, **{k: stats(t, n) for k, t in times.items()},
           "luminance_equals_pairs": bool(torch.equal(x, xl))}
    if a.baseline_lib:
        legs["baseline"]()
        torch.cuda.synchronize()
        res["baseline_equals_pairs"] = bool(torch.equal(x, xb) and torch.equal(y, yb))
    print("hdr pairs [%d,%d,%d,3], medians of %d in ms: %s" % (
        n, s, s, a.runs, ", ".join(f"{k} {res[k]['median_ms']:.4f}" for k in legs)))
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
