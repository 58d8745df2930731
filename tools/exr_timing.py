"""Time the OpenEXR pixel kernels (csrc/exr.hip) beside the host work of reading a file.

    python tools/exr_timing.py [--runs 10] [--warmup 2] [--seed 0] [--small] [--out FILE]

Two pictures: [4096,8192] half ZIP and [2160,3840] float ZIPS (--small: 1/8 of each side, to try
the tool), synthetic log-normal radiance with smooth structure and 1 % noise, written once with
exr.write_exr.  In one process, the legs alternating, each timed --runs times after --warmup:

  unpack        cnnitmo_exr_unpack: its three launches, arguments on the device (device events)
  pack          cnnitmo_exr_pack, coded (device events)
  inflate 1/8   exr.parse_exr of the file's bytes with workers = 1 and 8 (host clock)
  numpy         tests/exr_ref.py's decode_chunk per chunk and the float conversion of the three
                channels: what the kernels take off the host (host clock)

Reported: median, min - max, and for the kernels the HBM traffic model over the median --
unpack: raw read + scanned bytes written + scanned bytes read + 12 B/pixel written; pack: 12 B/pixel
read + the record bytes written -- beside the 6.3 TB/s of DESIGN section 3.
Prints a text report, --out also writes it to a file.  Needs a GPU.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cnn_itmo_amd import exr, ops  # noqa: E402
import exr_ref as ER  # noqa: E402

PEAK_TBS = 6.3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def clocked(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def radiance(h, w, g):
    coarse = torch.randn(1, 1, h // 8 + 1, w // 8 + 1, device="cuda", generator=g)
    base = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False)[0, 0]
    img = torch.exp(np.log(10.0) * (0.85 * base - 0.5))[..., None] * \
        (0.5 + 0.5 * torch.rand(h, w, 3, device="cuda", generator=g))
    return (img * (1 + 0.01 * torch.randn(h, w, 3, device="cuda", generator=g))).contiguous()


def numpy_leg(parsed):
    lay = parsed.layout
    h, w, lb, lines = lay["h"], lay["w"], lay["line_bytes"], lay["lines_per_chunk"]
    rec = np.empty_like(parsed.raw)
    for i in range(lay["nchunks"]):
        lo, hi = i * lines * lb, min(h, (i + 1) * lines) * lb
        rec[lo:hi] = ER.decode_chunk(parsed.raw[lo:hi]) if lay["coded"][i] else parsed.raw[lo:hi]
    rows = rec.reshape(h, lb)
    out = np.empty((h, w, 3), np.float32)
    for k, (off, typ) in enumerate(zip(lay["ch_off"], lay["ch_type"])):
        dt = ER.DTYPES[typ]
        out[..., k] = np.ascontiguousarray(rows[:, off:off + w * dt.itemsize]).view(dt).reshape(h, w)
    return out


def one_picture(h, w, pixel_type, compression, a, g, path):
    img = radiance(h, w, g)
    exr.write_exr(path, img, pixel_type=pixel_type, compression=compression)
    data = open(path, "rb").read()
    parsed = exr.parse_exr(data)
    lay = parsed.layout
    ptype, lines = lay["ch_type"][0], lay["lines_per_chunk"]
    raw = torch.from_numpy(parsed.raw).cuda()
    coded = torch.from_numpy(lay["coded"]).cuda()
    ws = ops.workspace(ops.exr_workspace_bytes(h, lines, lay["line_bytes"]))
    rgb = torch.empty(h, w, 3, device="cuda")
    out = torch.empty_like(raw)
    legs = {
        "unpack": (timed, lambda: ops.exr_unpack(raw, coded, lines, lay["line_bytes"], lay["ch_off"], lay["ch_type"],
                                                 rgb, ws=ws)),
        "pack": (timed, lambda: ops.exr_pack(img, ptype, lines, 1, out)),
        "inflate 1": (clocked, lambda: exr.parse_exr(data, workers=1)),
        "inflate 8": (clocked, lambda: exr.parse_exr(data, workers=8)),
        "numpy": (clocked, lambda: numpy_leg(parsed)),
    }
    for _ in range(a.warmup):
        for clock, fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, (clock, fn) in legs.items():  # alternating
            times[k].append(clock(fn))
    # what was timed is what the reference computes
    want = numpy_leg(parsed)
    assert np.array_equal(rgb.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out.cpu().numpy(), parsed.raw) or not lay["coded"].all()
    px, nraw = h * w, parsed.raw.size
    model = {"unpack": 3 * nraw + 12 * px, "pack": 12 * px + nraw}
    lines_out = [f"[{h},{w}] {pixel_type} {compression.upper()}: file {len(data) / 1e6:.1f} MB, "
                 f"raw {nraw / 1e6:.1f} MB ({nraw / px:.0f} B/pixel), {int(lay['coded'].sum())} of {lay['nchunks']} "
                 f"chunks coded; ms, median of {a.runs} after {a.warmup} warm-ups (min - max)"]
    for k, t in times.items():
        med = float(np.median(t))
        line = f"  {k:10s} {med:10.3f}  ({min(t):.3f} - {max(t):.3f})"
        if k in model:
            tbs = model[k] / med / 1e9
            line += (f"   traffic model {model[k] / px:.0f} B/pixel = {model[k] / 1e6:.0f} MB -> {tbs:.2f} TB/s, "
                     f"{100 * tbs / PEAK_TBS:.0f} % of {PEAK_TBS} TB/s")
        lines_out.append(line)
    return lines_out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--small", action="store_true", help="1/8 of each side")
    ap.add_argument("--tmp", default=None, help="directory for the two files (default: a temporary one)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("exr_timing: needs a GPU")
    import tempfile
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    d = 8 if a.small else 1
    lines = []
    with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
        for h, w, ptype, comp in ((4096, 8192, "half", "zip"), (2160, 3840, "float", "zips")):
            lines += one_picture(h // d, w // d, ptype, comp, a, g, os.path.join(tmp, "picture.exr"))
    report = "\n".join(lines)
    print(report)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(report + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
