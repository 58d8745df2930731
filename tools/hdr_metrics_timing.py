"""Time the HDR quality metrics (csrc/hdrmetrics.hip): cnnitmo_lum_percentile, cnnitmo_hdr_encode
(PQ and log), the whole hdrmetrics.hdr_psnr_ssim, and cnnitmo_image_metrics alone in the same run
as the comparison.

    python tools/hdr_metrics_timing.py [--shape 8,1080,1920] [--runs 30] [--warmup 5] [--json FILE]

tools/metrics_timing.py's protocol: device events around one call, warm-up runs first, then the
median of --runs runs, the timed calls alternating.  The encode is reported in ms and in GB/s over
its 24 B per pixel (12 B read, 12 B written), with the share of the 8 TB/s HBM peak: far below it
means the two fp64 pow per value bound the kernel, not the memory.  Prints the times and one JSON
line.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnn_itmo_amd import hdrmetrics, ops  # noqa: E402

HBM_PEAK = 8.0e12  # B/s


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
        raise SystemExit("hdr_metrics_timing: needs a GPU")
    # a +-7 stop reference and a noisy, 3.7x brighter prediction (tests/hdrmetrics_ref.make_pair's recipe)
    gen = torch.Generator(device="cuda").manual_seed(0)
    yy = torch.arange(h, device="cuda", dtype=torch.float32).view(1, h, 1, 1)
    xx = torch.arange(w, device="cuda", dtype=torch.float32).view(1, 1, w, 1)
    cc = torch.arange(3, device="cuda", dtype=torch.float32).view(1, 1, 1, 3)
    base = torch.sin(0.011 * yy + 0.007 * xx + 0.4 * cc) * torch.cos(0.005 * xx - 0.003 * yy)
    ref = torch.exp2(7.0 * base + 0.3 * torch.randn(n, h, w, 3, device="cuda", generator=gen)).contiguous()
    pred = (ref * torch.exp2(0.1 * torch.randn(n, h, w, 3, device="cuda", generator=gen)) * 3.7).contiguous()
    sp, sr = hdrmetrics.hdr_scales(pred, ref)
    enc_p, enc_r = torch.empty_like(pred), torch.empty_like(ref)
    q_out = torch.empty(n, dtype=torch.float32, device="cuda")
    met = torch.empty(n, 3, dtype=torch.float64, device="cuda")
    ws_q = ops.workspace(ops.lum_percentile_workspace_bytes(n))
    ws_m = ops.workspace(ops.image_metrics_workspace_bytes(n, h, w))
    whole = [None]

    def percentile():
        ops.call("cnnitmo_lum_percentile", ref.data_ptr(), n, h, w, None, 0.999, q_out.data_ptr(), ws_q.data_ptr(),
                 ws_q.numel(), ops.stream_ptr())

    def encode_pq():
        ops.hdr_encode(ops.HDR_ENCODINGS["pq"], pred, sp, enc_p)

    def encode_log():
        ops.hdr_encode(ops.HDR_ENCODINGS["log"], ref, sr, enc_r)

    def encode_ref_pq():
        ops.hdr_encode(ops.HDR_ENCODINGS["pq"], ref, sr, enc_r)

    def image_metrics():
        ops.call("cnnitmo_image_metrics", 3, enc_p.data_ptr(), enc_r.data_ptr(), n, h, w, 1.0, met.data_ptr(),
                 ws_m.data_ptr(), ws_m.numel(), ops.stream_ptr())

    def hdr_psnr_ssim():
        whole[0] = hdrmetrics.hdr_psnr_ssim(pred, ref)

    # (encode_ref_pq last among the encodes: image_metrics then scores the PQ planes of both images)
    calls = [percentile, encode_log, encode_pq, encode_ref_pq, image_metrics, hdr_psnr_ssim]
    for _ in range(a.warmup):
        for fn in calls:
            fn()
    torch.cuda.synchronize()
    times = {fn.__name__: [] for fn in calls}
    for _ in range(a.runs):
        for fn in calls:
            times[fn.__name__].append(timed(fn))
    ms = {k: float(np.median(v)) for k, v in times.items()}
    got = met.cpu().numpy()
    ps, ss = (v.cpu().numpy() for v in whole[0])
    if not (np.array_equal(got[:, 1], ps) and np.array_equal(got[:, 2], ss)):
        raise SystemExit(f"hdr_metrics_timing: the composed calls {got[:, 1:]} and hdr_psnr_ssim {ps} {ss} disagree")
    nbytes = n * h * w * 24
    gbs = {k: nbytes / (ms[k] * 1e-3) / 1e9 for k in ("encode_pq", "encode_log")}
    res = {"shape": [n, h, w, 3], "runs": a.runs, "warmup": a.warmup,
           "lum_percentile_ms": round(ms["percentile"], 4),
           "hdr_encode_pq_ms": round(ms["encode_pq"], 4), "hdr_encode_pq_GBps": round(gbs["encode_pq"], 1),
           "hdr_encode_pq_hbm_peak_fraction": round(gbs["encode_pq"] * 1e9 / HBM_PEAK, 4),
           "hdr_encode_log_ms": round(ms["encode_log"], 4), "hdr_encode_log_GBps": round(gbs["encode_log"], 1),
           "encode_bytes": nbytes, "image_metrics_ms": round(ms["image_metrics"], 4),
           "hdr_psnr_ssim_ms": round(ms["hdr_psnr_ssim"], 4),
           "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
           "psnr_dB": [round(float(v), 4) for v in ps], "ssim": [round(float(v), 6) for v in ss]}
    print(f"[{n},{h},{w},3], medians of {a.runs}: cnnitmo_lum_percentile {ms['percentile']:.3f} ms; "
          f"cnnitmo_hdr_encode PQ {ms['encode_pq']:.3f} ms = {gbs['encode_pq']:.0f} GB/s of {nbytes / 1e6:.0f} MB "
          f"({100 * gbs['encode_pq'] * 1e9 / HBM_PEAK:.1f}% of the HBM peak), log {ms['encode_log']:.3f} ms = "
          f"{gbs['encode_log']:.0f} GB/s; cnnitmo_image_metrics {ms['image_metrics']:.3f} ms; "
          f"hdr_psnr_ssim {ms['hdr_psnr_ssim']:.3f} ms")
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
