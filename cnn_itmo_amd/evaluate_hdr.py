"""Score a directory of HDR reconstructions against their HDR references (hdrmetrics.py).

    python -m cnn_itmo_amd.evaluate_hdr --pred DIR --reference DIR [--encoding pq|log] \\
        [--align logmean|median|none] [--anchor key|percentile|FLOAT] [--key 0.18] \\
        [--white-nits 203] [--percentile 0.999] [--peak-nits 1000] [--ms-ssim] [--csv FILE]

Every ``.hdr`` / ``.pic`` / ``.pfm`` / ``.exr`` file of ``--pred`` (sorted) is paired with the file
of the same stem in ``--reference`` (any of the four extensions), both are read with
``hdrio.load_image``, aligned, anchored to cd/m^2 and encoded, and PSNR / SSIM of the encoded
pair are printed per file and as the mean.  A missing reference is reported and skipped, a size
mismatch is an error (as ``predict --reference``).  ``--csv``: also write
``name;psnr;ssim;scale_pred;scale_ref`` rows.  ``--ms-ssim``: also the multi-scale SSIM of the
encoded pair (hdrmetrics.hdr_ms_ssim; files of at least 161 x 161 pixels), printed and as a last
``ms_ssim`` column.  ``predict --hdr DIR --hdr-reference DIR`` scores
the reconstructions it wrote with the same functions.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

EXTENSIONS = (".hdr", ".pic", ".pfm", ".exr")
CSV_HEADER = "name;psnr;ssim;scale_pred;scale_ref"


def hdr_files(directory):
    """The HDR image files of a directory, sorted by name."""
    return sorted(os.path.join(directory, f) for f in os.listdir(directory)
                  if os.path.splitext(f)[1].lower() in EXTENSIONS)


def find_reference(ref_dir, stem):
    """The file ``stem`` + one of EXTENSIONS in ref_dir (either letter case), or None."""
    for ext in EXTENSIONS:
        for e in (ext, ext.upper()):
            p = os.path.join(ref_dir, stem + e)
            if os.path.exists(p):
                return p
    return None


def score_files(pred_path, ref_path, encoding="pq", ms_ssim=False, **opts):
    """(psnr dB, ssim, scale_pred, scale_ref) of the HDR file pred_path against ref_path, both read
    from disk, and with ``ms_ssim`` a fifth value, hdrmetrics.hdr_ms_ssim; ``opts``:
    hdrmetrics.hdr_scales' keywords."""
    from . import hdrio, hdrmetrics, ops
    p, r = hdrio.load_image(pred_path), hdrio.load_image(ref_path)
    if p.shape != r.shape:
        raise ValueError(f"{ref_path}: reference is {r.shape[1]}x{r.shape[0]}, the prediction "
                         f"{os.path.basename(pred_path)} {p.shape[1]}x{p.shape[0]}")
    out, sp, sr = hdrmetrics._score(ops.MSE_PSNR | ops.SSIM, p, r, encoding, **opts)
    score = float(out[0, 1].item()), float(out[0, 2].item()), float(sp.item()), float(sr.item())
    if ms_ssim:
        score += (float(hdrmetrics.hdr_ms_ssim(p, r, encoding, **opts).item()),)
    return score


def log_score(log, name, score):
    ps, ss, sp, sr = score[:4]
    ms = f", ms_ssim {score[4]:.6f}" if len(score) > 4 else ""
    log(f"{name}: hdr psnr {ps:.4f} dB, ssim {ss:.6f}{ms} (scale_pred {sp:.6g}, scale_ref {sr:.6g})")


def log_mean(log, scores):
    if scores:
        log(f"mean of {len(scores)} scored HDR files: psnr {np.mean([s[1] for s in scores]):.4f} dB, "
            f"ssim {np.mean([s[2] for s in scores]):.6f}"
            + (f", ms_ssim {np.mean([s[5] for s in scores]):.6f}" if len(scores[0]) > 5 else ""))


def write_csv(path, scores, ms_ssim=False):
    """scores: (name, psnr, ssim, scale_pred, scale_ref) tuples, or with ``ms_ssim`` a sixth value
    and column."""
    with open(path, "w", newline="") as fh:
        fh.write(CSV_HEADER + (";ms_ssim" if ms_ssim else "") + "\n")
        for name, ps, ss, sp, sr, *ms in scores:
            fh.write(f"{name};{ps:.10g};{ss:.10g};{sp:.17g};{sr:.17g}" + "".join(f";{v:.10g}" for v in ms) + "\n")


def evaluate_dir(pred_dir, ref_dir, csv=None, log=print, encoding="pq", ms_ssim=False, **opts):
    """Score every HDR file of pred_dir; returns the (name, psnr, ssim, scale_pred, scale_ref) rows,
    with ``ms_ssim`` each followed by that value."""
    files = hdr_files(pred_dir)
    if not files:
        raise FileNotFoundError(f"no {'/'.join(EXTENSIONS)} files in {pred_dir}")
    scores = []
    for f in files:
        name = os.path.basename(f)
        ref = find_reference(ref_dir, os.path.splitext(name)[0])
        if ref is None:
            log(f"{name}: no reference in {ref_dir}, not scored")
            continue
        if ms_ssim:
            opts = dict(opts, ms_ssim=True)
        score = score_files(f, ref, encoding=encoding, **opts)
        log_score(log, name, score)
        scores.append((name,) + tuple(score))
    log_mean(log, scores)
    if csv:
        write_csv(csv, scores, ms_ssim)
    return scores


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pred", required=True, help="directory of HDR reconstructions (.hdr / .pic / .pfm / .exr)")
    ap.add_argument("--reference", required=True, help="directory of ground-truth HDR files, paired by stem")
    ap.add_argument("--encoding", default="pq", choices=["pq", "log"])
    ap.add_argument("--align", default="logmean", choices=["logmean", "median", "none"],
                    help="the scale that aligns a reconstruction to its reference")
    ap.add_argument("--anchor", default="key",
                    help="key, percentile, or a number: cd/m^2 per unit of the reference (calibrated files)")
    ap.add_argument("--key", type=float, default=0.18, help="anchor key: the key placed on --white-nits")
    ap.add_argument("--white-nits", type=float, default=203.0)
    ap.add_argument("--percentile", type=float, default=0.999,
                    help="anchor percentile: the luminance percentile placed on --peak-nits")
    ap.add_argument("--peak-nits", type=float, default=1000.0)
    ap.add_argument("--ms-ssim", action="store_true",
                    help="also score the multi-scale SSIM of the encoded pair (a last ms_ssim column in --csv)")
    ap.add_argument("--csv", default=None, help=f"write {CSV_HEADER} rows to this file")
    a = ap.parse_args(argv)
    from . import hdrmetrics
    try:
        anchor = hdrmetrics._anchor(a.anchor)
    except ValueError as e:
        ap.error(str(e))
    if not 0.0 < a.percentile <= 1.0:
        ap.error(f"--percentile {a.percentile} outside (0, 1]")
    scores = evaluate_dir(a.pred, a.reference, csv=a.csv, encoding=a.encoding, align=a.align, anchor=anchor,
                          key=a.key, white_nits=a.white_nits, q=a.percentile, peak_nits=a.peak_nits,
                          ms_ssim=a.ms_ssim)
    print(f"scored {len(scores)} of {len(hdr_files(a.pred))} files of {a.pred}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
