"""Inference CLI with the reference's I/O conventions.

/root/reference/predict.py:24-70 loads a Keras checkpoint, then for every
``images_to_predict/input/*.png``: ``np.asarray(Image.open(f)).astype(float) / 255``
(float64, :59), ``model.predict`` on a batch of one (:62),
``(pred * 255)[0].astype('uint8')`` -- truncation, not rounding (:64) -- and
``Image.fromarray(...).save('images_to_predict/output/' + name)`` (:68-69).

Here the same conventions run batched on the GPU:

    python -m cnn_itmo_amd.predict --model saved7-model-218-0.73.hdf5 \\
        [--input images_to_predict/input] [--output images_to_predict/output] \\
        [--batch 8] [--dtype float32|bfloat16] [--tile TH,TW] \\
        [--reference ground_truth_dir [--metrics-csv scores.csv]] \\
        [--hdr DIR [--hdr-format hdr|pfm] [--hdr-mode script|exact] [--hdr-key A] \\
         [--hdr-log-average G|reference] [--hdr-reference hdr_ground_truth_dir [--hdr-metrics-csv scores.csv]]]

Differences, all deliberate: images are processed in sorted order, in batches
of equal-sized frames; the output file name is the input's base name (the
reference splits on a Windows '\\\\' separator, which on Linux yields the whole
input path); frames whose size differs from the checkpoint's input run
through a copy of the (fully convolutional) network built for their size,
padded to a multiple of 16 rows/columns and cropped back.
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np


def read_png(path):
    """uint8 [H, W, 3] (grey / RGBA inputs are converted to RGB)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def to_input(u8):
    """predict.py:59 -- float64 division by 255, then the model's float32."""
    return np.true_divide(np.asarray(u8).astype(float), 255).astype(np.float32)


def to_png(pred):
    """predict.py:64 -- (pred * 255).astype('uint8'): truncation toward zero."""
    return (np.asarray(pred, dtype=np.float32) * 255).astype("uint8")


def model_for_size(model, h, w, cache=None):
    """The same network and weights for frames of size (h, w): `model` itself when
    it fits (up to 15 rows short are padded by the engine), else a rebuilt copy
    whose input is (h, w) rounded up to multiples of 16."""
    H, W, _ = model.inputs[0].shape
    if W == w and 0 <= H - h < 16:
        return model
    key = (-(-h // 16) * 16, -(-w // 16) * 16)
    if cache is not None and key in cache:
        return cache[key]
    from . import keras_h5
    cfg = keras_h5.model_config(model)
    for node in cfg["config"]["layers"]:
        if node["class_name"] == "InputLayer":
            node["config"]["batch_input_shape"] = [None, key[0], key[1], 3]
    m = keras_h5.build_from_config(cfg)
    m.set_named_weights(model.named_weights())
    m.compile(optimizer="rmsprop", loss="mse", metrics=["accuracy"], dtype=model.dtype)
    if cache is not None:
        cache[key] = m
    return m


def _pad_cols(x, W):
    if x.shape[2] == W:
        return x
    out = np.zeros(x.shape[:2] + (W, x.shape[3]), dtype=x.dtype)
    out[:, :, :x.shape[2]] = x
    return out


def predict_frames(model, frames_u8, batch=8, cache=None, tile=None, return_float=False):
    """uint8 frames (equal sizes) -> uint8 predictions, reference conventions.
    ``tile`` (th, tw): spatially tiled inference with 96-px halos (tiled.py; same
    result, activation memory bounded by the window instead of the frame).
    ``return_float``: return (uint8 predictions, float32 predictions) -- the model's output
    before the 8-bit truncation, for the HDR reconstruction of ``--hdr-mode exact``."""
    h, w = frames_u8[0].shape[:2]
    floats = []
    if tile is not None:
        from .tiled import predict_tiled
        outs = []
        for i in range(0, len(frames_u8), batch):
            x = np.stack([to_input(f) for f in frames_u8[i:i + batch]])
            y = predict_tiled(model, x, tile, batch_size=batch, cache=cache)
            outs.extend(to_png(y[j]) for j in range(y.shape[0]))
            if return_float:
                floats.extend(y[j] for j in range(y.shape[0]))
        return (outs, floats) if return_float else outs
    m = model_for_size(model, h, w, cache)
    W = m.inputs[0].shape[1]
    outs = []
    for i in range(0, len(frames_u8), batch):
        x = np.stack([to_input(f) for f in frames_u8[i:i + batch]])
        y = m.predict(_pad_cols(x, W), batch_size=batch)
        outs.extend(to_png(y[j, :h, :w]) for j in range(y.shape[0]))
        if return_float:
            floats.extend(y[j, :h, :w] for j in range(y.shape[0]))
    return (outs, floats) if return_float else outs


def score_png(pred_u8, ref_path, ms_ssim=False):
    """(psnr dB, ssim) of a written uint8 prediction against the PNG at ref_path, on the 0..255
    values (max_val 255): what measuring the two files gives.  ``ms_ssim``: a third value,
    metrics.ms_ssim of the same pair."""
    from . import metrics
    ref = np.array(read_png(ref_path))  # (a writable copy: PIL's buffer is read-only)
    if ref.shape != pred_u8.shape:
        raise ValueError(f"{ref_path}: reference is {ref.shape[1]}x{ref.shape[0]}, the prediction "
                         f"{pred_u8.shape[1]}x{pred_u8.shape[0]}")
    ps, ss = metrics.psnr_ssim(pred_u8, ref, max_val=255.0)
    if ms_ssim:
        return float(ps.item()), float(ss.item()), float(metrics.ms_ssim(pred_u8, ref, max_val=255.0).item())
    return float(ps.item()), float(ss.item())


def write_hdr_prediction(path, pred_u8, pred_f32=None, mode="script", key=0.18, log_average=1.0):
    """The HDR reconstruction of one prediction as ``path`` (.hdr, .pfm or .exr: half, ZIP).  ``script``:
    inverse_Reinhard.m on the written 8-bit prediction; ``exact``: the algebraic inverse of
    Reinhard.m on the float prediction for the HDR log-average ``log_average``.  The inverse map
    and the RGBE encode run on the GPU; a .hdr leaves the device as 4 bytes per pixel."""
    from . import hdrio, tonemap
    if mode == "script":
        hdr = tonemap.inverse_reinhard(np.ascontiguousarray(pred_u8), a=key, mode="script")
    elif mode == "exact":
        hdr = tonemap.inverse_reinhard(np.ascontiguousarray(pred_f32), a=key, g=log_average, mode="exact")
    else:
        raise ValueError(f"hdr mode {mode!r} (script or exact)")
    hdrio.save_image(path, hdr[0])


def reference_log_average(ref_path):
    """The log-average luminance of the HDR file ref_path (``--hdr-log-average reference``)."""
    from . import hdrio, tonemap
    return float(tonemap.log_average(hdrio.load_image(ref_path)).item())


def predict_dir(model, in_dir, out_dir, batch=8, pattern="*.png", log=print, tile=None, reference=None,
                metrics_csv=None, hdr_dir=None, hdr_format="hdr", hdr_mode="script", hdr_key=0.18,
                hdr_log_average=1.0, hdr_reference=None, hdr_metrics_csv=None, ms_ssim=False, max_side=None,
                resample="bilinear"):
    """``max_side``: a frame whose longer side exceeds it is resized after loading, on the GPU, to
    ``resize.fit_within(h, w, max_side)`` with the filter ``resample`` through the uint8 path, so the
    network sees what ``PIL.Image.resize`` would have produced; the PNGs and HDR files written have
    the resized size.
    ``reference``: a directory of ground-truth PNGs; every written prediction is scored
    against the file of the same name there (PSNR / SSIM, logged per file and as the mean; a
    missing reference is reported and skipped, a size mismatch raises).  ``metrics_csv``:
    also write ``name;psnr;ssim`` rows to that file.  ``ms_ssim``: also score the multi-scale
    SSIM (images of at least 161 x 161 pixels), logged and as a further ``ms_ssim`` column.
    ``hdr_dir``: also write every prediction's HDR reconstruction there as ``name.hdr`` (Radiance
    RGBE), ``name.pfm`` or ``name.exr`` (OpenEXR: half, ZIP), by ``hdr_format``;
    ``hdr_mode`` 'script' applies inverse_Reinhard.m to the written 8-bit prediction, 'exact' the
    exact inverse of Reinhard.m (key ``hdr_key``, log-average ``hdr_log_average``) to the float
    prediction.  The PNGs are the same either way.
    ``hdr_reference``: a directory of ground-truth HDR files (.hdr / .pic / .pfm / .exr); every
    reconstruction written to ``hdr_dir`` is read back from disk and scored against the file of the
    same stem there (hdrmetrics.hdr_psnr_ssim with its defaults; logged per file and as the mean, a
    missing reference reported and skipped, a size mismatch raises).  ``hdr_metrics_csv``: also
    write ``name;psnr;ssim;scale_pred;scale_ref`` rows.  ``hdr_log_average='reference'`` ('exact'
    mode, with ``hdr_reference``): each file's log-average is that of its reference."""
    from PIL import Image
    from . import evaluate_hdr as EH
    if hdr_format not in ("hdr", "pfm", "exr"):
        raise ValueError(f"hdr format {hdr_format!r} (hdr, pfm or exr)")
    if hdr_mode not in ("script", "exact"):
        raise ValueError(f"hdr mode {hdr_mode!r} (script or exact)")
    if hdr_reference is not None and hdr_dir is None:
        raise ValueError("hdr_reference needs hdr_dir: the reconstructions written there are what is scored")
    if hdr_metrics_csv and hdr_reference is None:
        raise ValueError("hdr_metrics_csv needs hdr_reference")
    from_reference = hdr_log_average == "reference"
    if from_reference and (hdr_reference is None or hdr_mode != "exact"):
        raise ValueError("hdr_log_average='reference' needs hdr_mode='exact' and hdr_reference")
    files = sorted(glob.glob(os.path.join(in_dir, pattern)))
    if not files:
        raise FileNotFoundError(f"no {pattern} files in {in_dir}")
    os.makedirs(out_dir, exist_ok=True)
    if hdr_dir is not None:
        os.makedirs(hdr_dir, exist_ok=True)
    want_float = hdr_dir is not None and hdr_mode == "exact"
    groups = {}
    frames = {f: read_png(f) for f in files}
    if max_side is not None:
        from . import resize
        for f, u8 in frames.items():
            size = resize.fit_within(u8.shape[0], u8.shape[1], max_side)
            if size != tuple(u8.shape[:2]):
                frames[f] = resize.resize(np.ascontiguousarray(u8), size, resample).cpu().numpy()
    for f in files:
        groups.setdefault(frames[f].shape, []).append(f)
    cache = {}
    written = []
    scores = []
    hdr_scores = []
    for shape, fs in groups.items():
        log(f"Grabbing {len(fs)} input files of {shape[1]}x{shape[0]}")
        preds = predict_frames(model, [frames[f] for f in fs], batch, cache, tile, return_float=want_float)
        preds, floats = preds if want_float else (preds, [None] * len(fs))
        for f, p, pf in zip(fs, preds, floats):
            dst = os.path.join(out_dir, os.path.basename(f))
            Image.fromarray(p).save(dst)
            written.append(dst)
            if hdr_dir is not None:
                stem = os.path.splitext(os.path.basename(f))[0]
                hdr_dst = os.path.join(hdr_dir, f"{stem}.{hdr_format}")
                hdr_ref = None if hdr_reference is None else EH.find_reference(hdr_reference, stem)
                if from_reference and hdr_ref is None:
                    raise FileNotFoundError(f"{os.path.basename(f)}: no reference {stem}.hdr/.pic/.pfm/.exr in "
                                            f"{hdr_reference} to take the log-average from")
                g = reference_log_average(hdr_ref) if from_reference else hdr_log_average
                write_hdr_prediction(hdr_dst, p, pf, hdr_mode, hdr_key, g)
                if hdr_reference is not None:
                    if hdr_ref is None:
                        log(f"{os.path.basename(hdr_dst)}: no reference in {hdr_reference}, not scored")
                    else:
                        score = EH.score_files(hdr_dst, hdr_ref)
                        EH.log_score(log, os.path.basename(hdr_dst), score)
                        hdr_scores.append((os.path.basename(hdr_dst),) + tuple(score))
            if reference is not None:
                ref = os.path.join(reference, os.path.basename(f))
                if not os.path.exists(ref):
                    log(f"{os.path.basename(f)}: no reference {ref}, not scored")
                    continue
                ps, ss, *ms = score_png(p, ref, ms_ssim)
                log(f"{os.path.basename(f)}: psnr {ps:.4f} dB, ssim {ss:.6f}"
                    + "".join(f", ms_ssim {v:.6f}" for v in ms))
                scores.append((os.path.basename(f), ps, ss, *ms))
    if reference is not None:
        if scores:
            log(f"mean of {len(scores)} scored files: psnr {np.mean([s[1] for s in scores]):.4f} dB, "
                f"ssim {np.mean([s[2] for s in scores]):.6f}"
                + (f", ms_ssim {np.mean([s[3] for s in scores]):.6f}" if ms_ssim else ""))
        if metrics_csv:
            with open(metrics_csv, "w", newline="") as fh:
                fh.write("name;psnr;ssim" + (";ms_ssim" if ms_ssim else "") + "\n")
                for name, *vals in scores:
                    fh.write(name + "".join(f";{v:.10g}" for v in vals) + "\n")
    if hdr_reference is not None:
        EH.log_mean(log, hdr_scores)
        if hdr_metrics_csv:
            EH.write_csv(hdr_metrics_csv, hdr_scores)
    return written


def _log_average_arg(s):
    """--hdr-log-average: a float, or the word 'reference'."""
    return "reference" if s == "reference" else float(s)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True, help="Keras HDF5 checkpoint (or an .npz from Model.save)")
    ap.add_argument("--input", default="images_to_predict/input")
    ap.add_argument("--output", default="images_to_predict/output")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dtype", default="float32", choices=["float32", "bfloat16"])
    ap.add_argument("--tile", default=None, help="TH,TW: spatially tiled inference (multiples of 16; 96-px halos)")
    ap.add_argument("--reference", default=None,
                    help="directory of ground-truth PNGs: score each written PNG against the same-named file "
                         "(PSNR and SSIM of the 8-bit images)")
    ap.add_argument("--metrics-csv", default=None, help="with --reference: write name;psnr;ssim rows to this file")
    ap.add_argument("--ms-ssim", action="store_true",
                    help="with --reference: also score the multi-scale SSIM (a further ms_ssim column in "
                         "--metrics-csv)")
    ap.add_argument("--hdr", default=None, metavar="DIR",
                    help="also write each prediction's HDR reconstruction (inverse Reinhard) to DIR/name.hdr")
    ap.add_argument("--hdr-format", default="hdr", choices=["hdr", "pfm", "exr"],
                    help="Radiance RGBE (.hdr), lossless PFM (.pfm) or OpenEXR (.exr: half, ZIP)")
    ap.add_argument("--hdr-mode", default="script", choices=["script", "exact"],
                    help="script: inverse_Reinhard.m on the written 8-bit PNG; exact: the exact inverse of "
                         "Reinhard.m on the float prediction (no banding)")
    ap.add_argument("--hdr-key", type=float, default=0.18, help="the Reinhard key a")
    ap.add_argument("--hdr-log-average", type=_log_average_arg, default=1.0, metavar="G|reference",
                    help="exact mode: the log-average luminance of the HDR image to reconstruct; 'reference' "
                         "(with --hdr-reference): that of each file's reference")
    ap.add_argument("--hdr-reference", default=None, metavar="DIR",
                    help="with --hdr: directory of ground-truth HDR files (.hdr / .pic / .pfm / .exr); score each "
                         "written reconstruction against the same-stem file (PQ PSNR and SSIM, hdrmetrics)")
    ap.add_argument("--hdr-metrics-csv", default=None,
                    help="with --hdr-reference: write name;psnr;ssim;scale_pred;scale_ref rows to this file")
    ap.add_argument("--max-side", type=int, default=None,
                    help="resize a frame whose longer side exceeds N to fit it before inference (antialiased, "
                         "GPU, PIL's arithmetic on the 8-bit frame); the outputs have the resized size")
    ap.add_argument("--resample", default="bilinear", choices=["box", "bilinear", "bicubic", "lanczos"],
                    help="the filter of --max-side")
    a = ap.parse_args(argv)
    if a.max_side is not None and a.max_side < 1:
        ap.error("--max-side takes a positive integer")
    if a.metrics_csv and not a.reference:
        ap.error("--metrics-csv needs --reference")
    if a.ms_ssim and not a.reference:
        ap.error("--ms-ssim needs --reference")
    if a.hdr_reference and not a.hdr:
        ap.error("--hdr-reference needs --hdr")
    if a.hdr_metrics_csv and not a.hdr_reference:
        ap.error("--hdr-metrics-csv needs --hdr-reference")
    if a.hdr_log_average == "reference" and not (a.hdr_reference and a.hdr_mode == "exact"):
        ap.error("--hdr-log-average reference needs --hdr-mode exact and --hdr-reference")
    tile = tuple(int(v) for v in a.tile.split(",")) if a.tile else None
    from .model import load_model
    m = load_model(a.model)
    if m.optimizer is None:
        m.compile(optimizer="rmsprop", loss="mse", metrics=["accuracy"])
    m.set_dtype(a.dtype)
    out = predict_dir(m, a.input, a.output, a.batch, tile=tile, reference=a.reference, metrics_csv=a.metrics_csv,
                      hdr_dir=a.hdr, hdr_format=a.hdr_format, hdr_mode=a.hdr_mode, hdr_key=a.hdr_key,
                      hdr_log_average=a.hdr_log_average, hdr_reference=a.hdr_reference,
                      hdr_metrics_csv=a.hdr_metrics_csv, ms_ssim=a.ms_ssim, max_side=a.max_side,
                      resample=a.resample)
    print(f"wrote {len(out)} predictions to {a.output}")
    if a.hdr:
        print(f"wrote {len(out)} .{a.hdr_format} reconstructions to {a.hdr}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
