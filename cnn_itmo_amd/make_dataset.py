"""Training pairs from HDR files: the offline step the reference does in MATLAB
(m-files/Reinhard.m for the targets, m-files/virtual_camera.m for the inputs).

    python -m cnn_itmo_amd.make_dataset --hdr-dir D [--out data/train] [--class-dir 0] \\
        [--crop TOP,LEFT,SIZE] [--max-side N [--resample F]] [--cameras K] [--seed S] [--response R]

For every ``.hdr`` / ``.pic`` / ``.pfm`` / ``.exr`` file of D, in sorted order (file_index = 0, 1, ...):
the image is read (hdrio.load_image), optionally cropped (tonemap.crop, 1-based MATLAB
coordinates), with ``--max-side N`` made to fit N (resize.fit_within) by the antialiased GPU
resampler (resize.resize, filter F = box / bilinear / bicubic / lanczos, default bilinear; the
last two floored at 0 so that no radiance is negative), and for k = 0..K-1

    out/output1/<class-dir>/<stem>_<k>.png = tonemap.reinhard(img, out_u8=True)             the target
    out/input1/<class-dir>/<stem>_<k>.png  = tonemap.virtual_camera(img, v, n, y, out_u8=True)  the input

with (v, n, y)[k] from ``tonemap.virtual_camera_params(K, np.random.default_rng(S + file_index))``.
``--response channel`` makes the inputs with ``tonemap.virtual_camera(..., response='channel')``: every
channel clips on its own, as on a sensor; the default ``luminance`` is virtual_camera.m.
``out/params.csv`` records ``name;v;n;y`` (repr of the float64 draws, so a row reproduces its
input exactly).  Both trees hold the same names, so two ``flow_from_directory(..., seed=1)``
streams over ``out/input1`` and ``out/output1`` stay paired (main.py:82-100).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

EXTENSIONS = (".hdr", ".pic", ".pfm", ".exr")


def make_dataset(hdr_dir, out="data/train", class_dir="0", crop=None, cameras=1, seed=0, log=print,
                 max_side=None, resample="bilinear", response="luminance"):
    """Returns the list of written pair names (``<stem>_<k>.png``).  ``max_side``: after the crop and
    before the tone maps, a picture whose longer side exceeds it is resized on the GPU to
    ``resize.fit_within(h, w, max_side)`` with the filter ``resample``.  ``response``: that of
    ``tonemap.virtual_camera``."""
    from PIL import Image
    from . import hdrio, resize, tonemap
    if response not in tonemap.RESPONSES:
        raise ValueError(f"response {response!r}: 'luminance' or 'channel'")
    if max_side is not None and resample not in resize.FILTERS:
        raise ValueError(f"resample {resample!r}: one of {', '.join(resize.FILTERS)}")
    files = sorted(f for f in os.listdir(hdr_dir) if os.path.splitext(f)[1].lower() in EXTENSIONS)
    if not files:
        raise FileNotFoundError(f"no {'/'.join(EXTENSIONS)} files in {hdr_dir}")
    if cameras < 1:
        raise ValueError(f"cameras {cameras}")
    stems = [os.path.splitext(f)[0] for f in files]
    if len(set(stems)) != len(stems):
        raise ValueError(f"{hdr_dir}: two files share a stem, their PNGs would overwrite each other")
    in_dir, tgt_dir = (os.path.join(out, d, str(class_dir)) for d in ("input1", "output1"))
    os.makedirs(in_dir, exist_ok=True)
    os.makedirs(tgt_dir, exist_ok=True)
    names = []
    rows = ["name;v;n;y"]
    for fi, (f, stem) in enumerate(zip(files, stems)):
        img = hdrio.load_image(os.path.join(hdr_dir, f))
        if crop is not None:
            full = tuple(img.shape[:2])
            img = tonemap.crop(img, *crop)
            if img.shape[0] != crop[2] or img.shape[1] != crop[2]:
                raise ValueError(f"{f}: crop {crop} does not fit a {full[1]}x{full[0]} image")
        if max_side is not None:
            size = resize.fit_within(int(img.shape[0]), int(img.shape[1]), max_side)
            if size != tuple(img.shape[:2]):
                img = resize.resize(img, size, resample,
                                    floor=0.0 if resample in resize.NEGATIVE_LOBES else None)
        v, cn, cy = tonemap.virtual_camera_params(cameras, np.random.default_rng(seed + fi))
        target = tonemap.reinhard(img, out_u8=True)[0].cpu().numpy()
        for k in range(cameras):
            name = f"{stem}_{k}.png"
            sdr = tonemap.virtual_camera(img, v[k], cn[k], cy[k], out_u8=True, response=response)[0].cpu().numpy()
            Image.fromarray(target).save(os.path.join(tgt_dir, name))
            Image.fromarray(sdr).save(os.path.join(in_dir, name))
            rows.append(f"{name};{float(v[k])!r};{float(cn[k])!r};{float(cy[k])!r}")
            names.append(name)
        log(f"{f}: {img.shape[1]}x{img.shape[0]}, {cameras} pair(s)")
    with open(os.path.join(out, "params.csv"), "w", newline="") as fh:
        fh.write("\n".join(rows) + "\n")
    return names


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--hdr-dir", required=True, help="directory of .hdr / .pic / .pfm / .exr files")
    ap.add_argument("--out", default="data/train")
    ap.add_argument("--class-dir", default="0", help="the class sub-directory flow_from_directory expects")
    ap.add_argument("--crop", default=None, help="TOP,LEFT,SIZE (1-based, as imcrop in Reinhard.m:10)")
    ap.add_argument("--max-side", type=int, default=None,
                    help="after --crop: resize a picture whose longer side exceeds N to fit it (antialiased, GPU)")
    ap.add_argument("--resample", default="bilinear", choices=["box", "bilinear", "bicubic", "lanczos"],
                    help="the filter of --max-side (PIL's arithmetic)")
    ap.add_argument("--cameras", type=int, default=1, help="virtual-camera inputs per HDR file")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--response", default="luminance", choices=["luminance", "channel"],
                    help="the camera curve and its clip on the luminance (virtual_camera.m) or on every channel")
    a = ap.parse_args(argv)
    crop = tuple(int(v) for v in a.crop.split(",")) if a.crop else None
    if crop is not None and len(crop) != 3:
        ap.error("--crop takes TOP,LEFT,SIZE")
    if a.max_side is not None and a.max_side < 1:
        ap.error("--max-side takes a positive integer")
    names = make_dataset(a.hdr_dir, a.out, a.class_dir, crop, a.cameras, a.seed, max_side=a.max_side,
                         resample=a.resample, response=a.response)
    print(f"wrote {len(names)} pairs to {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
