"""Training pairs straight from HDR files, on the GPU: ``HDRPairGenerator``.

The offline route (make_dataset, then two seed-locked ``ImageDataGenerator.flow_from_directory``
streams) writes 8-bit PNGs of ``tonemap.reinhard`` / ``tonemap.virtual_camera`` and re-decodes and
warps them every epoch: targets quantised to 1/255, the camera draws frozen when the data set is
built.  Here the HDR pictures stay on the device in their file format (RGBE bytes for ``.hdr`` /
``.pic``, fp32 for ``.pfm``; an ``.exr`` is unpacked to fp32 on the device once per load, exr.py)
and one ``cnnitmo_hdr_pairs`` call (csrc/hdrpairs.hip) makes a batch:
it gathers a warped window of each picture, takes its log-average and writes the virtual-camera
input ``x`` and the Reinhard target ``y``.  No pixel is touched on the host.

    gen = HDRPairGenerator(rotation_range=90, horizontal_flip=True, vertical_flip=True, zoom_range=0.2)
    it = gen.flow_from_directory("hdr/", target_size=(512, 512), batch_size=32, seed=1)
    model.fit_generator(it, steps_per_epoch=len(it), epochs=100)

The iterator is a ``datagen.Iterator``: the same reseeding before every batch, permutation, rank
sharding (every rank replays the draws of the whole global batch and keeps its ``_local`` share)
and ``last_global_batch``.  Per frame of the global batch the draws are, from the iterator's
``RandomState`` and in this order:

1. ``ImageDataGenerator.get_random_transform`` at ``target_size`` (the geometric arguments);
2. the window of ``window_size`` (default ``target_size``) inside the picture -- ``'random'``:
   ``top = randint(0, hs-ch+1)`` then ``left = randint(0, ws-cw+1)``; ``'center'`` and ``'full'``
   (the whole picture) draw nothing;
3. ``cameras='random'``: ``v = 8*random_sample() - 4``, ``n = normal(0.6, sqrt(0.1))`` redrawn while
   <= 0, then ``y = normal(0.9, sqrt(0.1))`` redrawn while <= 0.  virtual_camera.m draws n and y
   unbounded; a non-positive one makes the curve singular, which a training stream cannot shrug off
   as an offline tool can.  ``cameras='fixed'`` draws nothing: file j always gets element 0 of
   ``tonemap.virtual_camera_params(1, np.random.default_rng(seed + j))``, make_dataset's
   ``--cameras 1`` values (a seed of None counts as 0), so validation batches repeat every epoch.
4. only with ``jpeg_quality`` set (the stream of a generator without it is unchanged):
   ``u = random_sample()``, then for a range ``(lo, hi)`` the quality ``q = randint(lo, hi + 1)``,
   drawn whether or not the frame is compressed, so the position of the stream does not depend on
   outcomes; the frame is compressed iff ``u < jpeg_prob``.  With ``cameras='fixed'`` nothing is
   drawn from the stream here either: file j takes ``u = random()`` and then, for a range,
   ``q = integers(lo, hi + 1)`` from its own ``default_rng(seed + j)``, after the camera's values.
   The draw's ``'jpeg'`` is the quality, 0 for a frame that is not compressed.
5. only with sensor noise on (``noise_shot`` or ``noise_read`` set; the stream of every generator
   without it, with or without JPEG, is unchanged): for ``noise_shot``, then ``noise_read``, a range
   ``(lo, hi)`` draws ``exp(log lo + random_sample() * (log hi - log lo))`` and a float draws
   nothing; then the frame's key ``k0 = randint(0, 2**32) * 2**32 + randint(0, 2**32)`` (``k1`` is 0).
   With ``cameras='fixed'`` file j takes the same values from its own ``default_rng(seed + j)``,
   after the JPEG values, through ``random`` and ``integers``.  The draw's ``'noise'`` is
   ``(a, b, k0)``, ``None`` when noise is off.

The matrix handed to the kernel maps an output pixel to the source picture:
``M_src = T(top, left) . S . M_keras``, with ``M_keras`` the ``ImageDataGenerator.affine`` matrix at
``target_size`` and ``S`` the centre-aligned resize ``src = (dst + 0.5) * (ch / H) - 0.5`` (the
identity when the window has the target size); the bilinear taps are clamped to the window.

``quantize``: ``'input'`` (default) rounds x to the 8-bit levels an SDR file has and leaves the
target in fp32; ``'both'`` also rounds y (what the PNG route trains on); ``None`` rounds neither.

``response``: ``'luminance'`` (default) is virtual_camera.m: the camera curve and the clip at 1 act on
the luminance and the three channels share one factor, so a highlight keeps its hue however far it
is overexposed.  ``'channel'`` exposes every channel on its own, ``e_c = key 2^v / G * hdr_c``, and
puts each through the curve and the clip, as a sensor whose channels reach full well one after the
other: a red lamp goes R = 1, then yellow, then white.  G is the log-average of the luminance in
both, and the target y is the same.

``noise_shot`` / ``noise_read``: ``None`` (default), a non-negative float or a range ``(lo, hi)`` with
``0 < lo <= hi``, drawn log-uniformly per frame; either one turns sensor noise on (the other then
counts as 0), which needs ``response='channel'``: the model lives on channel exposures.  Before the
curve every exposure becomes ``max(0, e + sqrt(a max(e, 0) + b^2) z)`` with ``a`` the shot-noise factor
(1 / full-well electrons), ``b`` the read-noise standard deviation in units of full well and ``z`` a
standard normal: signal-dependent noise, strongest relative to the signal in the shadows.  ``z``
comes from Philox4x64-10 (numpy's ``np.random.Philox``) inside the kernel, keyed by the frame's
drawn key and counted by the pixel's index in the frame (csrc/sensor_px.h), so a frame's noise is the
same bits on any rank, at any batch position and in any batch size.  The order is a camera's:
noise, curve, quantisation, JPEG.  The target y carries no noise.

``jpeg_quality``: ``None`` (default) leaves x as the camera made it; an int or an inclusive range
``(lo, hi)`` of libjpeg qualities puts each input, with probability ``jpeg_prob``, through a
baseline-JPEG round trip on the GPU (``degrade.jpeg_roundtrip``'s kernel, ``jpeg_subsampling``
``'4:2:0'`` or ``'4:4:4'``), the compression the SDR material in the wild has been through.  The target
y is never touched.  JPEG codes 8-bit samples, so ``quantize=None`` with it is a ``ValueError``.

``flow_from_directory(..., max_side=N, resample='bilinear')``: a picture whose longer side exceeds
``N`` is decoded when it is first loaded and made smaller once on the GPU, to
``resize.fit_within(h, w, N)`` with the antialiased filter ``resample`` (``resize.resize``, PIL's
arithmetic), and kept as an fp32 source; ``sizes``, the window draws and the "smaller than the
window" check refer to the resized sizes.  So a 512 x 512 window shows a light source together with
its surroundings, and no highlight falls between the taps of the pair kernel's bilinear gather.
``'bicubic'`` and ``'lanczos'`` have negative lobes: their result is floored at 0, since negative
radiance next to a highlight would make the log-average a NaN.  With ``max_side=None`` (default)
nothing changes: the same draws, bits and launches.  With ``cache=False`` the decode and the
resize repeat every time a picture is loaded.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import re

import numpy as np

from . import degrade, exr, hdrio, resize
from .datagen import ImageDataGenerator, Iterator
from .make_dataset import EXTENSIONS

QUANTIZE = {None: 0, "input": 1, "both": 3}
RESPONSES = {"luminance": 0, "channel": 1}  # cnnitmo_hdr_pairs_sensor's response


def noise_level(name, v):
    """None, a float >= 0 -> (v, v) or a range 0 < lo <= hi -> (lo, hi), as floats."""
    if v is None:
        return None
    if np.ndim(v) == 0:
        v = float(v)
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"{name} {v!r}: a finite value >= 0")
        return (v, v)
    lo, hi = (float(t) for t in v)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi):
        raise ValueError(f"{name} {v!r}: a range (lo, hi) with 0 < lo <= hi")
    return (lo, hi)


def image_size(path):
    """(h, w) of a ``.hdr`` / ``.pic`` / ``.pfm`` / ``.exr`` file from its header alone."""
    if os.path.splitext(path)[1].lower() == ".exr":
        return exr.exr_size(path)
    with open(path, "rb") as fh:
        buf = fh.read(1 << 16)
    if os.path.splitext(path)[1].lower() == ".pfm":
        m = re.match(rb"PF\s+(\d+)\s+(\d+)\s", buf)
        if not m:
            raise ValueError(f"{path}: not a colour PFM file")
        return int(m.group(2)), int(m.group(1))
    first, pos = hdrio._line(buf, 0)
    if not first.startswith(hdrio.MAGICS):
        raise ValueError(f"{path}: missing #?RADIANCE / #?RGBE magic line")
    raw = first
    while raw:
        raw, pos = hdrio._line(buf, pos)
    res, _ = hdrio._line(buf, pos)
    m = re.fullmatch(r"[-+]Y +(\d+) +\+X +(\d+)", res.decode("latin-1").strip())
    if not m:
        raise ValueError(f"{path}: bad or unsupported resolution line {res!r}")
    return int(m.group(1)), int(m.group(2))


def read_source(path):
    """A picture in its file format, row 0 = top: RGBE uint8 [h,w,4] (``.hdr`` / ``.pic``, as
    hdrio.parse_hdr returns it), float32 [h,w,3] (``.pfm``) or an exr.Parsed (``.exr``: the
    inflated chunks, which the GPU unpacks to float32 [h,w,3] when the source is uploaded)."""
    if os.path.splitext(path)[1].lower() == ".exr":
        with open(path, "rb") as fh:
            return exr.parse_exr(fh.read())
    if os.path.splitext(path)[1].lower() == ".pfm":
        return np.ascontiguousarray(hdrio.read_pfm(path))
    with open(path, "rb") as fh:
        return hdrio.parse_hdr(fh.read())[1]


def resize_matrix(ch, cw, h, w):
    """S: target pixel -> window pixel, centres aligned; the identity for a window of target size."""
    sr, sc = ch / h, cw / w
    return np.array([[sr, 0, 0.5 * sr - 0.5], [0, sc, 0.5 * sc - 0.5], [0, 0, 1]])


class HDRPairGenerator:
    """The geometric arguments are ``ImageDataGenerator``'s; ``key`` / ``lum`` those of
    ``tonemap.reinhard`` / ``tonemap.virtual_camera``; ``response``, ``noise_shot`` and ``noise_read``: the
    sensor in front of the camera curve, see the module's docstring."""

    def __init__(self, rotation_range=0, zoom_range=0, horizontal_flip=False, vertical_flip=False, shear_range=0,
                 width_shift_range=0, height_shift_range=0, key=0.18, lum=None, quantize="input", cameras="random",
                 jpeg_quality=None, jpeg_prob=1.0, jpeg_subsampling="4:2:0", response="luminance", noise_shot=None,
                 noise_read=None):
        if quantize not in QUANTIZE:
            raise ValueError(f"quantize {quantize!r}: 'input', 'both' or None")
        if cameras not in ("random", "fixed"):
            raise ValueError(f"cameras {cameras!r}: 'random' or 'fixed'")
        self.geometry = ImageDataGenerator(rotation_range=rotation_range, zoom_range=zoom_range,
                                           horizontal_flip=horizontal_flip, vertical_flip=vertical_flip,
                                           shear_range=shear_range, width_shift_range=width_shift_range,
                                           height_shift_range=height_shift_range)
        self.key = float(key)
        self.lum = None if lum is None else tuple(float(c) for c in lum)
        self.quantize, self.cameras = quantize, cameras
        self.jpeg = None  # (lo, hi) qualities, inclusive
        self.jpeg_range = bool(np.ndim(jpeg_quality))  # a range draws its quality, an int does not
        if jpeg_quality is not None:
            lo, hi = jpeg_quality if np.ndim(jpeg_quality) else (jpeg_quality, jpeg_quality)
            self.jpeg = (degrade.check_quality(lo), degrade.check_quality(hi))
            if self.jpeg[0] > self.jpeg[1]:
                raise ValueError(f"jpeg_quality {jpeg_quality!r}: lo > hi")
            if quantize is None:
                raise ValueError("jpeg_quality needs 8-bit inputs: quantize 'input' or 'both', not None")
        if not 0.0 <= jpeg_prob <= 1.0:
            raise ValueError(f"jpeg_prob {jpeg_prob!r}: a probability in [0, 1]")
        if jpeg_subsampling not in degrade.SUBSAMPLINGS:
            raise ValueError(f"jpeg_subsampling {jpeg_subsampling!r}: '4:4:4' or '4:2:0'")
        self.jpeg_prob, self.jpeg_subsampling = float(jpeg_prob), jpeg_subsampling
        if response not in RESPONSES:
            raise ValueError(f"response {response!r}: 'luminance' or 'channel'")
        self.response = response
        self.noise = None  # ((lo, hi) of shot, (lo, hi) of read); a range draws its value, a float does not
        if noise_shot is not None or noise_read is not None:
            if response != "channel":
                raise ValueError("sensor noise is defined on channel exposures: it needs response='channel'")
            self.noise = tuple(noise_level(k, v) or (0.0, 0.0)
                               for k, v in (("noise_shot", noise_shot), ("noise_read", noise_read)))
            self.noise_range = (bool(np.ndim(noise_shot)), bool(np.ndim(noise_read)))

    def jpeg_draw(self, uniform, integers):
        """Step 4 of a frame's draws from the two given callables: the quality, 0 = not compressed."""
        lo, hi = self.jpeg
        u = uniform()
        q = int(integers(lo, hi + 1)) if self.jpeg_range else lo
        return q if u < self.jpeg_prob else 0

    def noise_draw(self, uniform, integers):
        """Step 5 of a frame's draws from the two given callables: (a, b, k0)."""
        ab = []
        for (lo, hi), ranged in zip(self.noise, self.noise_range):
            ab.append(float(np.exp(np.log(lo) + uniform() * (np.log(hi) - np.log(lo)))) if ranged else lo)
        k0 = int(integers(0, 2 ** 32)) * 2 ** 32 + int(integers(0, 2 ** 32))
        return ab[0], ab[1], k0

    def flow_from_directory(self, hdr_dir, target_size, window="random", window_size=None, batch_size=32,
                            shuffle=True, seed=None, cache=True, workers=8, rank=None, world=None, output="cuda",
                            max_side=None, resample="bilinear"):
        """``batch_size`` is per rank; ``rank`` / ``world`` as ``ImageDataGenerator.flow_from_directory``.
        ``max_side`` / ``resample``: see the module's docstring; with ``cache=False`` a picture is
        decoded and resized again every time it is loaded."""
        return HDRPairIterator(hdr_dir, self, target_size, window, window_size, batch_size, shuffle, seed, cache,
                               workers, rank, world, output, max_side, resample)


class HDRPairIterator(Iterator):
    """Yields ``(x, y)``: fp32 CUDA tensors [B, H, W, 3] (numpy arrays with ``output='numpy'``)."""

    def __init__(self, hdr_dir, gen, target_size, window, window_size, batch_size, shuffle, seed, cache, workers,
                 rank=None, world=None, output="cuda", max_side=None, resample="bilinear"):
        if window not in ("random", "center", "full"):
            raise ValueError(f"window {window!r}: 'random', 'center' or 'full'")
        if output not in ("cuda", "numpy"):
            raise ValueError(f"output {output!r}: 'cuda' or 'numpy'")
        self.gen, self.target_size, self.window = gen, tuple(int(v) for v in target_size), window
        self.window_size = self.target_size if window_size is None else tuple(int(v) for v in window_size)
        self.cache, self.output = bool(cache), output
        names = sorted(f for f in os.listdir(hdr_dir) if os.path.splitext(f)[1].lower() in EXTENSIONS)
        if not names:
            raise FileNotFoundError(f"no {'/'.join(EXTENSIONS)} files in {hdr_dir}")
        self.filenames = [os.path.join(hdr_dir, f) for f in names]
        self.file_sizes = self.sizes = [image_size(f) for f in self.filenames]
        self.max_side, self.resample = max_side, resample
        if max_side is not None:
            if resample not in resize.FILTERS:
                raise ValueError(f"resample {resample!r}: one of {', '.join(resize.FILTERS)}")
            self.sizes = [resize.fit_within(hs, ws, max_side) for hs, ws in self.file_sizes]
        if window != "full":
            ch, cw = self.window_size
            for f, (hs, ws) in zip(self.filenames, self.sizes):
                if hs < ch or ws < cw:
                    raise ValueError(f"{f}: a {hs} x {ws} picture is smaller than the {ch} x {cw} window")
        self.fixed_cameras = self.fixed_jpeg = self.fixed_noise = None
        if gen.cameras == "fixed":
            from .tonemap import virtual_camera_params
            base = 0 if seed is None else seed
            self.fixed_cameras, self.fixed_jpeg, self.fixed_noise = [], [], []
            for j in range(len(names)):
                own = np.random.default_rng(base + j)
                self.fixed_cameras.append(tuple(float(a[0]) for a in virtual_camera_params(1, own)))
                self.fixed_jpeg.append(gen.jpeg_draw(own.random, own.integers) if gen.jpeg else 0)
                self.fixed_noise.append(gen.noise_draw(own.random, own.integers) if gen.noise else None)
        self._sources = {}
        self._pool = cf.ThreadPoolExecutor(max_workers=workers)
        self.last_draws = None
        print(f"Found {len(names)} HDR images.")
        super().__init__(len(names), batch_size, shuffle, seed, rank, world)

    # ---- the random stream (host only) ----------------------------------------------------
    def _draw(self, index_array):
        """The draws of every frame of the global batch, in the documented order; returns this
        rank's share as dicts (j, params, top, left, ch, cw, camera = (v, n, y), jpeg = quality or 0,
        noise = (a, b, k0) or None)."""
        h, w = self.target_size
        rng, draws = self.rng, []
        for j in index_array:
            j = int(j)
            params = self.gen.geometry.get_random_transform((h, w, 3), rng)
            hs, ws = self.sizes[j]
            ch, cw = (hs, ws) if self.window == "full" else self.window_size
            if self.window == "random":
                top = int(rng.randint(0, hs - ch + 1))
                left = int(rng.randint(0, ws - cw + 1))
            else:
                top, left = (hs - ch) // 2, (ws - cw) // 2
            if self.fixed_cameras is not None:
                camera = self.fixed_cameras[j]
            else:
                v = 8 * rng.random_sample() - 4
                n = rng.normal(0.6, np.sqrt(0.1))
                while n <= 0:
                    n = rng.normal(0.6, np.sqrt(0.1))
                y = rng.normal(0.9, np.sqrt(0.1))
                while y <= 0:
                    y = rng.normal(0.9, np.sqrt(0.1))
                camera = (float(v), float(n), float(y))
            jpeg = 0
            if self.gen.jpeg:
                jpeg = self.fixed_jpeg[j] if self.fixed_jpeg is not None else \
                    self.gen.jpeg_draw(rng.random_sample, rng.randint)
            noise = None
            if self.gen.noise:
                noise = self.fixed_noise[j] if self.fixed_noise is not None else \
                    self.gen.noise_draw(rng.random_sample, rng.randint)
            draws.append({"j": j, "params": params, "top": top, "left": left, "ch": ch, "cw": cw, "camera": camera,
                          "jpeg": jpeg, "noise": noise})
        lo, hi = self._local(len(draws))
        return draws[lo:hi]

    def next_draws(self):
        """Advance the stream by one batch and return its draws without producing pixels."""
        blk = next(self._gen)
        self.last_global_batch = len(blk)
        self.last_draws = self._draw(blk)
        return self.last_draws

    def source_matrix(self, d):
        """(M_src [6] float64, flip bits) of one draw: output pixel -> source-picture pixel."""
        h, w = self.target_size
        m6, flips = ImageDataGenerator.affine(d["params"], h, w)
        m = np.vstack([m6.reshape(2, 3), [0.0, 0.0, 1.0]])
        t = np.array([[1, 0, d["top"]], [0, 1, d["left"]], [0, 0, 1]], np.float64)
        m = np.dot(t, np.dot(resize_matrix(d["ch"], d["cw"], h, w), m))
        return m[:2].reshape(-1).astype(np.float64), flips

    # ---- pixels (GPU) -----------------------------------------------------------------------
    def _load(self, js):
        """{j: device tensor in file format}; cached files are uploaded on first use."""
        have = self._sources if self.cache else {}
        missing = sorted(set(js) - set(have))
        arrays = list(self._pool.map(lambda j: read_source(self.filenames[j]), missing))
        if missing:
            import torch
            for j, a in zip(missing, arrays):
                if tuple(a.shape[:2]) != self.file_sizes[j]:
                    raise ValueError(f"{self.filenames[j]}: the picture changed size since its header was read")
                t = exr.unpack(a) if isinstance(a, exr.Parsed) else torch.from_numpy(a).cuda()
                if self.sizes[j] != self.file_sizes[j]:
                    t = self._shrink(t, self.sizes[j])
                have[j] = t
        return have

    def _shrink(self, t, size):
        """A source in file format -> fp32 [oh,ow,3], resized once on the GPU."""
        import torch
        from . import ops
        if t.dtype == torch.uint8:
            t = ops.rgbe_decode(t, torch.empty(t.shape[:2] + (3,), dtype=torch.float32, device=t.device))
        return resize.resize(t, size, self.resample, floor=0.0 if self.resample in resize.NEGATIVE_LOBES else None)

    def _batch(self, index_array):
        import torch
        from . import ops
        draws = self.last_draws = self._draw(index_array)
        n = len(draws)
        h, w = self.target_size
        have = self._load([d["j"] for d in draws])
        srcs = [have[d["j"]] for d in draws]
        desc = ops.hdr_descriptors(srcs, [(d["top"], d["left"], d["top"] + d["ch"] - 1, d["left"] + d["cw"] - 1)
                                          for d in draws])
        mats, flips = zip(*[self.source_matrix(d) for d in draws])
        cam = np.array([[self.gen.key * 2.0 ** d["camera"][0], d["camera"][1], d["camera"][2]] for d in draws],
                       np.float64)
        # one upload: descriptors, matrices, cameras, with noise its levels and keys (8-byte items), then the flips
        parts = [desc.view(np.uint8).reshape(-1), np.stack(mats).view(np.uint8).reshape(-1),
                 cam.view(np.uint8).reshape(-1)]
        if self.gen.noise:
            parts += [np.array([d["noise"][:2] for d in draws], np.float64).view(np.uint8).reshape(-1),
                      np.array([[d["noise"][2], 0] for d in draws], np.uint64).view(np.uint8).reshape(-1)]
        parts.append(np.asarray(flips, np.int32).view(np.uint8))
        dev = torch.from_numpy(np.concatenate(parts)).cuda()
        cuts = np.cumsum([0] + [p.size for p in parts])
        d_desc, d_mats, d_cam, *d_noise, d_flips = (dev[cuts[k]:cuts[k + 1]] for k in range(len(parts)))
        x = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev.device)
        y = torch.empty_like(x)
        if self.gen.response == "luminance":  # noise needs 'channel'
            ops.hdr_pairs(d_desc, d_mats.view(torch.float64), d_flips.view(torch.int32), d_cam.view(torch.float64),
                          x, y, key=self.gen.key, lum=self.gen.lum, quantize=QUANTIZE[self.gen.quantize])
        else:
            d_ab, d_keys = (d_noise[0].view(torch.float64), d_noise[1].view(torch.int64)) if d_noise else (None, None)
            ops.hdr_pairs_sensor(d_desc, d_mats.view(torch.float64), d_flips.view(torch.int32),
                                 d_cam.view(torch.float64), x, y, key=self.gen.key, lum=self.gen.lum,
                                 quantize=QUANTIZE[self.gen.quantize], response=RESPONSES[self.gen.response],
                                 noise=d_ab, keys=d_keys)
        if any(d["jpeg"] for d in draws):  # in place, on x alone; the tables and the flags are host arrays
            ops.jpeg_roundtrip(x, np.stack([degrade.quant_tables(d["jpeg"] or 50) for d in draws]),
                               self.gen.jpeg_subsampling, apply=[d["jpeg"] for d in draws], out=x)
        if self.output == "numpy":
            return x.cpu().numpy(), y.cpu().numpy()
        return x, y
