"""Antialiased image resampling on the GPU with Pillow's arithmetic: ``resize``.

``resize(x, (oh, ow), filter)`` is what ``PIL.Image.resize`` computes -- byte for byte for uint8
RGB, bit for bit for float32 (which PIL can only do one channel at a time, mode ``F``) -- for the
filters ``'box'``, ``'bilinear'``, ``'bicubic'`` and ``'lanczos'``: a separable filter whose support
grows with the reduction, so that every source pixel contributes.  The arithmetic is stated in
include/cnn_itmo.h (cnnitmo_resize) and restated in numpy in tests/resize_ref.py; the kernels are in
csrc/resize.hip.  The coefficient tables come from the library's host function
``cnnitmo_resize_coeffs`` (``coefficients``), are uploaded in one copy, and that upload is the only
point at which a call waits for the host.

    small = resize(hdr, fit_within(h, w, 1024))                   # fp32 [h,w,3] -> CUDA fp32
    thumb = resize(frames_u8, (540, 960), "lanczos")              # uint8 [n,h,w,3] -> CUDA uint8
"""
from __future__ import annotations

import numpy as np

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
NEGATIVE_LOBES = ("bicubic", "lanczos")  # filters that can undershoot next to a highlight


def _filter_id(filter):
    from . import ops
    if filter not in ops.RESIZE_FILTERS:
        raise ValueError(f"filter {filter!r}: one of {', '.join(FILTERS)}")
    return ops.RESIZE_FILTERS[filter]


def _positive(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} {v!r}: a positive integer")
    return int(v)


def coefficients(n_in, n_out, filter="bilinear"):
    """The tables of one axis, ``n_in`` -> ``n_out`` samples: ``(bounds, kk)``, numpy int32
    ``[n_out, 2]`` = (first source sample, tap count) and float64 ``[n_out, ksize]``, the normalised
    taps, zero beyond the count.  Computed by the library (host code, no GPU needed)."""
    from . import ops
    fid = _filter_id(filter)
    return ops.resize_coeffs(_positive("n_in", n_in), _positive("n_out", n_out), fid)


def fit_within(h, w, max_side):
    """``(oh, ow)`` of an ``h`` x ``w`` picture made to fit ``max_side``: the longer side becomes
    ``max_side``, the other ``max(1, round(other * max_side / longer))`` with halves rounded up
    (in integers: ``(2 * other * max_side + longer) // (2 * longer)``); a picture whose longer side
    is at most ``max_side`` keeps its size."""
    h, w, m = _positive("h", h), _positive("w", w), _positive("max_side", max_side)
    longer = max(h, w)
    if longer <= m:
        return h, w

    def other(v):
        return max(1, (2 * v * m + longer) // (2 * longer))
    return (m, other(w)) if h >= w else (other(h), m)


def resize(x, size, filter="bilinear", floor=None):
    """``x``: numpy array or CUDA tensor, ``[h,w,3]`` or ``[n,h,w,3]``, floating point or uint8;
    ``size`` = ``(oh, ow)``.  Returns a CUDA tensor of the same rank: float32 for a float input,
    uint8 for uint8.  ``floor`` (float pictures only): values below it are raised to it where the
    result is stored, a NaN stays a NaN; ``None`` is PIL's behaviour.  An axis that keeps its
    size is not filtered; equal sizes give a copy."""
    import torch
    from . import ops
    fid = _filter_id(filter)
    try:
        oh, ow = size
    except (TypeError, ValueError):
        raise ValueError(f"size {size!r}: (oh, ow)") from None
    oh, ow = _positive("oh", oh), _positive("ow", ow)
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        t = torch.from_numpy(a if a.flags.writeable else a.copy())  # torch wants a writable array
    else:
        t = x
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"x: a numpy array or a torch tensor, not {type(x).__name__}")
    if t.ndim not in (3, 4) or t.shape[-1] != 3 or min(t.shape) < 1:
        raise ValueError(f"x: expected [h,w,3] or [n,h,w,3], got {tuple(t.shape)}")
    if t.dtype == torch.uint8:
        if floor is not None:
            raise ValueError("floor is for float pictures, not uint8")
    elif not t.dtype.is_floating_point:
        raise ValueError(f"x: float or uint8, not {t.dtype}")
    lo = float("-inf") if floor is None else float(floor)
    if lo != lo:
        raise ValueError("floor is NaN")
    if not isinstance(x, np.ndarray) and not t.is_cuda:
        raise ValueError("x: a tensor must be on the GPU (pass host data as numpy)")
    t = t.cuda()
    if t.dtype != torch.uint8:
        t = t.to(torch.float32)
    t = t.contiguous()
    x4 = t if t.ndim == 4 else t.unsqueeze(0)
    n, h, w, _ = x4.shape
    # one upload: the fp64 taps of both axes, then their int32 bounds
    tabs = {a: ops.resize_coeffs(i, o, fid) for a, i, o in (("x", w, ow), ("y", h, oh)) if i != o}
    dev_tabs = {"x": None, "y": None}
    if tabs:
        order = sorted(tabs)
        parts = [tabs[a][1].view(np.uint8).reshape(-1) for a in order] + \
                [tabs[a][0].view(np.uint8).reshape(-1) for a in order]
        dev = torch.from_numpy(np.concatenate(parts)).to(x4.device)
        cuts = np.cumsum([0] + [p.size for p in parts])
        for i, a in enumerate(order):
            kk = dev[cuts[i]:cuts[i + 1]].view(torch.float64).view(tabs[a][1].shape)
            j = len(order) + i
            dev_tabs[a] = (dev[cuts[j]:cuts[j + 1]].view(torch.int32).view(-1, 2), kk)
    out = torch.empty((n, oh, ow, 3), dtype=x4.dtype, device=x4.device)
    ops.resize(x4, out, dev_tabs["x"], dev_tabs["y"], lo=lo)
    return out if t.ndim == 4 else out[0]
