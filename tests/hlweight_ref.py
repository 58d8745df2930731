"""numpy float64 reference of the highlight-weighted training loss and its gradient
(csrc/hlweight.hip).

Per pixel p of a mask source s, a prediction y and a target t, [n,h,w,3]:

    m   = max_c s[p][c]
    a   = fmin(fmax((m - tau) / (1 - tau), 0), 1)      (a NaN gives 0, m == tau exactly 0)
    wgt = 1 + gain a
    l   = (y-t)^2 ('mse') or |y-t| ('mae'),   l' = 2 (y-t) or sign(y-t), sign(0) = 0

and per image i, N = h w 3:  A = sum_p a / (h w),  B = sum l / N,  L = sum wgt l / N,
H = sum a l / (3 sum_p a) (0 if sum_p a == 0).  ``loss_grad`` returns out [n,4] = {A, B, L, H}
and dy = (wgt l') / (F N), F = frames (None: n), the operations in the kernel's order so that
the fp64 values agree; only the order of the sums is numpy's.  tests/test_hlweight_host.py
checks dy against central differences of sum_i L_i / F.  Everything is float64 whatever the
arguments' dtype; ``oracle_loss`` / ``oracle_grad_z`` (what UNetRef.backward looks up as ``mse`` /
``mse_grad_z``) return the dtype of y.
"""
import numpy as np

BASES = ("mae", "mse")
BASE_IDS = {"mae": 1, "mse": 2}  # CNNITMO_BASE_*


def _batch(v):
    v = np.asarray(v, np.float64)
    return v[None] if v.ndim == 3 else v


def mask(s, tau):
    """a [n,h,w]."""
    s = _batch(s)
    m = np.fmax(np.fmax(s[..., 0], s[..., 1]), s[..., 2])
    return np.fmin(np.fmax((m - float(tau)) / (1.0 - float(tau)), 0.0), 1.0)


def loss_grad(s, y, t, base, tau, gain, frames=None):
    """(out [n,4] = {A, B, L, H}, dy [n,h,w,3] = d(sum_i L_i / frames)/dy)."""
    if base not in BASES:
        raise ValueError(base)
    s, y, t = _batch(s), _batch(y), _batch(t)
    n, h, w, _ = y.shape
    a = mask(s, tau)[..., None]
    wgt = 1.0 + float(gain) * a
    d = y - t
    if base == "mse":
        l, lp = d * d, 2.0 * d
    else:
        l, lp = np.abs(d), np.sign(d)
    n_elem = float(h * w * 3)
    sa = a.sum(axis=(1, 2, 3))
    out = np.empty((n, 4))
    out[:, 0] = sa / float(h * w)
    out[:, 1] = l.sum(axis=(1, 2, 3)) / n_elem
    out[:, 2] = (wgt * l).sum(axis=(1, 2, 3)) / n_elem
    sal = (a * l).sum(axis=(1, 2, 3))
    out[:, 3] = np.where(sa == 0.0, 0.0, sal / np.where(sa == 0.0, 1.0, 3.0 * sa))
    f = float(n if frames is None else frames)
    return out, (wgt * lp) / (f * n_elem)


def oracle_loss(s, base, tau, gain):
    """UNetRef's ``mse(yhat, t)`` for this loss: the batch mean of L_i.  s: the mask source
    (the input's valid rows), or None for the target."""
    return lambda y, t: float(loss_grad(t if s is None else s, y, t, base, tau, gain)[0][:, 2].mean())


def oracle_grad_z(s, base, tau, gain):
    """UNetRef's ``mse_grad_z(yhat, t)``: dy * y(1-y), in the dtype of y."""
    def f(y, t):
        dy = loss_grad(t if s is None else s, y, t, base, tau, gain)[1]
        y64 = np.asarray(y, np.float64)
        return (dy * y64 * (1.0 - y64)).astype(np.asarray(y).dtype)
    return f


def patch_oracle(monkeypatch, R, s_valid, base, tau, gain):
    """Point oracle.unet_ref's loss at this loss, as dssim_ref.patch_oracle does.  s_valid: the
    mask source in the prediction's layout (source='input': the input's valid rows), None for
    source='target'."""
    monkeypatch.setattr(R, "mse", oracle_loss(s_valid, base, tau, gain))
    monkeypatch.setattr(R, "mse_grad_z", oracle_grad_z(s_valid, base, tau, gain))


def make_case(shape, tau, seed, source="input", flat_image=None, full_image=None, equal_every=7):
    """(s, y, t) fp32 [n,h,w,3] whose every image mixes pixels with m < tau, m == tau exactly (tau
    must be an fp32 value), m inside the ramp and m == 1.0, laid out with a stride of 5 that is
    coprime to the kernel's 4-pixel groups; every `equal_every`-th element has y == t.
    flat_image: that image has no pixel above tau (A = H = 0 exactly); full_image: every pixel
    of that image has m == 1.  source 'target': t is s (the mask comes from the target)."""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    tau32 = np.float32(tau)
    assert float(tau32) == float(tau)
    s = (rng.uniform(0.0, 1.0, (n, h * w, 3)) * float(tau) * 0.98).astype(np.float32)  # all below tau
    kind = (np.arange(h * w)[None, :] + np.arange(n)[:, None]) % 5
    for i in range(n):
        ch = rng.integers(0, 3, h * w)
        px = np.arange(h * w)
        k = kind[i]
        at = px[k == 1]
        s[i, at, ch[at]] = tau32
        ramp = px[k == 2]
        s[i, ramp, ch[ramp]] = (float(tau) + (1.0 - float(tau)) * rng.uniform(0.05, 0.95, ramp.size)).astype(np.float32)
        top = px[k == 3]
        s[i, top, ch[top]] = 1.0
        over = px[k == 4][::2]  # some above 1 (a clips at 1)
        s[i, over, ch[over]] = 1.25
    if flat_image is not None:
        s[flat_image] = np.minimum(s[flat_image], tau32)
    if full_image is not None:
        s[full_image, :, 0] = 1.0
    t = s.copy() if source == "target" else rng.uniform(0.0, 1.0, (n, h * w, 3)).astype(np.float32)
    y = np.clip(t + rng.normal(0.0, 0.1, t.shape), 0.0, 1.0).astype(np.float32)
    yf, tf = y.reshape(-1), t.reshape(-1)
    yf[::equal_every] = tf[::equal_every]
    return s.reshape(n, h, w, 3), y.reshape(n, h, w, 3), t.reshape(n, h, w, 3)
