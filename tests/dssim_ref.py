"""numpy float64 reference of the DSSIM training loss and its gradient (csrc/dssim.hip).

Per image i of a prediction y and a target t, [n,h,w,3] in [0, 1]:

    L_i = alpha (1 - SSIM_i) + (1 - alpha) B_i,   B_i = mean |y-t| ('mae') or mean (y-t)^2 ('mse')

with metrics_ref's SSIM (window, constants, valid positions, max_val 1); without a base alpha
is 1.  ``loss_grad`` returns the per-image (ssim, B, L) and dy = d(sum_i L_i / F)/dy, F =
grad_frames (None: n).  The SSIM part of the gradient is written from the Gaussian-weighted
moments at each map position q,

    A1 = 2 my mt + C1, A2 = 2 cov + C2, B1 = my^2 + mt^2 + C1, B2 = vy + vt + C2, S = A1 A2/(B1 B2)
    Pc = 2 A1/(B1 B2),  Pb = -2 S/B2,  Pa = 2 mt A2/(B1 B2) - 2 my S/B1 - mt Pc - my Pb
    d(sum_q S_q)/dy_p = Fa_p + y_p Fb_p + t_p Fc_p,

F. the full (zero-padded) correlation of a coefficient map with the window: the adjoint of
metrics_ref._filter_valid.  tests/test_dssim_host.py checks dy against central differences.
Everything is computed in float64 whatever the arguments' dtype; ``oracle_loss`` /
``oracle_grad_z`` (what UNetRef.backward looks up as ``mse`` / ``mse_grad_z``) return the
dtype of y, so a float32 run of the oracle keeps its own arithmetic everywhere else.
"""
import numpy as np

import metrics_ref as MR

BASES = (None, "mae", "mse")
BASE_IDS = {None: 0, "mae": 1, "mse": 2}  # CNNITMO_BASE_*
C1, C2 = MR.K1 ** 2, MR.K2 ** 2


def coefficients(y, t):
    """(S, Pa, Pb, Pc), each [n, h-10, w-10, 3]."""
    g = MR.taps()
    f = MR._filter_valid
    my, mt = f(y, g), f(t, g)
    vy = f(y * y, g) - my * my
    vt = f(t * t, g) - mt * mt
    cov = f(y * t, g) - my * mt
    a1, a2 = 2 * my * mt + C1, 2 * cov + C2
    b1, b2 = my * my + mt * mt + C1, vy + vt + C2
    s = (a1 * a2) / (b1 * b2)
    pc = 2 * a1 / (b1 * b2)
    pb = -2 * s / b2
    pa = 2 * mt * a2 / (b1 * b2) - 2 * my * s / b1 - mt * pc - my * pb
    return s, pa, pb, pc


def adjoint(p, h, w):
    """Full correlation of a map [n, h-10, w-10, c] with the window: [n, h, w, c]."""
    g = MR.taps()
    n, mh, mw, c = p.shape
    v = np.zeros((n, h, mw, c))
    for i in range(MR.SIZE):
        v[:, i:i + mh] += g[i] * p
    out = np.zeros((n, h, w, c))
    for j in range(MR.SIZE):
        out[:, :, j:j + mw] += g[j] * v
    return out


def base_term(base, y, t):
    """B per image [n]."""
    if base is None:
        return np.zeros(y.shape[0])
    d = y - t
    return (np.abs(d) if base == "mae" else d * d).mean(axis=(1, 2, 3))


def loss(y, t, base=None, alpha=1.0):
    """(ssim, B, L), each per image [n]."""
    y, t = MR._batch(y), MR._batch(t)
    alpha = 1.0 if base is None else float(alpha)
    ssim = MR.ssim(y, t)
    b = base_term(base, y, t)
    return ssim, b, alpha * (1.0 - ssim) + (1.0 - alpha) * b


def loss_grad(y, t, base=None, alpha=1.0, grad_frames=None):
    """(ssim, B, L, dy): dy [n,h,w,3] = d(sum_i L_i / grad_frames)/dy."""
    y, t = MR._batch(y), MR._batch(t)
    n, h, w, _ = y.shape
    alpha = 1.0 if base is None else float(alpha)
    frames = float(n if grad_frames is None else grad_frames)
    s, pa, pb, pc = coefficients(y, t)
    ssim = s.mean(axis=(1, 2, 3))
    b = base_term(base, y, t)
    dy = -alpha / (frames * 3 * (h - 10) * (w - 10)) * (adjoint(pa, h, w) + y * adjoint(pb, h, w)
                                                       + t * adjoint(pc, h, w))
    if base is not None:
        d = y - t
        dy = dy + (1.0 - alpha) / (frames * h * w * 3) * (np.sign(d) if base == "mae" else 2.0 * d)
    return ssim, b, alpha * (1.0 - ssim) + (1.0 - alpha) * b, dy


def oracle_loss(base, alpha):
    """UNetRef's ``mse(yhat, t)`` for this loss: the batch mean of L_i."""
    return lambda y, t: float(loss(y, t, base, alpha)[2].mean())


def oracle_grad_z(base, alpha):
    """UNetRef's ``mse_grad_z(yhat, t)``: dy * y(1-y), in the dtype of y."""
    def f(y, t):
        dy = loss_grad(y, t, base, alpha)[3]
        y64 = np.asarray(y, np.float64)
        return (dy * y64 * (1.0 - y64)).astype(np.asarray(y).dtype)
    return f


def patch_oracle(monkeypatch, R, base, alpha):
    """Point oracle.unet_ref's loss at this DSSIM loss, as ref_objectives.patch_oracle does."""
    monkeypatch.setattr(R, "mse", oracle_loss(base, alpha))
    monkeypatch.setattr(R, "mse_grad_z", oracle_grad_z(base, alpha))


def flat_pair(shape=(1, 45, 84), seed=5):
    """A nearly flat pair: target constant 128/255, prediction = target + N(0, 1e-3); fp32."""
    n, h, w = shape
    t = np.full((n, h, w, 3), 128.0 / 255.0)
    p = t + np.random.default_rng(seed).normal(0.0, 1e-3, t.shape)
    return p.astype(np.float32), t.astype(np.float32)
