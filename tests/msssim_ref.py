"""numpy float64 reference of multi-scale SSIM as a metric and as a training loss with its
gradient (csrc/msssim.hip), after tf.image.ssim_multiscale.

Per image of a prediction y and a target t, [n,h,w,3], M = len(power_factors) <= 5:

    level 0 = the image (fp64 from the fp32 inputs); level k+1 = the 2x2 mean of level k, an odd
        side first extended by a copy of its last row / column (SYMMETRIC pad 1, avg_pool VALID)
    cs = (2 cov + C2)/(vy + vt + C2),  l = (2 my mt + C1)/(my^2 + mt^2 + C1)  (metrics_ref's window)
    F[k][c] = mean_q cs for k < M-1,  F[M-1][c] = mean_q l cs
    MS_c = prod_k max(F[k][c], 0)^w_k,   MS-SSIM = (MS_0 + MS_1 + MS_2)/3
    L = alpha (1 - MS-SSIM) + (1 - alpha) B,  B = dssim_ref.base_term

The weights are used as given (TF's defaults do not sum to 1 over fewer scales).  Gradient:
dMS/dy = 1/3 sum_c MS_c sum_k (w_k/F[k][c]) dF[k][c]/dy, exactly 0 for a channel with any factor
<= 0; dF/dy_k is dssim_ref's (Fa + y_k Fb + t_k Fc)/n_pos_k, with the planes of S at the last level
and of cs (A1 = B1 = 1) below it; the level gradients go through the adjoint of pad + pool
(``pool_adjoint``).  tests/test_msssim_host.py checks dy against central differences.
"""
import numpy as np

import dssim_ref as DR
import metrics_ref as MR

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)  # tf.image.ssim_multiscale's power_factors


def min_side(scales):
    return 10 * 2 ** (scales - 1) + 1


def pool(x):
    """[n,h,w,c] -> [n,ceil(h/2),ceil(w/2),c]: an odd side repeats its last row / column."""
    n, h, w, c = x.shape
    if h % 2:
        x = np.concatenate([x, x[:, -1:]], 1)
    if w % 2:
        x = np.concatenate([x, x[:, :, -1:]], 2)
    return 0.25 * ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2]))


def pool_adjoint(g, h, w):
    """The adjoint of ``pool`` on an [n,h,w,c] level: every source takes a quarter of its parent;
    a pad copy folds onto the last real row / column."""
    n, h2, w2, c = g.shape
    out = np.zeros((n, 2 * h2, 2 * w2, c))
    for i in (0, 1):
        for j in (0, 1):
            out[:, i::2, j::2] = 0.25 * g
    if h % 2:
        out[:, h - 1] += out[:, h]
    if w % 2:
        out[:, :, w - 1] += out[:, :, w]
    return out[:, :h, :w]


def levels(x, scales):
    out = [MR._batch(x)]
    for _ in range(scales - 1):
        out.append(pool(out[-1]))
    return out


def _weights(power_factors):
    w = WEIGHTS if power_factors is None else tuple(float(v) for v in power_factors)
    if not 1 <= len(w) <= 5:
        raise ValueError(f"{len(w)} power factors")
    return w


def _check(y, scales):
    h, w = y.shape[1:3]
    if min(h, w) < min_side(scales):
        raise ValueError(f"ms_ssim with {scales} scales needs at least {min_side(scales)} pixels a side, got {h} x {w}")


def coefficients(y, t, last, max_val=1.0):
    """(term, Pa, Pb, Pc) of one level, each [n, h-10, w-10, 3]: the term is S = l cs at the last
    level and cs below it."""
    g = MR.taps()
    f = MR._filter_valid
    c1, c2 = (MR.K1 * max_val) ** 2, (MR.K2 * max_val) ** 2
    my, mt = f(y, g), f(t, g)
    vy = f(y * y, g) - my * my
    vt = f(t * t, g) - mt * mt
    cov = f(y * t, g) - my * mt
    a2, b2 = 2 * cov + c2, vy + vt + c2
    if not last:
        cs = a2 / b2
        pc = 2.0 / b2
        pb = -2 * cs / b2
        return cs, -mt * pc - my * pb, pb, pc
    a1, b1 = 2 * my * mt + c1, my * my + mt * mt + c1
    s = (a1 * a2) / (b1 * b2)
    pc = 2 * a1 / (b1 * b2)
    pb = -2 * s / b2
    pa = 2 * mt * a2 / (b1 * b2) - 2 * my * s / b1 - mt * pc - my * pb
    return s, pa, pb, pc


def factors(y, t, power_factors=None, max_val=1.0):
    """F [n, M, 3]."""
    m = len(_weights(power_factors))
    y, t = MR._batch(y), MR._batch(t)
    _check(y, m)
    ly, lt = levels(y, m), levels(t, m)
    return np.stack([coefficients(ly[k], lt[k], k == m - 1, max_val)[0].mean(axis=(1, 2)) for k in range(m)], 1)


def _score(f, w):
    """MS_c [n, 3] from F [n, M, 3]."""
    return np.prod(np.maximum(f, 0.0) ** np.asarray(w)[None, :, None], axis=1)


def ms_ssim(y, t, max_val=1.0, power_factors=None):
    """MS-SSIM per image [n]."""
    return _score(factors(y, t, power_factors, max_val), _weights(power_factors)).mean(axis=1)


def loss(y, t, base=None, alpha=1.0, power_factors=None, max_val=1.0):
    """(ms_ssim, B, L), each per image [n]."""
    y, t = MR._batch(y), MR._batch(t)
    alpha = 1.0 if base is None else float(alpha)
    ms = ms_ssim(y, t, max_val, power_factors)
    b = DR.base_term(base, y, t)
    return ms, b, alpha * (1.0 - ms) + (1.0 - alpha) * b


def loss_grad(y, t, base=None, alpha=1.0, power_factors=None, grad_frames=None):
    """(ms_ssim, B, L, F, dy): F [n,M,3], dy [n,h,w,3] = d(sum_i L_i / grad_frames)/dy (max_val 1)."""
    w = _weights(power_factors)
    m = len(w)
    y, t = MR._batch(y), MR._batch(t)
    _check(y, m)
    n = y.shape[0]
    alpha = 1.0 if base is None else float(alpha)
    frames = float(n if grad_frames is None else grad_frames)
    ly, lt = levels(y, m), levels(t, m)
    co = [coefficients(ly[k], lt[k], k == m - 1) for k in range(m)]
    f = np.stack([c[0].mean(axis=(1, 2)) for c in co], 1)
    msc = _score(f, w)
    live = (f > 0).all(axis=1)  # [n, 3]
    ms = msc.mean(axis=1)
    g = None  # d(sum_i ms_i)/d level, coarse to fine
    for k in range(m - 1, -1, -1):
        _, pa, pb, pc = co[k]
        hk, wk = ly[k].shape[1:3]
        with np.errstate(divide="ignore", invalid="ignore"):
            sc = np.where(live, msc * w[k] / f[:, k], 0.0) / (3.0 * (hk - 10) * (wk - 10))
        own = sc[:, None, None, :] * (DR.adjoint(pa, hk, wk) + ly[k] * DR.adjoint(pb, hk, wk)
                                      + lt[k] * DR.adjoint(pc, hk, wk))
        own = np.where(live[:, None, None, :], own, 0.0)
        g = own if g is None else own + pool_adjoint(g, hk, wk)
    b = DR.base_term(base, y, t)
    dy = -alpha / frames * g
    if base is not None:
        d = y - t
        dy = dy + (1.0 - alpha) / (frames * d[0].size) * (np.sign(d) if base == "mae" else 2.0 * d)
    return ms, b, alpha * (1.0 - ms) + (1.0 - alpha) * b, f, dy


def oracle_loss(base, alpha, power_factors=None):
    """UNetRef's ``mse(yhat, t)`` for this loss: the batch mean of L_i."""
    return lambda y, t: float(loss(y, t, base, alpha, power_factors)[2].mean())


def oracle_grad_z(base, alpha, power_factors=None):
    """UNetRef's ``mse_grad_z(yhat, t)``: dy * y(1-y), in the dtype of y."""
    def f(y, t):
        dy = loss_grad(y, t, base, alpha, power_factors)[4]
        y64 = np.asarray(y, np.float64)
        return (dy * y64 * (1.0 - y64)).astype(np.asarray(y).dtype)
    return f


def patch_oracle(monkeypatch, R, base, alpha, power_factors=None):
    """Point oracle.unet_ref's loss at this loss, as dssim_ref.patch_oracle does."""
    monkeypatch.setattr(R, "mse", oracle_loss(base, alpha, power_factors))
    monkeypatch.setattr(R, "mse_grad_z", oracle_grad_z(base, alpha, power_factors))


def blocky_pair(shape, seed, sigma):
    """The GPU tests' images: target = 8 x 8 blocks of uniform noise * 0.8 + 0.1 fine uniform noise,
    prediction = clip(target + N(0, sigma)); fp32 [n,h,w,3].  Structure at every scale, so no
    factor is near the clamp.  ``sigma`` may be one level or one per image."""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    blocks = rng.uniform(size=(n, (h + 7) // 8, (w + 7) // 8, 3))
    t = 0.8 * np.repeat(np.repeat(blocks, 8, 1), 8, 2)[:, :h, :w] + 0.1 * rng.uniform(size=(n, h, w, 3))
    lv = np.broadcast_to(np.asarray(sigma, np.float64), (n,)).reshape(n, 1, 1, 1)
    p = np.clip(t + rng.normal(0.0, 1.0, t.shape) * lv, 0.0, 1.0)
    return p.astype(np.float32), t.astype(np.float32)
