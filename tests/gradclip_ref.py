"""numpy restatement of cnnitmo_grad_sumsq / cnnitmo_grad_clip (include/cnn_itmo.h), the reference of
tests/test_gpu_gradclip.py; pinned on hand-worked vectors by tests/test_training_controls.py."""
import math

import numpy as np


def sumsq(g):
    """sum g[i]^2 of fp32 values in fp64: every square is exact, math.fsum adds them without error,
    so this is the real sum rounded once."""
    g = np.asarray(g, np.float32).reshape(-1)
    chunks = (g[i:i + (1 << 20)].astype(np.float64) for i in range(0, g.size, 1 << 20))
    return math.fsum(x for c in chunks for x in (c * c).tolist())


def clip(g, S, grad_scale=1.0, clipnorm=0.0, clipvalue=0.0):
    """The fp32 vector cnnitmo_grad_clip leaves in g, given S = sum g^2 (a float; inf / NaN allowed)."""
    g = np.asarray(g, np.float32)
    f = np.float64(1.0)
    if clipnorm and clipnorm > 0:
        S = np.float64(S)
        N = np.float64(grad_scale) * np.sqrt(S)
        if np.isfinite(S) and N >= clipnorm:
            f = np.float64(clipnorm) / N
    with np.errstate(invalid="ignore", over="ignore"):
        v = (g.astype(np.float64) * f).astype(np.float32)
    if clipvalue and clipvalue > 0:
        b = np.float32(np.float64(clipvalue) / np.float64(grad_scale))
        v = np.where(v < -b, -b, np.where(v > b, b, v)).astype(np.float32)  # comparisons: a NaN stays
    return v
