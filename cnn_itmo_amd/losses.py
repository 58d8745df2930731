"""Training losses that are not a per-element term of the head kernel.

DSSIM: the structural-dissimilarity loss, alone or mixed with L1 / L2 (Zhao et al. 2017,
"Loss Functions for Image Restoration with Neural Networks"), per image

    L = alpha * (1 - SSIM(y, t)) + (1 - alpha) * B,   B = mean |y-t| ('mae') or mean (y-t)^2 ('mse')

with the SSIM of ``metrics.ssim`` (max_val 1).  Loss and gradient are cnnitmo_dssim_loss_grad;
the head takes the gradient through cnnitmo_head_fwd_bwd_given (engine.HeadStage).
"""
from __future__ import annotations

from . import _lib as L


class DSSIM:
    """compile(loss=DSSIM(base='mae' | 'mse' | None, alpha=0.84)).  Without a base the loss is
    1 - SSIM and alpha is 1."""

    class_name = "DSSIM"

    def __init__(self, base=None, alpha=0.84):
        if base not in L.DSSIM_BASES:
            raise ValueError(f"DSSIM base {base!r} (one of 'mae', 'mse', None)")
        alpha = 1.0 if base is None else float(alpha)
        if not 0.0 <= alpha <= 1.0:  # (NaN fails both)
            raise ValueError(f"DSSIM alpha {alpha!r} outside [0, 1]")
        self.base, self.alpha = base, alpha

    @property
    def base_id(self):
        return L.DSSIM_BASES[self.base]

    def get_config(self):
        return {"base": self.base, "alpha": self.alpha}

    def __eq__(self, other):
        return isinstance(other, DSSIM) and (self.base, self.alpha) == (other.base, other.alpha)

    def __hash__(self):
        return hash((self.class_name, self.base, self.alpha))

    def __repr__(self):
        return f"DSSIM(base={self.base!r}, alpha={self.alpha!r})"


def get(loss):
    """compile()'s DSSIM forms -> a DSSIM: 'dssim', a DSSIM, or serialize()'s dict; else None."""
    if isinstance(loss, DSSIM):
        return loss
    if isinstance(loss, str) and loss in ("dssim", "DSSIM"):
        return DSSIM()
    if isinstance(loss, dict) and loss.get("class_name") == DSSIM.class_name:
        return DSSIM(**loss.get("config", {}))
    return None


def serialize(loss):
    """Model.loss as the saved training config holds it: the canonical name of a pointwise
    loss, {'class_name': 'DSSIM', 'config': {...}} for a DSSIM (json keeps alpha exactly)."""
    if isinstance(loss, DSSIM):
        return {"class_name": loss.class_name, "config": loss.get_config()}
    return loss
