"""Training losses that are not a per-element term of the head kernel.

DSSIM: the structural-dissimilarity loss, alone or mixed with L1 / L2 (Zhao et al. 2017,
"Loss Functions for Image Restoration with Neural Networks"), per image

    L = alpha * (1 - SSIM(y, t)) + (1 - alpha) * B,   B = mean |y-t| ('mae') or mean (y-t)^2 ('mse')

with the SSIM of ``metrics.ssim`` (max_val 1).  Loss and gradient are cnnitmo_dssim_loss_grad;
the head takes the gradient through cnnitmo_head_fwd_bwd_given (engine.HeadStage).

MSSSIM: the same mix with the multi-scale SSIM of ``metrics.ms_ssim`` (tf.image.ssim_multiscale)
in SSIM's place, the form Zhao et al. found to train better than single-scale SSIM: it also sees
errors wider than the 11-pixel window.  Loss and gradient are cnnitmo_msssim_loss_grad.
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


class MSSSIM:
    """compile(loss=MSSSIM(base='mae' | 'mse' | None, alpha=0.84, power_factors=None)): alpha
    (1 - MS-SSIM) + (1 - alpha) base term.  Without a base the loss is 1 - MS-SSIM and alpha is 1.
    power_factors: the weights of 1..5 scales, used as given; None: TensorFlow's five.  The
    coarsest scale must hold the 11 x 11 window: frames of at least ``min_side`` pixels a side
    (161 for five scales)."""

    class_name = "MSSSIM"

    def __init__(self, base=None, alpha=0.84, power_factors=None):
        if base not in L.DSSIM_BASES:
            raise ValueError(f"MSSSIM base {base!r} (one of 'mae', 'mse', None)")
        alpha = 1.0 if base is None else float(alpha)
        if not 0.0 <= alpha <= 1.0:  # (NaN fails both)
            raise ValueError(f"MSSSIM alpha {alpha!r} outside [0, 1]")
        self.base, self.alpha = base, alpha
        self.power_factors = check_power_factors(power_factors)

    @property
    def base_id(self):
        return L.DSSIM_BASES[self.base]

    @property
    def min_side(self):
        return min_side(len(self.power_factors))

    def get_config(self):
        return {"base": self.base, "alpha": self.alpha, "power_factors": list(self.power_factors)}

    def _key(self):
        return self.base, self.alpha, self.power_factors

    def __eq__(self, other):
        return isinstance(other, MSSSIM) and self._key() == other._key()

    def __hash__(self):
        return hash((self.class_name,) + self._key())

    def __repr__(self):
        return f"MSSSIM(base={self.base!r}, alpha={self.alpha!r}, power_factors={self.power_factors!r})"


MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)  # tf.image.ssim_multiscale's power_factors


def min_side(scales):
    """The smallest height or width whose coarsest of ``scales`` levels (each ceil(side / 2) of the
    one before) still holds the 11 x 11 window: 11, 21, 41, 81, 161."""
    return 10 * 2 ** (scales - 1) + 1


def check_power_factors(power_factors):
    """The weights of an MS-SSIM as a tuple of 1..5 finite floats >= 0 (None: TensorFlow's five)."""
    if power_factors is None:
        return MSSSIM_WEIGHTS
    try:
        w = tuple(float(v) for v in power_factors)
    except TypeError:
        raise ValueError(f"ms_ssim power_factors {power_factors!r}: a sequence of 1..5 weights") from None
    if not 1 <= len(w) <= 5 or not all(0.0 <= v < float("inf") for v in w):  # (NaN fails)
        raise ValueError(f"ms_ssim power_factors {power_factors!r}: 1..5 finite weights >= 0")
    return w


def get(loss):
    """The forms of a structural loss -> its object: a DSSIM or an MSSSIM, 'dssim', 'ms_ssim' /
    'msssim' (1 - MS-SSIM), or serialize()'s dict; else None."""
    if isinstance(loss, (DSSIM, MSSSIM)):
        return loss
    if isinstance(loss, str) and loss in ("dssim", "DSSIM"):
        return DSSIM()
    if isinstance(loss, str) and loss in ("ms_ssim", "msssim"):
        return MSSSIM()
    if isinstance(loss, dict) and loss.get("class_name") == DSSIM.class_name:
        return DSSIM(**loss.get("config", {}))
    if isinstance(loss, dict) and loss.get("class_name") == MSSSIM.class_name:
        return MSSSIM(**loss.get("config", {}))
    return None


def serialize(loss):
    """Model.loss as the saved training config holds it: the canonical name of a pointwise
    loss, {'class_name': 'DSSIM' | 'MSSSIM', 'config': {...}} for a DSSIM or an MSSSIM (json keeps
    alpha and the weights exactly)."""
    if isinstance(loss, (DSSIM, MSSSIM)):
        return {"class_name": loss.class_name, "config": loss.get_config()}
    return loss
