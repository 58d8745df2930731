"""Training losses that are not a per-element term of the head kernel.

DSSIM: the structural-dissimilarity loss, alone or mixed with L1 / L2 (Zhao et al. 2017,
"Loss Functions for Image Restoration with Neural Networks"), per image

    L = alpha * (1 - SSIM(y, t)) + (1 - alpha) * B,   B = mean |y-t| ('mae') or mean (y-t)^2 ('mse')

with the SSIM of ``metrics.ssim`` (max_val 1).  Loss and gradient are cnnitmo_dssim_loss_grad;
the head takes the gradient through cnnitmo_head_fwd_bwd_given (engine.HeadStage).

MSSSIM: the same mix with the multi-scale SSIM of ``metrics.ms_ssim`` (tf.image.ssim_multiscale)
in SSIM's place, the form Zhao et al. found to train better than single-scale SSIM: it also sees
errors wider than the 11-pixel window.  Loss and gradient are cnnitmo_msssim_loss_grad.

HighlightWeighted: the pointwise L2 / L1 loss with every pixel weighted by 1 + gain * a, a the soft
saturation mask of Eilertsen et al. 2017 ("HDR image reconstruction from a single exposure using
deep CNNs"), a = clip((max_c s - threshold) / (1 - threshold), 0, 1), taken from the network's
input frame or from the target: the clipped pixels are the ones an inverse tone-mapping network
has to invent, and a few percent of a frame.  Loss and gradient are cnnitmo_highlight_loss_grad;
``highlight_weighted`` is the functional form, for reporting the error inside the highlights.
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


class HighlightWeighted:
    """compile(loss=HighlightWeighted(base='mse' | 'mae', threshold=0.95, gain=1.0, source='input' |
    'target')): per image the mean over pixels and channels of (1 + gain * a) * l, l = (y-t)^2 or
    |y-t|, a = clip((max_c s - threshold) / (1 - threshold), 0, 1).  source 'input': s is the
    network's input frame (where the camera clipped); 'target': s is the target (its bright
    regions).  The sum is divided by the element count, not by the sum of the weights: gain 0 is
    the base loss and unsaturated pixels keep the gradient they have under it.  threshold 0.95 is
    HDRCNN's tau; gain 1.0 is a starting point, not a tuned value."""

    class_name = "HighlightWeighted"

    def __init__(self, base="mse", threshold=0.95, gain=1.0, source="input"):
        if base not in ("mse", "mae"):
            raise ValueError(f"HighlightWeighted base {base!r} (one of 'mse', 'mae')")
        if source not in ("input", "target"):
            raise ValueError(f"HighlightWeighted source {source!r} (one of 'input', 'target')")
        try:
            threshold, gain = float(threshold), float(gain)
        except (TypeError, ValueError):
            raise ValueError(f"HighlightWeighted threshold {threshold!r}, gain {gain!r}: two numbers") from None
        if not 0.0 <= threshold < 1.0:  # (NaN fails both)
            raise ValueError(f"HighlightWeighted threshold {threshold!r} outside [0, 1)")
        if not 0.0 <= gain < float("inf"):
            raise ValueError(f"HighlightWeighted gain {gain!r} negative or not finite")
        self.base, self.threshold, self.gain, self.source = base, threshold, gain, source

    @property
    def base_id(self):
        return L.DSSIM_BASES[self.base]

    def get_config(self):
        return {"base": self.base, "threshold": self.threshold, "gain": self.gain, "source": self.source}

    def _key(self):
        return self.base, self.threshold, self.gain, self.source

    def __eq__(self, other):
        return isinstance(other, HighlightWeighted) and self._key() == other._key()

    def __hash__(self):
        return hash((self.class_name,) + self._key())

    def __repr__(self):
        return (f"HighlightWeighted(base={self.base!r}, threshold={self.threshold!r}, gain={self.gain!r}, "
                f"source={self.source!r})")


def highlight_weighted(x, y, t, base="mse", threshold=0.95, gain=1.0, source="input"):
    """The highlight-weighted loss of predictions y against targets t for the input frames x, per
    image: a float64 [n, 4] CUDA tensor {A, B, L, H} = the mean mask (the saturated share), the
    unweighted base term, the loss HighlightWeighted(base, threshold, gain, source) trains for and
    the base error inside the highlights (sum a l / (3 sum a), 0 without a masked pixel).  x, y, t:
    numpy arrays or CUDA tensors, [h,w,3] or [n,h,w,3]; with source 'target' x is not read (None
    will do).  Nothing synchronises with the host."""
    import torch
    from . import ops
    from .tonemap import _dev
    hw = HighlightWeighted(base, threshold, gain, source)
    y, t = _dev(y, torch.float32), _dev(t, torch.float32)
    s = t if source == "target" else _dev(x, torch.float32)
    if not y.shape == t.shape == s.shape:
        raise ValueError(f"image batches differ in shape: {tuple(s.shape)}, {tuple(y.shape)}, {tuple(t.shape)}")
    return ops.highlight_loss_grad(hw.base_id, hw.threshold, hw.gain, s, y, t)


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
    """The forms of a loss of this module -> its object: a DSSIM, an MSSSIM or a HighlightWeighted,
    'dssim', 'ms_ssim' / 'msssim' (1 - MS-SSIM), or serialize()'s dict; else None."""
    if isinstance(loss, (DSSIM, MSSSIM, HighlightWeighted)):
        return loss
    if isinstance(loss, str) and loss in ("dssim", "DSSIM"):
        return DSSIM()
    if isinstance(loss, str) and loss in ("ms_ssim", "msssim"):
        return MSSSIM()
    if isinstance(loss, dict) and loss.get("class_name") == DSSIM.class_name:
        return DSSIM(**loss.get("config", {}))
    if isinstance(loss, dict) and loss.get("class_name") == MSSSIM.class_name:
        return MSSSIM(**loss.get("config", {}))
    if isinstance(loss, dict) and loss.get("class_name") == HighlightWeighted.class_name:
        return HighlightWeighted(**loss.get("config", {}))
    return None


def serialize(loss):
    """Model.loss as the saved training config holds it: the canonical name of a pointwise
    loss, {'class_name': 'DSSIM' | 'MSSSIM' | 'HighlightWeighted', 'config': {...}} for an object of
    this module (json keeps alpha, the weights, threshold and gain exactly)."""
    if isinstance(loss, (DSSIM, MSSSIM, HighlightWeighted)):
        return {"class_name": loss.class_name, "config": loss.get_config()}
    return loss
