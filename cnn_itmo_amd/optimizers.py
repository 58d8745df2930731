"""keras.optimizers RMSprop / Adam / SGD (Keras 2.2 arithmetic) over the engine's flat buffers.

An optimizer holds hyper-parameters only.  Its state lives in the engine: ``slots`` flat
fp32 buffers shaped like the parameters (RMSprop: the accumulators; SGD: the moments;
Adam: m and v) and ``iterations``, the number of updates applied so far.  ``decay`` is the
host's: every update runs with lr / (1 + decay * iterations), as Keras does.

``clipnorm`` / ``clipvalue`` (Keras 2.2 ``get_gradients``): the gradient is scaled down to the
global norm ``clipnorm`` over all tensors, then clamped to +-``clipvalue``, on the device, in
the flat gradient buffer, before the update kernel reads it (``Optimizer._clip``).
"""
from __future__ import annotations

import inspect
import math


class Optimizer:
    class_name = None
    slots = 1  # flat state buffers the update kernel reads and writes

    def _base(self, lr, decay, kwargs, clipnorm=None, clipvalue=None):
        lr = kwargs.pop("learning_rate", lr)
        if kwargs:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {sorted(kwargs)}")
        self.lr = float(lr)
        self.decay = float(decay)
        if self.decay < 0:
            raise ValueError("decay must not be negative")
        # keras.optimizers.Optimizer: both optional, 0 / None = off, a negative value refused
        for name, v in (("clipnorm", clipnorm), ("clipvalue", clipvalue)):
            if v is not None and not float(v) >= 0:
                raise ValueError(f"Expected {name} >= 0, received: {v}")
            setattr(self, name, float(v) if v else None)

    def _clip_config(self, config):
        """get_config's tail: 'clipnorm' / 'clipvalue' only when set, as Keras writes them."""
        for name in ("clipnorm", "clipvalue"):
            if getattr(self, name) is not None:
                config[name] = getattr(self, name)
        return config

    def _clip(self, grads, grad_scale=1.0):
        """Keras' get_gradients on the flat buffer, in place and without a host round trip: scale
        by clipnorm / ||g'|| when the GLOBAL norm of g' = grads * grad_scale reaches clipnorm,
        then clamp g' to +-clipvalue.  With neither set nothing is launched."""
        if self.clipnorm is None and self.clipvalue is None:
            return
        from . import ops
        sumsq = ops.grad_sumsq(grads) if self.clipnorm is not None else None
        ops.grad_clip(grads, sumsq, grad_scale, self.clipnorm or 0.0, self.clipvalue or 0.0)

    def lr_at(self, iterations):
        """The learning rate of update number `iterations` (0-based), in double."""
        return self.lr / (1.0 + self.decay * iterations)


class RMSprop(Optimizer):
    """keras.optimizers.RMSprop(lr=0.001, rho=0.9, epsilon=None->1e-7, decay=0)."""
    class_name = "RMSprop"

    def __init__(self, lr=0.001, rho=0.9, epsilon=None, decay=0.0, clipnorm=None, clipvalue=None,
                 **kwargs):
        self._base(lr, decay, kwargs, clipnorm, clipvalue)
        self.rho = float(rho)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def get_config(self):
        return self._clip_config({"lr": self.lr, "rho": self.rho, "decay": self.decay, "epsilon": self.epsilon})

    def apply(self, params, grads, slots, iterations, grad_scale=1.0):
        from . import ops
        self._clip(grads, grad_scale)
        ops.rmsprop(params, grads, slots[0], self.lr_at(iterations), self.rho, self.epsilon, grad_scale)


class Adam(Optimizer):
    """keras.optimizers.Adam(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None->1e-7, decay=0,
    amsgrad=False); amsgrad is not on the path."""
    class_name = "Adam"
    slots = 2

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False,
                 clipnorm=None, clipvalue=None, **kwargs):
        if amsgrad:
            raise NotImplementedError("Adam(amsgrad=True) is not on the path")
        self._base(lr, decay, kwargs, clipnorm, clipvalue)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)
        self.amsgrad = False

    def get_config(self):
        return self._clip_config({"lr": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "decay": self.decay,
                                  "epsilon": self.epsilon, "amsgrad": False})

    def lr_t(self, iterations):
        """Keras' bias-corrected rate lr * sqrt(1 - beta_2^t) / (1 - beta_1^t), t = iterations + 1."""
        t = iterations + 1
        return self.lr_at(iterations) * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def apply(self, params, grads, slots, iterations, grad_scale=1.0):
        from . import ops
        self._clip(grads, grad_scale)
        ops.adam(params, grads, slots[0], slots[1], self.lr_t(iterations), self.beta_1, self.beta_2, self.epsilon,
                 grad_scale)


class SGD(Optimizer):
    """keras.optimizers.SGD(lr=0.01, momentum=0, decay=0, nesterov=False)."""
    class_name = "SGD"

    def __init__(self, lr=0.01, momentum=0.0, decay=0.0, nesterov=False, clipnorm=None, clipvalue=None, **kwargs):
        self._base(lr, decay, kwargs, clipnorm, clipvalue)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)

    def get_config(self):
        return self._clip_config({"lr": self.lr, "momentum": self.momentum, "decay": self.decay,
                                  "nesterov": self.nesterov})

    def apply(self, params, grads, slots, iterations, grad_scale=1.0):
        from . import ops
        self._clip(grads, grad_scale)
        ops.sgd(params, grads, slots[0], self.lr_at(iterations), self.momentum, self.nesterov, grad_scale)


CLASSES = {c.class_name: c for c in (RMSprop, Adam, SGD)}
_BY_STRING = {k.lower(): c for k, c in CLASSES.items()}


def from_config(class_name, config):
    """The optimizer of a Keras ``optimizer_config`` ({'class_name', 'config'})."""
    if class_name not in CLASSES:
        raise NotImplementedError(f"optimizer {class_name!r} (one of {sorted(CLASSES)})")
    cls = CLASSES[class_name]
    known = set(inspect.signature(cls.__init__).parameters) | {"learning_rate"}
    # (later Keras versions add keys such as 'name' or 'centered': not on the path, ignored)
    return cls(**{k: v for k, v in (config or {}).items() if k in known})


def get(optimizer):
    """compile()'s optimizer argument: an instance, a Keras name ('rmsprop', 'adam', 'sgd',
    any case) or an {'class_name', 'config'} dict."""
    if isinstance(optimizer, Optimizer):
        return optimizer
    if isinstance(optimizer, str):
        if optimizer.lower() not in _BY_STRING:
            raise NotImplementedError(f"optimizer {optimizer!r} (one of {sorted(_BY_STRING)})")
        return _BY_STRING[optimizer.lower()]()
    if isinstance(optimizer, dict):
        return from_config(optimizer.get("class_name"), optimizer.get("config"))
    raise TypeError(f"optimizer {optimizer!r}")
