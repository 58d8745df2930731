"""keras.optimizers RMSprop / Adam / SGD (Keras 2.2 arithmetic) over the engine's flat buffers.

An optimizer holds hyper-parameters only.  Its state lives in the engine: ``slots`` flat
fp32 buffers shaped like the parameters (RMSprop: the accumulators; SGD: the moments;
Adam: m and v) and ``iterations``, the number of updates applied so far.  ``decay`` is the
host's: every update runs with lr / (1 + decay * iterations), as Keras does.
"""
from __future__ import annotations

import inspect
import math


class Optimizer:
    class_name = None
    slots = 1  # flat state buffers the update kernel reads and writes

    def _base(self, lr, decay, kwargs):
        lr = kwargs.pop("learning_rate", lr)
        if kwargs:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {sorted(kwargs)}")
        self.lr = float(lr)
        self.decay = float(decay)
        if self.decay < 0:
            raise ValueError("decay must not be negative")

    def lr_at(self, iterations):
        """The learning rate of update number `iterations` (0-based), in double."""
        return self.lr / (1.0 + self.decay * iterations)


class RMSprop(Optimizer):
    """keras.optimizers.RMSprop(lr=0.001, rho=0.9, epsilon=None->1e-7, decay=0)."""
    class_name = "RMSprop"

    def __init__(self, lr=0.001, rho=0.9, epsilon=None, decay=0.0, **kwargs):
        self._base(lr, decay, kwargs)
        self.rho = float(rho)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)

    def get_config(self):
        return {"lr": self.lr, "rho": self.rho, "decay": self.decay, "epsilon": self.epsilon}

    def apply(self, params, grads, slots, iterations, grad_scale=1.0):
        from . import ops
        ops.rmsprop(params, grads, slots[0], self.lr_at(iterations), self.rho, self.epsilon, grad_scale)


class Adam(Optimizer):
    """keras.optimizers.Adam(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None->1e-7, decay=0,
    amsgrad=False); amsgrad is not on the path."""
    class_name = "Adam"
    slots = 2

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False, **kwargs):
        if amsgrad:
            raise NotImplementedError("Adam(amsgrad=True) is not on the path")
        self._base(lr, decay, kwargs)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = 1e-7 if epsilon is None else float(epsilon)
        self.amsgrad = False

    def get_config(self):
        return {"lr": self.lr, "beta_1": self.beta_1, "beta_2": self.beta_2, "decay": self.decay,
                "epsilon": self.epsilon, "amsgrad": False}

    def lr_t(self, iterations):
        """Keras' bias-corrected rate lr * sqrt(1 - beta_2^t) / (1 - beta_1^t), t = iterations + 1."""
        t = iterations + 1
        return self.lr_at(iterations) * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def apply(self, params, grads, slots, iterations, grad_scale=1.0):
        from . import ops
        ops.adam(params, grads, slots[0], slots[1], self.lr_t(iterations), self.beta_1, self.beta_2, self.epsilon,
                 grad_scale)


class SGD(Optimizer):
    """keras.optimizers.SGD(lr=0.01, momentum=0, decay=0, nesterov=False)."""
    class_name = "SGD"

    def __init__(self, lr=0.01, momentum=0.0, decay=0.0, nesterov=False, **kwargs):
        self._base(lr, decay, kwargs)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)

    def get_config(self):
        return {"lr": self.lr, "momentum": self.momentum, "decay": self.decay, "nesterov": self.nesterov}

    def apply(self, params, grads, slots, iterations, grad_scale=1.0):
        from . import ops
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
