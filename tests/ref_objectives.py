"""Numpy reference of the selectable training losses and optimizers (Keras 2.2 definitions).

Losses are written in terms of the head's output y = sigmoid(z) and the target t, as
oracle.unet_ref's ``mse(yhat, t)`` / ``mse_grad_z(yhat, t)`` are, and keep the dtype of their
arguments (fp64 for references, float32 for the oracle's precision-floor runs).  ``term`` is
the per-element loss, ``dterm_dz`` its derivative with respect to the logit z; ``loss`` is the
mean and ``grad_z`` its gradient (the 1/size of the mean included), the two functions
UNetRef.backward looks up as ``mse`` and ``mse_grad_z``.
"""
import numpy as np

LOSSES = ("mse", "mae", "logcosh", "msle", "binary_crossentropy")
LOSS_IDS = {k: i for i, k in enumerate(LOSSES)}  # CNNITMO_LOSS_*
EPS = 1e-7  # Keras' epsilon (msle's clip, binary_crossentropy's probability clip)
LN2 = float(np.log(2.0))


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def term(name, y, t):
    if name == "mse":
        return (y - t) ** 2
    if name == "mae":
        return np.abs(y - t)
    if name == "logcosh":  # Keras: x + softplus(-2x) - ln 2
        a = np.abs(y - t)
        return a + np.log1p(np.exp(-2.0 * a)) - LN2
    if name == "msle":
        return (np.log(np.maximum(y, EPS) + 1.0) - np.log(np.maximum(t, EPS) + 1.0)) ** 2
    if name == "binary_crossentropy":  # on the unclipped y (the kernel works on the logit)
        return -(t * np.log(y) + (1.0 - t) * np.log1p(-y))
    raise KeyError(name)


def dterm_dz(name, y, t):
    s = y * (1.0 - y)  # dy/dz
    if name == "mse":
        return 2.0 * (y - t) * s
    if name == "mae":
        return np.sign(y - t) * s
    if name == "logcosh":
        return np.tanh(y - t) * s
    if name == "msle":
        a = np.log(np.maximum(y, EPS) + 1.0) - np.log(np.maximum(t, EPS) + 1.0)
        return np.where(y >= EPS, 2.0 * a / (y + 1.0) * s, 0.0 * s)
    if name == "binary_crossentropy":
        return y - t
    raise KeyError(name)


def loss(name, y, t):
    return float(np.mean(term(name, y, t)))


def grad_z(name, y, t):
    return dterm_dz(name, y, t) / y.size


def bce_logit(z, t):
    """The kernel's form of binary_crossentropy, from the logit."""
    return np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z)))


def bce_keras(z, t):
    """Keras 2.2 (TF backend): clip y to [eps, 1-eps], back to a logit, then the same formula."""
    y = np.clip(sigmoid(z), EPS, 1.0 - EPS)
    return bce_logit(np.log(y / (1.0 - y)), t)


def patch_oracle(monkeypatch, R, name):
    """Point oracle.unet_ref's loss at `name` (UNetRef.backward looks both up at call time)."""
    monkeypatch.setattr(R, "mse", lambda y, t: loss(name, y, t))
    monkeypatch.setattr(R, "mse_grad_z", lambda y, t: grad_z(name, y, t))


def mae_safe_target(y_ref, t, margin=1e-3):
    """MAE's sign(y - t) is discontinuous: move every target closer than `margin` to the
    reference prediction to y_ref +- 2*margin (inside [0, 1]), so that no implementation
    within `margin` of the reference can land on the other side.  Returns float32-exact
    values (what the device receives)."""
    t = np.asarray(t, np.float64).copy()
    near = np.abs(y_ref - t) < margin
    up = y_ref + 2 * margin
    t[near] = np.where(up <= 1.0, up, y_ref - 2 * margin)[near]
    t = np.clip(t, 0.0, 1.0).astype(np.float32).astype(np.float64)
    assert float(np.abs(y_ref - t).min()) >= margin
    return t


# ---- optimizers: one update in the dtype of the arguments -------------------------------
def lr_at(lr, decay, iterations):
    return lr / (1.0 + decay * iterations)


def rmsprop(p, g, a, iterations=0, lr=1e-3, rho=0.9, eps=1e-7, decay=0.0):
    a = rho * a + (1.0 - rho) * g * g
    return p - lr_at(lr, decay, iterations) * g / (np.sqrt(a) + eps), a


def adam(p, g, m, v, iterations, lr=1e-3, beta_1=0.9, beta_2=0.999, eps=1e-7, decay=0.0):
    t = iterations + 1
    lr_t = lr_at(lr, decay, iterations) * np.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t)
    m = beta_1 * m + (1.0 - beta_1) * g
    v = beta_2 * v + (1.0 - beta_2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def sgd(p, g, mom, iterations=0, lr=1e-2, momentum=0.0, nesterov=False, decay=0.0):
    lr = lr_at(lr, decay, iterations)
    mom = momentum * mom - lr * g
    return (p + momentum * mom - lr * g if nesterov else p + mom), mom
