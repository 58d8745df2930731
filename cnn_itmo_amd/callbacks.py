"""Minimal keras.callbacks equivalents used by the reference's train loop
(main.py:69,121,123-124): CSVLogger, ModelCheckpoint, LambdaCallback."""
from __future__ import annotations

import csv
import math
import os
import warnings


class Callback:
    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None): pass
    def on_train_end(self, logs=None): pass
    def on_epoch_begin(self, epoch, logs=None): pass
    def on_epoch_end(self, epoch, logs=None): pass
    def on_batch_begin(self, batch, logs=None): pass
    def on_batch_end(self, batch, logs=None): pass


class CallbackList:
    def __init__(self, cbs, model):
        self.cbs = list(cbs)
        for c in self.cbs:
            c.set_model(model)

    def call(self, name, *args):
        for c in self.cbs:
            getattr(c, name)(*args)


def monitor_mode(monitor, mode, who="ModelCheckpoint"):
    """'min' / 'max' for a monitored log key.  'auto' (and, with a warning, an unknown mode) is max
    when the name contains 'acc', 'psnr' or 'ssim' and min otherwise -- this package's rule for
    every monitoring callback (Keras' own 'auto' knows 'acc' only)."""
    if mode not in ("auto", "min", "max"):
        warnings.warn(f"{who} mode {mode!r} is unknown, fallback to auto mode.", RuntimeWarning)
        mode = "auto"
    if mode == "auto":
        mode = "max" if any(s in monitor for s in ("acc", "psnr", "ssim")) else "min"
    return mode


class LambdaCallback(Callback):
    def __init__(self, on_epoch_begin=None, on_epoch_end=None, on_batch_begin=None, on_batch_end=None,
                 on_train_begin=None, on_train_end=None):
        self._f = dict(on_epoch_begin=on_epoch_begin, on_epoch_end=on_epoch_end,
                       on_batch_begin=on_batch_begin, on_batch_end=on_batch_end,
                       on_train_begin=on_train_begin, on_train_end=on_train_end)
        for k, f in self._f.items():
            if f is not None:
                setattr(self, k, f)


class CSVLogger(Callback):
    """CSVLogger('log.csv', append=True, separator=';') -- main.py:121."""

    def __init__(self, filename, separator=",", append=False):
        self.filename, self.sep, self.append = filename, separator, append
        self.keys = None

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        if self.keys is None:
            self.keys = sorted(logs)
        new = not (self.append and os.path.exists(self.filename) and os.path.getsize(self.filename) > 0)
        mode = "a" if self.append else ("w" if epoch == 0 else "a")
        with open(self.filename, mode, newline="") as f:
            w = csv.writer(f, delimiter=self.sep)
            if new and (self.append or epoch == 0):
                w.writerow(["epoch"] + self.keys)
            w.writerow([epoch] + [logs.get(k, "") for k in self.keys])


class ModelCheckpoint(Callback):
    """ModelCheckpoint(filepath) -- main.py:123-124; filepath may use {epoch} and log keys.

    ``save_best_only=True`` saves only when the ``monitor`` log improves on the best so far:
    ``mode`` 'min' / 'max', or 'auto' = max when the monitored name contains 'acc', 'psnr'
    or 'ssim' and min otherwise.  A monitored key missing from the logs skips the save with
    a warning.  The default saves every ``period`` epochs."""

    def __init__(self, filepath, monitor="val_loss", verbose=0, save_best_only=False, mode="auto",
                 save_weights_only=False, period=1):
        self.filepath, self.verbose, self.weights_only, self.period = filepath, verbose, save_weights_only, period
        mode = monitor_mode(monitor, mode)
        self.monitor, self.save_best_only, self.mode = monitor, bool(save_best_only), mode
        self.best = -math.inf if mode == "max" else math.inf

    def _improved(self, value):
        return value > self.best if self.mode == "max" else value < self.best

    def on_epoch_end(self, epoch, logs=None):
        if (epoch + 1) % self.period:
            return
        if self.save_best_only:
            value = (logs or {}).get(self.monitor)
            if value is None:
                warnings.warn(f"Can save best model only with {self.monitor} available, skipping.", RuntimeWarning)
                return
            if not self._improved(value):
                if self.verbose:
                    print(f"Epoch {epoch + 1}: {self.monitor} did not improve from {self.best:.5f}")
                return
            self.best = value
        path = self.filepath.format(epoch=epoch + 1, **(logs or {}))
        (self.model.save_weights if self.weights_only else self.model.save)(path)
        if self.verbose:
            print(f"Epoch {epoch + 1}: saving model to {path}")


def _is_float(v):
    import numpy as np
    return isinstance(v, (float, np.floating))


class LearningRateScheduler(Callback):
    """keras.callbacks.LearningRateScheduler(schedule, verbose=0): before every epoch
    ``optimizer.lr = schedule(epoch, lr)`` (or ``schedule(epoch)`` for a one-parameter schedule);
    the result must be a Python or numpy float.  The epoch logs gain ``lr``."""

    def __init__(self, schedule, verbose=0):
        self.schedule, self.verbose = schedule, verbose

    def on_epoch_begin(self, epoch, logs=None):
        if not hasattr(self.model.optimizer, "lr"):
            raise ValueError('Optimizer must have a "lr" attribute.')
        lr = float(self.model.optimizer.lr)
        try:  # the two-parameter form first, as Keras does
            lr = self.schedule(epoch, lr)
        except TypeError:
            lr = self.schedule(epoch)
        if not _is_float(lr):
            raise ValueError('The output of the "schedule" function should be float.')
        self.model.optimizer.lr = float(lr)
        if self.verbose:
            print(f"\nEpoch {epoch + 1:05d}: LearningRateScheduler setting learning rate to {float(lr)}.")

    def on_epoch_end(self, epoch, logs=None):
        if logs is not None:
            logs["lr"] = float(self.model.optimizer.lr)


class ReduceLROnPlateau(Callback):
    """keras.callbacks.ReduceLROnPlateau (Keras 2.2.4 state machine): after ``patience`` epochs
    without an improvement of more than ``min_delta`` the learning rate becomes
    max(lr * factor, min_lr); ``cooldown`` epochs then pass before epochs are counted again.
    The epoch logs gain ``lr`` (the rate the epoch ran with).  mode 'auto': monitor_mode."""

    def __init__(self, monitor="val_loss", factor=0.1, patience=10, verbose=0, mode="auto", min_delta=1e-4,
                 cooldown=0, min_lr=0, **kwargs):
        if "epsilon" in kwargs:  # Keras' older name
            min_delta = kwargs.pop("epsilon")
        if kwargs:
            raise TypeError(f"ReduceLROnPlateau: unexpected arguments {sorted(kwargs)}")
        if factor >= 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0.")
        self.monitor, self.factor, self.patience, self.verbose = monitor, factor, patience, verbose
        self.min_delta, self.cooldown, self.min_lr = min_delta, cooldown, min_lr
        self.mode = monitor_mode(monitor, mode, "Learning Rate Plateau Reducing")
        self._reset()

    def _reset(self):
        self.best = -math.inf if self.mode == "max" else math.inf
        self.wait = 0
        self.cooldown_counter = 0

    def _improved(self, current):
        return current > self.best + self.min_delta if self.mode == "max" else current < self.best - self.min_delta

    def in_cooldown(self):
        return self.cooldown_counter > 0

    def on_train_begin(self, logs=None):
        self._reset()

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        logs["lr"] = float(self.model.optimizer.lr)
        current = logs.get(self.monitor)
        if current is None:
            warnings.warn(f"Reduce LR on plateau conditioned on metric `{self.monitor}` which is not available. "
                          f"Available metrics are: {','.join(sorted(logs))}", RuntimeWarning)
            return
        if self.in_cooldown():
            self.cooldown_counter -= 1
            self.wait = 0
        if self._improved(current):
            self.best = current
            self.wait = 0
        elif not self.in_cooldown():
            self.wait += 1
            if self.wait >= self.patience:
                old = float(self.model.optimizer.lr)
                if old > self.min_lr:
                    new = max(old * self.factor, self.min_lr)
                    self.model.optimizer.lr = float(new)
                    if self.verbose:
                        print(f"\nEpoch {epoch + 1:05d}: ReduceLROnPlateau reducing learning rate to {new}.")
                    self.cooldown_counter = self.cooldown
                    self.wait = 0


class EarlyStopping(Callback):
    """keras.callbacks.EarlyStopping (Keras 2.2.4): stop once ``patience`` epochs in a row failed
    to better the best value (``baseline`` to begin with) by more than |min_delta|;
    ``restore_best_weights`` puts the weights of the best epoch back.  mode 'auto': monitor_mode."""

    def __init__(self, monitor="val_loss", min_delta=0, patience=0, verbose=0, mode="auto", baseline=None,
                 restore_best_weights=False):
        self.monitor, self.patience, self.verbose, self.baseline = monitor, patience, verbose, baseline
        self.min_delta = abs(min_delta)
        self.restore_best_weights = bool(restore_best_weights)
        self.mode = monitor_mode(monitor, mode, "EarlyStopping")
        self.wait = 0
        self.stopped_epoch = 0
        self.best_weights = None
        self.best = self._start()

    def _start(self):
        if self.baseline is not None:
            return self.baseline
        return -math.inf if self.mode == "max" else math.inf

    def _improved(self, current):
        return current - self.min_delta > self.best if self.mode == "max" else current + self.min_delta < self.best

    def on_train_begin(self, logs=None):
        self.wait = 0
        self.stopped_epoch = 0
        self.best_weights = None
        self.best = self._start()

    def on_epoch_end(self, epoch, logs=None):
        current = (logs or {}).get(self.monitor)
        if current is None:
            warnings.warn(f"Early stopping conditioned on metric `{self.monitor}` which is not available. "
                          f"Available metrics are: {','.join(sorted(logs or {}))}", RuntimeWarning)
            return
        if self._improved(current):
            self.best = current
            self.wait = 0
            if self.restore_best_weights:
                self.best_weights = self.model.get_weights()
            return
        self.wait += 1
        if self.wait >= self.patience:
            self.stopped_epoch = epoch
            self.model.stop_training = True
            if self.restore_best_weights and self.best_weights is not None:  # (None: no epoch beat the baseline)
                if self.verbose:
                    print("Restoring model weights from the end of the best epoch")
                self.model.set_weights(self.best_weights)

    def on_train_end(self, logs=None):
        if self.stopped_epoch > 0 and self.verbose:
            print(f"Epoch {self.stopped_epoch + 1:05d}: early stopping")


class TerminateOnNaN(Callback):
    """keras.callbacks.TerminateOnNaN: stop when a ``loss`` in the logs is NaN or infinite.  Checked
    after every batch as in Keras and also after every epoch: the batch logs here carry no loss
    (it stays on the device until the epoch ends), so the epoch check is the one that fires."""

    def _check(self, where, logs):
        loss = (logs or {}).get("loss")
        if loss is not None and not math.isfinite(loss):
            print(f"{where}: Invalid loss, terminating training")
            self.model.stop_training = True

    def on_batch_end(self, batch, logs=None):
        self._check(f"Batch {batch}", logs)

    def on_epoch_end(self, epoch, logs=None):
        self._check(f"Epoch {epoch + 1}", logs)
