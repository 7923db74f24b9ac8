"""Learning-rate schedule of the reference's trainer for the row-sparse optimizers.

``Trainer._build_scheduler`` (trainer.py:80-89) builds ``torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer,
mode="max", factor=0.5, patience=2)`` and steps it once per epoch on the validation metric (trainer.py:125-132).
torch's class refuses any object that is not a ``torch.optim.Optimizer``, so it cannot drive
``RowSparseAdam`` / ``RowSparseAdamW`` / ``RowSparseSGD``; this one has torch's semantics and only reads and sets
``opt.lr`` (which writes the device scalar every apply launch reads: captured graphs follow).
"""

from __future__ import annotations

import math


class ReduceLROnPlateau:
    """``torch.optim.lr_scheduler.ReduceLROnPlateau`` over ``opt.lr``: after more than ``patience`` steps without
    an improvement (``threshold`` relative or absolute, per ``threshold_mode``) the learning rate becomes
    ``max(lr * factor, min_lr)`` — unless that changes it by ``eps`` or less — and ``cooldown`` steps follow in
    which bad steps are not counted.  Defaults are the reference trainer's (mode "max", factor 0.5, patience 2)."""

    def __init__(self, optimizer, mode: str = "max", factor: float = 0.5, patience: int = 2,
                 threshold: float = 1e-4, threshold_mode: str = "rel", cooldown: int = 0, min_lr: float = 0.0,
                 eps: float = 1e-8) -> None:
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if mode not in ("min", "max"):
            raise ValueError(f"mode {mode} is unknown!")
        if threshold_mode not in ("rel", "abs"):
            raise ValueError(f"threshold mode {threshold_mode} is unknown!")
        self.optimizer = optimizer
        self.mode, self.factor, self.patience = mode, factor, patience
        self.threshold, self.threshold_mode = threshold, threshold_mode
        self.cooldown, self.min_lr, self.eps = cooldown, float(min_lr), eps
        self.best = math.inf if mode == "min" else -math.inf
        self.num_bad_epochs = 0
        self.cooldown_counter = 0
        self.last_epoch = 0

    @property
    def in_cooldown(self) -> bool:
        return self.cooldown_counter > 0

    def is_better(self, a: float, best: float) -> bool:
        if self.mode == "min":
            return a < best * (1.0 - self.threshold) if self.threshold_mode == "rel" else a < best - self.threshold
        return a > best * (self.threshold + 1.0) if self.threshold_mode == "rel" else a > best + self.threshold

    def step(self, metrics) -> None:
        current = float(metrics)
        self.last_epoch += 1
        if self.is_better(current, self.best):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.in_cooldown:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            old = float(self.optimizer.lr)
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.optimizer.lr = new
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0

    def get_last_lr(self):
        return [float(self.optimizer.lr)]

    def state_dict(self) -> dict:
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, sd: dict) -> None:
        self.__dict__.update(sd)


def build_scheduler(optimizer, cfg):
    """The scheduler ``Trainer._build_scheduler`` (trainer.py:80-89) would build for ``cfg.training.scheduler``:
    ``reduce_on_plateau`` -> ``ReduceLROnPlateau(opt, mode="max", factor=0.5, patience=2)``, ``none`` -> None."""
    name = cfg.training.scheduler
    if name == "reduce_on_plateau":
        return ReduceLROnPlateau(optimizer, mode="max", factor=0.5, patience=2)
    if name == "none":
        return None
    raise ValueError(f"Unknown scheduler: {name}")
