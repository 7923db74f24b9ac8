"""DenseTableAdam / DenseTableAdamW / DenseTableSGD: the optimizer of the fused mixed-schema step.

A mixed schema's tables are small (MovieLens: 3 112 rows, a quarter of the tower's parameters), so here they are
simply dense parameters: EVERY parameter of the model — ``(V, d)`` and ``(V, 1)`` tables, EmbeddingBag tables,
projections, DENSE-field Linears, tower, head — is a view of one flat parameter / gradient / moment buffer, the
embedding's parameters first (``n_l2``: they take the L2 term of base.py:78-83).  One step is the dense half of the
row-sparse optimizer's launches (same device bodies): ``dfm_step_dense_prepare`` (gradient slabs + L2 + norm
partials), ``dfm_grad_norm_finalize`` (clip coefficient, step / dropout-seed tick), ``dfm_step_dense_apply``.

Unlike the row-sparse optimizers this IS the reference's trajectory (trainer.py:212-240): dense Adam moves rows no
sample named (L2, stale moments) exactly as ``torch.optim.Adam`` over ``model.parameters()`` does.  Everything else
— ``opt.lr`` on the device, ``param_groups``, ``state_dict()`` / ``load_state_dict()`` keyed by parameter name or
read from the torch optimizer of the same kind, ``build_scheduler`` — is ``RowSparseOptimizer``'s.  One rank only.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from deepfm_amd import _lib
from deepfm_amd.training import exchange
from deepfm_amd.training.rowsparse import RowSparseOptimizer


class DenseTableOptimizer(RowSparseOptimizer):
    row_tables = False

    def __init__(self, model: torch.nn.Module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 l2: float = 0.0, max_grad_norm: Optional[float] = None, weight_decay: float = 0.0,
                 momentum: float = 0.0) -> None:
        if exchange.world_size(None) > 1:
            raise NotImplementedError("the dense-table optimizers run on one rank")
        super().__init__(model, lr=lr, betas=betas, eps=eps, l2=l2, max_grad_norm=max_grad_norm,
                         weight_decay=weight_decay, momentum=momentum)
        if self.split:
            raise NotImplementedError("the dense-table optimizers have no data-parallel exchange")
        n = self.flat_param.numel()
        self._partials = torch.zeros(_lib.load().dfm_step_dense_num_partials(n), dtype=torch.float32,
                                     device=self.device)

    @torch.no_grad()
    def exchange(self) -> None:
        """One rank: nothing to exchange."""

    @torch.no_grad()
    def apply(self) -> None:
        """Slabs + L2 + global norm, clip coefficient, the update rule on the whole flat buffer: three launches,
        no host synchronisation.  The gradient buffer is left zeroed."""
        lib, st = _lib.load(), _lib.stream_handle()
        n = self.flat_param.numel()
        refs, n_refs = self.slab_refs if self.slab_refs is not None else (None, 0)
        _lib.check(lib.dfm_step_dense_prepare(self.l2, self.flat_grad.data_ptr(), self.flat_param.data_ptr(), n,
                                              self.n_l2, refs, n_refs, self._partials.data_ptr(), st))
        _lib.check(lib.dfm_grad_norm_finalize(self._partials.data_ptr(), self._partials.numel(),
                                              self.max_grad_norm or 0.0, self.sq_norm.data_ptr(),
                                              self.clip_coef.data_ptr(), self.step_count.data_ptr(),
                                              _lib.ptr(self.seed_tick), st))
        _lib.check(lib.dfm_step_dense_apply(self.clip_coef.data_ptr(), C.byref(self._optim_struct()),
                                            self.step_count.data_ptr(), self.flat_param.data_ptr(),
                                            self.flat_m.data_ptr(), self._flat_v_ptr(), self.flat_grad.data_ptr(), n, 1,
                                            st))


class DenseTableAdam(DenseTableOptimizer):
    """torch.optim.Adam over every parameter (trainer.py:67-70)."""
    kind = "adam"

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, l2: float = 0.0,
                 max_grad_norm: Optional[float] = None) -> None:
        super().__init__(model, lr=lr, betas=betas, eps=eps, l2=l2, max_grad_norm=max_grad_norm)


class DenseTableAdamW(DenseTableOptimizer):
    """torch.optim.AdamW (trainer.py:71-72; default ``weight_decay=0.01``); the decay is not part of the norm."""
    kind = "adamw"

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 l2: float = 0.0, max_grad_norm: Optional[float] = None) -> None:
        super().__init__(model, lr=lr, betas=betas, eps=eps, l2=l2, max_grad_norm=max_grad_norm,
                         weight_decay=weight_decay)


class DenseTableSGD(DenseTableOptimizer):
    """torch.optim.SGD(momentum=0.9) (trainer.py:73-76): the buffer lives in ``flat_m``; no second moment."""
    kind = "sgd"

    def __init__(self, model, lr: float = 1e-3, momentum: float = 0.9, l2: float = 0.0,
                 max_grad_norm: Optional[float] = None) -> None:
        super().__init__(model, lr=lr, l2=l2, max_grad_norm=max_grad_norm, momentum=momentum)


DENSE_OPTIMIZERS = {"adam": DenseTableAdam, "adamw": DenseTableAdamW, "sgd": DenseTableSGD}


def build_dense_optimizer(model: torch.nn.Module, cfg) -> DenseTableOptimizer:
    """``build_optimizer`` for the fused mixed-schema step: the dense-table optimizer of ``training.optimizer``
    with torch's defaults, ``training.lr``, ``feature.embedding_l2_reg`` and ``training.gradient_clip_norm``."""
    tc = cfg.training
    cls = DENSE_OPTIMIZERS.get(tc.optimizer)
    if cls is None:
        raise ValueError(f"Unknown optimizer: {tc.optimizer}")
    clip = tc.gradient_clip_norm
    return cls(model, lr=tc.lr, l2=cfg.feature.embedding_l2_reg, max_grad_norm=clip if clip else None)
