"""Fused, graph-captured training step for mixed schemas (MovieLens: a SEQUENCE bag, projected fields of width 4 / 8,
DENSE fields): the step of ``fused_step.py`` with the embedding tables as DENSE parameters.

``set_grad_mode("rowsparse")`` refuses these schemas for a reason: all tables together are a
quarter of the tower, so row-sparse updates save nothing.  Turned round: tables that small can live in the flat
parameter buffer (``training/dense_table.py``), and the step is

    record gather: first_order, flat (the tower's input), fe, FM value, labels      1 launch (graph node, re-pointed)
    tower + head                                                               ``_FusedTowerStep``'s launches
    FM backward g (S - e) into d fe                                                 1 launch (dfm_fm_backward)
    tower backward; layer 1 stores d flat alone (flat and fe are different bytes)
    embedding backward from the record: every table / projection / DENSE-field
      gradient as batch slices, no atomics (dfm_embedding_backward_record)          1 launch (graph node, re-pointed)
    slabs + L2 + norm, clip coefficient, update rule on the flat buffer             3 launches

No autograd, no row plan, no lazy moments: dense Adam moves untouched rows and L2 reaches every row, as the
reference's ``torch.optim.Adam`` over ``model.parameters()`` does (trainer.py:212-240) — the trajectory IS the
reference's, and bitwise reproducible.

xDeepFM and AttentionDeepFM train on the same schemas through the same record machinery (``_FusedMixedStep``):

    ``FusedMixedXDeepFMStep``          the CIN reads fe; its backward and nothing else writes d fe; no FM term
    ``FusedMixedAttentionDeepFMStep``  the tower reads xcat = [attention(fe) | flat]: the gather writes flat into its
                                       second part at the row stride, the blocks' d x is d fe, and the FM backward
                                       rides in the embedding backward (``dfm_embedding_backward_record``, fold_fm, the
                                       trio g_logits, S = sum_f e from the gather, fe): no ``dfm_fm_backward`` launch

``mixed_step_class`` picks the class; ``mixed_step_ineligible_reason`` (training/eligibility.py) names a refusal.
"""

from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, Optional

import torch

from deepfm_amd import _lib
from deepfm_amd.training.dense_table import DenseTableOptimizer
from deepfm_amd.training.eligibility import (backward_lds_bytes, mixed_step_ineligible_reason,  # noqa: F401
                                             mixed_train_ineligible_reason, model_kind)
from deepfm_amd.training.fused_step import FusedAttentionDeepFMStep, FusedXDeepFMStep, _FusedTowerStep


def check_tail_rows(model, n: int) -> None:
    """``ValueError`` for a trailing batch no step can train on.  Host only."""
    if n < 1:
        raise ValueError(f"a tail step needs at least one row, got {n}")
    if n == 1:
        width = model.dnn.mlp[0].out_features
        raise ValueError("Expected more than 1 value per channel when training, got input size "
                         f"torch.Size([1, {width}]) (an epoch whose trailing batch is one row: BatchNorm1d has no "
                         "batch statistics for it; change batch_size or drop a row)")


class _FusedMixedStep(_FusedTowerStep):
    """The schema side of the mixed steps: record packing, the record gather and the record backward as the two
    graph nodes re-pointed per launch, ``capture()``'s restore check, ``total_norm``.  Subclasses say what feeds the
    logit (``_interaction_forward`` / ``_interaction_backward``), which optional outputs the gather has
    (``gather_outputs``), which instantiation of the embedding backward runs (``folded_fm``) and, with it, the FM
    trio (``_fm_trio``)."""

    rowplan_first_default = False      # no row plan at all: the tables are dense parameters
    plan_lookahead_default = False
    folded_fm = False                  # dfm_embedding_backward_record's fold_fm: the instantiation with the FM term

    @classmethod
    def ineligible_reason(cls, model, batch_size: Optional[int] = None) -> Optional[str]:
        if model_kind(model) != cls.model_kind:
            return f"{cls.__name__} does not take {type(model).__name__} (mixed_step_class(model) names the step)"
        return mixed_step_ineligible_reason(model, batch_size)

    def __init__(self, model, optimizer: DenseTableOptimizer, batch_size: int, use_graph: bool = True) -> None:
        super().__init__(model, optimizer, batch_size, use_graph)
        self._grads = {id(p): p.grad for p in self.emb.parameters()}
        self._cur_record: torch.Tensor = self.inbox      # the record the embedding backward reads
        self._backward_node: Optional[C.c_void_p] = None      # of the record backward captured last

    # ------------------------------------------------------------------ hooks
    def _check_optimizer(self, optimizer) -> None:
        if not isinstance(optimizer, DenseTableOptimizer):
            raise ValueError(f"{type(self).__name__} needs a dense-table optimizer (build_dense_optimizer)")

    def _check_embedding(self) -> None:
        """``dense`` grad mode (checked by ``ineligible_reason``): the step never calls autograd."""

    def _dense_slice_count(self) -> int:
        return int(_lib.load().dfm_embedding_backward_record_parts(self.B))

    @functools.cached_property
    def T(self) -> int:
        """Width of flat_embeddings: every field at its own width."""
        return sum(s.embedding_dim for s in self.model.schema.fields.values())

    def _tower_input(self) -> torch.Tensor:
        """The tower reads flat (B, T); ``_flat`` / ``_g_flat`` are (address, floats between rows) of flat and d flat."""
        self.flat = torch.empty(self.B, self.T, dtype=torch.float32, device=self.fe.device)
        self.g_flat = torch.empty_like(self.flat)
        self._flat, self._g_flat = (self.flat.data_ptr(), self.T), (self.g_flat.data_ptr(), self.T)
        return self.flat

    def _tower_input_grad(self) -> torch.Tensor:
        return self.g_flat

    def _build_rowplan(self) -> None:
        """No row plan."""

    def _fm_trio(self):
        """``folded_fm``: (g_fm, S, fe) addresses of the FM backward inside the embedding backward, or Nones."""
        return None, None, None

    # ------------------------------------------------------------------ inputs
    def pack_record(self, batch: Dict[str, torch.Tensor], labels: torch.Tensor) -> torch.Tensor:
        """One device record of ``batch`` (the reference's dict: SPARSE (B,) ids, DENSE (B,) values, SEQUENCE
        (B, max_length) ids, 0-padded) and ``labels`` (B,), for ``run_from`` / ``run_group``."""
        rec = torch.zeros(self.packed_bytes, dtype=torch.uint8, device=self.inbox.device)
        self._fill(rec, batch, labels)
        return rec

    def _fill(self, rec: torch.Tensor, batch: Dict[str, torch.Tensor], labels: torch.Tensor) -> None:
        from deepfm_amd.data.packed import RecordLayout
        views, lab = RecordLayout.of(self.model.schema, self.B).unpack(rec)
        for name, dst in views.items():
            dst.copy_(batch[name].to(dst.dtype), non_blocking=True)
        lab.copy_(labels.to(torch.float32), non_blocking=True)

    def load_batch(self, batch: Dict[str, torch.Tensor], labels: torch.Tensor) -> None:   # noqa: D102
        """``batch`` dict and ``labels`` into the inbox record; the next ``run()`` trains on it."""
        self._fill(self.inbox, batch, labels)
        self._record = self.inbox

    def pack_batches(self, *args, **kwargs):
        raise NotImplementedError("mixed records are built by pack_record() or PackedBatchLoader")

    # ------------------------------------------------------------------ the two launches that read the record
    def _forward_args(self, record: torch.Tensor):
        out = self._gather_args()
        return (record.data_ptr(), self.B, self.fo, self.fe, *self._flat, out["fm_out"], self.labels, out["fm_sum"])

    def _backward_args(self, record: torch.Tensor):
        opt = self.opt
        trio = tuple(C.c_void_p(p) for p in self._fm_trio())
        return (C.c_void_p(record.data_ptr()), self.B, self.g_logits.data_ptr(), self.g_fe.data_ptr(),
                C.c_void_p(self._g_flat[0]), self._g_flat[1], C.c_void_p(self._flat[0]), self._flat[1], *trio,
                int(self.folded_fm),
                self.emb._grad_struct(self._grads), opt.flat_grad.data_ptr(), opt.n_l2, self._dense_partial.data_ptr())

    def _gather(self, record: Optional[torch.Tensor] = None) -> None:
        record = self._record if record is None else record
        self._cur_record = record
        self.emb.forward_record(*self._forward_args(record))

    def _launch_backward(self, record: torch.Tensor, at: _lib.Launch) -> None:
        _lib.check(_lib.load().dfm_embedding_backward_record(self.emb._ensure_plan(self.fe.device),
                                                             *self._backward_args(record), at))

    def _capture_gather(self, record: torch.Tensor, with_plan: bool = True) -> C.c_void_p:
        self._gather(record)
        return _lib.last_node()

    def _record_nodes(self, gather_node):
        return {"gather": gather_node, "backward": self._backward_node}

    def _update_gather(self, at, record: torch.Tensor) -> None:
        self.emb.forward_record(*self._forward_args(record), at=at["gather"])
        self._launch_backward(record, at["backward"])

    def _embedding_backward(self, g_fo: torch.Tensor, g_fe: torch.Tensor) -> None:
        self._launch_backward(self._cur_record, _lib.stream_handle())
        if torch.cuda.is_current_stream_capturing():
            self._backward_node = _lib.last_node()

    # ------------------------------------------------------------------ capture
    def capture(self, warmup_iters: int = 1, timed_variant: bool = False, steps_per_graph: int = 1) -> None:
        """``RowSparseTrainStep.capture``; the warm-up steps run on an all-padding batch, and with dense Adam even
        that batch moves every parameter (L2, stale moments), so the restore is checked here: model, optimizer state,
        step counter and dropout seed must come back bit for bit."""
        if timed_variant:
            raise NotImplementedError("the mixed step has no timed variant")
        if not self.use_graph:
            return
        state = self._mutable_state()
        saved = [t.clone() for t in state]
        super().capture(warmup_iters, False, steps_per_graph)
        for t, v in zip(state, saved):
            if not torch.equal(t, v):
                raise RuntimeError("capture() did not restore the training state bit for bit")

    def total_norm(self) -> float:
        """Global gradient norm of the last step (synchronises)."""
        return float(self.opt.sq_norm.sqrt().item())


class FusedMixedDeepFMStep(_FusedMixedStep):
    """DeepFM (deepfm.py:30-42) on a mixed schema: logits = (fo + fm) + output_linear(dnn(flat)).  ``optimizer`` is a
    ``DenseTableOptimizer`` (``build_dense_optimizer``); records are ``RecordLayout.of(schema, B)`` records
    (``pack_record``, ``PackedBatchLoader`` / ``DeviceBatchRing``)."""

    head_name = "output_linear"
    model_kind = "deepfm"
    gather_outputs = ("fm",)

    @classmethod
    def ineligible_reason(cls, model, batch_size: Optional[int] = None) -> Optional[str]:
        return mixed_train_ineligible_reason(model, batch_size)       # (its DeepFM-only wording for another model)

    def _interaction_forward(self):
        return self.fm

    def _interaction_backward(self):
        # d fe = g (S - e): flat and fe are different buffers here, so layer 1's d-input epilogue cannot carry it
        B, F, D = self.fe.shape
        _lib.check(_lib.load().dfm_fm_backward(self.fe.data_ptr(), self.g_logits.data_ptr(), B, F, D,
                                               self.g_fe.data_ptr(), _lib.stream_handle()))
        return None


class FusedMixedXDeepFMStep(_FusedMixedStep, FusedXDeepFMStep):
    """xDeepFM (xdeepfm.py:36-48) on a mixed schema: logits = (fo + cin_linear(cin(fe))) + dnn_linear(dnn(flat)).
    ``FusedXDeepFMStep``'s CIN launches on fe; the CIN's backward stores d fe (nothing else reaches fe: the tower
    reads flat), and the embedding backward runs without an FM term."""

    folded_fm = True                   # (trio NULL: the plain kernel's bits, and the faster of the two here)
    cin_grad_in_place = True           # dfm_cin_backward writes g_fe itself, no addend for layer 1's epilogue

    def _interaction_backward(self):
        self._cin_backward()
        return None


class FusedMixedAttentionDeepFMStep(_FusedMixedStep, FusedAttentionDeepFMStep):
    """AttentionDeepFM (attention_deepfm.py:48-66) on a mixed schema: logits = (fo + fm) +
    output_linear(dnn(xcat)), xcat = [attention(fe) | flat] (B, F D + T).  The gather writes flat into xcat's second
    part, the last block its output into the first; backward, the last block reads d attention-out in place from
    d xcat, the first block's d x IS d fe, and the embedding backward takes d flat at d xcat's row stride and the FM
    backward's operands (g_logits, S, fe)."""

    folded_fm = True
    copy_fe = False                    # the gather has written flat into xcat's second part: flat is not fe here
    _tower_input = FusedAttentionDeepFMStep._tower_input           # xcat, not _FusedMixedStep's flat
    _tower_input_grad = FusedAttentionDeepFMStep._tower_input_grad

    @functools.cached_property
    def _ld(self) -> int:
        return self.fe[0].numel() + self.T

    def _fm_trio(self):
        return self.g_logits.data_ptr(), self.fm_sum.data_ptr(), self.fe.data_ptr()

    def _grad_tail(self) -> dict:
        """Nothing: the first block's d x IS d fe (d flat and the FM backward belong to the embedding backward)."""
        return dict(g_flat=None, ld_flat=0, g_fm=None, fm_sum=None)


MIXED_STEPS = [FusedMixedDeepFMStep, FusedMixedXDeepFMStep, FusedMixedAttentionDeepFMStep]


def mixed_step_class(model):
    """The fused mixed-schema step that takes ``model``, or None (``mixed_step_ineligible_reason`` says why)."""
    return next((cls for cls in MIXED_STEPS if cls.eligible(model)), None)
