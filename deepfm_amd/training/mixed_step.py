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
reference's, and bitwise reproducible.  DeepFM only; ``mixed_train_ineligible_reason`` names what else is refused.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from deepfm_amd import _lib
from deepfm_amd.data.schema import FeatureType
from deepfm_amd.training.dense_table import DenseTableOptimizer
from deepfm_amd.training.fused_step import _FusedTowerStep, _tower_fusable
from deepfm_amd.training.predict import _released_table, record_gather_reason

_BWD_STAGE = 256      # csrc/embedding.hip: kBwdStage (samples in LDS at a time)


def backward_lds_bytes(model) -> int:
    """LDS bytes per workgroup of ``dfm_embedding_backward_record`` for this schema (csrc/embedding.hip:
    describe_bwd_record): the widest field's staged vectors + ids + projection, or a projection job's operands."""
    D = model.embedding.fm_embed_dim
    need = 0
    for spec in model.schema.fields.values():
        d = spec.embedding_dim
        L = spec.max_length if spec.feature_type is FeatureType.SEQUENCE else 1
        proj = D * d if d != D else 0
        need = max(need, 16 * (_BWD_STAGE * (d // 4 + 1) + (_BWD_STAGE * L + 3) // 4 + 1) + 4 * proj)
        if proj:
            need = max(need, 4 * _BWD_STAGE * (D + d))
    return need


def mixed_train_ineligible_reason(model, batch_size: Optional[int] = None) -> Optional[str]:
    """Why ``FusedMixedDeepFMStep`` cannot take ``model`` (None: it can).  Checked on the host only, before any device
    work.  ``batch_size``: also check the row-owned scan's size cap for that batch."""
    from deepfm_amd.models.deepfm import DeepFM
    if type(model) is not DeepFM:
        return (f"no fused mixed-schema step for {type(model).__name__}: DeepFM only (xDeepFM and AttentionDeepFM "
                "are the next step, DESIGN.md section 9)")
    emb = model.embedding
    D = emb.fm_embed_dim
    specs = list(model.schema.fields.values())
    if all(s.feature_type is not FeatureType.SEQUENCE and s.embedding_dim == D for s in specs) and D % 4 == 0:
        return "uniform schema: use the row-sparse step (set_grad_mode('rowsparse') and fused_step_class(model))"
    reason = record_gather_reason(model)
    if reason is not None:
        return reason
    for name, spec in model.schema.fields.items():
        if spec.feature_type is FeatureType.SEQUENCE and spec.combiner == "max":
            return (f"field {name!r} pools with max: the embedding backward's arg-max recompute is not built "
                    "(mean and sum bags only; train it in dense autograd mode)")
    nbytes = backward_lds_bytes(model)
    if nbytes > _lib.BWD_RECORD_LDS_BYTES:
        return (f"the embedding backward stages {nbytes} bytes of LDS for the widest field, over its cap of "
                f"{_lib.BWD_RECORD_LDS_BYTES}")
    rows = sum(s.vocabulary_size for s in specs if s.feature_type is not FeatureType.DENSE)
    if batch_size is not None and rows * batch_size > _lib.BWD_RECORD_MAX_ROW_SAMPLES:
        return (f"{rows} table rows x {batch_size} samples is over the row-owned scan's cap of "
                f"{_lib.BWD_RECORD_MAX_ROW_SAMPLES} (tables this large belong to a row-sparse design)")
    if emb.grad_mode != "dense":
        return "the embedding must be in 'dense' grad mode (its tables are dense parameters of the flat buffer)"
    if not model.training:
        return "the model must be in training mode"
    if not _tower_fusable(model):
        return ("the DNN tower is not fusable: Linear -> BatchNorm1d (affine, momentum) -> ReLU, hidden widths "
                "multiples of 4, the last one a multiple of 32 and <= 256, input width a multiple of 4")
    name = _released_table(model)
    if name is not None:
        return f"the embedding table of field {name!r} is released (field-sharded model): call restore_tables() first"
    return None


class FusedMixedDeepFMStep(_FusedTowerStep):
    """DeepFM (deepfm.py:30-42) on a mixed schema: logits = (fo + fm) + output_linear(dnn(flat)).  ``optimizer`` is a
    ``DenseTableOptimizer`` (``build_dense_optimizer``); records are ``RecordLayout.of(schema, B)`` records
    (``pack_record``, ``PackedBatchLoader`` / ``DeviceBatchRing``)."""

    head_name = "output_linear"
    rowplan_first_default = False      # no row plan at all: the tables are dense parameters
    plan_lookahead_default = False

    @staticmethod
    def eligible(model) -> bool:
        return mixed_train_ineligible_reason(model) is None

    def __init__(self, model, optimizer: DenseTableOptimizer, batch_size: int, use_graph: bool = True) -> None:
        reason = mixed_train_ineligible_reason(model, batch_size)
        if reason is not None:
            raise ValueError(f"{type(self).__name__}: {reason}")
        if not isinstance(optimizer, DenseTableOptimizer):
            raise ValueError(f"{type(self).__name__} needs a dense-table optimizer (build_dense_optimizer)")
        super().__init__(model, optimizer, batch_size, use_graph)
        self.fm = torch.empty(batch_size, dtype=torch.float32, device=optimizer.device)
        self._grads = {id(p): p.grad for p in self.emb.parameters()}
        self._cur_record: torch.Tensor = self.inbox      # the record the embedding backward reads
        self._nodes: Optional[Dict[str, C.c_void_p]] = None

    # ------------------------------------------------------------------ hooks
    def _check_embedding(self) -> None:
        """``dense`` grad mode (checked by ``mixed_train_ineligible_reason``): the step never calls autograd."""

    def _dense_slice_count(self) -> int:
        return int(_lib.load().dfm_embedding_backward_record_parts(self.B))

    def _tower_input(self) -> torch.Tensor:
        self.T = sum(s.embedding_dim for s in self.model.schema.fields.values())
        self.flat = torch.empty(self.B, self.T, dtype=torch.float32, device=self.fe.device)
        return self.flat

    def _tower_input_grad(self) -> torch.Tensor:
        self.g_flat = torch.empty_like(self.flat)
        return self.g_flat

    def _build_rowplan(self) -> None:
        """No row plan."""

    def _interaction_forward(self):
        return self.fm

    def _interaction_backward(self):
        # d fe = g (S - e): flat and fe are different buffers here, so layer 1's d-input epilogue cannot carry it
        B, F, D = self.fe.shape
        _lib.check(_lib.load().dfm_fm_backward(self.fe.data_ptr(), self.g_logits.data_ptr(), B, F, D,
                                               self.g_fe.data_ptr(), _lib.stream_handle()))
        return None

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
        return (record.data_ptr(), self.B, self.fo, self.fe, self.flat.data_ptr(), self.T, self.fm, self.labels)

    def _backward_args(self, record: torch.Tensor):
        opt = self.opt
        return (C.c_void_p(record.data_ptr()), self.B, self.g_logits.data_ptr(), self.g_fe.data_ptr(),
                self.g_flat.data_ptr(), self.T, self.flat.data_ptr(), self.T, self.emb._grad_struct(self._grads),
                opt.flat_grad.data_ptr(), opt.n_l2, self._dense_partial.data_ptr())

    def _gather(self, record: Optional[torch.Tensor] = None) -> None:
        record = self._record if record is None else record
        self._cur_record = record
        self.emb.forward_record(*self._forward_args(record))

    def _capture_gather(self, record: torch.Tensor):
        self._gather(record)
        nodes = {"gather": C.c_void_p(), "backward": None}
        _lib.check(_lib.load().dfm_graph_last_node(_lib.stream_handle(), C.byref(nodes["gather"])))
        self._nodes = nodes                    # _embedding_backward adds its node
        return nodes

    def _update_gather(self, graph_exec: int, nodes, record: torch.Tensor) -> None:
        self.emb.forward_record_update(graph_exec, nodes["gather"], *self._forward_args(record))
        _lib.check(_lib.load().dfm_embedding_backward_record_update(
            self.emb._ensure_plan(self.fe.device), C.c_void_p(graph_exec), nodes["backward"],
            *self._backward_args(record)))

    def _embedding_backward(self, g_fo: torch.Tensor, g_fe: torch.Tensor) -> None:
        lib = _lib.load()
        _lib.check(lib.dfm_embedding_backward_record(self.emb._ensure_plan(self.fe.device),
                                                     *self._backward_args(self._cur_record), _lib.stream_handle()))
        if self._nodes is not None and torch.cuda.is_current_stream_capturing():
            node = C.c_void_p()
            _lib.check(lib.dfm_graph_last_node(_lib.stream_handle(), C.byref(node)))
            self._nodes["backward"], self._nodes = node, None

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
