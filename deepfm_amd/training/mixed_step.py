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
reference's, and bitwise reproducible.  ``mixed_train_ineligible_reason`` names what that step refuses.

xDeepFM and AttentionDeepFM train on the same schemas through the same record machinery (``_FusedMixedStep``):

    ``FusedMixedXDeepFMStep``          the CIN reads fe; its backward and nothing else writes d fe; no FM term
    ``FusedMixedAttentionDeepFMStep``  the tower reads xcat = [attention(fe) | flat]: the gather writes flat into its
                                       second part at the row stride, the blocks' d x is d fe, and the FM backward
                                       rides in the embedding backward (``dfm_embedding_backward_record_fm`` with
                                       g_logits, S = sum_f e from the gather, fe): no ``dfm_fm_backward`` launch

``mixed_step_class`` / ``mixed_step_ineligible_reason`` answer for the family.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from deepfm_amd import _lib
from deepfm_amd.data.schema import FeatureType
from deepfm_amd.training.dense_table import DenseTableOptimizer
from deepfm_amd.training.fused_step import (FusedAttentionDeepFMStep, FusedXDeepFMStep, _FusedTowerStep, _tower_fusable,
                                            attention_forward)
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
    return _schema_reason(model, batch_size)


def _schema_reason(model, batch_size: Optional[int] = None) -> Optional[str]:
    """The checks every mixed-schema step shares: schema, record gather and backward caps, grad mode, training mode,
    tower, released tables."""
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


def _cin_reason(model) -> Optional[str]:
    """The CIN stacks ``dfm_cin_forward`` lays out (csrc/cin.hip:make_layout); the matrix-core and the general fp32
    kernels take every such stack between them."""
    cin = model.cin
    sizes = list(cin.layer_sizes)
    if not 1 <= len(sizes) <= 16:
        return f"the CIN has {len(sizes)} layers: the CIN kernels take 1 to 16"
    for i, c in enumerate(sizes):
        if c < 1 or (cin.split_half and i < len(sizes) - 1 and c < 2):
            return f"CIN layer {i} has {c} feature maps: too small" + (" to split in half" if c == 1 else "")
    return None


def _attention_reason(model) -> Optional[str]:
    att = model.attention
    F = model.schema.num_fields
    if att.embed_dim % 4 or att.attention_dim % 4 or att.embed_dim > 64:
        return (f"attention embed_dim {att.embed_dim} / attention_dim {att.attention_dim}: the fused attention kernels "
                "take multiples of 4 with embed_dim <= 64")
    if not _lib.load().dfm_attention_core_supported(F, att.attention_dim, att.num_heads):
        return (f"attention over {F} fields with attention_dim {att.attention_dim} and {att.num_heads} heads is outside "
                "the attention core kernel's shapes (dfm_attention_core_supported)")
    if not all(b.gemm_path for b in att.layers):
        return "an attention block does not run on the GEMM path (gemm_path is off)"
    return None


def _family():
    from deepfm_amd.models.attention_deepfm import AttentionDeepFM
    from deepfm_amd.models.deepfm import DeepFM
    from deepfm_amd.models.xdeepfm import xDeepFM
    return {DeepFM: (FusedMixedDeepFMStep, None), xDeepFM: (FusedMixedXDeepFMStep, _cin_reason),
            AttentionDeepFM: (FusedMixedAttentionDeepFMStep, _attention_reason)}


def mixed_step_ineligible_reason(model, batch_size: Optional[int] = None) -> Optional[str]:
    """Why no fused mixed-schema step (``FusedMixedDeepFMStep``, ``FusedMixedXDeepFMStep``,
    ``FusedMixedAttentionDeepFMStep``) can take ``model`` (None: ``mixed_step_class(model)`` can).  Host only."""
    entry = _family().get(type(model))
    if entry is None:
        return (f"no fused mixed-schema step for {type(model).__name__}: DeepFM, xDeepFM and AttentionDeepFM only")
    reason = _schema_reason(model, batch_size)
    if reason is None and entry[1] is not None:
        reason = entry[1](model)
    return reason


def mixed_step_class(model):
    """The fused mixed-schema step that takes ``model``, or None (``mixed_step_ineligible_reason`` says why)."""
    if mixed_step_ineligible_reason(model) is not None:
        return None
    return _family()[type(model)][0]


class _FusedMixedStep(_FusedTowerStep):
    """The schema side of the mixed steps: record packing, the record gather and the record backward as the two
    graph nodes re-pointed per launch, ``capture()``'s restore check, ``total_norm``.  Subclasses say what feeds the
    logit (``_interaction_forward`` / ``_interaction_backward``), which optional outputs the gather has
    (``_gather_outputs``) and, with ``folded_fm``, the FM trio of the embedding backward (``_fm_trio``)."""

    rowplan_first_default = False      # no row plan at all: the tables are dense parameters
    plan_lookahead_default = False
    folded_fm = False                  # True: dfm_embedding_backward_record_fm instead of ..._record

    @classmethod
    def _ineligible_reason(cls, model, batch_size: Optional[int] = None) -> Optional[str]:
        if _family().get(type(model), (None,))[0] is not cls:
            return f"{cls.__name__} does not take {type(model).__name__} (mixed_step_class(model) names the step)"
        return mixed_step_ineligible_reason(model, batch_size)

    @classmethod
    def eligible(cls, model) -> bool:
        return cls._ineligible_reason(model) is None

    def __init__(self, model, optimizer: DenseTableOptimizer, batch_size: int, use_graph: bool = True) -> None:
        reason = self._ineligible_reason(model, batch_size)
        if reason is not None:
            raise ValueError(f"{type(self).__name__}: {reason}")
        if not isinstance(optimizer, DenseTableOptimizer):
            raise ValueError(f"{type(self).__name__} needs a dense-table optimizer (build_dense_optimizer)")
        super().__init__(model, optimizer, batch_size, use_graph)
        self._grads = {id(p): p.grad for p in self.emb.parameters()}
        self._cur_record: torch.Tensor = self.inbox      # the record the embedding backward reads
        self._nodes: Optional[Dict[str, C.c_void_p]] = None

    # ------------------------------------------------------------------ hooks
    def _check_embedding(self) -> None:
        """``dense`` grad mode (checked by ``mixed_train_ineligible_reason``): the step never calls autograd."""

    def _dense_slice_count(self) -> int:
        return int(_lib.load().dfm_embedding_backward_record_parts(self.B))

    def _tower_input(self) -> torch.Tensor:
        """The tower reads flat (B, T); ``_flat`` / ``_g_flat`` are (address, floats between rows) of flat and d flat."""
        self.T = sum(s.embedding_dim for s in self.model.schema.fields.values())
        self.flat = torch.empty(self.B, self.T, dtype=torch.float32, device=self.fe.device)
        self.g_flat = torch.empty_like(self.flat)
        self._flat, self._g_flat = (self.flat.data_ptr(), self.T), (self.g_flat.data_ptr(), self.T)
        return self.flat

    def _tower_input_grad(self) -> torch.Tensor:
        return self.g_flat

    def _build_rowplan(self) -> None:
        """No row plan."""

    def _gather_outputs(self):
        """(FM value (B) or None, S = sum_f e (B, D) or None) of the record gather."""
        return None, None

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
        fm, fm_sum = self._gather_outputs()
        return (record.data_ptr(), self.B, self.fo, self.fe, *self._flat, fm, self.labels, fm_sum)

    def _backward_args(self, record: torch.Tensor):
        opt = self.opt
        trio = tuple(C.c_void_p(p) for p in self._fm_trio()) if self.folded_fm else ()
        return (C.c_void_p(record.data_ptr()), self.B, self.g_logits.data_ptr(), self.g_fe.data_ptr(),
                C.c_void_p(self._g_flat[0]), self._g_flat[1], C.c_void_p(self._flat[0]), self._flat[1], *trio,
                self.emb._grad_struct(self._grads), opt.flat_grad.data_ptr(), opt.n_l2, self._dense_partial.data_ptr())

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
        lib = _lib.load()
        update = lib.dfm_embedding_backward_record_fm_update if self.folded_fm else lib.dfm_embedding_backward_record_update
        _lib.check(update(self.emb._ensure_plan(self.fe.device), C.c_void_p(graph_exec), nodes["backward"],
                          *self._backward_args(record)))

    def _embedding_backward(self, g_fo: torch.Tensor, g_fe: torch.Tensor) -> None:
        lib = _lib.load()
        launch = lib.dfm_embedding_backward_record_fm if self.folded_fm else lib.dfm_embedding_backward_record
        _lib.check(launch(self.emb._ensure_plan(self.fe.device), *self._backward_args(self._cur_record),
                          _lib.stream_handle()))
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


class FusedMixedDeepFMStep(_FusedMixedStep):
    """DeepFM (deepfm.py:30-42) on a mixed schema: logits = (fo + fm) + output_linear(dnn(flat)).  ``optimizer`` is a
    ``DenseTableOptimizer`` (``build_dense_optimizer``); records are ``RecordLayout.of(schema, B)`` records
    (``pack_record``, ``PackedBatchLoader`` / ``DeviceBatchRing``)."""

    head_name = "output_linear"

    @classmethod
    def _ineligible_reason(cls, model, batch_size: Optional[int] = None) -> Optional[str]:
        return mixed_train_ineligible_reason(model, batch_size)

    def __init__(self, model, optimizer: DenseTableOptimizer, batch_size: int, use_graph: bool = True) -> None:
        super().__init__(model, optimizer, batch_size, use_graph)
        self.fm = torch.empty(batch_size, dtype=torch.float32, device=optimizer.device)

    def _gather_outputs(self):
        return self.fm, None

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

    head_name = "dnn_linear"
    folded_fm = True
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

    head_name = "output_linear"
    folded_fm = True

    def _tower_input(self) -> torch.Tensor:
        B, F, D = self.fe.shape
        self.T = sum(s.embedding_dim for s in self.model.schema.fields.values())
        self._ld = F * D + self.T
        f32 = dict(dtype=torch.float32, device=self.fe.device)
        self.xcat = torch.empty(B, self._ld, **f32)
        self.g_xcat = torch.empty_like(self.xcat)
        self.g_att = torch.empty(B, F * D, **f32)      # d attention-out, contiguous: a last block without residual
        self._flat = (self.xcat.data_ptr() + 4 * F * D, self._ld)
        self._g_flat = (self.g_xcat.data_ptr() + 4 * F * D, self._ld)
        return self.xcat

    def _tower_input_grad(self) -> torch.Tensor:
        return self.g_xcat

    def _gather_outputs(self):
        return self.fm, self.fm_sum

    def _fm_trio(self):
        return self.g_logits.data_ptr(), self.fm_sum.data_ptr(), self.fe.data_ptr()

    def _interaction_forward(self):
        self._ctxs = attention_forward(self.blocks, self.fe, self.xcat, ld=self._ld, copy_fe=False)
        return self.fm

    def _finish_embedding_grad(self) -> None:
        from deepfm_amd.models.layers.attention import _AttnGemmFn
        lib, st = _lib.load(), _lib.stream_handle()
        B, F, D = self.fe.shape
        FD = F * D
        if self.blocks[-1].use_residual:       # the residual LayerNorm's backward reads rows of d xcat in place
            g = self.g_xcat
            self._ctxs[-1].g_from = self._ld
        else:
            g = self.g_att.view(B, F, D)
            _lib.check(lib.dfm_copy_2d(self.g_xcat.data_ptr(), self._ld, g.data_ptr(), FD, B, FD, st))
        # the first block's d x is d fe as it stands: its whole-block kernel stores it into g_fe (a tail of nothing)
        self._ctxs[0].grad_tail = dict(out=self.g_fe, g_flat=None, ld_flat=0, g_fm=None, fm_sum=None)
        for block, ctx in zip(reversed(self.blocks), reversed(self._ctxs)):
            out = _AttnGemmFn.backward(ctx, g)
            g = out[1]
            if len(out) > 2:           # the flat buffer is not laid out for direct writes: add the temporaries
                ps = block._param_list()
                torch._foreach_add_([p.grad for p in ps], [t.view_as(p) for t, p in zip(out[2:], ps)])
        if not getattr(self._ctxs[0], "tail_done", False):
            _lib.check(lib.dfm_copy_2d(g.data_ptr(), FD, self.g_fe.data_ptr(), FD, B, FD, st))
