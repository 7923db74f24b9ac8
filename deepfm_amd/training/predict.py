"""Eval-mode forward on the project's kernels, as one HIP graph per batch, and on-device evaluation.

``model.predict`` (reference ``base.py``: sigmoid(forward)) runs the DNN tower on the stock ``nn.Sequential`` in
eval mode, layer by layer from Python.  ``FusedPredictor`` computes the same eval-mode probabilities with

    staged gather (+ FM value) from a batch record                           1 launch (graph node, re-pointed)
    interaction layer (xDeepFM: CIN + cin_linear; AttentionDeepFM: blocks)  the fused training step's launches
    per layer: GEMM + BatchNorm (running statistics) + ReLU                  1 launch (dfm_linear_bn_eval)
    head: logit, sigmoid, rows < valid only                                 1 launch (graph node, re-pointed)
    with a calibrator: its map of the logits, rows < valid only             1 launch (graph node, re-pointed)

``MixedSchemaPredictor`` does the same for any schema of SPARSE, SEQUENCE and DENSE fields with projections and
mixed widths (MovieLens): its gather (``dfm_embedding_forward_record``) reads a record in the mixed layout
(``data/packed.py:mixed_record_layout``) and writes flat_embeddings straight into the tower's input.

``QuantizedPredictor`` is ``FusedPredictor`` serving from row-wise int8 or 4-bit tables (``training/quantized.py``):
its gather (``dfm_embedding_forward_quant``) reads one 16 + D or 8 + D / 2 byte record per (sample, SPARSE field)
instead of an fp32 row and a first-order weight, and after construction the fp32 SPARSE tables are never read.

``QuantizedMixedPredictor`` is ``MixedSchemaPredictor`` serving its SPARSE and SEQUENCE fields of width 16, 32 or 64
from such records, each field at its own width (``dfm_embedding_forward_record_quant``): a history bag is pooled in one
walk of records that carry the first-order weight with the codes.

``evaluate`` scores a whole split in order (the final batch padded, ``drop_last=False`` as trainer.py:244-294)
into one device score buffer, then computes AUC and log loss there (``training/metrics.py``), and on request the
ranking metrics HR@k / NDCG@k per user, the grouped AUC and the calibration numbers (overall, per bin and per
slice).  ``evaluate_loader`` does the same over a ``DeviceEpochLoader``'s rows, which never leave the device.

It never changes the model: parameters, running statistics, optimizer state and dropout seeds are only read, no
row plan is built and ``model.training`` is left alone.  Graph mode pins the embedding module's kernel plan, as
the training steps do: parameters must not be re-homed (``.to()``, ``p.data = ...``) while a predictor lives.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional

import torch

from deepfm_amd import _lib
from deepfm_amd.data.packed import PackedColumns, RecordLayout
from deepfm_amd.data.schema import FeatureType
from deepfm_amd.training import fused_step
from deepfm_amd.training.step import GraphPair
from deepfm_amd.training.eligibility import (ineligible_reason, mixed_ineligible_reason, mixed_param_bytes,  # noqa: F401
                                             model_kind, record_gather_reason, released_table_reason)
from deepfm_amd.training.quantized import (FORMATS, QuantizedMixedTables, QuantizedTables,
                                           quantized_ineligible_reason, quantized_mixed_ineligible_reason)
from deepfm_amd.training.metrics import Evaluation, _check_ks, enqueue_evaluation, read_evaluations


class _Requests(NamedTuple):
    """One evaluation against the schema: ``what`` to compute (``training/metrics.py:Evaluation``) and its id columns as
    rows among the SPARSE fields (a record's id rows; None for a role that nothing asks for) with their ranges."""
    what: Evaluation
    user_row: Optional[int]
    num_users: int
    slice_row: Optional[int]
    num_slices: int
    unit_row: Optional[int]

    def rows(self) -> List[int]:              # the id rows to collect: each once, in the order user, slice, unit
        return list(dict.fromkeys(r for r in (self.user_row, self.slice_row, self.unit_row) if r is not None))


class FusedPredictor:
    """Eval-mode probabilities of a DeepFM / xDeepFM / AttentionDeepFM for batches of up to ``batch_size``
    samples.  Ineligible models raise ``ValueError`` naming the reason (keep ``model.predict`` for them).

    With a ``calibrator`` (``training/calibrator.py``) the forward ends in one more launch, inside the same graph: the
    head writes the raw logits and the calibrator's apply turns them into the probabilities that ``predict``,
    ``predict_from``, ``evaluate`` and ``evaluate_loader`` return and score; ``last_logits`` stays raw.  The apply
    reads the calibrator's parameters on the device, so a refit changes the next launch without a re-capture."""

    _ineligible = staticmethod(ineligible_reason)

    def __init__(self, model, batch_size: int, use_graph: bool = True, calibrator=None) -> None:
        reason = self._ineligible(model)
        if reason is not None:
            raise ValueError(f"{type(self).__name__}: {reason}")
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        emb = model.embedding
        p0 = next(model.parameters())
        _lib.require_device(p0, "model parameters")
        dev = p0.device
        self.model, self.B, self.emb, self.device = model, batch_size, emb, dev
        if calibrator is not None and calibrator.params.device != dev:
            raise ValueError(f"{type(self).__name__}: the calibrator is on {calibrator.params.device}, the model is "
                             f"on {dev}")
        self.calibrator = calibrator
        self.kind = model_kind(model)
        lib = _lib.load()
        B = batch_size
        self.layout = RecordLayout.of(model.schema, B)
        self.ns, self.nd, self.record_bytes = self.layout.n_sparse, self.layout.n_dense, self.layout.record_bytes
        f32 = dict(dtype=torch.float32, device=dev)
        self.st_labels = torch.zeros(B, **f32)      # the gather copies the record's labels here; never read
        self.inbox = torch.zeros(self.record_bytes, dtype=torch.uint8, device=dev)
        self._in_ids, self._in_dense, _, self._in_bags = self.layout.views(self.inbox)
        F, D = model.schema.num_fields, emb.fm_embed_dim
        self.fo = torch.empty(B, 1, **f32)
        self.fm = torch.empty(B, **f32) if self.kind != "xdeepfm" else None
        self._gather_buffers(F, D)
        self.logits = torch.empty(B, **f32)
        self.probs = torch.empty(B, **f32)
        self.raw_probs = torch.empty(B, **f32) if calibrator is not None else None     # the head's, never read
        dnn = model.dnn
        self.lin = [dnn.mlp[4 * i] for i in range(dnn._n_layers)]
        self.bn = [dnn.mlp[4 * i + 1] for i in range(dnn._n_layers)]
        self.a = [torch.empty(B, lin.out_features, **f32) for lin in self.lin]
        self.head = model.dnn_linear if self.kind == "xdeepfm" else model.output_linear
        if self.kind == "xdeepfm":
            cin = model.cin
            self.cin_L = len(cin.layer_sizes)
            self.cin_sizes = (C.c_int32 * self.cin_L)(*cin.layer_sizes)
            self.cin_split = 1 if cin.split_half else 0
            self.cin_out = torch.empty(B, cin.output_dim, **f32)
            self.cin_lin = torch.empty(B, 1, **f32)
            self.cin_saved = torch.empty(max(lib.dfm_cin_saved_bytes(self.cin_sizes, self.cin_L, self.cin_split,
                                                                     B, F, D) // 4, 1), **f32)
            self.cin_ws_f = torch.empty(max(lib.dfm_cin_forward_workspace_bytes(self.cin_sizes, self.cin_L,
                                                                                self.cin_split, F, D), 16),
                                        dtype=torch.uint8, device=dev)
            hd = model.cin_linear
            self.head1 = bool(lib.dfm_linear1_supported(hd.in_features)) and hd.out_features == 1
        elif self.kind == "attention":
            self.blocks = list(model.attention.layers)
        self.use_graph = use_graph
        self._pair: Optional[GraphPair] = None
        if use_graph:
            emb.pin_plan(dev)                 # captured graphs hold raw parameter pointers from here on
            self._capture()

    def _gather_buffers(self, F: int, D: int) -> None:
        """Where the gather writes the embeddings: ``fe`` (B, F, D) and the tower's input ``x0``."""
        B, lay = self.B, self.layout
        f32 = dict(dtype=torch.float32, device=self.device)
        # the staged gather refreshes these "static inputs" from the record it reads (its stage outputs); never read
        self.st_ids = torch.zeros(lay.id_rows, B, dtype=torch.int64, device=self.device)
        self.st_dense = torch.zeros(lay.dense_rows, B, **f32)
        ids, dense = iter(self.st_ids), iter(self.st_dense)
        self.stage: List[torch.Tensor] = [next(ids if k is FeatureType.SPARSE else dense) for k in lay.kinds]
        self.fe = torch.empty(B, F, D, **f32)
        # AttentionDeepFM's tower reads cat([attention(fe).flatten(1), flat])
        self.x0 = torch.empty(B, 2 * F * D, **f32) if self.kind == "attention" else self.fe.view(B, -1)

    # ------------------------------------------------------------------ the forward
    def _gather_call(self, record_ptr: int, labels_out: torch.Tensor):
        lay = self.layout
        return ([record_ptr + o for o in lay.field_offsets], self.stage, self.B, self.fo, self.fe), \
            dict(fm_out=self.fm, extra_src_ptr=record_ptr + lay.labels_offset, extra_dst=labels_out)

    def _head_args(self, valid: int, probs: torch.Tensor, logits: Optional[torch.Tensor]):
        last = self.a[-1]
        extra = self.cin_lin if self.kind == "xdeepfm" else self.fm
        if self.calibrator is not None:       # the head leaves the logits for the apply, which writes `probs`
            logits, probs = (logits if logits is not None else self.logits), self.raw_probs
        return (last.data_ptr(), self.B, last.shape[1], self.head.weight.data_ptr(), _lib.ptr(self.head.bias),
                self.fo.data_ptr(), extra.data_ptr(), valid, _lib.ptr(logits), probs.data_ptr())

    def _apply(self, valid: int, probs: torch.Tensor, logits: Optional[torch.Tensor],
               at: Optional[_lib.Launch] = None) -> None:
        src = logits if logits is not None else self.logits
        self.calibrator.apply_into(src.data_ptr(), valid, probs.data_ptr(), at)

    def _gather(self, record_ptr: int, labels_out: torch.Tensor, at: Optional[_lib.Launch] = None) -> None:
        a, kw = self._gather_call(record_ptr, labels_out)
        self.emb.forward_staged(*a, **kw, at=at)

    def _attention(self) -> None:
        fused_step.attention_forward(self.blocks, self.fe, self.x0)

    def _forward(self, record_ptr: int, valid: int, probs: torch.Tensor, logits: Optional[torch.Tensor],
                 labels_out: torch.Tensor, nodes: Optional[dict] = None) -> None:
        """``nodes`` (while capturing): takes the nodes ``_launch`` re-points — gather, head, the calibrator's apply."""
        lib, B = _lib.load(), self.B
        self._gather(record_ptr, labels_out)
        if nodes is not None:
            nodes["gather"] = _lib.last_node()
        if self.kind == "xdeepfm":
            fused_step.cin_forward(self, self.model)
        elif self.kind == "attention":
            self._attention()
        x = self.x0
        st = _lib.stream_handle()
        for lin, bn, out in zip(self.lin, self.bn, self.a):
            _lib.check(lib.dfm_linear_bn_eval(
                x.data_ptr(), x.shape[1], lin.weight.data_ptr(), _lib.ptr(lin.bias), B, lin.out_features,
                lin.in_features, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                bn.running_var.data_ptr(), float(bn.eps), out.data_ptr(), st))
            x = out
        _lib.check(lib.dfm_predict_head(*self._head_args(valid, probs, logits), _lib.stream_handle()))
        if nodes is not None:
            nodes["head"], nodes["apply"] = _lib.last_node(), None
        if self.calibrator is not None:
            self._apply(valid, probs, logits)
            if nodes is not None:
                nodes["apply"] = _lib.last_node()

    def _capture(self) -> None:
        # warm-up on the all-zero inbox (id 0 everywhere): writes the predictor's own buffers only
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._forward(self.inbox.data_ptr(), self.B, self.probs, self.logits, self.st_labels)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        def record() -> dict:
            nodes: dict = {}
            self._forward(self.inbox.data_ptr(), self.B, self.probs, self.logits, self.st_labels, nodes)
            return nodes
        self._pair = GraphPair(record, capture_error_mode="thread_local")

    @property
    def slots(self) -> list:
        """The two graph copies (``training/step.py:GraphPair``); empty in eager mode."""
        return self._pair.slots if self._pair is not None else []

    def _launch(self, record_ptr: int, valid: int, probs: torch.Tensor, logits: Optional[torch.Tensor],
                labels_out: torch.Tensor) -> None:
        if self._pair is None:
            self._forward(record_ptr, valid, probs, logits, labels_out)
            return
        slot = self._pair.next()
        self._gather(record_ptr, labels_out, slot.at["gather"])
        _lib.check(_lib.load().dfm_predict_head(*self._head_args(valid, probs, logits), slot.at["head"]))
        if self.calibrator is not None:
            self._apply(valid, probs, logits, slot.at["apply"])
        slot.graph.replay()
        slot.done.record()

    def _check_tables(self) -> None:
        reason = released_table_reason(self.model)
        if reason is not None:
            raise ValueError(f"{type(self).__name__}: {reason}")

    # ------------------------------------------------------------------ public
    def predict(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """``model.predict(batch)`` in eval mode: (n, 1) probabilities, n <= batch_size; SEQUENCE inputs (n, L)."""
        self._check_tables()
        inputs, n = self.emb._gather_inputs(batch)
        if not 0 < n <= self.B:
            raise ValueError(f"batch of {n} samples for a predictor of batch_size {self.B}")
        if n < self.B:
            self.inbox.zero_()
        kinds = self.layout.kinds
        ids = [x for x, k in zip(inputs, kinds) if k is FeatureType.SPARSE]
        dense = [x for x, k in zip(inputs, kinds) if k is FeatureType.DENSE]
        bags = [x for x, k in zip(inputs, kinds) if k is FeatureType.SEQUENCE]
        if ids:
            self._in_ids[:, :n].copy_(torch.stack(ids))
        if dense:
            self._in_dense[:, :n].copy_(torch.stack(dense))
        for blk, x in zip(self._in_bags, bags):
            blk[:n].copy_(x)
        return self._predict_record(self.inbox, n)

    def predict_from(self, record: torch.Tensor, valid: Optional[int] = None) -> torch.Tensor:
        """Probabilities of the first ``valid`` (default: all) samples of a batch record of this schema and
        batch size (``data/packed.py:RecordLayout``; a uniform schema's is the training record): (valid, 1)."""
        if record.numel() != self.record_bytes or record.dtype != torch.uint8 or not record.is_contiguous():
            raise ValueError("predict_from expects one contiguous batch record of this schema and batch size")
        if record.data_ptr() % 16:
            raise ValueError("batch records must be 16-byte aligned")
        _lib.require_device(record, "batch record")
        self._check_tables()
        n = self.B if valid is None else int(valid)
        if not 0 < n <= self.B:
            raise ValueError(f"valid = {n} outside [1, {self.B}]")
        return self._predict_record(record, n)

    def _predict_record(self, record: torch.Tensor, n: int) -> torch.Tensor:
        self._launch(record.data_ptr(), n, self.probs, self.logits, self.st_labels)
        if self.emb.strict_indices:
            self.emb.raise_on_bad_index()
        return self.probs[:n].clone().view(n, 1)

    def last_logits(self, n: Optional[int] = None) -> torch.Tensor:
        """Logits of the last ``predict`` / ``predict_from`` call, (n, 1) (a copy)."""
        n = self.B if n is None else n
        return self.logits[:n].clone().view(n, 1)

    def evaluate(self, columns: PackedColumns, ring: int = 4, ranking_ks: Optional[List[int]] = None,
                 user_field: str = "user_id", group_auc: bool = False, calibration_bins: Optional[int] = None,
                 slice_field: Optional[str] = None, bootstrap: int = 0, bootstrap_by: Optional[str] = None,
                 bootstrap_seed: int = 0, bootstrap_grouped: bool = False) -> Dict[str, float]:
        """AUC and log loss of the model on every sample of ``columns``, in order (reference Trainer.evaluate,
        trainer.py:244-294: ``auc`` is 0.0 for a single-class split).  One H2D copy per batch, the scores stay on
        the device, one host synchronisation at the end (besides waiting for a staging slot's earlier copy).

        With ``ranking_ks`` and a SPARSE field ``user_field`` in the schema, the dict also holds the reference's
        ``HR@k`` / ``NDCG@k`` (trainer.py:296-332: users with both classes, ``num_users`` the field's vocabulary
        size, ties in dataset order: ``training/metrics.py:ranking_metrics_device``) from the same device
        buffers; without such a field no ranking keys are added, as in the reference.  With ``group_auc`` and such a
        field it also holds ``gauc`` / ``uauc``, the AUC per user averaged over the users with both classes
        (``training/metrics.py:grouped_auc_device``), from the same buffers and the same host read.

        With ``calibration_bins`` it also holds the floats of ``training/metrics.py:calibration_dict`` (``mean_pred``,
        ``base_rate``, ``brier``, ``ece``, ``mce``, ``copc``, ``ne``) over that many equal-width bins, again from the
        same buffers and the same host read; the (bins, 3) table ``[count, positives, sum of predictions]`` stays on
        the device as ``self.last_calibration["bins"]``.  ``slice_field`` names a SPARSE field whose ids slice the
        samples (slice 0 is its OOV / padding row): ``self.last_calibration["slices"]`` is then the (vocabulary size,
        4) device table ``[count, positives, sum of predictions, sum of log loss]``.

        With ``bootstrap`` (replicates; 0: off) it also holds the spread of ``auc`` and ``logloss`` under that many
        Poisson-bootstrap replicates (``training/metrics.py:bootstrap_dict``: ``auc_se``, ``auc_lo``, ``auc_hi``,
        ``auc_replicates`` and the same for ``logloss``; 95 % percentile intervals), again from the same buffers and
        the same host read.  ``bootstrap_by`` names a SPARSE field whose ids are the resampling units (``"user_id"``:
        the candidates of one user are not independent samples); without it every sample is its own unit.
        ``bootstrap_seed`` fixes the resampling: two evaluations with one seed weigh every unit alike.

        With ``bootstrap_grouped`` the same replicates also resample the per-user metrics that were asked for: the dict
        then holds, behind the pooled bootstrap's keys and from the same host read, ``{m}_se``, ``{m}_lo``, ``{m}_hi``
        and ``{m}_replicates`` for ``m`` in ``HR@k``..., ``NDCG@k``..., ``gauc``, ``uauc``
        (``training/metrics.py:bootstrap_grouped_dict``).  It needs ``bootstrap`` > 0, ``bootstrap_by == user_field``
        (the users are the units of both bootstraps: one seed, one resampled population) and ``ranking_ks`` or
        ``group_auc``; ``ValueError`` names what is missing."""
        self._check_source(columns)
        self._check_tables()
        if len(columns) == 0:
            raise ValueError("no samples")
        req = self._requests(ranking_ks, user_field, group_auc, calibration_bins, slice_field, bootstrap, bootstrap_by,
                             bootstrap_seed, bootstrap_grouped)
        # the user column (and the slice and unit columns, when they are others) travels once, before the scoring loop
        ids = {row: torch.from_numpy(columns.ids[row]).to(self.device) for row in req.rows()}
        scores, labels, _ = self._score_columns(columns, ring)
        return self._finish_evaluation(scores, labels, len(columns), ids, req)

    def _score(self, records, scores: torch.Tensor, logits: Optional[torch.Tensor] = None,
               labels: Optional[torch.Tensor] = None) -> None:
        """The one scoring loop: a launch per ``(record address, valid count)`` of ``records``, batch k into ``scores[k
        * B:]`` (``logits``, ``labels`` alike).  A generator forms each record just ahead of its launch."""
        B, launch, unread = self.B, self._launch, self.st_labels
        for k, (ptr, cnt) in enumerate(records):
            s = k * B
            launch(ptr, cnt, scores[s:], None if logits is None else logits[s:], unread if labels is None else labels[s:])

    def _score_buffers(self, n: int, want_logits: bool):
        nb = (n + self.B - 1) // self.B          # (batches, scores, labels, logits or None) of whole batches, float32
        scores, labels, logits = (torch.empty(nb * self.B, dtype=torch.float32, device=self.device) if want else None
                                  for want in (True, True, want_logits))
        return nb, scores, labels, logits

    def _score_columns(self, columns: PackedColumns, ring: int = 4, want_logits: bool = False):
        """The scoring of ``evaluate``: (scores, labels, logits or None) device buffers of whole batches, the samples of
        ``columns`` in order in front, each record written on the host into a pinned ring and copied once."""
        n, B, dev = len(columns), self.B, self.device
        nb, scores, labels, logits = self._score_buffers(n, want_logits)
        stride = (self.record_bytes + 255) // 256 * 256
        depth = max(2, min(ring, nb))
        host = torch.empty(depth, stride, dtype=torch.uint8).pin_memory()
        host_np = [host[i].numpy() for i in range(depth)]
        dev_rec = torch.empty(depth, stride, dtype=torch.uint8, device=dev)
        copied: List[Optional[torch.cuda.Event]] = [None] * depth

        def records():
            for k in range(nb):
                j = k % depth
                if copied[j] is not None:
                    copied[j].synchronize()           # the slot's previous H2D copy has read it
                s, e = k * B, min(n, (k + 1) * B)
                self.layout.write(host_np[j], columns, s, e)
                dev_rec[j].copy_(host[j], non_blocking=True)
                if copied[j] is None:
                    copied[j] = torch.cuda.Event()
                copied[j].record()
                yield dev_rec[j].data_ptr(), e - s
        self._score(records(), scores, logits, labels)
        return scores, labels, logits

    def _score_loader(self, loader, rows=(), want_logits: bool = False):
        """The scoring of ``evaluate_loader``: (scores, labels, {row: ids of that SPARSE row}, logits) device buffers,
        the records assembled on the device (``rows_into_next``)."""
        n, B = loader.rows, self.B
        nb, scores, labels, logits = self._score_buffers(n, want_logits)
        ids = {row: torch.empty(nb * B, dtype=torch.int64, device=self.device) for row in rows}

        def records():
            for s in range(0, n, B):
                rec = loader.rows_into_next(s, min(B, n - s))
                yield rec.data_ptr(), min(B, n - s)
                for row, col in ids.items():          # behind the launch, as the record's next use
                    col[s:s + B].copy_(rec[8 * B * row:8 * B * (row + 1)].view(torch.int64))
        self._score(records(), scores, logits, labels)
        return scores, labels, ids, logits

    def _check_source(self, source) -> bool:
        """True for a ``DeviceEpochLoader``, False for ``PackedColumns``; ``ValueError`` for another schema or batch."""
        is_loader = hasattr(source, "rows_into_next")
        schema = source.columns.schema if is_loader else source.schema
        if schema is not self.model.schema and list(schema.fields) != list(self.model.schema.fields):
            raise ValueError("a loader of another schema" if is_loader else "columns of another schema")
        if is_loader and source.batch_size != self.B:
            raise ValueError(f"a loader of batch_size {source.batch_size} for a predictor of batch_size {self.B}")
        return is_loader

    def collect_logits(self, source, ring: int = 4):
        """(labels, logits): float32 device vectors of every sample of ``source`` (``PackedColumns``, or a
        ``DeviceEpochLoader`` in its current order), from the scoring loop of ``evaluate`` / ``evaluate_loader``; the
        logits are raw whether or not the predictor has a calibrator.  What ``Calibrator.fit`` takes; no host
        synchronisation besides the staging slots' of ``evaluate``."""
        is_loader = self._check_source(source)
        self._check_tables()
        n = source.rows if is_loader else len(source)
        if n == 0:
            raise ValueError("no samples")
        if is_loader:
            _, labels, _, logits = self._score_loader(source, want_logits=True)
        else:
            _, labels, logits = self._score_columns(source, ring, want_logits=True)
        if self.emb.strict_indices:
            self.emb.raise_on_bad_index()
        return labels[:n], logits[:n]

    def _sparse_field(self, name: str, role: str):
        """(row of the field ``name`` among the SPARSE fields, i.e. the order of a record's id rows, its vocabulary
        size); ``ValueError`` when the schema has no such SPARSE field (``role``: the keyword that named it)."""
        sparse = [nm for nm, sp in self.model.schema.fields.items() if sp.feature_type is FeatureType.SPARSE]
        if name not in sparse:
            raise ValueError(f"{role} {name!r} is not a SPARSE field of the schema")
        return sparse.index(name), self.model.schema.fields[name].vocabulary_size

    def _ranking_setup(self, ranking_ks, user_field: str, group_auc: bool = False):
        """(ks or None, row of ``user_field`` or None, num_users): the ranking metrics and the grouped AUC need it."""
        ks = None if ranking_ks is None else _check_ks(ranking_ks)
        if ks is None and not group_auc:
            return None, None, 0
        try:
            return (ks, *self._sparse_field(user_field, "user_field"))
        except ValueError:                    # as in the reference: without such a field, no ranking keys
            return ks, None, 0

    def _requests(self, ranking_ks, user_field, group_auc, calibration_bins, slice_field, bootstrap, bootstrap_by,
                  bootstrap_seed, bootstrap_grouped: bool = False) -> _Requests:
        """The keywords of ``evaluate`` / ``evaluate_loader`` checked against the schema, as one value."""
        ks, user_row, num_users = self._ranking_setup(ranking_ks, user_field, group_auc)
        bins = None if calibration_bins is None else int(calibration_bins)
        if bins is not None and not 1 <= bins <= 1024:
            raise ValueError(f"calibration_bins = {calibration_bins}: between 1 and 1024 bins are supported")
        if slice_field is not None and bins is None:
            raise ValueError("slice_field slices the calibration numbers: it needs calibration_bins")
        slice_row, num_slices = (None, 0) if slice_field is None else self._sparse_field(slice_field, "slice_field")
        if not 0 <= int(bootstrap) <= _lib.BOOTSTRAP_MAX_REPLICATES:
            raise ValueError(f"bootstrap = {bootstrap}: between 0 (off) and {_lib.BOOTSTRAP_MAX_REPLICATES} replicates "
                             "are supported")
        if bootstrap_by is not None and not int(bootstrap):
            raise ValueError("bootstrap_by names the units of the bootstrap: it needs bootstrap")
        unit_row = None if bootstrap_by is None else self._sparse_field(bootstrap_by, "bootstrap_by")[0]
        if bootstrap_grouped:
            if not int(bootstrap):
                raise ValueError("bootstrap_grouped resamples the per-user metrics: it needs bootstrap (replicates > 0)")
            if bootstrap_by != user_field:
                raise ValueError(f"bootstrap_grouped resamples whole users: it needs bootstrap_by == user_field "
                                 f"({user_field!r}), got bootstrap_by = {bootstrap_by!r}")
            if ks is None and not group_auc:
                raise ValueError("bootstrap_grouped has no per-user metric to resample: it needs ranking_ks or "
                                 "group_auc")
        what = Evaluation(ks, bool(group_auc), bins, int(bootstrap), bootstrap_seed, bool(bootstrap_grouped))
        return _Requests(what, user_row, num_users, slice_row, num_slices, unit_row)

    def _finish_evaluation(self, scores, labels, n: int, ids, req: _Requests) -> Dict[str, float]:
        """The metrics of the first ``n`` scored samples (``ids``: {row: id column}): every family that ``req.what``
        asks for is enqueued on the device, then one host read (``training/metrics.py:enqueue_evaluation``)."""
        y, s = labels[:n], scores[:n]
        uid, sid, bid = (None if row is None else ids[row][:n] for row in (req.user_row, req.slice_row, req.unit_row))
        enqueued = enqueue_evaluation(req.what, y, s, uid, req.num_users, sid, req.num_slices or None, bid)
        if self.emb.strict_indices:
            self.emb.raise_on_bad_index()
        result, = read_evaluations([enqueued])
        self.last_scores, self.last_labels = s, y
        if enqueued[2] is not None:            # the calibration's tables: visible once its numbers are accepted
            self.last_calibration = enqueued[2]
        return result

    def evaluate_loader(self, loader, ranking_ks: Optional[List[int]] = None, user_field: str = "user_id",
                        group_auc: bool = False, calibration_bins: Optional[int] = None,
                        slice_field: Optional[str] = None, bootstrap: int = 0, bootstrap_by: Optional[str] = None,
                        bootstrap_seed: int = 0, bootstrap_grouped: bool = False) -> Dict[str, float]:
        """``evaluate`` over the rows of a ``DeviceEpochLoader`` (``data/device_epoch.py``; any candidate source) in
        the loader's current order, the trailing partial batch included: the same dict, with no host-built row and
        no host-to-device copy.  One ``dfm_record_assemble`` and one forward launch per batch; the labels and the
        user ids are read from the records that were scored, on the device.  ``shuffle`` may be on: AUC and log loss
        do not depend on the order, the ranking metrics group by user (ties keep the loader's order) and the grouped AUC
        of ``group_auc`` and the calibration numbers of ``calibration_bins`` / ``slice_field`` do not depend on it
        either; the slice ids are read from the scored records as the user ids are, and so are the resampling units
        of ``bootstrap`` / ``bootstrap_by`` (``evaluate``); resampled by such a field the intervals do not depend on the
        order either, resampled by sample the unit is the position in the loader's order.  ``bootstrap_grouped``: as
        in ``evaluate``."""
        self._check_source(loader)
        self._check_tables()
        req = self._requests(ranking_ks, user_field, group_auc, calibration_bins, slice_field, bootstrap, bootstrap_by,
                             bootstrap_seed, bootstrap_grouped)
        scores, labels, ids, _ = self._score_loader(loader, req.rows())
        return self._finish_evaluation(scores, labels, loader.rows, ids, req)

    def field_importance(self, source, **kw):
        """Permutation importance of the schema's fields on ``source`` (``PackedColumns``, a ``DeviceEpochLoader`` or a
        ``RecordSet``): ``training/importance.py:FieldImportance(self).run(source, **kw)``, an ``ImportanceReport``."""
        from deepfm_amd.training.importance import FieldImportance
        return FieldImportance(self).run(source, **kw)


class MixedSchemaPredictor(FusedPredictor):
    """``FusedPredictor`` for any schema of SPARSE, SEQUENCE and DENSE fields, projections and mixed widths
    (MovieLens: a ``genres`` bag, widths 4 / 8 / 16, six DENSE fields).  One record gather per batch
    (``dfm_embedding_forward_record``) writes first_order, the FM value (DeepFM, AttentionDeepFM), fe (xDeepFM,
    AttentionDeepFM) and flat_embeddings straight into the tower's input; the interaction layer, the tower and the
    head are ``FusedPredictor``'s.  Records are in ``data/packed.py:mixed_record_layout``; SEQUENCE inputs are
    (n, max_length) ids, 0-padded.  Ineligible models raise ``ValueError`` naming the reason."""

    _ineligible = staticmethod(mixed_ineligible_reason)

    def _gather_buffers(self, F: int, D: int) -> None:
        """The record gather writes flat_embeddings straight into the tower's input: ``x0`` is (B, T), or
        (B, F*D + T) with the attention blocks' output in front; DeepFM's tower reads flat only, so no ``fe``."""
        B = self.B
        f32 = dict(dtype=torch.float32, device=self.device)
        T = sum(s.embedding_dim for s in self.model.schema.fields.values())
        self.fe = torch.empty(B, F, D, **f32) if self.kind != "deepfm" else None
        front = F * D if self.kind == "attention" else 0
        self.x0 = torch.empty(B, front + T, **f32)
        self._flat_ptr, self._ld = self.x0.data_ptr() + 4 * front, front + T

    def _gather(self, record_ptr: int, labels_out: torch.Tensor, at: Optional[_lib.Launch] = None) -> None:
        self.emb.forward_record(record_ptr, self.B, self.fo, self.fe, self._flat_ptr, self._ld, self.fm, labels_out,
                                at=at)

    def _attention(self) -> None:
        # the gather has written flat into x0[:, F*D:]; the blocks fill x0[:, :F*D]
        fused_step.attention_forward(self.blocks, self.fe, self.x0, ld=self._ld, copy_fe=False)


class QuantizedPredictor(FusedPredictor):
    """``FusedPredictor`` whose SPARSE fields are served from ``QuantizedTables`` (``tables=None``: built from the model
    here in the format ``fmt``, ``"int8"`` or ``"uint4"``; given tables serve in their own format, whatever ``fmt``
    says).  Only the gather differs: the interaction layer, the tower, the head, the two alternating graphs, their
    re-pointing, ``predict`` / ``predict_from`` / ``last_logits`` / ``evaluate`` and the strict-index check are
    ``FusedPredictor``'s.  After construction the fp32 SPARSE tables are never read (only the DENSE-field Linears, the
    tower, the CIN / attention and the head are); ``tables.refresh()`` requantises them into the same buffers, which
    live graphs keep reading.  Ineligible models raise ``ValueError`` naming the reason."""

    _ineligible = staticmethod(quantized_ineligible_reason)

    def __init__(self, model, batch_size: int, tables: Optional[QuantizedTables] = None, use_graph: bool = True,
                 calibrator=None, fmt: str = "int8") -> None:
        reason = self._ineligible(model)
        if reason is not None:
            raise ValueError(f"{type(self).__name__}: {reason}")
        if tables is None:
            tables = QuantizedTables.from_model(model, fmt)
        reason = tables.matches(model)
        if reason is not None:
            raise ValueError(f"{type(self).__name__}: {reason}")
        if tables.device != next(model.parameters()).device:
            raise ValueError(f"{type(self).__name__}: the tables are on {tables.device}, the model is on "
                             f"{next(model.parameters()).device} (QuantizedTables.to)")
        self.tables = tables
        super().__init__(model, batch_size, use_graph, calibrator)

    def _gather_buffers(self, F: int, D: int) -> None:
        """``fe`` (B, F, D) and the tower's input ``x0`` as ``FusedPredictor``'s, without stage outputs; the gather's
        field table is built once: record and parameter addresses do not change while the predictor lives."""
        B = self.B
        f32 = dict(dtype=torch.float32, device=self.device)
        self.fe = torch.empty(B, F, D, **f32)
        self.x0 = torch.empty(B, 2 * F * D, **f32) if self.kind == "attention" else self.fe.view(B, -1)
        self.emb._ensure_plan(self.device)          # the module's error flag lives with its plan
        self._qfields = self._quant_fields()

    def _quant_fields(self):
        emb = self.emb
        arr = (_lib.QuantField * len(emb.field_names))()
        for i, name in enumerate(emb.field_names):
            spec, fd = self.model.schema.fields[name], arr[i]
            if spec.feature_type is FeatureType.SPARSE:
                fd.kind, fd.vocab, fd.rows = _lib.SPARSE, spec.vocabulary_size, self.tables.records[name].data_ptr()
            else:
                second, first = emb.second_order_embeddings[name], emb.first_order_embeddings[name]
                fd.kind, fd.vocab = _lib.DENSE, 0
                fd.w2, fd.b2 = second.weight.data_ptr(), second.bias.data_ptr()
                fd.w1, fd.b1 = first.weight.data_ptr(), first.bias.data_ptr()
        return arr

    def _gather(self, record_ptr: int, labels_out: torch.Tensor, at: Optional[_lib.Launch] = None) -> None:
        lay = self.layout
        if not self.use_graph:
            self._qfields = self._quant_fields()    # eager mode follows re-homed DENSE parameters, as the plan does
        inputs = (C.c_void_p * len(lay.field_offsets))(*[record_ptr + o for o in lay.field_offsets])
        _lib.check(_lib.load().dfm_embedding_forward_quant(
            self._qfields, len(lay.field_offsets), self.emb.fm_embed_dim, FORMATS[self.tables.format], inputs,
            record_ptr + lay.labels_offset, labels_out.data_ptr(), self.B, self.fo.data_ptr(), self.fe.data_ptr(),
            _lib.ptr(self.fm), None, self.emb._err.data_ptr(), at or _lib.stream_handle()))


class QuantizedMixedPredictor(MixedSchemaPredictor):
    """``MixedSchemaPredictor`` whose SPARSE and SEQUENCE fields of width 16, 32 or 64 (``fields``: that subset) are
    served from ``QuantizedMixedTables`` (``tables=None``: built from the model here in the format ``fmt``; given
    tables serve in their own format, whatever ``fmt`` says).  Only the gather differs
    (``dfm_embedding_forward_record_quant``: one record per id, a bag pooled in one walk); narrower fields, DENSE
    fields and the projections are read in fp32 as before, and everything else is ``MixedSchemaPredictor``'s.  After
    construction the fp32 tables of the quantised fields are never read; ``tables.refresh()`` requantises them into
    the same buffers, which live graphs keep reading.  Ineligible models raise ``ValueError`` naming the reason."""

    _ineligible = staticmethod(quantized_mixed_ineligible_reason)

    def __init__(self, model, batch_size: int, tables: Optional[QuantizedMixedTables] = None, use_graph: bool = True,
                 calibrator=None, fmt: str = "int8", fields=None) -> None:
        reason = self._ineligible(model)
        if reason is not None:
            raise ValueError(f"{type(self).__name__}: {reason}")
        if tables is None:
            tables = QuantizedMixedTables.from_model(model, fmt, fields)
        reason = tables.matches(model)
        if reason is not None:
            raise ValueError(f"{type(self).__name__}: {reason}")
        if tables.device != next(model.parameters()).device:
            raise ValueError(f"{type(self).__name__}: the tables are on {tables.device}, the model is on "
                             f"{next(model.parameters()).device} (QuantizedMixedTables.to)")
        self.tables = tables
        self._qrows = self._quant_rows(model.embedding)
        super().__init__(model, batch_size, use_graph, calibrator)

    def _quant_rows(self, emb):
        """The gather's table of record bases, schema order; None where the field is read in fp32."""
        recs = self.tables.records
        return (C.c_void_p * len(emb.field_names))(*[recs[n].data_ptr() if n in recs else None
                                                     for n in emb.field_names])

    def _gather(self, record_ptr: int, labels_out: torch.Tensor, at: Optional[_lib.Launch] = None) -> None:
        if not self.use_graph:
            self._qrows = self._quant_rows(self.emb)      # as QuantizedPredictor's field table in eager mode
        self.emb.forward_record_quant(self._qrows, FORMATS[self.tables.format], record_ptr, self.B, self.fo, self.fe,
                                      self._flat_ptr, self._ld, self.fm, labels_out, at=at)
