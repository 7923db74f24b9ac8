"""Permutation field importance on the device, for every fused predictor (DESIGN.md §7d "Field importance").

Shuffle one field, or one group of fields, across the evaluation set, score again and report how much every metric
degrades.  The evaluation set stays on the device as whole batch records (``RecordSet``); per repeat one launch writes
the sort keys of a permutation (``dfm_permutation_keys``) and one ``torch.sort`` orders them; per (group, repeat) and
batch one launch forms the shuffled record (``dfm_records_permute``, ``csrc/importance.hip``) in a small ring of scratch
records and the predictor's ordinary launch scores it on the same stream.  The metrics of every variant are enqueued on
the original labels and ids (``training/metrics.py``) and all of them come back in one host read.

The permutation depends on ``(seed, repeat)`` only, never on the field or group: every group of a repeat is shuffled by
the same permutation (common random numbers), so differences between groups are paired and
``delta(a + b) - delta(a) - delta(b)`` means something (``ImportanceReport.interaction``).

Permutation breaks the correlation between the shuffled fields and the others: the importance of correlated fields is
shared out among them arbitrarily, and a shuffled record may be one the data could never hold.

``RecordSet``          the evaluation set as device batch records, from ``PackedColumns`` or a ``DeviceEpochLoader``;
``FieldImportance``    the loop; ``FusedPredictor.field_importance`` builds and runs one;
``ImportanceReport``   baseline, values under permutation, deltas, their mean and standard error over the repeats,
                       rankings, interactions and a JSON-serialisable dict.
Nothing here needs the GPU at import time; the host-side checks run without one.
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from deepfm_amd import _lib
from deepfm_amd.data.packed import PackedColumns, RecordLayout
from deepfm_amd.data.schema import FeatureType
from deepfm_amd.training.metrics import Evaluation, _check_ks, enqueue_evaluation, read_evaluations

SET_MAX_BYTES = 2 << 30
_KIND = {FeatureType.SPARSE: _lib.SPARSE, FeatureType.DENSE: _lib.DENSE, FeatureType.SEQUENCE: _lib.SEQUENCE}


def check_request(names: Sequence[str], fields=None, groups=None, repeats: int = 5) -> List[Tuple[str, Tuple[str, ...], int]]:
    """The groups of a run as ``[(label, field names, mask)]``: every name of ``fields`` (default: every field of the
    schema, ``names``) as its own group, then the ``groups`` ``{label: [field names]}``; ``mask`` has bit f set for
    field f of the schema.  ``ValueError`` for a name missing from the schema, an empty group or field list, a
    duplicate label or ``repeats`` outside [1, 2^24).  Host only."""
    names = list(names)
    if len(names) > _lib.MAX_FIELDS:
        raise ValueError(f"a schema of {len(names)} fields: at most {_lib.MAX_FIELDS} are supported")
    if isinstance(repeats, bool) or int(repeats) != repeats or not 1 <= int(repeats) < _lib.PERMUTATION_MAX_REPEATS:
        raise ValueError(f"repeats = {repeats!r}: an integer in [1, 2^24) is needed")
    index = {name: f for f, name in enumerate(names)}
    singles = names if fields is None else list(fields)
    if isinstance(fields, str):
        raise ValueError("fields is a list of field names, not one name")
    plan: List[Tuple[str, Tuple[str, ...], int]] = []
    seen = set()

    def add(label, members) -> None:
        members = tuple(members)
        if not members:
            raise ValueError(f"group {label!r} is empty")
        if label in seen:
            raise ValueError(f"duplicate label {label!r}")
        mask = 0
        for name in members:
            if name not in index:
                raise ValueError(f"{name!r} is not a field of the schema")
            mask |= 1 << index[name]
        seen.add(label)
        plan.append((label, members, mask))

    for name in singles:
        add(name, (name,))
    for label, members in (groups or {}).items():
        if isinstance(members, str):
            raise ValueError(f"group {label!r}: a list of field names is needed, not one name")
        add(label, members)
    if not plan:
        raise ValueError("no field and no group to permute")
    return plan


class ImportanceReport:
    """What a run measured.  ``groups`` the labels, ``members`` ``{label: field names}``, ``metrics`` the metric names
    in ``evaluate``'s spelling (``auc``, ``logloss``, then ``HR@k`` / ``NDCG@k`` per k, ``gauc``, ``uauc`` as
    requested), ``baseline`` (M,) float64, ``values`` (G, R, M) the metric under permutation, ``delta`` = values -
    baseline.  A ranking or grouped metric that no user qualifies for is NaN."""

    def __init__(self, groups: Sequence[str], metrics: Sequence[str], baseline, values,
                 members: Optional[Dict[str, Sequence[str]]] = None, seed: int = 0, n: int = 0) -> None:
        self.groups, self.metrics = list(groups), list(metrics)
        self.baseline = np.asarray(baseline, np.float64).reshape(len(self.metrics))
        self.values = np.asarray(values, np.float64)
        if self.values.ndim != 3 or self.values.shape[0] != len(self.groups) or self.values.shape[2] != len(self.metrics):
            raise ValueError(f"values of shape {self.values.shape} for {len(self.groups)} groups and "
                             f"{len(self.metrics)} metrics: (G, R, M) is needed")
        if len(set(self.groups)) != len(self.groups):
            raise ValueError("duplicate label")
        self.members = {g: tuple((members or {}).get(g, (g,))) for g in self.groups}
        self.delta = self.values - self.baseline
        self.repeats, self.seed, self.n = self.values.shape[1], int(seed), int(n)

    def _metric(self, metric: str) -> int:
        if metric not in self.metrics:
            raise KeyError(f"metric {metric!r} was not computed (have {self.metrics})")
        return self.metrics.index(metric)

    def _group(self, label: str) -> int:
        if label not in self.groups:
            raise KeyError(f"group {label!r} was not run")
        return self.groups.index(label)

    def mean(self) -> np.ndarray:
        """(G, M): the mean delta over the repeats."""
        return self.delta.mean(axis=1)

    def se(self) -> np.ndarray:
        """(G, M): the standard error of the mean delta over the repeats (ddof 1); NaN for one repeat."""
        R = self.repeats
        if R < 2:
            return np.full(self.delta.shape[::2], np.nan)
        return self.delta.std(axis=1, ddof=1) / math.sqrt(R)

    def ranking(self, metric: str = "logloss") -> List[str]:
        """The labels from most to least harmful under permutation: harm is the mean rise of ``logloss``, the mean drop
        of any other metric.  Ties keep the order of ``groups`` (schema order); a NaN harm goes last."""
        m = self._metric(metric)
        harm = self.mean()[:, m] * (1.0 if metric == "logloss" else -1.0)
        key = np.where(np.isnan(harm), -np.inf, harm)
        return [self.groups[g] for g in np.argsort(-key, kind="stable")]

    def interaction(self, a: str, b: str, metric: str = "logloss", per_repeat: bool = False):
        """``delta(a + b) - delta(a) - delta(b)`` for ``metric``, paired by repeat (one permutation per repeat for all
        three) and averaged over the repeats ((R,) with ``per_repeat``).  The group of the union is found by its
        fields, whatever its label; ``KeyError`` names whichever of the three was not run."""
        m = self._metric(metric)
        ga, gb = self._group(a), self._group(b)
        union = set(self.members[a]) | set(self.members[b])
        both = [g for g, label in enumerate(self.groups) if set(self.members[label]) == union]
        if not both:
            raise KeyError(f"no group of the fields {sorted(union)} ({a!r} + {b!r}) was run")
        d = self.delta[both[0], :, m] - self.delta[ga, :, m] - self.delta[gb, :, m]
        return d if per_repeat else float(d.mean())

    def to_dict(self) -> Dict:
        """JSON-serialisable, without NaN (None instead: the ``se`` of a single repeat, an undefined metric)."""
        def num(x):
            x = float(x)
            return None if math.isnan(x) else x
        mean, se = self.mean(), self.se()
        return {
            "n": self.n, "repeats": self.repeats, "seed": self.seed, "metrics": list(self.metrics),
            "groups": {g: list(self.members[g]) for g in self.groups},
            "baseline": {name: num(self.baseline[m]) for m, name in enumerate(self.metrics)},
            "importance": {g: {name: {"mean": num(mean[i, m]), "se": num(se[i, m]),
                                      "delta": [num(v) for v in self.delta[i, :, m]]}
                               for m, name in enumerate(self.metrics)} for i, g in enumerate(self.groups)},
        }

    def __eq__(self, other) -> bool:
        return (isinstance(other, ImportanceReport) and self.groups == other.groups and self.metrics == other.metrics
                and self.members == other.members and np.array_equal(self.baseline, other.baseline, equal_nan=True)
                and np.array_equal(self.values, other.values, equal_nan=True))

    __hash__ = None


def _set_bytes(n: int, layout: RecordLayout, max_bytes: int) -> Tuple[int, int]:
    """(records, stride) of a set of ``n`` samples; ``ValueError`` when it is empty or takes more than ``max_bytes``."""
    if n < 1:
        raise ValueError("no samples")
    if n > _lib.PERMUTATION_MAX_N:
        raise ValueError(f"{n} samples: the permutation takes fewer than 2^31")
    nb = (n + layout.batch_size - 1) // layout.batch_size
    stride = (layout.record_bytes + 255) // 256 * 256          # records stay 256-byte aligned
    if nb * stride > max_bytes:
        raise ValueError(f"a record set of {n} samples takes {nb * stride} bytes ({nb} records of {stride}), more than "
                         f"max_bytes = {max_bytes}")
    return nb, stride


class RecordSet:
    """An evaluation set on the device as ``ceil(n / B)`` whole batch records in the predictor's ``RecordLayout``,
    ``stride`` bytes apart: sample g is slot ``g % B`` of record ``g // B``; the slots behind the last sample are
    ``RecordLayout.write``'s padding.  ``labels`` and ``ids(name)`` are read from these records: the grouping ids of a
    run always come from the unpermuted set."""

    def __init__(self, layout: RecordLayout, n: int, records: torch.Tensor) -> None:
        self.layout, self.n, self.records = layout, n, records
        self.stride = records.shape[1]

    def __len__(self) -> int:
        return self.n

    @classmethod
    def from_columns(cls, predictor, columns: PackedColumns, max_bytes: int = SET_MAX_BYTES) -> "RecordSet":
        """Every sample of ``columns`` in order: written on the host (``RecordLayout.write``), every record uploaded
        once."""
        if predictor._check_source(columns):
            raise TypeError("from_columns takes PackedColumns (from_loader takes a loader)")
        lay = predictor.layout
        n, B = len(columns), lay.batch_size
        nb, stride = _set_bytes(n, lay, max_bytes)
        host = torch.zeros(nb, stride, dtype=torch.uint8)
        host_np = host.numpy()
        for k in range(nb):
            lay.write(host_np[k][:lay.record_bytes], columns, k * B, min(n, (k + 1) * B))
        return cls(lay, n, host.to(predictor.device))

    @classmethod
    def from_loader(cls, predictor, loader, max_bytes: int = SET_MAX_BYTES) -> "RecordSet":
        """The rows of a ``DeviceEpochLoader`` in its current order, the candidate rows of its source included: one
        ``rows_into_next`` per batch, copied into the set on the device."""
        if not predictor._check_source(loader):
            raise TypeError("from_loader takes a DeviceEpochLoader (from_columns takes PackedColumns)")
        lay = predictor.layout
        n, B = loader.rows, lay.batch_size
        nb, stride = _set_bytes(n, lay, max_bytes)
        records = torch.zeros(nb, stride, dtype=torch.uint8, device=predictor.device)
        for k in range(nb):
            rec = loader.rows_into_next(k * B, min(B, n - k * B))
            records[k, :lay.record_bytes].copy_(rec)
        return cls(lay, n, records)

    @property
    def labels(self) -> torch.Tensor:
        """(n,) float32 device vector."""
        lay = self.layout
        block = self.records[:, lay.labels_offset:lay.labels_offset + 4 * lay.batch_size].contiguous()
        return block.view(torch.float32).reshape(-1)[:self.n]

    def ids(self, name: str) -> torch.Tensor:
        """(n,) int64 device vector: the id column of the SPARSE field ``name``."""
        lay = self.layout
        if name not in lay.names or lay.kinds[lay.names.index(name)] is not FeatureType.SPARSE:
            raise ValueError(f"{name!r} is not a SPARSE field of the schema")
        off = lay.field_offsets[lay.names.index(name)]
        block = self.records[:, off:off + 8 * lay.batch_size].contiguous()
        return block.view(torch.int64).reshape(-1)[:self.n]


def record_fields(layout: RecordLayout):
    """``layout`` as the ``dfm_record_field`` array of ``dfm_records_permute``."""
    arr = (_lib.RecordField * len(layout.names))()
    lengths = iter(layout.seq_lengths)
    for fd, kind, off in zip(arr, layout.kinds, layout.field_offsets):
        fd.kind, fd.offset = _KIND[kind], off
        fd.max_length = next(lengths) if kind is FeatureType.SEQUENCE else 1
    return arr


def permutation_keys(seed: int, repeat: int, n: int, device) -> torch.Tensor:
    """Enqueue the (n,) int64 sort keys of the permutation of ``(seed, repeat)`` (``dfm_permutation_keys``)."""
    keys = torch.empty(n, dtype=torch.int64, device=device)
    _lib.check(_lib.load().dfm_permutation_keys(int(seed) & 0xFFFFFFFFFFFFFFFF, repeat, n, keys.data_ptr(),
                                                _lib.stream_handle()))
    return keys


def permute_into(rs: RecordSet, fields, sorted_keys: Optional[torch.Tensor], mask: int, first: int, count: int,
                 out: torch.Tensor) -> None:
    """One launch: the record of samples ``[first, first + count)`` of ``rs`` with the fields of ``mask`` taken through
    the permutation of ``sorted_keys``, into the device record ``out`` (``dfm_records_permute``)."""
    lay = rs.layout
    if out.dtype != torch.uint8 or out.numel() < lay.record_bytes or not out.is_contiguous():
        raise ValueError("permute_into expects one contiguous batch record of this schema and batch size")
    _lib.require_device(out, "batch record")
    _lib.check(_lib.load().dfm_records_permute(
        rs.records.data_ptr(), rs.stride, fields, len(lay.names), lay.batch_size, lay.labels_offset, lay.record_bytes,
        rs.n, _lib.ptr(sorted_keys), mask, first, count, out.data_ptr(), _lib.stream_handle()))


class FieldImportance:
    """Permutation importance of the fields of ``predictor``'s schema (module docstring): a ``FusedPredictor``, a
    ``MixedSchemaPredictor`` or a ``QuantizedPredictor``; one with a calibrator is scored on its calibrated
    probabilities, as ``evaluate`` is.  The predictor's parameters, calibrator, ``last_scores`` and buffers that
    outlive a launch are only read."""

    def __init__(self, predictor, ring: int = 4) -> None:
        if ring < 2:
            raise ValueError("ring must be at least 2")
        self.predictor, self.ring = predictor, ring
        self.scores: Optional[torch.Tensor] = None       # with keep_scores: (1 + G * R, n), the baseline in front

    def run(self, source, fields=None, groups=None, repeats: int = 5, seed: int = 0,
            ranking_ks: Optional[List[int]] = None, user_field: str = "user_id", group_auc: bool = False,
            keep_scores: bool = False, max_bytes: int = SET_MAX_BYTES) -> ImportanceReport:
        """The report of ``source`` (``PackedColumns``, a ``DeviceEpochLoader`` in its current order, or a
        ``RecordSet``).  ``fields``: names, each its own group (default: every field of the schema); ``groups``:
        ``{label: [field names]}``, permuted jointly, added behind them.  ``ranking_ks`` / ``group_auc`` add ``HR@k`` /
        ``NDCG@k`` and ``gauc`` / ``uauc`` grouped by the SPARSE field ``user_field`` as ``evaluate`` does (without
        such a field neither is added); the grouping ids are the unpermuted ones also when that field is shuffled.
        ``keep_scores`` keeps every variant's score vector in ``self.scores``.

        Nothing is read on the host until every variant is enqueued; then all metric vectors come back in one read.
        A variant with NaN scores raises ``ValueError`` as ``evaluate`` does."""
        pred = self.predictor
        plan = check_request(list(pred.model.schema.fields), fields, groups, repeats)     # host only, before the device
        ks = None if ranking_ks is None else _check_ks(ranking_ks)
        repeats = int(repeats)
        ks, user_row, num_users = pred._ranking_setup(ks, user_field, group_auc)
        if isinstance(source, RecordSet):
            rs = source
            if rs.layout != pred.layout:
                raise ValueError("a record set of another schema or batch size")
        elif pred._check_source(source):
            rs = RecordSet.from_loader(pred, source, max_bytes)
        else:
            rs = RecordSet.from_columns(pred, source, max_bytes)
        pred._check_tables()
        lay, n, B, dev = rs.layout, rs.n, pred.B, pred.device
        nb = (n + B - 1) // B
        G, R = len(plan), repeats
        labels = rs.labels
        uid = rs.ids(user_field) if user_row is not None else None
        what = Evaluation(ks, bool(group_auc))
        names = what.point_names(uid is not None)
        fields_arr = record_fields(lay)
        scratch = torch.zeros(self.ring, rs.stride, dtype=torch.uint8, device=dev)
        kept = torch.empty(1 + G * R, nb * B, dtype=torch.float32, device=dev) if keep_scores else None
        reused = None if keep_scores else torch.empty(nb * B, dtype=torch.float32, device=dev)
        enqueued: List = [None] * (1 + G * R)            # per variant, what enqueue_evaluation returns
        turn = 0

        def records(sorted_keys: Optional[torch.Tensor], mask: int):
            nonlocal turn
            for k in range(nb):
                cnt = min(B, n - k * B)
                if mask:
                    rec = scratch[turn][:lay.record_bytes]
                    turn = (turn + 1) % self.ring
                    permute_into(rs, fields_arr, sorted_keys, mask, k * B, cnt, rec)
                    yield rec.data_ptr(), cnt
                else:
                    yield rs.records[k].data_ptr(), cnt                     # the baseline reads the set itself

        def score(v: int, sorted_keys: Optional[torch.Tensor], mask: int) -> None:
            # one score buffer serves every variant: its metrics are enqueued behind its launches on this stream
            scores = kept[v] if keep_scores else reused
            pred._score(records(sorted_keys, mask), scores)
            enqueued[v] = enqueue_evaluation(what, labels, scores[:n], uid, num_users)

        score(0, None, 0)
        for r in range(R):
            sorted_keys = torch.sort(permutation_keys(seed, r, n, dev)).values
            for g, (_, _, mask) in enumerate(plan):
                score(1 + g * R + r, sorted_keys, mask)
        if pred.emb.strict_indices:
            pred.emb.raise_on_bad_index()
        self.scores = kept[:, :n] if keep_scores else None
        # a key that evaluate omits (no qualifying user) is NaN in the report
        rows = [[d.get(name, math.nan) for name in names] for d in read_evaluations(enqueued)]
        values = [rows[1 + g * R:1 + (g + 1) * R] for g in range(G)]        # variant 1 + g * R + r: (G, R, M)
        return ImportanceReport([p[0] for p in plan], names, rows[0], values, {p[0]: p[1] for p in plan}, seed, n)
