"""Feature encoders on the device: raw integer keys and raw values to the int64 ids in ``[0, V)`` and
the scaled float32 values that ``PackedColumns``, ``DeviceColumns``, the steps and the predictors take.

The reference encodes on the host, value by value: ``LabelEncoder`` is a Python ``dict`` (``deepfm/data/
transforms.py:14-23``), ``MultiHotEncoder`` a Python loop per row (``:65-71``), ``MinMaxScaler`` a numpy expression
(``:44-49``).  Here a vocabulary is an open-addressing hash table in device memory (``dfm_vocab_build``) and every
column of a data set, or of one serving batch, is encoded by ``dfm_encode_columns``: one launch per 64 columns that
writes straight into ``DeviceColumns``' matrices or into a batch record in ``RecordLayout``'s byte format.

``DeviceLabelEncoder``     ``fit`` / ``transform`` of one int64 column; ``min_count`` and ``max_vocab`` prune the
                           vocabulary (the usual Criteo rule; the reference keeps everything), ``hashed`` needs no fit;
``DeviceMultiHotEncoder``  the same over padded token matrices with optional lengths;
``DeviceMinMaxScaler``     min / max from a double reduction, ``(v - min) / (max - min)`` in double, cast to float32;
``DeviceFeatureEncoder``   one of the above per field of a ``DatasetSchema``; ``transform`` gives ``DeviceColumns``,
                           ``encode_into`` one batch record for ``run_from`` / ``predict_from``.

Indices follow ascending key order among the kept keys and index 0 is OOV, so with the defaults the numbering is the
reference's ``sorted(set(values))``.  Strings are out of scope: the caller brings integer keys (a string column is
hashed or dictionary-coded to int64 wherever it is parsed).  The fit runs on torch (a sort, run lengths, a threshold, a
top-K, a compaction) and reads sizes back once; ``transform`` and ``encode_into`` read nothing back and allocate
nothing but their output.  Nothing here needs the GPU at import time; the dtype and shape checks run without one.
"""

from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from deepfm_amd import _lib
from deepfm_amd.data.device_epoch import DeviceColumns
from deepfm_amd.data.packed import RecordLayout
from deepfm_amd.data.schema import DatasetSchema, FeatureType

_INT32_MAX = 2**31 - 1


def _as_tensor(values, what: str) -> torch.Tensor:
    if isinstance(values, torch.Tensor):
        return values
    if isinstance(values, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(values))
    raise TypeError(f"{what}: expected a torch tensor or a numpy array, got {type(values).__name__}")


def _int64_column(values, what: str, ndim: int = 1) -> torch.Tensor:
    """``values`` as an int64 tensor of ``ndim`` axes, wherever it lives: checked on the host, nothing is copied."""
    t = _as_tensor(values, what)
    if t.dtype != torch.int64:
        raise TypeError(f"{what}: raw keys are int64, got {t.dtype} (strings and other integer widths are the "
                        "caller's to convert)")
    if t.dim() != ndim:
        raise ValueError(f"{what}: expected {ndim} axis/axes, got shape {tuple(t.shape)}")
    return t


def _float_column(values, what: str) -> torch.Tensor:
    t = _as_tensor(values, what)
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: raw values are float32 or float64, got {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"{what}: expected one axis, got shape {tuple(t.shape)}")
    return t


def _lengths_column(lengths, n: int, what: str) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    t = _as_tensor(lengths, what)
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: lengths are int32 or int64, got {t.dtype}")
    if tuple(t.shape) != (n,):
        raise ValueError(f"{what}: expected lengths of shape ({n},), got {tuple(t.shape)}")
    return t


def _row_stride(t: torch.Tensor, what: str) -> int:
    """Elements between consecutive samples of a column the kernel reads in place; a layout it cannot address (an
    inner stride, a stride past int32) is refused rather than copied."""
    if t.dim() == 2 and t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{what}: the tokens of a row must be contiguous")
    stride = t.stride(0) if t.shape[0] > 1 else (t.shape[1] if t.dim() == 2 else 1)
    width = t.shape[1] if t.dim() == 2 else 1
    if not width <= stride <= _INT32_MAX:
        raise ValueError(f"{what}: row stride {stride} cannot be addressed by the encode kernel")
    return stride


class _Vocabulary:
    """The kept keys of one field, their counts, and the device hash table built from them."""

    def __init__(self, device) -> None:
        self.device = torch.device(device)
        self.keys = torch.zeros(0, dtype=torch.int64)          # ascending; on the device after fit, the host after load
        self.counts = torch.zeros(0, dtype=torch.int64)
        self.slots: Optional[torch.Tensor] = None              # (capacity, 2) int64: the bytes of dfm_vocab_slot[]
        self.log2_capacity = 0

    def set(self, keys: torch.Tensor, counts: torch.Tensor) -> None:
        if keys.numel() > _lib.VOCAB_MAX_KEYS:
            raise ValueError(f"{keys.numel()} keys: a vocabulary holds at most {_lib.VOCAB_MAX_KEYS}")
        self.keys, self.counts, self.slots = keys, counts, None

    def table(self) -> torch.Tensor:
        """The hash table, built on first use: once per fit or load, never per transform."""
        if self.slots is not None:
            return self.slots
        lib = _lib.load()
        keys = self.keys.to(self.device).contiguous()
        _lib.require_device(keys, "the vocabulary")
        capacity = lib.dfm_vocab_capacity(keys.numel())
        slots = torch.empty(capacity, 2, dtype=torch.int64, device=self.device)
        status = torch.empty(2, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.dfm_vocab_build(_lib.ptr(keys), keys.numel(), _lib.ptr(slots), capacity, _lib.ptr(status),
                                           _lib.stream_handle()))
        no_slot, unordered = status.tolist()                    # once per fit
        if unordered:
            raise ValueError(f"vocabulary keys must be strictly increasing: {unordered} of {keys.numel()} are not")
        if no_slot:
            raise RuntimeError(f"{no_slot} of {keys.numel()} keys found no slot in a table of {capacity}")
        self.keys, self.slots, self.log2_capacity = keys, slots, capacity.bit_length() - 1
        return slots


def _fit_vocabulary(values: torch.Tensor, min_count: int, max_vocab: Optional[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(kept keys ascending, their counts) of a flat int64 tensor: sort + run lengths, the ``min_count`` threshold,
    then the ``max_vocab`` most frequent with ties going to the smaller key."""
    keys, counts = torch.unique(values, sorted=True, return_counts=True)
    if min_count > 1:
        keep = counts >= min_count
        keys, counts = keys[keep], counts[keep]
    if max_vocab is not None and keys.numel() > max_vocab:
        # keys ascend, so a stable descending sort of the counts breaks ties by the smaller key
        top = torch.sort(counts, descending=True, stable=True).indices[:max_vocab]
        top = torch.sort(top).values
        keys, counts = keys[top], counts[top]
    return keys.contiguous(), counts.contiguous()


def _check_vocab_settings(min_count, max_vocab) -> None:
    if not isinstance(min_count, int) or min_count < 1:
        raise ValueError(f"min_count must be a positive int, got {min_count!r}")
    if max_vocab is not None and (not isinstance(max_vocab, int) or max_vocab < 0):
        raise ValueError(f"max_vocab must be None or a non-negative int, got {max_vocab!r}")


class _VocabularyEncoder:
    """What the label and the multi-hot encoder share: the settings, the fitted vocabulary, its state."""

    def __init__(self, min_count: int = 1, max_vocab: Optional[int] = None, device="cuda", name: str = "") -> None:
        _check_vocab_settings(min_count, max_vocab)
        self.min_count, self.max_vocab, self.name = min_count, max_vocab, name
        self.device = torch.device(device)
        self.num_buckets: Optional[int] = None
        self._vocab = _Vocabulary(self.device)
        self._fitted = False

    def _what(self, kind: str) -> str:
        return f"{kind} field {self.name!r}" if self.name else kind

    def _fit_flat(self, flat: torch.Tensor) -> None:
        if self.num_buckets is not None:
            return                                                  # hashed: nothing to learn
        keys, counts = _fit_vocabulary(flat.to(self.device), self.min_count, self.max_vocab)
        self._vocab.set(keys, counts)
        self._vocab.table()
        self._fitted = True

    def _require_fitted(self) -> None:
        if self.num_buckets is None and not self._fitted:
            raise RuntimeError(f"{self._what('encoder of')}: fit or load_state_dict first")

    @property
    def vocabulary_size(self) -> int:
        """Rows of the field's embedding table: the kept keys (or the buckets) + 1 for OOV / padding at index 0."""
        return 1 + (self.num_buckets if self.num_buckets is not None else self._vocab.keys.numel())

    @property
    def classes_(self) -> torch.Tensor:
        """The kept keys, ascending: key ``classes_[i]`` encodes to ``i + 1``."""
        return self._vocab.keys

    @property
    def counts_(self) -> torch.Tensor:
        """How often each kept key occurred in the fitted data."""
        return self._vocab.counts

    def state_dict(self) -> dict:
        """The sorted keys, their counts and the settings, on the host; the hash table is not stored."""
        return {"keys": self._vocab.keys.cpu().clone(), "counts": self._vocab.counts.cpu().clone(),
                "min_count": self.min_count, "max_vocab": self.max_vocab, "num_buckets": self.num_buckets}

    def load_state_dict(self, state: dict) -> None:
        keys = _int64_column(state["keys"], "state_dict keys").cpu().clone()
        counts = _int64_column(state["counts"], "state_dict counts").cpu().clone()
        if keys.shape != counts.shape:
            raise ValueError("state_dict: keys and counts differ in length")
        if keys.numel() > 1 and not bool((keys[1:] > keys[:-1]).all()):
            raise ValueError("state_dict: keys must be strictly increasing")
        _check_vocab_settings(state["min_count"], state["max_vocab"])
        self.min_count, self.max_vocab, self.num_buckets = state["min_count"], state["max_vocab"], state["num_buckets"]
        self._vocab.set(keys, counts)                               # the table is rebuilt at the first transform
        self._fitted = True

    def _job(self, kind: int, raw: torch.Tensor, out_ptr: int, out_stride: int, width: int = 1, raw_width: int = 1,
             lengths: Optional[torch.Tensor] = None) -> _lib.EncodeJob:
        job = _lib.EncodeJob(in_=raw.data_ptr(), out=out_ptr, kind=kind, in_stride=_row_stride(raw, self._what("raw")),
                             out_stride=out_stride, width=width, raw_width=raw_width)
        if self.num_buckets is not None:
            job.kind = _lib.ENC_HASHED
            job.u.num_buckets = self.num_buckets
        else:
            job.u.table.slots = self._vocab.table().data_ptr()
            job.u.table.lengths = _lib.ptr(lengths)
            job.log2_capacity = self._vocab.log2_capacity
        return job


def _launch(jobs: Sequence[_lib.EncodeJob], n: int, n_out: int) -> None:
    """``dfm_encode_columns`` over ``jobs`` on the current stream, 64 jobs per launch."""
    lib = _lib.load()
    stream = _lib.stream_handle()
    for i in range(0, len(jobs), _lib.MAX_FIELDS):
        chunk = jobs[i:i + _lib.MAX_FIELDS]
        _lib.check(lib.dfm_encode_columns((_lib.EncodeJob * len(chunk))(*chunk), len(chunk), n, n_out, stream))


def _zero_job(out_ptr: int, floats_per_sample: int) -> _lib.EncodeJob:
    return _lib.EncodeJob(in_=None, out=out_ptr, kind=_lib.ENC_ZERO_F32, in_stride=0, out_stride=floats_per_sample,
                          width=floats_per_sample, raw_width=1)


class DeviceLabelEncoder(_VocabularyEncoder):
    """The reference's ``LabelEncoder`` (``transforms.py:8-28``) for int64 keys, on the device.

    ``fit(values)`` keeps the keys seen at least ``min_count`` times and, of those, the ``max_vocab`` most frequent
    (ties: the smaller key); the kept keys are numbered 1.. in ascending order, everything else encodes to 0.
    ``values`` is an int64 tensor or numpy array, on the host or the device; any other dtype is a ``TypeError``:
    strings are out of scope, the caller brings integer keys."""

    @classmethod
    def hashed(cls, num_buckets: int, device="cuda", name: str = "") -> "DeviceLabelEncoder":
        """An encoder without a vocabulary: ``1 + mix64(key) % num_buckets`` (``include/deepfm_hip.h``); no fit."""
        if not isinstance(num_buckets, int) or not 1 <= num_buckets < 2**62:
            raise ValueError(f"num_buckets must be a positive int, got {num_buckets!r}")
        enc = cls(device=device, name=name)
        enc.num_buckets = num_buckets
        return enc

    def fit(self, values) -> "DeviceLabelEncoder":
        self._fit_flat(_int64_column(values, self._what("SPARSE")))
        return self

    def job(self, raw: torch.Tensor, out_ptr: int, out_stride: int = 1) -> _lib.EncodeJob:
        return self._job(_lib.ENC_LOOKUP, raw, out_ptr, out_stride)

    def transform(self, values) -> torch.Tensor:
        """(n,) int64 indices on the device."""
        raw = _int64_column(values, self._what("SPARSE"))
        self._require_fitted()
        raw = raw.to(self.device)
        out = torch.empty(raw.shape[0], dtype=torch.int64, device=self.device)
        if raw.shape[0]:
            with torch.cuda.device(self.device):
                _launch([self.job(raw, out.data_ptr())], raw.shape[0], raw.shape[0])
        return out


def _bag_input(tokens, lengths, what: str) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    if isinstance(tokens, (tuple, list)) and len(tokens) == 2 and lengths is None:
        tokens, lengths = tokens
    t = _int64_column(tokens, what, ndim=2)
    if t.shape[1] < 1:
        raise ValueError(f"{what}: a token matrix needs at least one column")
    return t, _lengths_column(lengths, t.shape[0], what)


class DeviceMultiHotEncoder(_VocabularyEncoder):
    """The reference's ``MultiHotEncoder`` (``transforms.py:52-76``) over padded token matrices.

    Input is ``tokens (n, raw_width) int64`` with ``lengths (n,)`` (int32 or int64; ``None``: every row is full);
    row i holds ``min(lengths[i], raw_width)`` valid tokens.  ``fit`` sees the valid tokens only.  ``transform`` gives
    ``(n, max_length)`` int64: position ``j < min(length, max_length)`` is the index of token j, an unseen token 0 in
    place, every other position 0."""

    def __init__(self, max_length: int = 6, min_count: int = 1, max_vocab: Optional[int] = None, device="cuda",
                 name: str = "") -> None:
        super().__init__(min_count, max_vocab, device, name)
        if not isinstance(max_length, int) or max_length < 1:
            raise ValueError(f"max_length must be a positive int, got {max_length!r}")
        self.max_length = max_length

    def fit(self, tokens, lengths=None) -> "DeviceMultiHotEncoder":
        t, ln = _bag_input(tokens, lengths, self._what("SEQUENCE"))
        t = t.to(self.device)
        if ln is not None:
            valid = torch.arange(t.shape[1], device=self.device)[None, :] < ln.to(self.device)[:, None]
            t = t[valid]
        self._fit_flat(t.reshape(-1))
        return self

    def job(self, raw: torch.Tensor, lengths: Optional[torch.Tensor], out_ptr: int) -> _lib.EncodeJob:
        return self._job(_lib.ENC_BAG, raw, out_ptr, self.max_length, self.max_length, raw.shape[1], lengths)

    def _device_input(self, tokens, lengths):
        t, ln = _bag_input(tokens, lengths, self._what("SEQUENCE"))
        self._require_fitted()
        t = t.to(self.device)
        if ln is not None:
            ln = ln.to(self.device, torch.int32).contiguous()
        return t, ln

    def transform(self, tokens, lengths=None) -> torch.Tensor:
        t, ln = self._device_input(tokens, lengths)
        out = torch.empty(t.shape[0], self.max_length, dtype=torch.int64, device=self.device)
        if t.shape[0]:
            with torch.cuda.device(self.device):
                _launch([self.job(t, ln, out.data_ptr())], t.shape[0], t.shape[0])
        return out

    def state_dict(self) -> dict:
        return dict(super().state_dict(), max_length=self.max_length)

    def load_state_dict(self, state: dict) -> None:
        super().load_state_dict(state)
        self.max_length = int(state["max_length"])


class DeviceMinMaxScaler:
    """The reference's ``MinMaxScaler`` (``transforms.py:31-49``) followed by ``PackedColumns``' float32 cast:
    ``float32((float64(v) - min) / (max - min))``, 0 when ``max == min``, no clipping.  ``fit`` reduces in double on
    the device and keeps ``min`` / ``max`` as Python floats; non-finite input is refused, naming the field."""

    def __init__(self, device="cuda", name: str = "") -> None:
        self.device, self.name = torch.device(device), name
        self.min, self.max = 0.0, 1.0                               # the reference's initial state

    def _what(self) -> str:
        return f"DENSE field {self.name!r}" if self.name else "DENSE"

    def fit(self, values) -> "DeviceMinMaxScaler":
        v = _float_column(values, self._what())
        if v.numel() == 0:
            raise ValueError(f"{self._what()}: cannot fit an empty column")
        v = v.to(self.device)
        lo, hi, bad = torch.stack([v.min().double(), v.max().double(), (~torch.isfinite(v)).sum().double()]).tolist()
        if bad:
            raise ValueError(f"{self._what()}: {int(bad)} non-finite value(s); a scaler cannot be fitted to NaN or inf")
        self.min, self.max = lo, hi
        return self

    def job(self, raw: torch.Tensor, out_ptr: int) -> _lib.EncodeJob:
        kind = _lib.ENC_SCALE_F64 if raw.dtype == torch.float64 else _lib.ENC_SCALE_F32
        job = _lib.EncodeJob(in_=raw.data_ptr(), out=out_ptr, kind=kind, in_stride=_row_stride(raw, self._what()),
                             out_stride=1, width=1, raw_width=1)
        job.u.scale.lo, job.u.scale.hi = self.min, self.max
        return job

    def transform(self, values) -> torch.Tensor:
        """(n,) float32 on the device."""
        v = _float_column(values, self._what()).to(self.device)
        out = torch.empty(v.shape[0], dtype=torch.float32, device=self.device)
        if v.shape[0]:
            with torch.cuda.device(self.device):
                _launch([self.job(v, out.data_ptr())], v.shape[0], v.shape[0])
        return out

    def state_dict(self) -> dict:
        return {"min": self.min, "max": self.max}

    def load_state_dict(self, state: dict) -> None:
        self.min, self.max = float(state["min"]), float(state["max"])


PerField = Union[None, int, Dict[str, int]]


def _per_field(setting: PerField, name: str, default):
    if isinstance(setting, dict):
        return setting.get(name, default)
    return default if setting is None else setting


class DeviceFeatureEncoder:
    """One encoder per field of a template ``DatasetSchema`` (its vocabulary sizes are ignored): a
    ``DeviceLabelEncoder`` per SPARSE field, a ``DeviceMultiHotEncoder`` per SEQUENCE field (``max_length`` from the
    field), a ``DeviceMinMaxScaler`` per DENSE field.  ``min_count``, ``max_vocab`` and ``hashed`` (a bucket count:
    that SPARSE field is hashed, not fitted) are each one int for every field or a dict by field name.

    ``raw`` is a dict from field name to an int64 column (SPARSE), a float32 / float64 column (DENSE), or
    ``(tokens (n, raw_width) int64, lengths (n,) or None)`` (SEQUENCE); tensors or numpy arrays, host or device.
    Strings are out of scope: the caller brings integer keys."""

    def __init__(self, schema: DatasetSchema, min_count: PerField = 1, max_vocab: PerField = None,
                 hashed: PerField = None, device="cuda") -> None:
        self.template = schema
        self.device = torch.device(device)
        self.encoders: Dict[str, object] = {}
        for name, spec in schema.fields.items():
            mc, mv = _per_field(min_count, name, 1), _per_field(max_vocab, name, None)
            if spec.feature_type is FeatureType.DENSE:
                self.encoders[name] = DeviceMinMaxScaler(self.device, name)
            elif spec.feature_type is FeatureType.SEQUENCE:
                self.encoders[name] = DeviceMultiHotEncoder(spec.max_length, mc, mv, self.device, name)
            else:
                buckets = _per_field(hashed, name, None)
                self.encoders[name] = (DeviceLabelEncoder.hashed(buckets, self.device, name) if buckets is not None
                                       else DeviceLabelEncoder(mc, mv, self.device, name))
        self._layouts: Dict[int, RecordLayout] = {}

    def fit(self, raw: dict) -> "DeviceFeatureEncoder":
        cols = self._checked(raw)[1]                                # every column is checked before any is fitted
        for name, enc in self.encoders.items():
            enc.fit(*cols[name]) if isinstance(enc, DeviceMultiHotEncoder) else enc.fit(cols[name][0])
        return self

    @property
    def schema(self) -> DatasetSchema:
        """A copy of the template with the fitted vocabulary sizes."""
        out = copy.deepcopy(self.template)
        for name, spec in out.fields.items():
            if spec.feature_type is not FeatureType.DENSE:
                spec.vocabulary_size = self.encoders[name].vocabulary_size
        return out

    def _checked(self, raw: dict):
        """(n, {field: (column, lengths or None)}): every field's column checked on the host (dtype, shape, one common
        length), wherever it lives."""
        cols, n = {}, None
        for name, enc in self.encoders.items():
            col = raw[name]                                         # KeyError for a missing field, like the reference
            if isinstance(enc, DeviceMultiHotEncoder):
                t, ln = _bag_input(col, None, enc._what("SEQUENCE"))
            elif isinstance(enc, DeviceMinMaxScaler):
                t, ln = _float_column(col, enc._what()), None
            else:
                t, ln = _int64_column(col, enc._what("SPARSE")), None
            if n is None:
                n = t.shape[0]
            if t.shape[0] != n:
                raise ValueError(f"field {name!r}: {t.shape[0]} samples, expected {n}")
            cols[name] = (t, ln)
        return n, cols

    def _inputs(self, raw: dict, labels):
        """``_checked`` plus the labels, then everything moved to the device where it is not there yet.  Returns
        (n, columns by field, labels or None)."""
        n, cols = self._checked(raw)
        if labels is not None:
            labels = _as_tensor(labels, "labels")
            if labels.dtype != torch.float32 or (n is not None and tuple(labels.shape) != (n,)):
                raise ValueError(f"labels: expected float32 of shape ({n},), got {labels.dtype} {tuple(labels.shape)}")
            if n is None:
                n = labels.shape[0]
        if n is None:
            raise ValueError("nothing to encode: the schema has no field and no labels were given")
        for name, enc in self.encoders.items():
            if not isinstance(enc, DeviceMinMaxScaler):
                enc._require_fitted()
            t, ln = cols[name]
            cols[name] = (t.to(self.device), None if ln is None else ln.to(self.device, torch.int32).contiguous())
        return n, cols, None if labels is None else labels.to(self.device)

    def _jobs(self, cols, labels, outs, labels_ptr: int) -> List[_lib.EncodeJob]:
        """The job of every field writing at ``outs[name]`` (a device address), plus the labels' copy."""
        jobs = []
        for name, enc in self.encoders.items():
            t, ln = cols[name]
            if isinstance(enc, DeviceMultiHotEncoder):
                jobs.append(enc.job(t, ln, outs[name]))
            else:
                jobs.append(enc.job(t, outs[name]))
        if labels is not None:
            jobs.append(_lib.EncodeJob(in_=labels.data_ptr(), out=labels_ptr, kind=_lib.ENC_COPY_F32,
                                       in_stride=_row_stride(labels, "labels"), out_stride=1, width=1, raw_width=1))
        return jobs

    def transform(self, raw: dict, labels) -> DeviceColumns:
        """The encoded data set as ``DeviceColumns``: ids (S, n), dense (Dn, n), labels (n,), bags; nothing is copied
        to the host."""
        if labels is None:
            raise ValueError("transform needs the labels: DeviceColumns holds them")
        n, cols, labels = self._inputs(raw, labels)
        schema = self.schema
        ns, nd = len(schema.sparse_fields), len(schema.dense_fields)
        ids = torch.empty(ns, n, dtype=torch.int64, device=self.device)
        dense = torch.empty(nd, n, dtype=torch.float32, device=self.device)
        out_labels = torch.empty(n, dtype=torch.float32, device=self.device)
        bags = [torch.empty(n, s.max_length, dtype=torch.int64, device=self.device) for s in schema.sequence_fields]
        result = DeviceColumns.from_device(schema, ids, dense, out_labels, bags)
        if n:
            outs = {name: t.data_ptr() for name, t in result.field_columns().items()}
            with torch.cuda.device(self.device):
                _launch(self._jobs(cols, labels, outs, out_labels.data_ptr()), n, n)
        return result

    def encode_into(self, record: torch.Tensor, raw: dict, labels=None, valid: Optional[int] = None) -> torch.Tensor:
        """One batch record in ``RecordLayout``'s byte format from the first ``valid`` samples of ``raw`` (default:
        all of them): what ``RecordLayout.write`` produces from host-encoded columns, its zero padding tail included
        (labels are zeros when none are given).  ``record`` is a uint8 device tensor of the layout's ``record_bytes``,
        16-byte aligned; its batch size follows from its length.  One ``dfm_encode_columns`` launch per 64 columns on
        the current stream; nothing is read back and nothing allocated once the raw columns are on the device.  The
        record goes straight to ``run_from`` / ``predict_from``.  Returns ``record``."""
        if not isinstance(record, torch.Tensor) or record.dtype != torch.uint8 or record.dim() != 1:
            raise TypeError("record: expected a flat uint8 tensor")
        n, cols, labels = self._inputs(raw, labels)
        valid = n if valid is None else valid
        if not 0 < valid <= n:
            raise ValueError(f"valid = {valid} outside (0, {n}]")
        lay = self._layout_of(record.numel(), valid)
        _lib.require_device(record, "record")
        if record.data_ptr() % 16:
            raise ValueError("record must be 16-byte aligned")
        base, B = record.data_ptr(), lay.batch_size
        outs = {name: base + off for name, off in zip(lay.names, lay.field_offsets)}
        jobs = self._jobs(cols, labels, outs, base + lay.labels_offset)
        if labels is None:
            jobs.append(_zero_job(base + lay.labels_offset, 1))
        if not lay.n_sparse:
            jobs.append(_zero_job(base + lay.ids_offset, 2))       # the padding row of an ids block without a field
        if not lay.n_dense:
            jobs.append(_zero_job(base + lay.dense_offset, 1))
        with torch.cuda.device(record.device):
            _launch(jobs, valid, B)
        return record

    def _layout_of(self, nbytes: int, valid: int) -> RecordLayout:
        """The layout whose record has ``nbytes`` bytes: a record is B times the bytes of one sample plus less than
        16 bytes of alignment per bag block, so B follows from the length (kept per length: no per-call search)."""
        lay = self._layouts.get(nbytes)
        if lay is None:
            schema = self.schema
            one = RecordLayout.of(schema, 1)
            per = 8 * one.id_rows + 4 * one.dense_rows + 4 + 8 * sum(one.seq_lengths)
            for B in range(max(1, (nbytes - 16 * len(one.seq_lengths)) // per), nbytes // per + 1):
                cand = RecordLayout.of(schema, B)
                if cand.record_bytes == nbytes:
                    lay = cand
                    break
            if lay is None:
                raise ValueError(f"a record of {nbytes} bytes is no batch record of this schema")
            self._layouts[nbytes] = lay
        if valid > lay.batch_size:
            raise ValueError(f"{valid} samples for a record of {lay.batch_size}")
        return lay

    def state_dict(self) -> dict:
        return {name: enc.state_dict() for name, enc in self.encoders.items()}

    def load_state_dict(self, state: dict) -> None:
        if set(state) != set(self.encoders):
            raise KeyError(f"state_dict fields {sorted(state)} != schema fields {sorted(self.encoders)}")
        for name, enc in self.encoders.items():
            enc.load_state_dict(state[name])
        self._layouts.clear()
