"""Row-wise int8 and 4-bit embedding tables for serving (``include/deepfm_hip.h``: DFM_QUANT_INT8_ROWWISE and
DFM_QUANT_UINT4_ROWWISE).

``"int8"``: one record of ``16 + D`` bytes per table row, D in {16, 32, 64}:

    [ scale fp32 | lo fp32 | w1 fp32 (the id's first-order weight, unchanged) | 0 | q[0..D) uint8 ]

with ``scale = (hi - lo) / 255``, ``q = min(255, rint((x - lo) / scale))`` (0 when ``scale == 0``) and the dequantised
value ``x' = q * scale + lo`` in two fp32 roundings, so a constant row (the all-zero padding row 0) is exact and every
other row has ``|x' - x| <= scale / 2 + 2**-21 * max(|lo|, |hi|)``.  32 / 48 / 80 bytes per id at D = 16 / 32 / 64
against 68 / 132 / 260 of the fp32 (row, first-order weight) pair.

``"uint4"``: one record of ``8 + D / 2`` bytes (16 / 24 / 40):

    [ scale binary16 | lo binary16 | w1 fp32 | q[0..D) 4 bits each, the low nibble for the even element ]

with ``lo`` the largest binary16 value not above the row's minimum, ``scale`` the smallest binary16 value not below
``(hi - lo) / 15`` (one more where ``lo + 15 * scale`` would still be under ``hi``), ``q = min(15, rint((x - lo) / scale))`` and the same ``x' = q * scale + lo``: the all-zero padding
row is exact and every row has ``|x' - x| <= scale / 2 + 2**-21 * max(|lo|, |lo + 15 * scale|)``.  A row whose
minimum is below -65504 or whose scale is beyond binary16 is refused, as a non-finite element is.

``QuantizedTables`` holds the records of every SPARSE field of a uniform schema; ``QuantizedPredictor``
(``training/predict.py``) serves from them and never reads the fp32 tables again.  ``QuantizedMixedTables`` holds the
records of the SPARSE and SEQUENCE fields of any schema the record gather takes (bags, projections, mixed widths), each
field at its own width, for ``QuantizedMixedPredictor``.  The quantiser, its inverse and the
gather are HIP kernels (``csrc/quant.hip``); tables built by ``from_records`` may sit on the host (files, checks), but
``dequantized()`` and the predictor need them on the device.
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from deepfm_amd import _lib
from deepfm_amd.data.schema import DatasetSchema, FeatureType
from deepfm_amd.training.eligibility import ineligible_reason, mixed_ineligible_reason

FORMATS = {"int8": _lib.QUANT_INT8_ROWWISE, "uint4": _lib.QUANT_UINT4_ROWWISE}
HEADER_BYTES = 16                                   # of an int8 record
_HEADER_BYTES = {"int8": HEADER_BYTES, "uint4": 8}
_LEVELS = {"int8": 255.0, "uint4": 15.0}            # the largest code


def row_bytes(dim: int, fmt: str = "int8") -> int:
    """Record size in bytes (``dfm_quant_row_bytes``); ``ValueError`` for an unsupported width or format."""
    if fmt not in FORMATS:
        raise ValueError(f"quantised format {fmt!r}: {sorted(FORMATS)} only")
    if dim not in _lib.QUANT_DIMS:
        raise ValueError(f"quantised tables of width {dim}: widths 16, 32 and 64 only")
    return _HEADER_BYTES[fmt] + (dim if fmt == "int8" else dim // 2)


def quantized_ineligible_reason(model) -> Optional[str]:
    """Why ``QuantizedPredictor`` cannot take ``model`` (None: it can): ``ineligible_reason(model)`` first, unchanged,
    then the widths and the field counts of the quantised gather.  Checked on the host only."""
    reason = ineligible_reason(model)
    if reason is not None:
        return reason
    D = model.embedding.fm_embed_dim
    if D not in _lib.QUANT_DIMS:
        return f"fm_embed_dim {D}: the quantised tables take the widths 16, 32 and 64"
    kinds = [s.feature_type for s in model.schema.fields.values()]
    ns, nd = kinds.count(FeatureType.SPARSE), kinds.count(FeatureType.DENSE)
    if ns > _lib.QUANT_MAX_SPARSE or nd > _lib.QUANT_MAX_DENSE:
        return (f"{ns} SPARSE + {nd} DENSE fields: the quantised gather takes at most {_lib.QUANT_MAX_SPARSE} SPARSE "
                f"and {_lib.QUANT_MAX_DENSE} DENSE fields")
    return None


def _refused(name: str, fmt: str) -> ValueError:
    return ValueError(f"the embedding table of field {name!r} has a non-finite element or a row whose "
                      f"range overflows the {fmt} format: it cannot be quantised")


def _as_records(name: str, r, V: int, rb: int) -> torch.Tensor:
    """Stored records of one field as a uint8 tensor of V * rb bytes; ``ValueError`` naming the field otherwise."""
    t = r if isinstance(r, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(r))
    if t.dtype != torch.uint8 or t.numel() != V * rb:
        raise ValueError(f"field {name!r}: expected {V} x {rb} uint8 bytes, got {tuple(t.shape)} {t.dtype}")
    return t


def _quantize_field(emb, name: str, V: int, dim: int, fmt: str, rec: torch.Tensor, flag_ptr: int) -> None:
    """One ``dfm_quantize_rows`` launch: field ``name``'s (second-order, first-order) pair of ``emb`` into ``rec``."""
    w2 = emb.second_order_embeddings[name].weight
    w1 = emb.first_order_embeddings[name].weight
    if w2.shape[0] != V:
        raise ValueError(f"the embedding table of field {name!r} is released: call restore_tables() first")
    for p in (w2, w1):
        _lib.require_device(p, f"table of field {name!r}")
        if p.dtype != torch.float32 or p.dim() != 2 or (p.shape[1] > 1 and p.stride(1) != 1):
            raise TypeError("embedding tables must be float32 with contiguous rows")
    _lib.check(_lib.load().dfm_quantize_rows(w2.data_ptr(), w2.stride(0), w1.data_ptr(), w1.stride(0), V, dim,
                                             FORMATS[fmt], rec.data_ptr(), flag_ptr, _lib.stream_handle()))


def _dequantize_field(name: str, rec: torch.Tensor, V: int, dim: int, fmt: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(w2 (V, dim), w1 (V, 1))`` as fp32, by ``dfm_dequantize_rows``."""
    _lib.require_device(rec, f"records of field {name!r}")
    w2 = torch.empty(V, dim, dtype=torch.float32, device=rec.device)
    w1 = torch.empty(V, 1, dtype=torch.float32, device=rec.device)
    _lib.check(_lib.load().dfm_dequantize_rows(rec.data_ptr(), V, dim, FORMATS[fmt], w2.data_ptr(), w1.data_ptr(),
                                               _lib.stream_handle()))
    return w2, w1


def _field_error_bound(rec: torch.Tensor, fmt: str) -> float:
    """max over a field's rows of scale / 2 + 2**-21 * max(|lo|, |hi|), hi as the record holds it."""
    half = torch.float32 if fmt == "int8" else torch.float16
    head = rec[:, :2 * half.itemsize].contiguous().view(half).double()
    scale, lo = head[:, 0], head[:, 1]
    hi = lo + _LEVELS[fmt] * scale
    bound = scale / 2 + 2.0 ** -21 * torch.maximum(lo.abs(), hi.abs())
    return float(bound.max()) if bound.numel() else 0.0


def _requantize(emb, fmt: str, fields, records, flags: torch.Tensor, check: bool) -> None:
    """``refresh`` of either table class: ``fields`` is [(name, V, dim)]; one launch per field into the same buffers,
    then (``check``) one read of the refusal flags."""
    flags.zero_()
    for i, (name, V, dim) in enumerate(fields):
        _quantize_field(emb, name, V, dim, fmt, records[name], flags.data_ptr() + 4 * i)
    if check and fields:
        for (name, _, _), flag in zip(fields, flags.cpu().tolist()):
            if flag:
                raise _refused(name, fmt)


def _sparse_vocab(schema: DatasetSchema, dim: int) -> Dict[str, int]:
    """{SPARSE field: vocabulary size}, schema order; ``ValueError`` naming a field the format cannot hold."""
    out = {}
    for name, spec in schema.fields.items():
        if spec.feature_type is FeatureType.SEQUENCE:
            raise ValueError(f"field {name!r} is a SEQUENCE field: quantised tables take SPARSE and DENSE fields")
        if spec.embedding_dim != dim:
            raise ValueError(f"field {name!r}: embedding_dim {spec.embedding_dim} is not the tables' width {dim}")
        if spec.feature_type is FeatureType.SPARSE:
            out[name] = int(spec.vocabulary_size)
    return out


class QuantizedTables:
    """The quantised (second-order row, first-order weight) records of every SPARSE field of a schema."""

    def __init__(self, schema: DatasetSchema, dim: int, fmt: str, records: Dict[str, torch.Tensor],
                 model=None) -> None:
        self.schema, self.dim, self.format = schema, int(dim), fmt
        self.row_bytes = row_bytes(self.dim, fmt)
        self.header_bytes = _HEADER_BYTES[fmt]
        self.vocab = _sparse_vocab(schema, self.dim)
        self.records = records                   # {field: (V, row_bytes) uint8}; the buffers are never replaced
        self._model = model
        self._flags: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_model(cls, model, fmt: str = "int8") -> "QuantizedTables":
        """Quantise every SPARSE field's (second-order, first-order) pair of ``model`` on the device, in ``'dense'``
        or ``'rowsparse'`` grad mode (contiguous tables or packed row records).  ``ValueError`` naming the field for
        a table with a non-finite element or a row whose range overflows (``"uint4"``: whose minimum or scale is
        beyond binary16)."""
        emb = model.embedding
        dim = emb.fm_embed_dim
        rb = row_bytes(dim, fmt)
        vocab = _sparse_vocab(model.schema, dim)
        p0 = next(model.parameters())
        _lib.require_device(p0, "model parameters")
        records = {name: torch.empty(V, rb, dtype=torch.uint8, device=p0.device) for name, V in vocab.items()}
        tables = cls(model.schema, dim, fmt, records, model)
        tables.refresh()
        return tables

    @classmethod
    def from_records(cls, schema: DatasetSchema, dim: int, records: Dict[str, object],
                     fmt: str = "int8") -> "QuantizedTables":
        """Tables from stored records: ``{field: uint8 array or tensor of V * row_bytes bytes}`` for every SPARSE field
        of ``schema`` (files, host-side checks).  A missing or extra field or a wrong size is refused by name."""
        rb = row_bytes(dim, fmt)
        vocab = _sparse_vocab(schema, dim)
        cls._check_names(vocab, records)
        out = {name: _as_records(name, records[name], V, rb).contiguous().view(V, rb) for name, V in vocab.items()}
        return cls(schema, dim, fmt, out)

    @staticmethod
    def _check_names(vocab: Dict[str, int], records) -> None:
        missing = [n for n in vocab if n not in records]
        extra = [n for n in records if n not in vocab]
        if missing:
            raise ValueError(f"no records for SPARSE field {missing[0]!r}")
        if extra:
            raise ValueError(f"records for {extra[0]!r}, which is no SPARSE field of the schema")

    def to(self, device) -> "QuantizedTables":
        """The same tables with their records on ``device`` (new buffers: for tables no predictor reads yet)."""
        return QuantizedTables(self.schema, self.dim, self.format, {n: r.to(device) for n, r in self.records.items()},
                               self._model)

    @property
    def device(self) -> torch.device:
        return next(iter(self.records.values())).device if self.records else torch.device("cpu")

    # ------------------------------------------------------------------ the quantiser
    def refresh(self, check: bool = True) -> "QuantizedTables":
        """Requantise the model's tables into the same buffers, in stream order: no pointer changes, so live graphs
        stay valid.  ``check`` reads the refusal flags once per table (one host synchronisation) and raises
        ``ValueError`` naming the field; the records of a refused table are meaningless."""
        if self._model is None:
            raise ValueError("these tables were built from records: there is no model to requantise")
        names = list(self.vocab)
        dev = self.device
        if self._flags is None or self._flags.device != dev:
            self._flags = torch.zeros(max(len(names), 1), dtype=torch.int32, device=dev)
        _requantize(self._model.embedding, self.format, [(n, self.vocab[n], self.dim) for n in names], self.records,
                    self._flags, check)
        return self

    def dequantized(self) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """``{field: (w2 (V, D), w1 (V, 1))}`` as fp32, by ``dfm_dequantize_rows``."""
        return {name: _dequantize_field(name, rec, self.vocab[name], self.dim, self.format)
                for name, rec in self.records.items()}

    # ------------------------------------------------------------------ sizes and bounds
    @property
    def nbytes(self) -> int:
        return sum(V * self.row_bytes for V in self.vocab.values())

    @property
    def fp32_nbytes(self) -> int:
        """Bytes of the same tables as contiguous fp32: a (D,) row and a first-order weight per id."""
        return sum(V * (4 * self.dim + 4) for V in self.vocab.values())

    def error_bound(self) -> Dict[str, float]:
        """``{field: max over rows of scale / 2 + 2**-21 * max(|lo|, |hi|)}``: the bound on ``|x' - x|`` of any
        element of the field's table (hi = lo + 255 * scale, or lo + 15 * scale, as the record holds them)."""
        return {name: _field_error_bound(rec, self.format) for name, rec in self.records.items()}

    # ------------------------------------------------------------------ persistence
    def state_dict(self) -> Dict[str, object]:
        return {"format": self.format, "dim": self.dim, "vocab": dict(self.vocab),
                "records": {n: r.clone() for n, r in self.records.items()}}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        """Copy stored records into these tables' buffers (no pointer changes).  Another format, width, field set or
        vocabulary than this schema's is refused by name."""
        if state.get("format") != self.format:
            raise ValueError(f"stored format {state.get('format')!r}, these tables hold {self.format!r}")
        if state.get("dim") != self.dim:
            raise ValueError(f"stored width {state.get('dim')}, these tables hold width {self.dim}")
        self._check_names(self.vocab, state["records"])
        self._check_names(self.vocab, state["vocab"])
        for name, V in self.vocab.items():
            if int(state["vocab"][name]) != V:
                raise ValueError(f"field {name!r}: stored vocabulary {state['vocab'][name]}, the schema has {V}")
            _as_records(name, state["records"][name], V, self.row_bytes)
        for name, V in self.vocab.items():
            r = _as_records(name, state["records"][name], V, self.row_bytes)
            self.records[name].copy_(r.view(self.records[name].shape))

    def matches(self, model) -> Optional[str]:
        """Why these tables cannot serve ``model`` (None: they can)."""
        if self.dim != model.embedding.fm_embed_dim:
            return f"tables of width {self.dim} for a model of fm_embed_dim {model.embedding.fm_embed_dim}"
        for name, spec in model.schema.fields.items():
            if spec.feature_type is FeatureType.SPARSE:
                if name not in self.vocab:
                    return f"no records for SPARSE field {name!r}"
                if self.vocab[name] != spec.vocabulary_size:
                    return f"field {name!r}: {self.vocab[name]} records, the schema has {spec.vocabulary_size} ids"
        extra = [n for n in self.vocab if n not in model.schema.fields]
        if extra:
            return f"records for {extra[0]!r}, which is no field of the model's schema"
        return None


# ====================================================================================================================
# mixed schemas: SEQUENCE fields, projections, mixed widths (MixedSchemaPredictor's models)
# ====================================================================================================================
def _quantisable(schema: DatasetSchema) -> Dict[str, Tuple[int, int]]:
    """{field: (vocabulary size, width)} of the SPARSE and SEQUENCE fields whose width a record format holds."""
    return {name: (int(spec.vocabulary_size), int(spec.embedding_dim)) for name, spec in schema.fields.items()
            if spec.feature_type is not FeatureType.DENSE and spec.embedding_dim in _lib.QUANT_DIMS}


def _chosen(schema: DatasetSchema, fields) -> Dict[str, Tuple[int, int]]:
    """``_quantisable`` narrowed to ``fields`` (None: all of it); a named field that cannot be quantised is refused
    by name."""
    can = _quantisable(schema)
    if fields is None:
        return can
    out = {}
    for name in fields:
        spec = schema.fields.get(name)
        if spec is None:
            raise ValueError(f"field {name!r} is no field of the schema")
        if spec.feature_type is FeatureType.DENSE:
            raise ValueError(f"field {name!r} is a DENSE field: it has no table to quantise")
        if name not in can:
            raise ValueError(f"field {name!r}: quantised tables of width {spec.embedding_dim}: widths 16, 32 and 64 "
                             "only (a narrower field stays fp32)")
        out[name] = can[name]
    return {name: out[name] for name in schema.fields if name in out}        # schema order


def quantized_mixed_ineligible_reason(model) -> Optional[str]:
    """Why ``QuantizedMixedPredictor`` cannot take ``model`` (None: it can): ``mixed_ineligible_reason(model)`` first,
    unchanged, then whether there is anything to quantise.  Checked on the host only."""
    reason = mixed_ineligible_reason(model)
    if reason is not None:
        return reason
    if not _quantisable(model.schema):
        return ("no SPARSE or SEQUENCE field of width 16, 32 or 64: nothing to quantise (MixedSchemaPredictor serves "
                "this model)")
    return None


class QuantizedMixedTables:
    """The quantised (second-order row, first-order weight) records of the SPARSE and SEQUENCE fields of any schema
    ``MixedSchemaPredictor`` serves, each field at its OWN width: ``dims[name]`` in {16, 32, 64}, whatever
    ``fm_embed_dim`` is (a projected field's records hold its raw row).  One format for all of them.

    A SPARSE or SEQUENCE field of width 4, 8 or any other is not quantised: it stays fp32, is listed in
    ``fp32_fields`` and is served through the model's own tables.  No narrow record formats exist, on purpose: an int8
    record of width 4 or 8 would take 20 / 24 bytes against the 20 / 36 of the fp32 (row, first-order weight) pair,
    as large or barely smaller.  DENSE fields have no table.

    The surface is ``QuantizedTables``': ``records``, ``vocab``, ``format``, ``refresh``, ``dequantized``,
    ``error_bound``, ``nbytes`` / ``fp32_nbytes`` (of the quantised fields), ``to``, ``state_dict`` /
    ``load_state_dict``, ``from_records`` and ``matches``; ``dims`` is per field."""

    def __init__(self, schema: DatasetSchema, fmt: str, records: Dict[str, torch.Tensor], model=None) -> None:
        if fmt not in FORMATS:
            raise ValueError(f"quantised format {fmt!r}: {sorted(FORMATS)} only")
        chosen = _chosen(schema, list(records))
        self.schema, self.format = schema, fmt
        self.vocab = {name: V for name, (V, _) in chosen.items()}
        self.dims = {name: d for name, (_, d) in chosen.items()}
        self.records = {name: records[name] for name in chosen}      # schema order; the buffers are never replaced
        self.fp32_fields = [name for name, spec in schema.fields.items()
                            if spec.feature_type is not FeatureType.DENSE and name not in chosen]
        self._model = model
        self._flags: Optional[torch.Tensor] = None

    def row_bytes(self, name: str) -> int:
        return row_bytes(self.dims[name], self.format)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_model(cls, model, fmt: str = "int8", fields=None) -> "QuantizedMixedTables":
        """Quantise, on the device, every SPARSE and SEQUENCE field of ``model`` whose ``embedding_dim`` is 16, 32 or
        64 (``fields``: that subset; a named field that is DENSE or narrow is refused by name), one
        ``dfm_quantize_rows`` launch per field at that field's width.  ``ValueError`` naming the field for a table with
        a non-finite element or a row the format cannot hold."""
        if fmt not in FORMATS:
            raise ValueError(f"quantised format {fmt!r}: {sorted(FORMATS)} only")
        chosen = _chosen(model.schema, fields)
        p0 = next(model.parameters())
        _lib.require_device(p0, "model parameters")
        records = {name: torch.empty(V, row_bytes(d, fmt), dtype=torch.uint8, device=p0.device)
                   for name, (V, d) in chosen.items()}
        return cls(model.schema, fmt, records, model).refresh()

    @classmethod
    def from_records(cls, schema: DatasetSchema, records: Dict[str, object], fmt: str = "int8",
                     fields=None) -> "QuantizedMixedTables":
        """Tables from stored records: ``{field: uint8 array or tensor of V * row_bytes bytes}`` for every
        quantisable field of ``schema`` (``fields``: for that subset).  A missing or extra field or a wrong size is
        refused by name."""
        if fmt not in FORMATS:
            raise ValueError(f"quantised format {fmt!r}: {sorted(FORMATS)} only")
        chosen = _chosen(schema, fields)
        cls._check_names(chosen, records)
        out = {}
        for name, (V, d) in chosen.items():
            rb = row_bytes(d, fmt)
            out[name] = _as_records(name, records[name], V, rb).contiguous().view(V, rb)
        return cls(schema, fmt, out)

    @staticmethod
    def _check_names(want, got) -> None:
        missing = [n for n in want if n not in got]
        extra = [n for n in got if n not in want]
        if missing:
            raise ValueError(f"no records for field {missing[0]!r}")
        if extra:
            raise ValueError(f"records for {extra[0]!r}, which is no quantised field of these tables")

    def to(self, device) -> "QuantizedMixedTables":
        """The same tables with their records on ``device`` (new buffers: for tables no predictor reads yet)."""
        return QuantizedMixedTables(self.schema, self.format, {n: r.to(device) for n, r in self.records.items()},
                                    self._model)

    @property
    def device(self) -> torch.device:
        return next(iter(self.records.values())).device if self.records else torch.device("cpu")

    # ------------------------------------------------------------------ the quantiser
    def refresh(self, check: bool = True) -> "QuantizedMixedTables":
        """Requantise the model's tables into the same buffers, in stream order: no pointer changes, so live graphs
        stay valid.  ``check`` reads the refusal flags once (one host synchronisation) and raises ``ValueError``
        naming the field; the records of a refused table are meaningless.  The fp32 fields are not looked at."""
        if self._model is None:
            raise ValueError("these tables were built from records: there is no model to requantise")
        dev = self.device
        if self._flags is None or self._flags.device != dev:
            self._flags = torch.zeros(max(len(self.records), 1), dtype=torch.int32, device=dev)
        _requantize(self._model.embedding, self.format, [(n, self.vocab[n], self.dims[n]) for n in self.records],
                    self.records, self._flags, check)
        return self

    def dequantized(self) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """``{field: (w2 (V, dims[field]), w1 (V, 1))}`` as fp32, by ``dfm_dequantize_rows``."""
        return {name: _dequantize_field(name, rec, self.vocab[name], self.dims[name], self.format)
                for name, rec in self.records.items()}

    # ------------------------------------------------------------------ sizes and bounds
    @property
    def nbytes(self) -> int:
        return sum(V * self.row_bytes(name) for name, V in self.vocab.items())

    @property
    def fp32_nbytes(self) -> int:
        """Bytes of the quantised fields' tables as contiguous fp32: a (d,) row and a first-order weight per id."""
        return sum(V * (4 * self.dims[name] + 4) for name, V in self.vocab.items())

    def error_bound(self) -> Dict[str, float]:
        """``{field: max over rows of scale / 2 + 2**-21 * max(|lo|, |hi|)}``, as ``QuantizedTables.error_bound``."""
        return {name: _field_error_bound(rec, self.format) for name, rec in self.records.items()}

    # ------------------------------------------------------------------ persistence
    def state_dict(self) -> Dict[str, object]:
        return {"format": self.format, "dims": dict(self.dims), "vocab": dict(self.vocab),
                "records": {n: r.clone() for n, r in self.records.items()}}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        """Copy stored records into these tables' buffers (no pointer changes).  Another format, field set, width or
        vocabulary than these tables' is refused by name."""
        if state.get("format") != self.format:
            raise ValueError(f"stored format {state.get('format')!r}, these tables hold {self.format!r}")
        for key in ("records", "vocab", "dims"):
            self._check_names(self.records, state[key])
        for name, V in self.vocab.items():
            if int(state["dims"][name]) != self.dims[name]:
                raise ValueError(f"field {name!r}: stored width {state['dims'][name]}, these tables hold width "
                                 f"{self.dims[name]}")
            if int(state["vocab"][name]) != V:
                raise ValueError(f"field {name!r}: stored vocabulary {state['vocab'][name]}, the schema has {V}")
            _as_records(name, state["records"][name], V, self.row_bytes(name))
        for name, V in self.vocab.items():
            r = _as_records(name, state["records"][name], V, self.row_bytes(name))
            self.records[name].copy_(r.view(self.records[name].shape))

    def matches(self, model) -> Optional[str]:
        """Why these tables cannot serve ``model`` (None: they can).  A SPARSE or SEQUENCE field of the model without
        records is served in fp32."""
        fields = model.schema.fields
        for name in self.records:
            spec = fields.get(name)
            if spec is None:
                return f"records for {name!r}, which is no field of the model's schema"
            if spec.feature_type is FeatureType.DENSE:
                return f"records for {name!r}, which is a DENSE field of the model's schema"
            if spec.embedding_dim != self.dims[name]:
                return f"field {name!r}: records of width {self.dims[name]}, the schema has width {spec.embedding_dim}"
            if spec.vocabulary_size != self.vocab[name]:
                return f"field {name!r}: {self.vocab[name]} records, the schema has {spec.vocabulary_size} ids"
        return None
