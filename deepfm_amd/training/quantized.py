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
(``training/predict.py``) serves from them and never reads the fp32 tables again.  The quantiser, its inverse and the
gather are HIP kernels (``csrc/quant.hip``); tables built by ``from_records`` may sit on the host (files, checks), but
``dequantized()`` and the predictor need them on the device.
"""

from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from deepfm_amd import _lib
from deepfm_amd.data.schema import DatasetSchema, FeatureType
from deepfm_amd.training.eligibility import ineligible_reason

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
        out = {}
        for name, V in vocab.items():
            r = records[name]
            t = r if isinstance(r, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(r))
            if t.dtype != torch.uint8 or t.numel() != V * rb:
                raise ValueError(f"field {name!r}: expected {V} x {rb} uint8 bytes, got {tuple(t.shape)} {t.dtype}")
            out[name] = t.contiguous().view(V, rb)
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
        emb = self._model.embedding
        lib = _lib.load()
        names = list(self.vocab)
        dev = self.device
        if self._flags is None or self._flags.device != dev:
            self._flags = torch.zeros(max(len(names), 1), dtype=torch.int32, device=dev)
        self._flags.zero_()
        st = _lib.stream_handle()
        for i, name in enumerate(names):
            w2 = emb.second_order_embeddings[name].weight
            w1 = emb.first_order_embeddings[name].weight
            V = self.vocab[name]
            if w2.shape[0] != V:
                raise ValueError(f"the embedding table of field {name!r} is released: call restore_tables() first")
            for p in (w2, w1):
                _lib.require_device(p, f"table of field {name!r}")
                if p.dtype != torch.float32 or p.dim() != 2 or (p.shape[1] > 1 and p.stride(1) != 1):
                    raise TypeError("embedding tables must be float32 with contiguous rows")
            _lib.check(lib.dfm_quantize_rows(w2.data_ptr(), w2.stride(0), w1.data_ptr(), w1.stride(0), V, self.dim,
                                             FORMATS[self.format], self.records[name].data_ptr(),
                                             self._flags.data_ptr() + 4 * i, st))
        if check and names:
            flags = self._flags.cpu().tolist()
            for name, flag in zip(names, flags):
                if flag:
                    raise ValueError(f"the embedding table of field {name!r} has a non-finite element or a row whose "
                                     f"range overflows the {self.format} format: it cannot be quantised")
        return self

    def dequantized(self) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """``{field: (w2 (V, D), w1 (V, 1))}`` as fp32, by ``dfm_dequantize_rows``."""
        lib = _lib.load()
        out = {}
        for name, rec in self.records.items():
            _lib.require_device(rec, f"records of field {name!r}")
            V = self.vocab[name]
            w2 = torch.empty(V, self.dim, dtype=torch.float32, device=rec.device)
            w1 = torch.empty(V, 1, dtype=torch.float32, device=rec.device)
            _lib.check(lib.dfm_dequantize_rows(rec.data_ptr(), V, self.dim, FORMATS[self.format], w2.data_ptr(),
                                               w1.data_ptr(), _lib.stream_handle()))
            out[name] = (w2, w1)
        return out

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
        out = {}
        half = torch.float32 if self.format == "int8" else torch.float16
        for name, rec in self.records.items():
            head = rec[:, :2 * half.itemsize].contiguous().view(half).double()
            scale, lo = head[:, 0], head[:, 1]
            hi = lo + _LEVELS[self.format] * scale
            bound = scale / 2 + 2.0 ** -21 * torch.maximum(lo.abs(), hi.abs())
            out[name] = float(bound.max()) if bound.numel() else 0.0
        return out

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
            r = state["records"][name]
            r = r if isinstance(r, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(r))
            if r.dtype != torch.uint8 or r.numel() != V * self.row_bytes:
                raise ValueError(f"field {name!r}: expected {V} x {self.row_bytes} uint8 bytes, got "
                                 f"{tuple(r.shape)} {r.dtype}")
        for name in self.vocab:
            r = state["records"][name]
            r = r if isinstance(r, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(r))
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
