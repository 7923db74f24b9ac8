"""Packed columnar batches: the input side of the hot path.

The reference feeds its models through ``TabularDataset`` + ``DataLoader`` + one ``.to(device)`` per
field (``deepfm/data/dataset.py:28-38``, ``deepfm/training/trainer.py:202-217``): a Python dict of
0-d tensors per SAMPLE, collated per batch — 3.8 K samples/s on 8 cores, four orders
of magnitude below the GPU step.  This module keeps the same data contract (a dict of per-field
numpy columns + a label column, int64 ids / float32 values) but moves batches as ONE record:

    record = [ ids (S, B) int64 | dense (Dn, B) float32 | labels (B) float32 | bags ]      (uint8 view)

S and Dn are at least 1; ``bags`` is one 16-byte-aligned (B, max_length) int64 block per SEQUENCE field, in schema
order, and empty for a uniform schema (the training record).

``RecordLayout``        the one description of a record: offsets, size, typed views of a host or device buffer,
                        the host writes (a contiguous slice with a padding tail; shuffled indices) and the
                        dict view.  Everything below, the training step and the predictors build on it;
``PackedColumns``       the dataset re-laid out once, column-major, in schema order;
``PackedBatchLoader``   host iterator of batch records (shuffle / drop_last like ``DataLoader``),
                        written straight into pinned staging slots: three fancy-index gathers
                        (or three memcpys without shuffle) per batch instead of B x F tensor objects;
``DeviceBatchRing``     H2D on a copy stream into a ring of device records, overlapped with the
                        previous steps; ``RowSparseTrainStep.run_from(record)`` consumes a record
                        directly (the gather reads it and refreshes the step's static inputs);
``unpack_record``       the reference's ``dict[str, Tensor]`` view of a record, for code that calls
                        ``model(batch)``.
The loader and the ring take any schema: a uniform one gives the row-sparse step's training record, one with SEQUENCE
fields the mixed record ``FusedMixedDeepFMStep.run_from`` and ``MixedSchemaPredictor.predict_from`` read;
``PackedColumns`` holds the SEQUENCE bags in ``columns.bags``.  ``record_layout`` / ``mixed_record_layout`` return the layout as plain tuples.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch

from deepfm_amd.data.schema import DatasetSchema, FeatureType


def _typed(buf, start: int, end: int, dtype: str, shape):
    """``buf[start:end]`` (uint8, numpy array or torch tensor, host or device) as a ``dtype`` view of ``shape``."""
    if isinstance(buf, torch.Tensor):
        return buf[start:end].view(getattr(torch, dtype)).view(shape)
    return buf[start:end].view(dtype).reshape(shape)


@dataclass(frozen=True)
class RecordLayout:
    """Where everything lies in one batch record of ``batch_size`` samples of a schema (module docstring).  The ids
    and dense blocks always hold at least one row, so no block of a record is empty."""

    batch_size: int
    n_sparse: int
    n_dense: int
    id_rows: int                           # rows of the ids / dense blocks: at least one each
    dense_rows: int
    ids_offset: int
    dense_offset: int
    labels_offset: int
    names: Tuple[str, ...]                 # per field, schema order:
    kinds: Tuple[FeatureType, ...]
    field_offsets: Tuple[int, ...]         # byte offset of the field's column (SEQUENCE: its block)
    seq_offsets: Tuple[int, ...]           # per SEQUENCE field, schema order
    seq_lengths: Tuple[int, ...]
    record_bytes: int

    @classmethod
    def of(cls, schema: DatasetSchema, batch_size: int, sequences: bool = True) -> "RecordLayout":
        """The layout of ``schema``; ``sequences=False`` is the training record, which refuses SEQUENCE fields."""
        B = batch_size
        specs = list(schema.fields.values())
        kinds = tuple(s.feature_type for s in specs)
        if not sequences and FeatureType.SEQUENCE in kinds:
            raise NotImplementedError("packed records hold SPARSE and DENSE fields only")
        ns = sum(k is FeatureType.SPARSE for k in kinds)
        nd = sum(k is FeatureType.DENSE for k in kinds)
        id_rows, dense_rows = max(ns, 1), max(nd, 1)       # at least one slot of each kind: said here only
        o1 = id_rows * B * 8
        o2 = o1 + dense_rows * B * 4
        end = o2 + B * 4
        offsets, seq, lengths, si, di = [], [], [], 0, 0
        for s in specs:
            if s.feature_type is FeatureType.SPARSE:
                offsets.append(si * B * 8); si += 1
            elif s.feature_type is FeatureType.DENSE:
                offsets.append(o1 + di * B * 4); di += 1
            else:
                off = (end + 15) // 16 * 16
                offsets.append(off); seq.append(off); lengths.append(s.max_length)
                end = off + B * s.max_length * 8
        return cls(B, ns, nd, id_rows, dense_rows, 0, o1, o2, tuple(schema.fields), kinds, tuple(offsets), tuple(seq), tuple(lengths), end)

    def views(self, buf):
        """(ids (>= 1, B) int64, dense (>= 1, B) float32, labels (B) float32, bags [(B, L) int64]) views of a
        record's bytes: a uint8 numpy array or torch tensor, on the host or the device."""
        B, o1, o2 = self.batch_size, self.dense_offset, self.labels_offset
        return (_typed(buf, self.ids_offset, o1, "int64", (self.id_rows, B)),
                _typed(buf, o1, o2, "float32", (self.dense_rows, B)),
                _typed(buf, o2, o2 + 4 * B, "float32", (B,)),
                [_typed(buf, off, off + B * L * 8, "int64", (B, L)) for off, L in zip(self.seq_offsets, self.seq_lengths)])

    def write(self, out: np.ndarray, columns: "PackedColumns", start: int, end: int) -> None:
        """Samples [start, end) of ``columns`` into the host record ``out``; rows past ``end - start`` are padding:
        id 0, value 0, label 0, all-padding bags."""
        cnt = end - start
        if not 0 < cnt <= self.batch_size:
            raise ValueError(f"{cnt} samples for a record of {self.batch_size}")
        ids, dense, labels, bags = self.views(out)
        if self.n_sparse:
            ids[:, :cnt] = columns.ids[:, start:end]
        if self.n_dense:
            dense[:, :cnt] = columns.dense[:, start:end]
        labels[:cnt] = columns.labels[start:end]
        for blk, bag in zip(bags, columns.bags):
            blk[:cnt] = bag[start:end]
        if cnt < self.batch_size:
            ids[:, cnt:] = 0
            dense[:, cnt:] = 0
            labels[cnt:] = 0
            for blk in bags:
                blk[cnt:] = 0

    def write_indexed(self, out: np.ndarray, columns: "PackedColumns", idx: np.ndarray) -> None:
        """Samples ``idx`` (``batch_size`` of them) of ``columns`` into the host record ``out``: gathers straight
        into the record, no temporaries."""
        ids, dense, labels, bags = self.views(out)
        if self.n_sparse:
            np.take(columns.ids, idx, axis=1, out=ids)
        if self.n_dense:
            np.take(columns.dense, idx, axis=1, out=dense)
        np.take(columns.labels, idx, out=labels)
        for blk, bag in zip(bags, columns.bags):
            np.take(bag, idx, axis=0, out=blk)

    def unpack(self, record):
        """(batch dict, labels) views of one record (numpy or torch): SEQUENCE fields (B, max_length)."""
        B, batch, lengths = self.batch_size, {}, iter(self.seq_lengths)
        for name, kind, off in zip(self.names, self.kinds, self.field_offsets):
            if kind is FeatureType.SPARSE:
                batch[name] = _typed(record, off, off + 8 * B, "int64", (B,))
            elif kind is FeatureType.DENSE:
                batch[name] = _typed(record, off, off + 4 * B, "float32", (B,))
            else:
                L = next(lengths)
                batch[name] = _typed(record, off, off + B * L * 8, "int64", (B, L))
        return batch, _typed(record, self.labels_offset, self.labels_offset + 4 * B, "float32", (B,))


def record_layout(schema: DatasetSchema, batch_size: int) -> Tuple[int, int, int, int, int]:
    """(n_sparse, n_dense, dense_offset, labels_offset, record_bytes) of a training record
    (``RowSparseTrainStep.pack_batches``); a SEQUENCE schema raises ``NotImplementedError``."""
    lay = RecordLayout.of(schema, batch_size, sequences=False)
    return lay.n_sparse, lay.n_dense, lay.dense_offset, lay.labels_offset, lay.record_bytes


def mixed_record_layout(schema: DatasetSchema, batch_size: int) -> Tuple[int, int, int, int, List[int], int]:
    """(n_sparse, n_dense, dense_offset, labels_offset, sequence_offsets, record_bytes) of a record of any schema."""
    lay = RecordLayout.of(schema, batch_size)
    return lay.n_sparse, lay.n_dense, lay.dense_offset, lay.labels_offset, list(lay.seq_offsets), lay.record_bytes


def unpack_mixed_record(schema: DatasetSchema, record: np.ndarray, batch_size: int) -> Tuple[Dict[str, np.ndarray], np.ndarray]:
    """(batch dict, labels) views of a host record of any schema: SEQUENCE fields (B, max_length)."""
    lay = RecordLayout.of(schema, batch_size)
    rec = np.asarray(record).view(np.uint8).reshape(-1)
    if rec.size != lay.record_bytes:
        raise ValueError("not a mixed record of this schema / batch size")
    return lay.unpack(rec)


def write_mixed_record(out: np.ndarray, columns: "PackedColumns", batch_size: int, start: int, end: int) -> None:
    """``RecordLayout.write`` for a caller without a layout: samples [start, end) of ``columns`` into ``out``."""
    RecordLayout.of(columns.schema, batch_size).write(out, columns, start, end)


class PackedColumns:
    """The whole dataset as two column-major matrices + labels, in schema order; SEQUENCE fields as
    ``bags``: one (n, max_length) int64 matrix per field, schema order."""

    def __init__(self, schema: DatasetSchema, features: Dict[str, np.ndarray], labels: np.ndarray) -> None:
        self.schema = schema
        n = len(labels)
        sparse, dense, bags = [], [], []
        for name, spec in schema.fields.items():
            col = np.asarray(features[name])                 # KeyError for a missing field, like the reference
            if spec.feature_type is FeatureType.SEQUENCE:
                if col.shape != (n, spec.max_length):
                    raise ValueError(f"SEQUENCE field {name!r}: expected shape ({n}, {spec.max_length}), got {col.shape}")
                if not np.issubdtype(col.dtype, np.integer):
                    raise TypeError(f"SEQUENCE field {name!r} needs integer ids, got {col.dtype}")
                bags.append(np.ascontiguousarray(col, dtype=np.int64))
                continue
            if col.shape != (n,):
                raise ValueError(f"field {name!r}: expected shape ({n},), got {col.shape}")
            if spec.feature_type is FeatureType.SPARSE:
                if not np.issubdtype(col.dtype, np.integer):
                    raise TypeError(f"SPARSE field {name!r} needs integer ids, got {col.dtype}")
                sparse.append(col.astype(np.int64, copy=False))
            else:
                dense.append(col.astype(np.float32, copy=False))
        self.ids = np.ascontiguousarray(np.stack(sparse)) if sparse else np.zeros((0, n), np.int64)
        self.dense = np.ascontiguousarray(np.stack(dense)) if dense else np.zeros((0, n), np.float32)
        self.bags: List[np.ndarray] = bags
        self.labels = np.ascontiguousarray(np.asarray(labels, dtype=np.float32))
        self.n = n

    def __len__(self) -> int:
        return self.n


class PackedBatchLoader:
    """Host-side batch records.  ``write(slot_bytes, k)`` fills a caller-owned (pinned) buffer with
    batch ``k`` of the current epoch; iteration order is re-drawn by ``set_epoch``."""

    def __init__(self, columns: PackedColumns, batch_size: int, shuffle: bool = False, drop_last: bool = True,
                 seed: int = 0) -> None:
        if not drop_last:
            raise NotImplementedError("the captured step has a fixed batch size: drop_last must be True")
        if batch_size <= 0 or batch_size > len(columns):
            raise ValueError("batch_size must be in [1, len(dataset)]")
        self.columns, self.batch_size, self.shuffle, self.seed = columns, batch_size, shuffle, seed
        self.layout = RecordLayout.of(columns.schema, batch_size)      # any schema: SEQUENCE bags travel as blocks
        self.record_bytes = self.layout.record_bytes
        self.num_batches = len(columns) // batch_size
        self.set_epoch(0)

    def set_epoch(self, epoch: int) -> None:
        n = len(self.columns)
        self.order = np.random.default_rng(self.seed + epoch).permutation(n) if self.shuffle else None

    def __len__(self) -> int:
        return self.num_batches

    def write(self, out: np.ndarray, k: int) -> None:
        """out: uint8 array of record_bytes (e.g. a numpy view of a pinned torch tensor)."""
        B = self.batch_size
        if not 0 <= k < self.num_batches:
            raise IndexError(k)
        if self.order is None:
            self.layout.write(out, self.columns, k * B, (k + 1) * B)
        else:
            self.layout.write_indexed(out, self.columns, self.order[k * B:(k + 1) * B])


def unpack_record(schema: DatasetSchema, record: torch.Tensor, batch_size: int) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """(batch dict, labels) views of one training record — the reference's ``model(batch)`` contract."""
    lay = RecordLayout.of(schema, batch_size, sequences=False)
    if record.numel() != lay.record_bytes or record.dtype != torch.uint8:
        raise ValueError("not a packed record of this schema / batch size")
    return lay.unpack(record)


class DeviceBatchRing:
    """Host -> device staging of batch records, overlapped with compute.

    ``depth`` pinned host slots and ``depth`` device records; batch k+depth-1 is packed and copied
    (copy stream) while batch k trains.  Iterating yields device records in order; a record stays
    valid until ``depth - 1`` further records have been requested (the consumer's work on it must
    have been ENQUEUED on the current stream by then, which ``step.run_from`` guarantees)."""

    def __init__(self, loader: PackedBatchLoader, device: torch.device, depth: int = 4) -> None:
        if depth < 2:
            raise ValueError("depth must be at least 2")
        self.loader, self.depth = loader, depth
        nbytes = (loader.record_bytes + 255) // 256 * 256          # records stay 256-byte aligned
        self.host = torch.empty(depth, nbytes, dtype=torch.uint8).pin_memory()
        self.host_np = [self.host[i].numpy() for i in range(depth)]
        self.dev = torch.empty(depth, nbytes, dtype=torch.uint8, device=device)
        self.copy_stream = torch.cuda.Stream(device=device)
        self.ready = [torch.cuda.Event() for _ in range(depth)]    # H2D of the slot has finished
        self.free = [torch.cuda.Event() for _ in range(depth)]     # consumers of the slot have finished
        self.copied = [torch.cuda.Event() for _ in range(depth)]   # host slot may be rewritten
        self._used = [False] * depth

    def _submit(self, k: int) -> None:
        slot = k % self.depth
        if self._used[slot]:
            self.copied[slot].synchronize()                         # the previous H2D out of this host slot is done
        self.loader.write(self.host_np[slot][:self.loader.record_bytes], k)
        with torch.cuda.stream(self.copy_stream):
            if self._used[slot]:
                self.copy_stream.wait_event(self.free[slot])        # the device slot is no longer being read
            self.dev[slot].copy_(self.host[slot], non_blocking=True)
            self.copied[slot].record(self.copy_stream)
            self.ready[slot].record(self.copy_stream)
        self._used[slot] = True

    def __iter__(self) -> Iterator[torch.Tensor]:
        n = len(self.loader)
        cur = torch.cuda.current_stream()
        for k in range(min(self.depth - 1, n)):
            self._submit(k)
        for k in range(n):
            if k + self.depth - 1 < n:
                # slot of batch k+depth-1 == slot of batch k-1: its consumer was enqueued one iteration ago
                prev = (k - 1) % self.depth
                if k >= 1:
                    self.free[prev].record(cur)
                self._submit(k + self.depth - 1)
            slot = k % self.depth
            cur.wait_event(self.ready[slot])
            yield self.dev[slot][:self.loader.record_bytes]
