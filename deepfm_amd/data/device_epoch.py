"""An epoch's input side on the device: per-epoch training negatives and batch records without a
per-step host gather or host-to-device copy.

The reference re-draws its training negatives every epoch (``deepfm/data/movielens.py:136-141, 532-565``: a pandas
row loop with ``random.sample`` over the user's unseen movies) and batches through a ``DataLoader``.  Here the
positives, an item table and the per-user seen-sets are uploaded once; ``dfm_sample_negatives`` draws an epoch's
negatives and ``dfm_record_assemble`` forms every batch record in ``RecordLayout``'s byte format
(``csrc/sampler.hip``), so ``run_from(record)`` / ``predict_from(record)`` consume them unchanged.

``DeviceColumns``      a ``PackedColumns`` uploaded once: ids (S, n), dense (Dn, n), labels, bags;
``SeenSets``           per-user bitmap of seen item rows + zero-count prefix table, built once on the host;
``ItemTable``          the columns of the ITEM fields over the item rows;
``BucketDifference``   a SPARSE field that depends on the (positive, item) pair (``movie_age_at_rating``);
``CandidateSource``    what the loader needs of a source of K candidate item rows per positive;
``NegativeSampler``    the K negatives per positive of an epoch, drawn on the device (``data/candidates.py`` has the
                       evaluation sources: weighted negatives and the whole catalogue);
``DeviceEpochLoader``  iterator of device batch records over the epoch's P * (1 + K) virtual rows.

An epoch's virtual rows: row j < P is positive j; row j >= P is negative t = (j - P) % K of positive p = (j - P) // K,
label 0, every column by its role.  With ``short_users="truncate"`` a user with fewer unseen rows than K gets
``min(K, unseen)`` candidates, as in the reference (``movielens.py:575-580``): the list is then ragged, ``counts[p]``
candidates of positive p from ``offsets[p]`` on in a flat ``neg_items``, and the epoch has P + ``total_candidates``
rows, row j >= P being candidate j - P of that list.  Nothing here needs the GPU at import time; the host-side checks
run without one.
"""

from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from deepfm_amd import _lib
from deepfm_amd.data.packed import PackedColumns, RecordLayout
from deepfm_amd.data.schema import DatasetSchema, FeatureType

SEEN_SETS_MAX_BYTES = 1 << 30     # bitmap + prefix; a larger catalogue needs another structure
_POPCOUNT8 = np.array([bin(b).count("1") for b in range(256)], np.uint8)
_KIND = {FeatureType.SPARSE: _lib.SPARSE, FeatureType.DENSE: _lib.DENSE, FeatureType.SEQUENCE: _lib.SEQUENCE}


class Role(enum.IntEnum):
    """How a negative row's column is filled (``enum dfm_assemble_role``)."""

    COPY = _lib.ROLE_COPY                   # the positive's value: user and context fields
    ITEM = _lib.ROLE_ITEM                   # the sampled item's row of the item table
    BUCKET_DIFF = _lib.ROLE_BUCKET_DIFF     # a ``BucketDifference``


class DeviceColumns:
    """``PackedColumns`` on ``device``, uploaded once."""

    def __init__(self, columns: PackedColumns, device) -> None:
        self.schema: DatasetSchema = columns.schema
        self.device = torch.device(device)
        self.n = len(columns)
        self.ids = torch.from_numpy(columns.ids).to(self.device)            # (S, n) int64
        self.dense = torch.from_numpy(columns.dense).to(self.device)        # (Dn, n) float32
        self.labels = torch.from_numpy(columns.labels).to(self.device)      # (n,) float32
        self.bags = [torch.from_numpy(b).to(self.device) for b in columns.bags]

    @classmethod
    def from_device(cls, schema: DatasetSchema, ids: torch.Tensor, dense: torch.Tensor, labels: torch.Tensor,
                    bags=()) -> "DeviceColumns":
        """Columns that are on the device already (``data/encoders.py`` writes them there): ids (S, n) int64, dense
        (Dn, n) float32, labels (n,) float32 and one (n, max_length) int64 bag per SEQUENCE field, schema order, all
        contiguous on one device.  Nothing is copied.  A bag may be a ``HistoryBag`` (``data/interactions.py``) of n
        queries and ``max_length`` ids instead of the tensor: the loader then forms that field's bags from the history
        index, batch by batch, and ``field_columns()`` returns the object."""
        from deepfm_amd.data.interactions import HistoryBag, _same_device        # (interactions imports this module)
        n, bags = labels.shape[0], list(bags)
        want = [("ids", ids, torch.int64, (len(schema.sparse_fields), n)),
                ("dense", dense, torch.float32, (len(schema.dense_fields), n)),
                ("labels", labels, torch.float32, (n,))]
        if len(bags) != len(schema.sequence_fields):
            raise ValueError(f"{len(bags)} bags for {len(schema.sequence_fields)} SEQUENCE fields")
        for s, b in zip(schema.sequence_fields, bags):
            if not isinstance(b, HistoryBag):
                want.append((f"bag of {s.name!r}", b, torch.int64, (n, s.max_length)))
            elif len(b) != n or b.length != s.max_length or not _same_device(b.device, labels.device):
                raise ValueError(f"bag of {s.name!r}: expected a HistoryBag of {n} queries and length {s.max_length} on "
                                 f"{labels.device}, got {len(b)} queries and length {b.length} on {b.device}")
        for what, t, dtype, shape in want:
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != labels.device:
                raise ValueError(f"{what}: expected a contiguous {dtype} tensor of shape {shape} on {labels.device}, "
                                 f"got {t.dtype} {tuple(t.shape)} on {t.device}")
        self = cls.__new__(cls)
        self.schema, self.device, self.n = schema, labels.device, n
        self.ids, self.dense, self.labels, self.bags = ids, dense, labels, bags
        return self

    def __len__(self) -> int:
        return self.n

    def field_columns(self) -> Dict[str, torch.Tensor]:
        """Per field, schema order: its (n,) / (n, L) column (a view), or its ``HistoryBag``."""
        out, si, di, qi = {}, 0, 0, 0
        for name, spec in self.schema.fields.items():
            if spec.feature_type is FeatureType.SPARSE:
                out[name] = self.ids[si]; si += 1
            elif spec.feature_type is FeatureType.DENSE:
                out[name] = self.dense[di]; di += 1
            else:
                out[name] = self.bags[qi]; qi += 1
        return out


class SeenSets:
    """Per user, the item rows it has interacted with: ``bitmap`` (n_users, W) uint32 with W = ceil(n_items / 32)
    (bit i of user u set = seen; the bits at and above n_items are set) and ``prefix`` (n_users, W + 1) uint32
    (``prefix[u][w]`` = zero bits in words < w, so ``prefix[u][W]`` is the user's unseen count).  Both are built
    once on the host: they do not change between epochs."""

    def __init__(self, bitmap: np.ndarray, prefix: np.ndarray, n_users: int, n_items: int) -> None:
        self.bitmap, self.prefix, self.n_users, self.n_items = bitmap, prefix, n_users, n_items
        self.words = bitmap.shape[1]

    @classmethod
    def from_interactions(cls, user_rows, item_rows, n_users: int, n_items: int) -> "SeenSets":
        if n_users < 1 or n_items < 1:
            raise ValueError("n_users and n_items must be positive")
        W = (n_items + 31) // 32
        nbytes = 4 * n_users * (2 * W + 1)
        if nbytes > SEEN_SETS_MAX_BYTES:
            raise ValueError(f"seen-set bitmap + prefix of {n_users} users x {n_items} items take {nbytes} bytes, "
                             f"more than {SEEN_SETS_MAX_BYTES}: a catalogue this large needs another structure")
        u = np.asarray(user_rows, dtype=np.int64).reshape(-1)
        i = np.asarray(item_rows, dtype=np.int64).reshape(-1)
        if u.shape != i.shape:
            raise ValueError("user_rows and item_rows differ in length")
        if u.size and (u.min() < 0 or u.max() >= n_users or i.min() < 0 or i.max() >= n_items):
            raise ValueError("an interaction names a user or an item row outside the tables")
        bitmap = np.zeros((n_users, W), np.uint32)
        if n_items % 32:
            bitmap[:, W - 1] = np.uint32((0xFFFFFFFF << (n_items % 32)) & 0xFFFFFFFF)
        np.bitwise_or.at(bitmap, (u, i >> 5), (np.uint32(1) << (i & 31).astype(np.uint32)))
        ones = _POPCOUNT8[bitmap.view(np.uint8)].reshape(n_users, W, 4).sum(axis=2, dtype=np.uint32)
        zeros = np.uint32(32) - ones
        prefix = np.zeros((n_users, W + 1), np.uint32)
        np.cumsum(zeros, axis=1, dtype=np.uint32, out=prefix[:, 1:])
        return cls(bitmap, prefix, n_users, n_items)

    @property
    def unseen(self) -> np.ndarray:
        """(n_users,) unseen item rows per user."""
        return self.prefix[:, self.words]

    def upload(self, device):
        """(bitmap, prefix) on ``device`` as int32 tensors of the same bits."""
        return (torch.from_numpy(self.bitmap.view(np.int32)).to(device),
                torch.from_numpy(self.prefix.view(np.int32)).to(device))


class ItemTable:
    """The columns, over the item rows, of the fields a negative takes from its item: SPARSE (n_items,) int64,
    DENSE (n_items,) float32, SEQUENCE (n_items, max_length) int64."""

    def __init__(self, schema: DatasetSchema, features: Dict[str, np.ndarray]) -> None:
        self.schema, self.columns, self.n_items = schema, {}, None
        for name, col in features.items():
            if name not in schema.fields:
                raise KeyError(f"item table column {name!r} is not a field of the schema")
            spec, col = schema.fields[name], np.asarray(col)
            n = col.shape[0] if col.ndim else 0
            if self.n_items is None:
                self.n_items = n
            want = (self.n_items, spec.max_length) if spec.feature_type is FeatureType.SEQUENCE else (self.n_items,)
            if col.shape != want:
                raise ValueError(f"item table column {name!r}: expected shape {want}, got {col.shape}")
            if spec.feature_type is FeatureType.DENSE:
                self.columns[name] = np.ascontiguousarray(col, dtype=np.float32)
            else:
                if not np.issubdtype(col.dtype, np.integer):
                    raise TypeError(f"item table column {name!r} needs integer ids, got {col.dtype}")
                self.columns[name] = np.ascontiguousarray(col, dtype=np.int64)
        if not self.n_items:
            raise ValueError("an item table needs at least one column of at least one row")


@dataclass
class BucketDifference:
    """A SPARSE field of a negative that depends on the pair: d = ctx[p] - item_val[item] in float32; bucket 0 if
    either operand is NaN or d < 0, else 1 + #{e in edges : e <= d}; the id written is ``bucket_ids[bucket]``."""

    ctx: np.ndarray           # (P,) float32, per positive
    item_val: np.ndarray      # (n_items,) float32, per item row
    edges: np.ndarray         # (E,) float32, ascending, E <= 64
    bucket_ids: np.ndarray    # (E + 2,) int64

    def __post_init__(self) -> None:
        self.ctx = np.ascontiguousarray(self.ctx, dtype=np.float32)
        self.item_val = np.ascontiguousarray(self.item_val, dtype=np.float32)
        self.edges = np.ascontiguousarray(self.edges, dtype=np.float32)
        self.bucket_ids = np.ascontiguousarray(self.bucket_ids, dtype=np.int64)
        if self.ctx.ndim != 1 or self.item_val.ndim != 1 or self.edges.ndim != 1:
            raise ValueError("BucketDifference: ctx, item_val and edges are vectors")
        if self.edges.size > _lib.MAX_BUCKET_EDGES or (np.diff(self.edges) < 0).any():
            raise ValueError(f"BucketDifference: at most {_lib.MAX_BUCKET_EDGES} edges, ascending")
        if self.bucket_ids.shape != (self.edges.size + 2,):
            raise ValueError(f"BucketDifference: {self.edges.size} edges need {self.edges.size + 2} bucket ids")


def default_roles(schema: DatasetSchema) -> Dict[str, Role]:
    """ITEM for the fields of group "item", COPY otherwise: the reference's grouping of the MovieLens schema
    (``movielens.py:346-418``)."""
    return {name: Role.ITEM if spec.group == "item" else Role.COPY for name, spec in schema.fields.items()}


def resolve_roles(columns: "DeviceColumns", items: ItemTable, roles, derived) -> Dict[str, Role]:
    """The role of every field for a candidate row, checked: ``default_roles`` overridden by ``roles``, BUCKET_DIFF
    for the ``derived`` fields.  The one statement of the role / derived-field rules of every candidate source."""
    schema = columns.schema
    out = dict(default_roles(schema), **{k: Role(v) for k, v in (roles or {}).items()})
    for name, bd in (derived or {}).items():
        if name not in schema.fields or schema.fields[name].feature_type is not FeatureType.SPARSE:
            raise ValueError(f"derived field {name!r} is not a SPARSE field of the schema")
        if bd.ctx.shape != (len(columns),) or bd.item_val.shape != (items.n_items,):
            raise ValueError(f"derived field {name!r}: ctx is per positive and item_val per item row")
        out[name] = Role.BUCKET_DIFF
    for name, role in out.items():
        if name not in schema.fields:
            raise ValueError(f"role given for {name!r}, which is not a field of the schema")
        if role is Role.ITEM and name not in items.columns:
            raise ValueError(f"field {name!r} has role ITEM but the item table has no column for it")
        if role is Role.BUCKET_DIFF and name not in (derived or {}):
            raise ValueError(f"field {name!r} has role BUCKET_DIFF but no BucketDifference")
    return out


SHORT_USERS = ("refuse", "truncate")


def tail_rows(rows: int, batch_size: int) -> int:
    """Rows of an epoch behind its last whole batch: ``rows - (rows // batch_size) * batch_size``."""
    if batch_size <= 0 or rows < 0:
        raise ValueError("batch_size must be positive and rows non-negative")
    return rows - (rows // batch_size) * batch_size


def check_ragged(counts, offsets, num_queries: int, num_neg: int) -> int:
    """``total_candidates`` of a ragged list, or ``ValueError``: ``counts`` (Q,) within [0, num_neg] and ``offsets``
    (Q + 1,) its exclusive scan.  The one host-side statement of what the ragged kernels are handed."""
    counts, offsets = np.asarray(counts), np.asarray(offsets)
    if counts.shape != (num_queries,) or offsets.shape != (num_queries + 1,):
        raise ValueError(f"a ragged list of {num_queries} queries needs counts ({num_queries},) and offsets "
                         f"({num_queries + 1},), got {counts.shape} and {offsets.shape}")
    bad = np.flatnonzero((counts < 0) | (counts > num_neg))
    if bad.size:
        q = int(bad[0])
        raise ValueError(f"counts[{q}] = {int(counts[q])} outside [0, num_neg = {num_neg}]")
    scan = np.zeros(num_queries + 1, np.int64)
    np.cumsum(counts, dtype=np.int64, out=scan[1:])
    bad = np.flatnonzero(offsets != scan)
    if bad.size:
        q = int(bad[0])
        raise ValueError(f"offsets[{q}] = {int(offsets[q])} is not the exclusive scan of counts ({int(scan[q])})")
    return int(scan[-1])


class CandidateSource:
    """What ``DeviceEpochLoader`` uses of a source of candidate rows: ``columns`` (the P positives, or queries),
    at most ``num_neg`` candidates per positive, ``roles``, ``item_columns``, ``derived_dev``, ``neg_items`` int32
    item rows, ``seen`` and ``sample(epoch)``, which fills ``neg_items`` on the current stream.  A rectangular source
    has ``counts = offsets = None``, ``neg_items`` (P, num_neg) and ``total_candidates = P * num_neg``; a ragged one
    (``short_users="truncate"`` and at least one short user) has ``counts`` (P,) int32, ``offsets`` (P + 1,) int64,
    its exclusive scan, both uploaded once, and a flat ``neg_items`` (total_candidates,).  ``_list()`` is that shape as
    the C entry points take it.  Subclasses validate on the host (``_validate``), then ``_upload``."""

    def _validate(self, columns: DeviceColumns, seen: SeenSets, user_of, items: ItemTable, roles, derived) -> np.ndarray:
        user_of = np.ascontiguousarray(user_of, dtype=np.int32).reshape(-1)
        if user_of.shape != (len(columns),):
            raise ValueError(f"user_of has {user_of.size} entries for {len(columns)} positives")
        if user_of.min() < 0 or user_of.max() >= seen.n_users:
            raise ValueError("user_of names a user outside the seen-sets")
        if items.n_items != seen.n_items:
            raise ValueError(f"the item table has {items.n_items} rows, the seen-sets {seen.n_items} items")
        self.derived = dict(derived or {})
        self.roles = resolve_roles(columns, items, roles, self.derived)
        return user_of

    def _refuse_short_users(self, seen: SeenSets, user_of: np.ndarray, num_neg: int, why: str) -> None:
        users = np.unique(user_of)
        short = users[seen.unseen[users] < num_neg]
        if short.size:
            u = int(short[0])
            raise ValueError(f"user {u} has {int(seen.unseen[u])} unseen items, fewer than num_neg = {num_neg} ({why})")

    def _short_users(self, seen: SeenSets, user_of: np.ndarray, num_neg: int, short_users: str, why: str):
        """The per-query counts ``min(num_neg, unseen)`` of a truncating source that has a short user, else ``None``
        (a source nobody is short in is rectangular); ``"refuse"`` raises on the first short user."""
        if short_users == "refuse":
            self._refuse_short_users(seen, user_of, num_neg, why)
            return None
        counts = np.minimum(seen.unseen[user_of].astype(np.int64), num_neg).astype(np.int32)
        return counts if (counts < num_neg).any() else None

    def _upload(self, columns: DeviceColumns, seen: SeenSets, user_of: np.ndarray, items: ItemTable, num_neg: int,
                counts: Optional[np.ndarray] = None) -> None:
        self.columns, self.seen, self.items, self.num_neg = columns, seen, items, num_neg
        self.user_of_host = user_of
        dev = columns.device
        self.user_of = torch.from_numpy(user_of).to(dev)
        self.bitmap, self.prefix = seen.upload(dev)
        self.item_columns = {k: torch.from_numpy(v).to(dev) for k, v in items.columns.items()}
        self.derived_dev = {k: tuple(torch.from_numpy(a).to(dev) for a in (bd.ctx, bd.item_val, bd.edges, bd.bucket_ids))
                            for k, bd in self.derived.items()}
        self.counts_host, self.offsets_host, self.counts, self.offsets = counts, None, None, None
        self.total_candidates = len(columns) * num_neg
        self._candidate_list: Optional[_lib.CandidateList] = None
        if counts is None:
            self.neg_items = torch.zeros(len(columns), num_neg, dtype=torch.int32, device=dev)
        else:
            self.offsets_host = np.zeros(len(columns) + 1, np.int64)
            np.cumsum(counts, dtype=np.int64, out=self.offsets_host[1:])
            self.total_candidates = check_ragged(counts, self.offsets_host, len(columns), num_neg)
            self.counts, self.offsets = torch.from_numpy(counts).to(dev), torch.from_numpy(self.offsets_host).to(dev)
            self.neg_items = torch.zeros(self.total_candidates, dtype=torch.int32, device=dev)
            self._candidate_list = _lib.CandidateList(self.counts.data_ptr(), self.offsets.data_ptr(),
                                                      self.total_candidates)
        self.epoch: Optional[int] = None

    def _list(self) -> Optional[_lib.CandidateList]:
        """The source's ``dfm_candidate_list`` over ``counts`` / ``offsets`` (which it keeps alive), built once by
        ``_upload``; None for a rectangular source."""
        return self._candidate_list

    def _draw(self, epoch: int, out: torch.Tensor) -> None:
        raise NotImplementedError

    @staticmethod
    def _check_draw(epoch: int, out: torch.Tensor, what: str) -> None:
        _lib.require_device(out, what)
        if epoch < 0:
            raise ValueError("epoch must be non-negative")

    def sample(self, epoch: int) -> torch.Tensor:
        """Fill ``neg_items`` (int32; (P, num_neg), or flat when ragged) with the candidates of ``(seed, epoch)``, on
        the current stream."""
        self._draw(epoch, self.neg_items)
        self.epoch = epoch
        return self.neg_items

    def negatives_host(self, epoch: int) -> np.ndarray:
        """The item rows of ``epoch``, shaped like ``neg_items``, as numpy (tests, debugging); the current epoch's
        draw stays."""
        out = torch.empty_like(self.neg_items)
        self._draw(epoch, out)
        return out.cpu().numpy()


class NegativeSampler(CandidateSource):
    """``num_neg`` negatives per positive row of ``columns``, re-drawn per epoch on the device: distinct item rows
    the positive's user (``user_of``, (P,) user rows) has not seen, uniform without replacement
    (``dfm_sample_negatives``).  A user with fewer unseen rows than ``num_neg`` is refused
    (``short_users="refuse"``) or gets each of its unseen rows once (``"truncate"``: the reference's
    ``min(num_neg, unseen)``; the source is then ragged); a positive that is not short receives the same items
    either way.  Every check runs on the host, before anything touches the device."""

    def __init__(self, columns: DeviceColumns, seen: SeenSets, user_of, items: ItemTable, num_neg: int,
                 roles: Optional[Dict[str, Role]] = None, derived: Optional[Dict[str, BucketDifference]] = None,
                 seed: int = 0, short_users: str = "refuse") -> None:
        if short_users not in SHORT_USERS:
            raise ValueError(f"short_users = {short_users!r}: expected one of {SHORT_USERS}")
        if not 1 <= num_neg <= _lib.MAX_NEGATIVES:
            raise ValueError(f"num_neg = {num_neg} outside [1, {_lib.MAX_NEGATIVES}]")
        user_of = self._validate(columns, seen, user_of, items, roles, derived)
        counts = self._short_users(seen, user_of, num_neg, short_users,
                                   "a captured step needs a fixed count per positive")
        self.seed = seed
        self._upload(columns, seen, user_of, items, num_neg, counts)

    def _draw(self, epoch: int, out: torch.Tensor) -> None:
        self._check_draw(epoch, out, "the negatives")
        _lib.check(_lib.load().dfm_sample_negatives(
            self.bitmap.data_ptr(), self.prefix.data_ptr(), self.user_of.data_ptr(), len(self.columns),
            self.seen.n_users, self.seen.n_items, self.num_neg, self.seed & 0xFFFFFFFFFFFFFFFF, epoch, self._list(),
            out.data_ptr(), _lib.stream_handle()))


class DeviceEpochLoader:
    """Device batch records of an epoch over ``columns`` (+ ``negatives``): ``set_epoch(e)`` draws the negatives of
    ``(seed, e)`` and a device permutation of the P * (1 + K) virtual rows (P + ``total_candidates`` of a ragged
    source: the loader's length, its permutation and its trailing partial batch follow that count); iterating (or
    ``record(k)``) writes batch k into the next of ``depth`` 256-byte aligned device records with one
    ``dfm_record_assemble`` launch on the current stream.  ``DeviceBatchRing``'s contract: a record stays valid until ``depth - 1`` further records
    have been requested; its consumer must have been enqueued on the same stream by then.  Iteration has drop_last
    semantics; the ``tail_rows`` rows behind the last whole batch are ``tail()``: a record of its own, of ``tail_rows``
    samples (a fused step of that batch size trains on it: ``make_tail_step``).

    A SEQUENCE column that is a ``HistoryBag`` is never materialised: both plans are bound to its history index
    (``dfm_assemble_plan_bind_history``) and the launch forms each slot's bag from it, the same bytes as from the
    ``(n, max_length)`` block.  The plans hold raw pointers into the bag's queries and the index's tensors; the loader
    keeps them alive through ``self.columns``, so ``columns.bags`` must not be replaced while the loader is in use."""

    def __init__(self, columns: DeviceColumns, batch_size: int, shuffle: bool = True, seed: int = 0,
                 negatives: Optional[CandidateSource] = None, depth: int = 4) -> None:
        if depth < 2:
            raise ValueError("depth must be at least 2")
        if negatives is not None and negatives.columns is not columns:
            raise ValueError("the candidate source was built over other columns")
        self.columns, self.batch_size, self.shuffle, self.seed = columns, batch_size, shuffle, seed
        self.negatives, self.depth = negatives, depth
        self.num_neg = negatives.num_neg if negatives is not None else 0
        self.rows = len(columns) + (negatives.total_candidates if negatives is not None else 0)
        if batch_size <= 0 or batch_size > self.rows:
            raise ValueError("batch_size must be in [1, rows of an epoch]")
        self.layout = RecordLayout.of(columns.schema, batch_size)
        self.record_bytes = self.layout.record_bytes
        self.num_batches = self.rows // batch_size
        self.tail_rows = tail_rows(self.rows, batch_size)
        _lib.require_device(columns.labels, "the dataset")
        nbytes = (self.record_bytes + 255) // 256 * 256
        self.ring = torch.zeros(depth, nbytes, dtype=torch.uint8, device=columns.device)
        # the trailing partial batch: a record of tail_rows samples (offsets depend on the batch size), its own plan
        self.tail_layout = RecordLayout.of(columns.schema, self.tail_rows) if self.tail_rows else None
        self._plan = self._tail_plan = None
        self._create_plan()
        self._tail_record = (torch.zeros((self.tail_layout.record_bytes + 255) // 256 * 256, dtype=torch.uint8,
                                         device=columns.device) if self.tail_rows else None)
        self._next = 0
        self.order: Optional[torch.Tensor] = None
        self.set_epoch(0)

    def _create_plan(self) -> None:
        """Both assemble plans, once: the batches' and, beside it, the trailing partial batch's."""
        self._plan = self._plan_for(self.layout)
        self._tail_plan = self._plan_for(self.tail_layout) if self.tail_rows else None

    def _plan_for(self, lay: RecordLayout) -> C.c_void_p:
        """The assemble plan of records in ``lay``, plain or ragged as the source is.  A ``HistoryBag`` column hands
        the plan its queries as ``pos`` and is bound to its index right after the plan exists."""
        from deepfm_amd.data.interactions import HistoryBag                      # (interactions imports this module)
        cols, neg, plan = self.columns, self.negatives, C.c_void_p()
        descs = (_lib.AssembleColumn * len(lay.names))()
        bound = []
        for f, (d, (name, src), off) in enumerate(zip(descs, cols.field_columns().items(), lay.field_offsets)):
            spec = cols.schema.fields[name]
            d.kind, d.length, d.record_offset, d.pos = _KIND[spec.feature_type], spec.max_length, off, src.data_ptr()
            d.role = int(neg.roles[name]) if neg is not None else _lib.ROLE_COPY
            if isinstance(src, HistoryBag):
                if d.role != Role.COPY:
                    raise ValueError(f"field {name!r} is a HistoryBag with role {Role(d.role).name}: a history belongs "
                                     "to its positive, so a candidate row copies it (Role.COPY)")
                bound.append((f, src))
            if d.role == Role.ITEM:
                d.item = neg.item_columns[name].data_ptr()
            elif d.role == Role.BUCKET_DIFF:
                ctx, item_val, edges, ids = neg.derived_dev[name]
                d.ctx, d.item, d.edges, d.bucket_ids = ctx.data_ptr(), item_val.data_ptr(), edges.data_ptr(), ids.data_ptr()
                d.num_edges = edges.numel()
        # the list the kernels will index by is checked here, on the host, whatever built the source
        if neg is not None and neg.counts is not None and (
                check_ragged(neg.counts_host, neg.offsets_host, len(cols), self.num_neg) != neg.total_candidates or
                neg.neg_items.shape != (neg.total_candidates,)):
            raise ValueError(f"the source's neg_items {tuple(neg.neg_items.shape)} and total_candidates = "
                             f"{neg.total_candidates} are not those of its counts")
        _lib.check(_lib.load().dfm_assemble_plan_create(
            descs, len(descs), lay.batch_size, lay.id_rows, lay.dense_rows, lay.dense_offset, lay.labels_offset,
            lay.record_bytes, cols.labels.data_ptr(), len(cols), neg.seen.n_items if neg is not None else 0,
            self.num_neg, neg._list() if neg is not None else None, C.byref(plan)))
        for f, bag in bound:
            rc = _lib.load().dfm_assemble_plan_bind_history(plan, f, bag.source())
            if rc:                                          # nobody owns the plan yet
                _lib.load().dfm_assemble_plan_destroy(plan)
                _lib.check(rc)
        return plan

    def __del__(self) -> None:
        for attr in ("_plan", "_tail_plan"):
            plan = getattr(self, attr, None)
            if plan:
                setattr(self, attr, None)
                try:
                    _lib.load().dfm_assemble_plan_destroy(plan)
                except Exception:                  # interpreter shutdown: the process frees the device memory
                    pass

    def set_epoch(self, epoch: int) -> None:
        if self.negatives is not None:
            self.negatives.sample(epoch)
        if self.shuffle:
            gen = torch.Generator(device=self.columns.device).manual_seed(self.seed + epoch)
            self.order = torch.randperm(self.rows, generator=gen, device=self.columns.device)
        else:
            self.order = None
        self.epoch = epoch

    def __len__(self) -> int:
        return self.num_batches

    def assemble_into(self, out: torch.Tensor, first: int, count: int) -> None:
        """One launch: the virtual rows ``order[first : first + count]`` into the device record ``out``
        (``count <= batch_size``; the slots past ``count`` are padding)."""
        if out.numel() != self.record_bytes or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("assemble_into expects one contiguous batch record of this schema and batch size")
        _lib.require_device(out, "batch record")
        self._assemble(self._plan, first, count, out)

    def _assemble(self, plan: C.c_void_p, first: int, count: int, out: torch.Tensor) -> None:
        _lib.check(_lib.load().dfm_record_assemble(
            plan, _lib.ptr(self.order), first, count,
            self.negatives.neg_items.data_ptr() if self.negatives is not None else 0, out.data_ptr(),
            _lib.stream_handle()))

    def rows_into_next(self, first: int, count: int) -> torch.Tensor:
        """``assemble_into`` the next ring slot: the virtual rows ``order[first : first + count]``, e.g. the
        trailing partial batch of an evaluation or the candidate rows alone."""
        rec = self.ring[self._next][:self.record_bytes]
        self._next = (self._next + 1) % self.depth
        self.assemble_into(rec, first, count)
        return rec

    def record(self, k: int) -> torch.Tensor:
        """Batch ``k`` of the current epoch, written into the next ring slot."""
        if not 0 <= k < self.num_batches:
            raise IndexError(k)
        return self.rows_into_next(k * self.batch_size, self.batch_size)

    def __iter__(self) -> Iterator[torch.Tensor]:
        for k in range(self.num_batches):
            yield self.record(k)

    def tail(self) -> Optional[torch.Tensor]:
        """The trailing partial batch of the current epoch, the virtual rows ``order[num_batches * batch_size :
        rows]``, as a device record in ``RecordLayout.of(schema, tail_rows)`` (one ``dfm_record_assemble`` launch on
        the current stream into the loader's one tail record), or None when the rows divide evenly."""
        if not self.tail_rows:
            return None
        rec = self._tail_record[:self.tail_layout.record_bytes]
        self._assemble(self._tail_plan, self.num_batches * self.batch_size, self.tail_rows, rec)
        return rec

    def negatives_host(self, epoch: int) -> np.ndarray:
        """``CandidateSource.negatives_host``: the item rows of ``epoch`` as numpy, (P, K) or flat when ragged."""
        if self.negatives is None:
            raise ValueError("this loader has no candidate source")
        return self.negatives.negatives_host(epoch)
