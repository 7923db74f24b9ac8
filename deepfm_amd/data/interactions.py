"""The interaction log on the device: what the reference's adapter does between reading the ratings
and fitting the encoders (``deepfm/data/movielens.py:235-304, 334-344, 467-480``), over ``(user row, item row,
timestamp, label)`` columns that are on the device, with no per-row host work.

``DeviceInteractionLog``   the four columns; ``temporal_split`` and ``leave_one_out_split`` give an
                           ``InteractionSplit`` of int64 device index tensors into the log, ``seen_sets`` the per-user
                           seen-sets over all interactions, ``counts`` the per-user / per-item counts;
``DeviceSeenSets``         a ``SeenSets`` whose bitmap and prefix were built on the device (``dfm_seen_sets_build``)
                           and stay there; the candidate sources take it unchanged;
``quantile_cutoff``        the float64 value ``pandas.Series.quantile`` gives, from two order statistics;
``popularity_weights``     ``item_weights`` of a device count vector;
``count_feature_table``    the reference's ``user_rating_count`` / ``item_rating_count`` feature per entity;
``DeviceHistoryIndex``     ``log.history_index(...)``: per log row (``lookup``) or per user (``latest``), the items the
                           user interacted with before, latest first, as a ``UserHistory`` of device tensors whose
                           ``bag`` is a SEQUENCE column of ``DeviceColumns.from_device``; ``history_field`` is its
                           schema entry;
``HistoryBag``             that SEQUENCE column without the ``(n, length)`` block: the queries and the index, bound to
                           the record assembly, which forms each batch's bags in its one launch.

Rows are dense entity numbers in ``[0, n_users)`` / ``[0, n_items)``, not raw keys.  Numbering the raw keys in
ascending order (for instance ``DeviceLabelEncoder().fit(all_keys).transform(keys) - 1``) makes "ascending user row"
here the reference's "ascending user_id", which is the order of its validation and test frames.

The sorts (``torch.sort(..., stable=True)``), the compactions (``nonzero``) and the size reads behind them are torch
plumbing; the marks come from ``csrc/interactions.hip``, the histories from ``csrc/history.hip``.  The two float64
transcendental steps (``count ** alpha``, ``log1p``) stay on the host over one value per entity: a device ``pow`` /
``log1p`` is not guaranteed to round like numpy's, and ``item_weights`` is pinned bit for bit.  Nothing here needs the
GPU at import time; the host-side refusals run without one.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np
import torch

from deepfm_amd import _lib
from deepfm_amd.data.candidates import item_weights
from deepfm_amd.data.device_epoch import SEEN_SETS_MAX_BYTES, SeenSets
from deepfm_amd.data.encoders import _as_tensor
from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema

MAX_ROWS = 2**31                  # a log holds fewer rows than this
MAX_TIMESTAMP = 2**53             # |timestamp| below this: the cutoffs are float64, and every such integer is one
HISTORY_MAX_BYTES = 1 << 32       # the (m, length) int64 bags of one lookup
HISTORY_TIES = ("position", "exclude")
HISTORY_BAG_TIES = HISTORY_TIES + ("latest",)   # a HistoryBag's queries are log rows, or user rows for "latest"
_OUTSIDE = "an interaction names a user or an item row outside the tables"      # SeenSets.from_interactions' words


def _check_column(values, dtype, what: str):
    """dtype and axes of a column, from its header alone: nothing is copied or read."""
    if not isinstance(values, (torch.Tensor, np.ndarray)):
        raise TypeError(f"{what}: expected a torch tensor or a numpy array, got {type(values).__name__}")
    have = values.dtype if isinstance(values, torch.Tensor) else torch.from_numpy(np.zeros(0, values.dtype)).dtype
    if have != dtype:
        raise TypeError(f"{what}: expected {dtype}, got {values.dtype}")
    if len(values.shape) != 1:
        raise ValueError(f"{what}: expected one axis, got shape {tuple(values.shape)}")
    return values


def _check_seen_bytes(n_users: int, n_items: int) -> int:
    """W, or ``SeenSets.from_interactions``' refusals in its words."""
    if n_users < 1 or n_items < 1:
        raise ValueError("n_users and n_items must be positive")
    W = (n_items + 31) // 32
    nbytes = 4 * n_users * (2 * W + 1)
    if nbytes > SEEN_SETS_MAX_BYTES:
        raise ValueError(f"seen-set bitmap + prefix of {n_users} users x {n_items} items take {nbytes} bytes, "
                         f"more than {SEEN_SETS_MAX_BYTES}: a catalogue this large needs another structure")
    return W


def _same_device(a: torch.device, b) -> bool:
    b = torch.device(b)
    if a.type != b.type:
        return False
    if a.type != "cuda" or a.index == b.index:
        return True
    current = torch.cuda.current_device()
    return (current if a.index is None else a.index) == (current if b.index is None else b.index)


def quantile_cutoff(a: float, b: float, gamma: float) -> float:
    """The linear interpolation between two neighbouring order statistics ``a <= b`` at fraction ``gamma``, in
    numpy's lerp form: ``a + (b - a) * gamma``, and ``b - (b - a) * (1 - gamma)`` when ``gamma >= 0.5``."""
    a, b, gamma = float(a), float(b), float(gamma)
    diff = b - a
    return b - diff * (1.0 - gamma) if gamma >= 0.5 else a + diff * gamma


def quantile_position(q: float, n: int) -> Tuple[int, int, float]:
    """``(lo, hi, gamma)``: the quantile ``q`` of ``n`` sorted values lies at fraction ``gamma`` between the order
    statistics ``lo`` and ``hi = min(lo + 1, n - 1)``, the virtual index being ``q * (n - 1)`` in float64.  ``q`` goes
    through ``q * 100.0 / 100.0`` first, as it does on its way from ``pandas.Series.quantile`` (which hands numpy a
    percentile) into numpy (which divides by 100 again)."""
    if n < 1:
        raise ValueError("the quantile of an empty column is undefined")
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"quantile {q} outside [0, 1]")
    q = q * 100.0 / 100.0
    virtual = (n - 1) * q
    lo = min(int(math.floor(virtual)), n - 1)
    return lo, min(lo + 1, n - 1), virtual - lo


def _check_ratios(val_ratio: float, test_ratio: float) -> None:
    ok = all(isinstance(r, (int, float)) and 0.0 <= r < 1.0 for r in (val_ratio, test_ratio))
    if not ok or not val_ratio + test_ratio < 1.0:
        raise ValueError(f"val_ratio = {val_ratio}, test_ratio = {test_ratio}: both must lie in [0, 1) and their sum "
                         "below 1")


def popularity_weights(item_counts, alpha: float) -> np.ndarray:
    """``item_weights`` of per-item counts of training positives (``log.counts("item", split.train)``): the
    reference's ``_build_popularity_weights`` as ``WeightedNegatives`` takes it.  The float64 ``pow`` stays on the
    host, over one value per item."""
    if isinstance(item_counts, torch.Tensor):
        item_counts = item_counts.cpu().numpy()
    return item_weights(item_counts, alpha)


def count_feature_table(counts, device=None):
    """(n_entities,) float32: the reference's count feature of every entity (``movielens.py:334-344, 447-458``) from
    its count of training positives.  The scaler's min and max are taken over ``log1p(count)`` of the entities with
    ``count >= 1`` (the reference fits on the groups that exist); the value is ``(log1p(count) - min) / (max - min)``
    in float64, a zero count going through ``log1p(0) = 0`` (the reference's ``fillna(0)``), all zeros when
    ``max == min``, cast to float32.  Computed on the host over one value per entity; a numpy array (an ``ItemTable``
    column as it is), or with ``device`` a tensor there, so that a log's column is ``table[log.user_rows[idx]]``."""
    if isinstance(counts, torch.Tensor):
        counts = counts.cpu().numpy()
    c = np.asarray(counts)
    if c.ndim != 1 or not np.issubdtype(c.dtype, np.integer) or (c < 0).any():
        raise ValueError("count_feature_table: counts must be a vector of non-negative integers")
    present = c >= 1
    if not present.any():
        raise ValueError("count_feature_table: no entity has a count, so there is nothing to fit the scaler on")
    log = np.log1p(c.astype(np.float64))
    lo, hi = float(log[present].min()), float(log[present].max())
    denom = hi - lo
    table = (np.zeros_like(log) if denom == 0 else (log - lo) / denom).astype(np.float32)
    return table if device is None else torch.from_numpy(table).to(device)


class DeviceSeenSets(SeenSets):
    """``SeenSets`` built into device memory by ``dfm_seen_sets_build``: the same bits as
    ``SeenSets.from_interactions``.  ``upload(device)`` returns the tensors it was built into, without a copy, when the
    device is theirs; ``bitmap``, ``prefix`` and ``unseen`` are numpy arrays downloaded on first use, so the candidate
    sources' host checks run on it as on a host-built one."""

    def __init__(self, bitmap: torch.Tensor, prefix: torch.Tensor, n_users: int, n_items: int) -> None:
        W = (n_items + 31) // 32
        for what, t, shape in (("bitmap", bitmap, (n_users, W)), ("prefix", prefix, (n_users, W + 1))):
            if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != bitmap.device:
                raise ValueError(f"{what}: expected a contiguous int32 tensor of shape {shape} on {bitmap.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
        self.bitmap_device, self.prefix_device = bitmap, prefix
        self.n_users, self.n_items, self.words = n_users, n_items, W
        self._bitmap: Optional[np.ndarray] = None
        self._prefix: Optional[np.ndarray] = None
        self._unseen: Optional[np.ndarray] = None

    @property
    def device(self) -> torch.device:
        return self.bitmap_device.device

    @property
    def bitmap(self) -> np.ndarray:
        if self._bitmap is None:
            self._bitmap = self.bitmap_device.cpu().numpy().view(np.uint32)
        return self._bitmap

    @property
    def prefix(self) -> np.ndarray:
        if self._prefix is None:
            self._prefix = self.prefix_device.cpu().numpy().view(np.uint32)
        return self._prefix

    @property
    def unseen(self) -> np.ndarray:
        """(n_users,) unseen item rows per user: the last column of the prefix alone is downloaded for it."""
        if self._prefix is not None:
            return self._prefix[:, self.words]
        if self._unseen is None:
            self._unseen = self.prefix_device[:, self.words].cpu().numpy().view(np.uint32)
        return self._unseen

    def upload(self, device):
        if _same_device(self.device, device):
            return self.bitmap_device, self.prefix_device
        return self.bitmap_device.to(device), self.prefix_device.to(device)


def device_seen_sets(user_rows: torch.Tensor, item_rows: torch.Tensor, n_users: int, n_items: int) -> DeviceSeenSets:
    """``SeenSets.from_interactions`` on the device the two int64 columns are on: three launches and one read of the
    count of refused rows, which raises as the host builder does."""
    W = _check_seen_bytes(n_users, n_items)
    _check_column(user_rows, torch.int64, "user_rows")
    _check_column(item_rows, torch.int64, "item_rows")
    if user_rows.shape != item_rows.shape:
        raise ValueError("user_rows and item_rows differ in length")
    if user_rows.shape[0] >= MAX_ROWS:
        raise ValueError(f"{user_rows.shape[0]} interactions: a log holds fewer than 2^31")
    _lib.require_device(user_rows, "user_rows")
    _lib.require_device(item_rows, "item_rows")
    dev = user_rows.device
    user_rows, item_rows = user_rows.contiguous(), item_rows.contiguous()
    bitmap = torch.empty(n_users, W, dtype=torch.int32, device=dev)
    prefix = torch.empty(n_users, W + 1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dfm_seen_sets_build(_lib.ptr(user_rows), _lib.ptr(item_rows), user_rows.numel(),
                                                   n_users, n_items, _lib.ptr(bitmap), _lib.ptr(prefix),
                                                   _lib.ptr(status), _lib.stream_handle()))
    if int(status.item()):                                  # once per build
        raise ValueError(_OUTSIDE)
    return DeviceSeenSets(bitmap, prefix, n_users, n_items)


def entity_counts(entity_rows: torch.Tensor, n_entities: int, labels: Optional[torch.Tensor] = None,
                  rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n_entities,) int64 on the device: per entity, the log rows (all of them, or ``rows``, an int64 index tensor)
    that name it and, when ``labels`` is given, have label 1 (``dfm_entity_counts``)."""
    _check_column(entity_rows, torch.int64, "entity_rows")
    _lib.require_device(entity_rows, "entity_rows")
    dev, n_log = entity_rows.device, entity_rows.shape[0]
    if n_entities < 1 or n_entities >= MAX_ROWS:
        raise ValueError(f"n_entities = {n_entities} outside [1, 2^31)")
    if labels is not None and (labels.dtype != torch.float32 or labels.shape != entity_rows.shape
                               or labels.device != dev):
        raise ValueError("labels: expected float32, one per log row, on the log's device")
    m = n_log
    if rows is not None:
        _check_column(rows, torch.int64, "rows")
        if rows.device != dev:
            raise ValueError(f"rows is on {rows.device}, the log on {dev}")
        rows, m = rows.contiguous(), rows.shape[0]
        if m == 0:                                          # an empty tensor has no address, and NULL means "all rows"
            return torch.zeros(n_entities, dtype=torch.int64, device=dev)
    if max(m, n_log) >= MAX_ROWS:
        raise ValueError(f"{max(m, n_log)} rows: a log holds fewer than 2^31")
    entity_rows = entity_rows.contiguous()
    labels = None if labels is None else labels.contiguous()
    counts = torch.empty(n_entities, dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dfm_entity_counts(_lib.ptr(entity_rows), _lib.ptr(labels), _lib.ptr(rows), m, n_log,
                                                 n_entities, _lib.ptr(counts), _lib.ptr(status), _lib.stream_handle()))
    bad_entity, bad_index = status.tolist()                 # once per call
    if bad_index:
        raise ValueError(f"{bad_index} of {m} entries of rows are outside the log's {n_log} rows")
    if bad_entity:
        raise ValueError(_OUTSIDE)
    return counts


@dataclass
class InteractionSplit:
    """The three parts of a split: int64 device index tensors into ``log``."""

    log: "DeviceInteractionLog"
    train: torch.Tensor
    val: torch.Tensor
    test: torch.Tensor
    cutoffs: Optional[Tuple[float, float]] = None      # temporal: (train_cutoff, val_cutoff), float64

    def __iter__(self):
        return iter((self.train, self.val, self.test))

    def user_of(self, which: str) -> np.ndarray:
        """The user rows of part ``which`` ("train", "val" or "test") as a numpy int32 array: what the candidate
        sources' host validation takes."""
        if which not in ("train", "val", "test"):
            raise ValueError(f"which = {which!r}: expected 'train', 'val' or 'test'")
        return self.log.user_rows[getattr(self, which)].cpu().numpy().astype(np.int32)


# ---------------------------------------------------------------------------------------------------- user histories
def _check_history_length(length) -> None:
    if not isinstance(length, int) or isinstance(length, bool) or not 1 <= length <= _lib.HISTORY_MAX_LENGTH:
        raise ValueError(f"length = {length!r} outside [1, {_lib.HISTORY_MAX_LENGTH}] (the bag cap of the record "
                         "assembly)")


def _check_index_tensor(t, what: str, device) -> torch.Tensor:
    """An int64 index tensor of one axis on the log's device, from its header alone."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor on {device}, got {type(t).__name__}")
    _check_column(t, torch.int64, what)
    if t.shape[0] >= MAX_ROWS:
        raise ValueError(f"{what}: {t.shape[0]} entries: an index holds fewer than 2^31")
    return t


def _check_on(t: torch.Tensor, what: str, device) -> None:
    if not _same_device(t.device, device):
        raise ValueError(f"{what} is on {t.device}, the log on {device}")


def history_field(name: str, length: int, n_items: int, embedding_dim: int, combiner: str = "mean",
                  group: str = "user") -> FieldSchema:
    """The SEQUENCE field of a ``UserHistory.bag`` of ``length`` ids over ``n_items`` item rows under the default
    ``item_ids`` (id = item row + 1, 0 the padding): ``vocabulary_size = n_items + 1``.  ``combiner="max"`` is refused
    in ``record_backward_reason``'s words (the fused steps cannot train it), ``group="item"`` because ``default_roles``
    would make the field ITEM and a negative would look its bag up in the item table instead of copying its
    positive's."""
    _check_history_length(length)
    if not isinstance(n_items, int) or not 1 <= n_items < MAX_ROWS:
        raise ValueError(f"n_items = {n_items!r} outside [1, 2^31)")
    if group == "item":
        raise ValueError(f"field {name!r}: group 'item' gives it the ITEM role, and a negative would look its bag up in "
                         "the item table; a history belongs to the user (or to the context)")
    spec = FieldSchema(name, FeatureType.SEQUENCE, vocabulary_size=n_items + 1, embedding_dim=embedding_dim,
                       group=group, max_length=length, combiner=combiner)
    if combiner == "max":
        from deepfm_amd.training.eligibility import record_backward_reason       # (training imports data)
        raise ValueError(record_backward_reason(SimpleNamespace(schema=DatasetSchema(fields={name: spec}))))
    if combiner not in ("mean", "sum"):
        raise ValueError(f"field {name!r}: combiner {combiner!r}: expected 'mean' or 'sum'")
    return spec


@dataclass
class UserHistory:
    """What ``DeviceHistoryIndex.lookup`` / ``latest`` return, device tensors: ``bag`` (m, length) int64, contiguous,
    the prior items' ids latest first and 0 behind them (a SEQUENCE column of ``DeviceColumns.from_device``); ``count``
    (m,) int64, the prior events, not capped by ``length``; ``gap`` (m,) int64, the query's timestamp minus the latest
    prior event's, -1 without one (and always for ``latest``)."""

    bag: torch.Tensor
    count: torch.Tensor
    gap: torch.Tensor


class DeviceHistoryIndex:
    """The events of a log, per user in (timestamp, log position) order, and for every log row how many of its user's
    events come before it (``dfm_history_index_build``): what ``DeviceInteractionLog.history_index`` builds once.

    A query ``q`` (a log row, event or not, repeats allowed) has the prior set
      ``ties="position"``  the user's events ``e`` with ``(ts[e], e) < (ts[q], q)``;
      ``ties="exclude"``   the user's events with ``ts[e] < ts[q]``: for a clock that ties (MovieLens' seconds), where
                           "earlier in the file" is no evidence of "earlier";
    ``latest`` takes user rows, and the prior set is every event of the user.  A row never sees itself."""

    def __init__(self, log: "DeviceInteractionLog", start, pos_of, rank, events, sorted_ts, event_count,
                 item_ids: Optional[torch.Tensor]) -> None:
        self.log, self.device = log, log.device
        self.n, self.n_users, self.n_items = log.n, log.n_users, log.n_items
        self.start, self.pos_of, self.rank, self.events = start, pos_of, rank, events
        self.sorted_ts, self.event_count, self.item_ids = sorted_ts, event_count, item_ids

    def lookup(self, rows: torch.Tensor, length: int, ties: str = "position") -> UserHistory:
        """The histories of the log rows ``rows`` (int64, on the log's device): one ``dfm_history_gather`` launch and
        one read of its status word, which refuses a row outside the log."""
        if ties not in HISTORY_TIES:
            raise ValueError(f"ties = {ties!r}: expected one of {HISTORY_TIES}")
        mode = _lib.HISTORY_POSITION if ties == "position" else _lib.HISTORY_EXCLUDE
        return self._gather(rows, "rows", length, mode)

    def latest(self, user_rows: torch.Tensor, length: int) -> UserHistory:
        """The history of each of ``user_rows`` as of now, every event of the user: what a ``CatalogueScorer`` query
        for a live user takes.  ``gap`` is -1: there is no query time."""
        return self._gather(user_rows, "user_rows", length, _lib.HISTORY_LATEST)

    def _gather(self, queries: torch.Tensor, what: str, length: int, mode: int) -> UserHistory:
        _check_history_length(length)
        m = _check_index_tensor(queries, what, self.device).shape[0]
        if m * length * 8 > HISTORY_MAX_BYTES:
            raise ValueError(f"{m} bags of {length} ids take {m * length * 8} bytes, more than {HISTORY_MAX_BYTES}: "
                             f"look the parts of {what} up separately")
        _check_on(queries, what, self.device)
        dev = queries.device
        out = UserHistory(torch.empty(m, length, dtype=torch.int64, device=dev),
                          torch.empty(m, dtype=torch.int64, device=dev), torch.empty(m, dtype=torch.int64, device=dev))
        if m == 0:                                          # an empty tensor has no address
            return out
        _lib.require_device(queries, what)
        queries, log = queries.contiguous(), self.log
        status = torch.zeros(2, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().dfm_history_gather(
                _lib.ptr(queries), m, mode, length, _lib.ptr(log.user_rows), _lib.ptr(log.item_rows),
                _lib.ptr(log.timestamps), _lib.ptr(self.item_ids), _lib.ptr(self.start), _lib.ptr(self.pos_of),
                _lib.ptr(self.rank), _lib.ptr(self.events), _lib.ptr(self.sorted_ts), _lib.ptr(self.event_count),
                self.n, self.n_users, self.n_items, _lib.ptr(out.bag), _lib.ptr(out.count), _lib.ptr(out.gap),
                _lib.ptr(status), _lib.stream_handle()))
        bad_query, bad_slot = status.tolist()               # once per call
        if bad_query:
            table = f"the user table's {self.n_users} rows" if mode == _lib.HISTORY_LATEST else f"the log's {self.n} rows"
            raise ValueError(f"{bad_query} of {m} entries of {what} are outside {table}")
        if bad_slot:
            raise ValueError(_OUTSIDE)
        return out


class HistoryBag:
    """A bag column that is not materialised: ``length`` ids per query, formed from ``index`` inside the record
    assembly (``dfm_assemble_plan_bind_history``), so the ``(n, length)`` int64 block of ``lookup`` never exists outside
    the one batch record being written.  ``DeviceColumns.from_device(bags=[...])`` takes it wherever it takes that
    block, and a ``DeviceEpochLoader`` over those columns writes the same record bytes.

    ``queries``: int64, one axis, on the index's device, one entry per row of the columns, repeats allowed: log rows
    for ``ties="position"`` / ``"exclude"`` (``DeviceHistoryIndex.lookup``'s rules), user rows for ``"latest"``.  It
    holds 8 bytes per row beside the index, whatever ``length`` is, and the 4 GiB cap of one lookup does not apply.
    Construction checks, with one device reduction and one host read, that every query is inside the log (the user
    table), in ``lookup``'s words; the kernel then needs no status word.  The field's role must be COPY (a negative
    takes its positive's bag): ``history_field`` steers there and ``DeviceEpochLoader`` refuses anything else."""

    def __init__(self, index: DeviceHistoryIndex, queries: torch.Tensor, length: int, ties: str = "position") -> None:
        if ties not in HISTORY_BAG_TIES:
            raise ValueError(f"ties = {ties!r}: expected one of {HISTORY_BAG_TIES}")
        _check_history_length(length)
        m = _check_index_tensor(queries, "queries", index.device).shape[0]
        _check_on(queries, "queries", index.device)
        self.index, self.length, self.ties = index, length, ties
        self.mode = {"position": _lib.HISTORY_POSITION, "exclude": _lib.HISTORY_EXCLUDE,
                     "latest": _lib.HISTORY_LATEST}[ties]
        self.queries = queries.contiguous()
        if m:
            _lib.require_device(self.queries, "queries")
            limit = index.n_users if ties == "latest" else index.n
            bad_query = int(((self.queries < 0) | (self.queries >= limit)).sum())      # once per bag
            if bad_query:
                table = f"the user table's {index.n_users} rows" if ties == "latest" else f"the log's {index.n} rows"
                raise ValueError(f"{bad_query} of {m} entries of queries are outside {table}")

    def __len__(self) -> int:
        return self.queries.shape[0]

    @property
    def device(self) -> torch.device:
        return self.queries.device

    def data_ptr(self) -> int:
        """The queries' address: what the column's ``pos`` is once it is bound."""
        return self.queries.data_ptr()

    def source(self) -> _lib.HistorySource:
        """``dfm_history_source`` over the index's tensors: raw addresses, so the index must outlive every plan the
        struct was bound to (the loader keeps this object, which keeps the index)."""
        ix, log = self.index, self.index.log
        return _lib.HistorySource(
            _lib.ptr(log.user_rows), _lib.ptr(log.item_rows), _lib.ptr(log.timestamps), _lib.ptr(ix.item_ids),
            _lib.ptr(ix.start), _lib.ptr(ix.pos_of), _lib.ptr(ix.rank), _lib.ptr(ix.events), _lib.ptr(ix.sorted_ts),
            _lib.ptr(ix.event_count), ix.n, ix.n_users, ix.n_items, self.mode)

    def materialize(self) -> UserHistory:
        """``index.lookup(queries, length, ties)`` / ``index.latest(queries, length)``: the block this object stands
        for, under the 4 GiB cap of one lookup."""
        if self.ties == "latest":
            return self.index.latest(self.queries, self.length)
        return self.index.lookup(self.queries, self.length, self.ties)


class DeviceInteractionLog:
    """``n`` interactions on ``device``: ``user_rows`` and ``item_rows`` (int64 dense entity numbers, see the module
    docstring for how to number raw keys), ``timestamps`` (int64) and ``labels`` (float32, 0 or 1), as numpy arrays or
    tensors.  Refused on the host, before any device work: columns of unequal length, ``n >= 2^31``, seen-sets above
    ``SEEN_SETS_MAX_BYTES`` (``SeenSets.from_interactions``' rule and words) and, for columns that arrive on the host,
    ``|timestamp| >= 2^53``.  The labels are checked on the device (with the timestamps of a column that arrived
    there); the one read of that check happens here and names the first offending position.  User and item rows
    outside the tables are counted by the kernels and refused by the method that meets them."""

    def __init__(self, user_rows, item_rows, timestamps, labels, n_users: int, n_items: int, device="cuda") -> None:
        cols = [_check_column(user_rows, torch.int64, "user_rows"), _check_column(item_rows, torch.int64, "item_rows"),
                _check_column(timestamps, torch.int64, "timestamps"), _check_column(labels, torch.float32, "labels")]
        n = cols[0].shape[0]
        if any(c.shape[0] != n for c in cols):
            raise ValueError("user_rows, item_rows, timestamps and labels differ in length: "
                             f"{[int(c.shape[0]) for c in cols]}")
        if n >= MAX_ROWS:
            raise ValueError(f"{n} interactions: a log holds fewer than 2^31")
        _check_seen_bytes(n_users, n_items)
        cols = [_as_tensor(c, "column") for c in cols]
        if n and not cols[2].is_cuda:
            bad = (cols[2] >= MAX_TIMESTAMP) | (cols[2] <= -MAX_TIMESTAMP)
            if bool(bad.any()):
                self._refuse_timestamp(cols[2], int(bad.to(torch.uint8).argmax()))
        self.device = torch.device(device)
        self.n, self.n_users, self.n_items = n, n_users, n_items
        self.user_rows, self.item_rows, self.timestamps, self.labels = (c.to(self.device).contiguous() for c in cols)
        _lib.require_device(self.labels, "the interaction log")
        if n:
            bad_label = (self.labels != 0) & (self.labels != 1)
            bad_ts = (self.timestamps >= MAX_TIMESTAMP) | (self.timestamps <= -MAX_TIMESTAMP)
            first = torch.stack([torch.where(b.any(), b.to(torch.uint8).argmax(), -1) for b in (bad_label, bad_ts)])
            first_label, first_ts = first.tolist()          # the one read of the construction
            self._refuse_timestamp(self.timestamps, first_ts)
            if first_label >= 0:
                raise ValueError(f"labels[{first_label}] = {float(self.labels[first_label])}: labels are 0 or 1")

    @staticmethod
    def _refuse_timestamp(timestamps: torch.Tensor, first: int) -> None:
        if first >= 0:
            raise ValueError(f"timestamps[{first}] = {int(timestamps[first])}: |timestamp| must be below 2^53 (the "
                             "cutoffs of the temporal split are float64)")

    @classmethod
    def from_ratings(cls, user_rows, item_rows, timestamps, ratings, label_threshold: float, n_users: int,
                     n_items: int, device="cuda") -> "DeviceInteractionLog":
        """``label = rating >= label_threshold`` as float32 (``movielens.py:211``); ``ratings`` of any real dtype."""
        if isinstance(ratings, np.ndarray):
            labels = (ratings >= label_threshold).astype(np.float32)
        elif isinstance(ratings, torch.Tensor):
            labels = (ratings >= label_threshold).to(torch.float32)
        else:
            raise TypeError(f"ratings: expected a torch tensor or a numpy array, got {type(ratings).__name__}")
        return cls(user_rows, item_rows, timestamps, labels, n_users, n_items, device)

    def __len__(self) -> int:
        return self.n

    def _stream(self):
        return torch.cuda.device(self.device)

    # ------------------------------------------------------------------------------------------------ splits
    def temporal_split(self, val_ratio: float, test_ratio: float) -> InteractionSplit:
        """The reference's ``_temporal_split`` (``movielens.py:269-304``).  Rows are ordered by timestamp, ties by
        log position (the reference's ``sort_values`` leaves ties unspecified: that rule is this project's choice).
        ``train_cutoff`` / ``val_cutoff`` are what pandas gives for ``quantile(1 - val_ratio - test_ratio)`` and
        ``quantile(1 - test_ratio)`` (``quantile_position``, ``quantile_cutoff``), computed on the host from the four
        order statistics read from the device-sorted column.  ``train``: the rows with ``timestamp <= train_cutoff``
        of any label, in sorted order.  ``val``: per user that occurs in train, its first positive in
        ``(train_cutoff, val_cutoff]``, by ascending user row.  ``test``: the same for ``timestamp > val_cutoff``."""
        _check_ratios(val_ratio, test_ratio)
        n = self.n
        if n == 0:
            raise ValueError("the temporal split of an empty log is undefined (its quantiles are)")
        sorted_ts, order = torch.sort(self.timestamps, stable=True)
        places = [quantile_position(q, n) for q in (1 - val_ratio - test_ratio, 1 - test_ratio)]
        at = torch.tensor([places[0][0], places[0][1], places[1][0], places[1][1]], device=self.device)
        stats = sorted_ts[at].tolist()
        cutoffs = [quantile_cutoff(stats[0], stats[1], places[0][2]), quantile_cutoff(stats[2], stats[3], places[1][2])]
        # an integer timestamp is <= a float64 cutoff exactly when it is <= the cutoff's floor (both below 2^53)
        floors = torch.tensor([math.floor(c) for c in cutoffs], dtype=torch.int64, device=self.device)
        n_train, n_trainval = torch.searchsorted(sorted_ts, floors, right=True).tolist()
        in_train = torch.empty(self.n_users, dtype=torch.uint8, device=self.device)
        first = torch.empty(2, self.n_users, dtype=torch.int64, device=self.device)
        status = torch.zeros(1, dtype=torch.int64, device=self.device)
        with self._stream():
            _lib.check(_lib.load().dfm_temporal_split_mark(
                _lib.ptr(self.user_rows), _lib.ptr(self.labels), _lib.ptr(order), n, self.n_users, n_train, n_trainval,
                _lib.ptr(in_train), _lib.ptr(first[0]), _lib.ptr(first[1]), _lib.ptr(status), _lib.stream_handle()))
        val, test = (order[f[f < n]] for f in first)
        if int(status.item()):
            raise ValueError(_OUTSIDE)
        return InteractionSplit(self, order[:n_train], val, test, tuple(cutoffs))

    def leave_one_out_split(self, min_interactions: int) -> InteractionSplit:
        """The reference's ``_leave_one_out_split`` (``movielens.py:235-267``).  Rows are sorted by (user row,
        timestamp, log position); a user with at least ``min_interactions`` rows gives its last row to test and its
        second-to-last to val, every other row goes to train; labels play no part.  ``train`` is in sorted order,
        ``val`` and ``test`` in ascending user row.  ``min_interactions < 2`` is refused (the reference raises
        ``IndexError`` there)."""
        if not isinstance(min_interactions, int) or min_interactions < 2:
            raise ValueError(f"min_interactions = {min_interactions}: a user gives two rows away, so at least 2")
        n = self.n
        by_time = torch.sort(self.timestamps, stable=True)[1]
        order = by_time[torch.sort(self.user_rows[by_time], stable=True)[1]]
        user_counts = entity_counts(self.user_rows, self.n_users)
        roles = torch.zeros(n, dtype=torch.uint8, device=self.device)
        status = torch.zeros(1, dtype=torch.int64, device=self.device)
        with self._stream():
            _lib.check(_lib.load().dfm_loo_split_mark(
                _lib.ptr(self.user_rows), _lib.ptr(order), _lib.ptr(user_counts), n, self.n_users, min_interactions,
                _lib.ptr(roles), _lib.ptr(status), _lib.stream_handle()))
        parts = [order[roles == r] for r in (0, 1, 2)]
        if int(status.item()):
            raise ValueError(_OUTSIDE)
        return InteractionSplit(self, *parts)

    # ------------------------------------------------------------------------------------------------ sets and counts
    def seen_sets(self) -> DeviceSeenSets:
        """Per user, the item rows of ALL its interactions, whatever their label or part: the reference's
        ``_user_items``."""
        return device_seen_sets(self.user_rows, self.item_rows, self.n_users, self.n_items)

    def counts(self, by: str, rows: Optional[torch.Tensor] = None, positives_only: bool = True) -> torch.Tensor:
        """(n_users,) or (n_items,) int64 on the device: per entity, the rows of the log (or of ``rows``, an int64
        index tensor such as ``split.train``) that name it, the positives among them alone by default.  Over
        ``split.train`` these are the reference's ``_user_counts`` / ``_item_counts`` and the counts behind its
        popularity weights."""
        if by not in ("user", "item"):
            raise ValueError(f"by = {by!r}: expected 'user' or 'item'")
        entity, n_entities = (self.user_rows, self.n_users) if by == "user" else (self.item_rows, self.n_items)
        return entity_counts(entity, n_entities, self.labels if positives_only else None, rows)

    # ------------------------------------------------------------------------------------------------ histories
    def history_index(self, source: Optional[torch.Tensor] = None, positives_only: bool = True,
                      item_ids=None) -> DeviceHistoryIndex:
        """The index behind per-row user histories (``DeviceHistoryIndex``).  An event is a log row that is in
        ``source`` (an int64 index tensor such as ``split.train``, duplicates collapse; None: every row) and, with
        ``positives_only``, has label 1.  ``item_ids``: (n_items,) int64 >= 0, the id a bag holds for an item row;
        None: item row + 1, the inverse of the numbering rule of the module docstring.  Two stable sorts into the
        (user row, timestamp, log position) order of ``leave_one_out_split``, the per-user counts and their exclusive
        scan, one ``dfm_history_index_build`` launch and one read of its status."""
        dev = self.device
        if source is not None:
            _check_index_tensor(source, "source", dev)
            _check_on(source, "source", dev)
        if item_ids is not None:
            _check_column(item_ids, torch.int64, "item_ids")
            if item_ids.shape[0] != self.n_items:
                raise ValueError(f"item_ids: expected one id per item row, shape ({self.n_items},), got "
                                 f"{tuple(item_ids.shape)}")
            item_ids = _as_tensor(item_ids, "item_ids")
            if bool((item_ids < 0).any()):                  # once per index
                raise ValueError("item_ids: an id is negative (0 is the padding id, every other id is positive)")
            item_ids = item_ids.to(dev).contiguous()
        n, n_users = self.n, self.n_users
        by_time = torch.sort(self.timestamps, stable=True)[1]
        order = by_time[torch.sort(self.user_rows[by_time], stable=True)[1]]
        user_counts = entity_counts(self.user_rows, n_users)             # refuses user rows outside the table
        start = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
        torch.cumsum(user_counts, 0, out=start[1:])
        mask, bad_source = None, torch.zeros((), dtype=torch.int64, device=dev)
        if source is not None:
            mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            bad_source = ((source < 0) | (source >= n)).sum()          # read with the status, below
            if n:
                mask[source.clamp(0, n - 1)] = 1                       # a clamped entry marks a log that is refused
        pos_of, rank, events = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        sorted_ts = torch.empty(n, dtype=torch.int64, device=dev)
        event_count = torch.empty(n_users, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int64, device=dev)
        with self._stream():
            _lib.check(_lib.load().dfm_history_index_build(
                _lib.ptr(self.user_rows), _lib.ptr(self.item_rows), _lib.ptr(self.timestamps),
                _lib.ptr(self.labels if positives_only else None), _lib.ptr(mask), _lib.ptr(order), _lib.ptr(start), n,
                n_users, self.n_items, _lib.ptr(pos_of), _lib.ptr(rank), _lib.ptr(events), _lib.ptr(sorted_ts),
                _lib.ptr(event_count), _lib.ptr(status), _lib.stream_handle()))
        bad_row, bad_source = torch.stack([status[0], bad_source]).tolist()     # once per index
        if bad_source:
            raise ValueError(f"{bad_source} of {source.shape[0]} entries of source are outside the log's {n} rows")
        if bad_row:
            raise ValueError(_OUTSIDE)
        return DeviceHistoryIndex(self, start, pos_of, rank, events, sorted_ts, event_count, item_ids)
