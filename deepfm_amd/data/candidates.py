"""Evaluation candidates on the device: the two candidate sources of an evaluation split, both
consumed by ``DeviceEpochLoader`` through the assembler that forms the training batches.

``item_weights``          the reference's sampling weights ``count ** alpha`` as integers in [1, 2^24];
``WeightedNegatives``     per query, C item rows drawn with replacement from the user's unseen rows with those
                          weights (``dfm_sample_weighted``): the reference's ``_add_eval_negatives``
                          (``movielens.py:567-604``), drawn once per split;
``CatalogueCandidates``   per query, every item row: the loader's rows from P on are the (Q, n_items) score matrix.

Every check runs on the host, before anything touches the device.
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from deepfm_amd import _lib
from deepfm_amd.data.device_epoch import (SHORT_USERS, BucketDifference, CandidateSource, DeviceColumns, ItemTable,
                                          Role, SeenSets)

WEIGHT_ONE = 1 << 24                  # the heaviest item's integer weight
CATALOGUE_MAX_BYTES = 1 << 30         # the (Q, n_items) float32 score matrix (and the int32 candidate lists)


def item_weights(counts, alpha: float) -> np.ndarray:
    """(n_items,) uint32 sampling weights in [1, 2^24] from per-item interaction counts: ``max(count, 1) ** alpha``
    in float64 (the reference's popularity weights, ``movielens.py:467-480``: a zero count counts as 1), divided by
    the maximum, times 2^24, rounded to nearest, clamped below at 1.

    Integers make the weighted draw exact and independent of summation order.  The price is the rounding: an item of
    float weight f (after the scaling, so the heaviest has f = 2^24) gets round(f), off by at most 1/2, a relative
    deviation of at most 1 / (2 f): 2^-25 for the heaviest item and larger for lighter ones, up to a factor 2 for an
    item whose f is below 1/2 and is clamped to 1."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    if c.size == 0 or not np.isfinite(c).all() or (c < 0).any():
        raise ValueError("item_weights: counts must be a non-empty vector of finite, non-negative numbers")
    if not np.isfinite(alpha):
        raise ValueError("item_weights: alpha must be finite")
    f = np.maximum(c, 1.0) ** float(alpha)
    w = np.rint(f / f.max() * WEIGHT_ONE)
    return np.maximum(w, 1.0).astype(np.uint32)


class WeightedNegatives(CandidateSource):
    """``num_neg`` evaluation candidates per query row of ``columns``: item rows the query's user (``user_of``, (Q,)
    user rows) has not seen, drawn with replacement, row i with probability ``weights[i] / sum(weights over the
    user's unseen rows)`` (``dfm_sample_weighted``; ``weights`` from ``item_weights``).  ``sample(epoch)`` fills
    ``neg_items`` (Q, num_neg) int32; one ``(seed, epoch)`` is one split's draw.

    A user with fewer unseen rows than ``num_neg`` is refused by default (``short_users="refuse"``), as
    ``NegativeSampler`` refuses it.  With ``short_users="truncate"`` it gets ``min(num_neg, unseen)`` draws, the
    reference's rule (``movielens.py:575-580``), and none when it has seen everything: the source is then ragged
    (``CandidateSource``), and every other query's draws are unchanged."""

    def __init__(self, columns: DeviceColumns, seen: SeenSets, user_of, items: ItemTable, weights, num_neg: int,
                 roles: Optional[Dict[str, Role]] = None, derived: Optional[Dict[str, BucketDifference]] = None,
                 seed: int = 0, short_users: str = "refuse") -> None:
        if short_users not in SHORT_USERS:
            raise ValueError(f"short_users = {short_users!r}: expected one of {SHORT_USERS}")
        if not 1 <= num_neg <= _lib.MAX_CANDIDATES:
            raise ValueError(f"num_neg = {num_neg} outside [1, {_lib.MAX_CANDIDATES}]")
        user_of = self._validate(columns, seen, user_of, items, roles, derived)
        w = np.asarray(weights)
        if w.shape != (seen.n_items,):
            raise ValueError(f"weights has shape {w.shape} for {seen.n_items} item rows")
        if not np.issubdtype(w.dtype, np.integer) or w.min() < 1 or w.max() > WEIGHT_ONE:
            raise ValueError(f"weights must be integers in [1, {WEIGHT_ONE}] (item_weights)")
        if seen.n_items > _lib.WEIGHTED_MAX_ITEMS:
            raise ValueError(f"{seen.n_items} item rows: the weighted draw takes at most {_lib.WEIGHTED_MAX_ITEMS}")
        if len(columns) > 1 << 19:
            raise ValueError(f"{len(columns)} queries: the weighted draw takes at most {1 << 19}")
        counts = self._short_users(seen, user_of, num_neg, short_users, "a loader's rows are a fixed count per query")
        self.seed = seed
        self._upload(columns, seen, user_of, items, num_neg, counts)
        self.weights = torch.from_numpy(np.ascontiguousarray(w, dtype=np.uint32).view(np.int32)).to(columns.device)

    def _draw(self, epoch: int, out: torch.Tensor) -> None:
        self._check_draw(epoch, out, "the candidates")
        _lib.check(_lib.load().dfm_sample_weighted(
            self.bitmap.data_ptr(), self.user_of.data_ptr(), self.weights.data_ptr(), len(self.columns),
            self.seen.n_users, self.seen.n_items, self.num_neg, self.seed & 0xFFFFFFFFFFFFFFFF, epoch, self._list(),
            out.data_ptr(), _lib.stream_handle()))


class CatalogueCandidates(CandidateSource):
    """Every item row as a candidate of every query row of ``columns``: ``num_neg = n_items`` and
    ``neg_items[q] = 0 .. n_items - 1``, whatever the epoch.  A ``DeviceEpochLoader`` over it with ``shuffle=False``,
    read from row ``Q`` on, yields the rows of the (Q, n_items) score matrix row-major
    (``training/catalogue.py:CatalogueScorer``).  Refused when that matrix exceeds ``CATALOGUE_MAX_BYTES``."""

    def __init__(self, columns: DeviceColumns, seen: SeenSets, user_of, items: ItemTable,
                 roles: Optional[Dict[str, Role]] = None, derived: Optional[Dict[str, BucketDifference]] = None) -> None:
        user_of = self._validate(columns, seen, user_of, items, roles, derived)
        n_items = seen.n_items
        if n_items > _lib.MAX_CANDIDATES:
            raise ValueError(f"{n_items} item rows: a candidate list holds at most {_lib.MAX_CANDIDATES}")
        nbytes = 4 * len(columns) * n_items
        if nbytes > CATALOGUE_MAX_BYTES:
            raise ValueError(f"the score matrix of {len(columns)} queries x {n_items} items takes {nbytes} bytes, "
                             f"more than {CATALOGUE_MAX_BYTES}: score the queries in several parts")
        self._upload(columns, seen, user_of, items, n_items)
        self.neg_items.copy_(torch.arange(n_items, dtype=torch.int32, device=columns.device).expand(len(columns), n_items))

    def _draw(self, epoch: int, out: torch.Tensor) -> None:
        if out is not self.neg_items:
            out.copy_(self.neg_items)
