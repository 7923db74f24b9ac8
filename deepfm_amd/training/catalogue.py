"""Scoring a set of queries against the whole catalogue on the device: what to recommend, and the
unsampled HR@k / NDCG@k that the reference's 1 + 999 sampled candidates (trainer.py:296-332) approximate.

``CatalogueScorer.scores()`` forms every (query, item) row with the training assembler (``dfm_record_assemble`` over
``data/candidates.py:CatalogueCandidates``) and scores it with a predictor's captured forward; ``dfm_catalogue_topk``
(``csrc/catalogue.hip``) then masks the seen rows, selects the top K and ranks a held-out target.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from deepfm_amd import _lib
from deepfm_amd.data.candidates import CatalogueCandidates
from deepfm_amd.data.device_epoch import DeviceEpochLoader
from deepfm_amd.training.metrics import _check_ks, _grouping_faults, ranking_dict


class CatalogueScorer:
    """``predictor`` (a ``FusedPredictor`` / ``MixedSchemaPredictor``) over ``candidates``' Q queries x n_items."""

    def __init__(self, predictor, candidates: CatalogueCandidates) -> None:
        cols = candidates.columns
        if cols.schema is not predictor.model.schema and list(cols.schema.fields) != list(predictor.model.schema.fields):
            raise ValueError("candidates of another schema")
        self.predictor, self.candidates = predictor, candidates
        self.Q, self.n_items = len(cols), candidates.num_neg
        self.loader = DeviceEpochLoader(cols, predictor.B, shuffle=False, negatives=candidates)

    def scores(self) -> torch.Tensor:
        """The (Q, n_items) float32 device matrix of probabilities, row q the query's scores by item row.  Per batch
        one ``dfm_record_assemble`` and one forward launch, all enqueued on the current stream: no host copy and no
        per-batch synchronisation (besides the predictor's wait for its graph slot of two launches ago)."""
        pred, B, n = self.predictor, self.predictor.B, self.Q * self.n_items
        pred._check_tables()
        out = torch.empty(self.Q, self.n_items, dtype=torch.float32, device=pred.device)
        # the candidate rows follow the Q query rows
        pred._score(((self.loader.rows_into_next(self.Q + s, min(B, n - s)).data_ptr(), min(B, n - s))
                     for s in range(0, n, B)), out.view(-1))
        if pred.emb.strict_indices:
            pred.emb.raise_on_bad_index()
        return out

    def _topk(self, scores: torch.Tensor, targets: Optional[torch.Tensor], k: int, exclude_seen: bool):
        if not 1 <= k <= _lib.TOPK_MAX_K:
            raise ValueError(f"k = {k} outside [1, {_lib.TOPK_MAX_K}]")
        c, dev = self.candidates, scores.device
        items = torch.empty(self.Q, k, dtype=torch.int32, device=dev)
        top = torch.empty(self.Q, k, dtype=torch.float32, device=dev)
        rank = torch.empty(self.Q, dtype=torch.int32, device=dev)
        status = torch.empty(3, dtype=torch.int64, device=dev)
        _lib.check(_lib.load().dfm_catalogue_topk(
            scores.data_ptr(), c.bitmap.data_ptr(), c.user_of.data_ptr(), _lib.ptr(targets), self.Q, c.seen.n_users,
            self.n_items, k, 1 if exclude_seen else 0, items.data_ptr(), top.data_ptr(), rank.data_ptr(),
            status.data_ptr(), _lib.stream_handle()))
        return items, top, rank, status

    @staticmethod
    def _raise_on_status(nan: float, bad_user: float, bad_target: float, n_items: int) -> None:
        if bad_target:
            raise ValueError(f"{int(bad_target)} targets outside [-1, {n_items})")
        _grouping_faults((bad_user, nan, 0.0))                 # the ranking metrics' messages for bad ids, NaN scores

    def recommend(self, k: int, exclude_seen: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per query the first ``k`` (at most 128) item rows in the ranking order (descending score, ties by ascending
        row), without the rows its user has seen unless ``exclude_seen`` is off: ``(items (Q, k) int32, scores (Q, k)
        float32)`` device tensors, padded with -1 / -inf.  Raises ``ValueError`` on NaN scores."""
        items, top, _, status = self._topk(self.scores(), None, k, exclude_seen)
        self._raise_on_status(*status.cpu().tolist(), self.n_items)
        return items, top

    def evaluate(self, targets, ks=(1, 5, 10, 20)) -> Dict[str, float]:
        """Unsampled leave-one-out ``HR@k`` / ``NDCG@k``: ``targets`` (Q,) holds each query's held-out item row, or -1
        for none.  rank = the unseen rows that precede the target in the ranking order (the target itself counts as
        unseen); HR@k = [rank < k], NDCG@k = [rank < k] / log2(rank + 2), averaged over the queries with a target
        (``{}`` without any).  Reduced on the device in float64 in a fixed order (a histogram of the ranks below
        max(ks), then one term per rank, ascending), one host read at the end; every k at most 128."""
        ks = _check_ks(ks)
        if max(ks) > _lib.TOPK_MAX_K:
            raise ValueError(f"ks {ks}: every k must be at most {_lib.TOPK_MAX_K}")
        dev = self.predictor.device
        t = targets if isinstance(targets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(targets, dtype=np.int32))
        t = t.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        if t.numel() != self.Q:
            raise ValueError(f"{t.numel()} targets for {self.Q} queries")
        _, _, rank, status = self._topk(self.scores(), t, 1, True)
        kmax = max(ks)
        rank = rank.to(torch.int64)
        has = rank >= 0
        # ranks at or above kmax and queries without a target fall into the last bin
        hist = torch.bincount(torch.where(has, rank.clamp(max=kmax), torch.full_like(rank, kmax)), minlength=kmax + 1)
        gain = torch.from_numpy(1.0 / np.log2(np.arange(kmax, dtype=np.float64) + 2.0)).to(dev)
        terms = hist[:kmax].to(torch.float64) * gain
        users = has.sum().to(torch.float64)
        hits = torch.cumsum(hist[:kmax], 0).to(torch.float64)  # integers: exact
        acc, ndcg = torch.zeros((), dtype=torch.float64, device=dev), {}
        for r in range(kmax):                                  # one add per rank, ascending: a fixed order
            acc = acc + terms[r]
            if r + 1 in ks:
                ndcg[r + 1] = acc
        out = torch.stack([users] + [hits[k - 1] / users for k in ks] + [ndcg[k] / users for k in ks]
                          + list(status.to(torch.float64)))
        host: List[float] = out.cpu().tolist()
        m = len(ks)
        nan, bad_user, bad_target = host[1 + 2 * m:]
        self._raise_on_status(nan, bad_user, bad_target, self.n_items)
        return ranking_dict(host[:1 + 2 * m] + [0.0, 0.0, 0.0], ks)
