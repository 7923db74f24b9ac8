"""numpy restatements of the evaluation-candidate kernels (``csrc/sampler.hip:sample_weighted_kernel``,
``csrc/catalogue.hip``), written from their specification in ``include/deepfm_hip.h`` and sharing no code with the
HIP side.  Every output is integer rows or copied float bits, so the GPU tests compare bit for bit.

Weighted draw t of query p over the user's ascending unseen rows, T = their summed weights (Python integers):
    x = seed * 0x9E3779B97F4A7C15 + (epoch << 40) + 0xD1B54A32D192ED03 + (p << 21) + 2 t        wrapping uint64
    h = mix32(x) << 32 | mix32(x + 1);  r = (h * T) >> 64
    item = the first unseen row whose inclusive prefix sum of weights exceeds r
Selection: key(i) = ord_bits(score_i) << 32 | (0xFFFFFFFF - i) over the eligible rows, larger first.
"""
from __future__ import annotations

import numpy as np

from tests.sampler_reference import mix32

_M64 = (1 << 64) - 1
SALT = 0xD1B54A32D192ED03


def weighted_draws(unseen_rows: np.ndarray, weights: np.ndarray, p: int, C: int, seed: int, epoch: int) -> np.ndarray:
    """(C,) int32: the draws of query ``p`` over ``unseen_rows`` (ascending); all -1 when there are none."""
    if len(unseen_rows) == 0:
        return np.full(C, -1, np.int32)
    cum = np.cumsum(np.asarray(weights, np.uint64)[unseen_rows], dtype=np.uint64)
    T = int(cum[-1])
    base = (seed * 0x9E3779B97F4A7C15 + (epoch << 40) + SALT + (p << 21)) & _M64
    with np.errstate(over="ignore"):
        x = np.uint64(base) + np.uint64(2) * np.arange(C, dtype=np.uint64)
        hi, lo = mix32(x), mix32(x + np.uint64(1))
    r = np.array([(((int(a) << 32) | int(b)) * T) >> 64 for a, b in zip(hi, lo)], dtype=np.uint64)
    return np.asarray(unseen_rows)[np.searchsorted(cum, r, side="right")].astype(np.int32)


def sample_weighted(unseen, user_of, weights, C: int, seed: int, epoch: int) -> np.ndarray:
    """(Q, C) int32.  ``unseen``: per user its ascending unseen rows; a user outside the list yields -1."""
    out = np.empty((len(user_of), C), np.int32)
    for p, u in enumerate(user_of):
        rows = unseen[u] if 0 <= u < len(unseen) else np.zeros(0, np.int64)
        out[p] = weighted_draws(rows, weights, p, C, seed, epoch)
    return out


def ord_bits(s: np.ndarray) -> np.ndarray:
    """Order-preserving uint32 of float32 scores, -0.0 as +0.0."""
    s = np.asarray(s, np.float32).copy()
    s[s == 0] = 0.0
    b = s.view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000).astype(np.uint64)


def catalogue_topk(scores, seen_sets, user_of, targets, K: int, exclude_seen: bool, n_users: int):
    """(items (Q, K) int32, scores (Q, K) float32, rank (Q,) int32, status [NaN, bad users, bad targets])."""
    scores = np.asarray(scores, np.float32)
    Q, n = scores.shape
    items = np.full((Q, K), -1, np.int32)
    top = np.full((Q, K), -np.inf, np.float32)
    rank = np.full(Q, -1, np.int32)
    status = [0, 0, 0]
    for q in range(Q):
        u, t = int(user_of[q]), int(targets[q])
        if t < -1 or t >= n:
            status[2] += 1
            t = -1
        if not 0 <= u < n_users:
            status[1] += 1
            continue
        eligible = np.ones(n, bool)
        if exclude_seen:
            eligible[list(seen_sets[u])] = False
        if t >= 0:
            eligible[t] = True
        rows = np.flatnonzero(eligible)
        status[0] += int(np.isnan(scores[q, rows]).sum())
        key = (ord_bits(scores[q]) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))
        order = rows[np.argsort(key[rows])[::-1]]            # the keys are distinct
        m = min(K, order.size)
        items[q, :m], top[q, :m] = order[:m], scores[q, order[:m]]
        if t >= 0:
            rank[q] = int((key[rows] > key[t]).sum())
    return items, top, rank, status


def full_ranking_metrics(rank: np.ndarray, ks) -> dict:
    """HR@k / NDCG@k of 0-based ranks (-1: no target) in ``CatalogueScorer.evaluate``'s order: a histogram of the
    ranks below max(ks), one float64 term count * (1 / log2(rank + 2)) per rank added in ascending rank order, then
    one division by the number of queries with a target."""
    rank = np.asarray(rank, np.int64)
    users = np.float64((rank >= 0).sum())
    if not users:
        return {}
    kmax = max(ks)
    hist = np.bincount(rank[(rank >= 0) & (rank < kmax)], minlength=kmax)
    gain = 1.0 / np.log2(np.arange(kmax, dtype=np.float64) + 2.0)
    out, acc = {}, np.float64(0.0)
    sums = {}
    for r in range(kmax):
        acc = acc + np.float64(hist[r]) * gain[r]
        sums[r + 1] = acc
    for k in ks:
        out[f"HR@{k}"] = float(np.float64(hist[:k].sum()) / users)
        out[f"NDCG@{k}"] = float(sums[k] / users)
    return out
