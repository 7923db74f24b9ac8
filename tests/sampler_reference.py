"""numpy restatement of ``csrc/sampler.hip``: the negative draw and the batch-record assembly, written from their
specification and sharing no code with the HIP side.  Every output is integer ids or copied float bits, so the
GPU tests compare bit for bit.

Draw t of positive p (t = 0..K-1), U = the user's unseen count:
    h = mix32(seed * 0x9E3779B97F4A7C15 + (epoch << 40) + 16 p + t)          wrapping uint64
    r = (uint64(h) * (U - t)) >> 32
    for every rank q already drawn for p, ascending:  if r >= q: r += 1
    item = the r-th (0-based) unseen item row of the user, ascending
Virtual rows of an epoch: j < P is positive j; j >= P is negative t = (j - P) % K of positive p = (j - P) // K with
item = neg_items[p][t], label 0; a column is the positive's value (COPY), the item table's row (ITEM) or a bucket of
ctx[p] - item_val[item] (BUCKET_DIFF).
"""
from __future__ import annotations

import numpy as np

COPY, ITEM, BUCKET_DIFF = 0, 1, 2
_M64 = (1 << 64) - 1


def mix32(x: np.ndarray) -> np.ndarray:
    """The library's counter hash (csrc/dropout.h) on a uint64 array -> uint32."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xff51afd7ed558ccd)
        x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xc4ceb9fe1a85ec53)
        x = x ^ (x >> np.uint64(33))
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def unseen_lists(seen_sets, n_items: int):
    """Per user, the ascending item rows it has not seen.  ``seen_sets``: per user, an iterable of seen rows."""
    return [np.setdiff1d(np.arange(n_items, dtype=np.int64), np.asarray(sorted(s), dtype=np.int64)) for s in seen_sets]


def sample_negatives(unseen, user_of, K: int, seed: int, epoch: int) -> np.ndarray:
    """(P, K) int32 item rows.  ``unseen``: ``unseen_lists``; ``user_of`` (P,) user rows."""
    user_of = np.asarray(user_of, dtype=np.int64)
    P = user_of.size
    counts = np.array([len(u) for u in unseen], dtype=np.uint64)
    table = np.full((len(unseen), max(int(counts.max()), 1)), -1, np.int64)
    for u, rows in enumerate(unseen):
        table[u, :len(rows)] = rows
    U = counts[user_of]
    assert (U >= K).all(), "a user has fewer than K unseen items"
    base = np.uint64((seed * 0x9E3779B97F4A7C15 + (epoch << 40)) & _M64)
    p = np.arange(P, dtype=np.uint64)
    drawn = np.zeros((P, 0), np.uint64)                   # ascending per row
    out = np.zeros((P, K), np.int32)
    for t in range(K):
        with np.errstate(over="ignore"):
            h = mix32(base + np.uint64(16) * p + np.uint64(t)).astype(np.uint64)
        r = (h * (U - np.uint64(t))) >> np.uint64(32)
        for i in range(t):
            r = r + (r >= drawn[:, i]).astype(np.uint64)
        drawn = np.sort(np.concatenate([drawn, r[:, None]], axis=1), axis=1)
        out[:, t] = table[user_of, r.astype(np.int64)]
    return out


def bucket_ids_of(ctx_p: np.ndarray, item_v: np.ndarray, edges: np.ndarray, bucket_ids: np.ndarray) -> np.ndarray:
    """BUCKET_DIFF ids of paired float32 operands."""
    x, y = np.asarray(ctx_p, np.float32), np.asarray(item_v, np.float32)
    with np.errstate(invalid="ignore"):
        d = (x - y).astype(np.float32)
        zero = np.isnan(x) | np.isnan(y) | (d < 0)
        b = 1 + (np.asarray(edges, np.float32)[None, :] <= d[:, None]).sum(axis=1)
    return np.asarray(bucket_ids, np.int64)[np.where(zero, 0, b)]


def assemble(layout, columns, rows: np.ndarray, K: int = 0, neg_items=None, item_features=None, roles=None,
             derived=None) -> np.ndarray:
    """The record (uint8, ``layout.record_bytes``) of the virtual rows ``rows`` (at most ``layout.batch_size``; the
    slots past them are zeros).  ``columns``: a ``PackedColumns`` of the positives; ``item_features``: name -> the item
    table's column; ``roles``: name -> COPY / ITEM / BUCKET_DIFF; ``derived``: name -> (ctx, item_val, edges,
    bucket_ids)."""
    rows = np.asarray(rows, dtype=np.int64)
    P, cnt = len(columns), rows.size
    rec = np.zeros(layout.record_bytes, np.uint8)
    batch, labels = layout.unpack(rec)
    neg = rows >= P
    p = np.where(neg, (rows - P) // max(K, 1), rows)         # the positive a row takes its COPY columns from
    item = np.zeros(cnt, np.int64)
    if neg.any():
        item[neg] = np.asarray(neg_items, np.int64).reshape(-1)[rows[neg] - P]
    labels[:cnt] = np.where(neg, np.float32(0), columns.labels[p])
    si = di = qi = 0
    for name, spec in columns.schema.fields.items():
        kind = spec.feature_type.value
        if kind == "sparse":
            src = columns.ids[si]; si += 1
        elif kind == "dense":
            src = columns.dense[di]; di += 1
        else:
            src = columns.bags[qi]; qi += 1
        val = src[p].copy()
        role = (roles or {}).get(name, COPY)
        if neg.any() and role == ITEM:
            val[neg] = np.asarray(item_features[name])[item[neg]]
        elif neg.any() and role == BUCKET_DIFF:
            ctx, item_val, edges, ids = derived[name]
            val[neg] = bucket_ids_of(np.asarray(ctx)[p[neg]], np.asarray(item_val)[item[neg]], edges, ids)
        batch[name][:cnt] = val
    return rec
