"""numpy restatement of the ragged candidate lists (``csrc/sampler.hip``: ``dfm_sample_negatives``,
``dfm_sample_weighted`` and the assemble plan over a ``dfm_candidate_list``), written from their specification in
``include/deepfm_hip.h`` on top of ``tests/sampler_reference.py`` and ``tests/candidates_reference.py`` and sharing no
code with the HIP side.  Every output is integer rows or copied float bits, so the GPU tests compare bit for bit.

The reference's rule (``movielens.py:575-580``): a user with U unseen rows gets ``min(num_neg, U)`` candidates.
    counts[q]  = min(num_neg, U(user_of[q]));  offsets = the exclusive scan of counts, offsets[Q] = total
    draw t < counts[q] of query q is entry offsets[q] + t of one flat list, hashed by (seed, epoch, q, t) exactly as
    draw t of the rectangular list: a query that is not short receives the same items
Virtual rows of a ragged epoch: j < P is positive j; j >= P is candidate c = j - P of the flat list, which belongs to
the query p with offsets[p] <= c < offsets[p + 1].
"""
from __future__ import annotations

import numpy as np

from tests import candidates_reference as CR
from tests import sampler_reference as R

_M64 = (1 << 64) - 1


def counts_offsets(seen, user_of, num_neg: int, n_items: int):
    """(counts (Q,) int32, offsets (Q + 1,) int64).  ``seen``: per user, an iterable of its seen item rows, all inside
    [0, n_items).  A query whose user row is outside the list keeps ``num_neg`` entries (the draws write -1 there, as
    the rectangular ones do)."""
    unseen = np.array([n_items - len(set(s)) for s in seen], np.int64)
    user_of = np.asarray(user_of, np.int64)
    inside = (user_of >= 0) & (user_of < len(unseen))
    counts = np.where(inside, np.minimum(num_neg, unseen[np.where(inside, user_of, 0)]), num_neg).astype(np.int32)
    offsets = np.zeros(user_of.size + 1, np.int64)
    np.cumsum(counts, dtype=np.int64, out=offsets[1:])
    return counts, offsets


def _uniform_draws(rows: np.ndarray, p: int, n: int, seed: int, epoch: int) -> np.ndarray:
    """The first ``n`` uniform draws without replacement of positive ``p`` over its user's ascending unseen ``rows``
    (``sampler_reference``'s draw, one query at a time); -1 once the rows are used up."""
    base = (seed * 0x9E3779B97F4A7C15 + (epoch << 40)) & _M64
    U, drawn, out = len(rows), [], np.full(n, -1, np.int32)
    for t in range(min(n, U)):
        h = int(R.mix32(np.array([(base + 16 * p + t) & _M64], np.uint64))[0])
        r = (h * (U - t)) >> 32
        for q in drawn:                                    # ascending
            r += r >= q
        drawn = sorted(drawn + [r])
        out[t] = rows[r]
    return out


def sample_negatives_ragged(unseen, user_of, counts, seed: int, epoch: int) -> np.ndarray:
    """(sum(counts),) int32: the flat list of the uniform draw.  ``unseen``: ``sampler_reference.unseen_lists``; a
    user row outside it yields -1 entries."""
    parts = [np.zeros(0, np.int32)]
    for p, (u, n) in enumerate(zip(user_of, counts)):
        parts.append(_uniform_draws(unseen[u], p, int(n), seed, epoch) if 0 <= u < len(unseen)
                     else np.full(int(n), -1, np.int32))
    return np.concatenate(parts)


def sample_weighted_ragged(unseen, user_of, weights, counts, seed: int, epoch: int) -> np.ndarray:
    """(sum(counts),) int32: the flat list of the weighted draw, ``candidates_reference.weighted_draws`` per query with
    its own count."""
    parts = [np.zeros(0, np.int32)]
    for p, (u, n) in enumerate(zip(user_of, counts)):
        rows = unseen[u] if 0 <= u < len(unseen) else np.zeros(0, np.int64)
        parts.append(CR.weighted_draws(rows, weights, p, int(n), seed, epoch))
    return np.concatenate(parts)


def virtual_row_map(offsets, P: int):
    """(p, t) per candidate c of the flat list, each (total,) int64: c is candidate t of query p, i.e. virtual row
    P + c.  Written as the definition, a walk over the queries, not as a search."""
    offsets = np.asarray(offsets, np.int64)
    assert offsets.shape == (P + 1,) and offsets[0] == 0 and (np.diff(offsets) >= 0).all()
    p = np.concatenate([np.zeros(0, np.int64)] + [np.full(int(offsets[q + 1] - offsets[q]), q, np.int64) for q in range(P)])
    return p, np.arange(int(offsets[P]), dtype=np.int64) - offsets[p]


def virtual_rows(columns, offsets, neg_items, item_features, roles, derived):
    """Every virtual row of a ragged epoch as ``PackedColumns`` (P + total rows, in row order), so that a batch record
    of rows ``idx`` is ``RecordLayout.write_indexed(out, virtual_rows(...), idx)``.  Arguments as
    ``sampler_reference.assemble``; ``neg_items`` is the flat list, every entry a valid item row."""
    from deepfm_amd.data.packed import PackedColumns
    P = len(columns)
    p_of, _ = virtual_row_map(offsets, P)
    item = np.asarray(neg_items, np.int64).reshape(-1)
    assert item.shape == p_of.shape
    src = np.concatenate([np.arange(P, dtype=np.int64), p_of])   # the positive a row takes its COPY columns from
    feats, si, di, qi = {}, 0, 0, 0
    for name, spec in columns.schema.fields.items():
        kind = spec.feature_type.value
        if kind == "sparse":
            col = columns.ids[si]; si += 1
        elif kind == "dense":
            col = columns.dense[di]; di += 1
        else:
            col = columns.bags[qi]; qi += 1
        val = col[src].copy()
        role = (roles or {}).get(name, R.COPY)
        if item.size and role == R.ITEM:
            val[P:] = np.asarray(item_features[name])[item]
        elif item.size and role == R.BUCKET_DIFF:
            ctx, item_val, edges, ids = derived[name]
            val[P:] = R.bucket_ids_of(np.asarray(ctx)[p_of], np.asarray(item_val)[item], edges, ids)
        feats[name] = val
    labels = np.concatenate([columns.labels, np.zeros(item.size, np.float32)])
    return PackedColumns(columns.schema, feats, labels)


def take(rows_columns, idx):
    """The rows ``idx`` of ``virtual_rows(...)`` as ``PackedColumns`` of their own, in that order."""
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.schema import FeatureType
    idx = np.asarray(idx, np.int64)
    its = {FeatureType.SPARSE: iter(rows_columns.ids), FeatureType.DENSE: iter(rows_columns.dense),
           FeatureType.SEQUENCE: iter(rows_columns.bags)}
    feats = {name: next(its[spec.feature_type])[idx] for name, spec in rows_columns.schema.fields.items()}
    return PackedColumns(rows_columns.schema, feats, rows_columns.labels[idx])


def record_of(layout, rows_columns, idx) -> np.ndarray:
    """The record of the virtual rows ``idx`` (at most ``layout.batch_size``; the slots past them are zeros)."""
    from deepfm_amd.data.packed import RecordLayout
    idx = np.asarray(idx, np.int64)
    rec = np.zeros(layout.record_bytes, np.uint8)
    if idx.size == layout.batch_size:
        layout.write_indexed(rec, rows_columns, idx)
        return rec
    short = RecordLayout.of(rows_columns.schema, idx.size)    # a partial batch: gather, then place slot by slot
    part = np.zeros(short.record_bytes, np.uint8)
    short.write_indexed(part, rows_columns, idx)
    for dst, srcv in zip(_blocks(layout.views(rec)), _blocks(short.views(part))):
        dst[..., :idx.size] = srcv
    return rec


def _blocks(views):
    """The views of a record with the sample axis last."""
    ids, dense, labels, bags = views
    return [ids, dense, labels] + [b.T for b in bags]
