"""numpy restatement of ``deepfm_amd/data/interactions.py`` (and so of the reference's ``_temporal_split``,
``_leave_one_out_split``, ``_user_items`` and count features, ``deepfm/data/movielens.py:235-304, 334-344, 447-458``):
stable sorts, the quantile formula, the bitmap via ``SeenSets.from_interactions``.  Shared by the CPU and GPU tests;
``tests/golden/interactions_reference.npz`` pins it to what the reference's own methods gave."""
import math

import numpy as np


def quantile(sorted_values, q):
    """``pandas.Series.quantile(q)`` of an ascending int64 column as float64: pandas hands numpy the percentile
    ``q * 100.0``, numpy divides it by 100 and interpolates linearly between the two order statistics around the
    virtual index ``q * (n - 1)``, in its lerp form."""
    n = len(sorted_values)
    q = q * 100.0 / 100.0
    virtual = (n - 1) * q
    lo = min(int(math.floor(virtual)), n - 1)
    hi = min(lo + 1, n - 1)
    g = virtual - lo
    a, b = float(sorted_values[lo]), float(sorted_values[hi])
    d = b - a
    return b - d * (1.0 - g) if g >= 0.5 else a + d * g


def temporal_split(user_rows, timestamps, labels, val_ratio, test_ratio):
    """(train, val, test) int64 index arrays into the log and the two cutoffs.  Order: timestamp, ties by log
    position."""
    user_rows, ts, labels = np.asarray(user_rows), np.asarray(timestamps), np.asarray(labels)
    order = np.argsort(ts, kind="stable")
    st = ts[order]
    train_cutoff = quantile(st, 1 - val_ratio - test_ratio)
    val_cutoff = quantile(st, 1 - test_ratio)
    f = st.astype(np.float64)
    train = order[f <= train_cutoff]
    train_users = set(user_rows[train].tolist())

    def first_positive_per_user(window):
        first = {}
        for r in order[window]:
            u = int(user_rows[r])
            if labels[r] == 1.0 and u in train_users and u not in first:
                first[u] = int(r)
        return np.array([first[u] for u in sorted(first)], np.int64)

    val = first_positive_per_user((f > train_cutoff) & (f <= val_cutoff))
    test = first_positive_per_user(f > val_cutoff)
    return train.astype(np.int64), val, test, (train_cutoff, val_cutoff)


def leave_one_out_split(user_rows, timestamps, min_interactions):
    """(train, val, test): rows sorted by (user row, timestamp, log position); a user with at least
    ``min_interactions`` rows gives its last to test and its second-to-last to val."""
    user_rows, ts = np.asarray(user_rows), np.asarray(timestamps)
    by_time = np.argsort(ts, kind="stable")
    order = by_time[np.argsort(user_rows[by_time], kind="stable")]
    train, val, test = [], [], []
    start, n = 0, len(order)
    while start < n:
        end = start
        while end < n and user_rows[order[end]] == user_rows[order[start]]:
            end += 1
        group = order[start:end].tolist()
        if len(group) >= min_interactions:
            test.append(group[-1]); val.append(group[-2]); train += group[:-2]
        else:
            train += group
        start = end
    return tuple(np.array(p, np.int64) for p in (train, val, test))


def entity_counts(entity_rows, n_entities, labels=None, rows=None):
    entity_rows = np.asarray(entity_rows)
    rows = np.arange(len(entity_rows)) if rows is None else np.asarray(rows)
    e = entity_rows[rows]
    if labels is not None:
        e = e[np.asarray(labels)[rows] == 1.0]
    return np.bincount(e, minlength=n_entities).astype(np.int64)


def count_feature_table(counts):
    """The reference's count feature per entity: MinMaxScaler fitted on log1p of the counts that exist, applied to
    log1p of every count, float64, then float32."""
    c = np.asarray(counts, dtype=np.float64)
    log = np.log1p(c)
    fitted = log[c >= 1]
    lo, hi = float(fitted.min()), float(fitted.max())
    if hi - lo == 0:
        return np.zeros(len(c), np.float32)
    return ((log - lo) / (hi - lo)).astype(np.float32)


def seen_pairs(user_rows, item_rows):
    """The distinct (user row, item row) pairs, sorted: ``_user_items`` flattened."""
    return np.unique(np.stack([np.asarray(user_rows), np.asarray(item_rows)], axis=1), axis=0)


def pairs_of_bitmap(bitmap, n_items):
    """The (user row, item row) pairs whose bit is set in a ``SeenSets`` bitmap, sorted, the tail bits left out."""
    bits = np.unpackbits(np.ascontiguousarray(bitmap).view(np.uint8), axis=1, bitorder="little")[:, :n_items]
    u, i = np.nonzero(bits)
    return np.stack([u, i], axis=1).astype(np.int64)
