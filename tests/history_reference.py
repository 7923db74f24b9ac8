"""Numpy restatements of the user histories of ``deepfm_amd/data/interactions.py`` (DESIGN.md §7b "User histories on
the device"), two of them, written independently of each other:

``histories``              vectorised: ``np.lexsort``, cumulative counts, fancy indexing;
``histories_brute_force``  the definition applied literally, per query over all rows, O(n m).

The definition.  The log's order is (user row, timestamp, log position).  An event is a log row ``e`` that is in
``source`` (None: every row; duplicates collapse) and, with ``positives_only``, has ``labels[e] == 1``.  A query is a
log row ``q`` of user ``u`` at time ``t`` (an event or not, repeats allowed); its prior set is

    ties="position"   the events e of u with (ts[e], e) < (t, q), lexicographically
    ties="exclude"    the events e of u with ts[e] < t
    ties="latest"     every event of u; the query is then a USER row, and there is no query time

Ordered latest first by (ts, e) as e_0, e_1, ...:  ``bag[j] = item_ids[item[e_j]]`` for ``j < min(L, |prior|)`` and 0
behind; ``count = |prior|``; ``gap = t - ts[e_0]``, -1 for an empty prior set and always for "latest".  ``item_ids``
defaults to item row + 1.  All three outputs are int64.
"""
import numpy as np

TIES = ("position", "exclude", "latest")


def _events(n, labels, source, positives_only):
    is_event = np.ones(n, bool)
    if source is not None:
        is_event[:] = False
        is_event[np.asarray(source, np.int64)] = True
    if positives_only:
        is_event &= np.asarray(labels) == 1
    return is_event


def _ids(item, item_ids):
    item = np.asarray(item, np.int64)
    return item + 1 if item_ids is None else np.asarray(item_ids, np.int64)[item]


def histories(user, item, ts, labels, queries, L, ties="position", source=None, positives_only=True, item_ids=None):
    """(bag (m, L), count (m,), gap (m,)), vectorised."""
    assert ties in TIES
    user, ts, queries = np.asarray(user, np.int64), np.asarray(ts, np.int64), np.asarray(queries, np.int64)
    n, m = len(user), len(queries)
    ids = _ids(item, item_ids)
    order = np.lexsort((np.arange(n), ts, user))                  # by user, then timestamp, then position
    ev = _events(n, labels, source, positives_only)[order]
    before = np.zeros(n + 1, np.int64)                            # before[p]: events at sorted positions < p
    np.cumsum(ev, out=before[1:])
    ev_rows = order[ev]                                           # every event, in the log's order
    su, st = user[order], ts[order]
    u = queries if ties == "latest" else user[queries]
    seg = np.searchsorted(su, u, side="left")                     # the first position of the user's segment
    if ties == "latest":
        at = np.searchsorted(su, u, side="right")
    elif ties == "position":
        pos_of = np.empty(n, np.int64)
        pos_of[order] = np.arange(n)
        at = pos_of[queries]
    else:                                                         # the first position of the (user, timestamp) run
        lo = int(ts.min()) if n else 0
        span = (int(ts.max()) - lo + 1) if n else 1
        at = np.searchsorted(su * span + (st - lo), u * span + (ts[queries] - lo), side="left")
    first = before[seg]                                           # the user's events start here in ev_rows
    count = before[at] - first
    j = np.arange(L, dtype=np.int64)[None, :]
    valid = j < count[:, None]
    where = np.where(valid, (first + count)[:, None] - 1 - j, 0)
    bag = np.where(valid, ids[ev_rows[where]] if len(ev_rows) else 0, 0).astype(np.int64)
    gap = np.full(m, -1, np.int64)
    if ties != "latest" and len(ev_rows):
        has = count > 0
        gap[has] = ts[queries[has]] - ts[ev_rows[(first + count - 1)[has]]]
    return bag.reshape(m, L), count.astype(np.int64), gap


def histories_brute_force(user, item, ts, labels, queries, L, ties="position", source=None, positives_only=True,
                          item_ids=None):
    """The same, by the definition: per query, every row of the log is asked whether it is a prior event."""
    assert ties in TIES
    n = len(user)
    in_source = None if source is None else set(int(s) for s in source)
    bags, counts, gaps = [], [], []
    for q in queries:
        q = int(q)
        u = q if ties == "latest" else int(user[q])
        prior = []
        for e in range(n):
            if in_source is not None and e not in in_source:
                continue
            if positives_only and labels[e] != 1:
                continue
            if int(user[e]) != u:
                continue
            if ties == "position" and not (int(ts[e]), e) < (int(ts[q]), q):
                continue
            if ties == "exclude" and not int(ts[e]) < int(ts[q]):
                continue
            prior.append(e)
        prior.sort(key=lambda e: (int(ts[e]), e), reverse=True)
        bag = [0] * L
        for j, e in enumerate(prior[:L]):
            bag[j] = int(item[e]) + 1 if item_ids is None else int(item_ids[int(item[e])])
        bags.append(bag)
        counts.append(len(prior))
        gaps.append(int(ts[q]) - int(ts[prior[0]]) if prior and ties != "latest" else -1)
    return (np.array(bags, np.int64).reshape(len(queries), L), np.array(counts, np.int64), np.array(gaps, np.int64))
