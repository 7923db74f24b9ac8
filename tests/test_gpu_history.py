"""GPU: user histories on the device (``csrc/history.hip``, ``DeviceInteractionLog.history_index``,
``DeviceHistoryIndex.lookup`` / ``latest``) against the vectorised numpy restatement ``tests/history_reference.py``.
Every comparison is exact (integers, or bytes), and every device call runs twice and must give the same bits: the
kernels use plain stores only.

1. index + lookup + latest over users whose segments are 0, 1, 63, 64, 65, 129 and 200 rows (no trip, one trip, the
   trip edge, two trips plus one, several trips), a user at one timestamp, a user without an event, every option;
2. the leave-one-out shape: validation and test rows see training rows only, each earlier than the query;
3. the refusals that come from the status words;
4. end to end: the bag as a SEQUENCE column of ``DeviceColumns.from_device`` through ``NegativeSampler``,
   ``DeviceEpochLoader`` and two steps of ``FusedMixedDeepFMStep``.
"""
import itertools

import numpy as np
import pytest
import torch

from tests import history_reference as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_ITEMS, TS_RANGE = 40, 25
LENGTHS = (1, 3, 8, 64, 200)
EDGES = (0, 1, 63, 64, 65, 129, 200)
SEGMENTS = {                       # per n_users, the logs as segment lengths per user
    1: [(s,) for s in EDGES],
    3: [(65, 0, 200), (63, 64, 129), (1, 129, 64)],
    70: [EDGES + tuple(np.random.default_rng(70).integers(0, 40, 70 - len(EDGES)).tolist())],
}


def _np(t):
    return t.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _twice(f):
    """f() twice; the two results (tuples of tensors) must be equal bits.  Returns the first as numpy."""
    a, b = f(), f()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    return [_np(x) for x in a]


def _parts(h):
    assert h.bag.is_contiguous() and h.bag.dtype == h.count.dtype == h.gap.dtype == torch.int64
    return h.bag, h.count, h.gap


def make_log(segments, rng):
    """Shuffled rows.  With three users or more, the user with the most rows has all of them at one timestamp and the
    one with the second most has no event (all its labels are 0); a lone user of 64 or 129 rows is at one timestamp.
    Returns the log, its host columns and the user without an event (or None)."""
    from deepfm_amd.data import DeviceInteractionLog
    n_users = len(segments)
    by_size = np.argsort(segments, kind="stable")
    one_time = int(by_size[-1]) if n_users >= 3 or segments[0] in (64, 129) else None
    no_event = int(by_size[-2]) if n_users >= 3 else None
    user = np.repeat(np.arange(n_users, dtype=np.int64), segments)
    user = user[rng.permutation(len(user))]
    n = len(user)
    item = rng.integers(0, N_ITEMS, n).astype(np.int64)
    ts = rng.integers(100, 100 + TS_RANGE, n).astype(np.int64)
    labels = (rng.random(n) < 0.6).astype(np.float32)
    if one_time is not None:
        ts[user == one_time] = 111
    if no_event is not None:
        labels[user == no_event] = 0
    log = DeviceInteractionLog(user, item, ts, labels, n_users, N_ITEMS, DEV)
    return log, (user, item, ts, labels), no_event


def query_rows(n, rng):
    """The whole log, a shuffled subset with repeats, a single row."""
    if n == 0:
        return [np.zeros(0, np.int64)]
    return [np.arange(n, dtype=np.int64), rng.integers(0, n, n // 2 + 3).astype(np.int64), np.array([n // 2], np.int64)]


# ----------------------------------------------------------------------------- 1. index, lookup, latest
@pytest.mark.parametrize("n_users", [1, 3, 70])
def test_lookup_and_latest_equal_the_restatement(n_users):
    rng = np.random.default_rng(n_users)
    checked = 0
    for segments in SEGMENTS[n_users]:
        log, host, no_event = make_log(segments, rng)
        n = len(log)
        assert sorted(np.bincount(host[0], minlength=n_users).tolist()) == sorted(segments)
        ids = rng.integers(1, 500, N_ITEMS).astype(np.int64)
        ids[[5, 17]] = 0                                          # two items share the padding id
        half = _dev(rng.permutation(n)[:n // 2].astype(np.int64))
        rows_list = query_rows(n, rng)
        users = np.arange(n_users, dtype=np.int64)
        for source, positives_only, item_ids in itertools.product((None, half), (True, False), (None, ids)):
            kw = dict(source=None if source is None else _np(source), positives_only=positives_only, item_ids=item_ids)
            index = log.history_index(source, positives_only, None if item_ids is None else _dev(item_ids))
            again = log.history_index(source, positives_only, item_ids)            # a numpy map is taken too
            for name in ("start", "pos_of", "rank", "sorted_ts", "event_count"):
                assert torch.equal(getattr(index, name), getattr(again, name)), name
            counts = _np(index.event_count)
            want_latest = H.histories(*host, users, max(LENGTHS), ties="latest", **kw)
            assert np.array_equal(counts, want_latest[1])
            if no_event is not None and positives_only:
                assert segments[no_event] >= 64 and counts[no_event] == 0
            for L in LENGTHS:
                bag, count, gap = _twice(lambda: _parts(index.latest(_dev(users), L)))
                assert bag.shape == (n_users, L) and np.array_equal(bag, want_latest[0][:, :L])
                assert np.array_equal(count, want_latest[1]) and (gap == -1).all()
            for ties in ("position", "exclude"):
                want = H.histories(*host, np.arange(n), max(LENGTHS), ties=ties, **kw)
                for L, rows in itertools.product(LENGTHS, rows_list):
                    d_rows = _dev(rows)
                    bag, count, gap = _twice(lambda: _parts(index.lookup(d_rows, L, ties)))
                    assert bag.shape == (len(rows), L) and count.shape == gap.shape == (len(rows),)
                    assert np.array_equal(bag, want[0][rows, :L]), (segments, ties, L, kw)
                    assert np.array_equal(count, want[1][rows]) and np.array_equal(gap, want[2][rows])
                    checked += 1
                if n_users == 70:
                    assert (want[1] > 8).any() and (want[1] == 0).any()      # L below some counts and above others
    assert checked >= 2 * 2 * 2 * 2 * len(LENGTHS)


def test_an_empty_query_gives_empty_outputs():
    log, _, _ = make_log((5, 3), np.random.default_rng(0))
    index = log.history_index()
    for h in (index.lookup(torch.zeros(0, dtype=torch.int64, device=DEV), 7),
              index.latest(torch.zeros(0, dtype=torch.int64, device=DEV), 7)):
        assert h.bag.shape == (0, 7) and h.count.shape == h.gap.shape == (0,) and h.bag.is_cuda


# ----------------------------------------------------------------------------- 2. the leave-one-out shape
def test_validation_and_test_rows_see_training_rows_only():
    """Every row is its own item, so a bag entry names the log row it came from."""
    from deepfm_amd.data import DeviceInteractionLog
    rng = np.random.default_rng(3)
    n, n_users, L = 500, 11, 16
    user = rng.integers(0, n_users, n).astype(np.int64)
    item = np.arange(n, dtype=np.int64)
    ts = rng.integers(0, TS_RANGE, n).astype(np.int64)
    labels = (rng.random(n) < 0.7).astype(np.float32)
    log = DeviceInteractionLog(user, item, ts, labels, n_users, n, DEV)
    split = log.leave_one_out_split(3)
    index = log.history_index(source=split.train)
    train = set(_np(split.train).tolist())
    for part in (split.val, split.test, split.train):
        rows = _np(part)
        bag, count, gap = _twice(lambda: _parts(index.lookup(part, L)))
        want = H.histories(user, item, ts, labels, rows, L, source=_np(split.train))
        assert all(np.array_equal(g, w) for g, w in zip((bag, count, gap), want))
        for q, entries in zip(rows, bag):
            events = entries[entries != 0] - 1
            assert set(events.tolist()) <= train and (user[events] == user[q]).all() and (labels[events] == 1).all()
            assert all((ts[e], e) < (ts[q], q) for e in events) and q not in events
    assert len(split.val) == len(split.test) == n_users and (count > 0).any()


# ----------------------------------------------------------------------------- 3. the status words
def test_queries_outside_the_log_and_users_outside_the_table_are_refused():
    from deepfm_amd import _lib
    log, host, _ = make_log((65, 0, 20), np.random.default_rng(4))
    n, index = len(log), log.history_index()
    with pytest.raises(ValueError, match=f"2 of 4 entries of rows are outside the log's {n} rows"):
        index.lookup(_dev(np.array([0, n, 3, -1], np.int64)), 4)
    with pytest.raises(ValueError, match="1 of 2 entries of rows are outside"):
        index.lookup(_dev(np.array([n + 7, 1], np.int64)), 4, ties="exclude")
    with pytest.raises(ValueError, match="2 of 3 entries of user_rows are outside the user table's 3 rows"):
        index.latest(_dev(np.array([3, 1, -1], np.int64)), 4)
    # the entry point itself: a refused query is counted, its outputs are zeros and -1, its neighbours are served
    q = _dev(np.array([1, n, 2, -5], np.int64))
    bag = torch.full((4, 6), 77, dtype=torch.int64, device=DEV)
    count, gap = torch.full((4,), 77, dtype=torch.int64, device=DEV), torch.full((4,), 77, dtype=torch.int64, device=DEV)
    status = torch.full((2,), 10, dtype=torch.int64, device=DEV)                # never cleared by the call
    _lib.check(_lib.load().dfm_history_gather(
        q.data_ptr(), 4, _lib.HISTORY_POSITION, 6, log.user_rows.data_ptr(), log.item_rows.data_ptr(),
        log.timestamps.data_ptr(), 0, index.start.data_ptr(), index.pos_of.data_ptr(), index.rank.data_ptr(),
        index.events.data_ptr(), index.sorted_ts.data_ptr(), index.event_count.data_ptr(), n, 3, N_ITEMS,
        bag.data_ptr(), count.data_ptr(), gap.data_ptr(), status.data_ptr(), _lib.stream_handle()))
    assert status.tolist() == [12, 10]
    want = H.histories(*host, np.array([1, 2]), 6)
    assert np.array_equal(_np(bag)[[0, 2]], want[0]) and np.array_equal(_np(count)[[0, 2]], want[1])
    assert np.array_equal(_np(gap)[[0, 2]], want[2])
    assert not _np(bag)[[1, 3]].any() and _np(count)[[1, 3]].tolist() == [0, 0] and _np(gap)[[1, 3]].tolist() == [-1, -1]


def test_a_log_with_a_row_outside_the_tables_is_refused_at_history_index():
    from deepfm_amd.data import DeviceInteractionLog
    user = np.array([0, 1, 2, 1, 0], np.int64)
    item = np.array([3, 2, 1, 0, 3], np.int64)
    ts, labels = np.arange(5, dtype=np.int64), np.ones(5, np.float32)
    for bad_user, bad_item in ((3, 1), (-1, 1), (1, 4), (1, -1)):
        u, i = user.copy(), item.copy()
        u[2], i[2] = bad_user, bad_item
        log = DeviceInteractionLog(u, i, ts, labels, 3, 4, DEV)
        with pytest.raises(ValueError, match="an interaction names a user or an item row outside the tables"):
            log.history_index()
    log = DeviceInteractionLog(user, item, ts, labels, 3, 4, DEV)
    with pytest.raises(ValueError, match="1 of 3 entries of source are outside the log's 5 rows"):
        log.history_index(source=_dev(np.array([0, 5, 1], np.int64)))
    with pytest.raises(ValueError, match="item_ids: an id is negative"):
        log.history_index(item_ids=_dev(np.array([1, -2, 3, 4], np.int64)))
    assert _np(log.history_index().latest(_dev(np.array([0], np.int64)), 3).bag).tolist() == [[4, 4, 0]]


# ----------------------------------------------------------------------------- 4. end to end
def _end_to_end():
    from deepfm_amd.data import (DeviceColumns, DeviceEpochLoader, DeviceInteractionLog, ItemTable, NegativeSampler,
                                 Role, history_field)
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    rng = np.random.default_rng(8)
    n, n_users, n_items, L, K, B = 600, 12, 40, 5, 2, 64
    user = rng.integers(0, n_users, n).astype(np.int64)
    item = rng.integers(0, n_items, n).astype(np.int64)
    ts = rng.integers(0, 60, n).astype(np.int64)
    labels = (rng.random(n) < 0.6).astype(np.float32)
    log = DeviceInteractionLog(user, item, ts, labels, n_users, n_items, DEV)
    split = log.leave_one_out_split(3)
    schema = DatasetSchema(fields={
        "user_id": FieldSchema("user_id", FeatureType.SPARSE, n_users + 1, 8, "user"),
        "item_id": FieldSchema("item_id", FeatureType.SPARSE, n_items + 1, 8, "item"),
        "hist": history_field("hist", L, n_items, 8)})
    rows = split.train
    hist = log.history_index(source=rows).lookup(rows, L)
    ids = torch.stack([log.user_rows[rows] + 1, log.item_rows[rows] + 1]).contiguous()
    dense = torch.empty(0, len(rows), dtype=torch.float32, device=DEV)
    dcols = DeviceColumns.from_device(schema, ids, dense, log.labels[rows].contiguous(), bags=[hist.bag])
    table = ItemTable(schema, {"item_id": np.arange(n_items, dtype=np.int64) + 1})
    sampler = NegativeSampler(dcols, log.seen_sets(), _np(log.user_rows[rows]).astype(np.int32), table, K, seed=6)
    assert sampler.roles == {"user_id": Role.COPY, "item_id": Role.ITEM, "hist": Role.COPY}
    loader = DeviceEpochLoader(dcols, B, shuffle=False, negatives=sampler, depth=2)
    loader.set_epoch(1)
    # the host columns of the epoch's P * (1 + K) virtual rows: the positives, then K negatives per positive, each
    # with its positive's user and bag and its own item
    r = _np(rows)
    P = len(r)
    want_bag = H.histories(user, item, ts, labels, r, L, source=r)[0]
    neg = loader.negatives_host(1)
    assert neg.shape == (P, K)
    of = np.concatenate([np.arange(P), np.repeat(np.arange(P), K)])
    host = PackedColumns(schema, {"user_id": user[r][of] + 1,
                                  "item_id": np.concatenate([item[r], neg.reshape(-1).astype(np.int64)]) + 1,
                                  "hist": want_bag[of]},
                         np.concatenate([labels[r], np.zeros(P * K, np.float32)]))
    assert (want_bag != 0).any() and not want_bag[:, L - 1].all() and want_bag[:, L - 1].any()
    return schema, loader, host, B


def test_the_bag_travels_through_the_sampler_the_loader_and_the_fused_step():
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    from deepfm_amd.training import DenseTableAdam, FusedMixedDeepFMStep
    schema, loader, host, B = _end_to_end()
    lay = loader.layout
    assert len(loader) >= 3 and len(host) == loader.rows
    host_records = []
    for k, rec in enumerate(loader):
        want = np.zeros(lay.record_bytes, np.uint8)
        lay.write(want, host, k * B, (k + 1) * B)
        assert np.array_equal(_np(rec), want), f"batch {k}"
        host_records.append(want)
    last = len(loader) - 1                                          # all negatives: every bag there is a copied one
    batch, labels = lay.unpack(host_records[last])
    assert not labels.any() and batch["hist"].any()

    losses = []
    for source in ("loader", "host"):
        cfg = ExperimentConfig()
        cfg.feature.fm_embed_dim = 8
        cfg.dnn.hidden_units = [32, 32]
        cfg.dnn.dropout = 0.1
        torch.manual_seed(3)
        model = create_model("deepfm", schema, cfg).cuda().train()
        model.embedding.strict_indices = True
        opt = DenseTableAdam(model, lr=1e-2, l2=1e-3, max_grad_norm=0.5)
        step = FusedMixedDeepFMStep(model, opt, B, use_graph=True)
        step.capture()
        got = []
        for k in (0, last):                                         # positives, then negatives
            step.run_from(loader.record(k) if source == "loader" else torch.from_numpy(host_records[k]).cuda())
            model.embedding.raise_on_bad_index()
            got.append(step.loss.clone())
        torch.cuda.synchronize()
        losses.append(got + [opt.flat_param.clone()])
    for a, b in zip(*losses):
        assert torch.equal(a, b)
    assert all(bool(torch.isfinite(x).all()) for x in losses[0])
