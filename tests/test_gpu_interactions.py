"""GPU: the interaction log on the device (``csrc/interactions.hip``, ``deepfm_amd/data/interactions.py``) against the
numpy restatement (``tests/interactions_reference.py``), ``SeenSets.from_interactions``, ``np.bincount`` and what the
reference's own adapter methods gave (``tests/golden/interactions_reference.npz``).  Every comparison is exact, and every
device call runs twice and must give the same bits: the kernels use integer atomics and plain stores only."""
import os

import numpy as np
import pytest
import torch

from tests import interactions_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interactions_reference.npz")
RATIOS = [(0.1, 0.1), (0.2, 0.2), (0.0, 0.1)]


@pytest.fixture(scope="module")
def G():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _np(t):
    return t.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _log(user, item, ts, labels, n_users, n_items):
    from deepfm_amd.data import DeviceInteractionLog
    return DeviceInteractionLog(np.asarray(user, np.int64), np.asarray(item, np.int64), np.asarray(ts, np.int64),
                                np.asarray(labels, np.float32), n_users, n_items, DEV)


def _twice(f):
    """f() twice; the two results (tuples of tensors) must be equal bits.  Returns the first as numpy."""
    a, b = f(), f()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    return [_np(x) for x in a]


# ---------------------------------------------------------------------------------------------------- seen-sets
def _interactions(n_users, n_items, n, rng):
    """n random interactions plus: user 0 has seen every item, the last user (when there are three or more) has no
    row, and every row of the first block is there twice."""
    u = rng.integers(0, max(n_users - 1, 1), n) if n_users >= 3 else rng.integers(0, n_users, n)
    i = rng.integers(0, n_items, n)
    u = np.concatenate([u, u[:50], np.zeros(n_items, np.int64)])
    i = np.concatenate([i, i[:50], np.arange(n_items)])
    perm = rng.permutation(len(u))
    return u[perm].astype(np.int64), i[perm].astype(np.int64)


def _seen_equal(n_users, n_items, u, i):
    from deepfm_amd.data import SeenSets
    from deepfm_amd.data.interactions import device_seen_sets
    want = SeenSets.from_interactions(u, i, n_users, n_items)
    du, di = _dev(u), _dev(i)
    bitmap, prefix = _twice(lambda: device_seen_sets(du, di, n_users, n_items).upload(DEV))
    assert bitmap.dtype == np.int32 and bitmap.shape == want.bitmap.shape and prefix.shape == want.prefix.shape
    assert np.array_equal(bitmap.view(np.uint32), want.bitmap), (n_users, n_items)
    assert np.array_equal(prefix.view(np.uint32), want.prefix), (n_users, n_items)
    return want


@pytest.mark.parametrize("n_users", [1, 3, 70])
def test_seen_sets_equal_the_host_builder(n_users):
    """Every word count around one word and two, a prefix of more than one 64-word trip (2053 items: 65 words), a
    scatter of several workgroups; duplicates, a user without a row, a user who has seen everything, an empty log."""
    rng = np.random.default_rng(n_users)
    for n_items in (1, 31, 32, 33, 64, 65, 2053):
        u, i = _interactions(n_users, n_items, 3000 if n_items == 65 else 200, rng)
        want = _seen_equal(n_users, n_items, u, i)
        assert want.unseen[0] == 0
        if n_users >= 3:
            assert want.unseen[n_users - 1] == n_items
        empty = _seen_equal(n_users, n_items, np.zeros(0, np.int64), np.zeros(0, np.int64))
        assert (empty.unseen == n_items).all()


def test_seen_sets_count_rows_outside_the_tables_and_the_mirror_raises():
    from deepfm_amd import _lib
    from deepfm_amd.data import SeenSets
    from deepfm_amd.data.interactions import device_seen_sets
    n_users, n_items, W = 3, 33, 2
    u = np.array([0, 1, -1, 3, 2, 2, 1, 0], np.int64)
    i = np.array([5, 32, 4, 4, 33, -1, 31, 0], np.int64)                      # four bad rows: -1, 3 | 33, -1
    good = (u >= 0) & (u < n_users) & (i >= 0) & (i < n_items)
    assert good.sum() == 4
    du, di = _dev(u), _dev(i)
    bitmap = torch.empty(n_users, W, dtype=torch.int32, device=DEV)
    prefix = torch.empty(n_users, W + 1, dtype=torch.int32, device=DEV)
    status = torch.full((1,), 10, dtype=torch.int64, device=DEV)              # never cleared by the call
    for k in (1, 2):
        _lib.check(_lib.load().dfm_seen_sets_build(du.data_ptr(), di.data_ptr(), len(u), n_users, n_items,
                                                   bitmap.data_ptr(), prefix.data_ptr(), status.data_ptr(),
                                                   _lib.stream_handle()))
        assert int(status.item()) == 10 + 4 * k
        want = SeenSets.from_interactions(u[good], i[good], n_users, n_items)    # a bad row contributes nothing
        assert np.array_equal(_np(bitmap).view(np.uint32), want.bitmap)
        assert np.array_equal(_np(prefix).view(np.uint32), want.prefix)
    with pytest.raises(ValueError, match="outside the tables"):
        device_seen_sets(du, di, n_users, n_items)
    with pytest.raises(ValueError, match="outside the tables"):
        _log(u, i, np.arange(8), np.ones(8), n_users, n_items).seen_sets()
    with pytest.raises(ValueError, match="outside the tables"):
        SeenSets.from_interactions(u, i, n_users, n_items)


def test_device_seen_sets_is_a_seen_sets_the_sampler_takes_unchanged():
    """upload() hands out the tensors it was built into; bitmap / prefix / unseen are the host builder's arrays; a
    NegativeSampler over it draws exactly what one over the host SeenSets draws."""
    from deepfm_amd.data import DeviceColumns, DeviceSeenSets, NegativeSampler, SeenSets
    from tests.test_gpu_trainer import _epoch_set
    s = _epoch_set(300, seed=5, n_users=40, n_items=60)
    u = np.concatenate([np.full(len(r), k, np.int64) for k, r in enumerate(s.seen_rows)])
    i = np.concatenate([np.array(sorted(r), np.int64) for r in s.seen_rows])
    log = _log(u, i, np.arange(len(u)), np.ones(len(u)), 40, 60)
    seen = log.seen_sets()
    assert isinstance(seen, DeviceSeenSets) and isinstance(seen, SeenSets) and seen.words == 2
    up = seen.upload(DEV)
    assert up[0] is seen.bitmap_device and up[1] is seen.prefix_device and seen.upload("cuda:0")[0] is up[0]
    assert seen.upload("cpu")[0].device.type == "cpu"
    assert np.array_equal(seen.unseen, s.seen.unseen) and seen.unseen.dtype == np.uint32
    assert np.array_equal(seen.bitmap, s.seen.bitmap) and np.array_equal(seen.prefix, s.seen.prefix)
    assert np.array_equal(seen.unseen, s.seen.unseen)                          # now a view of the downloaded prefix
    dcols = DeviceColumns(s.cols, DEV)
    for short in ("refuse", "truncate"):
        on_host = NegativeSampler(dcols, s.seen, s.user_of, s.table, 4, derived=s.derived, seed=9, short_users=short)
        on_dev = NegativeSampler(dcols, seen, s.user_of, s.table, 4, derived=s.derived, seed=9, short_users=short)
        assert on_dev.bitmap is seen.bitmap_device
        for epoch in (0, 3):
            assert np.array_equal(on_dev.negatives_host(epoch), on_host.negatives_host(epoch))
    with pytest.raises(ValueError, match="user_of names a user outside"):       # the host checks still run
        NegativeSampler(dcols, seen, s.user_of + 40, s.table, 4, derived=s.derived)


# ---------------------------------------------------------------------------------------------------- counts
def _lds_limit():
    from deepfm_amd import _lib
    return _lib.COUNTS_LDS_ENTITIES


@pytest.mark.parametrize("n_entities", [1, 7, "lds", "lds+1"])
def test_counts_equal_bincount(n_entities):
    """Both routes (a workgroup's histogram in LDS up to COUNTS_LDS_ENTITIES entities, global atomics above), several
    workgroups in each (9000 rows: three LDS workgroups, 36 global ones); all rows, an index subset with repeats, an
    empty subset; with and without labels."""
    from deepfm_amd.data.interactions import entity_counts
    n_entities = {"lds": _lds_limit(), "lds+1": _lds_limit() + 1}.get(n_entities, n_entities)
    rng = np.random.default_rng(n_entities)
    n_log = 9000
    e = np.minimum(rng.zipf(1.3, n_log) - 1, n_entities - 1).astype(np.int64)
    e[:3] = n_entities - 1                                                      # the last counter is used
    labels = (rng.random(n_log) < 0.4).astype(np.float32)
    subset = np.concatenate([rng.integers(0, n_log, 5000), np.full(7, n_log - 1)]).astype(np.int64)
    de, dl = _dev(e), _dev(labels)
    for rows in (None, subset, subset[:1], np.zeros(0, np.int64)):
        for lab in (None, labels):
            drows = None if rows is None else _dev(rows)
            got, = _twice(lambda: (entity_counts(de, n_entities, None if lab is None else dl, drows),))
            assert got.dtype == np.int64 and np.array_equal(got, R.entity_counts(e, n_entities, lab, rows))
    assert R.entity_counts(e, n_entities, labels, subset).sum() == (labels[subset] == 1).sum()


@pytest.mark.parametrize("n_entities", [7, "lds+1"])
def test_counts_refuse_rows_and_indices_outside_their_tables(n_entities):
    from deepfm_amd import _lib
    from deepfm_amd.data.interactions import entity_counts
    n_entities = {"lds+1": _lds_limit() + 1}.get(n_entities, n_entities)
    e = np.array([0, 1, n_entities, 2, -1, 1], np.int64)
    index = np.array([0, 5, 6, -1, 2, 1, 4], np.int64)            # two bad indices, then two rows with a bad entity
    de, di = _dev(e), _dev(index)
    counts = torch.empty(n_entities, dtype=torch.int64, device=DEV)
    status = torch.tensor([100, 200], dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().dfm_entity_counts(de.data_ptr(), 0, di.data_ptr(), len(index), len(e), n_entities,
                                             counts.data_ptr(), status.data_ptr(), _lib.stream_handle()))
    assert status.tolist() == [102, 202]
    assert np.array_equal(_np(counts), np.bincount([0, 1, 1], minlength=n_entities))
    with pytest.raises(ValueError, match="entries of rows are outside the log's 6 rows"):
        entity_counts(de, n_entities, rows=di)
    with pytest.raises(ValueError, match="outside the tables"):
        entity_counts(de, n_entities)
    log = _log([0, 1, 2], [0, 9, 1], [1, 2, 3], [1, 1, 0], 3, 9)
    with pytest.raises(ValueError, match="outside the tables"):
        log.counts("item")
    assert _np(log.counts("user")).tolist() == [1, 1, 0] and _np(log.counts("user", positives_only=False)).tolist() == [1, 1, 1]
    with pytest.raises(ValueError, match="expected 'user' or 'item'"):
        log.counts("movie")


# ---------------------------------------------------------------------------------------------------- temporal split
def _split_equal(log, user, ts, labels, v, t):
    want = R.temporal_split(user, ts, labels, v, t)
    got = _twice(lambda: tuple(log.temporal_split(v, t)))
    for g, w, name in zip(got, want, ("train", "val", "test")):
        assert g.dtype == np.int64 and np.array_equal(g, w), (name, v, t, len(user))
    assert log.temporal_split(v, t).cutoffs == want[3]
    return got


def _random_log(n, n_users, n_items, rng, n_times=None, label_p=0.6):
    user = rng.integers(0, n_users, n)
    item = rng.integers(0, n_items, n)
    ts = rng.integers(0, n_times or max(n // 3, 2), n) + 874724710
    return user, item, ts, (rng.random(n) < label_p).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 10, 11, 101, 300])
def test_temporal_split_equals_the_restatement(n):
    rng = np.random.default_rng(n)
    for n_users in (1, 4, 37):
        user, item, ts, labels = _random_log(n, n_users, 9, rng)
        log = _log(user, item, ts, labels, n_users, 9)
        for v, t in RATIOS:
            train, val, test = _split_equal(log, user, ts, labels, v, t)
            assert len(train) >= 1 and len(np.unique(user[val])) == len(val) and (labels[val] == 1).all()
            if v == 0:
                assert len(val) == 0


def test_temporal_split_of_the_fixture_equals_the_reference(G):
    log = _log(G["user_rows"], G["item_rows"], G["timestamps"], G["labels"], int(G["n_users"]), int(G["n_items"]))
    for k in range(4):
        v, t = float(G[f"temporal/{k}/val_ratio"]), float(G[f"temporal/{k}/test_ratio"])
        train, val, test = _split_equal(log, G["user_rows"], G["timestamps"], G["labels"], v, t)
        assert np.array_equal(np.sort(train), np.sort(G[f"temporal/{k}/train"]))     # pandas' tie order is its own
        assert np.array_equal(val, G[f"temporal/{k}/val"]) and np.array_equal(test, G[f"temporal/{k}/test"])


def test_temporal_split_edge_cases():
    # all timestamps equal: both cutoffs are that timestamp, everything is train
    n = 10
    log = _log(np.arange(n) % 3, np.arange(n) % 4, np.full(n, 77), np.ones(n), 3, 4)
    train, val, test = _split_equal(log, np.arange(n) % 3, np.full(n, 77), np.ones(n, np.float32), 0.1, 0.1)
    assert train.tolist() == list(range(n)) and len(val) == 0 and len(test) == 0
    # ten rows at timestamps 0..9, (0.2, 0.2): cutoffs 5.4 and 7.2, so train = 0..5, val window = {6, 7}, test = {8, 9}
    ts = np.arange(10)
    #        row:  0  1  2  3  4  5 | 6  7 | 8  9
    user = np.array([0, 0, 1, 1, 2, 0, 3, 1, 0, 0])     # user 3 is in the val window only: absent from train, dropped
    labels = np.array([1, 0, 1, 1, 0, 1, 1, 0, 1, 1], np.float32)   # user 1's window row is a negative: no val row
    log = _log(user, np.zeros(10), ts, labels, 5, 4)
    train, val, test = _split_equal(log, user, ts, labels, 0.2, 0.2)
    assert log.temporal_split(0.2, 0.2).cutoffs == (5.4, 7.2)
    assert train.tolist() == [0, 1, 2, 3, 4, 5] and val.tolist() == [] and test.tolist() == [8]   # two positives: the first
    # two positives of one user in one window at EQUAL timestamps: the tie goes to the smaller log position
    ts2 = np.array([0, 1, 2, 3, 4, 5, 6, 7, 9, 9])
    for flip in (False, True):
        order = np.arange(10)
        if flip:
            order[[8, 9]] = [9, 8]
        train, val, test = _split_equal(_log(user[order], np.zeros(10), ts2[order], labels[order], 5, 4), user[order],
                                        ts2[order], labels[order], 0.2, 0.2)
        assert test.tolist() == [8]
    # a window without positives, and a user row outside the table
    train, val, test = _split_equal(_log(user, np.zeros(10), ts, np.zeros(10), 5, 4), user, ts, np.zeros(10, np.float32),
                                    0.2, 0.2)
    assert len(train) == 6 and len(val) == 0 and len(test) == 0
    with pytest.raises(ValueError, match="outside the tables"):
        _log(user, np.zeros(10), ts, labels, 3, 4).temporal_split(0.2, 0.2)
    with pytest.raises(ValueError, match="empty log"):
        _log([], [], [], [], 3, 4).temporal_split(0.1, 0.1)


def test_temporal_marks_are_what_the_header_says():
    """The kernel's own outputs: in_train, first_val, first_test per user (n = none), status never cleared."""
    from deepfm_amd import _lib
    user = np.array([0, 0, 1, 1, 2, 0, 3, 1, 0, 0, 9, 2], np.int64)         # position 10 names user 9 of 5
    labels = np.array([1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1], np.float32)
    order = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12], np.int64)      # position 11 names row 12 of 12
    n, n_users = 12, 5
    du, dl, do = _dev(user), _dev(labels), _dev(order)
    in_train = torch.empty(n_users, dtype=torch.uint8, device=DEV)
    first = torch.empty(2, n_users, dtype=torch.int64, device=DEV)
    status = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    for k in (1, 2):
        _lib.check(_lib.load().dfm_temporal_split_mark(du.data_ptr(), dl.data_ptr(), do.data_ptr(), n, n_users, 6, 8,
                                                       in_train.data_ptr(), first[0].data_ptr(), first[1].data_ptr(),
                                                       status.data_ptr(), _lib.stream_handle()))
        assert int(status.item()) == 5 + 2 * k
        assert _np(in_train).tolist() == [1, 1, 1, 0, 0]
        assert _np(first).tolist() == [[n, 7, n, n, n], [8, n, n, n, n]]


@pytest.mark.parametrize("seed", [0, 1])
def test_splits_of_a_permuted_log_are_the_same_rows(seed):
    """Tie-free timestamps: the log's row order plays no part, so the split of a permuted log names the same rows,
    in the same order, through the permutation."""
    rng = np.random.default_rng(seed)
    n, n_users = 300, 23
    user, item = rng.integers(0, n_users, n), rng.integers(0, 9, n)
    ts = rng.permutation(5 * n)[:n] + 1000
    labels = (rng.random(n) < 0.5).astype(np.float32)
    perm = rng.permutation(n)
    a, b = _log(user, item, ts, labels, n_users, 9), _log(user[perm], item[perm], ts[perm], labels[perm], n_users, 9)
    for split in (lambda log: log.temporal_split(0.1, 0.1), lambda log: log.leave_one_out_split(3)):
        for x, y in zip(_twice(lambda: tuple(split(a))), _twice(lambda: tuple(split(b)))):
            assert np.array_equal(x, perm[y])


# ---------------------------------------------------------------------------------------------------- leave one out
def _loo_equal(user, ts, n_users, m):
    log = _log(user, np.zeros(len(user)), ts, np.zeros(len(user)), n_users, 4)
    want = R.leave_one_out_split(user, ts, m)
    got = _twice(lambda: tuple(log.leave_one_out_split(m)))
    for g, w, name in zip(got, want, ("train", "val", "test")):
        assert g.dtype == np.int64 and np.array_equal(g, w), (name, m)
    return got


@pytest.mark.parametrize("m", [2, 3])
def test_leave_one_out_split_equals_the_restatement(m, G):
    # users with m + 1, m, m - 1 and 1 rows and one without any; equal timestamps inside users 0 and 1
    sizes = [m + 1, m, m - 1, 1, 0, 6]
    user = np.repeat(np.arange(len(sizes)), sizes)
    rng = np.random.default_rng(m)
    ts = rng.integers(0, 50, len(user))
    ts[:2] = 7                                                    # user 0: its first two rows tie
    ts[m + 1:2 * m + 1] = 9                                       # user 1: all of its rows tie
    perm = rng.permutation(len(user))
    train, val, test = _loo_equal(user[perm], ts[perm], len(sizes), m)
    eligible = [u for u, s in enumerate(sizes) if s >= m]
    assert user[perm][val].tolist() == eligible and user[perm][test].tolist() == eligible
    assert len(train) == len(user) - 2 * len(eligible)
    # user 1's rows all tie: the last two log positions among them go to val and test
    rows1 = np.flatnonzero(user[perm] == 1)
    assert val[1] == rows1[-2] and test[1] == rows1[-1]
    # a single user, below and at the threshold; several workgroups
    for n in (m - 1, m, 700):
        train, val, test = _loo_equal(np.zeros(n, np.int64), rng.integers(0, 9, n), 1, m)
        assert (len(val), len(test)) == ((1, 1) if n >= m else (0, 0))
    for n_users in (4, 37):
        u, _, t, _ = _random_log(300, n_users, 4, rng, n_times=40)
        _loo_equal(u, t, n_users, m)
    # the fixture: the reference's own rows
    parts = _loo_equal(G["user_rows"], G["timestamps"], int(G["n_users"]), m)
    for got, name in zip(parts, ("train", "val", "test")):
        assert np.array_equal(got, G[f"loo/{m}/{name}"])


def test_leave_one_out_refusals_and_status():
    from deepfm_amd import _lib
    log = _log([0, 1, 5, 1], [0, 0, 0, 0], [1, 2, 3, 4], [0, 0, 0, 0], 3, 4)
    with pytest.raises(ValueError, match="at least 2"):
        log.leave_one_out_split(1)
    with pytest.raises(ValueError, match="outside the tables"):
        log.leave_one_out_split(2)
    assert all(len(p) == 0 for p in _log([], [], [], [], 3, 4).leave_one_out_split(2))
    # the kernel alone: position 2 names user 5 of 3 (role 0, counted, and it ends user 1's run on both sides)
    user, order = _dev(np.array([1, 1, 5, 1, 1, 1], np.int64)), _dev(np.arange(6, dtype=np.int64))
    counts = _dev(np.array([0, 5, 0], np.int64))
    roles = torch.full((6,), 9, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().dfm_loo_split_mark(user.data_ptr(), order.data_ptr(), counts.data_ptr(), 6, 3, 2,
                                              roles.data_ptr(), status.data_ptr(), _lib.stream_handle()))
    assert _np(roles).tolist() == [1, 2, 0, 0, 1, 2] and int(status.item()) == 4
    assert _lib.load().dfm_loo_split_mark(user.data_ptr(), order.data_ptr(), counts.data_ptr(), 6, 3, 1,
                                          roles.data_ptr(), status.data_ptr(), _lib.stream_handle()) != 0


# ---------------------------------------------------------------------------------------------------- construction
def test_labels_are_checked_on_the_device_and_the_first_offender_is_named():
    from deepfm_amd.data import DeviceInteractionLog
    u, i, ts = np.zeros(6, np.int64), np.zeros(6, np.int64), np.arange(6, dtype=np.int64)
    for bad in (0.5, 2.0, -1.0, float("nan")):
        labels = np.array([0, 1, 1, bad, 0, bad], np.float32)
        with pytest.raises(ValueError, match=r"labels\[3\] = .*: labels are 0 or 1"):
            _log(u, i, ts, labels, 1, 1)
    t2 = ts.copy(); t2[4] = -2**53
    with pytest.raises(ValueError, match=r"timestamps\[4\] = -9007199254740992"):       # a column that is on the device
        DeviceInteractionLog(_dev(u), _dev(i), _dev(t2), _dev(np.ones(6, np.float32)), 1, 1, DEV)
    log = DeviceInteractionLog.from_ratings(_dev(u), i, ts, np.array([1, 2, 3, 4, 5, 4.5]), 4.0, 1, 1, DEV)
    assert _np(log.labels).tolist() == [0, 0, 0, 1, 1, 1] and log.labels.dtype == torch.float32 and len(log) == 6
    ratings = _dev(np.array([5, 3, 4, 1, 2, 4], np.int64))
    assert _np(DeviceInteractionLog.from_ratings(u, i, ts, ratings, 4.0, 1, 1, DEV).labels).tolist() == [1, 0, 1, 0, 0, 1]


def test_counts_and_features_of_the_fixture_equal_the_reference(G):
    """log -> split -> counts on the device, then the two host-side feature functions: the reference's per-entity
    counts, its two count-feature columns bit for bit, and item_weights of its counts."""
    from deepfm_amd.data import count_feature_table, item_weights, popularity_weights
    n_users, n_items = int(G["n_users"]), int(G["n_items"])
    log = _log(G["user_rows"], G["item_rows"], G["timestamps"], G["labels"], n_users, n_items)
    seen = log.seen_sets()
    assert np.array_equal(R.pairs_of_bitmap(seen.bitmap, n_items), G["user_items"])
    for prefix, split in (("temporal/0", log.temporal_split(0.1, 0.1)), ("loo/3", log.leave_one_out_split(3))):
        for by, rows in (("user", log.user_rows), ("item", log.item_rows)):
            counts = log.counts(by, split.train)
            assert counts.is_cuda and np.array_equal(_np(counts), G[f"{prefix}/{by}_counts"])
            column = count_feature_table(counts, device=DEV)[rows]
            assert np.array_equal(_np(column).view(np.uint32), G[f"{prefix}/{by}_rating_count"].view(np.uint32))
        assert np.array_equal(popularity_weights(log.counts("item", split.train), 0.75),
                              item_weights(G[f"{prefix}/item_counts"], 0.75))
        assert split.user_of("val").dtype == np.int32
        assert np.array_equal(split.user_of("val"), G["user_rows"][_np(split.val)])
        with pytest.raises(ValueError, match="expected 'train', 'val' or 'test'"):
            split.user_of("valid")


# ---------------------------------------------------------------------------------------------------- end to end
def test_log_to_trainer_in_one_chain(tmp_path):
    """A synthetic log -> temporal split -> DeviceFeatureEncoder.fit(train) / transform -> seen-sets, counts, weights
    -> NegativeSampler (K = 4), WeightedNegatives (truncating) -> loaders -> one Trainer epoch of a small DeepFM.
    The loaders have the reference's row counts: P * 5 for train, Q + sum(min(C, unseen)) for an evaluation part."""
    import deepfm_amd.training as T
    from deepfm_amd.data import (DeviceEpochLoader, DeviceFeatureEncoder, ItemTable, NegativeSampler, WeightedNegatives,
                                 count_feature_table, popularity_weights)
    from deepfm_amd.data.synthetic import movielens_fields, schema_from_fields
    from tests.test_gpu_trainer import _trainer_config, _trainer_model
    rng = np.random.default_rng(3)
    n_users, n_items, K, C = 80, 60, 4, 30
    # four heavy users rate 200 times out of 52 items (8 or a few more stay unseen: short of C, not of K); the others
    # share 2200 ratings out of 30 items each
    sizes = np.concatenate([np.full(4, 200), rng.multinomial(2200 - 76 * 4, np.ones(76) / 76) + 4])
    user = np.repeat(np.arange(n_users), sizes)
    item = np.concatenate([rng.permutation(n_items)[:52 if u < 4 else 30][rng.integers(0, 52 if u < 4 else 30, s)]
                           for u, s in enumerate(sizes)])
    n = len(user)
    perm = rng.permutation(n)
    user, item = user[perm], item[perm]
    ts = rng.integers(0, 10**6, n) + 874724710
    ratings = rng.integers(1, 6, n)
    from deepfm_amd.data import DeviceInteractionLog
    log = DeviceInteractionLog.from_ratings(user, item, ts, ratings, 3.0, n_users, n_items, DEV)
    split = log.temporal_split(0.1, 0.1)
    seen = log.seen_sets()
    user_counts, item_counts = log.counts("user", split.train), log.counts("item", split.train)
    weights = popularity_weights(item_counts, 0.75)
    user_table, item_table = count_feature_table(user_counts, DEV), count_feature_table(item_counts, DEV)

    # raw columns of the MovieLens field list: per-user and per-item attributes as integer keys, gathered on the device
    def keys(hi, size):
        return _dev(rng.integers(0, hi, size).astype(np.int64) * 7 + 3)
    of_user = {"gender": keys(2, n_users), "age": keys(7, n_users), "occupation": keys(21, n_users),
               "zip_prefix": keys(300, n_users)}
    of_item = {"release_year_bucket": keys(12, n_items), "num_genres": keys(6, n_items)}
    genres, genre_len = keys(18, (n_items, 6)), _dev(rng.integers(1, 7, n_items).astype(np.int32))
    movie_age, cyc = keys(7, n), {c: _dev(rng.uniform(-1, 1, n).astype(np.float32))
                                  for c in ("dow_sin", "dow_cos", "hour_sin", "hour_cos")}
    user_key, item_key = 1000 + 3 * log.user_rows, 5 + 7 * log.item_rows

    def raw(idx):
        u, i = log.user_rows[idx], log.item_rows[idx]
        out = {"user_id": user_key[idx], "movie_id": item_key[idx], "movie_age_at_rating": movie_age[idx],
               "genres": (genres[i], genre_len[i]), "user_rating_count": user_table[u], "item_rating_count": item_table[i]}
        out.update({k: v[u] for k, v in of_user.items()})
        out.update({k: v[i] for k, v in of_item.items()})
        out.update({k: v[idx] for k, v in cyc.items()})
        return out

    template = schema_from_fields(movielens_fields(n_users, n_items))
    enc = DeviceFeatureEncoder(template, device=DEV).fit(raw(split.train))
    schema = enc.schema
    every_item = torch.arange(n_items, device=DEV)
    e = enc.encoders
    items = ItemTable(schema, {
        "movie_id": _np(e["movie_id"].transform(5 + 7 * every_item)),
        "genres": _np(e["genres"].transform(genres, genre_len)),
        "release_year_bucket": _np(e["release_year_bucket"].transform(of_item["release_year_bucket"])),
        "num_genres": _np(e["num_genres"].transform(of_item["num_genres"])),
        "item_rating_count": _np(e["item_rating_count"].transform(item_table))})
    cfg = _trainer_config(tmp_path, num_epochs=1)
    loaders = {}
    for part in ("train", "val", "test"):
        idx = getattr(split, part)
        dcols = enc.transform(raw(idx), log.labels[idx])
        if part == "train":
            src = NegativeSampler(dcols, seen, split.user_of(part), items, K, seed=cfg.seed)
        else:
            src = WeightedNegatives(dcols, seen, split.user_of(part), items, weights, C, seed=cfg.seed,
                                    short_users="truncate")
        loaders[part] = DeviceEpochLoader(dcols, cfg.training.batch_size, shuffle=part == "train", seed=cfg.seed,
                                          negatives=src)
    # the reference's row counts, from the host restatement of the split and the host seen-sets
    want_train, want_val, want_test, _ = R.temporal_split(user, ts, (ratings >= 3.0).astype(np.float32), 0.1, 0.1)
    unseen = n_items - np.array([len(set(item[user == u].tolist())) for u in range(n_users)])
    assert np.array_equal(seen.unseen, unseen)
    assert loaders["train"].rows == len(want_train) * (1 + K) and len(want_train) > 2000
    ragged = False
    for part, want in (("val", want_val), ("test", want_test)):
        assert np.array_equal(_np(getattr(split, part)), want) and len(want) >= 10
        assert loaders[part].rows == len(want) + np.minimum(C, unseen[user[want]]).sum()
        ragged |= bool((unseen[user[want]] < C).any())
    assert ragged and (unseen >= K).all()
    trainer = T.Trainer(_trainer_model(schema, cfg), schema, cfg, loaders["train"], loaders["val"], loaders["test"])
    metrics = trainer.train()
    assert metrics and all(np.isfinite(v) for v in metrics.values()) and {"auc", "logloss"} <= set(metrics)
