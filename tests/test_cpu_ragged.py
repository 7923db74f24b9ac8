"""Host-side tests of the ragged candidate lists (``short_users="truncate"`` of ``NegativeSampler`` and
``WeightedNegatives``; ``data/device_epoch.py``, ``data/candidates.py``) and of the numpy restatement the GPU tests
compare against (``tests/ragged_reference.py``): the reference's ``min(num_neg, unseen)`` (``movielens.py:575-580``)
as counts and offsets, the draws of a query that is not short unchanged, a short user's uniform draw a permutation of
its unseen rows, and the virtual-row map with empty queries."""
import numpy as np
import pytest

from tests import candidates_reference as CR
from tests import ragged_reference as RR
from tests import sampler_reference as R
from tests.test_cpu_device_epoch import _dataset

N_USERS, N_ITEMS, K = 5, 40, 4


def _hand_written(K=K):
    """Users with 0, 1, K - 1, K and K + 1 unseen rows of 40, and a query list that names each at least once."""
    left = [set(), {33}, {0, 31, 39}, {2, 32, 35, 38}, {1, 30, 31, 32, 39}]
    assert [len(s) for s in left] == [0, 1, K - 1, K, K + 1]
    seen = [set(range(N_ITEMS)) - s for s in left]
    user_of = np.array([3, 0, 2, 4, 1, 0, 2, 3, 4, 1, 0], np.int32)
    return left, seen, user_of


def _seen_sets(seen):
    from deepfm_amd.data import SeenSets
    u = np.concatenate([np.full(len(s), i, np.int64) for i, s in enumerate(seen)])
    it = np.concatenate([np.array(sorted(s), dtype=np.int64) for s in seen])
    return SeenSets.from_interactions(u, it, len(seen), N_ITEMS)


def _source(cls, seen=None, user_of=None, **kw):
    import torch
    from deepfm_amd.data import DeviceColumns, ItemTable, SeenSets
    schema, cols, data_users, items = _dataset(P=11 if user_of is not None else 30)
    if user_of is None:
        user_of = data_users
    if seen is None:
        seen = SeenSets.from_interactions(user_of, cols.ids[1] - 1, N_USERS, N_ITEMS)
    args = dict(columns=DeviceColumns(cols, torch.device("cpu")), seen=seen, user_of=user_of,
                items=ItemTable(schema, items))
    if cls.__name__ == "WeightedNegatives":
        args.update(weights=np.arange(1, N_ITEMS + 1, dtype=np.uint32), num_neg=20)
    else:
        args.update(num_neg=K)
    args.update(kw)
    return cls(**args)


def _classes():
    from deepfm_amd.data import NegativeSampler, WeightedNegatives
    return NegativeSampler, WeightedNegatives


# ----------------------------------------------------------------------------- the option
@pytest.mark.parametrize("which", [0, 1])
def test_short_users_takes_refuse_or_truncate_only(which):
    cls = _classes()[which]
    for bad in ("bogus", "", None, "Truncate"):
        with pytest.raises(ValueError, match="short_users = .*: expected one of"):
            _source(cls, short_users=bad)
    for ok in ("refuse", "truncate"):                      # nobody is short in the plain data set: both build
        s = _source(cls, short_users=ok)
        assert s.counts is None and s.offsets is None and s.total_candidates == 30 * s.num_neg
        assert s.neg_items.shape == (30, s.num_neg)


@pytest.mark.parametrize("which", [0, 1])
def test_the_default_still_refuses_with_its_message(which):
    cls = _classes()[which]
    _, seen, user_of = _hand_written()
    num_neg = K if which == 0 else 20
    with pytest.raises(ValueError, match=rf"user \d has \d+ unseen items, fewer than num_neg = {num_neg} \("):
        _source(cls, seen=_seen_sets(seen), user_of=user_of)
    with pytest.raises(ValueError, match=rf"user 0 has 0 unseen items, fewer than num_neg = {num_neg} \("):
        _source(cls, seen=_seen_sets(seen), user_of=user_of, short_users="refuse")


# ----------------------------------------------------------------------------- counts and offsets
def test_counts_and_offsets_of_a_hand_written_seen_set():
    from deepfm_amd.data import NegativeSampler, WeightedNegatives
    _, seen, user_of = _hand_written()
    want_counts = np.array([4, 0, 3, 4, 1, 0, 3, 4, 4, 1, 0], np.int32)           # min(K, [0, 1, 3, 4, 5][user])
    want_offsets = np.array([0, 4, 4, 7, 11, 12, 12, 15, 19, 23, 24, 24], np.int64)
    counts, offsets = RR.counts_offsets(seen, user_of, K, N_ITEMS)
    assert counts.dtype == np.int32 and offsets.dtype == np.int64
    assert np.array_equal(counts, want_counts) and np.array_equal(offsets, want_offsets)
    s = _source(NegativeSampler, seen=_seen_sets(seen), user_of=user_of, short_users="truncate")
    assert s.counts.dtype.is_floating_point is False and str(s.counts.dtype) == "torch.int32"
    assert str(s.offsets.dtype) == "torch.int64"
    assert np.array_equal(s.counts.numpy(), want_counts) and np.array_equal(s.offsets.numpy(), want_offsets)
    assert np.array_equal(s.counts_host, want_counts) and np.array_equal(s.offsets_host, want_offsets)
    assert s.total_candidates == 24 and s.neg_items.shape == (24,) and str(s.neg_items.dtype) == "torch.int32"
    assert s.num_neg == K
    w = _source(WeightedNegatives, seen=_seen_sets(seen), user_of=user_of, short_users="truncate")
    assert np.array_equal(w.counts.numpy(), np.array([0, 1, 3, 4, 5])[user_of])   # all short of 20
    assert w.total_candidates == int(w.offsets.numpy()[-1]) == w.neg_items.numel() == 26
    # out of range in the restatement only (the classes refuse such a user_of): a full list of -1 entries
    c, o = RR.counts_offsets(seen, [0, 7, -1, 4], K, N_ITEMS)
    assert c.tolist() == [0, 4, 4, 4] and o.tolist() == [0, 0, 4, 8, 12]


def test_check_ragged_names_the_entry():
    from deepfm_amd.data.device_epoch import check_ragged
    assert check_ragged([2, 0, 3], [0, 2, 2, 5], 3, 3) == 5
    with pytest.raises(ValueError, match=r"counts\[2\] = 4 outside \[0, num_neg = 3\]"):
        check_ragged([2, 0, 4], [0, 2, 2, 6], 3, 3)
    with pytest.raises(ValueError, match=r"counts\[0\] = -1 outside"):
        check_ragged([-1, 0, 3], [0, -1, -1, 2], 3, 3)
    with pytest.raises(ValueError, match=r"offsets\[2\] = 3 is not the exclusive scan of counts \(2\)"):
        check_ragged([2, 0, 3], [0, 2, 3, 5], 3, 3)
    with pytest.raises(ValueError, match=r"offsets\[3\] = 6 is not the exclusive scan"):
        check_ragged([2, 0, 3], [0, 2, 2, 6], 3, 3)
    with pytest.raises(ValueError, match="needs counts"):
        check_ragged([2, 0], [0, 2, 2, 5], 3, 3)


# ----------------------------------------------------------------------------- the restated draws
@pytest.mark.parametrize("epoch", [0, 3])
def test_restated_ragged_draws_equal_the_rectangular_ones_where_nobody_is_short(epoch):
    left, seen, user_of = _hand_written()
    unseen = R.unseen_lists(seen, N_ITEMS)
    counts, offsets = RR.counts_offsets(seen, user_of, K, N_ITEMS)
    flat = RR.sample_negatives_ragged(unseen, user_of, counts, 5, epoch)
    assert flat.shape == (24,) and flat.dtype == np.int32
    # the rectangular restatement refuses a short user: point the short queries at a user who is not, compare the rest
    full = np.flatnonzero(counts == K)
    rect = R.sample_negatives(unseen, np.where(counts == K, user_of, 4), K, 5, epoch)
    for q in full:
        assert np.array_equal(flat[offsets[q]:offsets[q + 1]], rect[q]), f"query {q}"
    assert full.tolist() == [0, 3, 7, 8]
    # a short user's draw: a permutation of exactly its unseen rows
    for q in np.flatnonzero(counts < K):
        got = flat[offsets[q]:offsets[q + 1]].tolist()
        assert sorted(got) == sorted(left[user_of[q]]), f"query {q}"
    # the weighted draw: per query the first counts[q] draws of the rectangular list, none for an empty user
    weights = np.random.default_rng(1).integers(1, (1 << 24) + 1, N_ITEMS).astype(np.uint32)
    counts, offsets = RR.counts_offsets(seen, user_of, 3, N_ITEMS)
    assert counts.tolist() == [3, 0, 3, 3, 1, 0, 3, 3, 3, 1, 0]
    flat = RR.sample_weighted_ragged(unseen, user_of, weights, counts, 7, epoch)
    rect = CR.sample_weighted(unseen, user_of, weights, 3, 7, epoch)
    for q in range(user_of.size):
        assert np.array_equal(flat[offsets[q]:offsets[q + 1]], rect[q, :counts[q]]), f"query {q}"
        assert not set(flat[offsets[q]:offsets[q + 1]].tolist()) - left[user_of[q]]


def test_restated_uniform_draw_of_a_short_user_uses_every_row_once():
    n_items = 70
    for U in (1, 2, 7, 15):
        rows = np.sort(np.random.default_rng(U).choice(n_items, U, replace=False))
        seen = [set(range(n_items)) - set(rows.tolist())]
        unseen = R.unseen_lists(seen, n_items)
        user_of = np.zeros(50, np.int64)
        counts, offsets = RR.counts_offsets(seen, user_of, 16, n_items)
        assert (counts == U).all()
        flat = RR.sample_negatives_ragged(unseen, user_of, counts, 2, 1).reshape(50, U)
        assert all(sorted(r.tolist()) == rows.tolist() for r in flat)
        assert U == 1 or len({tuple(r.tolist()) for r in flat}) > 1


# ----------------------------------------------------------------------------- the virtual-row map
def test_virtual_row_map_with_empty_queries_at_the_front_and_in_the_middle():
    p, t = RR.virtual_row_map([0, 0, 3, 3, 4], 4)
    assert p.tolist() == [1, 1, 1, 3] and t.tolist() == [0, 1, 2, 0]
    p, t = RR.virtual_row_map([0, 2, 2, 2, 5, 5], 5)      # and at the end
    assert p.tolist() == [0, 0, 3, 3, 3] and t.tolist() == [0, 1, 0, 1, 2]
    p, t = RR.virtual_row_map([0, 0, 0], 2)
    assert p.size == 0 and t.size == 0


def test_restated_virtual_rows_equal_the_rectangular_assembly_when_every_count_is_k():
    """With counts = K everywhere the ragged rows are the rectangular ones: ``sampler_reference.assemble``."""
    from deepfm_amd.data.packed import RecordLayout
    schema, cols, user_of, items = _dataset()
    P, k = len(cols), 3
    rng = np.random.default_rng(0)
    neg = rng.integers(0, N_ITEMS, (P, k)).astype(np.int32)
    offsets = np.arange(P + 1, dtype=np.int64) * k
    roles = {"movie_id": R.ITEM, "genres": R.ITEM, "item_count": R.ITEM, "movie_age": R.BUCKET_DIFF}
    derived = {"movie_age": (rng.uniform(0, 30, P).astype(np.float32), rng.uniform(-5, 25, N_ITEMS).astype(np.float32),
                             np.array([1, 3, 5, 10, 15, 20], np.float32), np.arange(8, dtype=np.int64))}
    rows = RR.virtual_rows(cols, offsets, neg.reshape(-1), items, roles, derived)
    assert len(rows) == P * (1 + k)
    order = rng.permutation(P * (1 + k))
    for B, idx in ((16, order[:16]), (16, order[16:32]), (16, order[112:])):
        lay = RecordLayout.of(schema, B)
        assert np.array_equal(RR.record_of(lay, rows, idx), R.assemble(lay, cols, idx, k, neg, items, roles, derived))


# ----------------------------------------------------------------------------- the loader's host side
def test_loader_rows_follow_the_total(monkeypatch):
    from deepfm_amd.data import DeviceEpochLoader, NegativeSampler
    monkeypatch.setattr(DeviceEpochLoader, "_create_plan", lambda self: None)      # the plan needs the device
    monkeypatch.setattr("deepfm_amd._lib.require_device", lambda t, what: None)
    monkeypatch.setattr(NegativeSampler, "sample", lambda self, epoch: None)
    _, seen, user_of = _hand_written()
    s = _source(NegativeSampler, seen=_seen_sets(seen), user_of=user_of, short_users="truncate")
    loader = DeviceEpochLoader(s.columns, 8, shuffle=True, seed=1, negatives=s, depth=2)
    assert loader.rows == 11 + 24 and len(loader) == 35 // 8
    assert sorted(loader.order.tolist()) == list(range(35))
    with pytest.raises(ValueError, match=r"batch_size must be in \[1, rows of an epoch\]"):
        DeviceEpochLoader(s.columns, 36, negatives=s)


def test_library_exports_the_ragged_symbols():
    """The shape is an argument: no ``_ragged`` twin in the library, the binding or the header, and the three entry
    points take the ``dfm_candidate_list`` before their output."""
    import ctypes as C
    import os
    from deepfm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "deepfm_hip.h")).read()
    for name in ("dfm_sample_negatives_ragged", "dfm_sample_weighted_ragged", "dfm_assemble_plan_create_ragged"):
        assert name not in _lib.SIGNATURES and not hasattr(lib, name) and name not in header
    for name, arity in (("dfm_sample_negatives", 12), ("dfm_sample_weighted", 12), ("dfm_assemble_plan_create", 14)):
        argtypes = _lib.SIGNATURES[name][1]
        assert hasattr(lib, name) and len(argtypes) == arity, name
        assert argtypes.index(C.POINTER(_lib.CandidateList)) == arity - (3 if "sample" in name else 2), name
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(");")].count(",") + 1 == arity, name
    assert lib.dfm_abi_version() == _lib.ABI_VERSION


def test_list_is_none_for_a_rectangular_source_and_names_the_uploaded_arrays_of_a_ragged_one():
    from deepfm_amd import _lib
    for cls in _classes():
        assert _source(cls)._list() is None
        assert _source(cls, short_users="truncate")._list() is None        # nobody is short: rectangular
        _, seen, user_of = _hand_written()
        s = _source(cls, seen=_seen_sets(seen), user_of=user_of, short_users="truncate")
        lst = s._list()
        assert isinstance(lst, _lib.CandidateList) and s._list() is lst    # built once, kept on the source
        assert lst.d_counts == s.counts.data_ptr() and lst.d_offsets == s.offsets.data_ptr()
        assert lst.total == s.total_candidates == int(s.offsets_host[-1]) > 0
