"""GPU tests of the ragged candidate lists (``csrc/sampler.hip``: ``dfm_sample_negatives``, ``dfm_sample_weighted``
and ``dfm_assemble_plan_create`` with a ``dfm_candidate_list``; ``short_users="truncate"`` in ``data/device_epoch.py``
and ``data/candidates.py``) against the numpy restatement ``tests/ragged_reference.py``.  Item rows and copied float bits
compare bit for bit; the end-to-end comparisons are the exact ones of ``tests/test_gpu_candidates.py``.

1. the two ragged draws vs the restatement inside a buffer of sentinels, at the word edges of the bitmap;
2. a source nobody is short in: both modes give the same items and the same records, and so does the ragged plan;
   at the entry points, a NULL list and a list whose every count is K give the same draws and the same records;
3. the ragged assembly (MovieLens-shaped schema, a batch boundary inside a query, empty queries, a partial batch)
   vs ``RecordLayout.write_indexed`` over the restated virtual rows;
4. ``evaluate_loader`` for the three models and one fused training epoch over ragged sources;
5. the host-side refusals of a wrong list.
"""
import numpy as np
import pytest
import torch

from tests import ragged_reference as RR
from tests import sampler_reference as R
from tests.test_gpu_candidates import _i32, _ref_args, _seen_sets
from tests.test_gpu_device_epoch import movielens_epoch

pytestmark = pytest.mark.gpu

DEV = "cuda"
W1 = 1 << 24
USER_OF = np.array([0, 1, 2, 3, 4, 5, -1, 3, 0, 2, 6], np.int32)          # six users; -1 and 6 are out of range
SENTINEL, PAD = -7, 5


# ----------------------------------------------------------------------------- 1. the draws
def _users_with_unseen(n_items, unseen_counts, rng):
    """Per user its seen set, leaving exactly that many unseen rows: the last row, then rows around the word edge at
    31 / 32, then random ones."""
    seen = []
    for n in unseen_counts:
        n = min(n, n_items)
        first = list(dict.fromkeys(i for i in (n_items - 1, 31, 32, 0) if i < n_items))[:n]
        rest = [i for i in rng.permutation(n_items).tolist() if i not in first][:n - len(first)]
        seen.append(set(range(n_items)) - set(first) - set(rest))
        assert n_items - len(seen[-1]) == n
    return seen


def _flat_inside_sentinels(total):
    return torch.full((PAD + total + PAD,), SENTINEL, dtype=torch.int32, device=DEV)


def _check_sentinels(buf, total):
    host = buf.cpu().numpy()
    assert (host[:PAD] == SENTINEL).all() and (host[PAD + total:] == SENTINEL).all(), "a sentinel was overwritten"
    return host[PAD:PAD + total]


def _candidate_list(counts, offsets, total=None):
    """A ``CandidateList`` over device copies of the two arrays, and those copies: they must outlive the call."""
    from deepfm_amd import _lib
    keep = (_i32(counts), torch.from_numpy(offsets).to(DEV))
    return _lib.CandidateList(keep[0].data_ptr(), keep[1].data_ptr(), int(offsets[-1]) if total is None else total), keep


def _draw_uniform(seen, n_items, K, seed, epoch, counts=None, offsets=None):
    """The flat output of ``dfm_sample_negatives`` inside sentinels: of the list ``counts`` / ``offsets``, or, without
    one, of the NULL list (the (Q, K) rectangle)."""
    from deepfm_amd import _lib
    bitmap, prefix = _seen_sets(seen, n_items).upload(DEV)
    lst, keep = _candidate_list(counts, offsets) if counts is not None else (None, None)
    total = lst.total if lst is not None else len(USER_OF) * K
    buf = _flat_inside_sentinels(total)
    d_user = _i32(USER_OF)                                 # named: it must outlive the call
    _lib.check(_lib.load().dfm_sample_negatives(
        bitmap.data_ptr(), prefix.data_ptr(), d_user.data_ptr(), len(USER_OF), len(seen), n_items, K, seed, epoch,
        lst, buf.data_ptr() + 4 * PAD, _lib.stream_handle()))
    return _check_sentinels(buf, total)


@pytest.mark.parametrize("n_items", [40, 33, 64])
def test_ragged_uniform_draw_matches_restatement(n_items):
    K = 4
    left = [0, 1, 3, 4, n_items - 4, n_items // 2]                             # 36 of 40 for the fifth user
    seen = _users_with_unseen(n_items, left, np.random.default_rng(n_items))
    unseen = R.unseen_lists(seen, n_items)
    counts, offsets = RR.counts_offsets(seen, USER_OF, K, n_items)
    assert counts.tolist() == [0, 1, 3, 4, 4, 4, 4, 4, 0, 3, 4]
    got = {e: _draw_uniform(seen, n_items, K, 5, e, counts, offsets) for e in (0, 3)}
    for e, g in got.items():
        assert np.array_equal(g, RR.sample_negatives_ragged(unseen, USER_OF, counts, 5, e)), f"epoch {e}"
    assert not np.array_equal(got[0], got[3]), "two epochs gave the same draws"
    # a query that is not short: the items of the rectangular draw (the short and outside ones pointed elsewhere)
    rect = R.sample_negatives(unseen, np.where((counts == K) & (USER_OF >= 0) & (USER_OF < 6), USER_OF, 4), K, 5, 3)
    for q, u in enumerate(USER_OF):
        row = got[3][offsets[q]:offsets[q + 1]]
        if u in (-1, 6):
            assert (row == -1).all() and row.size == K
        elif counts[q] == K:
            assert np.array_equal(row, rect[q]), f"query {q}"
        else:                                              # a short user: each unseen row once
            assert sorted(row.tolist()) == unseen[u].tolist(), f"query {q}"


def _draw_weighted(seen, weights, n_items, C, seed, epoch, counts=None, offsets=None):
    """``_draw_uniform`` for ``dfm_sample_weighted``."""
    from deepfm_amd import _lib
    bitmap, _ = _seen_sets(seen, n_items).upload(DEV)
    lst, keep = _candidate_list(counts, offsets) if counts is not None else (None, None)
    total = lst.total if lst is not None else len(USER_OF) * C
    buf = _flat_inside_sentinels(total)
    d_user, d_weight = _i32(USER_OF), _i32(weights)
    _lib.check(_lib.load().dfm_sample_weighted(
        bitmap.data_ptr(), d_user.data_ptr(), d_weight.data_ptr(), len(USER_OF), len(seen), n_items, C, seed, epoch,
        lst, buf.data_ptr() + 4 * PAD, _lib.stream_handle()))
    return _check_sentinels(buf, total)


@pytest.mark.parametrize("n_items", [40, 33, 64])
def test_ragged_weighted_draw_matches_restatement(n_items):
    from tests import candidates_reference as CR
    C = 20
    rng = np.random.default_rng(100 + n_items)
    seen = _users_with_unseen(n_items, [0, 2, 19, 20, 33, n_items // 2], rng)
    unseen = R.unseen_lists(seen, n_items)
    weights = rng.integers(1, W1 + 1, n_items).astype(np.uint32)
    weights[rng.choice(n_items, 6, replace=False)] = [1, 1, 1 << 8, 1 << 16, W1, W1]
    weights[n_items - 1] = 1                               # the lightest weight on the last row of the bitmap
    counts, offsets = RR.counts_offsets(seen, USER_OF, C, n_items)
    assert counts.tolist() == [0, 2, 19, 20, 20, min(C, n_items // 2), 20, 20, 0, 19, 20]
    got = {e: _draw_weighted(seen, weights, n_items, C, 5, e, counts, offsets) for e in (0, 3)}
    for e, g in got.items():
        assert np.array_equal(g, RR.sample_weighted_ragged(unseen, USER_OF, weights, counts, 5, e)), f"epoch {e}"
    assert not np.array_equal(got[0], got[3]), "two epochs gave the same draws"
    rect = CR.sample_weighted(unseen, USER_OF, weights, C, 5, 0)             # the first counts[q] rectangular draws
    for q, u in enumerate(USER_OF):
        row = got[0][offsets[q]:offsets[q + 1]]
        assert np.array_equal(row, rect[q, :counts[q]]), f"query {q}"
        if u in (-1, 6):
            assert (row == -1).all()
        else:
            assert not set(row.tolist()) & seen[u] and (row >= 0).all() and (row < n_items).all()


def test_ragged_draws_cut_a_list_that_is_too_short_and_launch_nothing_for_an_empty_one():
    """The kernels never write past ``total_candidates``, whatever counts say: a list two entries short of its
    counts loses exactly those entries.  An empty list is no launch."""
    from deepfm_amd import _lib
    n_items, K = 40, 4
    seen = _users_with_unseen(n_items, [0, 1, 3, 4, 36, 20], np.random.default_rng(0))
    counts, offsets = RR.counts_offsets(seen, USER_OF, K, n_items)
    want = RR.sample_negatives_ragged(R.unseen_lists(seen, n_items), USER_OF, counts, 5, 0)
    total = int(offsets[-1]) - 2                            # the last query (four -1 entries) keeps two
    bitmap, prefix = _seen_sets(seen, n_items).upload(DEV)
    buf = _flat_inside_sentinels(total)
    d_user, lib = _i32(USER_OF), _lib.load()

    def draw(lst, out):
        return lib.dfm_sample_negatives(bitmap.data_ptr(), prefix.data_ptr(), d_user.data_ptr(), len(USER_OF),
                                        len(seen), n_items, K, 5, 0, lst, out, _lib.stream_handle())

    lst, keep = _candidate_list(counts, offsets, total)
    _lib.check(draw(lst, buf.data_ptr() + 4 * PAD))
    assert np.array_equal(_check_sentinels(buf, total), want[:total])
    buf = _flat_inside_sentinels(0)
    zeros = torch.zeros(len(USER_OF) + 1, dtype=torch.int64, device=DEV)
    _lib.check(draw(_lib.CandidateList(zeros.data_ptr(), zeros.data_ptr(), 0), 0))
    assert (buf.cpu().numpy() == SENTINEL).all()
    lst, keep = _candidate_list(counts, offsets, len(USER_OF) * K + 1)
    rc = draw(lst, buf.data_ptr())
    assert rc != 0 and b"total_candidates 45 outside [0, 44]" in lib.dfm_last_error()


@pytest.mark.parametrize("n_items", [40, 33, 64])
def test_a_null_list_and_a_list_of_full_counts_give_the_uniform_draw_of_the_restatement(n_items):
    """Both instantiations of the uniform kernel at the entry point: the rectangle of the NULL list and the flat list
    whose every count is K are the same items, those of ``sampler_reference``."""
    K, Q = 4, len(USER_OF)
    seen = _users_with_unseen(n_items, [K, K + 1, 8, n_items, n_items - 4, n_items // 2], np.random.default_rng(n_items))
    inside = (USER_OF >= 0) & (USER_OF < 6)
    counts, offsets = np.full(Q, K, np.int32), np.arange(Q + 1, dtype=np.int64) * K
    for epoch in (0, 3):
        want = R.sample_negatives(R.unseen_lists(seen, n_items), np.where(inside, USER_OF, 0), K, 5, epoch)
        want[~inside] = -1                                 # a user outside the tables: -1 entries
        rect = _draw_uniform(seen, n_items, K, 5, epoch)
        flat = _draw_uniform(seen, n_items, K, 5, epoch, counts, offsets)
        assert np.array_equal(rect, flat), f"epoch {epoch}: the two shapes differ"
        assert np.array_equal(rect.reshape(Q, K), want), f"epoch {epoch}"


@pytest.mark.parametrize("n_items", [40, 33, 64])
def test_a_null_list_and_a_list_of_full_counts_give_the_weighted_draw_of_the_restatement(n_items):
    """The same for the weighted kernel and ``candidates_reference``; one user has no unseen row, one has two."""
    from tests import candidates_reference as CR
    C, Q = 20, len(USER_OF)
    rng = np.random.default_rng(200 + n_items)
    seen = _users_with_unseen(n_items, [0, 2, 19, 20, 33, n_items // 2], rng)
    weights = rng.integers(1, W1 + 1, n_items).astype(np.uint32)
    weights[n_items - 1] = 1                               # the lightest weight on the last row of the bitmap
    counts, offsets = np.full(Q, C, np.int32), np.arange(Q + 1, dtype=np.int64) * C
    for epoch in (0, 3):
        want = CR.sample_weighted(R.unseen_lists(seen, n_items), USER_OF, weights, C, 5, epoch)
        rect = _draw_weighted(seen, weights, n_items, C, 5, epoch)
        flat = _draw_weighted(seen, weights, n_items, C, 5, epoch, counts, offsets)
        assert np.array_equal(rect, flat), f"epoch {epoch}: the two shapes differ"
        assert np.array_equal(rect.reshape(Q, C), want), f"epoch {epoch}"
        assert (want[[0, 6, 8, 10]] == -1).all() and (want[[1, 2, 3, 4, 5, 7, 9]] >= 0).all()


# ----------------------------------------------------------------------------- 2. equality with today
def _records(loader):
    return [rec.cpu().numpy().copy() for rec in loader]


@pytest.mark.parametrize("which", ["uniform", "weighted"])
def test_a_source_nobody_is_short_in_is_todays_in_both_modes_and_through_the_ragged_plan(which):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, NegativeSampler, WeightedNegatives
    P, B = 130, 64
    K = 4 if which == "uniform" else 17
    schema, cols, user_of, item_of, table, items, derived, seen = movielens_epoch(P, 4, seed=2)
    dcols = DeviceColumns(cols, DEV)
    w = np.random.default_rng(K).integers(1, W1 + 1, seen.n_items).astype(np.uint32)

    def source(**kw):
        if which == "uniform":
            return NegativeSampler(dcols, seen, user_of, table, K, derived=derived, seed=9, **kw)
        return WeightedNegatives(dcols, seen, user_of, table, w, K, derived=derived, seed=9, **kw)

    got = {}
    for mode in ("default", "refuse", "truncate", "ragged"):
        src = source() if mode == "default" else source(short_users="truncate" if mode == "ragged" else mode)
        assert src.counts is None and src.offsets is None and src.total_candidates == P * K
        if mode == "ragged":                               # the ragged kernels over a list every count of which is K
            src._upload(dcols, seen, src.user_of_host, table, K, counts=np.full(P, K, np.int32))
            assert src.neg_items.shape == (P * K,) and src.offsets_host[-1] == P * K
        loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=4, negatives=src, depth=3)
        loader.set_epoch(2)
        assert loader.rows == P * (1 + K) and len(loader) == P * (1 + K) // B
        got[mode] = (src.neg_items.cpu().numpy().reshape(P, K), loader.order.cpu().numpy(), _records(loader),
                     loader.rows_into_next(len(loader) * B, loader.rows - len(loader) * B).cpu().numpy().copy())
    for mode in ("refuse", "truncate", "ragged"):
        assert np.array_equal(got[mode][0], got["default"][0]), f"{mode}: neg_items"
        assert np.array_equal(got[mode][1], got["default"][1]), f"{mode}: order"
        assert len(got[mode][2]) == len(got["default"][2])
        for k, (a, b) in enumerate(zip(got[mode][2], got["default"][2])):
            assert np.array_equal(a, b), f"{mode}: record {k}"
        assert np.array_equal(got[mode][3], got["default"][3]), f"{mode}: the trailing partial batch"


def test_a_plan_of_a_null_list_and_one_of_a_list_of_full_counts_assemble_the_same_records():
    """Both instantiations of the assemble kernel at the entry point: ``dfm_assemble_plan_create`` with NULL (the
    loader's own plans) and with the list whose every count is K, one full batch and the trailing partial batch."""
    from deepfm_amd import _lib
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, NegativeSampler
    P, B, K = 130, 64, 4
    schema, cols, user_of, item_of, table, items, derived, seen = movielens_epoch(P, 4, seed=2)
    dcols = DeviceColumns(cols, DEV)
    src = NegativeSampler(dcols, seen, user_of, table, K, derived=derived, seed=9)
    loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=4, negatives=src, depth=3)
    loader.set_epoch(2)
    assert src._list() is None and loader.tail_rows == P * (1 + K) % B == 10
    lst, keep = _candidate_list(np.full(P, K, np.int32), np.arange(P + 1, dtype=np.int64) * K)
    src._list = lambda: lst                                # the same candidates, described as a list
    for lay, first, count, want in ((loader.layout, B, B, loader.record(1)),
                                    (loader.tail_layout, len(loader) * B, loader.tail_rows, loader.tail())):
        out = torch.zeros(lay.record_bytes, dtype=torch.uint8, device=DEV)
        plan = loader._plan_for(lay)
        try:
            loader._assemble(plan, first, count, out)
            torch.cuda.synchronize()
        finally:
            _lib.check(_lib.load().dfm_assemble_plan_destroy(plan))
        assert want.any() and np.array_equal(out.cpu().numpy(), want.cpu().numpy()), f"rows from {first}"


# ----------------------------------------------------------------------------- 3. the ragged assembly
Q, N_ITEMS, B, C = 12, 100, 64, 20


def _ragged_set(unseen_of, P=Q, seed=0):
    """P rows over Q users (row i is user i % Q) of the MovieLens-shaped schema of ``data/synthetic.py``; user u
    keeps ``unseen_of[u]`` unseen rows (default: about 70), every row's own item among the seen ones."""
    from deepfm_amd.data import BucketDifference, ItemTable, SeenSets
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.synthetic import movielens_fields, random_fields_batch, schema_from_fields
    rng = np.random.default_rng(seed)
    fields = movielens_fields(Q, N_ITEMS)
    schema = schema_from_fields(fields)
    items = {f["name"]: random_fields_batch([f], N_ITEMS, rng, zero_frac=0.0)[f["name"]]
             for f in fields if f["group"] == "item"}
    items["movie_id"] = np.arange(N_ITEMS, dtype=np.int64) + 1
    user_of = (np.arange(P) % Q).astype(np.int32)
    seen_rows = []
    for u in range(Q):
        n_seen = N_ITEMS - unseen_of.get(u, 70)
        seen_rows.append(set(rng.permutation(N_ITEMS)[:n_seen].tolist()))
    target = np.array([sorted(seen_rows[u])[int(rng.integers(0, len(seen_rows[u])))] for u in user_of])
    feats = random_fields_batch(fields, P, rng, zero_frac=0.0)
    feats["user_id"] = user_of.astype(np.int64) + 1
    for name, col in items.items():
        feats[name] = col[target]
    seen = SeenSets.from_interactions(np.concatenate([np.full(len(s), u, np.int64) for u, s in enumerate(seen_rows)]),
                                      np.concatenate([np.array(sorted(s), np.int64) for s in seen_rows]), Q, N_ITEMS)
    assert [int(x) for x in seen.unseen] == [unseen_of.get(u, 70) for u in range(Q)]
    ctx = rng.uniform(20.0, 30.0, P).astype(np.float32)
    item_val = rng.uniform(0.0, 35.0, N_ITEMS).astype(np.float32)             # differences of both signs
    ctx[3], item_val[::13] = np.nan, np.nan
    bd = BucketDifference(ctx, item_val, np.array([1, 2, 5, 10, 20], np.float32), np.arange(7, dtype=np.int64))
    cols = PackedColumns(schema, feats, (rng.random(P) < 0.7).astype(np.float32) if P != Q else np.ones(P, np.float32))
    counts = np.bincount(np.concatenate([np.array(sorted(s), np.int64) for s in seen_rows]), minlength=N_ITEMS)
    return fields, schema, cols, user_of, ItemTable(schema, items), items, {"movie_age_at_rating": bd}, seen, seen_rows, counts


@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("unseen_of", [{0: 0, 6: 7, 11: 19}, {0: 0, 1: 0, 6: 0, 7: 3, 11: 0}],
                         ids=["three_short", "empty_front_middle_end"])
def test_ragged_assembly_matches_write_indexed_over_the_restated_rows(unseen_of, shuffle):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, WeightedNegatives, item_weights
    fields, schema, cols, user_of, table, items, derived, seen, seen_rows, pop = _ragged_set(unseen_of)
    dcols = DeviceColumns(cols, DEV)
    w = item_weights(pop, 0.75)
    src = WeightedNegatives(dcols, seen, user_of, table, w, C, derived=derived, seed=9, short_users="truncate")
    counts, offsets = RR.counts_offsets(seen_rows, user_of, C, N_ITEMS)
    assert np.array_equal(src.counts.cpu().numpy(), counts) and np.array_equal(src.offsets.cpu().numpy(), offsets)
    total = int(offsets[-1])
    assert src.total_candidates == total == sum(min(C, unseen_of.get(u, 70)) for u in range(Q))
    loader = DeviceEpochLoader(dcols, B, shuffle=shuffle, seed=4, negatives=src, depth=3)
    loader.set_epoch(2)
    rows_total = Q + total
    assert loader.rows == rows_total and len(loader) == rows_total // B and rows_total % B
    neg = loader.negatives_host(2)
    assert neg.shape == (total,) and np.array_equal(src.neg_items.cpu().numpy(), neg)
    assert np.array_equal(neg, RR.sample_weighted_ragged(R.unseen_lists(seen_rows, N_ITEMS), user_of, w, counts, 9, 2))
    order = loader.order.cpu().numpy() if shuffle else np.arange(rows_total)
    assert sorted(order.tolist()) == list(range(rows_total))
    if not shuffle:                                        # a batch boundary inside one query's candidates
        p_of, t_of = RR.virtual_row_map(offsets, Q)
        assert p_of[B - Q] == p_of[B - Q - 1] and t_of[B - Q] > 0
    roles, ref_derived = _ref_args(src, derived)
    rows = RR.virtual_rows(cols, offsets, neg, items, roles, ref_derived)
    assert len(rows) == rows_total
    for k, rec in enumerate(loader):
        want = RR.record_of(loader.layout, rows, order[k * B:(k + 1) * B])
        assert np.array_equal(rec.cpu().numpy(), want), f"batch {k}"
    tail = rows_total - len(loader) * B                    # the trailing partial batch, over a dirty slot
    loader.ring.fill_(0xAB)
    want = RR.record_of(loader.layout, rows, order[rows_total - tail:])
    assert np.array_equal(loader.rows_into_next(rows_total - tail, tail).cpu().numpy(), want)
    # a row the order names outside the epoch is padding, as in the rectangular plan
    bad = torch.tensor([rows_total, Q, -1, rows_total - 1], dtype=torch.int64, device=DEV)
    loader.order = bad
    got = loader.rows_into_next(0, 4).cpu().numpy()
    want = RR.record_of(loader.layout, rows, np.array([Q, rows_total - 1]))
    batch, _ = loader.layout.unpack(got)
    ref, _ = loader.layout.unpack(want)
    for name in batch:
        assert not batch[name][[0, 2]].any() and np.array_equal(batch[name][[1, 3]].view(np.uint8), ref[name][:2].view(np.uint8))


# ----------------------------------------------------------------------------- 4. end to end
def _small_model(kind, fields, seed):
    from deepfm_amd.models import create_model
    from deepfm_amd.data.synthetic import schema_from_fields
    from tests.test_cpu_mixed_predict import movielens_cfg
    torch.manual_seed(seed)
    with torch.device("cuda"):
        model = create_model(kind, schema_from_fields(fields), movielens_cfg(kind, hidden_units=[32, 32]))
    model.embedding.strict_indices = True
    return model.eval()


@pytest.mark.parametrize("kind", ["deepfm", "xdeepfm", "attention_deepfm"])
def test_evaluate_loader_over_a_ragged_source_equals_evaluate_over_the_same_host_rows(kind):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, WeightedNegatives, item_weights
    from deepfm_amd.training import MixedSchemaPredictor
    unseen_of = {0: 0, 6: 7, 11: 19}                       # three short users, one with nothing unseen
    fields, schema, cols, user_of, table, items, derived, seen, seen_rows, pop = _ragged_set(unseen_of)
    pred = MixedSchemaPredictor(_small_model(kind, fields, 2), B)
    dcols = DeviceColumns(cols, DEV)
    src = WeightedNegatives(dcols, seen, user_of, table, item_weights(pop, 0.75), C, derived=derived, seed=11,
                            short_users="truncate")
    loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=5, negatives=src, depth=3)
    loader.set_epoch(1)
    n = Q + 9 * C + 7 + 19
    assert loader.rows == n and n % B                      # a trailing partial batch
    order = loader.order.cpu().numpy()
    roles, ref_derived = _ref_args(src, derived)
    rows = RR.virtual_rows(cols, src.offsets_host, loader.negatives_host(1), items, roles, ref_derived)
    host = RR.take(rows, order)
    ks = [1, 5]
    m_loader = pred.evaluate_loader(loader, ranking_ks=ks)
    s_loader, l_loader = pred.last_scores.clone(), pred.last_labels.clone()
    m_host = pred.evaluate(host, ranking_ks=ks)
    assert torch.equal(s_loader, pred.last_scores) and torch.equal(l_loader, pred.last_labels)
    assert m_loader == m_host, (m_loader, m_host)
    assert {"auc", "logloss", "HR@1", "NDCG@1", "HR@5", "NDCG@5"} == set(m_loader)
    # the query without a candidate is scored (one label per query, n scores) and left out of the ranking metrics
    scores, labels = s_loader.cpu().numpy(), l_loader.cpu().numpy()
    assert scores.shape == (n,) and int(labels.sum()) == Q
    p_of, _ = RR.virtual_row_map(src.offsets_host, Q)
    user = np.concatenate([np.arange(Q), p_of])[order]
    hits = {k: 0 for k in ks}
    for u in range(1, Q):                                  # user 0 has one class only
        mine = user == u
        rank = int(np.argsort(-scores[mine], kind="stable").tolist().index(int(np.flatnonzero(labels[mine])[0])))
        for k in ks:
            hits[k] += rank < k
    assert not (user[labels == 0] == 0).any()
    for k in ks:
        assert m_loader[f"HR@{k}"] == hits[k] / (Q - 1), f"HR@{k} over the {Q - 1} users with both classes"


def test_fused_training_epoch_over_a_truncating_sampler_equals_host_built_records():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, NegativeSampler
    from deepfm_amd.training import DenseTableAdam, FusedMixedDeepFMStep
    from tests.test_gpu_device_epoch import _model
    P, K = 60, 4
    unseen_of = {0: 0, 6: 1, 11: 3}
    fields, schema, cols, user_of, table, items, derived, seen, seen_rows, _ = _ragged_set(unseen_of, P=P, seed=1)
    dcols = DeviceColumns(cols, DEV)
    src = NegativeSampler(dcols, seen, user_of, table, K, derived=derived, seed=1, short_users="truncate")
    counts, offsets = RR.counts_offsets(seen_rows, user_of, K, N_ITEMS)
    assert np.array_equal(src.counts_host, counts) and sorted(set(counts.tolist())) == [0, 1, 3, 4]
    loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=1, negatives=src, depth=2)
    loader.set_epoch(1)
    total = 5 * (0 + 1 + 3) + 45 * K
    assert loader.rows == P + total and len(loader) == (P + total) // B == 4
    neg, order = loader.negatives_host(1), loader.order.cpu().numpy()
    assert np.array_equal(neg, RR.sample_negatives_ragged(R.unseen_lists(seen_rows, N_ITEMS), user_of, counts, 1, 1))
    roles, ref_derived = _ref_args(src, derived)
    rows = RR.virtual_rows(cols, offsets, neg, items, roles, ref_derived)
    host = [RR.record_of(loader.layout, rows, order[k * B:(k + 1) * B]) for k in range(len(loader))]
    finals, steps = [], []
    for source in ("loader", "host"):
        model = _model(schema, 3)
        opt = DenseTableAdam(model, lr=1e-2, l2=1e-3, max_grad_norm=0.5)
        step = FusedMixedDeepFMStep(model, opt, B, use_graph=True)
        step.capture()
        n = 0
        for rec in (loader if source == "loader" else (torch.from_numpy(h).cuda() for h in host)):
            step.run_from(rec)
            model.embedding.raise_on_bad_index()
            n += 1
        torch.cuda.synchronize()
        steps.append(n)
        finals.append([opt.flat_param.clone(), opt.flat_m.clone(), opt.flat_v.clone(), step.loss.clone()])
    assert steps == [len(loader), len(loader)]
    for a, b in zip(*finals):
        assert torch.equal(a, b)
    assert torch.isfinite(finals[0][3]).all()


# ----------------------------------------------------------------------------- 5. refusals
def test_a_wrong_list_is_refused_on_the_host_before_any_launch():
    from deepfm_amd import _lib
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, WeightedNegatives, item_weights
    fields, schema, cols, user_of, table, items, derived, seen, seen_rows, pop = _ragged_set({0: 0, 6: 7, 11: 19})
    dcols = DeviceColumns(cols, DEV)

    def source():
        return WeightedNegatives(dcols, seen, user_of, table, item_weights(pop, 0.75), C, derived=derived,
                                 short_users="truncate")

    src = source()
    src.counts_host = src.counts_host.copy()
    src.counts_host[3] = C + 1
    with pytest.raises(ValueError, match=rf"counts\[3\] = {C + 1} outside \[0, num_neg = {C}\]"):
        DeviceEpochLoader(dcols, B, negatives=src)
    src = source()
    src.offsets_host = src.offsets_host.copy()
    src.offsets_host[7] += 1
    with pytest.raises(ValueError, match=r"offsets\[7\] = \d+ is not the exclusive scan of counts"):
        DeviceEpochLoader(dcols, B, negatives=src)
    src = source()
    src.total_candidates += 1
    with pytest.raises(ValueError, match="are not those of its counts"):
        DeviceEpochLoader(dcols, B, negatives=src)
    # the device copies are read back once by the plan's constructor and held to the same rule
    src = source()
    src.counts[3] = C + 1
    with pytest.raises(_lib.HipLibraryError, match=rf"counts\[3\] = {C + 1} outside \[0, k = {C}\]"):
        DeviceEpochLoader(dcols, B, negatives=src)
    src = source()
    src.offsets[7] += 1
    with pytest.raises(_lib.HipLibraryError, match=r"offsets\[7\] = \d+ is not the sum \d+ of the counts before it"):
        DeviceEpochLoader(dcols, B, negatives=src)
    DeviceEpochLoader(dcols, B, negatives=source())        # and the untouched source builds
