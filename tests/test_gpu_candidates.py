"""GPU tests of the evaluation candidates (``csrc/sampler.hip:dfm_sample_weighted``, ``csrc/catalogue.hip``,
``data/candidates.py``, ``training/catalogue.py``, ``FusedPredictor.evaluate_loader``) against the numpy restatements
``tests/candidates_reference.py`` / ``tests/sampler_reference.py``.  Item rows, ranks and copied float bits compare
bit for bit; only scores()-versus-predict carries the predictor tests' bound, imported from ``tests/helpers.py``.

1. the weighted draw vs the restatement at every word edge, C = 1, 17, 999;
2. the assembly of candidate lists longer than 16 (with repeated items) and of the whole catalogue vs the restatement;
3. ``dfm_catalogue_topk`` vs the restatement: ties, signed zeros, infinities, NaNs, every kind of target and user;
4. ``CatalogueScorer`` and ``evaluate_loader`` end to end for the three models.
"""
import numpy as np
import pytest
import torch

from tests import candidates_reference as CR
from tests import sampler_reference as R
from tests.helpers import RTOL, assert_close, npy
from tests.test_gpu_device_epoch import movielens_epoch

pytestmark = pytest.mark.gpu

DEV = "cuda"
W1 = 1 << 24


def _seen_sets(seen, n_items):
    from deepfm_amd.data import SeenSets
    u = np.concatenate([np.full(len(s), i, np.int64) for i, s in enumerate(seen)])
    it = np.concatenate([np.array(sorted(s), dtype=np.int64) for s in seen])
    return SeenSets.from_interactions(u, it, len(seen), n_items)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


# ----------------------------------------------------------------------------- 1. the weighted draw
def _weighted_case(n_items):
    rng = np.random.default_rng(n_items)
    last = 32 * ((n_items - 1) // 32)                     # first row of the last word
    lone = int(rng.integers(0, n_items))
    seen = [set(), set(range(n_items)) - {lone}, set(range(last)) if last else {0},
            set(rng.choice(n_items, n_items // 2, replace=False).tolist()), set(range(n_items))]
    weights = rng.integers(1, W1 + 1, n_items).astype(np.uint32)
    weights[rng.choice(n_items, 4, replace=False)] = [1, 1, W1, W1]
    user_of = np.array([0, 1, 2, 3, 4, 5, -1, 3, 0, 2, 1], np.int32)      # 4: nothing unseen; 5, -1: out of range
    return seen, weights, user_of, lone


def _draw_weighted(seen, weights, user_of, n_items, C, seed, epoch):
    from deepfm_amd import _lib
    bitmap, _ = _seen_sets(seen, n_items).upload(DEV)
    out = torch.full((len(user_of), C), -7, dtype=torch.int32, device=DEV)
    d_user, d_weight = _i32(user_of), _i32(weights)       # named: they must outlive the call
    _lib.check(_lib.load().dfm_sample_weighted(bitmap.data_ptr(), d_user.data_ptr(), d_weight.data_ptr(),
                                               len(user_of), len(seen), n_items, C, seed, epoch, None, out.data_ptr(),
                                               _lib.stream_handle()))
    return out.cpu().numpy()


@pytest.mark.parametrize("C", [1, 17, 999])
@pytest.mark.parametrize("n_items", [31, 32, 33, 100, 2049])
def test_weighted_draw_matches_restatement(n_items, C):
    seen, weights, user_of, lone = _weighted_case(n_items)
    unseen = R.unseen_lists(seen, n_items)
    got = {e: _draw_weighted(seen, weights, user_of, n_items, C, 5, e) for e in (0, 3)}
    for e, g in got.items():
        assert np.array_equal(g, CR.sample_weighted(unseen, user_of, weights, C, 5, e)), f"epoch {e}"
    assert not np.array_equal(got[0], got[3]), "two epochs gave the same draws"
    assert np.array_equal(_draw_weighted(seen, weights, user_of, n_items, C, 5, 3), got[3]), "a repeat gave other draws"
    assert not np.array_equal(_draw_weighted(seen, weights, user_of, n_items, C, 6, 3), got[3]), "seeds agree"
    g = got[0]
    for p, u in enumerate(user_of):                       # the properties, not only the restatement's word for them
        if u in (4, 5, -1):
            assert (g[p] == -1).all()
        else:
            assert not set(g[p].tolist()) & seen[u] and (g[p] >= 0).all() and (g[p] < n_items).all()
    assert (g[user_of == 1] == lone).all()
    assert (g[user_of == 2] >= 32 * ((n_items - 1) // 32)).all() or n_items <= 32


def test_weighted_draw_refuses_a_catalogue_over_its_cap():
    from deepfm_amd import _lib
    t = torch.zeros(8, dtype=torch.int32, device=DEV)
    rc = _lib.load().dfm_sample_weighted(t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 1, _lib.WEIGHTED_MAX_ITEMS + 1, 1,
                                         0, 0, None, t.data_ptr(), _lib.stream_handle())
    assert rc == _lib.ERR_UNSUPPORTED


# ----------------------------------------------------------------------------- 2. assembly of long candidate lists
def _ref_args(src, derived):
    bd = derived["movie_age_at_rating"]
    return {n: int(r) for n, r in src.roles.items()}, {"movie_age_at_rating": (bd.ctx, bd.item_val, bd.edges, bd.bucket_ids)}


@pytest.mark.parametrize("B", [64, 257])
@pytest.mark.parametrize("K", [17, 999, "catalogue"])
def test_assembly_of_candidate_lists_matches_restatement(K, B):
    from deepfm_amd.data import CatalogueCandidates, DeviceColumns, DeviceEpochLoader, WeightedNegatives
    P, n_items = 20, 100 if K == "catalogue" else 1100
    schema, cols, user_of, item_of, table, items, derived, seen = movielens_epoch(P, 4, n_items=n_items, seed=3)
    dcols = DeviceColumns(cols, DEV)
    if K == "catalogue":
        src = CatalogueCandidates(dcols, seen, user_of, table, derived=derived)
        K = n_items
    else:
        w = np.random.default_rng(K).integers(1, W1 + 1, n_items).astype(np.uint32)
        src = WeightedNegatives(dcols, seen, user_of, table, w, K, derived=derived, seed=9)
    loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=4, negatives=src, depth=3)
    loader.set_epoch(2)
    neg = loader.negatives_host(2)
    assert neg.shape == (P, K) and np.array_equal(src.neg_items.cpu().numpy(), neg)
    if isinstance(src, WeightedNegatives):
        seen_rows = [set(item_of[user_of == u].tolist()) for u in range(seen.n_users)]
        assert np.array_equal(neg, CR.sample_weighted(R.unseen_lists(seen_rows, n_items), user_of, w, K, 9, 2))
        if K == 999:
            assert any(len(set(row.tolist())) < K for row in neg), "no repeated item: the draw is with replacement"
    else:
        assert (neg == np.arange(n_items)[None, :]).all()
    order = loader.order.cpu().numpy()
    rows_total = P * (1 + K)
    assert loader.rows == rows_total and sorted(order.tolist()) == list(range(rows_total))
    roles, ref_derived = _ref_args(src, derived)
    for k in sorted({0, len(loader) // 2, len(loader) - 1}):
        want = R.assemble(loader.layout, cols, order[k * B:(k + 1) * B], K, neg, items, roles, ref_derived)
        assert np.array_equal(loader.record(k).cpu().numpy(), want), f"batch {k}"
    tail = rows_total - len(loader) * B                   # the trailing partial batch, as evaluate_loader reads it
    if tail:
        want = R.assemble(loader.layout, cols, order[rows_total - tail:], K, neg, items, roles, ref_derived)
        assert np.array_equal(loader.rows_into_next(rows_total - tail, tail).cpu().numpy(), want)
    plain = DeviceEpochLoader(dcols, B, shuffle=False, negatives=src, depth=2)   # the candidate rows alone, in order
    plain.set_epoch(2)
    first = P + K                                         # positive 1's candidates on (positive 0's ctx is NaN)
    want = R.assemble(plain.layout, cols, np.arange(first, first + B), K, neg, items, roles, ref_derived)
    got = plain.rows_into_next(first, B).cpu().numpy()
    assert np.array_equal(got, want)
    batch, labels = plain.layout.unpack(got)
    assert not labels.any() and len(set(batch["movie_age_at_rating"].tolist())) > 1 and batch["genres"].shape == (B, 6)


# ----------------------------------------------------------------------------- 3. the selection
def _topk(scores, seen, user_of, targets, K, exclude_seen, n_users=None):
    from deepfm_amd import _lib
    Q, n_items = scores.shape
    bitmap, _ = _seen_sets(seen, n_items).upload(DEV)
    items = torch.full((Q, K), -7, dtype=torch.int32, device=DEV)
    top = torch.full((Q, K), 7.0, dtype=torch.float32, device=DEV)
    rank = torch.full((Q,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    d_scores = torch.from_numpy(np.ascontiguousarray(scores)).to(DEV)     # named: they must outlive the call
    d_user, d_target = _i32(np.asarray(user_of, np.int32)), _i32(np.asarray(targets, np.int32))
    _lib.check(_lib.load().dfm_catalogue_topk(
        d_scores.data_ptr(), bitmap.data_ptr(), d_user.data_ptr(), d_target.data_ptr(), Q, n_users or len(seen),
        n_items, K, int(exclude_seen),
        items.data_ptr(), top.data_ptr(), rank.data_ptr(), status.data_ptr(), _lib.stream_handle()))
    return items.cpu().numpy(), top.cpu().numpy(), rank.cpu().numpy(), status.cpu().tolist()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: items"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), f"{what}: scores"
    assert np.array_equal(got[2], want[2]), f"{what}: ranks"
    assert got[3] == want[3], f"{what}: status"


def _selection_case(n_items, rng):
    few = set(range(n_items)) - set(rng.choice(n_items, min(5, n_items), replace=False).tolist())
    seen = [set(), set(range(n_items)), set(rng.choice(n_items, n_items // 2, replace=False).tolist()), few]
    patterns = [np.full(n_items, 0.25, np.float32),
                rng.integers(0, 4, n_items).astype(np.float32) / 4,
                np.where(rng.random(n_items) < 0.5, np.float32(-0.0), np.float32(0.0)) * (rng.random(n_items) < 0.7),
                rng.choice(np.array([np.inf, -np.inf, 0.5, -1.5, 2.0], np.float32), n_items),
                rng.standard_normal(n_items).astype(np.float32)]
    scores, user_of, targets = [], [], []
    for u, s in enumerate(seen):
        for j, pat in enumerate(patterns):
            scores.append(pat.astype(np.float32))
            user_of.append(u)
            kind = (u + j) % 3                             # a seen target, an unseen one, none
            pool = sorted(s) if kind == 0 else sorted(set(range(n_items)) - s) if kind == 1 else []
            targets.append(int(rng.choice(pool)) if pool else -1)
    return np.stack(scores), seen, user_of, targets


@pytest.mark.parametrize("K", [1, 10, 128])
@pytest.mark.parametrize("n_items", [1, 31, 33, 64, 65, 1000, 4097, 7001])
def test_catalogue_topk_matches_restatement(n_items, K):
    from deepfm_amd import _lib
    assert (n_items > _lib.TOPK_LDS_ITEMS) == (n_items == 7001)          # one case takes the several-pass kernel
    scores, seen, user_of, targets = _selection_case(n_items, np.random.default_rng(n_items + K))
    assert any(t >= 0 and t in seen[u] for u, t in zip(user_of, targets)) or n_items == 1
    for exclude in (True, False):
        got = _topk(scores, seen, user_of, targets, K, exclude)
        _same(got, CR.catalogue_topk(scores, seen, user_of, targets, K, exclude, len(seen)), f"exclude_seen={exclude}")
        assert got[3] == [0, 0, 0]
    got = _topk(scores, seen, user_of, targets, K, True)
    full = got[0][np.asarray(user_of) == 1]                # seen everything: the target only, or nothing
    t_full = np.asarray(targets)[np.asarray(user_of) == 1]
    assert (full[:, 0] == t_full).all() and (full[:, 1:] == -1).all()
    assert (got[2][np.asarray(user_of) == 1] == np.where(t_full >= 0, 0, -1)).all()


def test_catalogue_topk_counts_nans_bad_users_and_bad_targets():
    n_items, K = 70, 10
    rng = np.random.default_rng(0)
    scores = rng.standard_normal((6, n_items)).astype(np.float32)
    seen = [{3, 40}, set()]
    scores[0, 3] = np.nan                                  # on a seen row: not counted
    assert _topk(scores, seen, [0, 1, 0, 1, 0, 1], [-1] * 6, K, True)[3] == [0, 0, 0]
    scores[1, 3] = scores[2, 69] = np.nan                  # on eligible rows
    user_of, targets = [0, 1, 0, 2, -1, 1], [40, -1, 5, 7, 70, -2]
    got = _topk(scores, seen, user_of, targets, K, True)
    want = CR.catalogue_topk(scores, seen, user_of, targets, K, True, 2)
    assert got[3] == want[3] == [2, 2, 2]
    for q in (3, 4):                                       # users out of range: padding, no rank
        assert (got[0][q] == -1).all() and np.isneginf(got[1][q]).all() and got[2][q] == -1
    assert got[2][5] == -1                                 # a target out of range is no target
    clean = [0, 5]
    _same(tuple(a[clean] for a in got[:3]) + ([],), tuple(a[clean] for a in want[:3]) + ([],), "rows without NaN")
    assert _topk(scores, seen, [0] * 6, [-1] * 6, K, False)[3] == [3, 0, 0]   # exclude_seen off: the seen row counts


def test_catalogue_topk_refuses_a_catalogue_over_its_cap():
    from deepfm_amd import _lib
    t = torch.zeros(8, dtype=torch.int32, device=DEV)
    rc = _lib.load().dfm_catalogue_topk(t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, 1, 1, _lib.MAX_CANDIDATES + 1, 1, 1,
                                        t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), _lib.stream_handle())
    assert rc == _lib.ERR_UNSUPPORTED


# ----------------------------------------------------------------------------- 4. end to end
Q, N_ITEMS, B = 37, 100, 64


def _eval_set(seed=0):
    """Q queries (one per user) over the small MovieLens-shaped schema: the query rows carry their held-out item."""
    from deepfm_amd.data import BucketDifference, ItemTable, SeenSets
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.synthetic import movielens_fields, random_fields_batch, schema_from_fields
    rng = np.random.default_rng(seed)
    fields = movielens_fields(Q, N_ITEMS)
    schema = schema_from_fields(fields)
    item_fields = [f for f in fields if f["group"] == "item"]
    items = {f["name"]: random_fields_batch([f], N_ITEMS, rng, zero_frac=0.0)[f["name"]] for f in item_fields}
    items["movie_id"] = np.arange(N_ITEMS, dtype=np.int64) + 1
    feats = random_fields_batch(fields, Q, rng, zero_frac=0.0)
    user_of = np.arange(Q, dtype=np.int32)
    target = rng.integers(0, N_ITEMS, Q)
    feats["user_id"] = user_of.astype(np.int64) + 1
    for name, col in items.items():
        feats[name] = col[target]
    hist_u = rng.integers(0, Q, 900)
    hist_i = rng.integers(0, N_ITEMS, 900)
    seen = SeenSets.from_interactions(np.concatenate([hist_u, user_of]), np.concatenate([hist_i, target]), Q, N_ITEMS)
    bd = BucketDifference(rng.uniform(20.0, 30.0, Q).astype(np.float32), rng.uniform(0.0, 28.0, N_ITEMS).astype(np.float32),
                          np.array([1, 2, 5, 10, 20], np.float32), np.arange(7, dtype=np.int64))
    cols = PackedColumns(schema, feats, np.ones(Q, np.float32))
    counts = np.bincount(np.concatenate([hist_i, target]), minlength=N_ITEMS)
    return fields, schema, cols, user_of, target, ItemTable(schema, items), items, {"movie_age_at_rating": bd}, seen, counts


def _host_rows(schema, cols, rows, K, neg, items, src, derived):
    """The virtual rows ``rows`` as host ``PackedColumns``, through the restated assembly."""
    from deepfm_amd.data.packed import PackedColumns, RecordLayout
    lay = RecordLayout.of(schema, len(rows))
    roles, ref_derived = _ref_args(src, derived)
    batch, labels = lay.unpack(R.assemble(lay, cols, rows, K, neg, items, roles, ref_derived))
    return PackedColumns(schema, {k: v.copy() for k, v in batch.items()}, labels.copy())


@pytest.mark.parametrize("kind", ["deepfm", "xdeepfm", "attention_deepfm"])
def test_catalogue_scorer_and_evaluate_loader_end_to_end(kind):
    from deepfm_amd.data import (CatalogueCandidates, DeviceColumns, DeviceEpochLoader, WeightedNegatives,
                                 item_weights)
    from deepfm_amd.training import CatalogueScorer, MixedSchemaPredictor
    from tests.test_gpu_mixed_predict import _movielens_model
    fields, schema, cols, user_of, target, table, items, derived, seen, counts = _eval_set()
    _, model = _movielens_model(kind, fields, seed=2)
    pred = MixedSchemaPredictor(model, B)
    dcols = DeviceColumns(cols, DEV)
    cand = CatalogueCandidates(dcols, seen, user_of, table, derived=derived)
    scorer = CatalogueScorer(pred, cand)
    got = scorer.scores()
    assert got.shape == (Q, N_ITEMS) and got.is_cuda
    # the same rows built on the host, through predict()
    neg = np.broadcast_to(np.arange(N_ITEMS, dtype=np.int32), (Q, N_ITEMS))
    host = _host_rows(schema, cols, np.arange(Q, Q + Q * N_ITEMS), N_ITEMS, neg, items, cand, derived)
    want = []
    for s in range(0, len(host), B):
        lay_cols = {n: torch.from_numpy(np.ascontiguousarray(v[s:s + B])).to(DEV)
                    for n, v in _field_columns(host).items()}
        want.append(pred.predict(lay_cols).view(-1))
    want = torch.cat(want).view(Q, N_ITEMS)
    assert_close(npy(got), npy(want), rtol=RTOL, what=f"{kind}: scores() vs predict on host-built rows")
    # recommend / evaluate vs numpy on those very scores
    sc = npy(got)
    seen_rows = [set(np.flatnonzero([(int(seen.bitmap[u, i >> 5]) >> (i & 31)) & 1 for i in range(N_ITEMS)]).tolist())
                 for u in range(Q)]
    none = [-1] * Q
    for k, excl in ((10, True), (128, True), (5, False)):
        it, top = scorer.recommend(k, exclude_seen=excl)
        w_it, w_top, _, _ = CR.catalogue_topk(sc, seen_rows, user_of, none, k, excl, Q)
        assert np.array_equal(npy(it), w_it) and np.array_equal(npy(top).view(np.uint32), w_top.view(np.uint32))
    assert all(not set(row[row >= 0].tolist()) & seen_rows[u] for u, row in enumerate(npy(scorer.recommend(10)[0])))
    targets = target.astype(np.int32).copy()
    targets[::9] = -1                                      # some queries without a target
    ks = [1, 5, 10, 20]
    rank = CR.catalogue_topk(sc, seen_rows, user_of, targets, 1, True, Q)[2]
    m = scorer.evaluate(targets, ks)
    assert m == CR.full_ranking_metrics(rank, ks), (m, CR.full_ranking_metrics(rank, ks))
    assert set(m) == {f"{a}@{k}" for a in ("HR", "NDCG") for k in ks} and 0.0 < m["HR@20"] <= 1.0
    # evaluate_loader over the weighted candidates == evaluate(columns) over the host-built rows of the same draw
    K = 20
    src = WeightedNegatives(dcols, seen, user_of, table, item_weights(counts, 0.75), K, derived=derived, seed=11)
    loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=5, negatives=src, depth=3)
    loader.set_epoch(1)
    assert loader.rows % B                                  # a trailing partial batch
    rows = loader.order.cpu().numpy()
    host = _host_rows(schema, cols, rows, K, loader.negatives_host(1), items, src, derived)
    m_loader = pred.evaluate_loader(loader, ranking_ks=ks)
    s_loader, l_loader = pred.last_scores.clone(), pred.last_labels.clone()
    m_host = pred.evaluate(host, ranking_ks=ks)
    assert torch.equal(s_loader, pred.last_scores) and torch.equal(l_loader, pred.last_labels)
    assert m_loader == m_host, (m_loader, m_host)
    assert {"auc", "logloss", "HR@10", "NDCG@10"} <= set(m_loader) and int(npy(l_loader).sum()) == Q


def _field_columns(cols):
    from tests.test_gpu_device_epoch import field_columns
    return field_columns(cols)
