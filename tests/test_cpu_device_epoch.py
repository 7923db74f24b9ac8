"""Host-side tests of the device epoch loader (``data/device_epoch.py``) and of the numpy restatement the GPU tests
compare against (``tests/sampler_reference.py``): the draw is without replacement over the unseen rows and uniform,
every refusal names its field or user, and the restated assembly with K = 0 is ``RecordLayout.write_indexed``."""
import itertools

import numpy as np
import pytest

from tests import sampler_reference as R


def _schema(groups=True):
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    S, D, Q = FeatureType.SPARSE, FeatureType.DENSE, FeatureType.SEQUENCE
    specs = [("user_id", S, 50, 16, "user", 1), ("movie_id", S, 40, 16, "item", 1), ("gender", S, 3, 4, "user", 1),
             ("genres", Q, 19, 8, "item", 6), ("movie_age", S, 8, 4, "context", 1), ("dow_sin", D, 0, 4, "context", 1),
             ("item_count", D, 0, 8, "item", 1)]
    return DatasetSchema(fields={n: FieldSchema(n, k, vocabulary_size=v, embedding_dim=d, group=g if groups else "",
                                                max_length=L) for n, k, v, d, g, L in specs})


def _dataset(P=30, n_users=5, n_items=40, seed=0):
    from deepfm_amd.data.packed import PackedColumns
    schema, rng = _schema(), np.random.default_rng(seed)
    user = rng.integers(0, n_users, P)
    feats = {"user_id": user + 1, "movie_id": rng.integers(1, n_items, P), "gender": rng.integers(0, 3, P),
             "genres": rng.integers(0, 19, (P, 6)), "movie_age": rng.integers(0, 8, P),
             "dow_sin": rng.random(P).astype(np.float32), "item_count": rng.random(P).astype(np.float32)}
    cols = PackedColumns(schema, feats, (rng.random(P) < 0.5).astype(np.float32))
    items = {"movie_id": np.arange(n_items) + 1, "genres": rng.integers(0, 19, (n_items, 6)),
             "item_count": rng.random(n_items).astype(np.float32)}
    return schema, cols, user.astype(np.int32), items


# ----------------------------------------------------------------------------- the restated sampler
@pytest.mark.parametrize("K", [1, 4, 16])
def test_restated_sampler_never_returns_seen_and_is_distinct(K):
    rng = np.random.default_rng(K)
    n_items = 70
    seen = [set(), set(range(n_items - K)), {0, 31, 32, n_items - 1}, set(rng.choice(n_items, 40, replace=False).tolist())]
    unseen = R.unseen_lists(seen, n_items)
    user_of = rng.integers(0, len(seen), 500)
    neg = R.sample_negatives(unseen, user_of, K, seed=3, epoch=2)
    assert neg.shape == (500, K) and neg.dtype == np.int32
    for p, u in enumerate(user_of):
        row = neg[p].tolist()
        assert len(set(row)) == K and not set(row) & seen[u] and all(0 <= i < n_items for i in row)


def test_user_with_exactly_k_unseen_gets_all_of_them():
    n_items, K = 37, 5
    left = {2, 11, 31, 32, 36}
    unseen = R.unseen_lists([set(range(n_items)) - left], n_items)
    neg = R.sample_negatives(unseen, np.zeros(64, np.int64), K, seed=1, epoch=0)
    assert all(set(row.tolist()) == left for row in neg)
    assert len({tuple(row.tolist()) for row in neg}) > 1          # and not always in one order


@pytest.mark.parametrize("epoch", [0, 1])
def test_draw_is_uniform_over_unordered_pairs(epoch):
    """One user, 12 items, 8 unseen, K = 2, 28 000 positives: Pearson's statistic over the 28 unordered pairs
    (expected 1000 each) below 55.5, the 0.1 % point of chi-square with 27 degrees of freedom; every pair occurs."""
    unseen = R.unseen_lists([{1, 4, 6, 9}], 12)
    neg = R.sample_negatives(unseen, np.zeros(28000, np.int64), 2, seed=0, epoch=epoch)
    pairs = {pr: 0 for pr in itertools.combinations(unseen[0].tolist(), 2)}
    assert len(pairs) == 28
    for a, b in np.sort(neg, axis=1).tolist():
        pairs[(a, b)] += 1
    counts = np.array(list(pairs.values()), dtype=np.float64)
    stat = float(((counts - 1000.0) ** 2 / 1000.0).sum())
    print(f"epoch {epoch}: Pearson statistic {stat:.1f} over 28 pairs, counts {int(counts.min())}..{int(counts.max())}")
    assert (counts > 0).all()
    assert stat < 55.5


def test_seen_sets_bitmap_and_prefix():
    from deepfm_amd.data import SeenSets
    for n_items in (31, 32, 33, 64, 100):
        rng = np.random.default_rng(n_items)
        sets = [set(), {0, 31 % n_items, 32 % n_items, n_items - 1}, set(rng.choice(n_items, n_items // 2, replace=False).tolist())]
        u = np.concatenate([np.full(len(s), i) for i, s in enumerate(sets)]).astype(np.int64)
        it = np.concatenate([np.array(sorted(s), dtype=np.int64) for s in sets])
        s = SeenSets.from_interactions(u, it, len(sets), n_items)
        W = (n_items + 31) // 32
        assert s.bitmap.shape == (3, W) and s.prefix.shape == (3, W + 1) and s.bitmap.dtype == s.prefix.dtype == np.uint32
        for i, st in enumerate(sets):
            bits = [(int(s.bitmap[i, b >> 5]) >> (b & 31)) & 1 for b in range(32 * W)]
            assert bits == [1 if (b in st or b >= n_items) else 0 for b in range(32 * W)]
            zeros = [32 - sum(bits[32 * w:32 * w + 32]) for w in range(W)]
            assert s.prefix[i].tolist() == [sum(zeros[:w]) for w in range(W + 1)]
            assert int(s.unseen[i]) == n_items - len(st)


# ----------------------------------------------------------------------------- refusals
def _sampler(**kw):
    import torch
    from deepfm_amd.data import DeviceColumns, ItemTable, NegativeSampler, SeenSets
    schema, cols, user_of, items = _dataset()
    n_users, n_items = 5, 40
    args = dict(columns=DeviceColumns(cols, torch.device("cpu")),
                seen=SeenSets.from_interactions(user_of, cols.ids[1] - 1, n_users, n_items), user_of=user_of,
                items=ItemTable(schema, items), num_neg=4)
    for k, v in kw.items():
        args[k] = v(args, schema, cols, user_of, items) if callable(v) else v
    return NegativeSampler(**args)


def test_valid_sampler_builds_on_the_host_with_default_roles_from_group():
    from deepfm_amd.data import Role
    s = _sampler()
    assert {k for k, r in s.roles.items() if r is Role.ITEM} == {"movie_id", "genres", "item_count"}
    assert all(s.roles[k] is Role.COPY for k in ("user_id", "gender", "movie_age", "dow_sin"))


@pytest.mark.parametrize("num_neg", [0, 17, -1])
def test_refuses_num_neg_outside_1_to_16(num_neg):
    with pytest.raises(ValueError, match=r"num_neg = -?\d+ outside \[1, 16\]"):
        _sampler(num_neg=num_neg)


def test_refuses_item_field_missing_from_the_table():
    from deepfm_amd.data import ItemTable
    with pytest.raises(ValueError, match="'genres' has role ITEM but the item table has no column"):
        _sampler(items=lambda a, schema, cols, u, items: ItemTable(schema, {k: v for k, v in items.items() if k != "genres"}))
    from deepfm_amd.data import Role
    with pytest.raises(ValueError, match="'gender' has role ITEM"):
        _sampler(roles={"gender": Role.ITEM})


def test_refuses_derived_field_that_is_not_sparse():
    from deepfm_amd.data import BucketDifference
    bd = BucketDifference(np.zeros(30, np.float32), np.zeros(40, np.float32), [1.0, 2.0], [0, 1, 2, 3])
    for name in ("dow_sin", "genres", "nope"):
        with pytest.raises(ValueError, match=f"derived field '{name}' is not a SPARSE field"):
            _sampler(derived={name: bd})
    assert _sampler(derived={"movie_age": bd}).roles["movie_age"].name == "BUCKET_DIFF"


def test_refuses_user_with_fewer_than_num_neg_unseen_and_names_it():
    from deepfm_amd.data import SeenSets

    def seen(a, schema, cols, user_of, items):
        u, it = list(user_of), list(cols.ids[1] - 1)
        victim = int(user_of[0])
        u += [victim] * 38
        it += list(range(38))                             # two rows left for the victim, four wanted
        return SeenSets.from_interactions(u, it, 5, 40)

    schema, cols, user_of, items = _dataset()
    with pytest.raises(ValueError, match=rf"user {int(user_of[0])} has [012] unseen items, fewer than num_neg = 4"):
        _sampler(seen=seen)

    def unused_victim(a, schema, cols, user_of, items):   # a user nobody trains on may have seen everything
        return SeenSets.from_interactions(list(user_of) + [5] * 40, list(cols.ids[1] - 1) + list(range(40)), 6, 40)
    _sampler(seen=unused_victim)


def test_refuses_seen_sets_over_one_gib():
    from deepfm_amd.data import SeenSets
    with pytest.raises(ValueError, match="more than 1073741824"):
        SeenSets.from_interactions([0], [0], 1 << 20, 1 << 14)


# ----------------------------------------------------------------------------- the restated assembly, K = 0
@pytest.mark.parametrize("B", [1, 7, 30])
def test_restated_assembly_without_negatives_is_write_indexed(B):
    from deepfm_amd.data.packed import RecordLayout
    schema, cols, _, _ = _dataset()
    lay = RecordLayout.of(schema, B)
    idx = np.random.default_rng(B).permutation(len(cols))[:B]
    want = np.zeros(lay.record_bytes, np.uint8)
    lay.write_indexed(want, cols, idx)
    assert np.array_equal(R.assemble(lay, cols, idx), want)
    if B > 1:                                             # a short batch: RecordLayout.write's padding tail
        want = np.zeros(lay.record_bytes, np.uint8)
        lay.write(want, cols, 1, B)
        assert np.array_equal(R.assemble(lay, cols, np.arange(1, B)), want)


def test_library_exports_the_sampler_symbols():
    import os
    import re
    from deepfm_amd import _lib
    lib = _lib.load()
    for name in ("dfm_sample_negatives", "dfm_assemble_plan_create", "dfm_assemble_plan_destroy", "dfm_record_assemble"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    # the one literal of the suite: library == binding == header == 11 (the other tests compare the three to each other)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "deepfm_hip.h")).read()
    assert lib.dfm_abi_version() == _lib.ABI_VERSION == 11
    assert re.search(r"#define DFM_ABI_VERSION 11\b", header)
