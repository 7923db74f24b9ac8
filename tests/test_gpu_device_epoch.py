"""GPU tests of the device epoch loader (``csrc/sampler.hip``, ``data/device_epoch.py``) against the numpy restatement
``tests/sampler_reference.py`` and ``RecordLayout``'s host writes.  Every output is integer ids or copied float bits:
all comparisons are bit for bit, no tolerance anywhere.

1. the sampler vs the restatement at every word edge (n_items 31..100), K = 1, 4, 16; epochs differ, runs repeat;
2. the assembly with K = 0 vs ``RecordLayout.write_indexed`` for four schemas, B around the workgroup's wave edge,
   and a short batch whose tail must be zero;
3. the assembly with negatives (ITEM / COPY / BUCKET_DIFF with NaNs and a negative difference) vs the restatement;
4. loader records through ``FusedMixedDeepFMStep.run_from`` and ``MixedSchemaPredictor.predict_from``.
"""
import numpy as np
import pytest
import torch

from tests import sampler_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _fs(name, kind, vocab=0, dim=8, group="", L=1):
    from deepfm_amd.data.schema import FeatureType, FieldSchema
    return FieldSchema(name, FeatureType(kind), vocabulary_size=vocab, embedding_dim=dim, group=group, max_length=L)


def _schema(specs):
    from deepfm_amd.data.schema import DatasetSchema
    return DatasetSchema(fields={s.name: s for s in specs})


def movielens_schema(n_users=20, n_items=50):
    """The reference's MovieLens schema (widths 4 / 8 / 16, bag of 6, its groups) over small tables."""
    sp = [("user_id", n_users + 1, 16, "user"), ("movie_id", n_items + 1, 16, "item"), ("gender", 3, 4, "user"),
          ("age", 8, 4, "user"), ("occupation", 22, 8, "user"), ("zip_prefix", 40, 8, "user")]
    fs = [_fs(n, "sparse", v, d, g) for n, v, d, g in sp]
    fs.append(_fs("genres", "sequence", 20, 8, "item", 6))
    fs += [_fs("release_year_bucket", "sparse", 16, 4, "item"), _fs("movie_age_at_rating", "sparse", 8, 4, "context"),
           _fs("num_genres", "sparse", 8, 4, "item")]
    fs += [_fs(n, "dense", 0, 4, "context") for n in ("dow_sin", "dow_cos", "hour_sin", "hour_cos")]
    fs += [_fs("user_rating_count", "dense", 0, 8, "user"), _fs("item_rating_count", "dense", 0, 8, "item")]
    return _schema(fs)


SCHEMAS = {
    "uniform": lambda: _schema([_fs("a", "sparse", 50), _fs("x", "dense"), _fs("b", "sparse", 9), _fs("c", "sparse", 700)]),
    "movielens": movielens_schema,
    "no_sparse": lambda: _schema([_fs("x", "dense"), _fs("g", "sequence", 20, 8, "", 3), _fs("y", "dense")]),
    "no_dense": lambda: _schema([_fs("a", "sparse", 50), _fs("g", "sequence", 20, 8, "", 6), _fs("b", "sparse", 9)]),
}


def random_columns(schema, n, rng):
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.schema import FeatureType
    feats = {}
    for name, s in schema.fields.items():
        if s.feature_type is FeatureType.SPARSE:
            feats[name] = rng.integers(0, s.vocabulary_size, n)
        elif s.feature_type is FeatureType.DENSE:
            feats[name] = rng.standard_normal(n).astype(np.float32)
        else:
            feats[name] = rng.integers(0, s.vocabulary_size, (n, s.max_length))
    return PackedColumns(schema, feats, (rng.random(n) < 0.4).astype(np.float32))


def field_columns(cols):
    """Per field, schema order: its host column."""
    from deepfm_amd.data.schema import FeatureType
    out, its = {}, {FeatureType.SPARSE: iter(cols.ids), FeatureType.DENSE: iter(cols.dense), FeatureType.SEQUENCE: iter(cols.bags)}
    for name, s in cols.schema.fields.items():
        out[name] = next(its[s.feature_type])
    return out


# ----------------------------------------------------------------------------- 1. the sampler
def _sampler_case(n_items, K):
    rng = np.random.default_rng(1000 * n_items + K)
    edge = {i for i in (0, 31, 32, n_items - 1) if i < n_items}
    rest = lambda: set(rng.choice(n_items, n_items - max(K, n_items // 2), replace=False).tolist())
    seen = [set(), set(rng.choice(n_items, n_items - K, replace=False).tolist()), edge, rest(), rest()]
    user_of = rng.integers(0, 5, 257).astype(np.int32)
    user_of[:5] = np.arange(5)
    return seen, user_of


def _draw(seen, user_of, n_items, K, seed, epoch):
    from deepfm_amd import _lib
    from deepfm_amd.data import SeenSets
    u = np.concatenate([np.full(len(s), i, np.int64) for i, s in enumerate(seen)])
    it = np.concatenate([np.array(sorted(s), dtype=np.int64) for s in seen])
    s = SeenSets.from_interactions(u, it, len(seen), n_items)
    bitmap, prefix = s.upload(DEV)
    out = torch.full((len(user_of), K), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().dfm_sample_negatives(bitmap.data_ptr(), prefix.data_ptr(), torch.from_numpy(user_of).to(DEV).data_ptr(),
                                                len(user_of), len(seen), n_items, K, seed, epoch, None, out.data_ptr(),
                                                _lib.stream_handle()))
    return out.cpu().numpy()


@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("n_items", [31, 32, 33, 64, 100])
def test_sampler_matches_restatement(n_items, K):
    seen, user_of = _sampler_case(n_items, K)
    unseen = R.unseen_lists(seen, n_items)
    got = {e: _draw(seen, user_of, n_items, K, 5, e) for e in (0, 3)}
    for e, g in got.items():
        assert np.array_equal(g, R.sample_negatives(unseen, user_of, K, 5, e)), f"epoch {e}"
    assert not np.array_equal(got[0], got[3]), "two epochs gave the same draws"
    assert np.array_equal(_draw(seen, user_of, n_items, K, 5, 3), got[3]), "the same (seed, epoch) gave other draws"
    assert not np.array_equal(_draw(seen, user_of, n_items, K, 6, 3), got[3]), "two seeds gave the same draws"
    for p, u in enumerate(user_of):                      # the property itself, not only the restatement's word for it
        row = got[0][p].tolist()
        assert len(set(row)) == K and not set(row) & seen[u] and all(0 <= i < n_items for i in row)
    assert all(set(got[0][p].tolist()) == set(unseen[1].tolist()) for p in np.flatnonzero(user_of == 1))


# ----------------------------------------------------------------------------- 2. assembly, K = 0
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", list(SCHEMAS))
def test_assembly_without_negatives_is_write_indexed(kind, B):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import RecordLayout
    schema, n = SCHEMAS[kind](), 300
    cols = random_columns(schema, n, np.random.default_rng(B))
    loader = DeviceEpochLoader(DeviceColumns(cols, DEV), B, shuffle=True, seed=2, depth=2)
    lay = RecordLayout.of(schema, B)
    assert loader.record_bytes == lay.record_bytes and len(loader) == n // B and loader.layout == lay
    loader.set_epoch(1)
    order = loader.order.cpu().numpy()
    assert sorted(order.tolist()) == list(range(n))
    for k in sorted({0, len(loader) - 1}):
        want = np.zeros(lay.record_bytes, np.uint8)
        lay.write_indexed(want, cols, order[k * B:(k + 1) * B])
        rec = loader.record(k)
        assert rec.data_ptr() % 256 == 0
        assert np.array_equal(rec.cpu().numpy(), want), f"batch {k}"
    # a short batch over a dirty record: the tail is written as zeros
    cnt = B - 1 if B > 1 else 1
    dirty = torch.full((lay.record_bytes,), 0xAB, dtype=torch.uint8, device=DEV)
    loader.assemble_into(dirty, 5, cnt)
    want, idx = np.zeros(lay.record_bytes, np.uint8), order[5:5 + cnt]
    wi, wd, wl, wb = lay.views(want)
    if lay.n_sparse:
        wi[:, :cnt] = cols.ids[:, idx]
    if lay.n_dense:
        wd[:, :cnt] = cols.dense[:, idx]
    wl[:cnt] = cols.labels[idx]
    for blk, bag in zip(wb, cols.bags):
        blk[:cnt] = bag[idx]
    got = dirty.cpu().numpy()
    ids, dense, labels, bags = lay.views(got)
    assert np.array_equal(ids, wi) and np.array_equal(dense.view(np.uint32), wd.view(np.uint32))
    assert np.array_equal(labels.view(np.uint32), wl.view(np.uint32)) and all(np.array_equal(a, b) for a, b in zip(bags, wb))
    assert not ids[:, cnt:].any() and not dense[:, cnt:].view(np.uint32).any() and not labels[cnt:].view(np.uint32).any()
    assert all(not b[cnt:].any() for b in bags)
    # unshuffled: contiguous slices, RecordLayout.write
    plain = DeviceEpochLoader(DeviceColumns(cols, DEV), B, shuffle=False, depth=2)
    want = np.zeros(lay.record_bytes, np.uint8)
    lay.write(want, cols, (len(plain) - 1) * B, len(plain) * B)
    assert np.array_equal(plain.record(len(plain) - 1).cpu().numpy(), want)


# ----------------------------------------------------------------------------- 3. assembly with negatives
def movielens_epoch(P=130, K=4, n_users=20, n_items=50, seed=0):
    """A MovieLens-shaped set: positives, item table, seen-sets and a BUCKET_DIFF field with NaNs in both operands
    and negative differences."""
    from deepfm_amd.data import BucketDifference, ItemTable, SeenSets
    rng = np.random.default_rng(seed)
    schema = movielens_schema(n_users, n_items)
    cols = random_columns(schema, P, rng)
    user_of = rng.integers(0, n_users, P).astype(np.int32)
    item_of = rng.integers(0, n_items, P)
    cols.ids[0], cols.ids[1] = user_of + 1, item_of + 1
    items = {"movie_id": np.arange(n_items, dtype=np.int64) + 1, "genres": rng.integers(0, 20, (n_items, 6)),
             "release_year_bucket": rng.integers(0, 16, n_items), "num_genres": rng.integers(0, 8, n_items),
             "item_rating_count": rng.random(n_items).astype(np.float32)}
    ctx = rng.uniform(0.0, 30.0, P).astype(np.float32)
    item_val = rng.uniform(-5.0, 25.0, n_items).astype(np.float32)       # differences of both signs
    ctx[::17] = np.nan
    item_val[::11] = np.nan
    item_val[3] = ctx[1]                                                 # a difference of exactly 0 exists
    edges = np.array([1.0, 3.0, 5.0, 10.0, 15.0, 20.0], np.float32)
    bd = BucketDifference(ctx, item_val, edges, np.array([1, 2, 3, 4, 5, 6, 7, 0], np.int64))
    seen = SeenSets.from_interactions(user_of, item_of, n_users, n_items)
    return schema, cols, user_of, item_of, ItemTable(schema, items), items, {"movie_age_at_rating": bd}, seen


def test_assembly_with_negatives_matches_restatement():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, NegativeSampler, Role
    P, K, B = 130, 4, 65
    schema, cols, user_of, item_of, table, items, derived, seen = movielens_epoch(P, K)
    dcols = DeviceColumns(cols, DEV)
    sampler = NegativeSampler(dcols, seen, user_of, table, K, derived=derived, seed=9)
    assert {n for n, r in sampler.roles.items() if r is Role.ITEM} == set(items)
    loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=4, negatives=sampler, depth=3)
    assert len(loader) == 10
    loader.set_epoch(2)
    neg = loader.negatives_host(2)
    seen_rows = [set(item_of[user_of == u].tolist()) for u in range(seen.n_users)]
    assert np.array_equal(neg, R.sample_negatives(R.unseen_lists(seen_rows, seen.n_items), user_of, K, 9, 2))
    assert np.array_equal(sampler.neg_items.cpu().numpy(), neg)
    order = loader.order.cpu().numpy()
    assert sorted(order.tolist()) == list(range(P * (1 + K)))
    bd = derived["movie_age_at_rating"]
    ref_derived = {"movie_age_at_rating": (bd.ctx, bd.item_val, bd.edges, bd.bucket_ids)}
    roles = {n: int(r) for n, r in sampler.roles.items()}
    copy = [n for n, r in sampler.roles.items() if r is Role.COPY]
    buckets = set()
    for k, rec in enumerate(loader):
        rows = order[k * B:(k + 1) * B]
        want = R.assemble(loader.layout, cols, rows, K, neg, items, roles, ref_derived)
        got = rec.cpu().numpy()
        assert np.array_equal(got, want), f"batch {k}"
        batch, labels = loader.layout.unpack(got)
        p = np.where(rows >= P, (rows - P) // K, rows)
        src = field_columns(cols)
        for n in copy:
            assert np.array_equal(batch[n].view(np.uint8), src[n][p].view(np.uint8)), f"batch {k}: COPY column {n}"
        assert np.array_equal(labels, np.where(rows >= P, np.float32(0), cols.labels[p]))
        buckets |= set(batch["movie_age_at_rating"][rows >= P].tolist())
    assert {1, 2, 0} <= buckets                        # NaN or negative difference (id 1), [0, 1) (id 2), >= 20 (id 0)


# ----------------------------------------------------------------------------- 4. through the consumers
def _model(schema, seed):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = 16
    cfg.dnn.hidden_units = [32, 32]
    cfg.dnn.dropout = 0.1
    torch.manual_seed(seed)
    model = create_model("deepfm", schema, cfg).cuda().train()
    model.embedding.strict_indices = True
    return model


def test_loader_records_through_the_fused_step_and_the_predictor():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, NegativeSampler
    from deepfm_amd.training import DenseTableAdam, FusedMixedDeepFMStep, MixedSchemaPredictor
    P, K, B = 130, 4, 64
    schema, cols, user_of, item_of, table, items, derived, seen = movielens_epoch(P, K, seed=1)
    dcols = DeviceColumns(cols, DEV)
    sampler = NegativeSampler(dcols, seen, user_of, table, K, derived=derived, seed=1)
    loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=1, negatives=sampler, depth=2)
    loader.set_epoch(1)
    neg, order = loader.negatives_host(1), loader.order.cpu().numpy()
    bd = derived["movie_age_at_rating"]
    host = [R.assemble(loader.layout, cols, order[k * B:(k + 1) * B], K, neg, items, {n: int(r) for n, r in sampler.roles.items()},
                       {"movie_age_at_rating": (bd.ctx, bd.item_val, bd.edges, bd.bucket_ids)}) for k in range(3)]
    finals = []
    for source in ("loader", "host"):
        model = _model(schema, 3)
        opt = DenseTableAdam(model, lr=1e-2, l2=1e-3, max_grad_norm=0.5)
        step = FusedMixedDeepFMStep(model, opt, B, use_graph=True)
        step.capture()
        records = iter(loader) if source == "loader" else (torch.from_numpy(h).cuda() for h in host)
        for _ in range(3):                              # depth 2: the third record reuses the first one's slot
            step.run_from(next(records))
            model.embedding.raise_on_bad_index()
        torch.cuda.synchronize()
        finals.append([opt.flat_param.clone(), opt.flat_m.clone(), opt.flat_v.clone(), step.loss.clone()])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
    model.eval()
    pred = MixedSchemaPredictor(model, B)
    rec = loader.record(3)
    got = pred.predict_from(rec).clone()
    batch, _ = loader.layout.unpack(rec.clone())
    want = pred.predict({k: v.contiguous() for k, v in batch.items()})
    assert torch.equal(got, want)
    assert np.array_equal(rec.cpu().numpy(), R.assemble(loader.layout, cols, order[3 * B:4 * B], K, neg, items,
                                                        {n: int(r) for n, r in sampler.roles.items()},
                                                        {"movie_age_at_rating": (bd.ctx, bd.item_val, bd.edges, bd.bucket_ids)}))
