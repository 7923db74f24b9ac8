"""GPU: permutation field importance.  Every comparison is an equality: the keys and the permuted records against the
numpy restatement (tests/importance_reference.py) bit for bit and byte for byte, the score buffer of every variant
against ``predict_from`` over host-built permuted records (a predictor's score of a sample does not depend on its batch
mates), the report against the metric functions on those scores.  The one bound (an AUC in [0.4, 0.6]) is a bound on
chance, stated where it is used."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import importance_reference as IR
from tests.helpers import npy

pytestmark = pytest.mark.gpu

B = IR.B
DEV = "cuda"


def _upload(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_perm(seed, repeat, n):
    from deepfm_amd.training.importance import permutation_keys
    keys = permutation_keys(seed, repeat, n, torch.device(DEV))
    return keys, torch.sort(keys).values


# ----------------------------------------------------------------------------- 1. keys
@pytest.mark.parametrize("n", IR.SIZES)
def test_keys_equal_the_restatement_bit_for_bit(n):
    for seed in (0, 2 ** 63 + 5):
        for repeat in (0, 3):
            keys, ordered = _device_perm(seed, repeat, n)
            assert np.array_equal(npy(keys), IR.keys(seed, repeat, n)), (seed, repeat)
            assert np.array_equal(npy(ordered) & 0xFFFFFFFF, IR.permutation(seed, repeat, n)), (seed, repeat)


def test_keys_refusals():
    from deepfm_amd import _lib
    lib, out = _lib.load(), torch.empty(4, dtype=torch.int64, device=DEV)
    for args in ((0, 0, 0), (0, 0, 1 << 31), (0, -1, 4), (0, 1 << 24, 4)):
        with pytest.raises(_lib.HipLibraryError, match="outside"):
            _lib.check(lib.dfm_permutation_keys(*args, out.data_ptr(), _lib.stream_handle()))


# ----------------------------------------------------------------------------- 2. permuted records
def _masks(lay):
    """Empty, one field of each kind the schema has, the first and the last field, all fields."""
    F = len(lay.names)
    masks = {0, 1, 1 << (F - 1), (1 << F) - 1}
    for kind in set(lay.kinds):
        masks.add(1 << lay.kinds.index(kind))
    return sorted(masks)


def _batches(n):
    """The first, a middle and the trailing partial batch, and a short count in the middle of the set."""
    nb = (n + B - 1) // B
    out = {(k * B, min(B, n - k * B)) for k in (0, nb // 2, nb - 1)}
    if n > B + 10:
        out.add((B, 10))
    return sorted(out)


def _reaching_repeat(n, seed=5):
    """A repeat whose permutation sends a slot of the first batch to a sample of the partial last record."""
    last = (n - 1) // B * B
    for repeat in range(64):
        if (IR.permutation(seed, repeat, n)[:min(B, n)] >= last).any():
            return repeat
    raise AssertionError("no such permutation among 64")


@pytest.mark.parametrize("which", IR.SCHEMAS)
@pytest.mark.parametrize("n", IR.SIZES)
def test_permuted_records_equal_the_restatement_byte_for_byte(which, n):
    from deepfm_amd.data.packed import RecordLayout
    from deepfm_amd.training.importance import RecordSet, permute_into, record_fields
    cols = IR.columns_of(IR.schema_fields(which), n, 3)
    lay = RecordLayout.of(cols.schema, B)
    recs = IR.set_records(lay, cols)
    rs = RecordSet(lay, n, _upload(recs))
    seed, repeat = 5, _reaching_repeat(n)
    perm = IR.permutation(seed, repeat, n)
    if n > B and n % B:
        assert (perm[:B] >= n // B * B).any()          # a slot of the first batch reads the partial last record
    _, ordered = _device_perm(seed, repeat, n)
    fields = record_fields(lay)
    canary = np.full(lay.record_bytes + 256, 0xA5, np.uint8)
    for mask in _masks(lay):
        for first, count in _batches(n):
            out = _upload(canary)
            permute_into(rs, fields, ordered, mask, first, count, out)
            want = IR.permute_record(lay, recs, n, perm, mask, first, count, canary.copy())
            got = npy(out)
            assert (got[lay.record_bytes:] == 0xA5).all(), "bytes beyond record_bytes were written"
            assert np.array_equal(got, want), (which, n, bin(mask), first, count)
    # the empty mask needs no keys and is RecordLayout.write's record
    out = _upload(canary)
    permute_into(rs, fields, None, 0, 0, min(B, n), out)
    assert np.array_equal(npy(out)[:lay.record_bytes], recs[0][:lay.record_bytes])


def test_keys_that_are_no_permutation_never_leave_the_set():
    """Low words at or above n are taken as the slot's own sample."""
    from deepfm_amd.data.packed import RecordLayout
    from deepfm_amd.training.importance import RecordSet, permute_into, record_fields
    n = 70
    cols = IR.columns_of(IR.schema_fields("mixed"), n, 4)
    lay = RecordLayout.of(cols.schema, B)
    recs = IR.set_records(lay, cols)
    rs = RecordSet(lay, n, _upload(recs))
    bad = torch.full((n,), (5 << 32) | 0xFFFFFFFF, dtype=torch.int64, device=DEV)
    bad[1] = n
    out = torch.zeros(lay.record_bytes, dtype=torch.uint8, device=DEV)
    permute_into(rs, record_fields(lay), bad, (1 << len(lay.names)) - 1, 0, B, out)
    assert np.array_equal(npy(out), recs[0][:lay.record_bytes])


def test_permute_refusals():
    from deepfm_amd import _lib
    from deepfm_amd.data.packed import RecordLayout
    from deepfm_amd.training.importance import record_fields
    n = 70
    cols = IR.columns_of(IR.schema_fields("mixed"), n, 4)
    lay = RecordLayout.of(cols.schema, B)
    stride = (lay.record_bytes + 255) // 256 * 256
    dset = torch.zeros(2, stride, dtype=torch.uint8, device=DEV)
    keys = torch.sort(_device_perm(0, 0, n)[0]).values
    out = torch.zeros(stride, dtype=torch.uint8, device=DEV)
    lib, F = _lib.load(), len(lay.names)
    good = dict(d_set=dset.data_ptr(), stride=stride, fields=record_fields(lay), F=F, B=B, lo=lay.labels_offset,
                nbytes=lay.record_bytes, n=n, keys=keys.data_ptr(), mask=1, first=0, count=B, out=out.data_ptr())

    def call(**over):
        a = dict(good, **over)
        return lib.dfm_records_permute(a["d_set"], a["stride"], a["fields"], a["F"], a["B"], a["lo"], a["nbytes"], a["n"],
                                       a["keys"], a["mask"], a["first"], a["count"], a["out"], _lib.stream_handle())
    _lib.check(call())
    shifted = record_fields(lay)
    shifted[F - 1].offset += 8
    longer = record_fields(lay)
    longer[1].max_length += 1                                       # the first SEQUENCE field: the layout moves
    for over, match in ((dict(first=64, count=7), "outside the set"), (dict(count=B + 1), "more than one batch"),
                        (dict(count=0), "outside the set"), (dict(first=-1), "outside the set"),
                        (dict(mask=1 << F), "mask names a field"), (dict(keys=None), "needs the sorted keys"),
                        (dict(fields=shifted), "offset"), (dict(fields=longer), "is not the layout's"),
                        (dict(nbytes=lay.record_bytes + 16), "record_bytes"), (dict(lo=lay.labels_offset + 4), "labels_offset"),
                        (dict(stride=lay.record_bytes - 16), "set_stride"), (dict(stride=stride + 8), "set_stride"),
                        (dict(out=out.data_ptr() + 8), "16-byte aligned"), (dict(F=0), "num_fields"),
                        (dict(n=0), "sample count"), (dict(B=0), "batch_size")):
        with pytest.raises(_lib.HipLibraryError, match=match):
            _lib.check(call(**over))
    assert call(first=64, count=6) == 0


# ----------------------------------------------------------------------------- 3. scores
def _bn_stats(model):
    with torch.no_grad():              # non-trivial running statistics
        for m in model.dnn.mlp:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
    return model


def _criteo_model(seed=0):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.synthetic import schema_from_fields
    from deepfm_amd.models import create_model
    fields = IR.schema_fields("criteo")
    torch.manual_seed(seed)
    with torch.device(DEV):
        model = create_model("deepfm", schema_from_fields(fields), ExperimentConfig())
    return fields, _bn_stats(model)


@functools.lru_cache(maxsize=None)
def _predictor(kind):
    """(fields, predictor) of DeepFM through FusedPredictor / QuantizedPredictor or the MovieLens-shaped model through
    MixedSchemaPredictor; built once."""
    import deepfm_amd.training as T
    if kind == "mixed":
        from tests.test_gpu_mixed_predict import _movielens_model
        fields, model = _movielens_model("deepfm", seed=5)
        return fields, T.MixedSchemaPredictor(model, B)
    fields, model = _criteo_model()
    return fields, (T.FusedPredictor if kind == "fused" else T.QuantizedPredictor)(model, B)


def _host_scores(pred, recs, n, perm, mask):
    """Scores of the set with ``mask`` permuted: the restatement's records, uploaded, through ``predict_from``."""
    lay, out = pred.layout, []
    for first in range(0, n, B):
        count = min(B, n - first)
        rec = IR.permute_record(lay, recs, n, perm, mask, first, count)
        out.append(pred.predict_from(_upload(rec), count).view(-1))
    return torch.cat(out)


def _point(labels, scores):
    from deepfm_amd.training.metrics import metrics_device
    auc, logloss, npos, nneg, nan = metrics_device(labels, scores).cpu().tolist()
    assert nan == 0
    return [auc if (npos and nneg) else 0.0, logloss]


CHOICE = {"fused": (["C1", "I1", "I13"], {"C26+I2": ["C26", "I2"]}),
          "quant": (["C1", "C26", "I13"], {"all": None}),
          "mixed": (["user_id", "genres", "item_rating_count"], {"item": ["movie_id", "genres", "release_year_bucket"]})}


@pytest.mark.parametrize("n", IR.SIZES)
@pytest.mark.parametrize("kind", ["fused", "mixed", "quant"])
def test_every_variants_scores_equal_predict_from_over_host_built_records(kind, n):
    from deepfm_amd.training import FieldImportance
    fields, pred = _predictor(kind)
    singles, groups = CHOICE[kind]
    groups = {k: v or list(pred.layout.names) for k, v in groups.items()}
    cols = IR.columns_of(fields, n, 6)
    recs = IR.set_records(pred.layout, cols)
    R, seed = 2, 3
    fi = FieldImportance(pred)
    report = fi.run(cols, fields=singles, groups=groups, repeats=R, seed=seed, keep_scores=True)
    assert report.groups == singles + list(groups) and report.metrics == ["auc", "logloss"]
    assert report.values.shape == (len(report.groups), R, 2) and report.n == n and fi.scores.shape == (1 + len(report.groups) * R, n)
    labels = _upload(cols.labels)
    base = _host_scores(pred, recs, n, None, 0)
    assert torch.equal(fi.scores[0], base)
    assert report.baseline.tolist() == _point(labels, base)
    for g, label in enumerate(report.groups):
        mask = IR.mask_of(pred.layout, report.members[label])
        for r in range(R):
            want = _host_scores(pred, recs, n, IR.permutation(seed, r, n), mask)
            got = fi.scores[1 + g * R + r]
            assert torch.equal(got, want), (kind, n, label, r)
            assert report.values[g, r].tolist() == _point(labels, want), (kind, n, label, r)
            if n >= 64:
                assert not torch.equal(got, base), (label, r)           # the shuffle reached the model
    # without keep_scores: the same report from one reused buffer
    again = FieldImportance(pred).run(cols, fields=singles, groups=groups, repeats=R, seed=seed)
    assert again == report
    if n >= 8:
        assert pred.field_importance(cols, fields=singles, groups=groups, repeats=R, seed=seed + 1) != report


def _user_columns(fields, n, users, seed):
    """``IR.columns_of`` with ``user_id`` in runs of ragged length over ``users`` users."""
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.synthetic import random_fields_batch, schema_from_fields
    rng = np.random.default_rng([13, seed])
    feats = random_fields_batch(fields, n, rng, zero_frac=0.05)
    feats["user_id"] = np.sort(rng.integers(1, users + 1, n)).astype(np.int64)
    return PackedColumns(schema_from_fields(fields), feats, (rng.random(n) < 0.3).astype(np.float32))


def test_ranking_and_grouped_metrics_group_by_the_original_user_ids():
    from deepfm_amd.training import FieldImportance
    from deepfm_amd.training.metrics import grouped_auc_device, ranking_metrics_device
    fields, pred = _predictor("mixed")
    n, ks = 3 * B + 7, [1, 5]
    cols = _user_columns(fields, n, 20, 1)
    fi = FieldImportance(pred)
    report = fi.run(cols, fields=["user_id", "movie_id", "genres"], repeats=2, seed=9, ranking_ks=ks, group_auc=True,
                    keep_scores=True)
    assert report.metrics == ["auc", "logloss", "HR@1", "NDCG@1", "HR@5", "NDCG@5", "gauc", "uauc"]
    labels, uid = _upload(cols.labels), _upload(cols.ids[0])
    num_users = pred.model.schema.fields["user_id"].vocabulary_size

    def want(scores):
        rk = ranking_metrics_device(uid, labels, scores, ks, num_users).cpu().tolist()
        ga = grouped_auc_device(uid, labels, scores, num_users).cpu().tolist()
        assert rk[0] > 0 and ga[0] > 0
        return _point(labels, scores) + [rk[1], rk[3], rk[2], rk[4], ga[1], ga[2]]
    assert report.baseline.tolist() == want(fi.scores[0])
    recs = IR.set_records(pred.layout, cols)
    for g, label in enumerate(report.groups):
        for r in range(2):
            scores = _host_scores(pred, recs, n, IR.permutation(9, r, n), IR.mask_of(pred.layout, [label]))
            assert torch.equal(fi.scores[1 + g * 2 + r], scores)
            assert report.values[g, r].tolist() == want(scores), (label, r)     # user_id shuffled: grouped by the originals
    # the same through a record set built once, and the id column it hands out
    from deepfm_amd.training import RecordSet
    rs = RecordSet.from_columns(pred, cols)
    assert torch.equal(rs.ids("user_id"), uid) and torch.equal(rs.labels, labels) and len(rs) == n
    assert pred.field_importance(rs, fields=["user_id", "movie_id", "genres"], repeats=2, seed=9, ranking_ks=ks,
                                 group_auc=True) == report
    with pytest.raises(ValueError, match="more than max_bytes = 4096"):
        RecordSet.from_columns(pred, cols, max_bytes=4096)


def test_record_set_from_a_loader_with_sampled_negatives():
    import deepfm_amd.training as T
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, NegativeSampler
    from tests import ragged_reference as RR
    from tests.test_gpu_mixed_predict import _movielens_model
    from tests.test_gpu_trainer import _epoch_set, _ref_args
    P, K = 39, 4
    s = _epoch_set(P, seed=5)
    dcols = DeviceColumns(s.cols, DEV)
    src = NegativeSampler(dcols, s.seen, s.user_of, s.table, K, derived=s.derived, seed=9)
    loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=4, negatives=src)
    loader.set_epoch(1)
    assert loader.rows == P * (1 + K) == 3 * B + 3
    _, model = _movielens_model("deepfm", fields=s.fields, seed=5)
    pred = T.MixedSchemaPredictor(model, B)
    roles, derived = _ref_args(src, s.derived)
    rows = RR.virtual_rows(s.cols, np.arange(P + 1, dtype=np.int64) * K, loader.negatives_host(1).reshape(-1), s.items,
                           roles, derived)
    host_cols = RR.take(rows, loader.order.cpu().numpy())
    a, b = T.RecordSet.from_loader(pred, loader), T.RecordSet.from_columns(pred, host_cols)
    assert a.n == b.n == loader.rows and torch.equal(a.records, b.records)
    kw = dict(fields=["user_id", "movie_id", "genres", "movie_age_at_rating"], repeats=2, seed=1, ranking_ks=[1, 5],
              group_auc=True)
    want = pred.field_importance(host_cols, **kw)
    assert pred.field_importance(loader, **kw) == want and pred.field_importance(a, **kw) == want
    assert "HR@5" in want.metrics and "gauc" in want.metrics and not np.isnan(want.values).any()


# ----------------------------------------------------------------------------- 4. meaning
MEANING_FIELDS = [dict(name="A", type="sparse", vocab=50, dim=16, max_len=1, combiner="mean"),
                  dict(name="Z", type="sparse", vocab=50, dim=16, max_len=1, combiner="mean"),
                  dict(name="C", type="sparse", vocab=30, dim=16, max_len=1, combiner="mean"),
                  dict(name="X", type="dense", vocab=0, dim=16, max_len=1, combiner="mean")]
MEANING_SEED = 0


def meaning_model(device):
    """A small DeepFM in which Z does nothing (both its tables zero) and A decides: its first-order weight is +4 for
    an odd id and -4 for an even one."""
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.synthetic import schema_from_fields
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim, cfg.dnn.hidden_units = 16, [32, 16]
    torch.manual_seed(MEANING_SEED)
    model = create_model("deepfm", schema_from_fields(MEANING_FIELDS), cfg).to(device)
    emb = model.embedding
    with torch.no_grad():
        emb.second_order_embeddings["Z"].weight.zero_()
        emb.first_order_embeddings["Z"].weight.zero_()
        ids = torch.arange(50, device=device)
        emb.first_order_embeddings["A"].weight[:, 0] = torch.where(ids % 2 == 1, 4.0, -4.0)
    return cfg, model


def meaning_columns(n):
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.synthetic import random_fields_batch, schema_from_fields
    rng = np.random.default_rng(MEANING_SEED)
    feats = random_fields_batch(MEANING_FIELDS, n, rng, zero_frac=0.0)
    return PackedColumns(schema_from_fields(MEANING_FIELDS), feats, (feats["A"] % 2).astype(np.float32))


def test_importance_means_what_it_says():
    from oracle import ctr_oracle as O
    from deepfm_amd.training import FusedPredictor
    n = 13 * B + 7
    cfg, model = meaning_model(DEV)
    cols = meaning_columns(n)
    # the numpy oracle, on the CPU: the baseline separates the classes
    sd = {k: npy(v) for k, v in model.state_dict().items()}
    batch = {"A": cols.ids[0], "Z": cols.ids[1], "C": cols.ids[2], "X": cols.dense[0]}
    logits = np.asarray(O.model_logits("deepfm", MEANING_FIELDS, sd, batch, dict(fm_dim=16, hidden_units=[32, 16]),
                                       training=False)).reshape(-1)
    pos = cols.labels == 1
    assert pos.any() and (~pos).any() and logits[pos].min() > 0 > logits[~pos].max()
    pred = FusedPredictor(model, B)
    report = pred.field_importance(cols, groups={"A+Z": ["A", "Z"]}, repeats=3, seed=MEANING_SEED)
    assert report.groups == ["A", "Z", "C", "X", "A+Z"]
    a, z = report.groups.index("A"), report.groups.index("Z")
    assert report.baseline[0] == 1.0
    assert (report.delta[z] == 0.0).all()                       # every metric, every repeat, exactly
    assert report.ranking("logloss")[0] == "A" and report.ranking("auc")[0] == "A"
    # 0.5 in expectation, standard deviation about 0.02 at this n: a bound on chance, not on arithmetic
    assert ((report.values[a, :, 0] >= 0.4) & (report.values[a, :, 0] <= 0.6)).all(), report.values[a, :, 0]
    for m in report.metrics:
        assert report.interaction("A", "Z", m) == 0.0
        assert (report.interaction("A", "Z", m, per_repeat=True) == 0.0).all()
    with pytest.raises(KeyError, match="C"):
        report.interaction("A", "C", "auc")


# ----------------------------------------------------------------------------- 5. determinism and isolation
def test_runs_repeat_and_leave_the_predictor_as_it_was():
    from deepfm_amd.training import Calibrator, FieldImportance, FusedPredictor
    fields, model = _criteo_model(seed=2)
    with torch.no_grad():
        for p in model.parameters():                       # logits with some spread
            p.mul_(3.0)
    n = 3 * B + 7
    cols = IR.columns_of(fields, n, 8)
    raw = FusedPredictor(model, B)
    labels, logits = raw.collect_logits(cols)
    cal = Calibrator("platt").fit(labels, logits)
    pred = FusedPredictor(model, B, calibrator=cal)
    before = pred.evaluate(cols)
    kept, kept_scores = pred.last_scores, pred.last_scores.clone()
    params, slots = cal.params.clone(), list(pred.slots)
    kw = dict(fields=["C1", "I1"], repeats=2, seed=4)
    fi = FieldImportance(pred)
    one = fi.run(cols, keep_scores=True, **kw)
    two = pred.field_importance(cols, **kw)
    assert one == two and np.array_equal(one.values, two.values)
    assert pred.last_scores is kept and torch.equal(kept, kept_scores)
    assert pred.calibrator is cal and torch.equal(cal.params, params)
    assert len(pred.slots) == len(slots) and all(a is b for a, b in zip(pred.slots, slots))
    assert pred.evaluate(cols) == before and torch.equal(pred.last_scores, kept_scores)
    # calibrated probabilities are what is scored
    assert torch.equal(fi.scores[0], kept_scores) and torch.equal(kept_scores, cal.apply(logits))
    assert one.baseline.tolist() == [before["auc"], before["logloss"]]
    raw_report = raw.field_importance(cols, **kw)
    assert raw_report.baseline[1] != one.baseline[1]
    recs = IR.set_records(pred.layout, cols)
    want = _host_scores(pred, recs, n, IR.permutation(4, 1, n), IR.mask_of(pred.layout, ["I1"]))
    assert torch.equal(fi.scores[1 + 1 * 2 + 1], want)


# ----------------------------------------------------------------------------- 6. the Trainer
def test_trainer_writes_the_report_of_every_field(tmp_path):
    import deepfm_amd.training as T
    from tests.test_gpu_trainer import _trainer_config, _trainer_data, _trainer_model
    cfg = _trainer_config(tmp_path / "run", num_epochs=2)
    schema, (train, val, test) = _trainer_data(cfg)
    trainer = T.Trainer(_trainer_model(schema, cfg), schema, cfg, train, val, test, importance=2)
    trainer.train()
    with open(tmp_path / "run" / "results.json") as f:
        res = json.load(f)
    got = res["field_importance"]
    assert list(got["groups"]) == list(schema.fields) and got["repeats"] == 2 and got["n"] == test.rows
    assert got["metrics"] == ["auc", "logloss"] + [f"{kind}@{k}" for k in (1, 5, 10) for kind in ("HR", "NDCG")]
    assert got == trainer.importance_report.to_dict()
    # a direct call on the trained weights, in a model and a predictor of their own
    fresh = _trainer_model(schema, cfg).cuda()
    fresh.load_state_dict(trainer.model.state_dict())
    direct = T.MixedSchemaPredictor(fresh, cfg.training.batch_size).field_importance(
        test, repeats=2, seed=cfg.seed, ranking_ks=cfg.training.ranking_ks)
    assert json.loads(json.dumps(direct.to_dict(), allow_nan=False)) == got
    assert direct == trainer.importance_report
    # off: no such key
    cfg0 = _trainer_config(tmp_path / "off", num_epochs=1)
    schema0, (train0, val0, test0) = _trainer_data(cfg0)
    off = T.Trainer(_trainer_model(schema0, cfg0), schema0, cfg0, train0, val0, test0)
    assert off.importance == 0
    off.train()
    with open(tmp_path / "off" / "results.json") as f:
        assert sorted(json.load(f)) == ["config", "run_id", "test_metrics", "timestamp", "training_info", "val_metrics"]
