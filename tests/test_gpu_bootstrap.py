"""GPU: the Poisson bootstrap (csrc/bootstrap.hip) against the numpy restatement (tests/bootstrap_reference.py), bit for
bit: the five integers and the two quotients of every replicate, at the edges of the chunk and of the replicate block,
over tied, constant, signed-zero and infinite scores, faulty samples and unit ids; independence of the sample order;
pairing under one seed; through ``compute_bootstrap`` / ``compare_bootstrap``, the predictors and the Trainer."""
import json

import numpy as np
import pytest
import torch

from tests import bootstrap_reference as BR

pytestmark = pytest.mark.gpu

KEYS = [f"{m}_{k}" for m in ("auc", "logloss") for k in ("se", "lo", "hi", "replicates")]
FAMILIES = ["continuous", "tenths", "equal", "run", "zeros", "inf"]


def _chunk():
    from deepfm_amd import _lib
    return _lib.BOOTSTRAP_CHUNK


def _block():
    from deepfm_amd import _lib
    return _lib.BOOTSTRAP_REPLICATE_BLOCK


def _scores(rng, n, family):
    s = rng.standard_normal(n).astype(np.float32)
    if family == "tenths":
        s = np.round(s, 1).astype(np.float32)
    elif family == "equal":
        s[:] = 0.25
    elif family == "run":
        # one constant run of the sorted order, laid across the first chunk boundary where there is one
        C = _chunk()
        s = np.sort(s)
        mid = C if n > C else n // 2
        a, b = max(0, mid - 40), min(n, mid + 40)
        s[a:b] = s[a]
        s = s[rng.permutation(n)]
    elif family == "zeros":
        s[::3] = 0.0
        s[1::3] = -0.0
    elif family == "inf":
        s[::5] = np.inf
        s[2::7] = -np.inf
    return s


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))      # == on the doubles


def _check(labels, scores, replicates, seed=0, unit_ids=None, what=""):
    """One device call against the restatement, bit for bit; returns (counts, values, faults) on the host."""
    from deepfm_amd.training import bootstrap_device
    uid = None if unit_ids is None else torch.from_numpy(np.asarray(unit_ids, np.int64)).cuda()
    counts, values, faults = bootstrap_device(torch.from_numpy(labels).cuda(), torch.from_numpy(scores).cuda(),
                                              replicates, seed, uid)
    counts, values, faults = counts.cpu().numpy(), values.cpu().numpy(), faults.cpu().numpy()
    want = BR.bootstrap(labels, scores, replicates, seed, unit_ids)
    assert counts.shape == (replicates, 5) and values.shape == (replicates, 2), what
    assert np.array_equal(faults, want["faults"]), (what, faults, want["faults"])
    bad = np.flatnonzero((counts != want["counts"]).any(axis=1))
    assert bad.size == 0, f"{what}: replicate {bad[0]}: {counts[bad[0]]} != {want['counts'][bad[0]]}"
    assert _same(values, want["values"]), what
    return counts, values, faults


def _sizes():
    C = _chunk()
    return [1, 2, 63, 64, 65, C - 1, C, C + 1, 3 * C + 7]


@pytest.mark.parametrize("k", range(9))
def test_counts_and_values_match_the_restatement(k):
    """Every n at an edge of the wave and of the chunk, crossed with the replicates around a replicate block and with
    every score family."""
    n, RB = _sizes()[k], _block()
    rng = np.random.default_rng(100 + k)
    for family in FAMILIES:
        y = (rng.random(n) < 0.4).astype(np.float32)
        s = _scores(rng, n, family)
        for R in (1, RB - 1, RB, RB + 1):
            _check(y, s, R, seed=k, what=f"n {n} R {R} {family}")


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_one_class_has_no_auc_and_a_log_loss(label):
    n, R = _chunk() + 1, _block() + 1
    rng = np.random.default_rng(7)
    s = rng.random(n).astype(np.float32)
    counts, values, _ = _check(np.full(n, label, np.float32), s, R, seed=3)
    assert np.isnan(values[:, 0]).all() and np.isfinite(values[:, 1]).all() and (counts[:, 0] == 0).all()
    assert (counts[:, 1 if label else 2] == counts[:, 4]).all() and (counts[:, 4] > 0).all()


def test_faulty_samples_are_counted_and_skipped():
    """NaN scores, labels 0.5 and 2 and unit ids -1 and 2^40, each in the first, a middle and the last chunk of the
    input; the clean samples give what they give alone."""
    C, R = _chunk(), _block() + 1
    n = 3 * C + 7
    rng = np.random.default_rng(8)
    y = (rng.random(n) < 0.4).astype(np.float32)
    s = np.round(rng.standard_normal(n), 1).astype(np.float32)
    u = rng.integers(0, 500, n)
    at = np.array([5, C + 11, 3 * C + 1])
    s[at] = np.nan
    y[at + 1] = 0.5
    y[at + 2] = 2.0
    u[at + 3] = -1
    u[at + 4] = 1 << 40
    counts, values, faults = _check(y, s, R, seed=1, unit_ids=u, what="faults, units")
    assert faults.tolist() == [3, 6, 6]
    clean = np.ones(n, bool)
    clean[(at[:, None] + np.arange(5)).reshape(-1)] = False
    alone = BR.bootstrap(y[clean], s[clean], R, 1, u[clean])
    assert np.array_equal(counts, alone["counts"]) and _same(values, alone["values"])
    # without unit ids the unit is the position: the two bad ids are not looked at
    _, _, faults = _check(y, s, R, seed=1, what="faults, positions")
    assert faults.tolist() == [3, 6, 0]
    # the summaries refuse each fault with its words
    from deepfm_amd.training import compute_bootstrap
    d = (torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(u).cuda())
    with pytest.raises(ValueError, match=r"^Input contains NaN\.$"):
        compute_bootstrap(d[0], d[1], 3, unit_ids=d[2])
    s[at] = 0.5
    with pytest.raises(ValueError, match=r"^6 labels other than 0 and 1$"):
        compute_bootstrap(y, torch.from_numpy(s).cuda(), 3, unit_ids=u)
    y[at + 1] = y[at + 2] = 1.0
    with pytest.raises(ValueError, match=r"^6 unit ids outside \[0, 2\^40\)$"):
        compute_bootstrap(y, torch.from_numpy(s).cuda(), 3, unit_ids=u)


@pytest.mark.parametrize("units", ["seven", "one", "high"])
def test_unit_ids(units):
    C, R = _chunk(), _block() + 1
    n = 3 * C + 7
    rng = np.random.default_rng(9)
    y = (rng.random(n) < 0.4).astype(np.float32)
    s = np.round(rng.standard_normal(n), 1).astype(np.float32)
    if units == "seven":
        u = rng.integers(0, 7, n)
    elif units == "one":
        u = np.full(n, 12345)
    else:
        u = (1 << 40) - 1 - rng.integers(0, 50, n)
    counts, values, _ = _check(y, s, R, seed=4, unit_ids=u, what=units)
    if units == "one":
        # every weight of a replicate is the same: the quotients are the point estimates or NaN
        w = np.array([BR.weights(4, r, np.array([12345]))[0] for r in range(R)])
        P, N = int((y == 1).sum()), int((y == 0).sum())
        assert np.array_equal(counts[:, 1], w * P) and np.array_equal(counts[:, 2], w * N)
        live = w > 0
        assert live.any() and np.isnan(values[~live]).all() and np.unique(values[live, 0]).size == 1


def test_the_order_of_the_samples_does_not_matter():
    C, R = _chunk(), _block() + 1
    n = 3 * C + 7
    rng = np.random.default_rng(10)
    y = (rng.random(n) < 0.4).astype(np.float32)
    s = np.round(rng.standard_normal(n), 1).astype(np.float32)
    u = rng.integers(0, 300, n)
    counts, values, _ = _check(y, s, R, seed=5, unit_ids=u)
    p = rng.permutation(n)
    counts_p, values_p, _ = _check(y[p], s[p], R, seed=5, unit_ids=u[p])
    assert np.array_equal(counts, counts_p) and _same(values, values_p)


def test_one_seed_resamples_alike_and_another_differently():
    from deepfm_amd.training import compare_bootstrap
    C, R = _chunk(), 2 * _block()
    n = C + 300
    rng = np.random.default_rng(11)
    y = (rng.random(n) < 0.4).astype(np.float32)
    sa = rng.random(n).astype(np.float32)
    sb = np.clip(sa + 0.2 * (y - 0.5) * rng.random(n), 0, 1).astype(np.float32)        # b is the better scorer
    u = rng.integers(0, 200, n)
    a, va, _ = _check(y, sa, R, seed=6, unit_ids=u)
    b, vb, _ = _check(y, sb, R, seed=6, unit_ids=u)
    assert np.array_equal(a[:, [1, 2, 4]], b[:, [1, 2, 4]]) and not np.array_equal(a[:, 0], b[:, 0])
    other, _, _ = _check(y, sa, R, seed=7, unit_ids=u)
    assert not np.array_equal(a[:, [1, 2, 4]], other[:, [1, 2, 4]])
    same = compare_bootstrap(y, sa, sa, R, seed=6, unit_ids=u)
    assert list(same) == [f"{m}_{k}" for m in ("auc", "logloss")
                          for k in ("a", "b", "delta", "delta_se", "delta_lo", "delta_hi", "b_better")]
    for m in ("auc", "logloss"):
        assert same[f"{m}_a"] == same[f"{m}_b"]
        assert [same[f"{m}_delta{k}"] for k in ("", "_se", "_lo", "_hi")] == [0.0] * 4 and same[f"{m}_b_better"] == 0.0
    d = compare_bootstrap(y, sa, sb, R, seed=6, unit_ids=u)
    delta, q = vb - va, (1 - 0.95) / 2
    assert d["auc_delta_se"] == np.std(delta[:, 0], ddof=1) and d["auc_delta_lo"] == np.quantile(delta[:, 0], q)
    assert d["logloss_delta_hi"] == np.quantile(delta[:, 1], 1 - q)
    assert d["auc_b_better"] == np.mean(delta[:, 0] > 0) == 1.0 and d["logloss_b_better"] == np.mean(delta[:, 1] < 0)
    assert d["auc_delta"] == d["auc_b"] - d["auc_a"] > 0 and d["auc_delta_lo"] > 0


def test_compute_bootstrap_is_the_point_and_the_spread_of_the_replicates():
    from deepfm_amd.training import compute_auc, compute_bootstrap, compute_logloss
    n, R = 3000, 70
    rng = np.random.default_rng(12)
    y = (rng.random(n) < 0.3).astype(np.float32)
    s = (1 / (1 + np.exp(-(rng.standard_normal(n) + y)))).astype(np.float32)
    u = rng.integers(0, 150, n)
    for unit_ids, level in ((None, 0.95), (u, 0.8)):
        d = compute_bootstrap(y, s, R, seed=2, unit_ids=unit_ids, level=level)
        assert list(d) == ["auc", "logloss"] + KEYS and all(type(d[k]) is float for k in d if "replicates" not in k)
        assert d["auc"] == compute_auc(y, s) and d["logloss"] == compute_logloss(y, s)
        want = BR.summary(BR.bootstrap(y, s, R, 2, unit_ids)["values"], level)
        assert {k: d[k] for k in KEYS} == want
        assert d["auc_lo"] < d["auc"] < d["auc_hi"] and d["logloss_lo"] < d["logloss"] < d["logloss_hi"]


def test_mid_size_case():
    """The only case above toy size: 98 chunks, two replicate blocks and one replicate."""
    n, R = 200_003, 2 * _block() + 1
    rng = np.random.default_rng(13)
    y = (rng.random(n) < 0.2).astype(np.float32)
    s = (1 / (1 + np.exp(-(rng.standard_normal(n) + y)))).astype(np.float32)
    s[::4] = np.round(s[::4], 2)
    _check(y, s, R, seed=99, unit_ids=rng.integers(0, 5000, n), what="mid size")


def test_more_chunks_than_one_tile_of_the_offset_scan():
    """The scan of the chunk totals walks a row 256 chunks at a time and carries the sum over: 257 chunks is the
    smallest input at which the carry is used (two replicates keep the restatement quick)."""
    n = 256 * _chunk() + 5
    rng = np.random.default_rng(14)
    y = (rng.random(n) < 0.5).astype(np.float32)
    s = np.round(rng.standard_normal(n), 2).astype(np.float32)
    _check(y, s, 2, seed=21, what="257 chunks")


# ----------------------------------------------------------------------------- the predictors
def _check_predictor(pred, cols, uid, loader, ks, slice_field):
    from deepfm_amd.training import compute_bootstrap
    for how in ("evaluate", "evaluate_loader"):
        run = (lambda **kw: pred.evaluate(cols, **kw)) if how == "evaluate" else \
            (lambda **kw: pred.evaluate_loader(loader, **kw))
        plain, again = run(ranking_ks=ks, group_auc=True), run(ranking_ks=ks, group_auc=True)
        assert list(plain) == list(again) and all(plain[k] == again[k] for k in plain), how
        assert list(plain)[:2] == ["auc", "logloss"] and list(plain)[-2:] == ["gauc", "uauc"], how
        assert not any(k in plain for k in KEYS), how
        m = run(ranking_ks=ks, group_auc=True, bootstrap=70, bootstrap_by="user_id")
        assert list(m) == list(plain) + KEYS and {k: m[k] for k in plain} == plain, how
        want = compute_bootstrap(pred.last_labels, pred.last_scores, 70, unit_ids=torch.from_numpy(uid).cuda())
        assert {k: m[k] for k in KEYS} == {k: want[k] for k in KEYS}, how
        assert (m["auc"], m["logloss"]) == (want["auc"], want["logloss"]) and 0 < m["auc_lo"] < m["auc_hi"] < 1
        ref = BR.summary(BR.bootstrap(pred.last_labels.cpu().numpy(), pred.last_scores.cpu().numpy(), 70, 0, uid)["values"])
        assert {k: m[k] for k in KEYS} == ref, how
        # by sample, another seed, and next to the calibration numbers
        m = run(bootstrap=33, bootstrap_seed=5, calibration_bins=10)
        want = compute_bootstrap(pred.last_labels, pred.last_scores, 33, seed=5)
        assert list(m)[-8:] == KEYS and {k: m[k] for k in KEYS} == {k: want[k] for k in KEYS}, how
        # all five families in one call and one host read: every key is the single-family call's, bit for bit
        full = run(ranking_ks=ks, group_auc=True, calibration_bins=10, slice_field=slice_field, bootstrap=33,
                   bootstrap_by="user_id")
        table = pred.last_calibration["slices"].clone()
        singles = [run(ranking_ks=ks), run(group_auc=True), run(calibration_bins=10, slice_field=slice_field),
                   run(bootstrap=33, bootstrap_by="user_id")]
        assert all(list(one)[:2] == ["auc", "logloss"] and len(one) > 2 for one in singles), how
        assert list(full) == ["auc", "logloss"] + [k for one in singles for k in list(one)[2:]], how
        for one in singles:
            assert {k: full[k] for k in one} == one, how                      # == on floats
        assert torch.equal(table, pred.last_calibration["slices"]), how      # the single calibration call's table
    with pytest.raises(ValueError, match="bootstrap_by 'visitor' is not a SPARSE field of the schema"):
        pred.evaluate(cols, bootstrap=10, bootstrap_by="visitor")
    with pytest.raises(ValueError, match="it needs bootstrap"):
        pred.evaluate_loader(loader, bootstrap_by="user_id")
    with pytest.raises(ValueError, match="bootstrap = 65537"):
        pred.evaluate(cols, bootstrap=65537)


def test_mixed_predictor_adds_the_intervals():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.schema import FeatureType
    from deepfm_amd.training import MixedSchemaPredictor
    from tests.helpers import random_fields_batch
    from tests.test_gpu_mixed_predict import _movielens_model
    fields, model = _movielens_model("deepfm", seed=5)
    U, C, B = 60, 50, 512
    n = U * C
    rng = np.random.default_rng(13)
    feats = random_fields_batch(fields, n, rng, zero_frac=0.05)
    feats["user_id"] = np.repeat(np.arange(1, U + 1, dtype=np.int64), C)
    labels = (rng.random(n) < 0.2).astype(np.float32)
    cols = PackedColumns(model.schema, feats, labels)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    kinds = {nm: sp.feature_type for nm, sp in model.schema.fields.items()}
    slice_field = next(nm for nm, k in kinds.items() if k is FeatureType.SPARSE and nm != "user_id")
    _check_predictor(MixedSchemaPredictor(model, B), cols, feats["user_id"], loader, [1, 5, 10], slice_field)


def test_uniform_predictor_adds_the_intervals():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FusedPredictor
    from tests.test_gpu_ranking import _user_model
    model = _user_model()
    users, cands, B = 90, 40, 512
    rng = np.random.default_rng(11)
    uid = np.repeat(np.arange(users, dtype=np.int64) * 7, cands)
    y = (rng.random(uid.size) < 0.25).astype(np.float32)
    feats = {"user_id": uid, "item_id": rng.integers(0, 5000, uid.size), "genre": rng.integers(0, 20, uid.size),
             "age": rng.random(uid.size).astype(np.float32)}
    cols = PackedColumns(model.schema, feats, y)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    _check_predictor(FusedPredictor(model, B), cols, uid, loader, [1, 5], "genre")


# ----------------------------------------------------------------------------- the Trainer
def test_trainer_reports_the_intervals_of_the_test_split_only(tmp_path):
    import deepfm_amd.training as T
    from tests.test_gpu_trainer import _trainer_config, _trainer_data, _trainer_model
    cfg = _trainer_config(tmp_path / "run", num_epochs=1)
    schema, (train, val, test) = _trainer_data(cfg)
    trainer = T.Trainer(_trainer_model(schema, cfg), schema, cfg, train, val, test, bootstrap=40)
    got = trainer.train()
    with open(tmp_path / "run" / "results.json") as f:
        res = json.load(f)
    assert res["val_metrics"] == got and not set(KEYS) & set(got)
    m = res["test_metrics"]
    assert set(KEYS) <= set(m) and m["auc_replicates"] == m["logloss_replicates"] == 40
    assert 0 < m["auc_lo"] < m["auc_hi"] <= 1 and 0 < m["logloss_lo"] < m["logloss_hi"] and m["auc_se"] > 0
