"""GPU: every caller of the evaluation unit (``training/metrics.py:enqueue_evaluation``) gives the same numbers, bit
for bit: ``evaluate`` and ``evaluate_loader`` with every family on equal each other and the union of the stand-alone
``compute_*`` functions on the scores they scored; the field importance's baseline is those values; with everything off
the dict is ``auc`` and ``logloss`` alone.  Both sides are the same integer sums and fixed-order fp64 sums, so no
comparison needs a tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, B, USERS, KS, BINS, REPLICATES, SEED = 150, 64, 7, [1, 3], 4, 17, 3


@pytest.fixture(scope="module")
def case():
    """A small DeepFM on the MovieLens schema over two whole batches and a trailing one of 22: 7 users, one with
    negatives only, one with positives only, two with a pair of rows alike (tied scores, one of each class)."""
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import MixedSchemaPredictor
    from tests.helpers import random_fields_batch
    from tests.test_gpu_mixed_predict import _movielens_model
    fields, model = _movielens_model("deepfm", seed=5)
    rng = np.random.default_rng(21)
    feats = random_fields_batch(fields, N, rng, zero_frac=0.05)
    uid = (np.arange(N) % USERS + 1).astype(np.int64)
    feats["user_id"] = uid
    labels = (rng.random(N) < 0.4).astype(np.float32)
    labels[uid == 2], labels[uid == 5] = 0.0, 1.0
    for user in (3, 6):
        a, b = np.flatnonzero(uid == user)[[1, 4]]
        for column in feats.values():
            column[b] = column[a]
        labels[a], labels[b] = 1.0, 0.0
    cols = PackedColumns(model.schema, feats, labels)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    assert N // B == 2 and N % B == 22
    return MixedSchemaPredictor(model, B), cols, loader, uid


EVERYTHING = dict(ranking_ks=KS, group_auc=True, calibration_bins=BINS, slice_field="user_id", bootstrap=REPLICATES,
                  bootstrap_by="user_id", bootstrap_seed=SEED, bootstrap_grouped=True)


def test_every_caller_gives_the_same_numbers(case):
    from deepfm_amd.training import (compute_auc, compute_bootstrap, compute_bootstrap_ranking, compute_calibration,
                                     compute_gauc, compute_logloss, compute_ranking_metrics)
    pred, cols, loader, uid = case
    m = pred.evaluate(cols, **EVERYTHING)
    for k, v in m.items():
        print(k, float(v).hex())
    y, s = pred.last_labels.clone(), pred.last_scores.clone()
    from_loader = pred.evaluate_loader(loader, **EVERYTHING)
    assert list(m) == list(from_loader) and m == from_loader                                    # 1: both sources
    assert torch.equal(s, pred.last_scores) and torch.equal(y, pred.last_labels)
    # the tied pairs are tied, and the two one-class users are what they should be
    host_s, host_y = s.cpu().numpy(), y.cpu().numpy()
    for user in (3, 6):
        a, b = np.flatnonzero(uid == user)[[1, 4]]
        assert host_s[a] == host_s[b] and (host_y[a], host_y[b]) == (1.0, 0.0)
    assert not host_y[uid == 2].any() and host_y[uid == 5].all()
    # 2: the union of the stand-alone functions on those scores, the user column and the same seed
    users = pred.model.schema.fields["user_id"].vocabulary_size
    d_uid = torch.from_numpy(uid).cuda()
    pooled = compute_bootstrap(y, s, REPLICATES, SEED, unit_ids=d_uid)
    grouped = compute_bootstrap_ranking(d_uid, y, s, KS, REPLICATES, SEED, users, group_auc=True)
    calibration = compute_calibration(y, s, BINS, d_uid, users)
    want = {"auc": compute_auc(y, s), "logloss": compute_logloss(y, s),
            **compute_ranking_metrics(d_uid, y, s, KS, users), **compute_gauc(d_uid, y, s, users),
            **{k: v for k, v in calibration.items() if k not in ("reliability", "slices")},
            **{k: v for k, v in pooled.items() if k not in ("auc", "logloss")},
            **{k: v for k, v in grouped.items() if "_" in k}}
    assert list(m) == list(want) and m == want
    assert (pooled["auc"], pooled["logloss"]) == (m["auc"], m["logloss"])
    per_user = ["HR@1", "NDCG@1", "HR@3", "NDCG@3", "gauc", "uauc"]
    assert [k for k in grouped if "_" not in k] == per_user and all(grouped[k] == m[k] for k in per_user)
    assert m["HR@3_replicates"] <= REPLICATES and m["auc_replicates"] <= REPLICATES and len(m) == 2 + 4 + 2 + 7 + 8 + 24
    table = pred.last_calibration["slices"].cpu().numpy()
    assert np.array_equal(table[:, 0], np.bincount(uid, minlength=users)) and pred.last_calibration["bins"].shape == (4, 3)
    # 3: the field importance's baseline is the evaluation of the unpermuted set
    report = pred.field_importance(cols, fields=["user_id"], ranking_ks=KS, group_auc=True, repeats=1)
    assert report.metrics == ["auc", "logloss", "HR@1", "NDCG@1", "HR@3", "NDCG@3", "gauc", "uauc"]
    assert report.baseline.tolist() == [m[name] for name in report.metrics]
    assert report.values.shape == (1, 1, 8) and not np.isnan(report.values).any()


def test_everything_off_gives_auc_and_logloss_alone(case):
    pred, cols, loader, _ = case
    m = pred.evaluate(cols)
    assert list(m) == ["auc", "logloss"] and m == pred.evaluate_loader(loader)                  # 4
    assert 0.0 < m["auc"] < 1.0 and m["logloss"] > 0.0
