"""GPU: on-device HR@k / NDCG@k (csrc/ranking.hip) against the reference's fixture, the numpy restatement of the
stable-tie contract (tests/test_cpu_ranking.py), on contiguous and interleaved layouts, and through
FusedPredictor.evaluate."""
import json

import numpy as np
import pytest
import torch

from tests.helpers import schema_from_fields
from tests.test_cpu_ranking import (assert_ranking_equal, fixture_cases, load_case, per_user_lists,
                                    stable_ranking)

pytestmark = pytest.mark.gpu

KS = [1, 5, 10, 20]


@pytest.mark.parametrize("case", fixture_cases()[1])
def test_reference_fixture(case):
    from deepfm_amd.training import RankingEvaluator, compute_ranking_metrics
    g, _ = fixture_cases()
    uid, y, s, ks = load_case(g, case)
    trainer = json.loads(str(g[f"{case}/trainer"]))
    evaluator = json.loads(str(g[f"{case}/evaluator"]))
    assert_ranking_equal(compute_ranking_metrics(uid, y, s, ks), trainer, f"{case} numpy")
    d_uid, d_y, d_s = (torch.from_numpy(x).cuda() for x in (uid, y, s))
    got = compute_ranking_metrics(d_uid, d_y, d_s, ks, num_users=int(uid.max()) + 1000)
    assert_ranking_equal(got, trainer, f"{case} device")
    assert all(type(v) is float for v in got.values())
    gs, gl = per_user_lists(uid, s, y)
    assert_ranking_equal(RankingEvaluator(ks).evaluate(gs, gl), evaluator, f"{case} evaluator")


def _tied_split(rng, lengths, contiguous, pos_rate=0.1):
    """Users of the given candidate counts; scores on a 1/16 grid (many exact ties, -0.0 among them); one positive
    per user at least where the user has two samples or more, more at ``pos_rate``."""
    uid = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    n = uid.size
    s = (np.floor(rng.random(n) * 16) / 16).astype(np.float32)
    s[rng.random(n) < 0.05] = -0.0
    y = (rng.random(n) < pos_rate).astype(np.float32)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    y[starts + (rng.random(len(lengths)) * lengths).astype(np.int64)] = 1.0
    if not contiguous:
        p = rng.permutation(n)
        uid, y, s = uid[p], y[p], s[p]
    return uid, y, s


# runs of 63 / 64 / 65 (a wave) and 255 / 256 / 257 (a workgroup) straddle both boundaries at every offset;
# 1000 candidates: the leave-one-out shape; 1 and 2: single-sample and tiny users
_LENGTHS = [63, 64, 65, 1, 255, 256, 257, 2, 1000, 3, 100, 129, 513, 1, 7] * 40


@pytest.mark.parametrize("contiguous", [True, False])
def test_ties_follow_the_stable_order(contiguous):
    from deepfm_amd.training import compute_ranking_metrics, ranking_metrics_device
    from deepfm_amd.training.metrics import ranking_dict
    rng = np.random.default_rng(7 if contiguous else 8)
    uid, y, s = _tied_split(rng, _LENGTHS, contiguous)
    ks = [1, 2, 5, 10, 64, 100, 257, 1000]
    want = stable_ranking(uid, y, s, ks)
    assert want
    assert_ranking_equal(compute_ranking_metrics(uid, y, s, ks), want, "filtered")
    d = [torch.from_numpy(x).cuda() for x in (uid, y, s)]
    for both in (True, False):
        first = ranking_metrics_device(*d, ks, require_both_classes=both)
        second = ranking_metrics_device(*d, ks, require_both_classes=both)
        assert torch.equal(first, second)                           # bitwise reproducible
        assert_ranking_equal(ranking_dict(first.cpu().tolist(), ks),
                             stable_ranking(uid, y, s, ks, require_both_classes=both), f"both={both}")


@pytest.mark.parametrize("users,cands", [(943, 1000), (20_000, 100)])
def test_leave_one_out_layouts(users, cands):
    """One positive per user, tied scores: the contiguous layout (a wave holds one or two users) and the shuffled
    one (per-lane atomics) each give the restatement's values for their own dataset order."""
    from deepfm_amd.training import compute_ranking_metrics
    rng = np.random.default_rng(users)
    uid, y, s = _tied_split(rng, [cands] * users, True, pos_rate=0.0)
    p = rng.permutation(uid.size)
    assert_ranking_equal(compute_ranking_metrics(uid, y, s, KS), stable_ranking(uid, y, s, KS), "contiguous")
    assert_ranking_equal(compute_ranking_metrics(uid[p], y[p], s[p], KS), stable_ranking(uid[p], y[p], s[p], KS),
                         "shuffled")


def test_no_qualifying_user_gives_no_keys():
    from deepfm_amd.training import RankingEvaluator, compute_ranking_metrics
    uid = np.repeat(np.arange(50), 10)
    y = (uid % 2).astype(np.float32)                  # every user single-class
    s = np.random.default_rng(0).random(uid.size).astype(np.float32)
    assert compute_ranking_metrics(uid, y, s, KS) == {}
    got = RankingEvaluator(KS).evaluate([s[:10], s[10:20], np.zeros(0, np.float32)],
                                        [y[:10], y[10:20], np.zeros(0, np.float32)])
    assert got == {"HR@1": 1 / 3, "NDCG@1": 1 / 3, "HR@5": 1 / 3, "NDCG@5": 1 / 3, "HR@10": 1 / 3,
                   "NDCG@10": 1 / 3, "HR@20": 1 / 3, "NDCG@20": 1 / 3}
    assert list(RankingEvaluator().evaluate([s[:10]], [y[:10]])) == ["HR@5", "NDCG@5", "HR@10", "NDCG@10",
                                                                    "HR@20", "NDCG@20"]


@pytest.mark.parametrize("bad", ["nan", "id_high", "id_negative", "label_half", "k0", "ks9", "empty"])
def test_bad_inputs_raise(bad):
    from deepfm_amd.training import compute_ranking_metrics
    rng = np.random.default_rng(1)
    uid = np.repeat(np.arange(100), 20)
    y = (rng.random(uid.size) < 0.2).astype(np.float32)
    s = rng.random(uid.size).astype(np.float32)
    ks, users = KS, 100
    if bad == "nan":
        s[77] = np.nan
    elif bad == "id_high":
        uid[1234] = 100
    elif bad == "id_negative":
        uid[5] = -3
    elif bad == "label_half":
        y[9] = 0.5
    elif bad == "k0":
        ks = [0, 5]
    elif bad == "ks9":
        ks = list(range(1, 10))
    else:
        uid, y, s = uid[:0], y[:0], s[:0]
    with pytest.raises(ValueError):
        compute_ranking_metrics(uid, y, s, ks, num_users=users)
    # the device is still healthy: a clean call right after gives the restatement's values
    torch.cuda.synchronize()
    uid, y, s = np.repeat(np.arange(100), 20), (rng.random(2000) < 0.2).astype(np.float32), rng.random(2000)
    s = s.astype(np.float32)
    assert_ranking_equal(compute_ranking_metrics(uid, y, s, KS), stable_ranking(uid, y, s, KS))


def _user_model():
    """A uniform-schema DeepFM with a SPARSE ``user_id`` field, trained a few fused steps."""
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    from deepfm_amd.training.fused_step import FusedDeepFMStep
    from deepfm_amd.training.rowsparse import RowSparseAdam
    D = 16
    fields = [dict(name="user_id", type="sparse", vocab=2000, dim=D, max_len=1, combiner="mean"),
              dict(name="item_id", type="sparse", vocab=5000, dim=D, max_len=1, combiner="mean"),
              dict(name="genre", type="sparse", vocab=20, dim=D, max_len=1, combiner="mean"),
              dict(name="age", type="dense", vocab=0, dim=D, max_len=1, combiner="mean")]
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = D
    torch.manual_seed(0)
    model = create_model("deepfm", schema_from_fields(fields), cfg).cuda().train()
    model.embedding.pack_tables_()
    model.embedding.set_grad_mode("rowsparse")
    opt = RowSparseAdam(model, lr=1e-3, l2=1e-5, max_grad_norm=1.0)
    Bt = 1024
    step = FusedDeepFMStep(model, opt, Bt, use_graph=True)
    g = torch.Generator(device="cuda").manual_seed(3)
    vocab = torch.tensor([2000, 5000, 20], device="cuda").view(3, 1)
    for k in range(8):
        ids = (torch.rand((3, Bt), generator=g, device="cuda") * vocab).long()
        dense = torch.rand((1, Bt), generator=g, device="cuda")
        labels = ((ids[1] % 7) < 2).float()
        step.load_batch(ids, dense, labels)
        if k == 0:
            step.capture()
        step.run()
    torch.cuda.synchronize()
    return model


def test_predictor_evaluate_adds_the_ranking_keys():
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FusedPredictor, compute_ranking_metrics
    model = _user_model()
    users, cands = 2000, 100
    rng = np.random.default_rng(11)
    uid = np.repeat(np.arange(users, dtype=np.int64), cands)
    y = np.zeros(uid.size, np.float32)
    y[np.arange(users) * cands + rng.integers(0, cands, users)] = 1.0
    feats = {"user_id": uid, "item_id": rng.integers(0, 5000, uid.size), "genre": rng.integers(0, 20, uid.size),
             "age": rng.random(uid.size).astype(np.float32)}
    cols = PackedColumns(model.schema, feats, y)
    pred = FusedPredictor(model, 4096)
    plain = pred.evaluate(cols)
    assert list(plain) == ["auc", "logloss"]
    scores0 = pred.last_scores.clone()
    m = pred.evaluate(cols, ranking_ks=KS)
    assert torch.equal(pred.last_scores, scores0)
    assert m["auc"] == plain["auc"] and m["logloss"] == plain["logloss"]
    ranking = {k: v for k, v in m.items() if k not in ("auc", "logloss")}
    assert list(m)[:2] == ["auc", "logloss"]
    want = stable_ranking(uid, pred.last_labels.cpu().numpy(), pred.last_scores.cpu().numpy(), KS)
    assert_ranking_equal(ranking, want, "predictor")
    d_uid = torch.from_numpy(uid).cuda()
    assert ranking == compute_ranking_metrics(d_uid, pred.last_labels, pred.last_scores, KS, num_users=2000)
    assert 0.0 < ranking["HR@20"] < 1.0
    # no SPARSE field of that name: no ranking keys, as the reference without dataset.features["user_id"]
    assert list(pred.evaluate(cols, ranking_ks=KS, user_field="visitor")) == ["auc", "logloss"]
    assert list(pred.evaluate(cols, ranking_ks=KS, user_field="age")) == ["auc", "logloss"]
