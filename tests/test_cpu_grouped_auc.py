"""CPU: the grouped-AUC entry points are declared, exported and bound; the numpy restatement agrees with a brute-force
pair count and with sklearn per group; ``grouped_auc_dict`` and the training loop's choice of the watched metric."""
import os
import re
import types

import numpy as np
import pytest

from tests import grouped_auc_reference as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dfm_grouped_auc_workspace_bytes", "dfm_grouped_auc_prepare", "dfm_grouped_auc_finish"]


def test_entry_points_are_declared_exported_and_bound():
    from deepfm_amd import _lib
    import deepfm_amd.training as T
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepfm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dfm_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    for name in ("grouped_auc_device", "grouped_auc_dict", "compute_gauc"):
        assert hasattr(T, name), name


def test_workspace_bytes():
    from deepfm_amd import _lib
    ws = _lib.load().dfm_grouped_auc_workspace_bytes
    for n, g in ((0, 10), (10, 0), (-1, 10), (10, -5), (0, 0)):
        assert ws(n, g) == 0
    groups = [1, 2, 255, 256, 257, 1000, 262_144, 262_145, 1_000_000, 1 << 30]
    sizes = [ws(100, g) for g in groups]
    assert sizes[0] >= 64 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-2] >= 24 * 1_000_000                  # two runs' bounds and a 64-bit numerator per group
    assert all(b % 8 == 0 for b in sizes)
    by_n = [ws(n, 1000) for n in (1, 2, 1000, 1 << 20, (1 << 31) - 1)]
    assert all(a <= b for a, b in zip(by_n, by_n[1:]))


@pytest.mark.parametrize("change", ["null_keys", "null_out", "n0", "n_2_31", "groups0", "groups_big", "unaligned"])
def test_bad_arguments_are_refused_before_any_launch(change):
    from deepfm_amd import _lib
    lib = _lib.load()
    fake = 1 << 20                                      # never dereferenced: every check runs before a launch
    a = dict(gid=fake, y=fake, s=fake, n=100, groups=10, keys=fake, ws=fake, out=fake)
    if change == "null_keys":
        a["keys"] = 0
    elif change == "null_out":
        a["out"] = 0
    elif change == "n0":
        a["n"] = 0
    elif change == "n_2_31":
        a["n"] = 1 << 31
    elif change == "groups0":
        a["groups"] = 0
    elif change == "groups_big":
        a["groups"] = (1 << 30) + 1
    else:
        a["ws"] = fake + 8
    if change != "null_out":
        assert lib.dfm_grouped_auc_prepare(a["gid"], a["y"], a["s"], a["n"], a["groups"], a["keys"], a["ws"], None) == 1
        assert lib.dfm_last_error()
    assert lib.dfm_grouped_auc_finish(a["keys"], a["n"], a["groups"], a["ws"], None, a["out"], None) == 1
    assert lib.dfm_last_error()


def _random_case(rng, n, groups, levels=None):
    g = rng.integers(0, groups, n)
    y = (rng.random(n) < 0.4).astype(np.float32)
    s = rng.standard_normal(n).astype(np.float32)
    if levels:
        s = (np.round(s * levels) / levels).astype(np.float32)
    return g, y, s


@pytest.mark.parametrize("seed", range(6))
def test_restatement_matches_a_brute_force_pair_count(seed):
    rng = np.random.default_rng(seed)
    g, y, s = _random_case(rng, 200 + 37 * seed, 7, levels=[None, 2, 4][seed % 3])
    s[::17] = -0.0
    s[5::29] = 0.0
    num, P, N, bad = GR.group_integers(g, y, s, 9)
    assert bad == (0, 0, 0)
    for gid in range(9):
        m = g == gid
        assert int(num[gid]) == GR.brute_force_numerator(y[m], s[m]), gid
        assert (P[gid], N[gid]) == (int((y[m] == 1).sum()), int((y[m] == 0).sum()))
    assert P[7] == N[7] == 0 and num[8] == 0


def test_ord_bits_order_and_signed_zero():
    s = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32)
    k = GR.ord_bits(s).astype(np.int64)
    assert k[3] == k[4] and np.all(np.diff(np.delete(k, 3)) > 0)


@pytest.mark.parametrize("seed", range(4))
def test_restatement_matches_sklearn_per_group(seed):
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(100 + seed)
    g, y, s = _random_case(rng, 3000, 40, levels=[None, 8][seed % 2])
    y[g == 3] = 1.0                                       # a group of one class
    y[g == 4] = 0.0
    r = GR.grouped_auc(g, y, s, 45)
    aucs, weights = [], []
    for gid in range(45):
        m = g == gid
        if 0 < y[m].sum() < m.sum():
            want = roc_auc_score(y[m], s[m])
            assert abs(r["per_group"][gid] - want) <= 1e-12, gid
            aucs.append(want)
            weights.append(int(m.sum()))
        else:
            assert np.isnan(r["per_group"][gid]), gid
    assert r["groups"] == len(aucs) == 38 and r["samples"] == sum(weights)
    assert abs(r["uauc"] - np.mean(aucs)) <= 1e-12
    assert abs(r["gauc"] - np.average(aucs, weights=weights)) <= 1e-12


def test_restatement_counts_and_skips_invalid_samples():
    g = np.array([0, 0, 0, 1, 1, 5, -1, 1, 0])
    y = np.array([0, 1, 1, 0, 1, 1, 0, 0.5, 0], np.float32)
    s = np.array([.1, .2, .1, .3, .3, .4, .5, .6, np.nan], np.float32)
    r = GR.grouped_auc(g, y, s, 2)
    assert (r["bad_id"], r["nan"], r["bad_label"]) == (2, 1, 1)
    assert r["per_group"].tolist() == [0.75, 0.5] and r["groups"] == 2 and r["samples"] == 5
    assert r["uauc"] == 0.625 and r["gauc"] == (3 * 0.75 + 2 * 0.5) / 5


def test_tree_sum_is_the_plain_sum_where_that_is_exact():
    assert GR.tree_sum(np.arange(1000.0)) == 499500.0
    assert GR.tree_sum(np.ones(300_000)) == 300_000.0    # more groups than leaves: the strided rounds
    assert GR.tree_sum([0.1]) == 0.1


def test_grouped_auc_dict():
    from deepfm_amd.training import grouped_auc_dict
    assert grouped_auc_dict([3.0, 0.75, 0.5, 12.0, 0.0, 0.0, 0.0]) == {"gauc": 0.75, "uauc": 0.5}
    assert list(grouped_auc_dict([3.0, 0.75, 0.5, 12.0, 0.0, 0.0, 0.0])) == ["gauc", "uauc"]
    assert grouped_auc_dict([0.0, float("nan"), float("nan"), 0.0, 0.0, 0.0, 0.0]) == {}
    with pytest.raises(ValueError, match=r"^4 group ids outside \[0, num_groups\)$"):
        grouped_auc_dict([3.0, 0.75, 0.5, 12.0, 4.0, 0.0, 0.0])
    with pytest.raises(ValueError, match=r"^Input contains NaN\.$"):
        grouped_auc_dict([3.0, 0.75, 0.5, 12.0, 0.0, 2.0, 0.0])
    with pytest.raises(ValueError, match=r"^7 labels other than 0 and 1$"):
        grouped_auc_dict([3.0, 0.75, 0.5, 12.0, 0.0, 0.0, 7.0])


def test_python_refuses_bad_arguments_before_any_device_work():
    from deepfm_amd.training import compute_gauc
    with pytest.raises(TypeError):
        compute_gauc([0, 1, 2], [0, 1, 0], [0.1, 0.2, 0.3])                                   # scores: no list


def _loop(metric, vals, patience=2, epochs=6):
    from deepfm_amd.config import TrainingConfig
    from deepfm_amd.training import run_training_loop
    tc = TrainingConfig(num_epochs=epochs, early_stopping_patience=patience, metric=metric, scheduler="none")
    it, saved, stepped = iter(vals), [], []
    sched = types.SimpleNamespace(step=stepped.append)
    r = run_training_loop(tc, lambda e: 0.5, lambda: dict(next(it)), lambda e, m: saved.append((e, m)), sched)
    return r, saved, stepped


def test_training_loop_watches_gauc():
    # auc rises all the time, gauc peaks at epoch 2: the loop follows gauc
    vals = [{"auc": 0.60 + 0.01 * i, "logloss": 0.5, "gauc": v, "uauc": 1.0 - v}
            for i, v in enumerate([0.70, 0.80, 0.75, 0.79, 0.90, 0.95])]
    r, saved, stepped = _loop("gauc", vals)
    assert saved == [(1, 0.70), (2, 0.80)] and stepped == [0.70, 0.80, 0.75, 0.79]
    assert (r.best_epoch, r.total_epochs) == (2, 4) and r.best_metrics == vals[1]
    # uauc falls from the start: the first epoch stays the best
    r, saved, stepped = _loop("uauc", vals)
    assert saved == [(1, 1.0 - 0.70)] and (r.best_epoch, r.total_epochs) == (1, 3) and stepped == [v["uauc"] for v in vals[:3]]


def test_training_loop_falls_back_to_auc_without_the_key():
    vals = [{"auc": a, "logloss": 0.5} for a in (0.6, 0.7, 0.65, 0.66)]
    r, saved, stepped = _loop("gauc", vals)
    assert saved == [(1, 0.6), (2, 0.7)] and stepped == [0.6, 0.7, 0.65, 0.66]
    assert (r.best_epoch, r.total_epochs) == (2, 4) and r.best_metrics == vals[1]


def test_trainer_asks_for_the_grouped_auc_only_when_it_is_watched():
    """``Trainer.evaluate`` on a stand-in predictor: the flag follows ``training.metric``."""
    from deepfm_amd.config import ExperimentConfig, TrainingConfig
    from deepfm_amd.data.device_epoch import DeviceEpochLoader
    from deepfm_amd.training import Trainer
    calls = []

    class Pred:
        def evaluate_loader(self, loader, **kw):
            calls.append(kw)
            return {"auc": 0.5}

    loader = DeviceEpochLoader.__new__(DeviceEpochLoader)
    loader.batch_size = 8
    for metric, want in (("auc", False), ("gauc", True), ("uauc", True), ("logloss", False), ("HR@10", False)):
        t = Trainer.__new__(Trainer)
        t.config = ExperimentConfig(training=TrainingConfig(metric=metric, ranking_ks=[1, 5]))
        t._predictor = lambda b: Pred()
        assert t.evaluate(loader) == {"auc": 0.5}
        assert calls[-1] == {"ranking_ks": [1, 5], "group_auc": want}, metric
