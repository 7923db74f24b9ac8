"""CPU: the bootstrap entry points are declared, exported and bound and refuse bad arguments before any launch; the
numpy restatement's weights are Poisson(1), its pair count agrees with a brute force and with sklearn's weighted AUC, its
spread with the DeLong standard error; ``bootstrap_dict``; the Trainer bootstraps the final test evaluation only."""
import decimal
import os
import re

import numpy as np
import pytest

from tests import bootstrap_reference as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dfm_bootstrap_workspace_bytes", "dfm_bootstrap_prepare", "dfm_bootstrap_replicates"]
KEYS = [f"{m}_{k}" for m in ("auc", "logloss") for k in ("se", "lo", "hi", "replicates")]


def test_entry_points_are_declared_exported_and_bound():
    from deepfm_amd import _lib
    import deepfm_amd.training as T
    text = open(os.path.join(ROOT, "include", "deepfm_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dfm_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    for name in ("bootstrap_device", "bootstrap_dict", "compute_bootstrap", "compare_bootstrap"):
        assert hasattr(T, name), name
    assert f"#define DFM_BOOTSTRAP_CHUNK {_lib.BOOTSTRAP_CHUNK}\n" in text
    assert f"#define DFM_BOOTSTRAP_REPLICATE_BLOCK {_lib.BOOTSTRAP_REPLICATE_BLOCK}\n" in text
    assert f"#define DFM_BOOTSTRAP_MAX_REPLICATES {_lib.BOOTSTRAP_MAX_REPLICATES}\n" in text
    assert _lib.BOOTSTRAP_MAX_N == 1 << 26 and "#define DFM_BOOTSTRAP_MAX_LOG2_N 26\n" in text


def test_workspace_bytes():
    from deepfm_amd import _lib
    ws = _lib.load().dfm_bootstrap_workspace_bytes
    for n, r in ((0, 10), (-1, 10), ((1 << 26) + 1, 10), (10, 0), (10, -3), (10, 65537), (0, 0)):
        assert ws(n, r) == 0, (n, r)
    C = _lib.BOOTSTRAP_CHUNK
    ns = [1, 2, 63, 64, 65, C - 1, C, C + 1, 3 * C + 7, 1_000_000, 1 << 26]
    rs = [1, 15, 16, 17, 200, 4096, 65536]
    table = np.array([[ws(n, r) for r in rs] for n in ns], dtype=object)
    assert all(int(b) > 0 and int(b) % 16 == 0 for b in table.reshape(-1))
    assert all(a <= b for col in table.T for a, b in zip(col, col[1:]))          # monotone in n
    assert all(a <= b for row in table for a, b in zip(row, row[1:]))            # ... and in the replicates
    assert ws(1_000_000, 200) >= 4 * 1_000_000                                    # a log-loss term per sample


@pytest.mark.parametrize("change", ["null_keys", "null_counts", "null_values", "null_faults", "null_ws", "n0", "n_big",
                                    "r0", "r_big", "unaligned"])
def test_bad_arguments_are_refused_before_any_launch(change):
    from deepfm_amd import _lib
    lib = _lib.load()
    fake = 1 << 20                                      # never dereferenced: every check runs before a launch
    a = dict(y=fake, s=fake, u=fake, n=100, r=10, k0=fake, k1=fake, ws=fake, counts=fake, values=fake, faults=fake)
    a.update({"null_keys": dict(k1=0), "null_counts": dict(counts=0), "null_values": dict(values=0),
              "null_faults": dict(faults=0), "null_ws": dict(ws=0), "n0": dict(n=0), "n_big": dict(n=(1 << 26) + 1),
              "r0": dict(r=0), "r_big": dict(r=65537), "unaligned": dict(ws=fake + 8)}[change])
    if change in ("null_keys", "null_ws", "n0", "n_big", "unaligned"):
        assert lib.dfm_bootstrap_prepare(a["y"], a["s"], a["u"], a["n"], a["k0"], a["k1"], a["ws"], None) == 1
        assert lib.dfm_last_error()
    assert lib.dfm_bootstrap_replicates(a["k0"], a["k1"], a["u"], a["n"], a["r"], 7, a["ws"], a["counts"], a["values"],
                                        a["faults"], None) == 1
    assert lib.dfm_last_error()


def test_thresholds_are_the_poisson_cdf():
    decimal.getcontext().prec = 50
    e_inv = decimal.Decimal(-1).exp()
    cdf, fact = decimal.Decimal(0), decimal.Decimal(1)
    for k in range(12):
        fact = fact * k if k else fact
        cdf += e_inv / fact
        assert int(BR.T[k]) == int((cdf * (1 << 32)).to_integral_value(rounding=decimal.ROUND_FLOOR)), k
    text = open(os.path.join(ROOT, "include", "deepfm_hip.h")).read()
    assert all(str(int(t)) in text for t in BR.T)


def test_weights_are_poisson_one():
    w = BR.weights(5, 3, np.arange(2_000_000))
    hist = np.bincount(w, minlength=13) / w.size
    for k, want in enumerate([np.exp(-1), np.exp(-1), np.exp(-1) / 2, np.exp(-1) / 6]):
        assert abs(hist[k] - want) <= 0.01 * want, (k, hist[k])
    assert abs(w.mean() - 1.0) <= 0.005 and w.max() <= 12
    # a function of (seed, replicate, unit): another seed or replicate resamples, the same one repeats
    assert np.array_equal(w[:1000], BR.weights(5, 3, np.arange(1000)))
    assert not np.array_equal(w[:1000], BR.weights(6, 3, np.arange(1000)))
    assert not np.array_equal(w[:1000], BR.weights(5, 4, np.arange(1000)))


def _tied_case(rng, n):
    y = (rng.random(n) < 0.4).astype(np.float32)
    s = np.round(rng.standard_normal(n), 1).astype(np.float32)
    s[::17] = -0.0
    s[5::29] = 0.0
    return y, s


@pytest.mark.parametrize("units", [False, True])
def test_restatement_matches_a_brute_force_pair_count(units):
    rng = np.random.default_rng(3)
    n = 300
    y, s = _tied_case(rng, n)
    uid = rng.integers(0, 40, n) if units else None
    r = BR.bootstrap(y, s, 5, seed=9, unit_ids=uid)
    assert r["faults"].tolist() == [0, 0, 0]
    for k in range(5):
        w = BR.weights(9, k, np.arange(n) if uid is None else uid)
        U, P, N, L, S = (int(v) for v in r["counts"][k])
        assert U == BR.brute_force_u(y, s, w), k
        assert (P, N, S) == (int(w[y == 1].sum()), int(w[y == 0].sum()), int(w.sum()))
        assert L == int((w * BR.logloss_terms(s, y == 1)).sum())


def test_restatement_matches_sklearn_weighted():
    from sklearn.metrics import log_loss, roc_auc_score
    rng = np.random.default_rng(4)
    n = 2000
    y = (rng.random(n) < 0.3).astype(np.float32)
    s = (1 / (1 + np.exp(-(rng.standard_normal(n) + y)))).astype(np.float32)
    s[::50] = np.round(s[::50], 1)
    r = BR.bootstrap(y, s, 6, seed=1)
    for k in range(6):
        w = BR.weights(1, k, np.arange(n))
        assert abs(r["values"][k, 0] - roc_auc_score(y, s, sample_weight=w)) <= 1e-12, k
        # the sums are in units of 2^-27: half a unit per sample at the most
        assert abs(r["values"][k, 1] - log_loss(y, s.astype(np.float64), sample_weight=w)) <= 2.0 ** -27, k


def test_restatement_counts_and_skips_faulty_samples():
    y = np.array([0, 1, 1, 0, 1, 0.5, 0, 2, 1, 0], np.float32)
    s = np.array([.1, .2, .1, .3, np.nan, .4, .5, .6, .7, np.nan], np.float32)
    u = np.array([0, 1, 2, 3, 4, 5, -1, 7, 1 << 40, 9])
    r = BR.bootstrap(y, s, 3, seed=2, unit_ids=u)
    assert r["faults"].tolist() == [2, 2, 2]
    keep = [0, 1, 2, 3]
    want = BR.bootstrap(y[keep], s[keep], 3, seed=2, unit_ids=u[keep])
    assert np.array_equal(r["counts"], want["counts"]) and np.array_equal(r["values"], want["values"], equal_nan=True)
    # without unit ids the unit is the position in the whole input, not among the used samples
    r = BR.bootstrap(y, s, 3, seed=2)
    assert r["faults"].tolist() == [2, 2, 0]
    keep = [0, 1, 2, 3, 6, 8]
    want = BR.bootstrap(y[keep], s[keep], 3, seed=2, unit_ids=np.array(keep))
    assert np.array_equal(r["counts"], want["counts"])


def test_single_class_replicates_are_nan_with_a_log_loss():
    s = np.array([.2, .4, .9], np.float32)
    r = BR.bootstrap(np.ones(3, np.float32), s, 8, seed=0)
    assert np.isnan(r["values"][:, 0]).all() and (r["counts"][:, [0, 2]] == 0).all()
    live = r["counts"][:, 4] > 0
    assert live.any() and np.isfinite(r["values"][live, 1]).all() and np.isnan(r["values"][~live, 1]).all()


def _delong_se(y, s):
    pos, neg = s[y].astype(np.float64), s[~y].astype(np.float64)
    cmp = (pos[:, None] > neg[None, :]) + 0.5 * (pos[:, None] == neg[None, :])
    v10, v01 = cmp.mean(axis=1), cmp.mean(axis=0)
    return float(np.sqrt(v10.var(ddof=1) / pos.size + v01.var(ddof=1) / neg.size)), float(cmp.mean())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_spread_agrees_with_delong(seed):
    """A condition on the restatement (the kernels are compared with it bit for bit): the standard deviation of
    ``auc_r`` within [0.8, 1.25] of the DeLong standard error; a numpy prototype gave 0.971, 0.972 and 1.085."""
    rng = np.random.default_rng(seed)
    n = 4000
    y = rng.random(n) < 0.3
    s = (1 / (1 + np.exp(-(rng.normal(size=n) + y)))).astype(np.float32)
    r = BR.bootstrap(y.astype(np.float32), s, 400, seed=seed + 11)
    d = BR.summary(r["values"])
    se, auc = _delong_se(y, s)
    ratio = d["auc_se"] / se
    print(f"seed {seed}: bootstrap se {d['auc_se']:.6f}, DeLong se {se:.6f}, ratio {ratio:.3f}")
    assert 0.8 <= ratio <= 1.25
    assert d["auc_lo"] <= auc <= d["auc_hi"] and d["auc_replicates"] == 400


def test_bootstrap_dict():
    from deepfm_amd.training import bootstrap_dict
    rng = np.random.default_rng(0)
    v = rng.random((50, 2))
    v[3, 0] = v[7, 0] = v[7, 1] = np.nan
    for level in (0.95, 0.8):
        d = bootstrap_dict(v, [0, 0, 0], level)
        q = (1 - level) / 2
        assert list(d) == KEYS
        assert d["auc_lo"] == np.nanquantile(v[:, 0], q) and d["auc_hi"] == np.nanquantile(v[:, 0], 1 - q)
        assert d["logloss_lo"] == np.nanquantile(v[:, 1], q) and d["logloss_hi"] == np.nanquantile(v[:, 1], 1 - q)
        assert d["auc_se"] == np.nanstd(v[:, 0], ddof=1) and d["logloss_se"] == np.nanstd(v[:, 1], ddof=1)
        assert (d["auc_replicates"], d["logloss_replicates"]) == (48, 49)
        assert d == BR.summary(v, level)
    # the flat (2 R,) host values of an evaluation's one read, as lists
    assert bootstrap_dict(v.reshape(-1).tolist(), [0.0, 0.0, 0.0]) == bootstrap_dict(v, [0, 0, 0])
    d = bootstrap_dict([[np.nan, 0.5]], [0, 0, 0])
    assert np.isnan([d["auc_se"], d["auc_lo"], d["auc_hi"], d["logloss_se"]]).all()
    assert (d["auc_replicates"], d["logloss_replicates"], d["logloss_lo"], d["logloss_hi"]) == (0, 1, 0.5, 0.5)
    with pytest.raises(ValueError, match=r"^Input contains NaN\.$"):
        bootstrap_dict(v, [2, 0, 0])
    with pytest.raises(ValueError, match=r"^7 labels other than 0 and 1$"):
        bootstrap_dict(v, [0, 7, 0])
    with pytest.raises(ValueError, match=r"^4 unit ids outside \[0, 2\^40\)$"):
        bootstrap_dict(v, [0, 0, 4])
    with pytest.raises(ValueError, match="level"):
        bootstrap_dict(v, [0, 0, 0], 1.0)


def test_python_refuses_bad_arguments_before_any_device_work():
    from deepfm_amd.training import compare_bootstrap, compute_bootstrap
    with pytest.raises(TypeError):
        compute_bootstrap([0, 1, 0], [0.1, 0.2, 0.3])                                         # scores: no list
    with pytest.raises(ValueError, match="level"):
        compute_bootstrap([0, 1, 0], [0.1, 0.2, 0.3], level=0.0)
    with pytest.raises(ValueError, match="level"):
        compare_bootstrap([0, 1, 0], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3], level=2)


def test_trainer_bootstraps_the_final_test_evaluation_only():
    """``Trainer.evaluate`` on a stand-in predictor: the per-epoch keywords are today's, the test split's gain the
    replicates, by user when the schema has a SPARSE ``user_id``."""
    from deepfm_amd.config import ExperimentConfig, TrainingConfig
    from deepfm_amd.data.device_epoch import DeviceEpochLoader
    from deepfm_amd.data.synthetic import criteo_fields, movielens_fields, schema_from_fields
    from deepfm_amd.training import Trainer
    calls = []

    class Pred:
        def evaluate_loader(self, loader, **kw):
            calls.append(kw)
            return {"auc": 0.5}

    loader = DeviceEpochLoader.__new__(DeviceEpochLoader)
    loader.batch_size = 8
    with_users, without = schema_from_fields(movielens_fields()), schema_from_fields(criteo_fields(50, 8))
    assert "user_id" in with_users.fields and "user_id" not in without.fields
    epoch = {"ranking_ks": [1, 5], "group_auc": False}
    for schema, bootstrap, extra in ((with_users, 0, {}), (with_users, 70, {"bootstrap": 70, "bootstrap_by": "user_id"}),
                                     (without, 70, {"bootstrap": 70})):
        t = Trainer.__new__(Trainer)
        t.config = ExperimentConfig(training=TrainingConfig(metric="auc", ranking_ks=[1, 5]))
        t.schema = schema
        if bootstrap:
            t.bootstrap = bootstrap
        t._predictor = lambda b: Pred()
        assert t._evaluation_keywords() == epoch
        for split in ("eval", "val"):
            assert t.evaluate(loader, split) == {"auc": 0.5} and calls[-1] == epoch
        assert t.evaluate(loader) == {"auc": 0.5} and calls[-1] == epoch
        assert t.evaluate(loader, "test") == {"auc": 0.5} and calls[-1] == {**epoch, **extra}
    with pytest.raises(ValueError, match=r"bootstrap = 65537 outside \[0, 65536\]"):
        Trainer(None, with_users, ExperimentConfig(), None, None, None, bootstrap=65537)
