"""CPU: the entry points of the per-user bootstrap are declared, exported and bound, size their workspace and refuse bad
arguments before any launch; the numpy restatement's weighted formulas equal its brute-force resample (integers exactly,
quotients to the fixed-point resolution) and its weights are the pooled bootstrap's; ``bootstrap_grouped_dict``; the
refusals of the Python layer and of the Trainer."""
import os
import re

import numpy as np
import pytest

from tests import bootstrap_reference as BR
from tests import bootstrap_units_reference as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dfm_bootstrap_units_workspace_bytes", "dfm_bootstrap_units", "dfm_ranking_user_ranks",
           "dfm_bootstrap_rank_columns", "dfm_grouped_auc_unit_columns"]
# 2^-30 is the unit of the gains and of auc_g: a rounding moves a term by at most 2^-31, and so a mean of terms
RESOLUTION = 1e-9
assert 2.0 ** -31 < RESOLUTION


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
    for name in ("ranking_user_ranks_device", "bootstrap_units_device", "bootstrap_grouped_device",
                 "bootstrap_grouped_dict", "compute_bootstrap_ranking", "compare_bootstrap_ranking"):
        assert hasattr(T, name), name
    assert f"#define DFM_BOOTSTRAP_UNITS_CHUNK {_lib.BOOTSTRAP_UNITS_CHUNK}\n" in text
    assert f"#define DFM_BOOTSTRAP_UNITS_MAX_COLS {_lib.BOOTSTRAP_UNITS_MAX_COLS}\n" in text
    assert _lib.BOOTSTRAP_UNITS_MAX_COLS == 24
    assert f"#define DFM_RANK_NOT_COUNTED ({_lib.RANK_NOT_COUNTED})\n" in text
    assert f"#define DFM_RANK_MISS ({_lib.RANK_MISS})\n" in text
    assert (_lib.RANK_NOT_COUNTED, _lib.RANK_MISS) == (UR.NOT_COUNTED, UR.MISS) == (-1, -2)


def test_the_header_documents_the_entry_points():
    text = open(os.path.join(ROOT, "include", "deepfm_hip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for name in SYMBOLS:
        assert name in comments, name
    for words in ("DFM_BOOTSTRAP_UNITS_CHUNK consecutive units", "llrint(2^30 / log2(i + 2))", "llrint(auc_g * 2^30)",
                  "DFM_RANK_NOT_COUNTED for a user that does not count", "wrapping unsigned 64-bit arithmetic",
                  "HR@k_r = sum w hit / sum w counted"):
        assert words in comments, words


def test_workspace_bytes():
    from deepfm_amd import _lib
    ws = _lib.load().dfm_bootstrap_units_workspace_bytes
    for u, c, r in ((0, 4, 10), (-1, 4, 10), ((1 << 30) + 1, 4, 10), (10, 0, 10), (10, -1, 10), (10, 25, 10),
                    (10, 4, 0), (10, 4, -3), (10, 4, 65537), (0, 0, 0)):
        assert ws(u, c, r) == 0, (u, c, r)
    C = _lib.BOOTSTRAP_UNITS_CHUNK
    us = [1, 2, 63, 64, 65, C - 1, C, C + 1, 3 * C + 7, 1_000_000, 1 << 30]
    cs = [1, 2, 9, 13, 17, 24]
    rs = [1, 15, 16, 17, 200, 4096, 65536]
    table = np.array([[[ws(u, c, r) for r in rs] for c in cs] for u in us], dtype=object)
    assert all(int(b) > 0 and int(b) % 16 == 0 for b in table.reshape(-1))
    for axis in range(3):                                                           # monotone in each argument
        t = np.moveaxis(table, axis, 0)
        assert all((a <= b).all() for a, b in zip(t, t[1:])), axis
    assert ws(1 << 30, 24, 200) < 1 << 20                                           # it does not grow with the units


@pytest.mark.parametrize("change", ["null_cols", "null_ws", "null_sums", "u0", "u_big", "c0", "c_big", "r0", "r_big",
                                    "unaligned_ws", "unaligned_cols"])
def test_units_refuses_bad_arguments_before_any_launch(change):
    from deepfm_amd import _lib
    lib = _lib.load()
    fake = 1 << 20                                      # never dereferenced: every check runs before a launch
    a = dict(cols=fake, u=100, c=4, r=10, ws=fake, sums=fake)
    a.update({"null_cols": dict(cols=0), "null_ws": dict(ws=0), "null_sums": dict(sums=0), "u0": dict(u=0),
              "u_big": dict(u=(1 << 30) + 1), "c0": dict(c=0), "c_big": dict(c=25), "r0": dict(r=0),
              "r_big": dict(r=65537), "unaligned_ws": dict(ws=fake + 8), "unaligned_cols": dict(cols=fake + 4)}[change])
    assert lib.dfm_bootstrap_units(a["cols"], a["u"], a["c"], a["r"], 7, a["ws"], a["sums"], None) == 1
    assert lib.dfm_last_error()


@pytest.mark.parametrize("change", ["null_rank", "null_gain", "null_cols", "u0", "ks0", "ks9", "k0", "k_beyond_gain"])
def test_rank_columns_refuses_bad_arguments_before_any_launch(change):
    import ctypes as C
    from deepfm_amd import _lib
    lib = _lib.load()
    fake = 1 << 20
    a = dict(rank=fake, u=100, ks=[1, 5], gain=fake, gain_len=5, cols=fake)
    a.update({"null_rank": dict(rank=0), "null_gain": dict(gain=0), "null_cols": dict(cols=0), "u0": dict(u=0),
              "ks0": dict(ks=[]), "ks9": dict(ks=[1] * 9), "k0": dict(ks=[0, 5]), "k_beyond_gain": dict(ks=[1, 6])}[change])
    h_ks = (C.c_int32 * max(1, len(a["ks"])))(*a["ks"])
    assert lib.dfm_bootstrap_rank_columns(a["rank"], a["u"], h_ks, len(a["ks"]), a["gain"], a["gain_len"], a["cols"],
                                          None) == 1
    assert lib.dfm_last_error()


def test_the_other_entry_points_refuse_bad_arguments_before_any_launch():
    from deepfm_amd import _lib
    lib = _lib.load()
    fake = 1 << 20
    ranks = lambda **kw: lib.dfm_ranking_user_ranks(*[{**dict(u=fake, y=fake, s=fake, n=10, users=4, both=1, ws=fake,
                                                             rank=fake, out=fake), **kw}[k]
                                                      for k in ("u", "y", "s", "n", "users", "both", "ws", "rank", "out")],
                                                    None)
    for kw in (dict(rank=0), dict(out=0), dict(ws=0), dict(n=0), dict(users=0), dict(ws=fake + 8)):
        assert ranks(**kw) == 1 and lib.dfm_last_error(), kw
    cols = lambda **kw: lib.dfm_grouped_auc_unit_columns(*[{**dict(keys=fake, n=10, groups=4, ws=fake, cols=fake),
                                                            **kw}[k] for k in ("keys", "n", "groups", "ws", "cols")],
                                                         None)
    for kw in (dict(keys=0), dict(cols=0), dict(ws=0), dict(n=0), dict(groups=0), dict(groups=(1 << 30) + 1),
               dict(ws=fake + 8)):
        assert cols(**kw) == 1 and lib.dfm_last_error(), kw


# ----------------------------------------------------------------------------- the restatement against a brute force
def _population(rng, users=30, require_ties=True):
    """A few dozen users with ties (rounded scores, -0 / +0), one with negatives only, one with positives only, one
    with a single sample and one id with no sample; interleaved."""
    sizes = rng.integers(2, 9, users)
    sizes[3], sizes[7] = 1, 0
    u = np.repeat(np.arange(users), sizes)
    y = (rng.random(u.size) < 0.35).astype(np.float32)
    y[u == 5], y[u == 11] = 0.0, 1.0
    s = np.round(rng.standard_normal(u.size), 1).astype(np.float32)
    s[::7], s[3::7] = 0.0, -0.0
    p = rng.permutation(u.size)
    return u[p], y[p], s[p], users


@pytest.mark.parametrize("require_both", [True, False])
def test_weighted_formulas_equal_the_brute_force_resample(require_both):
    rng = np.random.default_rng(3 if require_both else 4)
    u, y, s, U = _population(rng)
    ks, R = [1, 3, 5], 12
    cols = UR.columns(u, y, s, ks, U, group_auc=True, require_both_classes=require_both)
    assert cols.shape == (1 + 2 * len(ks) + 4, U)
    sums = UR.weighted_sums(cols, R, seed=9)
    values = UR.replicate_values(sums, len(ks), True)
    assert values.shape == (R, 2 * len(ks) + 2)
    seen_zero = False
    for r in range(R):
        w = BR.weights(9, r, np.arange(U))
        if r == R - 1:
            w[:] = 0                                    # an empty resample: every quotient is NaN
            sums[r] = 0
            values[r] = UR.replicate_values(sums[r:r + 1], len(ks), True)[0]
        brute = UR.brute_force_replicate(u, y, s, ks, w, U, group_auc=True, require_both_classes=require_both)
        m = len(ks)
        assert int(sums[r, 0]) == brute["counted"]
        assert [int(v) for v in sums[r, 1:1 + m]] == brute["hits"]
        assert int(sums[r, 1 + 2 * m]) == brute["qual"] and int(sums[r, 3 + 2 * m]) == brute["size"]
        want = brute["HR"] + brute["NDCG"] + [brute["gauc"], brute["uauc"]]
        for got, ref in zip(values[r], want):
            if np.isnan(ref):
                assert np.isnan(got)
                seen_zero = True
            else:
                assert abs(got - ref) <= RESOLUTION, (r, got, ref)
        assert list(values[r, :m]) == brute["HR"] or not brute["counted"]       # no fixed point in HR: the same division
    assert seen_zero


def test_one_class_users_and_absent_users_are_not_counted():
    rng = np.random.default_rng(5)
    u, y, s, U = _population(rng)
    rank, counted, faults = UR.user_ranks(u, y, s, U)
    assert faults == [0, 0, 0] and counted == int((rank >= 0).sum())
    assert rank[5] == rank[11] == rank[7] == rank[3] == UR.NOT_COUNTED
    loose, counted_loose, _ = UR.user_ranks(u, y, s, U, require_both_classes=False)
    assert loose[5] == UR.MISS and loose[11] == 0 and loose[7] == UR.NOT_COUNTED and counted_loose == U - 1
    assert np.array_equal(loose[rank >= 0], rank[rank >= 0])
    cols = UR.rank_columns(loose, [1, 4])
    assert cols[0, 5] == 1 and cols[1:, 5].sum() == 0 and cols[:, 7].sum() == 0
    assert cols[3, 11] == UR.gain_table(1)[0] == 1 << 30


def test_the_weights_are_the_pooled_bootstraps():
    """sum_u w_u count_u over the bincount column is column S of the pooled bootstrap resampled by user."""
    rng = np.random.default_rng(6)
    n, U, R = 700, 40, 20
    u = rng.integers(0, U, n)
    y = (rng.random(n) < 0.4).astype(np.float32)
    s = rng.random(n).astype(np.float32)
    counts = np.bincount(u, minlength=U)[None, :]
    pooled = BR.bootstrap(y, s, R, seed=11, unit_ids=u)["counts"]
    assert np.array_equal(UR.weighted_sums(counts, R, seed=11)[:, 0].astype(np.int64), pooled[:, 4])
    assert not np.array_equal(UR.weighted_sums(counts, R, seed=12)[:, 0].astype(np.int64), pooled[:, 4])


def test_weighted_sums_wrap():
    cols = np.array([[np.iinfo(np.uint64).max, 5, 1 << 63]], np.uint64)
    w = BR.weights(0, 0, np.arange(3))
    want = sum(int(a) * int(b) for a, b in zip(cols[0], w)) % (1 << 64)
    assert int(UR.weighted_sums(cols, 1)[0, 0]) == want


def test_bootstrap_grouped_dict():
    from deepfm_amd.training import bootstrap_grouped_dict, grouped_metric_names
    rng = np.random.default_rng(7)
    ks = [1, 10]
    names = grouped_metric_names(ks, True)
    assert names == ["HR@1", "HR@10", "NDCG@1", "NDCG@10", "gauc", "uauc"] == UR.names(ks, True)
    v = rng.random((50, len(names)))
    v[::5, 2] = np.nan
    v[:, 5] = np.nan
    d = bootstrap_grouped_dict(v, [0, 0, 0], ks, True, level=0.9)
    assert list(d) == [f"{m}_{k}" for m in names for k in ("se", "lo", "hi", "replicates")]
    want = UR.summary(v, names, 0.9)
    assert list(d) == list(want)
    assert all(d[k] == want[k] or (np.isnan(d[k]) and np.isnan(want[k])) for k in d)
    assert d["NDCG@1_replicates"] == 40 and d["uauc_replicates"] == 0 and np.isnan(d["uauc_se"])
    assert list(bootstrap_grouped_dict(v[:, 4:], [0, 0, 0], [], True)) == [f"{m}_{k}" for m in ("gauc", "uauc")
                                                                          for k in ("se", "lo", "hi", "replicates")]
    with pytest.raises(ValueError, match=r"^3 user ids outside \[0, num_users\)$"):
        bootstrap_grouped_dict(v, [3, 0, 0], ks, True)
    with pytest.raises(ValueError, match=r"^Input contains NaN\.$"):
        bootstrap_grouped_dict(v, [0, 2, 0], ks, True)
    with pytest.raises(ValueError, match=r"^1 labels other than 0 and 1$"):
        bootstrap_grouped_dict(v, [0, 0, 1], ks, True)
    with pytest.raises(ValueError, match="level"):
        bootstrap_grouped_dict(v, [0, 0, 0], ks, True, level=1.0)


def test_python_refuses_bad_arguments_before_any_device_work():
    from deepfm_amd.training import compare_bootstrap_ranking, compute_bootstrap_ranking
    with pytest.raises(TypeError):
        compute_bootstrap_ranking([0, 0, 0], [0, 1, 0], [0.1, 0.2, 0.3])                       # scores: no list
    with pytest.raises(ValueError, match="level"):
        compute_bootstrap_ranking([0, 0, 0], [0, 1, 0], [0.1, 0.2, 0.3], level=0.0)
    with pytest.raises(ValueError, match="level"):
        compare_bootstrap_ranking([0, 0, 0], [0, 1, 0], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3], level=2)


def test_trainer_refuses_bootstrap_grouped_without_what_it_needs():
    """The refusals come before any device work; the final test evaluation alone gains the keyword."""
    from deepfm_amd.config import ExperimentConfig, TrainingConfig
    from deepfm_amd.data.synthetic import criteo_fields, movielens_fields, schema_from_fields
    from deepfm_amd.training import Trainer
    with_users, without = schema_from_fields(movielens_fields()), schema_from_fields(criteo_fields(50, 8))
    ranked = ExperimentConfig(training=TrainingConfig(metric="auc", ranking_ks=[1, 5]))
    plain = ExperimentConfig(training=TrainingConfig(metric="auc", ranking_ks=[]))
    for schema, cfg, bootstrap, words in ((with_users, ranked, 0, "bootstrap_grouped needs bootstrap"),
                                          (without, ranked, 40, "it needs a SPARSE user_id field"),
                                          (with_users, plain, 40, "it needs training.ranking_ks or training.metric")):
        with pytest.raises(ValueError, match=words):
            Trainer(None, schema, cfg, None, None, None, bootstrap=bootstrap, bootstrap_grouped=True)
    t = Trainer.__new__(Trainer)
    t.config, t.schema, t.bootstrap, t.bootstrap_grouped = ranked, with_users, 40, True
    assert t._test_keywords() == {"ranking_ks": [1, 5], "group_auc": False, "bootstrap": 40, "bootstrap_by": "user_id",
                                  "bootstrap_grouped": True}
    assert "bootstrap_grouped" not in t._evaluation_keywords()
    t.bootstrap_grouped = False
    assert "bootstrap_grouped" not in t._test_keywords()
