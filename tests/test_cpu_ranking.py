"""CPU: the leave-one-out ranking fixture agrees with the numpy restatement of the stable-tie contract, and the
ranking entry points are declared, exported, bound and refuse bad arguments before any device work."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ranking_reference.npz")
SYMBOLS = ["dfm_ranking_workspace_bytes", "dfm_ranking_metrics"]


def stable_ranking(user_ids, labels, scores, ks, require_both_classes=True):
    """The contract in numpy: group by user id (dataset order kept), keep users with both classes (or, unfiltered,
    every user); a user's rank is the position of its first positive in ``np.argsort(-scores, kind="stable")``
    (none: a miss); HR@k = #(rank < k) / users, NDCG@k = sum over rank < k of 1 / log2(rank + 2), / users, summed
    in user-id order.  ``{}`` when no user is kept."""
    uid = np.asarray(user_ids, np.int64)
    y = np.asarray(labels, np.float32)
    s = np.asarray(scores, np.float32)
    order = np.argsort(uid, kind="stable")
    bounds = np.flatnonzero(np.diff(uid[order])) + 1
    ranks = []                                    # per kept user: first positive's position, or None
    for idx in np.split(order, bounds):
        yu = y[idx]
        if require_both_classes and not (0 < yu.sum() < yu.size):
            continue
        hit = np.flatnonzero(yu[np.argsort(-s[idx], kind="stable")] == 1)
        ranks.append(int(hit[0]) if hit.size else None)
    if not ranks:
        return {}
    out = {}
    for k in ks:
        inside = [r for r in ranks if r is not None and r < k]
        out[f"HR@{k}"] = len(inside) / len(ranks)
        out[f"NDCG@{k}"] = float(sum(1.0 / np.log2(r + 2.0) for r in inside) / len(ranks))
    return out


def assert_ranking_equal(got, want, what=""):
    """Same keys in the same order, HR@k bit-equal, NDCG@k within 1e-12 relative."""
    assert list(got) == list(want), (what, list(got), list(want))
    for key, v in want.items():
        if key.startswith("HR@"):
            assert got[key] == v, (what, key, got[key], v)
        else:
            assert abs(got[key] - v) <= 1e-12 * abs(v), (what, key, got[key], v)


def fixture_cases():
    g = np.load(GOLDEN, allow_pickle=False)
    return g, [str(c) for c in g["cases"]]


def load_case(g, name):
    """(user_ids int64, labels f32, scores f32, ks) of a fixture case, decoded as tools/make_ranking_golden.py
    describes: scores are codes times a power-of-two scale; a case with a ``base`` is that case's samples in the
    stride permutation ``j <- (j * stride) mod n``."""
    base = str(g[f"{name}/base"]) if f"{name}/base" in g.files else name
    uid = g[f"{base}/user_ids"].astype(np.int64)
    y = g[f"{base}/labels"].astype(np.float32)
    s = (g[f"{base}/score_codes"].astype(np.float64) * float(g[f"{base}/score_scale"])).astype(np.float32)
    if base != name:
        src = (np.arange(uid.size, dtype=np.int64) * int(g[f"{name}/stride"])) % uid.size
        assert np.unique(src).size == uid.size
        uid, y, s = uid[src], y[src], s[src]
    return uid, y, s, g[f"{name}/ks"].tolist()


def per_user_lists(uid, scores, labels):
    """Per-user arrays in first-appearance order (the reference trainer's grouping, trainer.py:311-320)."""
    _, first = np.unique(uid, return_index=True)
    users = uid[np.sort(first)]
    return [scores[uid == u] for u in users], [labels[uid == u] for u in users]


@pytest.mark.parametrize("case", fixture_cases()[1])
def test_fixture_matches_the_stable_restatement(case):
    g, _ = fixture_cases()
    uid, y, s, ks = load_case(g, case)
    assert uid.shape == y.shape == s.shape
    assert set(np.unique(y).tolist()) <= {0.0, 1.0}
    for su in per_user_lists(uid, s, y)[0]:
        assert np.unique(su).size == su.size             # tie-free within a user: argsort order is unique
    trainer = json.loads(str(g[f"{case}/trainer"]))
    evaluator = json.loads(str(g[f"{case}/evaluator"]))
    assert_ranking_equal(stable_ranking(uid, y, s, ks), trainer, case)
    assert_ranking_equal(stable_ranking(uid, y, s, ks, require_both_classes=False), evaluator, case)
    assert list(trainer) == [f"{m}@{k}" for k in ks for m in ("HR", "NDCG")]


def test_fixture_covers_the_issue_cases():
    g, cases = fixture_cases()
    assert {"loo_contiguous", "loo_shuffled", "mixed", "sparse_ids", "large_ks"} <= set(cases)
    uid = load_case(g, "loo_contiguous")[0]
    assert np.unique(uid).size == 943 and uid.size == 943 * 100 and np.all(np.diff(uid) >= 0)
    shuffled = load_case(g, "loo_shuffled")[0]
    assert np.all(shuffled[1:] != shuffled[:-1])                 # neighbours belong to different users
    assert np.array_equal(np.sort(shuffled), uid)
    sparse = load_case(g, "sparse_ids")[0]
    assert sparse.max() >= 100_000 and np.unique(sparse).size == 5000
    assert load_case(g, "large_ks")[3] == [3, 50, 1000]
    uid, y = load_case(g, "mixed")[:2]
    npos = np.bincount(uid, weights=y)
    cnt = np.bincount(uid)
    assert np.any(npos > 1) and np.any((npos == 0) & (cnt > 1)) and np.any((npos == cnt) & (cnt > 1))
    assert np.any(cnt == 1) and np.any((cnt > 1) & (cnt < 20))
    assert np.any(np.diff(uid) < 0)                              # interleaved
    assert os.path.getsize(GOLDEN) < 256 * 1024


def test_restatement_orders_ties_by_dataset_order():
    # user 0: the positive ties with two negatives, one before and one after it -> rank 1
    # user 1: -0.0 and +0.0 tie (the negative comes first) -> rank 1; user 2: two tied positives -> rank 0
    uid = np.array([0, 0, 0, 0, 1, 1, 2, 2, 2])
    y = np.array([0, 0, 1, 0, 0, 1, 0, 1, 1], np.float32)
    s = np.array([0.1, 0.5, 0.5, 0.5, -0.0, 0.0, 0.2, 0.9, 0.9], np.float32)
    got = stable_ranking(uid, y, s, [1, 2])
    assert got["HR@1"] == 1 / 3 and got["HR@2"] == 1.0
    assert got["NDCG@2"] == pytest.approx((2 / np.log2(3) + 1.0) / 3, rel=1e-15)


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
    for name in ("RankingEvaluator", "compute_ranking_metrics", "ranking_metrics_device"):
        assert hasattr(T, name), name


def test_workspace_bytes():
    from deepfm_amd import _lib
    lib = _lib.load()
    small, big = lib.dfm_ranking_workspace_bytes(100, 10), lib.dfm_ranking_workspace_bytes(100, 200_000)
    assert 0 < small < big
    assert big >= 20 * 200_000                     # best + counts + ranks per user
    assert big % 8 == 0
    assert lib.dfm_ranking_workspace_bytes(0, 10) == 0 and lib.dfm_ranking_workspace_bytes(10, 0) == 0


@pytest.mark.parametrize("change", ["null", "n0", "n_2_32", "users0", "ks0", "ks9", "k0"])
def test_bad_arguments_are_refused_before_any_launch(change):
    from deepfm_amd import _lib
    lib = _lib.load()
    fake = 1 << 20                                 # never dereferenced: every check runs before a launch
    args = dict(uid=fake, y=fake, s=fake, n=100, users=10, ks=[1, 5], ws=fake, out=fake)
    if change == "null":
        args["out"] = 0
    elif change == "n0":
        args["n"] = 0
    elif change == "n_2_32":
        args["n"] = 1 << 32
    elif change == "users0":
        args["users"] = 0
    elif change == "ks0":
        args["ks"] = []
    elif change == "ks9":
        args["ks"] = list(range(1, 10))
    else:
        args["ks"] = [5, 0]
    h_ks = (C.c_int32 * max(len(args["ks"]), 1))(*args["ks"])
    rc = lib.dfm_ranking_metrics(args["uid"], args["y"], args["s"], args["n"], args["users"], h_ks, len(args["ks"]),
                                 1, args["ws"], args["out"], None)
    assert rc == 1                                 # DFM_ERR_INVALID
    assert lib.dfm_last_error()


@pytest.mark.parametrize("ks", [[], [0, 5], list(range(1, 10))])
def test_python_refuses_bad_ks_before_any_device_work(ks):
    from deepfm_amd.training import compute_ranking_metrics
    with pytest.raises(ValueError):
        compute_ranking_metrics(np.zeros(3, np.int64), np.array([0, 1, 0], np.float32),
                                np.array([0.1, 0.2, 0.3], np.float32), ks)
