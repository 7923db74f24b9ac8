"""CPU: the one statement of which metric families an evaluation holds and how their host values become ``evaluate``'s
dict (``training/metrics.py``: ``Evaluation``, ``decode_evaluation``, ``read_evaluations``, ``delta_dict``), on
hand-written host vectors: the exact dict with its key order for every combination of families, the keys that
``evaluate`` omits, every family's refusals, and the shared delta loop against both spellings it replaced."""
import math

import numpy as np
import pytest

from tests import bootstrap_reference as BR
from tests import bootstrap_units_reference as UR

R = 5
POINTS = [0.75, 0.5, 3.0, 4.0, 0.0]                                  # auc, logloss, positives, negatives, NaN scores
RANKING = [5.0, 0.2, 0.6, 0.2, 0.4, 0.0, 0.0, 0.0]                   # users, HR@1, HR@3, NDCG@1, NDCG@3, three faults
GAUC = [4.0, 0.7, 0.65, 30.0, 0.0, 0.0, 0.0]                         # groups, gauc, uauc, samples, three faults
CALIBRATION = [10.0, 4.0, 0.5, 0.2, 0.6, 0.05, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0]
CALIBRATION_DICT = {"mean_pred": 0.5, "base_rate": 0.4, "brier": 0.2, "ece": 0.05, "mce": 0.1, "copc": 0.5 * 10.0 / 4.0,
                    "ne": 0.6 / -(0.4 * math.log(0.4) + 0.6 * math.log(0.6))}
OK = [0.0, 0.0, 0.0]


def _replicates(columns, seed):
    v = np.random.default_rng(seed).random((R, columns))
    v[1, 0] = np.nan                                                 # a replicate without a value is dropped
    return v


POOLED, GROUPED, GROUPED_NO_KS = _replicates(2, 1), _replicates(6, 2), _replicates(2, 3)


def _decode(req, host, **kw):
    from deepfm_amd.training.metrics import decode_evaluation
    return decode_evaluation(req, [np.asarray(part, np.float64).reshape(-1) for part in host], **kw)


def _same(got, want):
    """The same keys in the same order and the same floats, bit for bit."""
    assert list(got) == list(want)
    for k in want:
        assert got[k] == want[k] and type(got[k]) is type(want[k]), (k, got[k], want[k])


def test_no_family_gives_the_two_points_in_either_spelling():
    from deepfm_amd.training.metrics import Evaluation
    _same(_decode(Evaluation(), [POINTS]), {"auc": 0.75, "logloss": 0.5})
    for one_class in ([0.75, 0.5, 0.0, 7.0, 0.0], [0.75, 0.5, 7.0, 0.0, 0.0]):      # evaluate: 0.0 for a single class
        _same(_decode(Evaluation(), [one_class]), {"auc": 0.0, "logloss": 0.5})
    nan_auc = _decode(Evaluation(), [[np.nan, 0.5, 0.0, 7.0, 0.0]], pooled="nan")   # compute_bootstrap: NaN
    assert list(nan_auc) == ["auc", "logloss"] and np.isnan(nan_auc["auc"]) and nan_auc["logloss"] == 0.5
    with pytest.raises(ValueError, match=r"^the model produced NaN scores$"):
        _decode(Evaluation(), [[0.75, 0.5, 3.0, 4.0, 2.0]])
    _same(_decode(Evaluation(), [[0.75, 0.5, 3.0, 4.0, 2.0]], pooled="nan"), {"auc": 0.75, "logloss": 0.5})
    # asked for, but the split has no user ids: evaluate leaves the per-user families out
    asked = Evaluation(ks=[1, 3], group_auc=True)
    _same(_decode(asked, [POINTS], users=False), {"auc": 0.75, "logloss": 0.5})
    assert asked.point_names(users=False) == ["auc", "logloss"]


def test_ranking_only():
    from deepfm_amd.training.metrics import Evaluation
    req = Evaluation(ks=[1, 3])
    want = {"auc": 0.75, "logloss": 0.5, "HR@1": 0.2, "NDCG@1": 0.2, "HR@3": 0.6, "NDCG@3": 0.4}
    _same(_decode(req, [POINTS, RANKING]), want)
    assert req.point_names() == list(want)
    _same(_decode(req, [POINTS, [0.0] + RANKING[1:]]), {"auc": 0.75, "logloss": 0.5})          # no qualifying user
    _same(_decode(req, [RANKING], pooled=None), {k: want[k] for k in list(want)[2:]})          # without the pooled points


def test_group_auc_only():
    from deepfm_amd.training.metrics import Evaluation
    req = Evaluation(group_auc=True)
    _same(_decode(req, [POINTS, GAUC]), {"auc": 0.75, "logloss": 0.5, "gauc": 0.7, "uauc": 0.65})
    assert req.point_names() == ["auc", "logloss", "gauc", "uauc"]
    _same(_decode(req, [POINTS, [0.0] + GAUC[1:]]), {"auc": 0.75, "logloss": 0.5})             # no group with both classes


def test_all_six_families_in_evaluates_order():
    from deepfm_amd.training.metrics import Evaluation
    req = Evaluation(ks=[1, 3], group_auc=True, bins=4, replicates=R, seed=9, grouped=True, level=0.9)
    got = _decode(req, [POINTS, RANKING, GAUC, CALIBRATION, POOLED, OK, GROUPED, OK])
    names = ["HR@1", "HR@3", "NDCG@1", "NDCG@3", "gauc", "uauc"]                                # the replicates' columns
    want = {"auc": 0.75, "logloss": 0.5, "HR@1": 0.2, "NDCG@1": 0.2, "HR@3": 0.6, "NDCG@3": 0.4, "gauc": 0.7,
            "uauc": 0.65, **CALIBRATION_DICT, **BR.summary(POOLED, 0.9), **UR.summary(GROUPED, names, 0.9)}
    _same(got, want)
    assert req.point_names() == list(want)[:8]
    assert (got["auc_replicates"], got["logloss_replicates"], got["HR@1_replicates"], got["uauc_replicates"]) == \
        (R - 1, R, R - 1, R)
    assert list(got)[-4:] == ["uauc_se", "uauc_lo", "uauc_hi", "uauc_replicates"]
    # no positive: no copc and no ne; one class only: no ne
    no_pos = CALIBRATION[:1] + [0.0] + CALIBRATION[2:]
    cal = _decode(Evaluation(bins=4), [POINTS, no_pos])
    assert list(cal) == ["auc", "logloss", "mean_pred", "base_rate", "brier", "ece", "mce"]
    all_pos = CALIBRATION[:1] + [10.0] + CALIBRATION[2:]
    assert list(_decode(Evaluation(bins=4), [POINTS, all_pos]))[-1] == "copc"


def test_grouped_bootstrap_with_empty_ks():
    from deepfm_amd.training.metrics import Evaluation
    req = Evaluation(ks=None, group_auc=True, replicates=R, grouped=True)
    got = _decode(req, [POINTS, GAUC, POOLED, OK, GROUPED_NO_KS, OK])
    _same(got, {"auc": 0.75, "logloss": 0.5, "gauc": 0.7, "uauc": 0.65, **BR.summary(POOLED, 0.95),
                **UR.summary(GROUPED_NO_KS, ["gauc", "uauc"], 0.95)})
    # compute_bootstrap_ranking's form: no pooled family, the points of the per-user metrics and their spread
    _same(_decode(req, [GAUC, GROUPED_NO_KS, OK], pooled=None),
          {"gauc": 0.7, "uauc": 0.65, **UR.summary(GROUPED_NO_KS, ["gauc", "uauc"], 0.95)})
    points, columns = _decode(req, [GAUC, GROUPED_NO_KS, OK], pooled=None, summarise=False)     # what compare_* takes
    assert points == {"gauc": 0.7, "uauc": 0.65} and list(columns) == ["gauc", "uauc"]
    assert np.array_equal(columns["uauc"], GROUPED_NO_KS[:, 1]) and np.isnan(columns["gauc"][1])


FAULTS = [
    ("ranking", 5, ["user ids outside [0, num_users)", None, "labels other than 0 and 1"]),
    ("gauc", 4, ["group ids outside [0, num_groups)", None, "labels other than 0 and 1"]),
    ("calibration", 7, ["slice ids outside [0, num_slices)", None, "scores outside [0, 1]", "labels other than 0 and 1"]),
    ("pooled", 0, [None, "labels other than 0 and 1", "unit ids outside [0, 2^40)"]),
    ("grouped", 0, ["user ids outside [0, num_users)", None, "labels other than 0 and 1"]),
]


@pytest.mark.parametrize("family, at, messages", FAULTS, ids=[f[0] for f in FAULTS])
def test_the_first_fault_of_each_family_raises_its_message(family, at, messages):
    import re
    from deepfm_amd.training.metrics import Evaluation
    req = Evaluation(ks=[1, 3], group_auc=True, bins=4, replicates=R, grouped=True)
    for first in range(len(messages)):
        host = {"ranking": list(RANKING), "gauc": list(GAUC), "calibration": list(CALIBRATION), "pooled": list(OK),
                "grouped": list(OK)}
        for j in range(first, len(messages)):                      # every later fault is set too: the first one speaks
            host[family][at + j] = 3.0 + j
        want = "Input contains NaN." if messages[first] is None else f"{3 + first} {messages[first]}"
        with pytest.raises(ValueError, match="^" + re.escape(want) + "$"):
            _decode(req, [POINTS, host["ranking"], host["gauc"], host["calibration"], POOLED, host["pooled"], GROUPED,
                          host["grouped"]])
        with pytest.raises(ValueError, match="^" + re.escape(want) + "$"):      # compare_* meets the same refusals
            _decode(req, [POINTS, host["ranking"], host["gauc"], host["calibration"], POOLED, host["pooled"], GROUPED,
                          host["grouped"]], summarise=False)


def test_one_read_decodes_any_number_of_evaluations():
    import torch
    from deepfm_amd.training.metrics import Evaluation, decode_evaluation, read_evaluations
    a, b = Evaluation(ks=[1, 3]), Evaluation(group_auc=True, replicates=R, grouped=True)
    t = lambda *parts: [torch.from_numpy(np.asarray(p, np.float64)) for p in parts]            # noqa: E731
    faults = torch.zeros(3, dtype=torch.int64)                                                  # integers travel too
    enqueued = [(t(POINTS, RANKING), lambda host, summarise=True: decode_evaluation(a, host, summarise=summarise), None),
                (t(POINTS, GAUC, POOLED) + [faults] + t(GROUPED_NO_KS, OK),
                 lambda host, summarise=True: decode_evaluation(b, host, summarise=summarise), None)]
    first, second = read_evaluations(enqueued)
    _same(first, _decode(a, [POINTS, RANKING]))
    _same(second, _decode(b, [POINTS, GAUC, POOLED, OK, GROUPED_NO_KS, OK]))
    (points, columns), _ = read_evaluations(enqueued, summarise=False)
    assert points == first and columns == {}


def test_delta_dict_is_both_loops_it_replaced():
    from deepfm_amd.training.metrics import _spread, delta_dict
    rng = np.random.default_rng(4)
    level = 0.9
    names = ["auc", "logloss"]
    va, vb = rng.random((R, 2)), rng.random((R, 2))
    vb[3, 1] = np.nan                                                # dropped, and counted out of logloss_b_better
    vb[0, 0] = va[0, 0]                                              # a zero delta is no improvement
    point_a, point_b = {"auc": 0.7, "logloss": 0.6}, {"auc": 0.72}  # a run without a point: NaN
    runs = [(p, dict(zip(names, v.T))) for p, v in ((point_a, va), (point_b, vb))]
    nan = float("nan")

    def loop(signs):                                                 # compare_bootstrap's loop, sign for log loss
        delta = vb - va
        out = {}
        for j, (name, sign) in enumerate(zip(names, signs)):
            a, b = point_a.get(name, nan), point_b.get(name, nan)
            se, lo, hi, used = _spread(delta[:, j], level)
            d = delta[:, j][~np.isnan(delta[:, j])]
            out.update({f"{name}_a": a, f"{name}_b": b, f"{name}_delta": b - a, f"{name}_delta_se": se,
                        f"{name}_delta_lo": lo, f"{name}_delta_hi": hi,
                        f"{name}_b_better": float(np.count_nonzero(sign * d > 0)) / used if used else nan})
        return out

    for signs in ((1.0, -1.0), (1.0, 1.0)):                          # the pooled metrics; the per-user ones (b higher)
        got, want = delta_dict(names, signs, *runs, level), loop(signs)
        assert list(got) == list(want) == [f"{m}_{k}" for m in names for k in
                                           ("a", "b", "delta", "delta_se", "delta_lo", "delta_hi", "b_better")]
        assert all(got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])) for k in want)
    d = delta_dict(names, (1.0, -1.0), *runs, level)
    delta = vb - va
    assert d["auc_b_better"] == np.count_nonzero(delta[:, 0] > 0) / R                           # the zero delta counts against
    kept = np.delete(delta[:, 1], 3)
    assert d["logloss_b_better"] == np.count_nonzero(kept < 0) / (R - 1)                        # lower is better
    assert d["logloss_delta_se"] == np.std(kept, ddof=1) and np.isnan(d["logloss_b"]) and np.isnan(d["logloss_delta"])
    assert d["auc_delta"] == 0.72 - 0.7 and d["auc_delta_lo"] == np.quantile(delta[:, 0], 0.05)
    empty = delta_dict(["auc"], [1.0], ({}, {"auc": np.full(R, np.nan)}), ({}, {"auc": np.zeros(R)}), level)
    assert all(np.isnan(v) for v in empty.values())
