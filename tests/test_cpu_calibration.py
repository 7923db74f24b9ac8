"""CPU: the calibration entry points are declared, exported and bound; the numpy restatement
(tests/calibration_reference.py) gives hand-computed answers and agrees with sklearn; ``calibration_dict``,
``downsampling_correction`` and the Trainer's refusals."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import calibration_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dfm_calibration_workspace_bytes", "dfm_calibration_route", "dfm_calibration"]
Q27 = 2.0 ** -27


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
    for name in ("calibration_device", "calibration_dict", "compute_calibration", "downsampling_correction"):
        assert hasattr(T, name), name


def test_workspace_bytes_and_route():
    from deepfm_amd import _lib
    lib = _lib.load()
    ws, route = lib.dfm_calibration_workspace_bytes, lib.dfm_calibration_route
    for k, s in ((0, 0), (-1, 5), (1025, 0), (10, -1), (10, (1 << 24) + 1)):
        assert ws(k, s) == 0 and route(k, s) == -1, (k, s)
    sizes = [ws(10, s) for s in (0, 1, 100, 10_000, 1 << 24)]
    assert sizes[0] >= 8 * (9 + 30) and all(a < b for a, b in zip(sizes, sizes[1:])) and all(b % 16 == 0 for b in sizes)
    assert sizes[-1] >= 32 << 24                          # four 64-bit sums per slice
    assert ws(1024, 0) >= 8 * (9 + 3 * 1024) > ws(1, 0) > 0
    # the switch: one slice count at which route 0 ends, for every bin count; the bins alone always fit
    for k in (1, 10, 1024):
        assert route(k, 0) == 0 and route(k, 1) == 0 and route(k, 1 << 24) == 1
        lo, hi = 1, 1 << 24
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if route(k, mid) == 0 else (lo, mid)
        assert all(route(k, s) == 0 for s in (lo - 1, lo)) and all(route(k, s) == 1 for s in (hi, hi + 1))
        assert lo >= 256                                  # a few hundred slices stay on chip even at 1024 bins


@pytest.mark.parametrize("change", ["null_out", "null_bins", "n0", "n_2_31", "bins0", "bins_big", "slices_neg",
                                    "slices_big", "ids_without_slices", "slices_without_ids", "slices_without_table",
                                    "ws_unaligned", "scores_unaligned"])
def test_bad_arguments_are_refused_before_any_launch(change):
    from deepfm_amd import _lib
    lib = _lib.load()
    fake = 1 << 20                                        # never dereferenced: every check runs before a launch
    a = dict(y=fake, s=fake, ids=fake, n=100, bins=10, slices=5, ws=fake, bt=fake, st=fake, out=fake)
    a.update({"null_out": dict(out=0), "null_bins": dict(bt=0), "n0": dict(n=0), "n_2_31": dict(n=1 << 31),
              "bins0": dict(bins=0), "bins_big": dict(bins=1025), "slices_neg": dict(slices=-1),
              "slices_big": dict(slices=(1 << 24) + 1), "ids_without_slices": dict(slices=0, st=0),
              "slices_without_ids": dict(ids=0), "slices_without_table": dict(st=0), "ws_unaligned": dict(ws=fake + 8),
              "scores_unaligned": dict(s=fake + 2)}[change])
    assert lib.dfm_calibration(a["y"], a["s"], a["ids"], a["n"], a["bins"], a["slices"], a["ws"], a["bt"], a["st"],
                               a["out"], None) == 1
    assert lib.dfm_last_error()


# ----------------------------------------------------------------------------- the restatement, by hand
def test_six_samples_by_hand():
    p = np.array([0.25, 0.75, 0.5, 0.125, 0.875, 0.5], np.float32)
    y = np.array([0, 1, 1, 0, 1, 0], np.float32)
    r = CR.calibration(y, p, bins=4)
    assert r["bins"].tolist() == [[1, 0, 0.125], [1, 0, 0.25], [2, 1, 1.0], [2, 2, 1.625]]
    out = r["out"]
    assert out[:4].tolist() == [6, 3, 0.5, 0.65625 / 6]
    assert out[5] == 0.75 / 6 and out[6] == 0.25          # gaps .125, .25, 0, .375; per count .125, .25, 0, .1875
    want_ll = (2 * -math.log(0.75) + 2 * -math.log(0.5) + 2 * -math.log(0.875)) / 6
    assert abs(out[4] - want_ll) <= Q27 / 2               # every term is rounded to a multiple of 2^-27
    assert out[7:].tolist() == [0, 0, 0, 0, 0] and r["slices"] is None
    d = CR.summary(r)
    assert d["mean_pred"] == 0.5 and d["base_rate"] == 0.5 and d["copc"] == 1.0 and d["brier"] == 0.109375
    assert abs(d["ne"] - want_ll / math.log(2)) <= Q27
    # with slices: 0 holds the first two samples, 2 the rest, 1 nothing
    r = CR.calibration(y, p, bins=4, slice_ids=[0, 0, 2, 2, 2, 2], num_slices=3)
    assert r["slices"][:, :3].tolist() == [[2, 1, 1.0], [0, 0, 0], [4, 2, 2.0]]
    assert abs(r["slices"][0, 3] - 2 * -math.log(0.75)) <= Q27 and r["slices"][1, 3] == 0
    assert np.array_equal(r["out"], out)


def test_one_class_and_no_positive():
    p = np.array([0.5, 0.25], np.float32)
    ones = CR.summary(CR.calibration(np.ones(2, np.float32), p, bins=2))
    assert "ne" not in ones and ones["copc"] == 0.375 and ones["base_rate"] == 1.0
    zeros = CR.summary(CR.calibration(np.zeros(2, np.float32), p, bins=2))
    assert "ne" not in zeros and "copc" not in zeros and zeros["base_rate"] == 0.0 and zeros["mean_pred"] == 0.375
    from deepfm_amd.training import calibration_dict
    for y in (np.ones(2, np.float32), np.zeros(2, np.float32)):
        r = CR.calibration(y, p, bins=2)
        assert calibration_dict(r["out"].tolist()) == CR.summary(r)


def test_scores_of_exactly_zero_and_one():
    p = np.array([0, 0, 1, 1], np.float32)
    y = np.array([0, 1, 0, 1], np.float32)
    r = CR.calibration(y, p, bins=10)
    assert r["bins"][0].tolist() == [2, 1, 0.0] and r["bins"][9].tolist() == [2, 1, 2.0]
    assert r["bins"][1:9].sum() == 0
    assert r["out"][:4].tolist() == [4, 2, 0.5, 0.5]      # the two wrong ones have squared error 1
    # the clipped terms: -log(1 - 2^-23) for the right ones, -log(2^-23) for the wrong ones
    L = CR.integers(y, p, 10)["glob"][4]
    assert L == 2 * 16 + 2 * int(np.rint(23 * math.log(2) * 2 ** 27))
    assert r["out"][5] == 0.5 and r["out"][6] == 0.5      # both bins: |sum p - positives| = 1 of 2 samples


def test_one_bin():
    rng = np.random.default_rng(0)
    p = rng.random(50).astype(np.float32)
    y = (rng.random(50) < 0.3).astype(np.float32)
    r = CR.calibration(y, p, bins=1)
    assert r["bins"].shape == (1, 3) and r["bins"][0, 0] == 50 and r["bins"][0, 1] == y.sum()
    gap = abs(r["bins"][0, 2] - y.sum())
    assert r["out"][5] == gap / 50 and r["out"][6] == gap / 50
    assert abs(r["out"][2] - p.astype(np.float64).mean()) <= 2.0 ** -33 + 1e-15


def test_faults_are_counted_and_enter_nothing_else():
    p = np.array([0.5, np.nan, 1.0000001, -0.0, -1e-9, 0.5, 0.5, 0.5, np.inf], np.float32)
    y = np.array([1, 0, 0, 0, 0, 0.5, 1, 0, 1], np.float32)
    sid = np.array([0, 0, 0, 1, 1, 1, -1, 2, 0])
    r = CR.calibration(y, p, bins=4, slice_ids=sid, num_slices=2)
    assert r["out"][7:].tolist() == [2, 1, 3, 1, 0]       # ids -1 and 2; one NaN; 1.0000001, -1e-9, inf; label 0.5
    assert r["out"][:2].tolist() == [2, 1]                # 0.5 / 1 in slice 0 and -0.0 / 0 in slice 1
    assert r["bins"].tolist() == [[1, 0, 0.0], [0, 0, 0], [1, 1, 0.5], [0, 0, 0]]
    assert r["slices"][:, :3].tolist() == [[1, 1, 0.5], [1, 0, 0.0]]


# ----------------------------------------------------------------------------- the restatement against sklearn
@pytest.mark.parametrize("seed,bins", [(0, 10), (1, 20), (2, 7)])
def test_restatement_matches_sklearn(seed, bins):
    from sklearn.calibration import calibration_curve
    from sklearn.metrics import brier_score_loss
    rng = np.random.default_rng(seed)
    n = 5_000
    p = (rng.beta(1.2, 6.0, n)).astype(np.float32)
    y = (rng.random(n) < p * 0.8).astype(np.float32)
    # a condition on the input: sklearn puts a score on an edge into the lower bin, the definition into the upper one
    edges = np.arange(1, bins) / bins
    assert np.abs(p.astype(np.float64)[:, None] - edges[None, :]).min() > 1e-6
    r = CR.calibration(y, p, bins=bins)
    frac_pos, mean_pred = calibration_curve(y, p.astype(np.float64), n_bins=bins, strategy="uniform")
    filled = r["bins"][:, 0] > 0
    assert filled.sum() == frac_pos.size
    assert np.abs(r["bins"][filled, 1] / r["bins"][filled, 0] - frac_pos).max() <= 1e-7
    assert np.abs(r["bins"][filled, 2] / r["bins"][filled, 0] - mean_pred).max() <= 1e-7
    assert abs(r["out"][3] - brier_score_loss(y, p.astype(np.float64))) <= 1e-9
    # ece and mce from sklearn's curve
    w = r["bins"][filled, 0] / n
    assert abs(r["out"][5] - float(np.sum(w * np.abs(frac_pos - mean_pred)))) <= 1e-7
    assert abs(r["out"][6] - float(np.max(np.abs(frac_pos - mean_pred)))) <= 1e-7
    # log loss: every term within half a quantum
    from sklearn.metrics import log_loss
    assert abs(r["out"][4] - log_loss(y, np.clip(p, 1e-7, 1 - 1e-7))) <= Q27


# ----------------------------------------------------------------------------- the host side of the package
def test_calibration_dict():
    from deepfm_amd.training import calibration_dict
    vals = [8.0, 2.0, 0.3, 0.2, 0.5, 0.05, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0]
    d = calibration_dict(vals)
    assert list(d) == ["mean_pred", "base_rate", "brier", "ece", "mce", "copc", "ne"]
    assert all(type(v) is float for v in d.values())
    assert d["mean_pred"] == 0.3 and d["base_rate"] == 0.25 and d["brier"] == 0.2
    assert d["ece"] == 0.05 and d["mce"] == 0.1
    assert d["copc"] == pytest.approx(0.3 * 8 / 2, rel=1e-15)
    assert d["ne"] == pytest.approx(0.5 / -(0.25 * math.log(0.25) + 0.75 * math.log(0.75)), rel=1e-15)
    assert list(calibration_dict([8.0, 0.0] + vals[2:])) == ["mean_pred", "base_rate", "brier", "ece", "mce"]
    assert list(calibration_dict([8.0, 8.0] + vals[2:])) == ["mean_pred", "base_rate", "brier", "ece", "mce", "copc"]
    for at, msg in ((7, r"^4 slice ids outside \[0, num_slices\)$"), (8, r"^Input contains NaN\.$"),
                    (9, r"^4 scores outside \[0, 1\]$"), (10, r"^4 labels other than 0 and 1$")):
        bad = list(vals)
        bad[at] = 4.0
        with pytest.raises(ValueError, match=msg):
            calibration_dict(bad)


def test_downsampling_correction():
    from deepfm_amd.training import downsampling_correction
    rng = np.random.default_rng(3)
    p = rng.random(1000)
    t = torch.from_numpy(p)
    for keep in (0.01, 0.2, 0.5):
        got = downsampling_correction(t, keep).numpy()
        assert got.dtype == np.float64
        # the same three operations in fp64; torch and numpy round each alike
        assert np.abs(got - p / (p + (1.0 - p) / keep)).max() <= 2.0 ** -52
        assert np.all(got <= p)
    # keep_rate 1: p / (p + (1 - p)), whose denominator is 1 up to two roundings
    assert np.abs(downsampling_correction(t, 1.0).numpy() - p).max() <= 2.0 ** -52
    ends = torch.tensor([0.0, 1.0], dtype=torch.float32)
    for keep in (0.05, 1.0):
        assert downsampling_correction(ends, keep).tolist() == [0.0, 1.0]
    assert downsampling_correction(ends, 0.5).dtype == torch.float32
    with pytest.raises(ValueError):
        downsampling_correction(t, 0.0)


def test_python_refuses_bad_arguments_before_any_device_work():
    from deepfm_amd.training import compute_calibration
    with pytest.raises(TypeError):
        compute_calibration([0, 1, 0], [0.1, 0.2, 0.3])                                       # scores: no list


@pytest.mark.parametrize("metric", ["ne", "ece", "mce", "brier", "copc"])
def test_trainer_refuses_to_watch_a_calibration_number(metric):
    from deepfm_amd.training.trainer import check_calibration
    with pytest.raises(ValueError, match="maximise"):
        check_calibration(metric, 10, None, None)


def test_trainer_refusals_around_the_slice_field_and_what_it_passes_on():
    from deepfm_amd.config import ExperimentConfig, TrainingConfig
    from deepfm_amd.data.device_epoch import DeviceEpochLoader
    from deepfm_amd.data.schema import FeatureType
    from deepfm_amd.training import Trainer
    from deepfm_amd.training.trainer import check_calibration
    from deepfm_amd.data.synthetic import schema_from_fields
    schema = schema_from_fields([dict(name="user_id", type="sparse", vocab=50, dim=8, max_len=1, combiner="mean"),
                                 dict(name="age", type="dense", vocab=0, dim=8, max_len=1, combiner="mean")])
    assert schema.fields["age"].feature_type is FeatureType.DENSE
    check_calibration("auc", 10, "user_id", schema)
    check_calibration("auc", 0, None, schema)
    for bins, field in ((10, "age"), (10, "no_such_field"), (0, "user_id"), (1025, None), (-1, None)):
        with pytest.raises(ValueError):
            check_calibration("auc", bins, field, schema)
    calls = []

    class Pred:
        def evaluate_loader(self, loader, **kw):
            calls.append(kw)
            return {"auc": 0.5}

    loader = DeviceEpochLoader.__new__(DeviceEpochLoader)
    loader.batch_size = 8
    t = Trainer.__new__(Trainer)
    t.config = ExperimentConfig(training=TrainingConfig(metric="auc", ranking_ks=[1, 5]))
    t._predictor = lambda b: Pred()
    t.calibration_bins, t.slice_field = 0, None
    t.evaluate(loader)
    assert calls[-1] == {"ranking_ks": [1, 5], "group_auc": False}
    t.calibration_bins, t.slice_field = 20, "genre"
    t.evaluate(loader)
    assert calls[-1] == {"ranking_ks": [1, 5], "group_auc": False, "calibration_bins": 20, "slice_field": "genre"}
