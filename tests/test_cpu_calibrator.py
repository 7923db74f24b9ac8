"""CPU: the numpy restatement of the calibrators (tests/calibrator_reference.py) agrees with sklearn; the five entry
points are declared, exported and bound; ``Calibrator`` and the Trainer refuse bad arguments before any device call."""
import os
import re

import numpy as np
import pytest

from tests import calibrator_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"dfm_platt_workspace_bytes": 1, "dfm_platt_fit": 10, "dfm_isotonic_workspace_bytes": 1,
           "dfm_isotonic_fit": 9, "dfm_calibrate_apply": 6}


# ----------------------------------------------------------------------------- the restatement against sklearn
@pytest.mark.parametrize("case", R.CASES, ids=[f"rate{c[0]}" for c in R.CASES])
def test_platt_restatement_matches_sklearn(case):
    linear_model = pytest.importorskip("sklearn.linear_model")
    y, z = R.synthetic(case, 20_000)
    assert 0 < y.sum() < y.size
    a, b, iterations = R.platt_newton(y, z)
    assert iterations < 50
    lr = linear_model.LogisticRegression(C=1e12, tol=1e-12, max_iter=10_000).fit(z.astype(np.float64)[:, None], y)
    print(f"restatement ({a!r}, {b!r}) in {iterations} iterations; sklearn ({lr.coef_[0, 0]!r}, {lr.intercept_[0]!r})")
    assert abs(a - lr.coef_[0, 0]) <= 1e-6 and abs(b - lr.intercept_[0]) <= 1e-6
    # the fit is near the truth the data were drawn from
    assert abs(a - case[1]) <= 0.15 * case[1] + 0.05 and abs(b - case[2]) <= 0.4


@pytest.mark.parametrize("bins", [16, 256, 1024])
def test_pav_restatement_matches_sklearn(bins):
    isotonic = pytest.importorskip("sklearn.isotonic")
    y, z = R.synthetic(R.CASES[2], 50_000)
    z = (z * np.float32(0.5)).astype(np.float32)              # a model whose scores are too flat: real pooling work
    table, hdr = R.histogram(y, z, bins)
    assert hdr == [y.size, int(y.sum()), 0, 0] and table[:, 0].sum() == y.size
    x, v, blocks = R.pav(table)
    filled = table[:, 0] > 0
    assert x.size == filled.sum() and 1 <= blocks <= x.size and np.all(np.diff(x) > 0) and np.all(np.diff(v) >= 0)
    rate = table[filled, 1] / table[filled, 0]
    iso = isotonic.IsotonicRegression(out_of_bounds="clip").fit(x, rate, sample_weight=table[filled, 0])
    grid = np.linspace(-20.0, 20.0, 4001)
    err = np.abs(np.interp(grid, x, v) - iso.predict(grid)).max()
    print(f"K = {bins}: {x.size} knots, {blocks} blocks, max |restatement - sklearn| = {err:.3e}")
    assert err <= 1e-12


def test_restatement_by_hand():
    y = np.array([0, 1, 0, 1, 1, 0.5, 1], np.float32)
    z = np.array([-3.0, -1.0, 1.0, 3.0, 100.0, 0.0, np.nan], np.float32)
    table, hdr = R.histogram(y, z, 4, -4.0, 4.0)               # bins of width 2; 100 is clamped to 4: the last bin
    assert hdr == [5, 3, 1, 1]
    assert table.tolist() == [[1, 0, -3 << 24], [1, 1, -1 << 24], [1, 0, 1 << 24], [2, 2, 7 << 24]]
    x, v, blocks = R.pav(table)
    assert x.tolist() == [-3.0, -1.0, 1.0, 3.5] and v.tolist() == [0.0, 0.5, 0.5, 1.0] and blocks == 3
    q = R.isotonic_apply(x, v, np.array([-9, -3, -2, -1, 0, 1, 2.25, 3.5, 9, -np.inf, np.inf, np.nan], np.float32))
    assert q[:11].tolist() == [0, 0, 0.25, 0.5, 0.5, 0.5, 0.75, 1, 1, 0, 1] and np.isnan(q[11])
    # ties are not pooled: equal neighbours stay separate blocks
    assert R.pav(np.array([[2, 1, 0], [4, 2, 9]]))[2] == 2


# ----------------------------------------------------------------------------- binding and argument checks
def test_entry_points_are_declared_exported_and_bound():
    from deepfm_amd import _lib
    import deepfm_amd.training as T
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepfm_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, count in SYMBOLS.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert decl is not None and name in _lib.SIGNATURES and hasattr(lib, name), name
        args = decl.group(1)
        assert len(args.split(",")) == count == len(_lib.SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    assert re.search(rf"#define DFM_ABI_VERSION {_lib.ABI_VERSION}\b", header)
    assert len(_lib.SIGNATURES["dfm_predict_head"][1]) == 11
    assert _lib.SIGNATURES["dfm_calibrate_apply"][1][-1] is _lib.LaunchArg
    assert hasattr(T, "Calibrator")
    assert lib.dfm_platt_workspace_bytes(0) == 0 and lib.dfm_platt_workspace_bytes(1 << 31) == 0
    assert 0 < lib.dfm_platt_workspace_bytes(1) < lib.dfm_platt_workspace_bytes(1 << 20) == \
        lib.dfm_platt_workspace_bytes((1 << 31) - 1)
    assert lib.dfm_isotonic_workspace_bytes(0) == 0 and lib.dfm_isotonic_workspace_bytes(1025) == 0
    assert lib.dfm_isotonic_workspace_bytes(1024) == 8 * (8 + 3 * 1024)
    assert _lib.ISOTONIC_KNOT_BYTES == int(re.search(r"DFM_ISOTONIC_KNOT_BYTES \(64 \+ (\d+) \*", header).group(1)) * \
        _lib.ISOTONIC_MAX_BINS + 64


@pytest.mark.parametrize("kwargs", [dict(bins=0), dict(bins=1025), dict(z_range=(-65.0, 16.0)),
                                    dict(z_range=(-16.0, 64.5)), dict(z_range=(2.0, 2.0)), dict(z_range=(3.0, -3.0)),
                                    dict(kind="beta"), dict(max_rounds=0), dict(gtol=-1.0)],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_calibrator_refuses_bad_arguments_before_any_device_call(kwargs, monkeypatch):
    import torch
    from deepfm_amd import _lib
    from deepfm_amd.training import Calibrator

    def no_device(*a, **k):
        raise AssertionError("a device call before the argument check")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(torch, "zeros", no_device)
    kw = dict(kind="isotonic")
    kw.update(kwargs)
    with pytest.raises(ValueError):
        Calibrator(kw.pop("kind"), **kw)


@pytest.mark.parametrize("change", ["launch", "kind", "null", "n0", "n_2_31", "params_unaligned", "logits_unaligned"])
def test_apply_refuses_bad_arguments_before_any_launch(change):
    from deepfm_amd import _lib
    lib = _lib.load()
    P = 1 << 20                                               # never dereferenced
    a = dict(kind=0, params=P, z=P, n=64, q=2 * P, at=None)
    a.update({"launch": dict(at=_lib.Launch(None, None, P)), "kind": dict(kind=2), "null": dict(q=0), "n0": dict(n=0),
              "n_2_31": dict(n=1 << 31), "params_unaligned": dict(params=P + 8),
              "logits_unaligned": dict(z=P + 2)}[change])
    assert lib.dfm_calibrate_apply(a["kind"], a["params"], a["z"], a["n"], a["q"], a["at"]) == 1
    assert ("launch destination" in lib.dfm_last_error().decode()) == (change == "launch")


@pytest.mark.parametrize("fit,change", [(f, c) for f in ("platt", "isotonic")
                                        for c in ("n0", "n_2_31", "ws_unaligned", "null_state", "labels_unaligned")] +
                         [("platt", c) for c in ("rounds0", "gtol_nan")] +
                         [("isotonic", c) for c in ("bins0", "bins_big", "range_wide", "range_empty")])
def test_fits_refuse_bad_arguments_before_any_launch(fit, change):
    """Only the call that the change makes invalid is made: the pointers are fake."""
    from deepfm_amd import _lib
    lib = _lib.load()
    P = 1 << 20
    a = dict(y=P, n=100, rounds=32, gtol=1e-9, ws=P, state=P, bins=16, lo=-16.0, hi=16.0)
    a.update({"n0": dict(n=0), "n_2_31": dict(n=1 << 31), "rounds0": dict(rounds=0), "gtol_nan": dict(gtol=float("nan")),
              "ws_unaligned": dict(ws=P + 8), "null_state": dict(state=0), "bins0": dict(bins=0),
              "bins_big": dict(bins=1025), "range_wide": dict(hi=64.5), "range_empty": dict(lo=16.0),
              "labels_unaligned": dict(y=P + 2)}[change])
    if fit == "platt":
        rc = lib.dfm_platt_fit(a["y"], P, a["n"], 1, 0, a["rounds"], a["gtol"], a["ws"], a["state"], None)
    else:
        rc = lib.dfm_isotonic_fit(a["y"], P, a["n"], a["bins"], a["lo"], a["hi"], a["ws"], a["state"], None)
    assert rc == 1 and lib.dfm_last_error()


# ----------------------------------------------------------------------------- the Trainer
def test_trainer_refuses_an_unknown_calibrator():
    from deepfm_amd.training import Trainer
    with pytest.raises(ValueError, match="bogus"):
        Trainer(None, None, None, None, None, None, calibrator="bogus")
