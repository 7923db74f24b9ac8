"""GPU: the score calibrators (csrc/calibrator.hip, training/calibrator.py) against the numpy restatement
(tests/calibrator_reference.py).

Bit-exact: the isotonic bin table (integer sums), its independence of the sample order, the fp64 knots (ratios of
integer sums), the isotonic apply (float32, one rounding per operation), two Platt fits of the same input, the
predictors' calibrated output against ``Calibrator.apply`` of their raw logits.  Toleranced: the Platt parameters
(through the restatement's fp64 gradient at the returned point, ``2 * gtol``: the device adds its partial sums in
another order than numpy, which moves a mean by about 1e-15) and the Platt apply (``expf``)."""
import gc
import json
import warnings

import numpy as np
import pytest
import torch

from tests import calibrator_reference as R
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

GTOL = 1e-9
PLATT_CHUNK, ISO_CHUNK = 1024, 4096            # samples per workgroup and walk of the Platt passes / the histogram
SIZES = [1, 7, PLATT_CHUNK - 1, PLATT_CHUNK, PLATT_CHUNK + 1, ISO_CHUNK - 1, ISO_CHUNK, ISO_CHUNK + 1,
         3 * ISO_CHUNK + 5, 100_003]
# (labels, logits) offsets in elements from a 16-byte aligned base: aligned; a scalar head of 3; of 1; never aligned
OFFSETS = [(0, 0), (1, 1), (3, 3), (0, 1), (1, 3)]


@pytest.fixture(autouse=True)
def _collect_dead_cycles_here():
    yield
    gc.collect()


def _view(x, offset):
    """A device view of ``x`` that starts ``offset`` elements past a 16-byte aligned address."""
    base = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    v = base[offset:offset + x.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    return v


def _data(n, case=3):
    """(labels, logits) of n samples with both classes and no perfect separation (n >= 7)."""
    if n == 7:
        return np.array([0, 1, 0, 0, 1, 0, 1], np.float32), np.array([-1.5, -1, -.5, 0, .5, 1, 1.5], np.float32)
    y, z = R.synthetic(R.CASES[case], n)
    assert 0 < y.sum() < n
    return y, z


def _platt(y, z, offsets=(0, 0), **kw):
    from deepfm_amd.training import Calibrator
    cal = Calibrator("platt", **kw)
    cal.fit(_view(y, offsets[0]), _view(z, offsets[1]))
    return cal


def _check_platt(cal, y, z, fit_slope=True, smooth=False):
    rep = cal.report()
    a, b = rep["a"], rep["b"]
    assert rep["status"] == "converged" and 1 <= rep["rounds"] <= cal.max_rounds, rep
    assert rep["positives"] == int(y.sum()) and rep["negatives"] == int((y == 0).sum())
    F, g, _ = R.platt_terms(a, b, z, R.platt_targets(y, smooth))
    print(f"n = {y.size}: (a, b) = ({a!r}, {b!r}) in {rep['rounds']} rounds, restatement g = {g.tolist()}")
    if fit_slope:
        assert np.abs(g).max() <= 2 * GTOL
    else:
        assert a == 1.0 and abs(g[1]) <= 2 * GTOL
    # the log loss against the fit's targets (the labels, or Platt's smoothed ones) is no worse than the identity's
    F0 = R.platt_terms(1.0, 0.0, z, R.platt_targets(y, smooth))[0]
    assert F <= F0
    # the state block's own account of the two
    assert abs(rep["logloss_after"] - F) <= 1e-12 and abs(rep["logloss_before"] - F0) <= 1e-12
    assert rep["logloss_after"] <= rep["logloss_before"]
    return rep


# ----------------------------------------------------------------------------- Platt
@pytest.mark.parametrize("n", SIZES[1:])
def test_platt_sizes_and_alignments(n):
    y, z = _data(n)
    for offsets in OFFSETS:
        _check_platt(_platt(y, z, offsets), y, z)


@pytest.mark.parametrize("case", range(5))
def test_platt_synthetic_cases(case):
    y, z = R.synthetic(R.CASES[case], 100_003)
    rep = _check_platt(_platt(y, z), y, z)
    a, b, _ = R.platt_newton(y, z)
    assert abs(rep["a"] - a) <= 1e-6 and abs(rep["b"] - b) <= 1e-6
    _check_platt(_platt(y, z, fit_slope=False), y, z, fit_slope=False)
    _check_platt(_platt(y, z, smooth=True), y, z, smooth=True)


def test_platt_two_fits_leave_identical_state_blocks():
    y, z = R.synthetic(R.CASES[2], 100_003)
    dy, dz = _view(y, 1), _view(z, 1)
    from deepfm_amd.training import Calibrator
    one, two = Calibrator("platt").fit(dy, dz), Calibrator("platt").fit(dy, dz)
    first = one.params.clone()
    assert torch.equal(first.view(torch.int64), two.params.view(torch.int64))
    one.fit(dy, dz)                                        # a refit in place, over the previous state
    assert torch.equal(first.view(torch.int64), one.params.view(torch.int64))
    assert one.report()["status"] == "converged"


def test_platt_separable():
    y, z = R.SEPARABLE
    rep = _check_platt(_platt(y, z), y, z)                 # F falls towards 0, the gradient with it
    assert rep["a"] > 10 and rep["logloss_after"] < 1e-8
    rep = _check_platt(_platt(y, z, smooth=True), y, z, smooth=True)
    a, b, _ = R.platt_newton(y, z, smooth=True)
    assert abs(rep["a"] - a) <= 1e-6 and abs(rep["b"] - b) <= 1e-6


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_platt_single_class(label):
    z = R.synthetic(R.CASES[2], 2000)[1]
    for n in (1, 2000):
        y = np.full(n, label, np.float32)
        cal = _platt(y, z[:n])
        with pytest.warns(UserWarning, match="single class"):
            rep = cal.report()
        assert (rep["status"], rep["a"], rep["b"], rep["rounds"]) == ("single_class", 1.0, 0.0, 0)
        assert rep["positives"] + rep["negatives"] == n


def test_platt_constant_logits():
    y = (np.arange(1000) % 4 == 0).astype(np.float32)
    z = np.full(1000, 0.7, np.float32)
    cal = _platt(y, z)
    with pytest.warns(UserWarning, match="slope"):
        rep = cal.report()
    assert rep["status"] == "converged" and rep["slope_unidentified"] and rep["a"] == 1.0
    g = R.platt_terms(1.0, rep["b"], z, y.astype(np.float64))[1]
    assert abs(g[1]) <= 2 * GTOL
    assert abs(rep["b"] - (np.log(0.25 / 0.75) - np.float64(np.float32(0.7)))) <= 1e-8


@pytest.mark.parametrize("fault", ["nan", "inf", "label"])
def test_platt_bad_input(fault):
    y, z = R.synthetic(R.CASES[2], 5000)
    y, z = y.copy(), z.copy()
    if fault == "label":
        y[[17, 4097]] = 0.5
    else:
        z[4999] = np.nan if fault == "nan" else -np.inf
    cal = _platt(y, z, (1, 3))
    want = "0 non-finite logits, 2 labels" if fault == "label" else "1 non-finite logits, 0 labels"
    with pytest.raises(ValueError, match=want):
        cal.report()
    state = cal.params.cpu().tolist()
    assert state[:2] == [1.0, 0.0] and state[5] == 0 and state[6] == 3
    probe = torch.linspace(-5, 5, 64, device="cuda")
    assert_close(cal.apply(probe).cpu().numpy(), R.platt_apply_fp64(1.0, 0.0, probe.cpu().numpy()), what="identity")


@pytest.mark.parametrize("offsets", [(0, 0), (1, 1), (0, 1), (3, 2)])
def test_platt_apply(offsets):
    y, z = R.synthetic(R.CASES[4], 3000)
    cal = _platt(y, z)
    rep = cal.report()
    rng = np.random.default_rng(5)
    for n in (1, 7, PLATT_CHUNK - 1, PLATT_CHUNK + 1, 5 * PLATT_CHUNK + 3):
        probe = rng.normal(0, 4, n).astype(np.float32)
        probe[-3:] = [-90, 90, 0][-min(n, 3):]
        src = _view(probe, offsets[0])
        out = torch.full((n + 8,), -1.0, device="cuda")
        lo = 4 + offsets[1]
        dst = out[lo:lo + n]
        got = cal.apply(src, out=dst)
        assert got.data_ptr() == dst.data_ptr()
        assert_close(got.cpu().numpy(), R.platt_apply_fp64(np.float32(rep["a"]), np.float32(rep["b"]), probe),
                     what=f"platt apply n={n}")
        guard = out.cpu().numpy()
        assert (guard[:lo] == -1).all() and (guard[lo + n:] == -1).all()      # nothing outside the n elements


# ----------------------------------------------------------------------------- isotonic
def _iso_data(n, case):
    y, z = _data(n, case) if n > 1 else (np.ones(1, np.float32), np.array([0.3], np.float32))
    return y, (z * np.float32(0.5)).astype(np.float32)     # too flat a model: neighbours get pooled


def _knots(cal):
    """(m, x32, v32, x, v) as stored in the knot table."""
    raw = cal.params.cpu()
    m = int(raw[:8].view(torch.int64)[0])
    x32, v32 = raw[64:64 + 4096].view(torch.float32).numpy(), raw[64 + 4096:64 + 8192].view(torch.float32).numpy()
    x, v = raw[64 + 8192:64 + 16384].view(torch.float64).numpy(), raw[64 + 16384:].view(torch.float64).numpy()
    for arr in (x32, v32, x, v):
        assert not arr[m:].any()
    return m, x32[:m], v32[:m], x[:m], v[:m]


def _probes(x32, lo, hi, rng):
    edge = np.array([lo, hi, -np.inf, np.inf, np.nan, lo - 1, hi + 1, 0.0, -0.0], np.float32)
    below = np.nextafter(x32[:1], np.float32(-np.inf))
    above = np.nextafter(x32[-1:], np.float32(np.inf))
    between = rng.uniform(x32[0] - 1, x32[-1] + 1, 700).astype(np.float32)
    return np.concatenate([edge, x32, below, above, np.nextafter(x32, np.float32(np.inf)), between])


def _check_isotonic(y, z, bins, offsets=(0, 0), z_range=(-16.0, 16.0), seed=0):
    from deepfm_amd.training import Calibrator
    cal = Calibrator("isotonic", bins=bins, z_range=z_range)
    cal.fit(_view(y, offsets[0]), _view(z, offsets[1]))
    want_table, want_hdr = R.histogram(y, z, bins, *z_range)
    table = cal.bin_table().cpu().numpy()
    assert np.array_equal(table, want_table)
    rep = cal.report()
    m, x32, v32, x, v = _knots(cal)
    want_x, want_v, want_blocks = R.pav(want_table)
    assert m == want_x.size == rep["knots"] and rep["blocks"] == want_blocks
    assert np.array_equal(x.view(np.int64), want_x.view(np.int64))
    assert np.array_equal(v.view(np.int64), want_v.view(np.int64))
    assert np.array_equal(rep["knots_x"], want_x) and np.array_equal(rep["knots_v"], want_v)
    assert np.array_equal(x32, want_x.astype(np.float32)) and np.array_equal(v32, want_v.astype(np.float32))
    assert [rep["samples"], rep["positives"], rep["nonfinite_logits"], rep["bad_labels"]] == want_hdr
    # the order of the samples does not matter, bit for bit
    rng = np.random.default_rng(seed)
    perm = rng.permutation(y.size)
    again = Calibrator("isotonic", bins=bins, z_range=z_range).fit(_view(y[perm], offsets[1]), _view(z[perm], offsets[0]))
    assert np.array_equal(again.bin_table().cpu().numpy(), want_table)
    assert torch.equal(again.params, cal.params)
    # the apply, bit for bit, and its shape
    probe = _probes(x32, np.float32(z_range[0]), np.float32(z_range[1]), rng)
    got = cal.apply(_view(probe, offsets[0])).cpu().numpy()
    want = R.isotonic_apply(want_x, want_v, probe)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    finite = ~np.isnan(probe)
    assert np.isnan(got[~finite]).all() and (got[finite] >= 0).all() and (got[finite] <= 1).all()
    order = np.argsort(probe[finite], kind="stable")
    assert (np.diff(got[finite][order]) >= 0).all()
    return cal, rep


@pytest.mark.parametrize("bins", [1, 16, 1024])
@pytest.mark.parametrize("n", SIZES)
def test_isotonic_sizes_and_alignments(n, bins):
    y, z = _iso_data(n, 3)
    for offsets in OFFSETS if bins == 16 else OFFSETS[:1] + OFFSETS[3:4]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                # n = 1 is a single class
            _check_isotonic(y, z, bins, offsets)


@pytest.mark.parametrize("bins", [16, 256, 1024])
@pytest.mark.parametrize("case", [0, 2, 4])
def test_isotonic_synthetic_cases(case, bins):
    """Case 0's logits reach far below z_lo (clamped into the first bin), case 4's crowd into a few bins."""
    y, z = R.synthetic(R.CASES[case], 100_003)
    cal, rep = _check_isotonic(y, z, bins)
    assert rep["status"] == "converged" and rep["blocks"] <= rep["knots"] <= bins
    if case == 0:
        assert (z < -16).mean() > 0.5 and cal.bin_table()[0, 0].item() >= (z < -16).sum()


def test_isotonic_narrow_range_and_values_on_the_edges():
    rng = np.random.default_rng(2)
    z = np.concatenate([np.arange(-64, 65) / 16.0, rng.normal(0, 3, 3000)]).astype(np.float32)   # on the bin edges
    y = (rng.random(z.size) < 1 / (1 + np.exp(-0.5 * z))).astype(np.float32)
    _check_isotonic(y, z, 64, (1, 1), z_range=(-4.0, 4.0))
    _check_isotonic(y, z, 1000, (0, 1), z_range=(-64.0, 64.0))
    _check_isotonic(y, z, 7, (3, 3), z_range=(-1.0, 2.5))


def test_isotonic_one_filled_bin_is_a_constant():
    y = (np.arange(500) % 5 == 0).astype(np.float32)
    z = np.full(500, 1.25, np.float32)
    cal, rep = _check_isotonic(y, z, 1024)
    assert rep["knots"] == 1 and rep["knots_v"].tolist() == [0.2] and rep["knots_x"].tolist() == [1.25]
    out = cal.apply(torch.linspace(-30, 30, 999, device="cuda"))
    assert (out == float(np.float32(0.2))).all()


def test_isotonic_decreasing_data_pool_into_one_block():
    z = np.linspace(-8, 8, 4001).astype(np.float32)
    y = (z < 0).astype(np.float32)                          # the wrong way round: everything is pooled
    cal, rep = _check_isotonic(y, z, 256, z_range=(-8.0, 8.0))
    assert rep["blocks"] == 1 and rep["knots"] == 256 and set(rep["knots_v"].tolist()) == {2000 / 4001}


def test_isotonic_faults_are_counted_and_not_used():
    y, z = R.synthetic(R.CASES[2], 9000)
    y, z = y.copy(), z.copy()
    z[[0, 4096, 8999]] = [np.nan, np.inf, -np.inf]
    y[[5, 8998]] = [2.0, 0.5]
    from deepfm_amd.training import Calibrator
    cal = Calibrator("isotonic", bins=16).fit(_view(y, 3), _view(z, 3))
    table, hdr = R.histogram(y, z, 16)
    assert hdr[2:] == [3, 2] and np.array_equal(cal.bin_table().cpu().numpy(), table)
    with pytest.raises(ValueError, match="3 non-finite logits, 2 labels"):
        cal.report()
    one = Calibrator("isotonic", bins=16).fit(np.zeros(300, np.float32), z[100:400])
    with pytest.warns(UserWarning, match="single class"):
        assert one.report()["status"] == "single_class"
    assert (one.apply(torch.linspace(-3, 3, 50, device="cuda")) == 0).all()


# ----------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("kind", ["platt", "isotonic"])
def test_state_dict_round_trip(kind, tmp_path):
    from deepfm_amd.training import Calibrator
    y, z = R.synthetic(R.CASES[2], 5000)
    cal = Calibrator(kind, bins=64).fit(y, z)
    torch.save(cal.state_dict(), tmp_path / "cal.pt")
    fresh = Calibrator(kind, bins=64)
    address = fresh.params.data_ptr()
    fresh.load_state_dict(torch.load(tmp_path / "cal.pt", weights_only=True))
    assert fresh.params.data_ptr() == address and torch.equal(fresh.params, cal.params)
    probe = torch.linspace(-9, 9, 1001, device="cuda")
    assert torch.equal(fresh.apply(probe), cal.apply(probe))
    with pytest.raises(ValueError):
        Calibrator("isotonic" if kind == "platt" else "platt").load_state_dict(cal.state_dict())


# ----------------------------------------------------------------------------- the predictors
B = 64


def _uniform_model():
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.synthetic import schema_from_fields
    from deepfm_amd.models import create_model
    D = 16
    fields = [dict(name="user_id", type="sparse", vocab=200, dim=D, max_len=1, combiner="mean"),
              dict(name="item_id", type="sparse", vocab=500, dim=D, max_len=1, combiner="mean"),
              dict(name="genre", type="sparse", vocab=20, dim=D, max_len=1, combiner="mean"),
              dict(name="age", type="dense", vocab=0, dim=D, max_len=1, combiner="mean")]
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = D
    cfg.dnn.hidden_units = [32, 16]
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = create_model("deepfm", schema_from_fields(fields), cfg)
    with torch.no_grad():
        for mod in model.dnn.mlp:
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.uniform_(-0.1, 0.1)
                mod.running_var.uniform_(0.5, 2.0)
        for p in model.parameters():                       # logits with some spread
            p.mul_(3.0)
    return fields, model


def _setup(which):
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FusedPredictor, MixedSchemaPredictor
    from tests.helpers import random_fields_batch
    if which == "uniform":
        fields, model = _uniform_model()
        cls = FusedPredictor
    else:
        from tests.test_gpu_mixed_predict import _movielens_model
        fields, model = _movielens_model("deepfm", seed=5)
        cls = MixedSchemaPredictor
    n = 5 * B + 17
    rng = np.random.default_rng(21)
    feats = random_fields_batch(fields, n, rng)
    labels = (rng.random(n) < 0.3).astype(np.float32)
    return model, cls, PackedColumns(model.schema, feats, labels)


def _record(pred, cols, start=0):
    host = np.zeros(pred.record_bytes, np.uint8)
    pred.layout.write(host, cols, start, start + B)
    return torch.from_numpy(host).cuda()


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("which", ["uniform", "movielens"])
def test_predictor_applies_the_calibrator_inside_its_launch(which, use_graph):
    from deepfm_amd.training import Calibrator
    model, cls, cols = _setup(which)
    before = cls(model, B, use_graph=use_graph)            # built before any calibrator of this test exists
    rec, rec2 = _record(before, cols), _record(before, cols, B)
    p_before = before.predict_from(rec)
    labels, logits = before.collect_logits(cols)
    assert torch.equal(labels.cpu(), torch.from_numpy(cols.labels)) and logits.shape == labels.shape
    for kind in ("platt", "isotonic"):
        cal = Calibrator(kind, bins=32).fit(labels, logits)
        pred = cls(model, B, use_graph=use_graph, calibrator=cal)
        raw = cls(model, B, use_graph=use_graph)
        assert raw.raw_probs is None and all(s.at["apply"] is None for s in raw.slots)
        assert torch.equal(raw.predict_from(rec), p_before)            # without the keyword nothing changes
        for r, valid in ((rec, None), (rec2, 37), (rec, 1)):
            got = pred.predict_from(r, valid)
            raw.predict_from(r, valid)
            z = raw.last_logits(valid or B)
            assert torch.equal(got, cal.apply(z)) and torch.equal(pred.last_logits(valid or B), z)
        # a refit with other data re-aims the captured graphs: no re-capture
        old = pred.predict_from(rec)
        cal.fit(1.0 - labels, logits * 0.5 + 0.25)
        new = pred.predict_from(rec)
        raw.predict_from(rec)
        assert torch.equal(new, cal.apply(raw.last_logits())) and not torch.equal(new, old)


def test_evaluate_scores_calibrated_probabilities():
    from deepfm_amd.training import Calibrator
    model, cls, cols = _setup("uniform")
    raw = cls(model, B)
    labels, logits = raw.collect_logits(cols)
    m_raw = raw.evaluate(cols, calibration_bins=20)
    # collect_logits returned what evaluate scored: the head's own sigmoid of these logits, and the labels
    identity = Calibrator("platt")
    assert torch.equal(identity.apply(logits), raw.last_scores) and torch.equal(labels, raw.last_labels)
    cal = Calibrator("platt").fit(labels, logits)
    assert cal.report()["status"] == "converged"
    pred = cls(model, B, calibrator=cal)
    m = pred.evaluate(cols, calibration_bins=20)
    print(f"raw copc {m_raw['copc']!r} logloss {m_raw['logloss']!r}; calibrated copc {m['copc']!r} logloss "
          f"{m['logloss']!r}")
    assert abs(m["copc"] - 1.0) <= 1e-5
    assert m["logloss"] <= m_raw["logloss"] + 1e-7
    assert torch.equal(pred.last_scores, cal.apply(logits))
    # the loader route scores the same samples, and collects the same logits
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    assert pred.evaluate_loader(loader, calibration_bins=20) == m
    l2, z2 = pred.collect_logits(loader)
    assert torch.equal(l2, labels) and torch.equal(z2, logits)       # raw, calibrator or not


def test_quantized_predictor_takes_the_calibrator():
    from deepfm_amd.training import Calibrator, QuantizedPredictor
    model, _, cols = _setup("uniform")
    raw = QuantizedPredictor(model, B)
    labels, logits = raw.collect_logits(cols)
    cal = Calibrator("isotonic", bins=16).fit(labels, logits)
    pred = QuantizedPredictor(model, B, tables=raw.tables, calibrator=cal)
    rec = _record(raw, cols)
    raw.predict_from(rec)
    assert torch.equal(pred.predict_from(rec), cal.apply(raw.last_logits()))


# ----------------------------------------------------------------------------- the Trainer
def test_trainer_fits_saves_and_reports_the_calibrator(tmp_path):
    import deepfm_amd.training as T
    from tests.test_gpu_trainer import _trainer_config, _trainer_data, _trainer_model
    cfg = _trainer_config(tmp_path / "run", num_epochs=1)
    schema, (train, val, test) = _trainer_data(cfg)
    trainer = T.Trainer(_trainer_model(schema, cfg), schema, cfg, train, val, test, calibrator="platt")
    trainer.train()
    with open(tmp_path / "run" / "results.json") as f:
        res = json.load(f)
    tm = res["test_metrics"]
    raw_keys = [k for k in tm if not k.startswith("calibrated_")]
    assert {"auc", "logloss", "HR@1"} <= set(raw_keys) and sorted(tm) == sorted(raw_keys + ["calibrated_" + k for k in raw_keys])
    assert not any(k.startswith("calibrated_") for k in res["val_metrics"])
    assert (tmp_path / "run" / "best_model.pt").exists()
    fresh = T.Calibrator("platt").load_state_dict(torch.load(tmp_path / "run" / "calibrator.pt", weights_only=True))
    probe = torch.linspace(-8, 8, 777, device="cuda")
    assert torch.equal(fresh.apply(probe), trainer.calibrator.apply(probe))
    assert fresh.report()["status"] == "converged"
