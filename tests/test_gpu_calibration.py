"""GPU: the calibration pass (csrc/calibration.hip) against the numpy restatement (tests/calibration_reference.py).

Everything derived from exact integers (counts, positives, the sums of predictions and squared errors, the whole bin
table, ece, mce, mean_pred, brier, the fault counts) is compared with ``==`` on the doubles.  The log-loss columns
(global and per slice) are compared as means within one quantum, 2^-27: the device's and numpy's fp64 logarithms may
differ in the last place, which moves a term by at most one quantum.  Then the independence of the sample order, and
the path through ``compute_calibration``, the predictors and the Trainer."""
import gc
import json

import numpy as np
import pytest
import torch

from tests import calibration_reference as CR

pytestmark = pytest.mark.gpu

Q27 = 2.0 ** -27
# the launch geometry of csrc/calibration.hip: chunks of 1024 threads x 4 samples, at most 512 workgroups
CHUNK, MAX_BLOCKS = 4096, 512


@pytest.fixture(autouse=True)
def _collect_dead_cycles_here():
    """A Trainer whose ``evaluate`` is replaced by a closure over its own method is a dead reference cycle that holds
    captured graphs and device buffers; ``torch.cuda.graph`` no longer collects before a capture, and a cycle freed by
    the automatic collector inside a later test's stream capture aborts the process.  Collect at the end of each test."""
    yield
    gc.collect()


def _dev(x):
    return x if isinstance(x, torch.Tensor) or x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same(a, b):
    """== on doubles, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _check(labels, scores, bins=10, slice_ids=None, num_slices=None, what="", device_inputs=None):
    """The device values of one input against the restatement; returns (out, bins, slices) device tensors."""
    from deepfm_amd.training import calibration_device
    y, p, sid = device_inputs if device_inputs is not None else (_dev(labels), _dev(scores), _dev(slice_ids))
    out, bt, st = calibration_device(y, p, bins, sid, num_slices)
    want = CR.calibration(labels, scores, bins, slice_ids, num_slices)
    got = out.cpu().numpy()
    print(f"{what}: N {got[0]:.0f} mean_pred {got[2]!r} brier {got[3]!r} logloss {got[4]!r} / {want['out'][4]!r} "
          f"ece {got[5]!r} mce {got[6]!r} faults {got[7:11].tolist()}")
    exact = [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11]
    assert _same(got[exact], want["out"][exact]), (what, got, want["out"])
    if want["out"][0]:
        assert abs(got[4] - want["out"][4]) <= Q27, what
    else:
        assert np.isnan(got[4]), what
    assert bt.shape == (bins, 3) and _same(bt.cpu().numpy(), want["bins"]), what
    if slice_ids is None:
        assert st is None
    else:
        g, w = st.cpu().numpy(), want["slices"]
        assert g.shape == w.shape and _same(g[:, :3], w[:, :3]), what
        cnt = np.maximum(w[:, 0], 1)
        assert np.all(np.abs(g[:, 3] - w[:, 3]) / cnt <= Q27) and np.all(g[w[:, 0] == 0, 3] == 0), what
    return out, bt, st


def _case(rng, n, slices=0, pos_rate=0.3):
    p = rng.beta(1.5, 5.0, n).astype(np.float32)
    y = (rng.random(n) < pos_rate).astype(np.float32)
    sid = rng.integers(0, slices, n) if slices else None
    return y, p, sid


# ----------------------------------------------------------------------------- sizes and alignment
# the wave (64) and workgroup (1024 threads) edges, a quarter of a workgroup, one more than a chunk (the second
# workgroup's first sample), than two chunks, and one more than the largest grid takes before a workgroup comes round
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1025, CHUNK + 1, 2 * CHUNK + 1,
                               CHUNK * MAX_BLOCKS + 1])
@pytest.mark.parametrize("slices", [0, 7])
def test_sample_counts(n, slices):
    rng = np.random.default_rng(n)
    y, p, sid = _case(rng, n, slices)
    _check(y, p, 10, sid, slices or None, what=f"n={n} slices={slices}")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 1030])
def test_views_offset_by_one_element(n):
    """All three tensors start one element into their allocation: three samples in front of the 16-byte body."""
    rng = np.random.default_rng(100 + n)
    y, p, sid = _case(rng, n + 1, 5)
    d = (_dev(y)[1:], _dev(p)[1:], _dev(sid)[1:])
    assert d[0].data_ptr() % 16 == 4 and d[1].data_ptr() % 16 == 4 and d[2].data_ptr() % 16 == 8
    _check(y[1:], p[1:], 10, sid[1:], 5, what=f"offset views n={n}", device_inputs=d)
    _check(y[1:], p[1:], 10, what=f"offset views n={n}, no slices", device_inputs=(d[0], d[1], None))


def test_views_that_never_line_up():
    """Labels and scores (or the ids) reach 16-byte alignment after different counts: every sample goes one by one."""
    rng = np.random.default_rng(7)
    n = 3000
    y, p, sid = _case(rng, n + 2, 9)
    dy, dp, ds = _dev(y), _dev(p), _dev(sid)
    _check(y[1:n + 1], p[2:], 10, what="labels + 1, scores + 2", device_inputs=(dy[1:n + 1], dp[2:], None))
    _check(y[1:n + 1], p[1:n + 1], 10, sid[:n], 9, what="labels + 1, scores + 1, ids + 0",
           device_inputs=(dy[1:n + 1], dp[1:n + 1], ds[:n]))


@pytest.mark.parametrize("bins", [1, 2, 10, 1024])
def test_bin_counts(bins):
    rng = np.random.default_rng(bins)
    n = 5000
    p = rng.random(n).astype(np.float32)                  # every bin of 1024 gets a few
    y = (rng.random(n) < p).astype(np.float32)
    sid = rng.integers(0, 30, n)
    out, bt, _ = _check(y, p, bins, sid, 30, what=f"bins={bins}")
    assert float(bt[:, 0].sum()) == n and int((bt[:, 0] > 0).sum()) >= min(bins, 1000)


# ----------------------------------------------------------------------------- special scores
def test_scores_on_bin_edges():
    y = np.array([0, 1, 1, 0], np.float32)
    _, bt, _ = _check(y[:3], np.array([0.25, 0.5, 0.75], np.float32), 4, what="K=4 edges")
    assert bt[:, 0].tolist() == [0, 1, 1, 1]              # an edge belongs to the bin above it
    # float32(0.3) * 10 rounds to 3 and float32(0.7) * 10 to 7 in float32 (the fp64 products: 3.0000001 and 6.9999999)
    p = np.array([0.3, 0.7, 0.3, 0.7], np.float32)
    assert float(p[1]) * 10 < 7 and p[1] * np.float32(10) == 7
    _, bt, _ = _check(y, p, 10, what="K=10 edges")
    assert bt[:, 0].tolist() == [0, 0, 0, 2, 0, 0, 0, 2, 0, 0]


def test_extreme_scores():
    tiny, below_one = np.float32(1e-45), np.nextafter(np.float32(1), np.float32(0))
    assert 0 < tiny < 1e-44 and below_one < 1
    p = np.array([0.0, 1.0, tiny, below_one] * 2, np.float32)
    y = np.array([0] * 4 + [1] * 4, np.float32)
    sid = np.array([0, 1, 2, 3] * 2)
    out, bt, st = _check(y, p, 10, sid, 4, what="extreme scores")
    assert bt[0].tolist() == [4, 2, 0.0] and bt[9, 0] == 4 and out[0] == 8
    # a certain and wrong prediction costs -log(2^-23) = 15.94, a certain and right one 1.2e-7
    assert abs(float(st[0, 3]) - (23 * np.log(2) + 2.0 ** -23)) <= 2 * Q27


def test_one_bin_and_one_slice_take_every_sample():
    n = 1 << 16
    rng = np.random.default_rng(5)
    p = (0.30 + 0.09 * rng.random(n)).astype(np.float32)
    y = (rng.random(n) < 0.35).astype(np.float32)
    out, bt, st = _check(y, p, 10, np.zeros(n, np.int64), 1, what="one bin, one slice")
    assert bt[3, 0] == n and st[0, 0] == n
    # and with the slice table on the global-atomics route: the one hot slice is the last of a large vocabulary
    from deepfm_amd import _lib
    S = 100_000
    assert _lib.load().dfm_calibration_route(10, S) == 1
    _check(y, p, 10, np.full(n, S - 1, np.int64), S, what="one bin, one slice, route 1")


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_one_class(label):
    from deepfm_amd.training import compute_calibration
    rng = np.random.default_rng(11)
    y, p, sid = _case(rng, 700, 3)
    y[:] = label
    out, _, _ = _check(y, p, 10, sid, 3, what=f"all labels {label}")
    assert out[1] == 700 * label
    d = compute_calibration(y, p, 10)
    assert "ne" not in d and ("copc" in d) == bool(label)


# ----------------------------------------------------------------------------- faults
def _faulty(rng):
    y, p, sid = _case(rng, 600, 8)
    p[10], p[11] = np.nan, np.nan
    p[20] = np.float32(1.0000001)
    p[21] = np.float32(-1e-9)
    p[22] = np.float32(-0.0)                              # valid: bin 0
    y[22] = 0.0
    y[30] = 0.5
    sid[40], sid[41], sid[42] = -1, 8, 8
    p[50], y[50], sid[50] = np.nan, 2.0, 99               # three faults at once: one count each, nothing else
    keep = np.ones(600, bool)
    keep[[10, 11, 20, 21, 30, 40, 41, 42, 50]] = False
    return y, p, sid, keep


def test_faulty_samples_are_counted_and_not_used():
    y, p, sid, keep = _faulty(np.random.default_rng(12))
    assert p[20] > 1 and p[21] < 0
    out, bt, st = _check(y, p, 10, sid, 8, what="faults")
    assert out[7:].tolist() == [4, 3, 2, 2, 0] and out[0] == keep.sum()
    clean, cbt, cst = _check(y[keep], p[keep], 10, sid[keep], 8, what="the same without them")
    assert torch.equal(out[:7], clean[:7]) and torch.equal(bt, cbt) and torch.equal(st, cst)
    assert clean[7:].tolist() == [0, 0, 0, 0, 0]
    # without slices the ids are not looked at
    out, _, _ = _check(y, p, 10, what="faults, no slices")
    assert out[7:].tolist() == [0, 3, 2, 2, 0]


@pytest.mark.parametrize("bad,msg", [("id", r"^3 slice ids outside \[0, num_slices\)$"),
                                     ("nan", r"^Input contains NaN\.$"), ("range", r"^2 scores outside \[0, 1\]$"),
                                     ("label", r"^1 labels other than 0 and 1$")])
def test_compute_calibration_raises_with_the_count(bad, msg):
    from deepfm_amd.training import compute_calibration
    y, p, sid = _case(np.random.default_rng(13), 500, 8)
    if bad == "id":
        sid[[1, 2, 3]] = [-5, 8, 1 << 40]
    elif bad == "nan":
        p[7] = np.nan
    elif bad == "range":
        p[[7, 8]] = [1.5, -0.25]
    else:
        y[9] = 0.5
    with pytest.raises(ValueError, match=msg):
        compute_calibration(y, p, 10, sid, 8)


def test_no_usable_sample_gives_nan_ratios():
    out, bt, st = _check(np.array([0.5, 2.0], np.float32), np.array([0.5, 0.5], np.float32), 3,
                         np.array([4, 0]), 2, what="nothing usable")
    assert out[0] == 0 and bool(torch.isnan(out[2:7]).all()) and out[7:].tolist() == [1, 0, 0, 2, 0]
    assert float(bt.abs().sum()) == 0 and float(st.abs().sum()) == 0


# ----------------------------------------------------------------------------- slices and the two routes
def test_one_slice():
    y, p, _ = _case(np.random.default_rng(14), 999)
    out, bt, st = _check(y, p, 10, np.zeros(999, np.int64), 1, what="num_slices=1")
    assert st[0, :3].tolist() == [out[0], out[1], float(bt[:, 2].sum())]


@pytest.mark.parametrize("bins", [10, 1024])
def test_both_sides_of_the_route_switch(bins):
    from deepfm_amd import _lib
    route = _lib.load().dfm_calibration_route
    lo, hi = 1, 1 << 24
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if route(bins, mid) == 0 else (lo, mid)
    assert route(bins, lo) == 0 and route(bins, hi) == 1 and hi == lo + 1
    rng = np.random.default_rng(bins)
    n = 6000
    for S in (lo, hi):
        y, p, sid = _case(rng, n, S)
        sid[:50], sid[50:100] = 0, S - 1
        _, _, st = _check(y, p, bins, sid, S, what=f"bins={bins} S={S} route {route(bins, S)}")
        assert st[0, 0] >= 50 and st[S - 1, 0] >= 50


# ----------------------------------------------------------------------------- order independence
@pytest.mark.parametrize("slices", [300, 5000], ids=["route0", "route1"])
def test_the_order_of_the_samples_does_not_matter(slices):
    from deepfm_amd import _lib
    from deepfm_amd.training import calibration_device
    assert _lib.load().dfm_calibration_route(20, slices) == (0 if slices == 300 else 1)
    n = 50_000
    y, p, sid = _case(np.random.default_rng(15), n, slices)
    first = _check(y, p, 20, sid, slices, what=f"order, S={slices}")
    again = calibration_device(_dev(y), _dev(p), 20, _dev(sid), slices)
    perm = (np.arange(n, dtype=np.int64) * 997) % n
    assert np.unique(perm).size == n
    moved = calibration_device(_dev(y[perm]), _dev(p[perm]), 20, _dev(sid[perm]), slices)
    for a, b, c in zip(first, again, moved):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()


# ----------------------------------------------------------------------------- compute_calibration
def test_compute_calibration_tables():
    from deepfm_amd.training import compute_calibration
    y, p, sid = _case(np.random.default_rng(16), 4000, 12)
    p[p >= 0.7] = np.float32(0.1)                         # empty bins at the top
    sid[sid == 5] = 4                                     # an empty slice
    y[sid == 6] = 0.0                                     # a slice without positives
    y[sid == 7] = 1.0                                     # and one without negatives
    want = CR.calibration(y, p, 10, sid, 12)
    for inputs in ((y, p, sid), (_dev(y), _dev(p), _dev(sid))):
        d = compute_calibration(inputs[0], inputs[1], 10, inputs[2], 12)
        s = CR.summary(want)
        assert list(d) == ["mean_pred", "base_rate", "brier", "ece", "mce", "copc", "ne", "reliability", "slices"]
        assert all(type(d[k]) is float for k in s)
        assert all(d[k] == s[k] for k in s if k != "ne") and abs(d["ne"] - s["ne"]) <= 4 * Q27
        rel, b = d["reliability"], want["bins"]
        filled = b[:, 0] > 0
        assert not filled[7:].any() and filled[:7].all()
        assert _same(rel["count"], b[:, 0]) and _same(rel["positives"], b[:, 1])
        assert _same(rel["mean_pred"][filled], b[filled, 2] / b[filled, 0])
        assert np.isnan(rel["mean_pred"][~filled]).all()
        assert _same(rel["frac_pos"][filled], b[filled, 1] / b[filled, 0]) and np.isnan(rel["frac_pos"][~filled]).all()
        sl, t = d["slices"], want["slices"]
        assert _same(sl["count"], t[:, 0]) and _same(sl["positives"], t[:, 1])
        some = t[:, 0] > 0
        assert some.sum() == 11 and all(np.isnan(sl[k][5]) for k in ("mean_pred", "base_rate", "logloss", "copc", "ne"))
        assert _same(sl["mean_pred"][some], t[some, 2] / t[some, 0])
        assert _same(sl["base_rate"][some], t[some, 1] / t[some, 0])
        assert np.abs(sl["logloss"][some] - t[some, 3] / t[some, 0]).max() <= Q27
        assert np.isnan(sl["copc"][6]) and sl["copc"][7] == t[7, 2] / t[7, 1]
        assert np.isnan(sl["ne"][6]) and np.isnan(sl["ne"][7]) and np.isfinite(np.delete(sl["ne"], [5, 6, 7])).all()
    # default num_slices: max + 1
    assert compute_calibration(y, p, 10, sid)["slices"]["count"].shape == (12,)
    assert "slices" not in compute_calibration(y, p, 10)


# ----------------------------------------------------------------------------- the predictors
CAL_KEYS = ["mean_pred", "base_rate", "brier", "ece", "mce", "copc", "ne"]


def _check_predictor(pred, cols, loader, ks, slice_field, slice_ids, dense_field):
    from deepfm_amd.training import compute_calibration
    vocab = pred.model.schema.fields[slice_field].vocabulary_size
    for how in ("evaluate", "evaluate_loader"):
        run = (lambda **kw: pred.evaluate(cols, ranking_ks=ks, group_auc=True, **kw)) if how == "evaluate" else \
            (lambda **kw: pred.evaluate_loader(loader, ranking_ks=ks, group_auc=True, **kw))
        plain = run()
        assert not set(CAL_KEYS) & set(plain)
        m = run(calibration_bins=10)
        assert list(m) == list(plain) + CAL_KEYS, how
        assert {k: m[k] for k in plain} == plain, how                         # bit for bit: == on floats
        want = compute_calibration(pred.last_labels, pred.last_scores, 10)
        assert {k: m[k] for k in CAL_KEYS} == {k: want[k] for k in CAL_KEYS}, how
        assert pred.last_calibration["slices"] is None
        bins = pred.last_calibration["bins"]
        assert bins.is_cuda and bins.shape == (10, 3) and float(bins[:, 0].sum()) == len(cols)
        sliced = run(calibration_bins=10, slice_field=slice_field)
        assert sliced == m, how
        want = compute_calibration(pred.last_labels, pred.last_scores, 10, slice_ids, vocab)
        table = pred.last_calibration["slices"]
        assert table.is_cuda and table.shape == (vocab, 4)
        assert np.array_equal(table[:, 0].cpu().numpy(), want["slices"]["count"])
        assert np.array_equal(table[:, 1].cpu().numpy(), want["slices"]["positives"])
        assert np.array_equal(table[:, 0].cpu().numpy(), np.bincount(slice_ids, minlength=vocab))
        ref = CR.calibration(pred.last_labels.cpu().numpy(), pred.last_scores.cpu().numpy(), 10, slice_ids, vocab)
        assert _same(table[:, :3].cpu().numpy(), ref["slices"][:, :3]) and _same(bins.cpu().numpy(), ref["bins"])
        assert 0.0 < m["ece"] <= m["mce"] < 1.0 and m["ne"] > 0
        with pytest.raises(ValueError, match="not a SPARSE field"):
            run(calibration_bins=10, slice_field=dense_field)
        with pytest.raises(ValueError, match="not a SPARSE field"):
            run(calibration_bins=10, slice_field="no_such_field")
        with pytest.raises(ValueError, match="needs calibration_bins"):
            run(slice_field=slice_field)
    # the user column serves both when the slices are the users
    by_user = pred.evaluate_loader(loader, ranking_ks=ks, group_auc=True, calibration_bins=10, slice_field="user_id")
    assert by_user == m
    assert pred.last_calibration["slices"].shape[0] == pred.model.schema.fields["user_id"].vocabulary_size
    only = pred.evaluate(cols, calibration_bins=10)
    assert list(only) == ["auc", "logloss"] + CAL_KEYS and only["ece"] == m["ece"]


def test_mixed_predictor_adds_the_calibration_numbers():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.schema import FeatureType
    from deepfm_amd.training import MixedSchemaPredictor
    from tests.helpers import random_fields_batch
    from tests.test_gpu_mixed_predict import _movielens_model
    fields, model = _movielens_model("deepfm", seed=5)
    U, C, B = 60, 50, 512
    n = U * C
    assert n % B
    rng = np.random.default_rng(13)
    feats = random_fields_batch(fields, n, rng, zero_frac=0.05)
    feats["user_id"] = np.repeat(np.arange(1, U + 1, dtype=np.int64), C)
    labels = (rng.random(n) < 0.2).astype(np.float32)
    cols = PackedColumns(model.schema, feats, labels)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    kinds = {nm: sp.feature_type for nm, sp in model.schema.fields.items()}
    slice_field = next(nm for nm, k in kinds.items() if k is FeatureType.SPARSE and nm != "user_id")
    assert kinds["dow_sin"] is FeatureType.DENSE
    _check_predictor(MixedSchemaPredictor(model, B), cols, loader, [1, 5, 10], slice_field,
                     np.asarray(feats[slice_field], np.int64), "dow_sin")


def test_uniform_predictor_adds_the_calibration_numbers():
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FusedPredictor
    from tests.test_gpu_ranking import _user_model
    model = _user_model()
    users, cands, B = 90, 40, 512
    rng = np.random.default_rng(11)
    uid = np.repeat(np.arange(users, dtype=np.int64) * 7, cands)
    y = (rng.random(uid.size) < 0.25).astype(np.float32)
    feats = {"user_id": uid, "item_id": rng.integers(0, 5000, uid.size), "genre": rng.integers(0, 20, uid.size),
             "age": rng.random(uid.size).astype(np.float32)}
    cols = PackedColumns(model.schema, feats, y)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    _check_predictor(FusedPredictor(model, B), cols, loader, [1, 5], "genre", feats["genre"], "age")


# ----------------------------------------------------------------------------- the Trainer
def test_trainer_reports_the_calibration_numbers(tmp_path):
    import deepfm_amd.training as T
    from deepfm_amd.data.schema import FeatureType
    from tests.test_gpu_trainer import _trainer_config, _trainer_data, _trainer_model
    cfg = _trainer_config(tmp_path / "run", num_epochs=2)
    schema, (train, val, test) = _trainer_data(cfg)
    slice_field = next(nm for nm, sp in schema.fields.items() if sp.feature_type is FeatureType.SPARSE)
    trainer = T.Trainer(_trainer_model(schema, cfg), schema, cfg, train, val, test, calibration_bins=10,
                        slice_field=slice_field)
    seen = []
    inner = trainer.evaluate
    trainer.evaluate = lambda ds, split="eval": seen.append(inner(ds, split)) or seen[-1]
    got = trainer.train()
    with open(tmp_path / "run" / "results.json") as f:
        res = json.load(f)
    assert len(seen) == 3 and got in seen[:2] and res["val_metrics"] == got and res["test_metrics"] == seen[2]
    for m in (res["val_metrics"], res["test_metrics"]):
        assert set(CAL_KEYS) <= set(m) and {"auc", "logloss", "HR@1"} <= set(m)
        # 1 positive + 20 candidates per query
        assert m["base_rate"] == 1 / 21 and 0 <= m["ece"] <= m["mce"] <= 1 and m["ne"] > 0 and m["brier"] > 0
    table = trainer.predictor.last_calibration["slices"]
    assert table.shape == (schema.fields[slice_field].vocabulary_size, 4) and float(table[:, 0].sum()) == test.rows
    # switched off, no key is added (the Trainer's default)
    trainer.calibration_bins, trainer.slice_field = 0, None
    assert not set(CAL_KEYS) & set(inner(val, "val"))


def test_trainer_refuses_to_watch_ece(tmp_path):
    import deepfm_amd.training as T
    from tests.test_gpu_trainer import _trainer_config, _trainer_data, _trainer_model
    cfg = _trainer_config(tmp_path / "run", metric="ece")
    schema, (train, val, test) = _trainer_data(cfg)
    with pytest.raises(ValueError, match=r"training\.metric = 'ece' cannot be watched: lower is better"):
        T.Trainer(_trainer_model(schema, cfg), schema, cfg, train, val, test, calibration_bins=10)
