"""CPU: the permutation-importance contract on the host: the numpy restatement (tests/importance_reference.py) is a
keyed bijection and its empty mask is ``RecordLayout.write``; the report arithmetic on a hand-made array; every refusal
of ``FieldImportance.run`` / ``Trainer`` before the device; the declarations."""
import json
import math
import os
import re
import types

import numpy as np
import pytest

from tests import importance_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dfm_permutation_keys", "dfm_records_permute")


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
    assert set(_lib.SIGNATURES) == declared
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    for name in ("FieldImportance", "ImportanceReport", "RecordSet"):
        assert hasattr(T, name), name
    assert hasattr(T.FusedPredictor, "field_importance")
    assert T.MixedSchemaPredictor.field_importance is T.FusedPredictor.field_importance
    assert T.QuantizedPredictor.field_importance is T.FusedPredictor.field_importance
    # the header states the counter and the key layout that the restatement uses
    assert f"0x{IR.GOLDEN:016X}" in text and f"0x{IR.SALT:016X}" in text and "(repeat << 40) + i" in text
    import ctypes
    assert ctypes.sizeof(_lib.RecordField) == 16


@pytest.mark.parametrize("n", IR.SIZES + (1000,))
def test_every_permutation_is_a_bijection_keyed_by_seed_and_repeat_alone(n):
    perms = {}
    for seed in (0, 7, 2 ** 63 + 5):
        for repeat in (0, 1, 4):
            k = IR.keys(seed, repeat, n)
            assert k.dtype == np.int64 and (k >= 0).all() and np.unique(k).size == n
            assert np.array_equal(k & 0xFFFFFFFF, np.arange(n))
            p = IR.permutation(seed, repeat, n)
            assert np.array_equal(np.sort(p), np.arange(n))
            assert np.array_equal(p, IR.permutation(seed, repeat, n))           # nothing else enters
            assert np.array_equal(p, np.argsort(k, kind="stable"))
            perms[seed, repeat] = p
    if n >= 8:
        vals = list(perms.values())
        assert all(not np.array_equal(a, b) for i, a in enumerate(vals) for b in vals[i + 1:])


def test_keys_follow_the_stated_counter():
    """One key by hand, in Python integers."""
    seed, repeat, i = 3, 2, 5
    x = (seed * IR.GOLDEN + IR.SALT + (repeat << 40) + i) & IR.MASK64
    for mul in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):
        x ^= x >> 33
        x = (x * mul) & IR.MASK64
    x ^= x >> 33
    assert int(IR.keys(seed, repeat, 8)[i]) == (((x & 0xFFFFFFFF) >> 1) << 32) | i
    # the low words of a prefix do not depend on n; the hash does not either
    assert np.array_equal(IR.keys(seed, repeat, 100)[:8], IR.keys(seed, repeat, 8))


@pytest.mark.parametrize("which", IR.SCHEMAS)
@pytest.mark.parametrize("n", IR.SIZES)
def test_empty_mask_reproduces_the_written_record(which, n):
    from deepfm_amd.data.packed import RecordLayout
    fields = IR.schema_fields(which)
    cols = IR.columns_of(fields, n, 1)
    lay = RecordLayout.of(cols.schema, IR.B)
    recs = IR.set_records(lay, cols)
    perm = IR.permutation(1, 0, n)
    nb = (n + IR.B - 1) // IR.B
    for k in range(nb):
        first, count = k * IR.B, min(IR.B, n - k * IR.B)
        want = np.zeros(lay.record_bytes, np.uint8)
        lay.write(want, cols, first, first + count)
        got = IR.permute_record(lay, recs, n, perm, 0, first, count)
        assert np.array_equal(got, want), (which, n, k)
        assert np.array_equal(got, recs[k][:lay.record_bytes])
    # a full mask is the record of the permuted samples, labels in place
    full = (1 << len(lay.names)) - 1
    count = min(IR.B, n)
    got = IR.permute_record(lay, recs, n, perm, full, 0, count)
    idx = np.concatenate([perm[:count], np.zeros(IR.B - count, np.int64)])
    want = np.zeros(lay.record_bytes, np.uint8)
    lay.write_indexed(want, cols, idx)
    ids, dense, labels, bags = lay.views(want)
    ids[:, count:], dense[:, count:] = 0, 0
    for b in bags:
        b[count:] = 0
    labels[:count], labels[count:] = cols.labels[:count], 0
    assert np.array_equal(got, want), (which, n)


def test_permute_record_leaves_the_rest_of_its_buffer_alone():
    from deepfm_amd.data.packed import RecordLayout
    cols = IR.columns_of(IR.schema_fields("mixed"), 70, 2)
    lay = RecordLayout.of(cols.schema, IR.B)
    out = np.full(lay.record_bytes + 64, 0xA5, np.uint8)
    IR.permute_record(lay, IR.set_records(lay, cols), 70, IR.permutation(0, 0, 70), 0b101, 64, 6, out)
    assert (out[lay.record_bytes:] == 0xA5).all() and not (out[:lay.record_bytes] == 0xA5).all()


# ---- the report
def _report():
    from deepfm_amd.training import ImportanceReport
    base = np.array([0.75, 0.5])
    values = np.array([[[0.5, 0.75], [0.625, 0.625]],           # a: harmful
                       [[0.75, 0.5], [0.75, 0.5]],              # z: nothing
                       [[0.5, 1.0], [0.5, 0.75]],               # b: the most harmful in both
                       [[0.5, 0.75], [0.625, 0.625]],           # a+z
                       [[0.75, 0.5], [0.75, 0.5]]])             # z2: ties with z
    return ImportanceReport(["a", "z", "b", "a+z", "z2"], ["auc", "logloss"], base, values,
                            {"a+z": ("a", "z")}, seed=4, n=10)


def test_report_arithmetic_on_a_hand_made_array():
    r = _report()
    assert r.delta.shape == (5, 2, 2) and np.array_equal(r.delta, r.values - r.baseline)
    assert np.array_equal(r.mean()[0], [-0.1875, 0.1875]) and np.array_equal(r.mean()[1], [0.0, 0.0])
    want_se = np.std(r.delta, axis=1, ddof=1) / math.sqrt(2)
    assert np.array_equal(r.se(), want_se) and r.se()[0, 0] == pytest.approx(0.0625, rel=1e-15)
    # harm: logloss rise a 0.1875, b 0.375, a+z 0.1875, z and z2 0 -> ties keep the order of the groups
    assert r.ranking("logloss") == ["b", "a", "a+z", "z", "z2"] == r.ranking()
    assert r.ranking("auc") == ["b", "a", "a+z", "z", "z2"]
    assert r.interaction("a", "z", "auc") == 0.0 and r.interaction("z", "a", "logloss") == 0.0
    assert np.array_equal(r.interaction("a", "z", "auc", per_repeat=True), [0.0, 0.0])
    with pytest.raises(KeyError, match="a.*b"):
        r.interaction("a", "b", "auc")                  # the union was not run
    with pytest.raises(KeyError, match="nope"):
        r.interaction("nope", "a", "auc")
    with pytest.raises(KeyError, match="gauc"):
        r.ranking("gauc")
    d = r.to_dict()
    assert json.loads(json.dumps(d, allow_nan=False)) == d
    assert d["groups"]["a+z"] == ["a", "z"] and d["repeats"] == 2 and d["metrics"] == ["auc", "logloss"]
    assert d["importance"]["a"]["logloss"] == {"mean": 0.1875, "se": float(want_se[0, 1]), "delta": [0.25, 0.125]}
    assert r == _report()


def test_single_repeat_has_no_standard_error_and_no_nan_in_the_dict():
    from deepfm_amd.training import ImportanceReport
    r = ImportanceReport(["f"], ["auc", "logloss", "HR@1"], [0.5, 0.7, math.nan], [[[0.5, 0.8, math.nan]]])
    assert np.isnan(r.se()).all() and r.se().shape == (1, 3)
    d = r.to_dict()
    json.dumps(d, allow_nan=False)
    assert d["importance"]["f"]["logloss"]["se"] is None and d["baseline"]["HR@1"] is None
    assert d["importance"]["f"]["HR@1"] == {"mean": None, "se": None, "delta": [None]}
    assert r.ranking("HR@1") == ["f"]
    with pytest.raises(ValueError, match=r"\(G, R, M\)"):
        ImportanceReport(["f"], ["auc"], [0.5], [[0.5]])


# ---- refusals, all before the device
class _NoDevice:
    """A predictor whose every attribute but the schema raises: a check that touches the device fails the test."""

    def __init__(self, names):
        self.model = types.SimpleNamespace(schema=types.SimpleNamespace(fields=dict.fromkeys(names)))

    def __getattr__(self, name):
        raise AssertionError(f"the check touched predictor.{name}")


@pytest.mark.parametrize("kw, match", [
    (dict(fields=["a", "nope"]), "'nope' is not a field"),
    (dict(groups={"g": ["a", "missing"]}), "'missing' is not a field"),
    (dict(groups={"g": []}), "group 'g' is empty"),
    (dict(groups={"a": ["b", "c"]}), "duplicate label 'a'"),
    (dict(fields=["a", "a"]), "duplicate label 'a'"),
    (dict(fields=[]), "no field and no group"),
    (dict(fields="a"), "list of field names"),
    (dict(repeats=0), "repeats = 0"),
    (dict(repeats=-3), "repeats = -3"),
    (dict(repeats=1.5), "repeats = 1.5"),
    (dict(ranking_ks=[0]), "every k must be >= 1"),
])
def test_refusals_come_before_the_device(kw, match):
    from deepfm_amd.training import FieldImportance
    with pytest.raises(ValueError, match=match):
        FieldImportance(_NoDevice(["a", "b", "c"])).run(object(), **kw)


def test_check_request_builds_labels_members_and_masks():
    from deepfm_amd.training.importance import check_request
    plan = check_request(["a", "b", "c"], None, {"a+c": ["a", "c"]}, 3)
    assert plan == [("a", ("a",), 1), ("b", ("b",), 2), ("c", ("c",), 4), ("a+c", ("a", "c"), 5)]
    assert check_request(["a", "b"], [], {"both": ("b", "a")}, 1) == [("both", ("b", "a"), 3)]
    with pytest.raises(ValueError, match="at most 64"):
        check_request([f"f{i}" for i in range(65)])


def test_record_set_size_is_refused_before_any_allocation():
    from deepfm_amd.data.packed import RecordLayout
    from deepfm_amd.data.synthetic import schema_from_fields
    from deepfm_amd.training.importance import _set_bytes
    lay = RecordLayout.of(schema_from_fields(IR.schema_fields("criteo")), 4096)
    nb, stride = _set_bytes(1_000_000, lay, 2 << 30)
    assert (nb, stride) == (245, (lay.record_bytes + 255) // 256 * 256)
    with pytest.raises(ValueError, match=rf"takes {nb * stride} bytes .* max_bytes = 1000"):
        _set_bytes(1_000_000, lay, 1000)
    with pytest.raises(ValueError, match="no samples"):
        _set_bytes(0, lay, 2 << 30)


def test_trainer_refuses_a_bad_importance_before_anything_else():
    from deepfm_amd.training import Trainer
    for bad in (-1, 1.5, True, 1 << 24):
        with pytest.raises(ValueError, match="importance"):
            Trainer(None, None, None, None, None, None, importance=bad)
    import inspect
    p = inspect.signature(Trainer.__init__).parameters["importance"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0
