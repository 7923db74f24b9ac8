"""CPU: the feature encoders' host side (``deepfm_amd/data/encoders.py``).  The restatement of the reference's transforms
(``tests/encoders_reference.py``) equals what the reference's own classes gave (``tests/golden/encoders_reference.npz``);
the new entry points are declared, exported and bound; refusals happen before any device work.  No compute."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import encoders_reference as R
from tests.helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE = ("user_id", "movie_id", "C0", "C1", "C2", "C3")
DENSE = ("age", "timestamp", "I0", "I1")
SPLITS = ("train", "heldout")


@pytest.fixture(scope="module")
def golden():
    return load("encoders_reference")


def test_golden_holds_what_the_issue_asks_for(golden):
    g = golden
    assert any((g[f"ref/{n}/heldout"] == 0).any() for n in SPARSE)          # unseen values in the held-out split
    assert (g["ref/genres/heldout"] == 0).any() and g["raw/genres/train/lengths"].max() > int(g["max_length"])
    assert g["raw/age/train"].dtype == np.float32 and g["raw/timestamp/train"].dtype == np.float64
    # a span float32 cannot hold: an encoder that cast the raw values to float32 before scaling would be told apart
    ts, lo, hi = g["raw/timestamp/train"], float(g["min/timestamp"]), float(g["max/timestamp"])
    early = R.minmax_transform(lo, hi, ts.astype(np.float32)).astype(np.float32)
    assert (early != g["ref/timestamp/train"].astype(np.float32)).mean() > 0.5


@pytest.mark.parametrize("name", SPARSE)
def test_restated_label_encoder_equals_the_reference(golden, name):
    keys, counts = R.fit_vocabulary(golden[f"raw/{name}/train"])
    assert len(keys) + 1 == int(golden[f"vocab/{name}"]) and counts.sum() == len(golden[f"raw/{name}/train"])
    for split in SPLITS:
        got = R.label_transform(keys, golden[f"raw/{name}/{split}"])
        want = golden[f"ref/{name}/{split}"]
        assert got.dtype == want.dtype == np.int64 and np.array_equal(got, want), (name, split)


def test_restated_multihot_encoder_equals_the_reference(golden):
    L = int(golden["max_length"])
    lists = R.valid_tokens(golden["raw/genres/train/tokens"], golden["raw/genres/train/lengths"])
    keys, _ = R.fit_vocabulary(np.array([t for row in lists for t in row], np.int64))
    assert len(keys) + 1 == int(golden["vocab/genres"])
    for split in SPLITS:
        got = R.multihot_transform(keys, golden[f"raw/genres/{split}/tokens"], golden[f"raw/genres/{split}/lengths"], L)
        assert np.array_equal(got, golden[f"ref/genres/{split}"]), split


@pytest.mark.parametrize("name", DENSE)
def test_restated_scaler_equals_the_reference_bit_for_bit(golden, name):
    lo, hi = R.minmax_fit(golden[f"raw/{name}/train"])
    assert lo == float(golden[f"min/{name}"]) and hi == float(golden[f"max/{name}"])
    for split in SPLITS:
        got = R.minmax_transform(lo, hi, golden[f"raw/{name}/{split}"])
        want = golden[f"ref/{name}/{split}"]
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, split)
    assert np.array_equal(R.minmax_transform(3.0, 3.0, np.array([1.0, 3.0])), np.zeros(2))


def test_restated_pruning_and_mixer():
    values = np.array([5, 5, 5, 1, 1, 9, 9, 7, 3, 3, -2], np.int64)         # counts: 5:3, 1:2, 9:2, 3:2, 7:1, -2:1
    keys, counts = R.fit_vocabulary(values, min_count=2)
    assert keys.tolist() == [1, 3, 5, 9] and counts.tolist() == [2, 2, 3, 2]
    keys, counts = R.fit_vocabulary(values, max_vocab=3)                     # the tie 1 / 3 / 9 at the cut: smaller keys
    assert keys.tolist() == [1, 3, 5] and counts.tolist() == [2, 2, 3]
    assert R.fit_vocabulary(values, min_count=2, max_vocab=10)[0].tolist() == [1, 3, 5, 9]
    assert R.fit_vocabulary(values, max_vocab=0)[0].size == 0
    # the published fmix64 of MurmurHash3: 0 is a fixed point, and the two forms agree on the edge keys
    assert R.mix64(0) == 0 and R.mix64(1) == 0xB456BCFC34C2CB2C
    edge = np.array([0, 1, -1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 1 << 33], np.int64)
    assert R.mix64_array(edge).tolist() == [R.mix64(int(k)) for k in edge]
    assert R.hashed(edge, 1).tolist() == [1] * len(edge) and R.hashed(edge, 7).max() <= 7


def test_encoder_symbols_are_declared_exported_and_bound():
    from deepfm_amd import _lib
    header = open(os.path.join(ROOT, "include", "deepfm_hip.h")).read()
    assert re.search(rf"#define DFM_ABI_VERSION {_lib.ABI_VERSION}\b", header)
    assert "0xFF51AFD7ED558CCD" in header and "0xC4CEB9FE1A85EC53" in header         # the mixer is written out
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    for name, count in (("dfm_vocab_capacity", 1), ("dfm_vocab_build", 6), ("dfm_encode_columns", 5)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert decl is not None and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(decl.group(1).split(",")) == count == len(_lib.SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert ctypes.sizeof(_lib.EncodeJob) == 56 and _lib.EncodeJob.kind.offset == 32
    assert _lib.EncodeJob.log2_capacity.offset == 52 and _lib.VOCAB_SLOT_BYTES == 16
    kinds = re.search(r"enum dfm_encode_kind \{(.*?)\}", header, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"=\s*(\d+)", kinds)] == [
        _lib.ENC_LOOKUP, _lib.ENC_BAG, _lib.ENC_HASHED, _lib.ENC_SCALE_F32, _lib.ENC_SCALE_F64, _lib.ENC_COPY_F32,
        _lib.ENC_ZERO_F32]


def test_capacity_rule_and_host_side_argument_checks():
    """dfm_vocab_capacity: the smallest power of two >= max(16, 2 n); the two entries refuse bad arguments with
    DFM_ERR_INVALID on the host, before any HIP call."""
    from deepfm_amd import _lib
    lib = _lib.load()
    for n, want in ((0, 16), (1, 16), (8, 16), (9, 32), (31, 64), (32, 64), (33, 128), (1000, 2048), (100000, 262144),
                    (1 << 30, 1 << 31), ((1 << 30) + 1, 0), (-1, 0)):
        assert lib.dfm_vocab_capacity(n) == want, n
    P = 0x1000
    assert lib.dfm_vocab_build(P, 10, P, 16, P, None) == 1 and "capacity" in lib.dfm_last_error().decode()
    assert lib.dfm_vocab_build(P, 10, P + 8, 32, P, None) == 1 and "misaligned" in lib.dfm_last_error().decode()
    job = _lib.EncodeJob(in_=P, out=P, kind=_lib.ENC_LOOKUP, in_stride=1, out_stride=1, width=1, raw_width=1,
                         log2_capacity=4)
    job.u.table.slots = P
    one = (_lib.EncodeJob * 1)(job)
    assert lib.dfm_encode_columns(one, 0, 1, 1, None) == 1 and "num_jobs" in lib.dfm_last_error().decode()
    assert lib.dfm_encode_columns(one, 65, 1, 1, None) == 1
    assert lib.dfm_encode_columns(one, 1, 2, 1, None) == 1 and "n_out" in lib.dfm_last_error().decode()
    for field, value, word in (("kind", 7, "kind"), ("width", 2, "width"), ("out_stride", 0, "stride"),
                               ("log2_capacity", 3, "table"), ("in_", P + 4, "misaligned")):
        bad = _lib.EncodeJob.from_buffer_copy(job)
        setattr(bad, field, value)
        assert lib.dfm_encode_columns((_lib.EncodeJob * 1)(bad), 1, 1, 1, None) == 1, field
        assert word in lib.dfm_last_error().decode(), field


def _template():
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    return DatasetSchema(fields={"u": FieldSchema("u", FeatureType.SPARSE, 0, 16),
                                 "g": FieldSchema("g", FeatureType.SEQUENCE, 0, 8, max_length=3),
                                 "x": FieldSchema("x", FeatureType.DENSE, embedding_dim=4)})


def test_refusals_happen_before_any_device_work():
    """Wrong dtypes and shapes are refused on the host: these calls name the default device "cuda", and no GPU (nor a
    fitted table) is needed to be told."""
    from deepfm_amd.data import (DeviceFeatureEncoder, DeviceLabelEncoder, DeviceMinMaxScaler, DeviceMultiHotEncoder)
    le = DeviceLabelEncoder()
    for bad in (np.arange(4, dtype=np.int32), np.arange(4.0), torch.arange(4, dtype=torch.int16),
                np.array(["a", "b"], dtype=object)):
        with pytest.raises(TypeError):
            le.fit(bad)
        with pytest.raises(TypeError):
            le.transform(bad)
    with pytest.raises(TypeError):
        le.fit(["a", "b"])                                                  # strings are out of scope
    with pytest.raises(ValueError):
        le.fit(np.zeros((2, 2), np.int64))
    with pytest.raises(RuntimeError, match="fit or load_state_dict"):
        le.transform(np.arange(4, dtype=np.int64))
    for kw in (dict(min_count=0), dict(max_vocab=-1), dict(min_count=1.5)):
        with pytest.raises(ValueError):
            DeviceLabelEncoder(**kw)
    for buckets in (0, -3, 2.5):
        with pytest.raises(ValueError):
            DeviceLabelEncoder.hashed(buckets)
    assert DeviceLabelEncoder.hashed(7).vocabulary_size == 8

    mh = DeviceMultiHotEncoder(max_length=3)
    with pytest.raises(ValueError):
        mh.fit(np.zeros(4, np.int64))                                       # one axis
    with pytest.raises(TypeError):
        mh.fit(np.zeros((4, 2), np.int32))
    with pytest.raises(ValueError):
        mh.fit(np.zeros((4, 2), np.int64), np.zeros(3, np.int32))           # lengths of another length
    with pytest.raises(TypeError):
        mh.fit(np.zeros((4, 2), np.int64), np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        DeviceMultiHotEncoder(max_length=0)

    sc = DeviceMinMaxScaler(name="price")
    with pytest.raises(TypeError, match="price"):
        sc.fit(np.arange(4))
    with pytest.raises(ValueError, match="price"):
        sc.fit(np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match="price"):
        sc.fit(np.zeros(0, np.float32))

    fe = DeviceFeatureEncoder(_template(), min_count={"u": 2}, max_vocab=5)
    assert fe.encoders["u"].min_count == 2 and fe.encoders["g"].min_count == 1 and fe.encoders["g"].max_vocab == 5
    assert fe.encoders["g"].max_length == 3
    raw = {"u": np.arange(4, dtype=np.int64), "g": (np.zeros((4, 5), np.int64), None), "x": np.zeros(4, np.float32)}
    with pytest.raises(KeyError):
        fe.fit({k: v for k, v in raw.items() if k != "x"})
    for name, bad in (("u", np.arange(4, dtype=np.int32)), ("x", np.arange(4)), ("g", np.zeros(4, np.int64))):
        with pytest.raises((TypeError, ValueError), match=name):
            fe.transform(dict(raw, **{name: bad}), np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="'x'"):
        fe.transform(dict(raw, x=np.zeros(5, np.float32)), np.zeros(4, np.float32))      # another length
    with pytest.raises(ValueError, match="labels"):
        fe.transform(raw, np.zeros(4, np.float64))
    with pytest.raises(TypeError):
        fe.encode_into(np.zeros(64, np.uint8), raw)
    with pytest.raises(TypeError):
        fe.encode_into(torch.zeros(64, dtype=torch.float32), raw)


def test_state_dict_round_trip_on_the_host():
    from deepfm_amd.data import DeviceFeatureEncoder, DeviceLabelEncoder, DeviceMultiHotEncoder
    keys = np.array([np.iinfo(np.int64).min, -1, 0, 5, np.iinfo(np.int64).max], np.int64)
    counts = np.array([1, 2, 3, 4, 5], np.int64)
    state = {"keys": torch.from_numpy(keys), "counts": torch.from_numpy(counts), "min_count": 2, "max_vocab": 9,
             "num_buckets": None}
    le = DeviceLabelEncoder()
    le.load_state_dict(state)
    assert le.vocabulary_size == 6 and (le.min_count, le.max_vocab) == (2, 9)
    assert le.classes_.tolist() == keys.tolist() and le.counts_.tolist() == counts.tolist()
    again = le.state_dict()
    assert sorted(again) == sorted(state) and "slots" not in again           # the hash table is not stored
    assert again["keys"].tolist() == keys.tolist() and again["counts"].tolist() == counts.tolist()
    with pytest.raises(ValueError, match="strictly increasing"):
        le.load_state_dict(dict(state, keys=torch.from_numpy(keys[::-1].copy())))
    with pytest.raises(ValueError):
        le.load_state_dict(dict(state, counts=torch.from_numpy(counts[:3].copy())))
    mh = DeviceMultiHotEncoder(max_length=2)
    mh.load_state_dict(dict(state, max_length=4))
    assert mh.max_length == 4 and mh.state_dict()["max_length"] == 4
    hs = DeviceLabelEncoder()
    hs.load_state_dict(DeviceLabelEncoder.hashed(11).state_dict())
    assert hs.num_buckets == 11 and hs.vocabulary_size == 12

    fe = DeviceFeatureEncoder(_template())
    sd = {"u": state, "g": dict(state, max_length=3), "x": {"min": -1.5, "max": 2.5}}
    fe.load_state_dict(sd)
    schema = fe.schema
    assert schema is not fe.template and fe.template.fields["u"].vocabulary_size == 0
    assert schema.fields["u"].vocabulary_size == 6 and schema.fields["g"].vocabulary_size == 6
    assert schema.fields["g"].max_length == 3 and schema.fields["x"].embedding_dim == 4
    out = fe.state_dict()
    assert out["x"] == {"min": -1.5, "max": 2.5} and out["g"]["keys"].tolist() == keys.tolist()
    with pytest.raises(KeyError):
        fe.load_state_dict({"u": state})


def test_device_columns_from_device_checks_its_blocks():
    from deepfm_amd.data import DeviceColumns
    schema, n = _template(), 5
    ids, dense, labels = torch.zeros(1, n, dtype=torch.int64), torch.zeros(1, n), torch.zeros(n)
    bags = [torch.zeros(n, 3, dtype=torch.int64)]
    cols = DeviceColumns.from_device(schema, ids, dense, labels, bags)
    assert len(cols) == n and cols.ids is ids and cols.bags[0] is bags[0] and cols.schema is schema
    assert list(cols.field_columns()) == ["u", "g", "x"]
    for bad in (dict(ids=ids.int()), dict(dense=torch.zeros(2, n)), dict(bags=[]), dict(bags=[bags[0][:, :2]]),
                dict(labels=torch.zeros(n, dtype=torch.float64))):
        args = dict(ids=ids, dense=dense, labels=labels, bags=bags)
        args.update(bad)
        with pytest.raises(ValueError):
            DeviceColumns.from_device(schema, **args)
