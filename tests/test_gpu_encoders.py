"""GPU: the device-side feature encoders (``csrc/encode.hip``, ``deepfm_amd/data/encoders.py``) against the numpy / dict
restatement of the reference's transforms (``tests/encoders_reference.py``) and against what the reference's own
classes gave (``tests/golden/encoders_reference.npz``).  Every comparison is exact: ids as integers, scaled values as
float32 bits, records as bytes, probabilities as bits."""
import numpy as np
import pytest
import torch

from tests import encoders_reference as R
from tests.helpers import load

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
EDGE_KEYS = [0, -1, I64.min, I64.max]
VOCAB_SIZES = [1, 2, 31, 32, 33, 1000, 100000]      # 32 keys fill a table of 64 exactly; 31 and 33 sit either side
COLUMN_LENGTHS = [1, 63, 64, 65, 257, 4097]         # around one wavefront, one workgroup, and several workgroups


def _keys(n, seed):
    """n distinct sorted keys: the edge keys first, then runs of consecutive integers, then random ones."""
    rng = np.random.default_rng(seed)
    pool = list(EDGE_KEYS[:n])
    runs = (n - len(pool)) // 2
    for base in (1, -(1 << 40), (1 << 62) - 7):
        pool += list(range(base, base + (runs + 2) // 3))
    keys = np.unique(np.array(pool, np.int64))[:n]
    while keys.size < n:
        keys = np.unique(np.concatenate([keys, rng.integers(I64.min, I64.max, n - keys.size, dtype=np.int64)]))
    return keys


def _absent(keys, m, seed):
    """m int64 values none of which is a key, neighbours of keys among them."""
    rng = np.random.default_rng(seed)
    with np.errstate(over="ignore"):
        near = keys[: m // 2 + 1] + np.int64(1)                             # INT64_MAX + 1 wraps; a key it hits is dropped
    cand = np.concatenate([near, rng.integers(I64.min, I64.max, 2 * m + 8, dtype=np.int64)])
    cand = cand[~np.isin(cand, keys)]
    assert cand.size >= m
    return cand[:m]


def _loaded(keys, **kw):
    from deepfm_amd.data import DeviceLabelEncoder
    enc = DeviceLabelEncoder(**kw)
    enc.load_state_dict({"keys": torch.from_numpy(keys), "counts": torch.ones(len(keys), dtype=torch.int64),
                         "min_count": 1, "max_vocab": None, "num_buckets": None})
    return enc


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- lookup
@pytest.mark.parametrize("n_keys", VOCAB_SIZES)
def test_lookup_equals_the_dict(n_keys):
    """Every vocabulary size x every column length x {none OOV, all OOV, heavy duplication, a mix}, exact."""
    keys = _keys(n_keys, n_keys)
    assert keys.size == n_keys and all(k in keys for k in EDGE_KEYS[:n_keys])
    enc = _loaded(keys)
    assert enc.vocabulary_size == n_keys + 1
    rng = np.random.default_rng(n_keys + 1)
    for L in COLUMN_LENGTHS:
        known, unknown = rng.choice(keys, L), _absent(keys, L, L)
        few = rng.choice(np.concatenate([keys[:2], unknown[:1]]), L)
        mixed = np.where(rng.random(L) < 0.5, known, unknown)
        for what, col in (("none OOV", known), ("all OOV", unknown), ("duplicates", few), ("mixed", mixed)):
            got = enc.transform(col)
            assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (L,)
            want = R.label_transform(keys, col)
            assert np.array_equal(_np(got), want), (n_keys, L, what)
        assert (R.label_transform(keys, unknown) == 0).all() and (R.label_transform(keys, known) > 0).all()
    # every key finds its own index, whatever slot it landed in
    assert np.array_equal(_np(enc.transform(keys)), np.arange(1, n_keys + 1))


def test_fit_numbers_the_keys_like_sorted_set():
    """fit on host and on device input: classes_ ascending, counts_, and the transform of the fitted data itself."""
    from deepfm_amd.data import DeviceLabelEncoder
    rng = np.random.default_rng(5)
    keys = _keys(1000, 9)
    values = np.concatenate([keys, rng.choice(keys, 5000)])
    rng.shuffle(values)
    want_keys, want_counts = R.fit_vocabulary(values)
    for source in (values, torch.from_numpy(values), torch.from_numpy(values).cuda()):
        enc = DeviceLabelEncoder().fit(source)
        assert np.array_equal(_np(enc.classes_), want_keys) and np.array_equal(_np(enc.counts_), want_counts)
        assert enc.vocabulary_size == len(want_keys) + 1 == len(set(values.tolist())) + 1
        assert np.array_equal(_np(enc.transform(source)), R.label_transform(want_keys, values))
    # one column of a row-major (n, 2) matrix is read in place through its stride; a stride of 0 is refused
    matrix = torch.from_numpy(np.stack([values, values[::-1]], axis=1)).cuda()
    assert matrix[:, 1].stride(0) == 2
    assert np.array_equal(_np(enc.transform(matrix[:, 1])), R.label_transform(want_keys, values[::-1]))
    with pytest.raises(ValueError, match="stride"):
        enc.transform(matrix[0, :1].expand(5))
    empty = DeviceLabelEncoder().fit(np.zeros(0, np.int64))                  # an empty table: everything is OOV
    assert empty.vocabulary_size == 1 and _np(empty.transform(np.array(EDGE_KEYS, np.int64))).tolist() == [0, 0, 0, 0]
    assert tuple(empty.transform(np.zeros(0, np.int64)).shape) == (0,)


def test_long_probe_runs_and_the_wrap_around():
    """Keys chosen (with the restated mixer) so that all 500 of them hash into the last 8 slots of their 1024-slot
    table: one probe run of 500 that wraps past the end.  Present keys, absent keys homed inside the run (they walk
    it to its end) and absent keys homed outside it."""
    cand = np.arange(1, 400000, dtype=np.int64)
    home = R.mix64_array(cand) & np.uint64(1023)
    inside = cand[home >= 1016]
    assert inside.size >= 1000
    keys, absent_inside = inside[:500], inside[500:1000]                    # ascending already
    enc = _loaded(keys)
    col = np.concatenate([keys[::-1], absent_inside, cand[home == 600][:100]])
    assert np.array_equal(_np(enc.transform(col)), R.label_transform(keys, col))


# ---------------------------------------------------------------------------------------------------- build
def test_build_reports_keys_that_do_not_increase_and_publishes_no_table():
    from deepfm_amd.data import encoders as E
    for bad in ([1, 2, 2, 3], [5, 4, 3], [0, I64.max, I64.min]):
        vocab = E._Vocabulary("cuda")
        vocab.set(torch.tensor(bad, dtype=torch.int64), torch.ones(len(bad), dtype=torch.int64))
        with pytest.raises(ValueError, match="strictly increasing"):
            vocab.table()
        assert vocab.slots is None
    # the status block itself: [0] keys without a slot, [1] keys not above their predecessor
    from deepfm_amd import _lib
    lib = _lib.load()
    keys = torch.tensor([3, 3, 2, 9, 9], dtype=torch.int64, device="cuda")
    slots = torch.empty(16, 2, dtype=torch.int64, device="cuda")
    status = torch.full((2,), 77, dtype=torch.int64, device="cuda")         # the call clears it first
    _lib.check(lib.dfm_vocab_build(keys.data_ptr(), 5, slots.data_ptr(), 16, status.data_ptr(), _lib.stream_handle()))
    assert status.tolist() == [0, 3]
    good = E._Vocabulary("cuda")
    good.set(torch.tensor([2, 3, 9], dtype=torch.int64), torch.ones(3, dtype=torch.int64))
    table = good.table()
    assert tuple(table.shape) == (16, 2) and good.log2_capacity == 4 and good.table() is table
    index = (table[:, 1] & 0xFFFFFFFF).cpu()
    assert sorted(index[index > 0].tolist()) == [1, 2, 3] and (table[:, 1] >> 32 == 0).all()
    assert sorted(table[:, 0].cpu()[index > 0].tolist()) == [2, 3, 9] and (table[:, 0].cpu()[index == 0] == 0).all()


@pytest.mark.parametrize("n_keys", [33, 100000])
def test_two_builds_give_the_same_lookups(n_keys):
    keys = _keys(n_keys, 3)
    col = np.concatenate([keys, _absent(keys, 4097, 1)])
    a, b = _loaded(keys).transform(col), _loaded(keys).transform(col)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- pruning
def _tied_values():
    """Counts with ties at every cut: keys 10..19 occur 3 times, 20..29 twice, 30..39 once, -5 and INT64_MAX 7 times."""
    parts = [np.repeat(np.arange(10, 20), 3), np.repeat(np.arange(20, 30), 2), np.arange(30, 40),
             np.repeat(np.array([-5, I64.max]), 7)]
    v = np.concatenate(parts).astype(np.int64)
    np.random.default_rng(0).shuffle(v)
    return v


@pytest.mark.parametrize("min_count,max_vocab", [(1, None), (2, None), (3, None), (4, None), (8, None), (1, 5), (1, 2),
                                                 (1, 12), (1, 17), (2, 17), (3, 6), (1, 0), (1, 1000)])
def test_min_count_and_max_vocab_equal_the_restatement(min_count, max_vocab):
    from deepfm_amd.data import DeviceLabelEncoder
    values = _tied_values()
    keys, counts = R.fit_vocabulary(values, min_count, max_vocab)
    enc = DeviceLabelEncoder(min_count=min_count, max_vocab=max_vocab).fit(values)
    assert np.array_equal(_np(enc.classes_), keys) and np.array_equal(_np(enc.counts_), counts)
    assert enc.vocabulary_size == len(keys) + 1
    probe = np.concatenate([values, np.array([0, 9, 40, I64.min], np.int64)])
    assert np.array_equal(_np(enc.transform(probe)), R.label_transform(keys, probe))
    if (min_count, max_vocab) == (1, 5):                                    # the tie among the 3-counts: smaller keys win
        assert keys.tolist() == [-5, 10, 11, 12, I64.max]


# ---------------------------------------------------------------------------------------------------- bags
@pytest.mark.parametrize("max_length", [1, 4, 6])
def test_bags_equal_the_reference_loop(max_length):
    from deepfm_amd.data import DeviceMultiHotEncoder
    rng = np.random.default_rng(max_length)
    W, n = max_length + 3, 257
    vocab = np.arange(50, 90, dtype=np.int64) * 11
    tokens = rng.choice(vocab, (n, W))
    lengths = rng.integers(0, W + 1, n).astype(np.int32)
    lengths[:5] = [0, 1, max_length - 1, max_length, max_length + 3]
    tokens[np.arange(W)[None, :] >= lengths[:, None]] = 777                 # junk past the length: never a vocabulary entry
    enc = DeviceMultiHotEncoder(max_length=max_length).fit(tokens, lengths)
    lists = R.valid_tokens(tokens, lengths)
    keys, counts = R.fit_vocabulary(np.array([t for row in lists for t in row], np.int64))
    assert 777 not in keys and np.array_equal(_np(enc.classes_), keys) and np.array_equal(_np(enc.counts_), counts)
    # held-out rows with unseen tokens in the middle, and lengths past the row (cut to the row)
    held = rng.choice(np.concatenate([vocab, [1, 2, 3]]), (n, W))
    held[:, W // 2] = 5
    held_len = rng.integers(0, W + 1, n).astype(np.int64)
    held_len[:7] = [0, 1, max_length - 1, max_length, max_length + 3, W + 5, -2]
    for tok, ln in ((tokens, lengths), (held, held_len), (held, None), (tokens[:1], lengths[:1]), (held[:65], None)):
        got = enc.transform(tok, ln)
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(tok), max_length)
        assert np.array_equal(_np(got), R.multihot_transform(keys, tok, ln, max_length))
    assert np.array_equal(_np(enc.transform((held, held_len))), R.multihot_transform(keys, held, held_len, max_length))
    full = DeviceMultiHotEncoder(max_length=max_length).fit(tokens)         # lengths=None: the junk is data
    assert 777 in _np(full.classes_)
    # a column-sliced token matrix is read in place through its row stride
    wide = torch.from_numpy(np.concatenate([held, held], axis=1)).cuda()
    assert np.array_equal(_np(enc.transform(wide[:, :W], held_len)), R.multihot_transform(keys, held, held_len, max_length))


# ---------------------------------------------------------------------------------------------------- scaler
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scaler_is_the_float64_expression_cast_once(dtype):
    from deepfm_amd.data import DeviceMinMaxScaler
    rng = np.random.default_rng(2)
    cases = {
        "plain": rng.normal(3, 10, 4097),
        "lognormal": rng.lognormal(0, 3, 257),
        "tiny": rng.normal(0, 1e-30, 65),
        "wide span": 1.0e9 + rng.integers(0, 1 << 34, 1000) / 1024.0,        # float32 holds neither the values nor the span
        "one": np.array([4.25]),
    }
    for what, col in cases.items():
        col = col.astype(dtype)
        sc = DeviceMinMaxScaler(name=what).fit(col)
        lo, hi = R.minmax_fit(col)
        assert (sc.min, sc.max) == (lo, hi) and isinstance(sc.min, float), what
        outside = np.concatenate([col, col.min() - np.abs(col[:3]), col.max() + np.abs(col[:3]) + 1]).astype(dtype)
        for probe in (col, outside, outside[:63]):
            got = sc.transform(probe)
            assert got.dtype == torch.float32 and got.is_cuda
            want = R.minmax_transform(lo, hi, probe).astype(np.float32)
            assert np.array_equal(_bits(_np(got)), _bits(want)), what
        if what not in ("one",):
            t = _np(sc.transform(outside))
            assert t.min() < 0 and t.max() > 1                                  # no clipping
    const = DeviceMinMaxScaler().fit(np.full(5, 7.5, dtype))                   # max == min: zeros, as in the reference
    assert _np(const.transform(np.array([7.5, 8, -1], dtype))).tolist() == [0.0, 0.0, 0.0]
    dev = DeviceMinMaxScaler().fit(torch.from_numpy(cases["plain"].astype(dtype)).cuda())
    assert (dev.min, dev.max) == R.minmax_fit(cases["plain"].astype(dtype))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_scaler_fit_refuses_non_finite_input(bad):
    from deepfm_amd.data import DeviceMinMaxScaler
    col = np.arange(100, dtype=np.float32)
    col[37] = bad
    sc = DeviceMinMaxScaler(name="price")
    with pytest.raises(ValueError, match="price"):
        sc.fit(col)
    with pytest.raises(ValueError, match="price"):
        sc.fit(torch.from_numpy(col.astype(np.float64)).cuda())
    assert (sc.min, sc.max) == (0.0, 1.0)


# ---------------------------------------------------------------------------------------------------- hashed
@pytest.mark.parametrize("num_buckets", [1, 7, 1 << 20])
def test_hashed_mode_is_the_restated_mixer(num_buckets):
    from deepfm_amd.data import DeviceLabelEncoder
    enc = DeviceLabelEncoder.hashed(num_buckets)
    assert enc.vocabulary_size == num_buckets + 1
    rng = np.random.default_rng(num_buckets)
    col = np.concatenate([np.array(EDGE_KEYS, np.int64), np.arange(-300, 300), rng.integers(I64.min, I64.max, 4097)])
    got = _np(enc.transform(col))
    assert np.array_equal(got, R.hashed(col, num_buckets)) and got.min() >= 1 and got.max() <= num_buckets
    assert got[:4].tolist() == [1 + R.mix64(k) % num_buckets for k in EDGE_KEYS]


# ---------------------------------------------------------------------------------------------------- end to end
MIXED = (("user_id", "sparse", 16), ("movie_id", "sparse", 16), ("genres", "sequence", 8), ("age", "dense", 4),
         ("timestamp", "dense", 8))
UNIFORM = (("C0", "sparse", 16), ("C1", "sparse", 16), ("I0", "dense", 16), ("C2", "sparse", 16), ("C3", "sparse", 16),
           ("I1", "dense", 16))
B = 64


@pytest.fixture(scope="module")
def golden():
    return load("encoders_reference")


def _template(fields, g):
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    out = {}
    for name, kind, dim in fields:
        out[name] = FieldSchema(name, FeatureType(kind), 0, dim,
                                max_length=int(g["max_length"]) if kind == "sequence" else 1)
    return DatasetSchema(fields=out)


def _raw(fields, g, split, device=None):
    raw = {}
    for name, kind, _ in fields:
        if kind == "sequence":
            raw[name] = (g[f"raw/{name}/{split}/tokens"], g[f"raw/{name}/{split}/lengths"])
        else:
            raw[name] = g[f"raw/{name}/{split}"]
    if device is not None:
        move = lambda a: torch.from_numpy(a).to(device)                      # noqa: E731
        raw = {k: tuple(move(x) for x in v) if isinstance(v, tuple) else move(v) for k, v in raw.items()}
    return raw


def _fitted(fields, g):
    from deepfm_amd.data import DeviceFeatureEncoder
    return DeviceFeatureEncoder(_template(fields, g)).fit(_raw(fields, g, "train"))


def _host_columns(schema, fields, g, split):
    """PackedColumns built on the host from the REFERENCE's outputs (its float64 scaled values cast by PackedColumns)."""
    from deepfm_amd.data.packed import PackedColumns
    return PackedColumns(schema, {name: g[f"ref/{name}/{split}"] for name, _, _ in fields}, g[f"labels/{split}"])


def _same_columns(dev, host):
    assert len(dev) == len(host)
    assert dev.ids.dtype == torch.int64 and np.array_equal(_np(dev.ids), host.ids)
    assert dev.dense.dtype == torch.float32 and np.array_equal(_bits(_np(dev.dense)), _bits(host.dense))
    assert np.array_equal(_bits(_np(dev.labels)), _bits(host.labels))
    assert len(dev.bags) == len(host.bags) and all(np.array_equal(_np(a), b) for a, b in zip(dev.bags, host.bags))


@pytest.mark.parametrize("fields", [MIXED, UNIFORM], ids=["mixed", "uniform"])
def test_fit_transform_equals_host_columns_of_the_reference_outputs(golden, fields):
    from deepfm_amd.data import DeviceColumns, DeviceFeatureEncoder
    g = golden
    enc = _fitted(fields, g)
    schema = enc.schema
    for name, kind, dim in fields:
        spec = schema.fields[name]
        assert spec.embedding_dim == dim and spec.vocabulary_size == (0 if kind == "dense" else int(g[f"vocab/{name}"]))
    for split in ("train", "heldout"):
        host = _host_columns(schema, fields, g, split)
        for device in (None, "cuda"):                                        # host arrays and device tensors alike
            cols = enc.transform(_raw(fields, g, split, device), g[f"labels/{split}"])
            assert isinstance(cols, DeviceColumns) and cols.ids.is_cuda and cols.schema.fields.keys() == schema.fields.keys()
            _same_columns(cols, host)
    held = enc.transform(_raw(fields, g, "heldout"), g["labels/heldout"])
    for name, t in held.field_columns().items():                             # 0 exactly where the reference has 0
        if schema.fields[name].feature_type.value != "dense":
            assert np.array_equal(_np(t) == 0, g[f"ref/{name}/heldout"] == 0), name
    assert (_np(held.ids) == 0).any()
    # a fresh encoder loaded from the state reproduces the transform; its tables are rebuilt, not stored
    state = enc.state_dict()
    assert all("slots" not in s for s in state.values())
    fresh = DeviceFeatureEncoder(_template(fields, g))
    fresh.load_state_dict(state)
    assert {n: s.vocabulary_size for n, s in fresh.schema.fields.items()} == \
           {n: s.vocabulary_size for n, s in schema.fields.items()}
    _same_columns(fresh.transform(_raw(fields, g, "heldout"), g["labels/heldout"]), _host_columns(schema, fields, g, "heldout"))


def _host_record(layout, host, start, end):
    out = np.zeros(layout.record_bytes, np.uint8)
    layout.write(out, host, start, end)
    return out


def _slice(raw, start, end):
    return {k: tuple(x[start:end] for x in v) if isinstance(v, tuple) else v[start:end] for k, v in raw.items()}


@pytest.mark.parametrize("fields", [MIXED, UNIFORM], ids=["mixed", "uniform"])
def test_encode_into_equals_record_layout_write_and_the_predictor_sees_the_same(golden, fields):
    from deepfm_amd.data.packed import RecordLayout
    from deepfm_amd.models import create_model
    from deepfm_amd.training import FusedPredictor, MixedSchemaPredictor
    from tests.test_cpu_mixed_predict import movielens_cfg
    g = golden
    enc = _fitted(fields, g)
    schema = enc.schema
    layout = RecordLayout.of(schema, B)
    host = _host_columns(schema, fields, g, "heldout")
    raw = _raw(fields, g, "heldout", "cuda")
    labels = torch.from_numpy(g["labels/heldout"]).cuda()
    torch.manual_seed(4)
    with torch.device("cuda"):
        model = create_model("deepfm", schema, movielens_cfg("deepfm", hidden_units=[32, 16]))
    model.embedding.strict_indices = True
    pred = (MixedSchemaPredictor if fields is MIXED else FusedPredictor)(model, B, use_graph=False)
    assert pred.record_bytes == layout.record_bytes
    for start, valid in ((0, B), (B, 100 - B), (3, 1)):                       # a full batch, valid < B, one sample
        want = _host_record(layout, host, start, start + valid)
        record = torch.full((layout.record_bytes,), 0, dtype=torch.uint8, device="cuda")
        if layout.seq_offsets:                                              # bytes no writer owns: the alignment gap
            assert layout.seq_offsets[0] - (layout.labels_offset + 4 * B) < 16
        record[: layout.labels_offset + 4 * B] = 0xAB                       # stale bytes the call must overwrite
        for off, L in zip(layout.seq_offsets, layout.seq_lengths):
            record[off: off + 8 * B * L] = 0xAB
        out = enc.encode_into(record, _slice(raw, start, start + valid), labels[start:start + valid])
        assert out is record and np.array_equal(_np(record), want), (start, valid)
        # the same through `valid` over longer columns
        again = torch.zeros_like(record)
        enc.encode_into(again, _slice(raw, start, 100), labels[start:], valid=valid)
        assert torch.equal(again, record)
        p_dev = pred.predict_from(record, valid)
        p_host = pred.predict_from(torch.from_numpy(want).cuda(), valid)
        assert tuple(p_dev.shape) == (valid, 1) and torch.equal(p_dev, p_host)
        assert torch.isfinite(p_dev).all()
    # no labels: zeros in their place
    nolab = torch.full((layout.record_bytes,), 0xCD, dtype=torch.uint8, device="cuda")
    enc.encode_into(nolab, _slice(raw, 0, B))
    assert (layout.views(nolab)[2] == 0).all() and torch.equal(layout.views(nolab)[0], layout.views(
        torch.from_numpy(_host_record(layout, host, 0, B)).cuda())[0])
    with pytest.raises(ValueError):
        enc.encode_into(torch.zeros(layout.record_bytes + 8, dtype=torch.uint8, device="cuda"), _slice(raw, 0, B))
    with pytest.raises(ValueError):
        enc.encode_into(record, _slice(raw, 0, B + 1))                      # more samples than slots


def test_a_schema_without_sparse_or_dense_fields_gets_its_padding_rows():
    """RecordLayout keeps one row in the ids and the dense block even without such a field; encode_into zeroes it."""
    from deepfm_amd.data import DeviceFeatureEncoder
    from deepfm_amd.data.packed import PackedColumns, RecordLayout
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    rng = np.random.default_rng(8)
    n = 20
    for name, kind, col in (("x", FeatureType.DENSE, rng.normal(size=n)),
                            ("c", FeatureType.SPARSE, rng.integers(-4, 4, n))):
        enc = DeviceFeatureEncoder(DatasetSchema(fields={name: FieldSchema(name, kind, 0, 8)})).fit({name: col})
        labels = rng.random(n).astype(np.float32)
        cols = enc.transform({name: col}, labels)
        keys = R.fit_vocabulary(col)[0] if kind is FeatureType.SPARSE else None
        want_col = R.label_transform(keys, col) if keys is not None else R.minmax_transform(*R.minmax_fit(col), col)
        host = PackedColumns(enc.schema, {name: want_col}, labels)
        _same_columns(cols, host)
        layout = RecordLayout.of(enc.schema, 32)
        record = torch.full((layout.record_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
        enc.encode_into(record, {name: col}, labels)
        assert np.array_equal(_np(record), _host_record(layout, host, 0, n))
