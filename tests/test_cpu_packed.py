"""CPU: packed columnar batches (deepfm_amd/data/packed.py) — layout, epoch coverage, dict view."""
import numpy as np
import pytest
import torch

from deepfm_amd.data.packed import (PackedBatchLoader, PackedColumns, RecordLayout, mixed_record_layout, record_layout,
                                    unpack_record)
from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
from tests.helpers import schema_from_fields
from tools_shared import criteo_fields


def _dataset(n=1000, seed=0):
    fields = criteo_fields(50, 8, n_sparse=3, n_dense=2)
    rng = np.random.default_rng(seed)
    feats = {f["name"]: (rng.integers(0, 50, n) if f["type"] == "sparse" else rng.random(n).astype(np.float32)) for f in fields}
    labels = (rng.random(n) < 0.3).astype(np.float32)
    return schema_from_fields(fields), feats, labels


def test_record_layout_matches_the_train_step_packing():
    schema, feats, labels = _dataset()
    B = 64
    ns, nd, o1, o2, nbytes = record_layout(schema, B)
    assert (ns, nd) == (3, 2) and o1 == 3 * B * 8 and o2 == o1 + 2 * B * 4 and nbytes == o2 + B * 4
    cols = PackedColumns(schema, feats, labels)
    loader = PackedBatchLoader(cols, B)
    out = np.zeros(nbytes, np.uint8)
    loader.write(out, 2)
    batch, lab = unpack_record(schema, torch.from_numpy(out), B)
    for name in schema.fields:
        want = feats[name][2 * B:3 * B]
        got = batch[name].numpy()
        assert got.dtype == (np.int64 if np.issubdtype(want.dtype, np.integer) else np.float32)
        assert np.array_equal(got, want.astype(got.dtype))
    assert np.array_equal(lab.numpy(), labels[2 * B:3 * B])


def test_shuffled_epoch_visits_every_sample_once_and_reshuffles():
    schema, feats, labels = _dataset(n=1024)
    feats["C1"] = np.arange(1024)            # sample identity rides in the first id column
    cols = PackedColumns(schema, feats, labels)
    B = 128
    loader = PackedBatchLoader(cols, B, shuffle=True, seed=5)
    _, _, o1, o2, nbytes = record_layout(schema, B)
    seen = []
    for epoch in range(2):
        loader.set_epoch(epoch)
        out = np.zeros(nbytes, np.uint8)
        got = []
        for k in range(len(loader)):
            loader.write(out, k)
            batch, lab = unpack_record(schema, torch.from_numpy(out.copy()), B)
            ids = batch["C1"].numpy()
            got.append(ids)
            assert np.array_equal(lab.numpy(), labels[ids])                 # rows stay aligned across columns
            assert np.array_equal(batch["I1"].numpy(), feats["I1"][ids])
        seen.append(np.concatenate(got))
        assert np.array_equal(np.sort(seen[-1]), np.arange(1024))
    assert not np.array_equal(seen[0], seen[1])


def test_contract_errors():
    schema, feats, labels = _dataset()
    with pytest.raises(KeyError):
        PackedColumns(schema, {k: v for k, v in feats.items() if k != "C2"}, labels)
    with pytest.raises(TypeError):
        PackedColumns(schema, dict(feats, C1=feats["C1"].astype(np.float32)), labels)
    cols = PackedColumns(schema, feats, labels)
    with pytest.raises(NotImplementedError):
        PackedBatchLoader(cols, 64, drop_last=False)
    with pytest.raises(ValueError):
        PackedBatchLoader(cols, 5000)


def _sequence_dataset(n, seed=1):
    """SPARSE, DENSE and two SEQUENCE fields of different lengths, interleaved."""
    specs = [FieldSchema("u", FeatureType.SPARSE, 40, 8), FieldSchema("g", FeatureType.SEQUENCE, 20, 8, max_length=5),
             FieldSchema("x", FeatureType.DENSE), FieldSchema("i", FeatureType.SPARSE, 30, 8),
             FieldSchema("t", FeatureType.SEQUENCE, 10, 8, max_length=3)]
    rng = np.random.default_rng(seed)
    feats = {}
    for f in specs:
        if f.feature_type is FeatureType.DENSE:
            feats[f.name] = rng.random(n).astype(np.float32) + 1.0           # never 0: padding is told apart
        else:
            shape = (n, f.max_length) if f.feature_type is FeatureType.SEQUENCE else n
            feats[f.name] = rng.integers(1, f.vocabulary_size, shape)
    return DatasetSchema(fields={f.name: f for f in specs}), feats, rng.random(n).astype(np.float32) + 1.0


@pytest.mark.parametrize("B", [1, 7, 4096])
@pytest.mark.parametrize("kind", ["uniform", "sequence"])
def test_one_layout_offsets_write_unpack_and_shuffled_write(kind, B):
    n = 5000
    schema, feats, labels = _dataset(n) if kind == "uniform" else _sequence_dataset(n)
    lay = RecordLayout.of(schema, B)
    # offsets and size: the public tuple functions
    ns, nd, o1, o2, seq, nbytes = mixed_record_layout(schema, B)
    assert (lay.n_sparse, lay.n_dense, lay.dense_offset, lay.labels_offset, list(lay.seq_offsets), lay.record_bytes) \
        == (ns, nd, o1, o2, seq, nbytes)
    assert lay.ids_offset == 0 and len(seq) == (2 if kind == "sequence" else 0)
    if kind == "uniform":
        assert record_layout(schema, B) == (ns, nd, o1, o2, nbytes)
    else:
        with pytest.raises(NotImplementedError):
            record_layout(schema, B)
        with pytest.raises(NotImplementedError):
            RecordLayout.of(schema, B, sequences=False)
    # per field: the offset of its column inside its block, schema order
    si = di = qi = 0
    for spec, off in zip(schema.fields.values(), lay.field_offsets):
        if spec.feature_type is FeatureType.SPARSE:
            assert off == si * B * 8; si += 1
        elif spec.feature_type is FeatureType.DENSE:
            assert off == o1 + di * B * 4; di += 1
        else:
            assert off == seq[qi] and off % 16 == 0; qi += 1
    cols = PackedColumns(schema, feats, labels)
    # write then unpack: the columns, then an all-zero padding tail
    for cnt in sorted({B, (B + 1) // 2}):
        out = np.full(nbytes, 0xAB, dtype=np.uint8)        # garbage: padding must be written, not assumed
        s = 11
        lay.write(out, cols, s, s + cnt)
        batch, lab = lay.unpack(out)
        assert list(batch) == list(schema.fields)
        for name, spec in schema.fields.items():
            got = batch[name]
            assert got.shape == ((B, spec.max_length) if spec.feature_type is FeatureType.SEQUENCE else (B,))
            assert got.dtype == (np.float32 if spec.feature_type is FeatureType.DENSE else np.int64)
            assert np.array_equal(got[:cnt], feats[name][s:s + cnt]), name
            assert not got[cnt:].any(), name
        assert np.array_equal(lab[:cnt], labels[s:s + cnt]) and not lab[cnt:].any()
    # the shuffled write is fancy indexing
    idx = np.random.default_rng(B).permutation(n)[:B]
    out = np.full(nbytes, 0xAB, dtype=np.uint8)
    lay.write_indexed(out, cols, idx)
    batch, lab = lay.unpack(out)
    for name in schema.fields:
        assert np.array_equal(batch[name], feats[name][idx]), name
    assert np.array_equal(lab, labels[idx])
