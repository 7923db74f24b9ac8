"""CPU: MixedSchemaPredictor's eligibility (reasons before any device work), the mixed batch-record layout and
its host packing, and the record gather's C entry points."""
import json
import os
import re

import numpy as np
import pytest

from tests.helpers import cfg_of, fields_of, load, schema_from_fields
from tools_shared import criteo_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dfm_embedding_forward_record"]


def movielens_cfg(kind, **dnn):
    """The reference's configs/*_movielens.yaml model sections (dropout off: eval mode ignores it)."""
    from deepfm_amd.config import ExperimentConfig
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = 16
    cfg.dnn.hidden_units, cfg.dnn.dropout = [256, 128, 64], 0.0
    if kind == "xdeepfm":
        cfg.cin.layer_sizes, cfg.cin.split_half = [64], True
    if kind == "attention_deepfm":
        cfg.attention.num_heads, cfg.attention.attention_dim = 4, 64
        cfg.attention.num_layers, cfg.attention.use_residual = 1, True
    for k, v in dnn.items():
        setattr(cfg.dnn, k, v)
    return cfg


def _model(kind, fields=None, **dnn):
    from deepfm_amd.models import create_model
    fields = fields or fields_of(load("model_deepfm_movielens"))
    return create_model(kind, schema_from_fields(fields), movielens_cfg(kind, **dnn))


def test_movielens_golden_model_is_eligible():
    from deepfm_amd.models import create_model
    from deepfm_amd.training import ineligible_reason, mixed_ineligible_reason
    from tests.test_gpu_models_step import _config
    g = load("model_deepfm_movielens")
    model = create_model(cfg_of(g)["kind"], schema_from_fields(fields_of(g)), _config(cfg_of(g)))
    assert mixed_ineligible_reason(model) is None
    assert "staged gather needs" in ineligible_reason(model)     # FusedPredictor still refuses it


@pytest.mark.parametrize("kind", ["deepfm", "xdeepfm", "attention_deepfm"])
def test_reference_movielens_configs_are_eligible(kind):
    from deepfm_amd.training import mixed_ineligible_reason
    from deepfm_amd.training.predict import mixed_param_bytes
    model = _model(kind)
    assert mixed_ineligible_reason(model) is None
    assert mixed_param_bytes(model) == 4 * (76 * 16 + 4 * (2 * 4 + 4) + 2 * (2 * 8 + 4))   # 5.2 KB


def _fields_with(**dims):
    fields = json.loads(json.dumps(fields_of(load("model_deepfm_movielens"))))
    for f in fields:
        if f["name"] in dims:
            f["dim"] = dims[f["name"]]
    return fields


@pytest.mark.parametrize("fields,dnn,why", [
    (_fields_with(genres=6), {}, "not a multiple of 4"),
    (_fields_with(dow_sin=1024), {}, "over the record gather's cap"),
    (_fields_with(genres=520, zip_prefix=520, occupation=520), {}, "over the record gather's cap"),
    (None, {"activation": "gelu"}, "BatchNorm1d -> ReLU"),
    (None, {"use_batch_norm": False}, "BatchNorm1d -> ReLU"),
    (None, {"hidden_units": [32, 18]}, "multiples of 4"),
])
def test_ineligible_models_are_refused_with_the_reason(fields, dnn, why):
    from deepfm_amd.training import MixedSchemaPredictor, mixed_ineligible_reason
    model = _model("deepfm", fields, **dnn)             # on the CPU: the refusal comes before any device work
    assert why in mixed_ineligible_reason(model)
    with pytest.raises(ValueError, match=re.escape(why)):
        MixedSchemaPredictor(model, 64)


def test_fm_dim_outside_the_kernels_is_refused():
    from deepfm_amd.models import create_model
    from deepfm_amd.training import mixed_ineligible_reason
    cfg = movielens_cfg("deepfm")
    cfg.feature.fm_embed_dim = 12
    model = create_model("deepfm", schema_from_fields(_fields_with()), cfg)
    assert "fm_embed_dim 12" in mixed_ineligible_reason(model)


@pytest.mark.parametrize("B", [1, 7, 64, 4096])
def test_mixed_layout_equals_record_layout_without_sequence_fields(B):
    from deepfm_amd.data.packed import mixed_record_layout, record_layout
    schema = schema_from_fields(criteo_fields(1000, 16))
    ns, nd, o1, o2, nbytes = record_layout(schema, B)
    assert mixed_record_layout(schema, B) == (ns, nd, o1, o2, [], nbytes)


def _movielens_columns(n, rng):
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.synthetic import random_fields_batch
    fields = fields_of(load("model_deepfm_movielens"))
    feats = random_fields_batch(fields, n, rng, zero_frac=0.2)
    return fields, PackedColumns(schema_from_fields(fields), feats, (rng.random(n) < 0.3).astype(np.float32)), feats


@pytest.mark.parametrize("B,cnt", [(64, 64), (37, 20), (5, 1)])
def test_sequence_blocks_are_aligned_and_round_trip(B, cnt):
    from deepfm_amd.data.packed import (mixed_record_layout, record_layout, unpack_mixed_record,
                                        write_mixed_record)
    rng = np.random.default_rng(B)
    fields, cols, feats = _movielens_columns(100, rng)
    schema = cols.schema
    with pytest.raises(NotImplementedError):
        record_layout(schema, B)                        # the training layout still refuses SEQUENCE fields
    ns, nd, o1, o2, seq, nbytes = mixed_record_layout(schema, B)
    assert (ns, nd, len(seq)) == (9, 6, 1)
    assert o1 == ns * B * 8 and o2 == o1 + nd * B * 4
    assert all(off % 16 == 0 and off >= o2 + 4 * B for off in seq)
    assert nbytes == seq[-1] + B * 6 * 8
    assert len(cols.bags) == 1 and cols.bags[0].shape == (100, 6)
    out = np.full(nbytes, 0xAB, dtype=np.uint8)          # garbage: padding must be written, not assumed
    s = 10
    write_mixed_record(out, cols, B, s, s + cnt)
    batch, labels = unpack_mixed_record(schema, out, B)
    for f in fields:
        got, want = batch[f["name"]], feats[f["name"]]
        assert got.shape == ((B, 6) if f["type"] == "sequence" else (B,))
        assert np.array_equal(got[:cnt], want[s:s + cnt]), f["name"]
        assert not got[cnt:].any(), f["name"]
    assert np.array_equal(labels[:cnt], cols.labels[s:s + cnt]) and not labels[cnt:].any()


def test_packed_columns_check_sequence_shapes():
    from deepfm_amd.data.packed import PackedColumns
    rng = np.random.default_rng(0)
    fields, cols, feats = _movielens_columns(50, rng)
    with pytest.raises(ValueError, match="genres"):
        PackedColumns(cols.schema, dict(feats, genres=feats["genres"][:, :5]), cols.labels)
    with pytest.raises(TypeError, match="genres"):
        PackedColumns(cols.schema, dict(feats, genres=feats["genres"].astype(np.float32)), cols.labels)


def test_new_entry_points_are_declared_exported_and_bound():
    from deepfm_amd import _lib
    import deepfm_amd.training as T
    text = open(os.path.join(ROOT, "include", "deepfm_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dfm_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    cap = re.search(r"#define DFM_RECORD_PARAM_LDS_BYTES (\d+)", text)
    assert cap and int(cap.group(1)) == _lib.RECORD_PARAM_LDS_BYTES
    for name in ("MixedSchemaPredictor", "mixed_ineligible_reason"):
        assert hasattr(T, name), name
