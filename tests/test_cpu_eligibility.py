"""CPU: every public eligibility predicate of the fused paths, pinned answer for answer.

The matrix: the three model kinds on bench.py's (Criteo) schema and on MovieLens, and every refusal that
tests/test_cpu_predict.py, test_cpu_mixed_predict.py, test_cpu_mixed_train.py and test_cpu_mixed_models_train.py
construct; each in ``dense`` and ``rowsparse`` grad mode, in train() and eval(), asked with batch_size None and 4096.
TABLE holds, per case and state, the code (index into ANSWERS) of what each of PREDICATES answers: a reason string,
None, the chosen class's name, a bool, or "!<Exception>" where the predicate cannot answer for such an object.  The
predicates that existed before training/eligibility.py answer what they answered then, string for string.
"""
import pytest

import torch

from tests.helpers import cfg_of, fields_of, load, schema_from_fields
from tests.test_gpu_models_step import _config

STATES = [(g, m) for g in ("dense", "rowsparse") for m in ("train", "eval")]
BATCHES = (None, 4096)
UNIFORM_STEPS = ["FusedDeepFMStep", "FusedXDeepFMStep", "FusedAttentionDeepFMStep"]
STEPS = UNIFORM_STEPS + ["FusedMixedDeepFMStep", "FusedMixedXDeepFMStep", "FusedMixedAttentionDeepFMStep"]
PREDICATES = ["ineligible_reason", "mixed_ineligible_reason", "record_gather_reason", "mixed_train_ineligible_reason",
              "mixed_step_ineligible_reason", "mixed_step_class", "fused_step_class"] + \
    [s + ".eligible" for s in STEPS] + [s + ".ineligible_reason" for s in STEPS]


def _bench(kind):
    """bench.py's models: the headline DeepFM and the xDeepFM / AttentionDeepFM extra configurations."""
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.synthetic import criteo_fields
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    D = 32 if kind == "attention_deepfm" else 16
    cfg.feature.fm_embed_dim = D
    if kind == "xdeepfm":
        cfg.cin.layer_sizes = [128, 128, 128]
    return create_model(kind, schema_from_fields(criteo_fields(1000, D)), cfg)


def _golden(case, **dnn):
    """tests/test_cpu_predict.py's models: a golden case's own configuration."""
    from deepfm_amd.models import create_model
    g = load(case)
    c = cfg_of(g)
    cfg = _config(c)
    for k, v in dnn.items():
        setattr(cfg.dnn, k, v)
    return create_model(c["kind"], schema_from_fields(fields_of(g)), cfg)


def _released():
    model = _golden("model_deepfm")
    name = next(n for n, s in model.schema.fields.items() if s.feature_type.name == "SPARSE")
    w = model.embedding.second_order_embeddings[name].weight
    w.data = w.data[:0]                             # what TableShard.release_foreign leaves behind
    return model


def _movielens():
    return fields_of(load("model_deepfm_movielens"))


def _with(**dims):
    return [dict(f, dim=dims.get(f["name"], f["dim"])) for f in _movielens()]


def _reference(kind, fields=None, fm_dim=16, **dnn):
    """tests/test_cpu_mixed_predict.py's models: the reference's *_movielens.yaml model sections."""
    from deepfm_amd.models import create_model
    from tests.test_cpu_mixed_predict import movielens_cfg
    cfg = movielens_cfg(kind, **dnn)
    cfg.feature.fm_embed_dim = fm_dim
    return create_model(kind, schema_from_fields(fields or _movielens()), cfg)


def _small(kind, fields=None, **kw):
    """tests/test_cpu_mixed_train.py's and tests/test_cpu_mixed_models_train.py's models."""
    from tests.test_cpu_mixed_models_train import _model
    return _model(fields or _movielens(), kind, **kw)


def _gemm_path_off():
    model = _small("attention_deepfm")
    model.attention.layers[0].gemm_path = False
    return model


class Other(torch.nn.Module):
    pass


UNIFORM = [dict(name=f"C{i}", type="sparse", vocab=50, dim=16, max_len=1, combiner="mean") for i in range(3)] + \
          [dict(name="I0", type="dense", vocab=0, dim=16, max_len=1, combiner="mean")]
MANY = [dict(name=f"P{i}", type="sparse", vocab=10, dim=32, max_len=1, combiner="mean") for i in range(20)]
KINDS = ("deepfm", "xdeepfm", "attention_deepfm")


def cases():
    c = {}
    for k in KINDS:
        c[f"bench/{k}"] = lambda k=k: _bench(k)
        c[f"movielens/{k}"] = lambda k=k: _small(k)
        c[f"movielens-reference/{k}"] = lambda k=k: _reference(k)
        c[f"golden/model_{k}"] = lambda k=k: _golden(f"model_{k}")
        # the refusals of the fused mixed-schema steps, per model kind
        c[f"uniform/{k}"] = lambda k=k: _small(k, UNIFORM)
        c[f"max-bag/{k}"] = lambda k=k: _small(k, [dict(f, combiner="max") if f["type"] == "sequence" else f
                                                   for f in _movielens()])
        c[f"no-batch-norm/{k}"] = lambda k=k: _small(k, use_batch_norm=False)
        c[f"last-width-24/{k}"] = lambda k=k: _small(k, hidden=(64, 24))
        c[f"many-projections/{k}"] = lambda k=k: _small(k, MANY)
        c[f"long-bag/{k}"] = lambda k=k: _small(k, _movielens() + [
            dict(name="hist", type="sequence", vocab=50, dim=8, max_len=64, combiner="mean")])
        c[f"gender-width-6/{k}"] = lambda k=k: _small(k, _with(gender=6))
    # the predictors' refusals
    c["golden/model_deepfm_movielens"] = lambda: _golden("model_deepfm_movielens")
    c["golden/model_deepfm/gelu"] = lambda: _golden("model_deepfm", activation="gelu")
    c["golden/model_xdeepfm/no-batch-norm"] = lambda: _golden("model_xdeepfm", use_batch_norm=False)
    c["golden/model_deepfm/hidden-32-18"] = lambda: _golden("model_deepfm", hidden_units=[32, 18])
    c["golden/model_deepfm/released-table"] = _released
    c["movielens-reference/genres-width-6"] = lambda: _reference("deepfm", _with(genres=6))
    c["movielens-reference/dow_sin-width-1024"] = lambda: _reference("deepfm", _with(dow_sin=1024))
    c["movielens-reference/three-widths-520"] = lambda: _reference(
        "deepfm", _with(genres=520, zip_prefix=520, occupation=520))
    c["movielens-reference/gelu"] = lambda: _reference("deepfm", activation="gelu")
    c["movielens-reference/no-batch-norm"] = lambda: _reference("deepfm", use_batch_norm=False)
    c["movielens-reference/hidden-32-18"] = lambda: _reference("deepfm", hidden_units=[32, 18])
    c["movielens-reference/fm-dim-12"] = lambda: _reference("deepfm", fm_dim=12)
    # model-specific refusals and the shapes the mixed steps were built for
    c["cin/1-8"] = lambda: _small("xdeepfm", cin_sizes=(1, 8))
    c["cin/2-8"] = lambda: _small("xdeepfm", cin_sizes=(2, 8))
    c["cin/16-16-8"] = lambda: _small("xdeepfm", hidden=(32, 32), cin_sizes=(16, 16, 8))
    c["cin/24-12"] = lambda: _small("xdeepfm", hidden=(32, 32), cin_sizes=(24, 12))
    c["attention/4-heads-dim-64"] = lambda: _small("attention_deepfm", hidden=(32, 32), heads=4, A=64)
    c["attention/dim-520"] = lambda: _small("attention_deepfm", heads=2, A=520)
    c["attention/gemm-path-off"] = _gemm_path_off
    c["other-module"] = Other
    return c


ANSWERS = [
    None,  # 0
    True,  # 1
    False,  # 2
    ("field 'gender': embedding_dim 4 with fm_embed_dim 16: the staged gather needs embedding_dim == "
     'fm_embed_dim, a multiple of 4'),  # 3
    ('no fused mixed-schema step for AttentionDeepFM: DeepFM only (xDeepFM and AttentionDeepFM are the '
     'next step, DESIGN.md section 9)'),  # 4
    'FusedMixedAttentionDeepFMStep',  # 5
    'FusedDeepFMStep does not take AttentionDeepFM (fused_step_class(model) names the step)',  # 6
    'FusedXDeepFMStep does not take AttentionDeepFM (fused_step_class(model) names the step)',  # 7
    "the embedding must be in 'rowsparse' grad mode (set_grad_mode('rowsparse'))",  # 8
    'FusedMixedXDeepFMStep does not take AttentionDeepFM (mixed_step_class(model) names the step)',  # 9
    'the model must be in training mode',  # 10
    "the embedding must be in 'dense' grad mode (its tables are dense parameters of the flat buffer)",  # 11
    'FusedAttentionDeepFMStep',  # 12
    "attention blocks outside the fused attention kernels' shapes",  # 13
    ("attention over 16 fields with attention_dim 520 and 2 heads is outside the attention core kernel's "
     'shapes (dfm_attention_core_supported)'),  # 14
    'an attention block does not run on the GEMM path (gemm_path is off)',  # 15
    "uniform schema: use the row-sparse step (set_grad_mode('rowsparse') and fused_step_class(model))",  # 16
    'FusedXDeepFMStep does not take DeepFM (fused_step_class(model) names the step)',  # 17
    'FusedAttentionDeepFMStep does not take DeepFM (fused_step_class(model) names the step)',  # 18
    'FusedMixedXDeepFMStep does not take DeepFM (mixed_step_class(model) names the step)',  # 19
    'FusedMixedAttentionDeepFMStep does not take DeepFM (mixed_step_class(model) names the step)',  # 20
    'FusedDeepFMStep',  # 21
    ('no fused mixed-schema step for xDeepFM: DeepFM only (xDeepFM and AttentionDeepFM are the next step, '
     'DESIGN.md section 9)'),  # 22
    'FusedDeepFMStep does not take xDeepFM (fused_step_class(model) names the step)',  # 23
    'FusedAttentionDeepFMStep does not take xDeepFM (fused_step_class(model) names the step)',  # 24
    'FusedMixedAttentionDeepFMStep does not take xDeepFM (mixed_step_class(model) names the step)',  # 25
    'FusedXDeepFMStep',  # 26
    'CIN layer 0 has 1 feature maps: too small to split in half',  # 27
    'FusedMixedXDeepFMStep',  # 28
    ("field 'gender': embedding_dim 6 with fm_embed_dim 16: the staged gather needs embedding_dim == "
     'fm_embed_dim, a multiple of 4'),  # 29
    "field 'gender': embedding_dim 6 is not a multiple of 4 (16-byte row pieces)",  # 30
    ('the DNN tower is not fusable: Linear -> BatchNorm1d (affine, momentum) -> ReLU, hidden widths '
     'multiples of 4, the last one a multiple of 32 and <= 256, input width a multiple of 4'),  # 31
    "the DNN tower must be Linear -> BatchNorm1d -> ReLU (use_batch_norm=True, activation='relu')",  # 32
    'hidden widths [32, 18] must be multiples of 4',  # 33
    ("the embedding table of field 'C1' is released (field-sharded model, TableShard.released): call "
     'restore_tables() first'),  # 34
    'the embedding backward stages 78352 bytes of LDS for the widest field, over its cap of 65536',  # 35
    ("field 'P0': embedding_dim 32 with fm_embed_dim 16: the staged gather needs embedding_dim == "
     'fm_embed_dim, a multiple of 4'),  # 36
    "projection and DENSE parameters take 40960 bytes of LDS, over the record gather's cap of 32768",  # 37
    ("field 'genres' pools with max: the embedding backward's arg-max recompute is not built (mean and sum"
     ' bags only; train it in dense autograd mode)'),  # 38
    'FusedMixedDeepFMStep',  # 39
    "projection and DENSE parameters take 78656 bytes of LDS, over the record gather's cap of 32768",  # 40
    ("field 'user_id': embedding_dim 16 with fm_embed_dim 12: the staged gather needs embedding_dim == "
     'fm_embed_dim, a multiple of 4'),  # 41
    'fm_embed_dim 12: the record gather takes 4, 8, 16, 32 or 64',  # 42
    "field 'genres': embedding_dim 6 is not a multiple of 4 (16-byte row pieces)",  # 43
    "projection and DENSE parameters take 103520 bytes of LDS, over the record gather's cap of 32768",  # 44
    'no fused predictor for Other (DeepFM, xDeepFM and AttentionDeepFM only)',  # 45
    '!AttributeError',  # 46
    ('no fused mixed-schema step for Other: DeepFM only (xDeepFM and AttentionDeepFM are the next step, '
     'DESIGN.md section 9)'),  # 47
    'no fused mixed-schema step for Other: DeepFM, xDeepFM and AttentionDeepFM only',  # 48
    'no fused step for Other: DeepFM, xDeepFM and AttentionDeepFM only',  # 49
    'FusedMixedXDeepFMStep does not take Other (mixed_step_class(model) names the step)',  # 50
    'FusedMixedAttentionDeepFMStep does not take Other (mixed_step_class(model) names the step)',  # 51
]

TABLE = {
    'attention/4-heads-dim-64': [
        [3, 0, 0, 4, 0, 5, 5, 2, 2, 2, 2, 2, 1, 6, 7, 8, 4, 9, 0],  # dense/train
        [3, 0, 0, 4, 10, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 10],  # dense/eval
        [3, 0, 0, 4, 11, 0, 12, 2, 2, 1, 2, 2, 2, 6, 7, 0, 4, 9, 11],  # rowsparse/train
        [3, 0, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 11],  # rowsparse/eval
    ],
    'attention/dim-520': [
        [3, 13, 0, 4, 14, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 14],  # dense/train
        [3, 13, 0, 4, 10, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 10],  # dense/eval
        [3, 13, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 14, 4, 9, 11],  # rowsparse/train
        [3, 13, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 11],  # rowsparse/eval
    ],
    'attention/gemm-path-off': [
        [3, 13, 0, 4, 15, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 15],  # dense/train
        [3, 13, 0, 4, 10, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 10],  # dense/eval
        [3, 13, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 15, 4, 9, 11],  # rowsparse/train
        [3, 13, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 11],  # rowsparse/eval
    ],
    'bench/attention_deepfm': [
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 16],  # dense/train
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 16],  # dense/eval
        [0, 0, 0, 4, 16, 0, 12, 2, 2, 1, 2, 2, 2, 6, 7, 0, 4, 9, 16],  # rowsparse/train
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 16],  # rowsparse/eval
    ],
    'bench/deepfm': [
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/train
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/eval
        [0, 0, 0, 16, 16, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 16, 19, 20],  # rowsparse/train
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 16, 19, 20],  # rowsparse/eval
    ],
    'bench/xdeepfm': [
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 16, 25],  # dense/train
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 16, 25],  # dense/eval
        [0, 0, 0, 22, 16, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 16, 25],  # rowsparse/train
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 16, 25],  # rowsparse/eval
    ],
    'cin/1-8': [
        [3, 0, 0, 22, 27, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 27, 25],  # dense/train
        [3, 0, 0, 22, 10, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 10, 25],  # dense/eval
        [3, 0, 0, 22, 11, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 11, 25],  # rowsparse/train
        [3, 0, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 11, 25],  # rowsparse/eval
    ],
    'cin/16-16-8': [
        [3, 0, 0, 22, 0, 28, 28, 2, 2, 2, 2, 1, 2, 23, 8, 24, 22, 0, 25],  # dense/train
        [3, 0, 0, 22, 10, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 10, 25],  # dense/eval
        [3, 0, 0, 22, 11, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 11, 25],  # rowsparse/train
        [3, 0, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 11, 25],  # rowsparse/eval
    ],
    'cin/2-8': [
        [3, 0, 0, 22, 0, 28, 28, 2, 2, 2, 2, 1, 2, 23, 8, 24, 22, 0, 25],  # dense/train
        [3, 0, 0, 22, 10, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 10, 25],  # dense/eval
        [3, 0, 0, 22, 11, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 11, 25],  # rowsparse/train
        [3, 0, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 11, 25],  # rowsparse/eval
    ],
    'cin/24-12': [
        [3, 0, 0, 22, 0, 28, 28, 2, 2, 2, 2, 1, 2, 23, 8, 24, 22, 0, 25],  # dense/train
        [3, 0, 0, 22, 10, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 10, 25],  # dense/eval
        [3, 0, 0, 22, 11, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 11, 25],  # rowsparse/train
        [3, 0, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 11, 25],  # rowsparse/eval
    ],
    'gender-width-6/attention_deepfm': [
        [29, 30, 30, 4, 30, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 30],  # dense/train
        [29, 30, 30, 4, 30, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 30],  # dense/eval
        [29, 30, 30, 4, 30, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 31, 4, 9, 30],  # rowsparse/train
        [29, 30, 30, 4, 30, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 30],  # rowsparse/eval
    ],
    'gender-width-6/deepfm': [
        [29, 30, 30, 30, 30, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 30, 19, 20],  # dense/train
        [29, 30, 30, 30, 30, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 30, 19, 20],  # dense/eval
        [29, 30, 30, 30, 30, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 30, 19, 20],  # rowsparse/train
        [29, 30, 30, 30, 30, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 30, 19, 20],  # rowsparse/eval
    ],
    'gender-width-6/xdeepfm': [
        [29, 30, 30, 22, 30, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 30, 25],  # dense/train
        [29, 30, 30, 22, 30, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 30, 25],  # dense/eval
        [29, 30, 30, 22, 30, 0, 0, 2, 2, 2, 2, 2, 2, 23, 31, 24, 22, 30, 25],  # rowsparse/train
        [29, 30, 30, 22, 30, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 30, 25],  # rowsparse/eval
    ],
    'golden/model_attention_deepfm': [
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 16],  # dense/train
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 16],  # dense/eval
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 31, 4, 9, 16],  # rowsparse/train
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 16],  # rowsparse/eval
    ],
    'golden/model_deepfm': [
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/train
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/eval
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 16, 19, 20],  # rowsparse/train
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 16, 19, 20],  # rowsparse/eval
    ],
    'golden/model_deepfm/gelu': [
        [32, 32, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/train
        [32, 32, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/eval
        [32, 32, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 16, 19, 20],  # rowsparse/train
        [32, 32, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 16, 19, 20],  # rowsparse/eval
    ],
    'golden/model_deepfm/hidden-32-18': [
        [33, 33, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/train
        [33, 33, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/eval
        [33, 33, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 16, 19, 20],  # rowsparse/train
        [33, 33, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 16, 19, 20],  # rowsparse/eval
    ],
    'golden/model_deepfm/released-table': [
        [34, 34, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/train
        [34, 34, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/eval
        [34, 34, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 16, 19, 20],  # rowsparse/train
        [34, 34, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 16, 19, 20],  # rowsparse/eval
    ],
    'golden/model_deepfm_movielens': [
        [3, 0, 0, 31, 31, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 31, 19, 20],  # dense/train
        [3, 0, 0, 10, 10, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 10, 19, 20],  # dense/eval
        [3, 0, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 11, 19, 20],  # rowsparse/train
        [3, 0, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 11, 19, 20],  # rowsparse/eval
    ],
    'golden/model_xdeepfm': [
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 16, 25],  # dense/train
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 16, 25],  # dense/eval
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 31, 24, 22, 16, 25],  # rowsparse/train
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 16, 25],  # rowsparse/eval
    ],
    'golden/model_xdeepfm/no-batch-norm': [
        [32, 32, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 16, 25],  # dense/train
        [32, 32, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 16, 25],  # dense/eval
        [32, 32, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 31, 24, 22, 16, 25],  # rowsparse/train
        [32, 32, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 16, 25],  # rowsparse/eval
    ],
    'last-width-24/attention_deepfm': [
        [3, 0, 0, 4, 31, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 31],  # dense/train
        [3, 0, 0, 4, 10, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 10],  # dense/eval
        [3, 0, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 31, 4, 9, 11],  # rowsparse/train
        [3, 0, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 11],  # rowsparse/eval
    ],
    'last-width-24/deepfm': [
        [3, 0, 0, 31, 31, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 31, 19, 20],  # dense/train
        [3, 0, 0, 10, 10, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 10, 19, 20],  # dense/eval
        [3, 0, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 11, 19, 20],  # rowsparse/train
        [3, 0, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 11, 19, 20],  # rowsparse/eval
    ],
    'last-width-24/xdeepfm': [
        [3, 0, 0, 22, 31, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 31, 25],  # dense/train
        [3, 0, 0, 22, 10, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 10, 25],  # dense/eval
        [3, 0, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 31, 24, 22, 11, 25],  # rowsparse/train
        [3, 0, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 11, 25],  # rowsparse/eval
    ],
    'long-bag/attention_deepfm': [
        [3, 0, 0, 4, 35, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 35],  # dense/train
        [3, 0, 0, 4, 35, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 35],  # dense/eval
        [3, 0, 0, 4, 35, 0, 12, 2, 2, 1, 2, 2, 2, 6, 7, 0, 4, 9, 35],  # rowsparse/train
        [3, 0, 0, 4, 35, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 35],  # rowsparse/eval
    ],
    'long-bag/deepfm': [
        [3, 0, 0, 35, 35, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 35, 19, 20],  # dense/train
        [3, 0, 0, 35, 35, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 35, 19, 20],  # dense/eval
        [3, 0, 0, 35, 35, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 35, 19, 20],  # rowsparse/train
        [3, 0, 0, 35, 35, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 35, 19, 20],  # rowsparse/eval
    ],
    'long-bag/xdeepfm': [
        [3, 0, 0, 22, 35, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 35, 25],  # dense/train
        [3, 0, 0, 22, 35, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 35, 25],  # dense/eval
        [3, 0, 0, 22, 35, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 35, 25],  # rowsparse/train
        [3, 0, 0, 22, 35, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 35, 25],  # rowsparse/eval
    ],
    'many-projections/attention_deepfm': [
        [36, 37, 37, 4, 37, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 37],  # dense/train
        [36, 37, 37, 4, 37, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 37],  # dense/eval
        [36, 37, 37, 4, 37, 0, 12, 2, 2, 1, 2, 2, 2, 6, 7, 0, 4, 9, 37],  # rowsparse/train
        [36, 37, 37, 4, 37, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 37],  # rowsparse/eval
    ],
    'many-projections/deepfm': [
        [36, 37, 37, 37, 37, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 37, 19, 20],  # dense/train
        [36, 37, 37, 37, 37, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 37, 19, 20],  # dense/eval
        [36, 37, 37, 37, 37, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 37, 19, 20],  # rowsparse/train
        [36, 37, 37, 37, 37, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 37, 19, 20],  # rowsparse/eval
    ],
    'many-projections/xdeepfm': [
        [36, 37, 37, 22, 37, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 37, 25],  # dense/train
        [36, 37, 37, 22, 37, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 37, 25],  # dense/eval
        [36, 37, 37, 22, 37, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 37, 25],  # rowsparse/train
        [36, 37, 37, 22, 37, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 37, 25],  # rowsparse/eval
    ],
    'max-bag/attention_deepfm': [
        [3, 0, 0, 4, 38, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 38],  # dense/train
        [3, 0, 0, 4, 38, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 38],  # dense/eval
        [3, 0, 0, 4, 38, 0, 12, 2, 2, 1, 2, 2, 2, 6, 7, 0, 4, 9, 38],  # rowsparse/train
        [3, 0, 0, 4, 38, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 38],  # rowsparse/eval
    ],
    'max-bag/deepfm': [
        [3, 0, 0, 38, 38, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 38, 19, 20],  # dense/train
        [3, 0, 0, 38, 38, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 38, 19, 20],  # dense/eval
        [3, 0, 0, 38, 38, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 38, 19, 20],  # rowsparse/train
        [3, 0, 0, 38, 38, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 38, 19, 20],  # rowsparse/eval
    ],
    'max-bag/xdeepfm': [
        [3, 0, 0, 22, 38, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 38, 25],  # dense/train
        [3, 0, 0, 22, 38, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 38, 25],  # dense/eval
        [3, 0, 0, 22, 38, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 38, 25],  # rowsparse/train
        [3, 0, 0, 22, 38, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 38, 25],  # rowsparse/eval
    ],
    'movielens-reference/attention_deepfm': [
        [3, 0, 0, 4, 0, 5, 5, 2, 2, 2, 2, 2, 1, 6, 7, 8, 4, 9, 0],  # dense/train
        [3, 0, 0, 4, 10, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 10],  # dense/eval
        [3, 0, 0, 4, 11, 0, 12, 2, 2, 1, 2, 2, 2, 6, 7, 0, 4, 9, 11],  # rowsparse/train
        [3, 0, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 11],  # rowsparse/eval
    ],
    'movielens-reference/deepfm': [
        [3, 0, 0, 0, 0, 39, 39, 2, 2, 2, 1, 2, 2, 8, 17, 18, 0, 19, 20],  # dense/train
        [3, 0, 0, 10, 10, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 10, 19, 20],  # dense/eval
        [3, 0, 0, 11, 11, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 11, 19, 20],  # rowsparse/train
        [3, 0, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 11, 19, 20],  # rowsparse/eval
    ],
    'movielens-reference/dow_sin-width-1024': [
        [3, 40, 40, 40, 40, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 40, 19, 20],  # dense/train
        [3, 40, 40, 40, 40, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 40, 19, 20],  # dense/eval
        [3, 40, 40, 40, 40, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 40, 19, 20],  # rowsparse/train
        [3, 40, 40, 40, 40, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 40, 19, 20],  # rowsparse/eval
    ],
    'movielens-reference/fm-dim-12': [
        [41, 42, 42, 42, 42, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 42, 19, 20],  # dense/train
        [41, 42, 42, 42, 42, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 42, 19, 20],  # dense/eval
        [41, 42, 42, 42, 42, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 42, 19, 20],  # rowsparse/train
        [41, 42, 42, 42, 42, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 42, 19, 20],  # rowsparse/eval
    ],
    'movielens-reference/gelu': [
        [3, 32, 0, 31, 31, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 31, 19, 20],  # dense/train
        [3, 32, 0, 10, 10, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 10, 19, 20],  # dense/eval
        [3, 32, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 11, 19, 20],  # rowsparse/train
        [3, 32, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 11, 19, 20],  # rowsparse/eval
    ],
    'movielens-reference/genres-width-6': [
        [3, 43, 43, 43, 43, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 43, 19, 20],  # dense/train
        [3, 43, 43, 43, 43, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 43, 19, 20],  # dense/eval
        [3, 43, 43, 43, 43, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 43, 19, 20],  # rowsparse/train
        [3, 43, 43, 43, 43, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 43, 19, 20],  # rowsparse/eval
    ],
    'movielens-reference/hidden-32-18': [
        [3, 33, 0, 31, 31, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 31, 19, 20],  # dense/train
        [3, 33, 0, 10, 10, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 10, 19, 20],  # dense/eval
        [3, 33, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 11, 19, 20],  # rowsparse/train
        [3, 33, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 11, 19, 20],  # rowsparse/eval
    ],
    'movielens-reference/no-batch-norm': [
        [3, 32, 0, 31, 31, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 31, 19, 20],  # dense/train
        [3, 32, 0, 10, 10, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 10, 19, 20],  # dense/eval
        [3, 32, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 11, 19, 20],  # rowsparse/train
        [3, 32, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 11, 19, 20],  # rowsparse/eval
    ],
    'movielens-reference/three-widths-520': [
        [3, 44, 44, 44, 44, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 44, 19, 20],  # dense/train
        [3, 44, 44, 44, 44, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 44, 19, 20],  # dense/eval
        [3, 44, 44, 44, 44, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 44, 19, 20],  # rowsparse/train
        [3, 44, 44, 44, 44, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 44, 19, 20],  # rowsparse/eval
    ],
    'movielens-reference/xdeepfm': [
        [3, 0, 0, 22, 0, 28, 28, 2, 2, 2, 2, 1, 2, 23, 8, 24, 22, 0, 25],  # dense/train
        [3, 0, 0, 22, 10, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 10, 25],  # dense/eval
        [3, 0, 0, 22, 11, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 11, 25],  # rowsparse/train
        [3, 0, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 11, 25],  # rowsparse/eval
    ],
    'movielens/attention_deepfm': [
        [3, 0, 0, 4, 0, 5, 5, 2, 2, 2, 2, 2, 1, 6, 7, 8, 4, 9, 0],  # dense/train
        [3, 0, 0, 4, 10, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 10],  # dense/eval
        [3, 0, 0, 4, 11, 0, 12, 2, 2, 1, 2, 2, 2, 6, 7, 0, 4, 9, 11],  # rowsparse/train
        [3, 0, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 11],  # rowsparse/eval
    ],
    'movielens/deepfm': [
        [3, 0, 0, 0, 0, 39, 39, 2, 2, 2, 1, 2, 2, 8, 17, 18, 0, 19, 20],  # dense/train
        [3, 0, 0, 10, 10, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 10, 19, 20],  # dense/eval
        [3, 0, 0, 11, 11, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 11, 19, 20],  # rowsparse/train
        [3, 0, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 11, 19, 20],  # rowsparse/eval
    ],
    'movielens/xdeepfm': [
        [3, 0, 0, 22, 0, 28, 28, 2, 2, 2, 2, 1, 2, 23, 8, 24, 22, 0, 25],  # dense/train
        [3, 0, 0, 22, 10, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 10, 25],  # dense/eval
        [3, 0, 0, 22, 11, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 11, 25],  # rowsparse/train
        [3, 0, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 11, 25],  # rowsparse/eval
    ],
    'no-batch-norm/attention_deepfm': [
        [3, 32, 0, 4, 31, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 31],  # dense/train
        [3, 32, 0, 4, 10, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 10],  # dense/eval
        [3, 32, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 31, 4, 9, 11],  # rowsparse/train
        [3, 32, 0, 4, 11, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 11],  # rowsparse/eval
    ],
    'no-batch-norm/deepfm': [
        [3, 32, 0, 31, 31, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 31, 19, 20],  # dense/train
        [3, 32, 0, 10, 10, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 10, 19, 20],  # dense/eval
        [3, 32, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 31, 17, 18, 11, 19, 20],  # rowsparse/train
        [3, 32, 0, 11, 11, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 11, 19, 20],  # rowsparse/eval
    ],
    'no-batch-norm/xdeepfm': [
        [3, 32, 0, 22, 31, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 31, 25],  # dense/train
        [3, 32, 0, 22, 10, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 10, 25],  # dense/eval
        [3, 32, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 31, 24, 22, 11, 25],  # rowsparse/train
        [3, 32, 0, 22, 11, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 11, 25],  # rowsparse/eval
    ],
    'other-module': [45, 45, 46, 47, 48, 0, 0, 2, 2, 2, 2, 2, 2, 49, 49, 49, 47, 50, 51],
    'uniform/attention_deepfm': [
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 16],  # dense/train
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 8, 4, 9, 16],  # dense/eval
        [0, 0, 0, 4, 16, 0, 12, 2, 2, 1, 2, 2, 2, 6, 7, 0, 4, 9, 16],  # rowsparse/train
        [0, 0, 0, 4, 16, 0, 0, 2, 2, 2, 2, 2, 2, 6, 7, 10, 4, 9, 16],  # rowsparse/eval
    ],
    'uniform/deepfm': [
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/train
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 8, 17, 18, 16, 19, 20],  # dense/eval
        [0, 0, 0, 16, 16, 0, 21, 1, 2, 2, 2, 2, 2, 0, 17, 18, 16, 19, 20],  # rowsparse/train
        [0, 0, 0, 16, 16, 0, 0, 2, 2, 2, 2, 2, 2, 10, 17, 18, 16, 19, 20],  # rowsparse/eval
    ],
    'uniform/xdeepfm': [
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 16, 25],  # dense/train
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 8, 24, 22, 16, 25],  # dense/eval
        [0, 0, 0, 22, 16, 0, 26, 2, 1, 2, 2, 2, 2, 23, 0, 24, 22, 16, 25],  # rowsparse/train
        [0, 0, 0, 22, 16, 0, 0, 2, 2, 2, 2, 2, 2, 23, 10, 24, 22, 16, 25],  # rowsparse/eval
    ],
}


def _call(fn, *args):
    try:
        out = fn(*args)
    except Exception as e:                       # a predicate that cannot answer for this object: pinned as well
        return "!" + type(e).__name__
    return out.__name__ if isinstance(out, type) else out


def _per_batch(fn, model):
    a, b = (_call(fn, model, bs) for bs in BATCHES)
    return a if a == b else (a, b)


def snapshot(model, grad, mode):
    """{predicate: answer} of ``model`` put into one state; an answer that depends on the batch size is a
    (None, 4096) pair."""
    import deepfm_amd.training as T
    from deepfm_amd.training import fused_step, mixed_step, predict
    model.train(mode == "train")
    emb = getattr(model, "embedding", None)
    if emb is not None:
        try:
            emb.set_grad_mode(grad)
        except NotImplementedError:              # a mixed schema: the predicates read the attribute alone
            emb.grad_mode = grad
    s = {"ineligible_reason": _call(T.ineligible_reason, model),
         "mixed_ineligible_reason": _call(T.mixed_ineligible_reason, model),
         "record_gather_reason": _call(predict.record_gather_reason, model),
         "mixed_train_ineligible_reason": _per_batch(T.mixed_train_ineligible_reason, model),
         "mixed_step_ineligible_reason": _per_batch(T.mixed_step_ineligible_reason, model),
         "mixed_step_class": _call(T.mixed_step_class, model),
         "fused_step_class": _call(fused_step.fused_step_class, model)}
    for name in STEPS:
        cls = getattr(fused_step, name, None) or getattr(mixed_step, name)
        s[name + ".eligible"] = _call(cls.eligible, model)
        s[name + ".ineligible_reason"] = _per_batch(cls.ineligible_reason, model)
    return s


@pytest.mark.parametrize("case", sorted(cases()))
def test_every_predicate_answers_as_pinned(case):
    model = cases()[case]()
    rows = TABLE[case]
    for i, (grad, mode) in enumerate(STATES):
        got = snapshot(model, grad, mode)
        want = rows[i] if isinstance(rows[0], list) else rows
        assert sorted(got) == sorted(PREDICATES)
        for name, code in zip(PREDICATES, want):
            assert got[name] == ANSWERS[code] and type(got[name]) is type(ANSWERS[code]), (case, grad, mode, name)
        for name in STEPS:                        # the bool and the reason are one answer
            assert got[name + ".eligible"] is (got[name + ".ineligible_reason"] is None), (case, grad, mode, name)


def test_the_table_covers_the_matrix():
    assert sorted(TABLE) == sorted(cases())
    picked = {ANSWERS[r[PREDICATES.index("fused_step_class")]] for rows in TABLE.values()
              for r in (rows if isinstance(rows[0], list) else [rows])}
    assert picked == set(STEPS) | {None}          # every class is chosen somewhere, and somewhere none is


@pytest.mark.parametrize("kind", KINDS)
def test_row_samples_cap_at_its_edge(kind):
    import deepfm_amd.training as T
    from deepfm_amd import _lib
    rows = sum(f["vocab"] for f in _movielens())
    big = _lib.BWD_RECORD_MAX_ROW_SAMPLES // rows + 1
    assert (rows, big, _lib.BWD_RECORD_MAX_ROW_SAMPLES) == (3112, 43130, 134217728)
    over = ("3112 table rows x 43130 samples is over the row-owned scan's cap of 134217728 (tables this large belong to "
            "a row-sparse design)")
    model = _small(kind)
    cls = T.mixed_step_class(model)
    assert T.mixed_step_ineligible_reason(model, big) == over == cls.ineligible_reason(model, big)
    assert T.mixed_step_ineligible_reason(model, big - 1) is None and cls.ineligible_reason(model, big - 1) is None
    if kind == "deepfm":
        assert T.mixed_train_ineligible_reason(model, big) == over
        assert T.mixed_train_ineligible_reason(model, big - 1) is None


@pytest.mark.parametrize("name", UNIFORM_STEPS)
def test_uniform_steps_refuse_with_the_reason_before_any_device_work(name):
    from deepfm_amd.training import fused_step
    cls = getattr(fused_step, name)
    model = _bench("deepfm" if name == "FusedDeepFMStep" else "xdeepfm" if name == "FusedXDeepFMStep"
                   else "attention_deepfm").train()
    with pytest.raises(ValueError, match="'rowsparse' grad mode"):
        cls(model, None, 64)
    model.embedding.set_grad_mode("rowsparse")
    assert cls.ineligible_reason(model) is None and cls.eligible(model)
    with pytest.raises(ValueError, match="training mode"):
        cls(model.eval(), None, 64)


def test_rules_live_in_one_module_and_the_old_names_still_import():
    import deepfm_amd.training as T
    from deepfm_amd.training import eligibility, fused_step, mixed_step, predict
    for name in ("ineligible_reason", "mixed_ineligible_reason", "record_gather_reason", "mixed_param_bytes"):
        assert getattr(predict, name) is getattr(eligibility, name), name
    for name in ("mixed_train_ineligible_reason", "mixed_step_ineligible_reason", "backward_lds_bytes"):
        assert getattr(mixed_step, name) is getattr(eligibility, name), name
    for name in ("ineligible_reason", "mixed_ineligible_reason", "mixed_train_ineligible_reason",
                 "mixed_step_ineligible_reason"):
        assert getattr(T, name) is getattr(eligibility, name), name
    assert T.mixed_step_class is mixed_step.mixed_step_class
    assert [c.__name__ for c in fused_step.UNIFORM_STEPS + mixed_step.MIXED_STEPS] == STEPS
