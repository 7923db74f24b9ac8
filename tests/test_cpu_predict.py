"""CPU: FusedPredictor refuses ineligible models with the reason before any GPU work; the eval-mode and metrics
entry points are declared, exported and bound."""
import os
import re

import pytest

from tests.helpers import cfg_of, fields_of, load, schema_from_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dfm_linear_bn_eval", "dfm_predict_head", "dfm_metrics_workspace_bytes", "dfm_metrics_prepare",
               "dfm_metrics_finish"]


def _model(case, **dnn):
    from deepfm_amd.models import create_model
    from tests.test_gpu_models_step import _config
    g = load(case)
    c = cfg_of(g)
    cfg = _config(c)
    for k, v in dnn.items():
        setattr(cfg.dnn, k, v)
    return create_model(c["kind"], schema_from_fields(fields_of(g)), cfg)


@pytest.mark.parametrize("case,dnn,why", [
    ("model_deepfm_movielens", {}, "staged gather needs"),
    ("model_deepfm", {"activation": "gelu"}, "BatchNorm1d -> ReLU"),
    ("model_xdeepfm", {"use_batch_norm": False}, "BatchNorm1d -> ReLU"),
    ("model_deepfm", {"hidden_units": [32, 18]}, "multiples of 4"),
])
def test_ineligible_models_are_refused_with_the_reason(case, dnn, why):
    from deepfm_amd.training import FusedPredictor, ineligible_reason
    model = _model(case, **dnn)                    # on the CPU: the refusal comes before any device work
    assert why in ineligible_reason(model)
    with pytest.raises(ValueError, match=re.escape(why)):
        FusedPredictor(model, 64)


@pytest.mark.parametrize("case", ["model_deepfm", "model_xdeepfm", "model_attention_deepfm"])
def test_eligible_models_have_no_reason(case):
    from deepfm_amd.training import ineligible_reason
    assert ineligible_reason(_model(case)) is None


def test_released_tables_are_refused():
    from deepfm_amd.training import ineligible_reason
    model = _model("model_deepfm")
    name = next(n for n, s in model.schema.fields.items() if s.feature_type.name == "SPARSE")
    w = model.embedding.second_order_embeddings[name].weight
    w.data = w.data[:0]                             # what TableShard.release_foreign leaves behind
    assert "released" in ineligible_reason(model)


def test_new_entry_points_are_declared_exported_and_bound():
    from deepfm_amd import _lib
    import deepfm_amd.training as T
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepfm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dfm_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES["dfm_predict_head"][1]) == 11         # 10 operands + the launch destination
    for name in ("FusedPredictor", "compute_auc", "compute_logloss"):
        assert hasattr(T, name), name
    assert lib.dfm_metrics_workspace_bytes(1) > 0


def test_metrics_refuse_host_tensors():
    import torch
    from deepfm_amd.training import compute_auc
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_auc(torch.tensor([0.0, 1.0]), torch.tensor([0.2, 0.7]))
