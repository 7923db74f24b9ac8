"""The Trainer's row-sparse family on the host: exports, ``preflight_rowsparse`` and the path choice (no device)."""

import re
from pathlib import Path

import pytest
import torch

from deepfm_amd.data.synthetic import criteo_fields, movielens_fields, schema_from_fields

ROOT = Path(__file__).resolve().parent.parent
NEW_EXPORTS = ["dfm_tables_sqnorm_num_partials", "dfm_tables_sqnorm", "dfm_rows_sqnorm", "dfm_loss_accumulate_tables"]
FIELDS = criteo_fields(300, 16, n_sparse=4, n_dense=2)
KINDS = {"deepfm": "FusedDeepFMStep", "xdeepfm": "FusedXDeepFMStep", "attention_deepfm": "FusedAttentionDeepFMStep"}


def _model(kind="deepfm", fields=FIELDS, hidden=(64, 32), rowsparse=True):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    cfg.dnn.hidden_units, cfg.dnn.dropout = list(hidden), 0.0
    cfg.cin.layer_sizes, cfg.cin.split_half = [32, 24, 16], True
    cfg.attention.num_heads, cfg.attention.attention_dim, cfg.attention.num_layers = 4, 32, 1
    torch.manual_seed(0)
    model = create_model(kind, schema_from_fields(fields), cfg).train()
    if rowsparse:
        model.embedding.set_grad_mode("rowsparse")
    return model


def test_new_exports_are_in_header_library_and_signatures_and_the_abi_is_the_bindings():
    from deepfm_amd import _lib
    header = (ROOT / "include" / "deepfm_hip.h").read_text()
    lib = _lib.load()
    assert lib.dfm_abi_version() == _lib.ABI_VERSION and re.search(rf"#define DFM_ABI_VERSION {_lib.ABI_VERSION}\b", header)
    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\(" % name, header), name
        assert getattr(lib, name) is not None
    # every argument of the declaration has its ctypes type
    for name in NEW_EXPORTS:
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "dfm_loss_accumulate" in _lib.SIGNATURES and len(_lib.SIGNATURES["dfm_loss_accumulate"][1]) == 6
    assert lib.dfm_tables_sqnorm_num_partials(1) == 1 and lib.dfm_tables_sqnorm_num_partials(65) == 2
    assert lib.dfm_tables_sqnorm_num_partials(10 ** 9) == lib.dfm_tables_sqnorm_num_partials(10 ** 8)


@pytest.mark.parametrize("kind", list(KINDS))
def test_preflight_rowsparse_names_the_uniform_step_of_each_kind(kind):
    import deepfm_amd.training.fused_step as F
    from deepfm_amd.training.trainer import preflight_rowsparse, takes_rowsparse_path
    model = _model(kind)
    assert takes_rowsparse_path(model)
    assert preflight_rowsparse(model, 64, 64 * 7 + 37) is getattr(F, KINDS[kind])
    assert preflight_rowsparse(model, 64, 64) is getattr(F, KINDS[kind])


def test_preflight_rowsparse_says_why_it_refuses():
    from deepfm_amd.training.trainer import preflight_rowsparse
    with pytest.raises(ValueError, match=r"'rowsparse' grad mode \(set_grad_mode\('rowsparse'\)\).*no autograd fallback"):
        preflight_rowsparse(_model(rowsparse=False), 64, 1000)
    with pytest.raises(ValueError, match=r"field 'gender': embedding_dim 4 with fm_embed_dim 16.*no autograd fallback"):
        preflight_rowsparse(_model(fields=movielens_fields(50, 60), rowsparse=False), 64, 1000)
    with pytest.raises(ValueError, match=r"the DNN tower is not fusable.*no autograd fallback"):
        preflight_rowsparse(_model(hidden=(64, 24)), 64, 1000)
    with pytest.raises(ValueError, match="63 training rows are fewer than one batch of 64"):
        preflight_rowsparse(_model(), 64, 63)
    with pytest.raises(ValueError, match="^Expected more than 1 value per channel when training"):
        preflight_rowsparse(_model(), 64, 64 * 3 + 1)
    with pytest.raises(ValueError, match="must be positive"):
        preflight_rowsparse(_model(), 0, 10)


def test_the_trainers_path_is_a_function_of_the_model_alone():
    from deepfm_amd.training.trainer import preflight, takes_rowsparse_path
    uniform_dense = _model(rowsparse=False)
    assert not takes_rowsparse_path(uniform_dense)             # -> preflight, which points at set_grad_mode
    assert not takes_rowsparse_path(_model(fields=movielens_fields(50, 60), rowsparse=False))
    assert takes_rowsparse_path(_model())
    for model in (uniform_dense, _model()):                    # preflight's own refusal of uniform schemas is unchanged
        with pytest.raises(ValueError, match=r"uniform schema: use the row-sparse step \(set_grad_mode\('rowsparse'\)"):
            preflight(model, 64, 1000)


def test_trainer_refuses_before_any_device_work(tmp_path):
    """Both refusals are raised from the host checks: the models are on the CPU and nothing is moved."""
    import types

    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.training.trainer import Trainer
    cfg = ExperimentConfig(output_dir=str(tmp_path))
    cfg.training.batch_size = 64
    ds = types.SimpleNamespace(features={}, labels=[0.0] * 63)
    with pytest.raises(ValueError, match="63 training rows are fewer than one batch"):
        Trainer(_model(), None, cfg, ds, ds, ds)
    with pytest.raises(ValueError, match="uniform schema: use the row-sparse step"):
        Trainer(_model(rowsparse=False), None, cfg, ds, ds, ds)
    with pytest.raises(ValueError, match="steps_per_graph must be at least 1"):
        Trainer(_model(), None, cfg, ds, ds, ds, steps_per_graph=0)
    assert not any(p.is_cuda for p in _model().parameters())
