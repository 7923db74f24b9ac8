"""Host-side tests of ``deepfm_amd.training.Trainer`` (no GPU).

1. ``run_training_loop`` against the REFERENCE's ``Trainer.train()`` on scripted epochs
   (``tests/golden/trainer_loop.json``, written by ``tools/make_trainer_golden.py``): the learning rate every epoch
   trains at, which epochs save a checkpoint, ``best_epoch``, ``total_epochs``, the returned metrics: all exact;
2. ``tail_rows`` arithmetic, the one-row-tail refusal and its wording;
3. the pre-flight refusals carry the existing eligibility messages;
4. the library exports ``dfm_loss_accumulate`` and its ABI version is still 10.
"""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, cfg_of, fields_of, load, schema_from_fields
from tests.test_gpu_models_step import _config

with open(os.path.join(GOLDEN, "trainer_loop.json")) as _f:
    CASES = json.load(_f)["cases"]
REQUIRED = {"improving_until_num_epochs", "plateau_two_halvings_then_stop", "exact_tie_is_no_improvement",
            "absent_metric_falls_back_to_auc", "patience_one", "scheduler_none",
            "improvement_when_patience_would_run_out"}


def test_the_golden_holds_every_required_script():
    assert REQUIRED <= {c["name"] for c in CASES}
    plateau = next(c for c in CASES if c["name"] == "plateau_two_halvings_then_stop")
    assert plateau["final_lr"] == plateau["training"]["lr"] / 4 and plateau["total_epochs"] < plateau["training"]["num_epochs"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_loop_matches_the_reference(case):
    from deepfm_amd.config import ExperimentConfig, TrainingConfig
    from deepfm_amd.training import build_scheduler, run_training_loop
    cfg = ExperimentConfig(training=TrainingConfig(**case["training"]))
    opt = types.SimpleNamespace(lr=cfg.training.lr)
    sched = build_scheduler(opt, cfg)
    assert (sched is None) == (case["training"]["scheduler"] == "none")
    epochs, val = [], iter(case["val"])

    def train_epoch(epoch):
        assert epoch == len(epochs) + 1
        epochs.append({"lr": opt.lr, "saved": False})
        return 0.5 / epoch

    saved = []

    def save_best(epoch, best_metric):
        epochs[epoch - 1]["saved"] = True
        saved.append(best_metric)

    r = run_training_loop(cfg.training, train_epoch, lambda: dict(next(val)), save_best, sched)
    assert epochs == case["epochs"]
    assert (r.best_epoch, r.total_epochs) == (case["best_epoch"], case["total_epochs"])
    assert r.best_metrics == case["returned"]
    assert saved[-1] == case["best_metric"]
    assert opt.lr == case["final_lr"]


# ----------------------------------------------------------------------------- tail arithmetic and refusals
@pytest.mark.parametrize("rows,batch,want", [(450_000, 4096, 3536), (100, 32, 4), (250, 64, 58), (128, 64, 0),
                                            (64, 64, 0), (65, 64, 1), (5, 64, 5)])
def test_tail_rows(rows, batch, want):
    from deepfm_amd.data.device_epoch import tail_rows
    assert tail_rows(rows, batch) == want
    with pytest.raises(ValueError):
        tail_rows(rows, 0)


def test_loader_tail_rows_follow_the_rows(monkeypatch):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns, RecordLayout
    monkeypatch.setattr(DeviceEpochLoader, "_create_plan", lambda self: None)      # the plans need the device
    monkeypatch.setattr("deepfm_amd._lib.require_device", lambda t, what: None)
    schema = schema_from_fields([dict(name="a", type="sparse", vocab=9, dim=8, max_len=1, combiner="mean")])
    cols = DeviceColumns(PackedColumns(schema, {"a": np.arange(100) % 9}, np.zeros(100, np.float32)), "cpu")
    loader = DeviceEpochLoader(cols, 32, shuffle=True, seed=3)
    assert (len(loader), loader.tail_rows) == (3, 4)
    assert loader.tail_layout == RecordLayout.of(schema, 4)          # its own layout, not the 32-row one with padding
    even = DeviceEpochLoader(cols, 25, shuffle=False)
    assert (len(even), even.tail_rows, even.tail_layout) == (4, 0, None) and even.tail() is None


def _movielens_model(kind="deepfm", **kw):
    from deepfm_amd.models import create_model
    g = load("model_deepfm_movielens")
    fields = [dict(f, **kw) if f["type"] == "sequence" else f for f in fields_of(g)]
    torch.manual_seed(0)
    return create_model(kind, schema_from_fields(fields), _config(dict(cfg_of(g), kind=kind, hidden_units=[64, 32]))).train()


def test_one_row_tail_is_refused_with_batchnorms_words():
    from deepfm_amd.training import preflight
    from deepfm_amd.training.mixed_step import check_tail_rows
    model = _movielens_model()
    with pytest.raises(ValueError, match=r"^Expected more than 1 value per channel when training"):
        check_tail_rows(model, 1)
    with pytest.raises(ValueError, match=r"^Expected more than 1 value per channel when training"):
        preflight(model, 64, 129)
    check_tail_rows(model, 2)
    from deepfm_amd.training import FusedMixedDeepFMStep
    assert preflight(model, 64, 130) is FusedMixedDeepFMStep and preflight(model, 64, 128) is FusedMixedDeepFMStep
    with pytest.raises(ValueError, match="fewer than one batch"):
        preflight(model, 64, 63)


def test_preflight_carries_the_eligibility_messages():
    from deepfm_amd.data.synthetic import criteo_fields
    from deepfm_amd.models import create_model
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.training import mixed_step_ineligible_reason, preflight
    uniform = create_model("deepfm", schema_from_fields(criteo_fields(100, 16)), ExperimentConfig()).train()
    reason = mixed_step_ineligible_reason(uniform, 64)
    assert reason.startswith("uniform schema: use the row-sparse step")
    with pytest.raises(ValueError) as e:
        preflight(uniform, 64, 1000)
    assert reason in str(e.value) and "no autograd fallback" in str(e.value)
    maxbag = _movielens_model(combiner="max")
    reason = mixed_step_ineligible_reason(maxbag, 64)
    assert "pools with max" in reason
    with pytest.raises(ValueError) as e:
        preflight(maxbag, 64, 1000)
    assert reason in str(e.value)


def test_track_loss_refuses_before_any_device_work():
    """The refusal of a non-dense-table optimizer is a host check (the method is there for every fused step)."""
    from deepfm_amd.training.fused_step import _FusedTowerStep
    step = _FusedTowerStep.__new__(_FusedTowerStep)
    step.opt = object()
    with pytest.raises(ValueError, match="dense-table optimizer"):
        step.track_loss()


# ----------------------------------------------------------------------------- the library
def test_library_exports_the_loss_accumulator():
    from deepfm_amd import _lib
    lib = _lib.load()
    assert "dfm_loss_accumulate" in _lib.SIGNATURES and hasattr(lib, "dfm_loss_accumulate")
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "deepfm_hip.h")) as f:
        assert "int dfm_loss_accumulate(const float* d_loss, float l2, const float* d_p, int64_t n_l2, double* d_acc," in f.read()


def test_save_results_writes_the_reference_keys(tmp_path):
    from deepfm_amd.utils.io import save_results
    path = tmp_path / "sub" / "results.json"
    save_results({"run_id": "x", "val_metrics": {"auc": np.float64(0.5)}, "when": tmp_path}, path)
    with open(path) as f:
        got = json.load(f)
    assert got == {"run_id": "x", "val_metrics": {"auc": 0.5}, "when": str(tmp_path)}
