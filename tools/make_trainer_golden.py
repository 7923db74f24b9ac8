#!/usr/bin/env python3
"""The control flow of the REFERENCE's ``Trainer.train()`` on scripted epochs -> tests/golden/trainer_loop.json.

Needs a checkout of the reference (it is imported, not copied), as tools/make_ranking_golden.py does; ``dacite``,
which ``deepfm.config`` imports and nothing here needs, is replaced by a stand-in in ``sys.modules``.

For every script below a reference ``Trainer`` is built on CPU over a two-field DeepFM (so that its optimizer and its
``ReduceLROnPlateau`` are the real torch objects), then ``_train_epoch`` and ``evaluate`` are replaced on the
instance by scripted sequences and ``train()`` runs: its own loop decides the metric, steps the scheduler, saves
checkpoints, counts patience and stops.  Recorded per epoch: the learning rate ``_train_epoch`` saw and whether
``save_checkpoint`` was called for that epoch; at the end ``best_epoch`` / ``total_epochs`` as handed to
``_save_results`` and the metrics ``train()`` returned.  ``tests/test_cpu_trainer.py`` drives
``deepfm_amd.training.run_training_loop`` with the same scripts and compares everything exactly.

A script: ``training`` (the ``TrainingConfig`` fields that matter), ``val`` (the validation dict of epoch 1, 2, ...;
at least ``num_epochs`` of them) and ``test`` (the final dict).

usage: python tools/make_trainer_golden.py REFERENCE_CHECKOUT   (the directory holding the reference's deepfm/)
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _val(aucs, **extra):
    """Validation dicts with the given auc; logloss falls with the epoch; ``extra``: further keys, one list each."""
    out = []
    for i, a in enumerate(aucs):
        d = {"auc": a, "logloss": 0.7 - 0.01 * i}
        d.update({k: v[i] for k, v in extra.items()})
        out.append(d)
    return out


def scripts():
    t = dict(lr=1e-3, scheduler="reduce_on_plateau", metric="auc")
    plateau = [0.6, 0.7] + [0.65] * 18
    return [
        dict(name="improving_until_num_epochs", training=dict(t, num_epochs=5, early_stopping_patience=5),
             val=_val([0.5, 0.6, 0.7, 0.8, 0.9])),
        dict(name="plateau_two_halvings_then_stop", training=dict(t, num_epochs=20, early_stopping_patience=8),
             val=_val(plateau)),
        dict(name="exact_tie_is_no_improvement", training=dict(t, num_epochs=10, early_stopping_patience=2),
             val=_val([0.6] * 10)),
        dict(name="absent_metric_falls_back_to_auc",
             training=dict(t, metric="NDCG@10", num_epochs=6, early_stopping_patience=2),
             val=_val([0.5, 0.7, 0.6, 0.65, 0.9, 0.9], **{"HR@10": [0.9, 0.1, 0.2, 0.3, 0.4, 0.5]})),
        dict(name="present_metric_is_watched",
             training=dict(t, metric="HR@10", num_epochs=6, early_stopping_patience=2),
             val=_val([0.5, 0.7, 0.6, 0.65, 0.9, 0.9], **{"HR@10": [0.2, 0.1, 0.3, 0.3, 0.25, 0.5]})),
        dict(name="patience_one", training=dict(t, num_epochs=10, early_stopping_patience=1),
             val=_val([0.6, 0.5, 0.9, 0.9])),
        dict(name="scheduler_none", training=dict(t, scheduler="none", num_epochs=20, early_stopping_patience=8),
             val=_val(plateau)),
        dict(name="improvement_when_patience_would_run_out",
             training=dict(t, num_epochs=12, early_stopping_patience=3),
             val=_val([0.6, 0.5, 0.5, 0.7, 0.6, 0.6, 0.6, 0.9, 0.9, 0.9, 0.9, 0.9])),
        # better for the early stop (strict >), not for the scheduler (relative threshold 1e-4): the rate halves
        # while the patience counter never leaves 0
        dict(name="improvements_below_the_scheduler_threshold",
             training=dict(t, num_epochs=8, early_stopping_patience=2),
             val=_val([0.7 + 1e-6 * i for i in range(8)])),
        dict(name="single_epoch", training=dict(t, num_epochs=1, early_stopping_patience=5), val=_val([0.4])),
    ]


def _reference(ref):
    sys.path.insert(0, ref)
    sys.modules.setdefault("dacite", types.SimpleNamespace(from_dict=None))
    import deepfm.training.trainer as trainer_module
    from deepfm.config import ExperimentConfig, TrainingConfig
    from deepfm.data.dataset import TabularDataset
    from deepfm.data.schema import DatasetSchema, FeatureType, FieldSchema
    from deepfm.models.deepfm import DeepFM
    return trainer_module, ExperimentConfig, TrainingConfig, TabularDataset, DatasetSchema, FeatureType, FieldSchema, DeepFM


def run_script(ref, script, out_dir):
    trainer_module, ExperimentConfig, TrainingConfig, TabularDataset, DatasetSchema, FeatureType, FieldSchema, DeepFM = ref
    schema = DatasetSchema(fields={n: FieldSchema(n, FeatureType.SPARSE, vocabulary_size=4, embedding_dim=8)
                                   for n in ("user_id", "item_id")}, label_field="label")
    ds = TabularDataset({"user_id": np.ones(4, np.int64), "item_id": np.ones(4, np.int64)}, np.zeros(4, np.float32))
    config = ExperimentConfig(training=TrainingConfig(**script["training"]), output_dir=out_dir)
    trainer = trainer_module.Trainer(DeepFM(schema, config), schema, config, ds, ds, ds, device="cpu")
    epochs, saved, info = [], [], {}
    val = iter(script["val"])
    test = {"auc": 0.123, "logloss": 0.456}

    def train_epoch(epoch):
        epochs.append({"lr": trainer.optimizer.param_groups[0]["lr"], "saved": False})
        return 0.5 / epoch

    trainer._train_epoch = train_epoch
    trainer.evaluate = lambda dataset, split_name="eval": dict(next(val)) if split_name == "val" else dict(test)
    trainer._save_results = lambda v, t, best_epoch, total_epochs: info.update(
        best_epoch=best_epoch, total_epochs=total_epochs, val_metrics=v, test_metrics=t)
    keep = trainer_module.save_checkpoint
    trainer_module.save_checkpoint = lambda state, path: saved.append(
        (state["epoch"], state["best_metric"], sorted(state)))
    try:
        returned = trainer.train()
    finally:
        trainer_module.save_checkpoint = keep
    for e, _, keys in saved:
        epochs[e - 1]["saved"] = True
        assert keys == ["best_metric", "epoch", "model_state_dict", "optimizer_state_dict"]
    return dict(script, test=test, epochs=epochs, best_metric=saved[-1][1] if saved else None,
                best_epoch=info["best_epoch"], total_epochs=info["total_epochs"], returned=returned,
                final_lr=trainer.optimizer.param_groups[0]["lr"])


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__.rsplit("usage: ", 1)[1])
    ref = _reference(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        cases = [run_script(ref, s, tmp) for s in scripts()]
    for c in cases:
        print(c["name"], "epochs", c["total_epochs"], "best", c["best_epoch"], "lr", [e["lr"] for e in c["epochs"]],
              flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "trainer_loop.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
