"""``Trainer``: the reference's epoch loop (``deepfm/training/trainer.py:24-332``) on the fused steps.

Same constructor, same ``train()`` / ``evaluate()`` / ``_train_epoch()``, same ``best_model.pt`` and ``results.json``;
what runs underneath is, for a mixed schema, ``mixed_step_class(model)`` over a ``build_dense_optimizer`` optimizer
and, for a uniform SPARSE / DENSE schema in ``'rowsparse'`` grad mode, ``fused_step_class(model)`` over a
``build_optimizer`` row-sparse optimizer (``steps_per_graph`` steps per graph launch), fed by a
``DeviceEpochLoader``, with no host synchronisation inside an epoch:

    every row is trained on   the loader's whole batches through the main step, its trailing partial batch
                              (``loader.tail()``) through the step's tail step (``make_tail_step``): the reference's
                              ``DataLoader(shuffle=True)`` keeps that batch (trainer.py:202-207);
    the epoch's mean loss     BCE + ``get_l2_reg_loss()`` per batch, summed on the device (``step.track_loss()``,
                              ``dfm_loss_accumulate`` / ``dfm_loss_accumulate_tables``) and read once at the end of
                              the epoch (trainer.py:239-242);
    evaluation                ``MixedSchemaPredictor`` / ``FusedPredictor`` ``.evaluate_loader``: AUC, log loss,
                              HR@k / NDCG@k on the device.

There is no autograd fallback: a model no fused step of its family takes is refused at construction with the reason
(``preflight`` / ``preflight_rowsparse``, host only).  The control flow of ``train()`` (metric choice, one scheduler step per epoch, strict
improvement, patience, early stop, last-weights test evaluation) is ``run_training_loop``, a pure host function over
callables, so that it can be pinned to the reference without a device.
"""

from __future__ import annotations

import dataclasses
import logging
from datetime import datetime
from pathlib import Path
from typing import Callable, Dict, Optional

import numpy as np
import torch

from deepfm_amd import _lib
from deepfm_amd.data.device_epoch import tail_rows
from deepfm_amd.training import eligibility
from deepfm_amd.training.dense_table import build_dense_optimizer
from deepfm_amd.training.mixed_step import check_tail_rows, mixed_step_class, mixed_step_ineligible_reason
from deepfm_amd.training.schedule import build_scheduler
from deepfm_amd.utils.io import save_checkpoint, save_results


@dataclasses.dataclass
class LoopResult:
    best_metrics: Dict[str, float]
    best_epoch: int
    total_epochs: int


def run_training_loop(tc, train_epoch: Callable[[int], float], evaluate: Callable[[], Dict[str, float]],
                      save_best: Callable[[int, float], None], scheduler=None,
                      before_epoch: Optional[Callable[[int], None]] = None,
                      log: Optional[Callable[[str], None]] = None) -> LoopResult:
    """The flow of the reference's ``Trainer.train`` (trainer.py:97-159) over callables; host only.

    Per epoch e = 1 .. ``tc.num_epochs``: ``before_epoch(e)``, ``train_epoch(e)``, ``evaluate()`` on the validation
    split; the watched metric is ``val.get(tc.metric, val.get("auc", 0.0))``; ``scheduler.step(metric)`` once when
    there is a scheduler; a strictly greater metric is an improvement (``save_best(e, metric)``, patience reset),
    anything else counts against ``tc.early_stopping_patience`` and stops the loop when it is used up."""
    best_metric, best_epoch, patience_counter = -float("inf"), 0, 0
    best_metrics: Dict[str, float] = {}
    epoch = 0
    for epoch in range(1, tc.num_epochs + 1):
        if before_epoch is not None:
            before_epoch(epoch)
        train_loss = train_epoch(epoch)
        val_metrics = evaluate()
        current = val_metrics.get(tc.metric, val_metrics.get("auc", 0.0))
        if log is not None:
            log(f"Epoch {epoch}/{tc.num_epochs}  train_loss={train_loss:.4f}  val_auc={val_metrics.get('auc', 0):.4f}  "
                f"val_logloss={val_metrics.get('logloss', 0):.4f}")
        if scheduler is not None:
            scheduler.step(current)
        if current > best_metric:
            best_metric, best_epoch, patience_counter, best_metrics = current, epoch, 0, val_metrics
            save_best(epoch, best_metric)
            if log is not None:
                log(f"  -> New best {tc.metric}={current:.4f}, saved checkpoint")
        else:
            patience_counter += 1
            if patience_counter >= tc.early_stopping_patience:
                if log is not None:
                    log(f"Early stopping at epoch {epoch} (no improvement for {tc.early_stopping_patience} epochs)")
                break
    return LoopResult(best_metrics, best_epoch, epoch)


def preflight(model, batch_size: int, train_rows: int):
    """The fused step class that will train ``model`` on ``train_rows`` rows per epoch in batches of ``batch_size``,
    or ``ValueError`` with the reason: ``mixed_step_ineligible_reason`` (a batch-size cap that holds for the batch
    holds for the shorter trailing batch), fewer rows than one batch, and the one-row trailing batch that
    ``nn.BatchNorm1d`` refuses.  Host only; nothing touches the device."""
    if batch_size < 1 or train_rows < 1:
        raise ValueError("batch_size and the training rows must be positive")
    reason = mixed_step_ineligible_reason(model, batch_size)
    if reason is not None:
        raise ValueError(f"Trainer: no fused mixed-schema step takes this model: {reason} (there is no autograd "
                         "fallback)")
    if train_rows < batch_size:
        raise ValueError(f"Trainer: {train_rows} training rows are fewer than one batch of {batch_size}")
    tail = tail_rows(train_rows, batch_size)
    if tail:
        check_tail_rows(model, tail)
    return mixed_step_class(model)


def takes_rowsparse_path(model) -> bool:
    """Which family trains ``model``: True for a uniform SPARSE / DENSE schema whose embedding is in ``'rowsparse'``
    grad mode (row tables, ``preflight_rowsparse``), False for everything else (``preflight``: the mixed-schema
    steps, which refuse a uniform schema in ``'dense'`` mode by pointing at ``set_grad_mode('rowsparse')``)."""
    return eligibility.uniform_schema_reason(model) is None and model.embedding.grad_mode == "rowsparse"


def preflight_rowsparse(model, batch_size: int, train_rows: int):
    """``preflight`` for the uniform, row-sparse family: the fused step class (``fused_step.UNIFORM_STEPS``) that will
    train ``model``, or ``ValueError`` with the reason: a schema that is not uniform, an embedding not in
    ``'rowsparse'`` grad mode, the class's own ``ineligible_reason``, released tables, fewer rows than one batch, the
    one-row trailing batch.  Host only; nothing touches the device."""
    from deepfm_amd.training.fused_step import UNIFORM_STEPS
    if batch_size < 1 or train_rows < 1:
        raise ValueError("batch_size and the training rows must be positive")
    reason = eligibility.uniform_schema_reason(model)
    if reason is None and model.embedding.grad_mode != "rowsparse":
        reason = "the embedding must be in 'rowsparse' grad mode (set_grad_mode('rowsparse'))"
    cls = None
    if reason is None:
        kind = eligibility.model_kind(model, exact=False)
        cls = next((c for c in UNIFORM_STEPS if c.model_kind == kind), None)
        reason = (cls.ineligible_reason(model) if cls is not None else
                  eligibility.family_reason(model, "fused step", exact=False) or f"no fused step takes {type(model).__name__}")
    reason = reason or eligibility.released_table_reason(model)
    if reason is not None:
        raise ValueError(f"Trainer: no fused row-sparse step takes this model: {reason} (there is no autograd "
                         "fallback)")
    if train_rows < batch_size:
        raise ValueError(f"Trainer: {train_rows} training rows are fewer than one batch of {batch_size}")
    tail = tail_rows(train_rows, batch_size)
    if tail:
        check_tail_rows(model, tail)
    return cls


# calibration numbers cannot be the watched metric: lower is better (or, for copc, the target is 1), and
# ``run_training_loop`` and the scheduler maximise
UNWATCHABLE_METRICS = ("ne", "ece", "mce", "brier", "copc")


def check_calibration(metric: str, calibration_bins: int, slice_field: Optional[str], schema) -> None:
    """The Trainer's refusals around the calibration numbers; host only."""
    from deepfm_amd.data.schema import FeatureType
    if metric in UNWATCHABLE_METRICS:
        raise ValueError(f"Trainer: training.metric = {metric!r} cannot be watched: "
                         f"{'its target is 1' if metric == 'copc' else 'lower is better'}, and the training loop and "
                         "the scheduler maximise the watched metric")
    if not 0 <= int(calibration_bins) <= 1024:
        raise ValueError(f"Trainer: calibration_bins = {calibration_bins} outside [0, 1024] (0: off)")
    if slice_field is not None:
        if not calibration_bins:
            raise ValueError("Trainer: slice_field slices the calibration numbers: it needs calibration_bins")
        spec = schema.fields.get(slice_field)
        if spec is None or spec.feature_type is not FeatureType.SPARSE:
            raise ValueError(f"Trainer: slice_field {slice_field!r} is not a SPARSE field of the schema")


class Trainer:
    """Trains a CTR model with early stopping and ranking evaluation: the reference's ``Trainer`` (same arguments).

    A data set is a ``DeviceEpochLoader`` (used as it is; ``batch_size`` must be ``config.training.batch_size``; with
    a candidate source it draws fresh negatives at every ``set_epoch``), a ``PackedColumns``, or any object with
    ``.features`` (dict of numpy columns) and ``.labels`` (the reference's ``TabularDataset``), uploaded once
    (shuffle on for training, off for evaluation, seed ``config.seed``).  ``adapter.resample_train()`` is honoured
    for epochs > 1 when given: the slow drop-in path, a fresh upload per epoch.  Epoch e (1-based) is the loader's
    ``set_epoch(e - 1)``.

    ``steps_per_graph`` (the uniform, row-sparse family only; clipped to the whole batches of an epoch): that many
    consecutive steps per graph launch (``run_group``); the whole batches a group does not fill run one by one, then
    the trailing batch on the tail step.  The training loader's ring must hold a group: ``depth >= steps_per_graph +
    2`` (a loader built here does; a caller's that does not is refused).

    ``calibration_bins`` (0: off) adds the calibration floats of ``training/metrics.py:calibration_dict`` to every
    evaluation, per slice of the SPARSE field ``slice_field`` as well when one is named.

    ``bootstrap`` (replicates; 0: off) adds standard errors and 95 % intervals of ``auc`` and ``logloss``
    (``training/metrics.py:bootstrap_dict``) to the final test evaluation only, and so to ``test_metrics`` of
    ``results.json``; the per-epoch validation is unchanged.  ``bootstrap_grouped`` adds, from the same replicates, the
    standard errors and intervals of the test evaluation's per-user metrics (``HR@k`` / ``NDCG@k`` of
    ``training.ranking_ks``, ``gauc`` / ``uauc`` when ``training.metric`` names one:
    ``training/metrics.py:bootstrap_grouped_dict``); it needs ``bootstrap`` > 0, a SPARSE ``user_id`` field and one of
    those metrics.

    ``calibrator`` (``"platt"``, ``"isotonic"`` or None: off): after the last epoch ``train()`` fits a ``Calibrator``
    of that kind on the validation split's logits (``training/calibrator.py``), evaluates the test split a second
    time through a predictor that applies it, adds those metrics to the test metrics under the same keys prefixed
    ``calibrated_`` and saves ``calibrator.pt`` (the calibrator's ``state_dict``) beside ``best_model.pt``.

    ``importance`` (repeats; 0: off): after the final test evaluation ``train()`` runs the permutation field importance
    of every field (``training/importance.py``) on the test split with the last weights, uncalibrated, with the test
    evaluation's ranking and grouped-AUC keywords and seed ``config.seed``; logs the five most harmful fields and
    writes the report's ``to_dict()`` as ``"field_importance"`` into ``results.json`` (``self.importance_report``
    keeps it).  With 0 ``results.json`` has no such key."""

    calibration_bins, slice_field = 0, None      # off unless the constructor says otherwise
    calibrator_kind, calibrator = None, None
    bootstrap, bootstrap_grouped = 0, False
    importance, importance_report = 0, None

    def __init__(self, model, schema, config, train_ds, val_ds, test_ds, adapter: object = None,
                 device: str = "cuda", *, steps_per_graph: int = 4, calibration_bins: int = 0,
                 slice_field: Optional[str] = None, calibrator: Optional[str] = None, bootstrap: int = 0,
                 importance: int = 0, bootstrap_grouped: bool = False) -> None:
        from deepfm_amd.training.calibrator import check_kind
        from deepfm_amd.training.predict import FusedPredictor, MixedSchemaPredictor
        if calibrator is not None:
            check_kind(calibrator)                # a refusal before any device work
        if not 0 <= int(bootstrap) <= _lib.BOOTSTRAP_MAX_REPLICATES:
            raise ValueError(f"Trainer: bootstrap = {bootstrap} outside [0, {_lib.BOOTSTRAP_MAX_REPLICATES}] (0: off)")
        self.bootstrap = int(bootstrap)
        if bootstrap_grouped:
            from deepfm_amd.data.schema import FeatureType
            if not self.bootstrap:
                raise ValueError("Trainer: bootstrap_grouped needs bootstrap (replicates > 0)")
            spec, tc = schema.fields.get("user_id"), config.training
            if spec is None or spec.feature_type is not FeatureType.SPARSE:
                raise ValueError("Trainer: bootstrap_grouped resamples whole users: it needs a SPARSE user_id field")
            if not tc.ranking_ks and tc.metric not in ("gauc", "uauc"):
                raise ValueError("Trainer: bootstrap_grouped has no per-user metric to resample: it needs "
                                 "training.ranking_ks or training.metric in ('gauc', 'uauc')")
        self.bootstrap_grouped = bool(bootstrap_grouped)
        if isinstance(importance, bool) or int(importance) != importance or \
                not 0 <= int(importance) < _lib.PERMUTATION_MAX_REPEATS:
            raise ValueError(f"Trainer: importance = {importance!r}: repeats in [0, 2^24) are needed (0: off)")
        self.importance = int(importance)
        self.calibrator_kind = calibrator
        self.schema, self.config, self.adapter = schema, config, adapter
        self.device = torch.device(device)
        self.logger = logging.getLogger("deepfm_amd.trainer")
        tc = config.training
        self.model = model.train()
        rows = train_ds.rows if hasattr(train_ds, "rows") else len(train_ds.labels)
        self.rowsparse = takes_rowsparse_path(self.model)
        # refusals come before any device work
        check_calibration(tc.metric, calibration_bins, slice_field, schema)
        self.calibration_bins, self.slice_field = int(calibration_bins), slice_field
        if self.rowsparse:
            if steps_per_graph < 1:
                raise ValueError("steps_per_graph must be at least 1")
            dist = torch.distributed
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError("Trainer: the row-sparse family trains on one rank (data-parallel and field-sharded "
                                 "steps have no tail step and no tracked loss)")
            step_cls = preflight_rowsparse(self.model, tc.batch_size, rows)
            self.steps_per_graph = max(1, min(steps_per_graph, rows // tc.batch_size))
        else:
            step_cls = preflight(self.model, tc.batch_size, rows)
            self.steps_per_graph = 1
        self._predictor_cls = FusedPredictor if self.rowsparse else MixedSchemaPredictor
        self._train_depth = max(4, self.steps_per_graph + 2)
        self.model = model.to(self.device)
        self.train_ds = self._loader(train_ds, shuffle=True)
        self.val_ds = self._loader(val_ds, shuffle=False)
        self.test_ds = self._loader(test_ds, shuffle=False)
        if self.rowsparse:
            from deepfm_amd.training.rowsparse import build_optimizer
            self.optimizer = build_optimizer(self.model, config)
        else:
            self.optimizer = build_dense_optimizer(self.model, config)
        self.scheduler = build_scheduler(self.optimizer, config)
        self.step = step_cls(self.model, self.optimizer, tc.batch_size)
        self.step.track_loss()
        self.tail_step = self.step.make_tail_step(self.train_ds.tail_rows) if self.train_ds.tail_rows else None
        if self.steps_per_graph > 1:      # (the timed variant: the whole batches left over by the groups run on it)
            self.step.capture(timed_variant=True, steps_per_graph=self.steps_per_graph)
        else:
            self.step.capture()
        if self.tail_step is not None:
            self.tail_step.capture()
        self._predictors = {tc.batch_size: self._predictor_cls(self.model, tc.batch_size)}
        self.predictor = self._predictors[tc.batch_size]
        self.output_dir = Path(config.output_dir)
        self.output_dir.mkdir(parents=True, exist_ok=True)

    # ------------------------------------------------------------------ data
    def _loader(self, ds, shuffle: bool):
        from deepfm_amd.data.device_epoch import DeviceColumns, DeviceEpochLoader
        from deepfm_amd.data.packed import PackedColumns
        B = self.config.training.batch_size
        if isinstance(ds, DeviceEpochLoader):
            if ds.batch_size != B:
                raise ValueError(f"a loader of batch_size {ds.batch_size} with training.batch_size = {B}")
            if shuffle and self.steps_per_graph > 1 and ds.depth < self.steps_per_graph + 2:
                raise ValueError(f"a training loader of depth {ds.depth} with steps_per_graph = {self.steps_per_graph}: "
                                 f"its ring must hold a group (depth >= {self.steps_per_graph + 2})")
            return ds
        if not isinstance(ds, PackedColumns):
            ds = PackedColumns(self.schema, {k: np.asarray(v) for k, v in ds.features.items()}, np.asarray(ds.labels))
        # (an evaluation split shorter than one batch, e.g. the reference's own 20-row test splits at batch 32, is
        # one batch of its own size)
        return DeviceEpochLoader(DeviceColumns(ds, self.device), B if shuffle else min(B, len(ds)), shuffle=shuffle,
                                 seed=self.config.seed, depth=self._train_depth if shuffle else 4)

    def _predictor(self, batch_size: int):
        if batch_size not in self._predictors:
            self._predictors[batch_size] = self._predictor_cls(self.model, batch_size)
        return self._predictors[batch_size]

    # ------------------------------------------------------------------ the reference's methods
    def _train_epoch(self, epoch: int) -> float:
        """One epoch over every row of the training loader (whole batches, then the trailing partial batch);
        returns the mean over batches of BCE + L2 term, read from the device once."""
        loader, step = self.train_ds, self.step
        loader.set_epoch(epoch - 1)
        step.reset_loss()
        G = self.steps_per_graph
        if G == 1:
            for record in loader:
                step.run_from(record)
        else:
            # groups of G batches, one graph launch each; no row-plan hand-off between launches (the loader's ring
            # re-uses addresses, and a hand-off is keyed by address); the whole batches left over: one by one
            whole = loader.num_batches // G * G
            for first in range(0, whole, G):
                step.run_group([loader.record(first + k) for k in range(G)])
            for k in range(whole, loader.num_batches):
                step.run_from(loader.record(k), eager_gather=True)
        if loader.tail_rows:
            if self.tail_step is None or self.tail_step.B != loader.tail_rows:
                raise ValueError(f"the training loader's trailing batch has {loader.tail_rows} rows, the tail step "
                                 f"was built for {self.tail_step.B if self.tail_step else 0}")
            self.tail_step.run_from(loader.tail())
        loss = step.mean_loss()
        if self.model.embedding.strict_indices:
            self.model.embedding.raise_on_bad_index()
        return loss

    def evaluate(self, dataset, split_name: str = "eval") -> Dict[str, float]:
        """auc, logloss and HR@k / NDCG@k (``training.ranking_ks``) over every row of ``dataset``, the trailing
        batch included; also ``gauc`` / ``uauc`` (the AUC per user, ``training/metrics.py``) when ``training.metric``
        names one of them, so that early stopping, the checkpoint and the scheduler watch it; and with the Trainer's
        ``calibration_bins`` the calibration floats (``mean_pred``, ``base_rate``, ``brier``, ``ece``, ``mce``,
        ``copc``, ``ne``; per slice of ``slice_field`` in ``predictor.last_calibration``), which reach the log, the
        returned metrics and ``results.json``.  ``split_name == "test"`` is the final evaluation: with the Trainer's
        ``bootstrap`` it also returns the standard errors and intervals of ``auc`` and ``logloss``."""
        from deepfm_amd.data.device_epoch import DeviceEpochLoader
        loader = dataset if isinstance(dataset, DeviceEpochLoader) else self._loader(dataset, shuffle=False)
        kw = self._test_keywords() if split_name == "test" else self._evaluation_keywords()
        return self._predictor(loader.batch_size).evaluate_loader(loader, **kw)

    def _evaluation_keywords(self) -> Dict:
        tc = self.config.training
        kw = dict(ranking_ks=tc.ranking_ks, group_auc=tc.metric in ("gauc", "uauc"))
        if self.calibration_bins:
            kw.update(calibration_bins=self.calibration_bins, slice_field=self.slice_field)
        return kw

    def _test_keywords(self) -> Dict:
        """The keywords of the final test evaluation (``split_name == "test"``): an epoch's, and with ``bootstrap`` the
        replicates, resampled by user when the schema has a SPARSE ``user_id`` (an evaluation split holds 1 + N
        candidates per user)."""
        from deepfm_amd.data.schema import FeatureType
        kw = self._evaluation_keywords()
        if self.bootstrap:
            kw["bootstrap"] = self.bootstrap
            spec = self.schema.fields.get("user_id")
            if spec is not None and spec.feature_type is FeatureType.SPARSE:
                kw["bootstrap_by"] = "user_id"
            if self.bootstrap_grouped:
                kw["bootstrap_grouped"] = True
        return kw

    def _calibrated_test_metrics(self) -> Dict[str, float]:
        """Fits the calibrator on the validation split's logits, saves it and returns the test split's metrics through
        a predictor that applies it, keys prefixed ``calibrated_``."""
        from deepfm_amd.training.calibrator import Calibrator
        labels, logits = self._predictor(self.val_ds.batch_size).collect_logits(self.val_ds)
        self.calibrator = Calibrator(self.calibrator_kind, device=self.device).fit(labels, logits)
        report = self.calibrator.report()                      # raises for bad input, warns for a degenerate fit
        self.logger.info(f"  calibrator ({self.calibrator_kind}): status {report['status']}")
        torch.save(self.calibrator.state_dict(), self.output_dir / "calibrator.pt")
        predictor = self._predictor_cls(self.model, self.test_ds.batch_size, calibrator=self.calibrator)
        metrics = predictor.evaluate_loader(self.test_ds, **self._test_keywords())
        return {f"calibrated_{k}": v for k, v in metrics.items()}

    def train(self) -> Dict[str, float]:
        """Full training loop with early stopping; returns the best validation metrics."""
        tc = self.config.training

        def before_epoch(epoch: int) -> None:
            if self.adapter is not None and epoch > 1:
                self._resample(self.adapter.resample_train())

        def save_best(epoch: int, best_metric: float) -> None:
            save_checkpoint({"epoch": epoch, "model_state_dict": self.model.state_dict(),
                             "optimizer_state_dict": self.optimizer.state_dict(), "best_metric": best_metric},
                            self.output_dir / "best_model.pt")

        result = run_training_loop(tc, self._train_epoch, lambda: self.evaluate(self.val_ds, "val"), save_best,
                                   self.scheduler, before_epoch, self.logger.info)
        self.logger.info("--- Final evaluation on test set ---")
        test_metrics = self.evaluate(self.test_ds, "test")       # the last weights, as in the reference
        if self.calibrator_kind is not None:
            test_metrics = {**test_metrics, **self._calibrated_test_metrics()}
        for k, v in test_metrics.items():
            self.logger.info(f"  test_{k} = {v:.4f}")
        if self.importance:
            self.importance_report = self._field_importance()
        self._save_results(result.best_metrics, test_metrics, result.best_epoch, result.total_epochs)
        return result.best_metrics

    def _field_importance(self):
        """The permutation importance of every field on the test split (the class docstring); logs the top five."""
        kw = self._evaluation_keywords()
        report = self._predictor(self.test_ds.batch_size).field_importance(
            self.test_ds, repeats=self.importance, seed=self.config.seed, ranking_ks=kw["ranking_ks"],
            group_auc=kw["group_auc"])
        mean, logloss = report.mean(), report.metrics.index("logloss")
        self.logger.info(f"--- Field importance on test set ({self.importance} repeats): rise of logloss ---")
        for label in report.ranking("logloss")[:5]:
            self.logger.info(f"  {label}: {mean[report.groups.index(label), logloss]:+.4f}")
        return report

    def _resample(self, ds) -> None:
        loader = self._loader(ds, shuffle=True)
        if loader.rows != self.train_ds.rows:
            raise ValueError(f"resample_train() returned {loader.rows} rows, the steps were built for "
                             f"{self.train_ds.rows}")
        self.train_ds = loader

    def _save_results(self, val_metrics, test_metrics, best_epoch: int, total_epochs: int) -> None:
        results = {
            "run_id": self.output_dir.name,
            "timestamp": datetime.now().isoformat(timespec="seconds"),
            "config": dataclasses.asdict(self.config),
            "val_metrics": val_metrics,
            "test_metrics": test_metrics,
            "training_info": {"best_epoch": best_epoch, "total_epochs": total_epochs},
        }
        if self.importance_report is not None:
            results["field_importance"] = self.importance_report.to_dict()
        save_results(results, self.output_dir / "results.json")
        self.logger.info(f"Results saved to {self.output_dir / 'results.json'}")
