"""Train-step tail for the HIP path: row-wise Adam / AdamW / SGD over touched rows + data-parallel exchange;
dense-table optimizers and the fused step for mixed (MovieLens) schemas; eval-mode prediction and on-device AUC / log loss / HR@k / NDCG@k / grouped AUC / calibration / bootstrap intervals / permutation field importance;
score calibrators (Platt, isotonic) fitted on the device and applied inside the predictors' graph launch."""
from deepfm_amd.training.rowsparse import (RowSparseAdam, RowSparseAdamW, RowSparseOptimizer,  # noqa: F401
                                           RowSparseSGD, build_optimizer)
from deepfm_amd.training.schedule import ReduceLROnPlateau, build_scheduler  # noqa: F401
from deepfm_amd.training.metrics import (RankingEvaluator, bootstrap_device, bootstrap_dict,  # noqa: F401
                                       bootstrap_grouped_device, bootstrap_grouped_dict, bootstrap_units_device,
                                       calibration_device, calibration_dict, compare_bootstrap,
                                       compare_bootstrap_ranking, compute_auc, compute_bootstrap,
                                       compute_bootstrap_ranking, compute_calibration, compute_gauc, compute_logloss,
                                       compute_ranking_metrics, downsampling_correction, grouped_auc_device,
                                       grouped_auc_dict, grouped_metric_names, ranking_metrics_device,
                                       ranking_user_ranks_device)
from deepfm_amd.training.predict import (FusedPredictor, MixedSchemaPredictor, QuantizedMixedPredictor,  # noqa: F401
                                         QuantizedPredictor, ineligible_reason, mixed_ineligible_reason)
from deepfm_amd.training.calibrator import Calibrator  # noqa: F401
from deepfm_amd.training.importance import FieldImportance, ImportanceReport, RecordSet  # noqa: F401
from deepfm_amd.training.quantized import (QuantizedMixedTables, QuantizedTables,  # noqa: F401
                                           quantized_ineligible_reason, quantized_mixed_ineligible_reason)
from deepfm_amd.training.catalogue import CatalogueScorer  # noqa: F401
from deepfm_amd.training.dense_table import (DenseTableAdam, DenseTableAdamW, DenseTableOptimizer,  # noqa: F401
                                             DenseTableSGD, build_dense_optimizer)
from deepfm_amd.training.mixed_step import (FusedMixedAttentionDeepFMStep, FusedMixedDeepFMStep,  # noqa: F401
                                            FusedMixedXDeepFMStep, mixed_step_class, mixed_step_ineligible_reason,
                                            mixed_train_ineligible_reason)
from deepfm_amd.training.trainer import Trainer, preflight, preflight_rowsparse, run_training_loop  # noqa: F401
