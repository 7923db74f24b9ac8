"""Train-step tail for the HIP path: row-wise Adam / AdamW / SGD over touched rows + data-parallel exchange."""
from deepfm_amd.training.rowsparse import (RowSparseAdam, RowSparseAdamW, RowSparseOptimizer,  # noqa: F401
                                           RowSparseSGD, build_optimizer)
from deepfm_amd.training.schedule import ReduceLROnPlateau, build_scheduler  # noqa: F401
