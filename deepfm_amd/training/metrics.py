"""AUC and log loss on the device (reference ``deepfm/training/metrics.py:9-18``).

``compute_auc`` / ``compute_logloss`` keep the reference's signatures and results: the exact Mann-Whitney AUC
(tied scores count 1/2; sklearn's ``roc_auc_score`` to fp64 rounding) and sklearn's ``log_loss`` of the scores
clipped to ``[1e-7, 1 - 1e-7]``.  The inputs are device tensors (numpy arrays are copied to the device); the work
is two HIP passes around one ``torch.sort`` of the negatives' scores (``csrc/predict.hip``), with integer
counts and fixed-order fp64 sums, so the results are deterministic.  Only the final scalars travel to the host.
"""

from __future__ import annotations

import numpy as np
import torch

from deepfm_amd import _lib


def _device_pair(labels, scores, device=None):
    def as_dev(x):
        if isinstance(x, np.ndarray):
            dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
            x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        elif not isinstance(x, torch.Tensor):
            raise TypeError(f"expected a device tensor or a numpy array, got {type(x).__name__}")
        _lib.require_device(x, "metrics input")
        return x.reshape(-1).to(torch.float32).contiguous()
    s = as_dev(scores)
    y = as_dev(labels) if isinstance(labels, torch.Tensor) else as_dev(np.asarray(labels))
    if y.numel() != s.numel():
        raise ValueError(f"labels ({y.numel()}) and scores ({s.numel()}) differ in length")
    if s.numel() == 0:
        raise ValueError("no samples")
    if y.device != s.device:
        y = y.to(s.device)
    return y, s


def metrics_device(labels: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
    """Enqueue both metrics of (labels, scores) float32 device vectors; returns a float64 device tensor
    ``[auc (NaN if a class is empty), logloss, npos, nneg, NaN scores]`` without synchronising."""
    lib = _lib.load()
    n = scores.numel()
    dev = scores.device
    keys = torch.empty(n, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.dfm_metrics_workspace_bytes(n), dtype=torch.uint8, device=dev)
    st = _lib.stream_handle()
    _lib.check(lib.dfm_metrics_prepare(labels.data_ptr(), scores.data_ptr(), n, keys.data_ptr(), ws.data_ptr(), st))
    # negatives' scores ascending in front, the positives' +inf keys behind them
    ordered = torch.sort(keys).values
    out = torch.empty(5, dtype=torch.float64, device=dev)
    _lib.check(lib.dfm_metrics_finish(labels.data_ptr(), scores.data_ptr(), n, ordered.data_ptr(), ws.data_ptr(),
                                      out.data_ptr(), _lib.stream_handle()))
    return out


def _host(out: torch.Tensor):
    auc, logloss, npos, nneg, nan = out.cpu().tolist()
    if nan:
        raise ValueError("Input contains NaN.")
    return auc, logloss, int(npos), int(nneg)


def compute_auc(labels, scores) -> float:
    """Area under the ROC curve; ``ValueError`` for a single-class label set (as sklearn)."""
    auc, _, npos, nneg = _host(metrics_device(*_device_pair(labels, scores)))
    if npos == 0 or nneg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return float(auc)


def compute_logloss(labels, scores) -> float:
    """Binary cross-entropy of the scores clipped to [1e-7, 1 - 1e-7] (mean, natural log).  A single-class label
    set raises ``ValueError``, as sklearn's ``log_loss`` does without ``labels``."""
    _, logloss, npos, nneg = _host(metrics_device(*_device_pair(labels, scores)))
    if npos == 0 or nneg == 0:
        raise ValueError("y_true contains only one label. Please provide the list of all expected class labels "
                         "explicitly through the labels argument.")
    return float(logloss)
