"""AUC, log loss and the leave-one-out ranking metrics on the device (reference ``deepfm/training/metrics.py``).

``compute_auc`` / ``compute_logloss`` keep the reference's signatures and results: the exact Mann-Whitney AUC
(tied scores count 1/2; sklearn's ``roc_auc_score`` to fp64 rounding) and sklearn's ``log_loss`` of the scores
clipped to ``[1e-7, 1 - 1e-7]``.  The inputs are device tensors (numpy arrays are copied to the device); the work
is two HIP passes around one ``torch.sort`` of the negatives' scores (``csrc/predict.hip``), with integer
counts and fixed-order fp64 sums, so the results are deterministic.  Only the final scalars travel to the host.

``compute_ranking_metrics`` / ``RankingEvaluator`` give the reference's HR@k / NDCG@k (``Trainer.evaluate``'s
ranking keys, ``RankingEvaluator.evaluate``) from one segmented pass per user over the same device buffers
(``csrc/ranking.hip``): integer atomics and fixed-order fp64 sums again, no sort.

``compute_gauc`` gives the grouped AUC (no reference counterpart): the Mann-Whitney AUC per user, averaged over the
users with both classes, weighted by their samples (``gauc``) or not (``uauc``), from two HIP passes around one
``torch.sort`` of int64 keys (``csrc/grouped_auc.hip``); bitwise independent of the order of the samples.

``compute_calibration`` says whether the probabilities are right (no reference counterpart): mean prediction against
base rate (``copc``), normalised entropy, Brier score, the reliability table with its expected and maximum calibration
error, and the same per slice, from one streaming HIP pass into 64-bit integer sums (``csrc/calibration.hip``); bitwise
independent of the order of the samples.

``compute_bootstrap`` / ``compare_bootstrap`` put a standard error and a percentile interval beside the pooled AUC and
log loss, or beside the difference of two score vectors (no reference counterpart): a Poisson bootstrap over the samples
or over whole users, every replicate exact in 64-bit integers, from two HIP calls around two ``torch.sort`` of int64
keys (``csrc/bootstrap.hip``); with unit ids bitwise independent of the order of the samples.

``compute_bootstrap_ranking`` / ``compare_bootstrap_ranking`` do the same for the per-user metrics, HR@k / NDCG@k and
gauc / uauc, resampling whole users with the pooled bootstrap's weights: each metric is a mean of per-user integers that
the ranking and grouped-AUC passes form once, and a replicate is a quotient of two weighted column sums over the users
(``csrc/bootstrap_units.hip``), exact in 64-bit integers.  ``Evaluation``, ``enqueue_evaluation``, ``read_evaluations``
state once which of these families an evaluation enqueues and how their one host read becomes ``evaluate``'s dict.
"""

from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional

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


def _device_ids(user_ids, device) -> torch.Tensor:
    if isinstance(user_ids, torch.Tensor):
        _lib.require_device(user_ids, "user ids")
        u = user_ids
    else:
        a = np.asarray(user_ids)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"user ids must be integers, got {a.dtype}")
        u = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
    return u.reshape(-1).to(device=device, dtype=torch.int64).contiguous()


def _open(labels, scores, ids=None, what: str = "user", count: Optional[int] = None, read_count: bool = True):
    """How every ``*_device`` function starts: ``(y, s, ids, n, count)`` with the float32 device pair, the int64 device
    ids of the same length (None without ``ids``) and ``count`` the size of the id range, ``max(ids) + 1`` when it is
    None and ``read_count``: the one host read.  The limit on ``n`` is the caller's."""
    y, s = _device_pair(labels, scores)
    n = s.numel()
    if ids is None:
        return y, s, None, n, count
    ids = _device_ids(ids, s.device)
    if ids.numel() != n:
        raise ValueError(f"{what} ids ({ids.numel()}) and scores ({n}) differ in length")
    if count is None and read_count:
        count = int(ids.max()) + 1                      # the one host read
    return y, s, ids, n, count if count is None else int(count)


def _read_parts(parts) -> List[np.ndarray]:
    """The one host read of an evaluation: the device tensors ``parts`` (float64, or integers below 2^53) leave the
    device as one float64 vector; returns the flat host array of each part, in order."""
    flat = [p.reshape(-1).to(torch.float64) for p in parts]
    host = (torch.cat(flat) if len(flat) > 1 else flat[0]).cpu().numpy()
    return np.split(host, np.cumsum([p.numel() for p in flat])[:-1])


_BAD_LABELS = "labels other than 0 and 1"


def _raise_faults(*faults) -> None:
    """``ValueError`` for the first non-zero count among ``(count, what)``: ``"<count> <what>"``, and sklearn's message
    for NaN scores (``what`` None)."""
    for count, what in faults:
        if count:
            raise ValueError("Input contains NaN." if what is None else f"{int(count)} {what}")


def _grouping_faults(faults, what: str = "user") -> None:
    """The fault check of the passes that group the samples by an id (ranking, grouped AUC, grouped bootstrap)."""
    bad_id, nan, bad_label = faults
    _raise_faults((bad_id, f"{what} ids outside [0, num_{what}s)"), (nan, None), (bad_label, _BAD_LABELS))


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


# ---- leave-one-out ranking metrics (reference trainer.py:296-332, metrics.py:62-111) ----------------------------

MAX_KS = 8


def _check_ks(ks) -> List[int]:
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= MAX_KS:
        raise ValueError(f"{len(ks)} cut-offs: between 1 and {MAX_KS} values of k are supported")
    if min(ks) < 1:
        raise ValueError(f"ks {ks}: every k must be >= 1")
    return ks


def _ranking_open(user_ids, labels, scores, num_users):
    """How both ranking passes start: ``(lib, y, s, uid, n, num_users, workspace)`` behind ``_open`` and two checks."""
    y, s, uid, n, num_users = _open(labels, scores, user_ids, "user", num_users)
    if n >= 1 << 32:
        raise ValueError(f"{n} samples: the ranking pass takes fewer than 2^32")
    if num_users < 1:
        raise ValueError(f"num_users = {num_users}: the user ids must lie in [0, num_users)")
    lib = _lib.load()
    return lib, y, s, uid, n, num_users, torch.empty(lib.dfm_ranking_workspace_bytes(n, num_users), dtype=torch.uint8,
                                                     device=s.device)


def ranking_metrics_device(user_ids, labels, scores, ks, num_users: Optional[int] = None,
                           require_both_classes: bool = True) -> torch.Tensor:
    """Enqueue HR@k / NDCG@k of the samples grouped by ``user_ids`` (``csrc/ranking.hip``); returns a float64
    device tensor ``[users, HR@k..., NDCG@k..., bad ids, NaN scores, non-binary labels]`` without synchronising.

    Per user the rank is the 0-based position of its first positive in the stable descending order of its scores
    (``np.argsort(-s, kind="stable")``: tied scores keep dataset order, ``-0.0 == +0.0``), i.e.
    ``#{j : s_j > s*} + #{j : s_j == s*, j < p*}`` for the user's best positive score ``s*`` at its lowest index
    ``p*``.  The reference's ``np.argsort(-s)`` leaves the order of ties undefined; without ties both agree.
    ``require_both_classes`` keeps only users with both classes (the trainer's filter); otherwise every user with
    a sample counts and one without a positive is a miss (``RankingEvaluator.evaluate``).  ``num_users=None``
    takes ``max(user_ids) + 1``, which reads one value back to the host."""
    ks = _check_ks(ks)
    lib, y, s, uid, n, num_users, ws = _ranking_open(user_ids, labels, scores, num_users)
    out = torch.empty(1 + 2 * len(ks) + 3, dtype=torch.float64, device=s.device)
    h_ks = (C.c_int32 * len(ks))(*ks)
    _lib.check(lib.dfm_ranking_metrics(uid.data_ptr(), y.data_ptr(), s.data_ptr(), n, num_users, h_ks, len(ks),
                                       1 if require_both_classes else 0, ws.data_ptr(), out.data_ptr(),
                                       _lib.stream_handle()))
    return out


def ranking_dict(values, ks) -> Dict[str, float]:
    """The reference's dict from the host values of ``ranking_metrics_device``: ``HR@k``, ``NDCG@k`` per k in ``ks``
    order, ``{}`` when no user qualifies; ``ValueError`` for bad ids, NaN scores or non-binary labels."""
    ks = list(ks)
    m = len(ks)
    _grouping_faults(values[1 + 2 * m:4 + 2 * m])
    if not values[0]:
        return {}
    out: Dict[str, float] = {}
    for j, k in enumerate(ks):
        out[f"HR@{k}"] = float(values[1 + j])
        out[f"NDCG@{k}"] = float(values[1 + m + j])
    return out


def compute_ranking_metrics(user_ids, labels, scores, ks=(1, 5, 10, 20),
                            num_users: Optional[int] = None) -> Dict[str, float]:
    """Reference ``Trainer._compute_ranking_metrics`` (trainer.py:296-332): users with both classes only, keys
    ``HR@k`` / ``NDCG@k`` in ``ks`` order, ``{}`` when no user qualifies.  Inputs are device tensors or numpy
    arrays; ties are ordered as in ``ranking_metrics_device``."""
    return ranking_dict(ranking_metrics_device(user_ids, labels, scores, ks, num_users).cpu().tolist(), ks)


class RankingEvaluator:
    """Reference ``RankingEvaluator`` (metrics.py:62-111): HR@k / NDCG@k over per-user score and label arrays, every
    user counted (one without a positive is a miss, one with only positives a hit at rank 0).  Scores are
    compared as float32; ties are ordered as in ``ranking_metrics_device``."""

    def __init__(self, ks: Optional[List[int]] = None) -> None:
        self.ks = ks or [5, 10, 20]

    def evaluate(self, user_scores, user_labels) -> Dict[str, float]:
        pairs = list(zip(user_scores, user_labels))
        if not pairs:
            raise ValueError("no users")
        scores, labels, lengths = [], [], []
        for s, y in pairs:
            s = np.asarray(s, dtype=np.float32).reshape(-1)
            y = np.asarray(y, dtype=np.float32).reshape(-1)
            if s.size != y.size:
                raise ValueError(f"a user has {s.size} scores and {y.size} labels")
            if s.size == 0:           # an empty list is a miss, as one negative is
                s, y = np.zeros(1, np.float32), np.zeros(1, np.float32)
            scores.append(s); labels.append(y); lengths.append(s.size)
        uid = np.repeat(np.arange(len(pairs), dtype=np.int64), lengths)
        out = ranking_metrics_device(uid, np.concatenate(labels), np.concatenate(scores), self.ks,
                                     num_users=len(pairs), require_both_classes=False)
        return ranking_dict(out.cpu().tolist(), self.ks)


# ---- grouped AUC: the per-group Mann-Whitney AUC averaged over the groups (csrc/grouped_auc.hip) -----------------

def grouped_auc_sorted(group_ids, labels, scores, num_groups: Optional[int] = None):
    """The grouped AUC's first half, ``dfm_grouped_auc_prepare`` and the ``torch.sort`` of its keys: ``(sorted keys,
    workspace, n, num_groups)``.  ``dfm_grouped_auc_finish`` and ``dfm_grouped_auc_unit_columns`` only read the keys and
    the workspace's header (the fault counts), so one evaluation forms it once for both (their ``prepared``)."""
    y, s, gid, n, num_groups = _open(labels, scores, group_ids, "group", num_groups)
    if n >= 1 << 31:
        raise ValueError(f"{n} samples: the grouped AUC takes fewer than 2^31")
    if not 1 <= num_groups <= 1 << 30:
        raise ValueError(f"num_groups = {num_groups}: the group ids must lie in [0, num_groups), num_groups <= 2^30")
    lib = _lib.load()
    keys = torch.empty(n, dtype=torch.int64, device=s.device)
    ws = torch.empty(lib.dfm_grouped_auc_workspace_bytes(n, num_groups), dtype=torch.uint8, device=s.device)
    _lib.check(lib.dfm_grouped_auc_prepare(gid.data_ptr(), y.data_ptr(), s.data_ptr(), n, num_groups,
                                           keys.data_ptr(), ws.data_ptr(), _lib.stream_handle()))
    # per group the negatives ascending in front of the positives ascending; invalid samples (INT64_MAX) last
    return torch.sort(keys).values, ws, n, num_groups


def grouped_auc_device(group_ids, labels, scores, num_groups: Optional[int] = None, per_group: bool = False,
                       prepared=None):
    """Enqueue the grouped AUC of the samples grouped by ``group_ids`` (a user column, or the ids of any SPARSE
    field); returns a float64 device tensor ``[qualifying groups, gauc, uauc, samples in qualifying groups, bad ids,
    NaN scores, non-binary labels]`` without synchronising, and with ``per_group`` also the ``(num_groups,)`` float64
    device tensor of ``auc_g`` (NaN for a group that does not qualify).

    A group qualifies when it has both classes (the trainer's filter).  With ``P_g`` / ``N_g`` its positives and
    negatives, ``W_g`` / ``T_g`` its (positive, negative) pairs with ``s_pos > s_neg`` / ``s_pos == s_neg`` (float32
    order, ``-0.0 == +0.0``): ``auc_g = (2 W_g + T_g) / (2 P_g N_g)``, ``gauc = sum (P_g + N_g) auc_g / sum (P_g +
    N_g)`` and ``uauc = mean auc_g`` over the qualifying groups.  Two HIP passes around one ``torch.sort`` of int64 keys
    ``group << 33 | label << 32 | order bits``; the numerators are integers and the fp64 sums run over the group ids in
    a fixed tree, so the values do not depend on the order of the samples, bit for bit.  ``num_groups=None`` takes
    ``max(group_ids) + 1``, which reads one value back to the host.  ``prepared``: their ``grouped_auc_sorted``."""
    ordered, ws, n, num_groups = prepared or grouped_auc_sorted(group_ids, labels, scores, num_groups)
    dev = ordered.device
    out = torch.empty(7, dtype=torch.float64, device=dev)
    groups = torch.empty(num_groups, dtype=torch.float64, device=dev) if per_group else None
    _lib.check(_lib.load().dfm_grouped_auc_finish(ordered.data_ptr(), n, num_groups, ws.data_ptr(), _lib.ptr(groups),
                                                  out.data_ptr(), _lib.stream_handle()))
    return (out, groups) if per_group else out


def grouped_auc_dict(values) -> Dict[str, float]:
    """``{"gauc": ..., "uauc": ...}`` from the host values of ``grouped_auc_device``, ``{}`` when no group qualifies;
    ``ValueError`` for bad ids, NaN scores or non-binary labels."""
    _grouping_faults(values[4:7], "group")
    if not values[0]:
        return {}
    return {"gauc": float(values[1]), "uauc": float(values[2])}


def compute_gauc(group_ids, labels, scores, num_groups: Optional[int] = None) -> Dict[str, float]:
    """Grouped AUC of device tensors or numpy arrays: ``gauc`` (groups weighted by their samples) and ``uauc`` (the
    plain mean) over the groups with both classes, ``{}`` when there is none (``grouped_auc_device``)."""
    return grouped_auc_dict(grouped_auc_device(group_ids, labels, scores, num_groups).cpu().tolist())


# ---- calibration: are the probabilities right, overall, per bin and per slice (csrc/calibration.hip) --------------

CALIBRATION_VALUES = 12


def calibration_device(labels, scores, bins: int = 10, slice_ids=None, num_slices: Optional[int] = None):
    """Enqueue the calibration pass over (labels, scores) and, with ``slice_ids``, per slice; returns
    ``(out, bin_table, slice_table or None)`` as float64 device tensors without synchronising:

    ``out`` (12): ``[N, positives, mean prediction, Brier score, log loss, ece, mce, bad slice ids, NaN scores, scores
    outside [0, 1], non-binary labels, 0]``; ``bin_table`` (bins, 3): ``[count, positives, sum of predictions]`` of the
    bin ``min(bins - 1, int(p * bins))`` (float32 product); ``slice_table`` (num_slices, 4): ``[count, positives, sum
    of predictions, sum of log loss]``.  A sample with a bad slice id, a NaN or out-of-range score or a label other
    than 0 / 1 is counted and enters nothing else.  Every sum is a 64-bit integer sum of fixed-point terms
    (predictions and squared errors in units of 2^-32, log loss in units of 2^-27; ``include/deepfm_hip.h``), so the
    values do not depend on the order of the samples, bit for bit.  ``ece`` is ``sum_b |sum of predictions_b -
    positives_b| / N`` and ``mce`` the largest ``|mean prediction_b - positive fraction_b|``.  ``num_slices=None`` with
    slice ids takes ``max(slice_ids) + 1``, which reads one value back to the host."""
    bins = int(bins)
    if not 1 <= bins <= 1024:
        raise ValueError(f"bins = {bins}: between 1 and 1024 bins are supported")
    if slice_ids is None and num_slices is not None:
        raise ValueError("num_slices without slice_ids")
    y, s, sid, n, num_slices = _open(labels, scores, slice_ids, "slice", num_slices)
    if n >= 1 << 31:
        raise ValueError(f"{n} samples: the calibration pass takes fewer than 2^31")
    if sid is None:
        num_slices = 0
    elif not 1 <= num_slices <= 1 << 24:
        raise ValueError(f"num_slices = {num_slices}: the slice ids must lie in [0, num_slices), num_slices <= 2^24")
    lib = _lib.load()
    dev = s.device
    ws = torch.empty(lib.dfm_calibration_workspace_bytes(bins, num_slices), dtype=torch.uint8, device=dev)
    out = torch.empty(CALIBRATION_VALUES, dtype=torch.float64, device=dev)
    bin_table = torch.empty(bins, 3, dtype=torch.float64, device=dev)
    slice_table = torch.empty(num_slices, 4, dtype=torch.float64, device=dev) if sid is not None else None
    _lib.check(lib.dfm_calibration(y.data_ptr(), s.data_ptr(), _lib.ptr(sid), n, bins, num_slices, ws.data_ptr(),
                                   bin_table.data_ptr(), _lib.ptr(slice_table), out.data_ptr(), _lib.stream_handle()))
    return out, bin_table, slice_table


def _entropy(rate: float) -> float:
    return -(rate * math.log(rate) + (1.0 - rate) * math.log(1.0 - rate))


def calibration_dict(values) -> Dict[str, float]:
    """The floats of the 12 host values of ``calibration_device``: ``mean_pred``, ``base_rate``, ``brier``, ``ece``,
    ``mce``; ``copc`` (predicted over observed positives; omitted without a positive) and ``ne`` (log loss over the
    entropy of the base rate; omitted when a class is empty).  ``ValueError`` for bad slice ids, NaN scores,
    out-of-range scores or non-binary labels."""
    n, npos, mean_pred, brier, logloss, ece, mce, bad_id, nan, bad_range, bad_label = values[:11]
    _raise_faults((bad_id, "slice ids outside [0, num_slices)"), (nan, None), (bad_range, "scores outside [0, 1]"),
                  (bad_label, _BAD_LABELS))
    rate = float(npos) / float(n)
    out = {"mean_pred": float(mean_pred), "base_rate": rate, "brier": float(brier), "ece": float(ece),
           "mce": float(mce)}
    if npos:
        out["copc"] = float(mean_pred) * float(n) / float(npos)
    if 0 < npos < n:
        out["ne"] = float(logloss) / _entropy(rate)
    return out


def compute_calibration(labels, scores, bins: int = 10, slice_ids=None, num_slices: Optional[int] = None) -> Dict:
    """Calibration of device tensors or numpy arrays: the floats of ``calibration_dict``, ``"reliability"`` (numpy
    arrays ``count``, ``positives``, ``mean_pred``, ``frac_pos`` per bin, NaN in empty bins) and, with ``slice_ids``,
    ``"slices"`` (``count``, ``positives``, ``mean_pred``, ``base_rate``, ``logloss``, ``copc``, ``ne`` per slice, NaN
    where undefined)."""
    out, bin_table, slice_table = calibration_device(labels, scores, bins, slice_ids, num_slices)
    host = _read_parts([out, bin_table] + ([slice_table] if slice_table is not None else []))
    result: Dict = calibration_dict(host[0].tolist())
    b = host[1].reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        cnt = np.where(b[:, 0] > 0, b[:, 0], np.nan)
        result["reliability"] = {"count": b[:, 0].copy(), "positives": b[:, 1].copy(), "mean_pred": b[:, 2] / cnt,
                                 "frac_pos": b[:, 1] / cnt}
        if slice_table is not None:
            t = host[2].reshape(-1, 4)
            cnt = np.where(t[:, 0] > 0, t[:, 0], np.nan)
            rate = t[:, 1] / cnt
            logloss = t[:, 3] / cnt
            mixed = (rate > 0) & (rate < 1)
            r = np.where(mixed, rate, 0.5)
            entropy = np.where(mixed, -(r * np.log(r) + (1.0 - r) * np.log(1.0 - r)), np.nan)
            result["slices"] = {"count": t[:, 0].copy(), "positives": t[:, 1].copy(), "mean_pred": t[:, 2] / cnt,
                                "base_rate": rate, "logloss": logloss,
                                "copc": t[:, 2] / np.where(t[:, 1] > 0, t[:, 1], np.nan), "ne": logloss / entropy}
    return result


# ---- Poisson bootstrap of the pooled AUC and log loss (csrc/bootstrap.hip) ---------------------------------------

def _check_level(level: float) -> float:
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"level = {level} outside (0, 1)")
    return level


def _check_replicates(replicates: int) -> int:
    replicates = int(replicates)
    if not 1 <= replicates <= _lib.BOOTSTRAP_MAX_REPLICATES:
        raise ValueError(f"replicates = {replicates}: between 1 and {_lib.BOOTSTRAP_MAX_REPLICATES} are supported")
    return replicates


def bootstrap_device(labels, scores, replicates: int, seed: int = 0, unit_ids=None):
    """Enqueue ``replicates`` Poisson-bootstrap replicates of the pooled AUC and log loss; returns ``(counts, values,
    faults)`` as device tensors without synchronising: ``counts`` (replicates, 5) int64 ``[U, P, N, L, S]``, ``values``
    (replicates, 2) float64 ``[auc_r, logloss_r]`` (NaN where a replicate has one class / no sample) and ``faults`` (3)
    int64 ``[NaN scores, labels other than 0 / 1, unit ids outside [0, 2^40)]``.

    Replicate ``r`` weighs every sample by an integer ``w`` that is a function of ``(seed, r, unit)`` only, Poisson(1)
    truncated at 12 (``include/deepfm_hip.h`` has the hash); the unit of sample ``i`` is ``unit_ids[i]`` (a user: the
    samples of one user are resampled together) or ``i`` itself.  ``P, N, S`` are the weights of the positives, the
    negatives and all samples, ``U`` the weighted ``2 W + T`` of the Mann-Whitney count (float32 order, ``-0.0 ==
    +0.0``) and ``L`` the weighted sum of the per-sample log loss in units of 2^-27; ``auc_r = U / (2 P N)`` and
    ``logloss_r = L 2^-27 / S``.  Two HIP calls around two ``torch.sort`` of int64 keys; every sum is an integer sum, so
    two calls with one seed resample identically and, with ``unit_ids``, the values do not depend on the order of the
    samples, bit for bit.  A faulty sample is counted and enters nothing else."""
    y, s, uid, n, _ = _open(labels, scores, unit_ids, "unit", read_count=False)
    replicates = _check_replicates(replicates)
    if n > _lib.BOOTSTRAP_MAX_N:
        raise ValueError(f"{n} samples: the bootstrap takes at most 2^26")
    lib = _lib.load()
    dev = s.device
    keys = torch.empty(2, n, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.dfm_bootstrap_workspace_bytes(n, replicates), dtype=torch.uint8, device=dev)
    _lib.check(lib.dfm_bootstrap_prepare(y.data_ptr(), s.data_ptr(), _lib.ptr(uid), n, keys[0].data_ptr(),
                                         keys[1].data_ptr(), ws.data_ptr(), _lib.stream_handle()))
    # ascending scores, tied ones negatives first (row 0) / positives first (row 1); unused samples (INT64_MAX) last
    ordered = torch.sort(keys, dim=1).values
    counts = torch.empty(replicates, 5, dtype=torch.int64, device=dev)
    values = torch.empty(replicates, 2, dtype=torch.float64, device=dev)
    faults = torch.empty(3, dtype=torch.int64, device=dev)
    _lib.check(lib.dfm_bootstrap_replicates(ordered[0].data_ptr(), ordered[1].data_ptr(), _lib.ptr(uid), n, replicates,
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, ws.data_ptr(), counts.data_ptr(),
                                            values.data_ptr(), faults.data_ptr(), _lib.stream_handle()))
    return counts, values, faults


def _bootstrap_faults(faults) -> None:
    nan, bad_label, bad_unit = faults
    _raise_faults((nan, None), (bad_label, _BAD_LABELS), (bad_unit, "unit ids outside [0, 2^40)"))


def _spread(x: np.ndarray, level: float):
    """(se, lo, hi, replicates used) of one column of replicates: NaN replicates are dropped and counted out."""
    x = x[~np.isnan(x)]
    q = (1.0 - level) / 2.0
    nan = float("nan")
    se = float(np.std(x, ddof=1)) if x.size > 1 else nan
    lo, hi = (float(v) for v in np.quantile(x, [q, 1.0 - q])) if x.size else (nan, nan)
    return se, lo, hi, int(x.size)


def _columns(values, names) -> Dict[str, np.ndarray]:
    """``{m: its replicates}`` of the host values (replicates, len(names)) of a bootstrap, flat or not."""
    return dict(zip(names, np.asarray(values, np.float64).reshape(-1, len(names)).T))


def _spread_dict(columns: Dict[str, np.ndarray], level: float) -> Dict[str, float]:
    """``{m}_se``, ``{m}_lo``, ``{m}_hi``, ``{m}_replicates`` per metric ``m`` of ``columns``, in its order."""
    out: Dict[str, float] = {}
    for name, x in columns.items():
        se, lo, hi, used = _spread(x, level)
        out.update({f"{name}_se": se, f"{name}_lo": lo, f"{name}_hi": hi, f"{name}_replicates": used})
    return out


def delta_dict(names, signs, run_a, run_b, level: float = 0.95) -> Dict[str, float]:
    """Two runs ``(points, {m: replicates})`` under one resampling, per metric ``m`` of ``names``: the points ``m_a``,
    ``m_b`` (NaN where a run has none) and ``m_delta`` (b - a), the spread of the replicates' deltas ``m_delta_se``,
    ``m_delta_lo``, ``m_delta_hi`` and ``m_b_better``, the share of the non-NaN deltas with ``sign * delta > 0``
    (``signs``: +1 where higher is better, -1 for log loss)."""
    nan = float("nan")
    out: Dict[str, float] = {}
    for name, sign in zip(names, signs):
        a, b = run_a[0].get(name, nan), run_b[0].get(name, nan)
        delta = run_b[1][name] - run_a[1][name]
        se, lo, hi, used = _spread(delta, level)
        d = delta[~np.isnan(delta)]
        out.update({f"{name}_a": a, f"{name}_b": b, f"{name}_delta": b - a, f"{name}_delta_se": se,
                    f"{name}_delta_lo": lo, f"{name}_delta_hi": hi,
                    f"{name}_b_better": float(np.count_nonzero(sign * d > 0)) / used if used else nan})
    return out


def bootstrap_dict(values, faults, level: float = 0.95) -> Dict[str, float]:
    """The spread of the host values of ``bootstrap_device``: per metric ``m`` in (``auc``, ``logloss``) the standard
    error ``m_se`` (standard deviation of the replicates, ddof 1), the interval ``m_lo`` / ``m_hi`` (``np.nanquantile``
    at (1 - level) / 2 and 1 - (1 - level) / 2, linear interpolation) and ``m_replicates``, how many replicates were not
    NaN; ``ValueError`` for NaN scores, non-binary labels or bad unit ids."""
    level = _check_level(level)
    _bootstrap_faults(faults)
    return _spread_dict(_columns(values, ("auc", "logloss")), level)


# ---- Poisson bootstrap of the per-user metrics: HR@k, NDCG@k, gauc, uauc (csrc/bootstrap_units.hip) ---------------

GAIN_UNIT = 2.0 ** -30
_gain_tables: Dict = {}


def ranking_user_ranks_device(user_ids, labels, scores, num_users: Optional[int] = None,
                              require_both_classes: bool = True):
    """Enqueue the per-user ranks behind ``ranking_metrics_device`` (``dfm_ranking_user_ranks``); returns ``(rank,
    out)`` without synchronising: ``rank`` (num_users) int64, the user's rank, ``_lib.RANK_NOT_COUNTED`` (-1) for a user
    that does not count and ``_lib.RANK_MISS`` (-2) for one that counts without a positive (only without
    ``require_both_classes``); ``out`` (4) float64 ``[users counted, bad ids, NaN scores, non-binary labels]``."""
    lib, y, s, uid, n, num_users, ws = _ranking_open(user_ids, labels, scores, num_users)
    rank = torch.empty(num_users, dtype=torch.int64, device=s.device)
    out = torch.empty(4, dtype=torch.float64, device=s.device)
    _lib.check(lib.dfm_ranking_user_ranks(uid.data_ptr(), y.data_ptr(), s.data_ptr(), n, num_users,
                                          1 if require_both_classes else 0, ws.data_ptr(), rank.data_ptr(),
                                          out.data_ptr(), _lib.stream_handle()))
    return rank, out


def bootstrap_units_device(cols: torch.Tensor, replicates: int, seed: int = 0) -> torch.Tensor:
    """Enqueue ``sums[r][m] = sum_u w(seed, r, u) cols[m][u]`` (``dfm_bootstrap_units``) for ``cols`` (num_cols,
    num_units) int64 on the device, read as unsigned; returns the (replicates, num_cols) int64 device tensor of the sums
    mod 2^64 without synchronising.  ``w`` is ``bootstrap_device``'s weight of unit ``u`` under the same seed."""
    _lib.require_device(cols, "columns")
    if cols.dtype != torch.int64 or cols.dim() != 2:
        raise TypeError(f"columns must be a (num_cols, num_units) int64 tensor, got {tuple(cols.shape)} {cols.dtype}")
    if cols.stride(1) != 1 or (cols.shape[0] > 1 and cols.stride(0) != cols.shape[1]):
        cols = cols.contiguous()
    num_cols, num_units = cols.shape
    replicates = _check_replicates(replicates)
    if not 1 <= num_cols <= _lib.BOOTSTRAP_UNITS_MAX_COLS:
        raise ValueError(f"{num_cols} columns: between 1 and {_lib.BOOTSTRAP_UNITS_MAX_COLS} are supported")
    if not 1 <= num_units <= _lib.BOOTSTRAP_UNITS_MAX_UNITS:
        raise ValueError(f"{num_units} units: between 1 and 2^30 are supported")
    lib = _lib.load()
    ws = torch.empty(lib.dfm_bootstrap_units_workspace_bytes(num_units, num_cols, replicates), dtype=torch.uint8,
                     device=cols.device)
    sums = torch.empty(replicates, num_cols, dtype=torch.int64, device=cols.device)
    _lib.check(lib.dfm_bootstrap_units(cols.data_ptr(), num_units, num_cols, replicates,
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, ws.data_ptr(), sums.data_ptr(),
                                       _lib.stream_handle()))
    return sums


def _gain_table(ks, device) -> torch.Tensor:
    """``rint(2^30 / log2(i + 2))`` for ``i < max(ks)`` as an int64 device tensor: numpy in float64, cached per (ks,
    device)."""
    key = (tuple(ks), str(device))
    if key not in _gain_tables:
        table = np.rint(2.0 ** 30 / np.log2(np.arange(max(ks), dtype=np.float64) + 2.0)).astype(np.int64)
        _gain_tables[key] = torch.from_numpy(table).to(device)
    return _gain_tables[key]


def grouped_metric_names(ks, group_auc: bool) -> List[str]:
    """The columns of ``bootstrap_grouped_device``'s values: ``HR@k``..., ``NDCG@k``..., then ``gauc``, ``uauc``."""
    ks = list(ks)
    return [f"HR@{k}" for k in ks] + [f"NDCG@{k}" for k in ks] + (["gauc", "uauc"] if group_auc else [])


def bootstrap_grouped_device(user_ids, labels, scores, ks, replicates: int, seed: int = 0,
                             num_users: Optional[int] = None, group_auc: bool = False,
                             require_both_classes: bool = True, prepared=None):
    """Enqueue ``replicates`` Poisson-bootstrap replicates over whole users of HR@k / NDCG@k (``ks``; may be empty with
    ``group_auc``) and, with ``group_auc``, of gauc / uauc; returns ``(values, faults)`` as float64 device tensors
    without synchronising: ``values`` (replicates, 2 len(ks) [+ 2]) in the order of ``grouped_metric_names`` (NaN where
    a replicate weighs no counted user) and ``faults`` (3) ``[bad user ids, NaN scores, non-binary labels]``.

    Each metric is a mean of per-user integers, which the ranking and grouped-AUC passes form once
    (``dfm_ranking_user_ranks`` + ``dfm_bootstrap_rank_columns``, ``dfm_grouped_auc_unit_columns``: counted and hit
    flags, the gain ``1 / log2(rank + 2)`` and ``auc_g`` in units of 2^-30); replicate ``r`` weighs user ``u`` by
    ``bootstrap_device``'s ``w(seed, r, u)``, so with ``unit_ids=user_ids`` there one seed gives one resampled
    population for every metric.  ``HR@k_r = sum w hit / sum w counted``, ``NDCG@k_r = sum w gain 2^-30 / sum w
    counted``, ``uauc_r = sum w q 2^-30 / sum w qual``, ``gauc_r = sum w size q 2^-30 / sum w size`` over the counted /
    qualifying users: integer sums, so the values depend on the order of the samples only where a user's rank does
    (tied scores keep dataset order).  ``num_users=None`` takes ``max(user_ids) + 1``, which reads one value back to
    the host.  ``prepared``: ``grouped_auc_sorted`` of the same arguments, when the caller has formed it."""
    ks = _check_ks(ks) if len(list(ks)) else []
    if not ks and not group_auc:
        raise ValueError("nothing to resample: give ks, group_auc or both")
    y, s, uid, n, num_users = _open(labels, scores, user_ids, "user", num_users)
    if n > _lib.BOOTSTRAP_MAX_N:
        raise ValueError(f"{n} samples: the bootstrap takes at most 2^26")
    if not 1 <= num_users <= _lib.BOOTSTRAP_UNITS_MAX_UNITS:
        raise ValueError(f"num_users = {num_users}: the user ids must lie in [0, num_users), num_users <= 2^30")
    lib = _lib.load()
    dev = s.device
    m = len(ks)
    ranking_cols = 1 + 2 * m if m else 0
    cols = torch.empty(ranking_cols + (4 if group_auc else 0), num_users, dtype=torch.int64, device=dev)
    rank, counts = ranking_user_ranks_device(uid, y, s, num_users, require_both_classes)      # the fault counts too
    if m:
        gain = _gain_table(ks, dev)
        h_ks = (C.c_int32 * m)(*ks)
        _lib.check(lib.dfm_bootstrap_rank_columns(rank.data_ptr(), num_users, h_ks, m, gain.data_ptr(), gain.numel(),
                                                  cols.data_ptr(), _lib.stream_handle()))
    if group_auc:
        ordered, ws, _, _ = prepared or grouped_auc_sorted(uid, y, s, num_users)
        _lib.check(lib.dfm_grouped_auc_unit_columns(ordered.data_ptr(), n, num_users, ws.data_ptr(),
                                                    cols[ranking_cols:].data_ptr(), _lib.stream_handle()))
    sums = bootstrap_units_device(cols, replicates, seed).to(torch.float64)        # below 2^60; rounded once each
    parts = []
    if m:
        parts += [sums[:, 1:1 + m] / sums[:, 0:1], sums[:, 1 + m:1 + 2 * m] * GAIN_UNIT / sums[:, 0:1]]
    if group_auc:
        g = sums[:, ranking_cols:]
        parts += [(g[:, 3] * GAIN_UNIT / g[:, 2]).unsqueeze(1), (g[:, 1] * GAIN_UNIT / g[:, 0]).unsqueeze(1)]
    return torch.cat(parts, dim=1), counts[1:4]


def bootstrap_grouped_dict(values, faults, ks, group_auc: bool, level: float = 0.95) -> Dict[str, float]:
    """The spread of the host values of ``bootstrap_grouped_device``: ``{m}_se``, ``{m}_lo``, ``{m}_hi``,
    ``{m}_replicates`` (as ``bootstrap_dict``) per metric ``m`` of ``grouped_metric_names(ks, group_auc)``;
    ``ValueError`` for bad user ids, NaN scores or non-binary labels."""
    level = _check_level(level)
    _grouping_faults(faults)
    return _spread_dict(_columns(values, grouped_metric_names(ks, group_auc)), level)


# ---- one evaluation: which families to enqueue on a split's scores, and how to decode their one host read ----------

class Evaluation(NamedTuple):
    """What one evaluation computes beside the pooled AUC and log loss: HR@k / NDCG@k at ``ks`` (None: none), gauc /
    uauc, the calibration over ``bins`` bins (None: none), the pooled bootstrap of ``replicates`` (0: off) and ``seed``,
    the same replicates over whole users for the per-user metrics asked for (``grouped``), the intervals' ``level``."""
    ks: Optional[List[int]] = None
    group_auc: bool = False
    bins: Optional[int] = None
    replicates: int = 0
    seed: int = 0
    grouped: bool = False
    level: float = 0.95

    def point_names(self, users: bool = True) -> List[str]:
        """The point metrics' keys in the decoded dict's order (one without a qualifying user is missing there)."""
        ranking = [f"{kind}@{k}" for k in self.ks or [] for kind in ("HR", "NDCG")]
        return ["auc", "logloss"] + (ranking + (["gauc", "uauc"] if self.group_auc else []) if users else [])


def _pooled_points(values, pooled: str) -> Dict[str, float]:
    """``metrics_device``'s host values in ``evaluate``'s spelling (``pooled == "evaluate"``: ``auc`` is 0.0 for a
    single-class split and NaN scores are refused) or ``compute_bootstrap``'s (``"nan"``: ``auc`` is NaN then)."""
    auc, logloss, npos, nneg, nan = values
    if nan and pooled == "evaluate":
        raise ValueError("the model produced NaN scores")
    return {"auc": float(auc) if (npos and nneg) or pooled == "nan" else 0.0, "logloss": float(logloss)}


def _families(req: Evaluation, users: bool, pooled: Optional[str]):
    """The families that ``req`` asks for in the order of ``evaluate``'s keys, each ``(enqueue, decode, names)``:
    ``enqueue(d)`` gives its device parts from the inputs ``d``.  A point family has ``names`` None and ``decode(host
    values)`` gives its dict; a replicate family's parts are (values, faults), ``names`` the values' columns and
    ``decode(faults)`` its fault check.  Left out: the per-user families without ``users`` (as ``evaluate`` does for a
    schema without the user field), the pooled AUC and log loss and their bootstrap with ``pooled`` None."""
    ks = req.ks or []
    out = []
    if pooled:
        out.append((lambda d: [metrics_device(d.y, d.s)], lambda v: _pooled_points(v, pooled), None))
    if users and req.ks is not None:
        out.append((lambda d: [ranking_metrics_device(d.uid, d.y, d.s, ks, d.num_users)],
                    lambda v: ranking_dict(v, ks), None))
    if users and req.group_auc:
        out.append((lambda d: [grouped_auc_device(d.uid, d.y, d.s, d.num_users, prepared=d.prepared)],
                    grouped_auc_dict, None))
    if req.bins is not None:
        def calibration(d):
            cal, bin_table, slice_table = calibration_device(d.y, d.s, req.bins, d.sid, d.num_slices)
            d.tables = {"bins": bin_table, "slices": slice_table}
            return [cal]
        out.append((calibration, calibration_dict, None))
    if pooled and req.replicates:
        out.append((lambda d: bootstrap_device(d.y, d.s, req.replicates, req.seed, d.bid)[1:], _bootstrap_faults,
                    ("auc", "logloss")))
    if req.grouped:
        out.append((lambda d: bootstrap_grouped_device(d.uid, d.y, d.s, ks, req.replicates, req.seed, d.num_users,
                                                       req.group_auc, prepared=d.prepared),
                    _grouping_faults, grouped_metric_names(ks, req.group_auc)))
    return out


def decode_evaluation(req: Evaluation, host, users: bool = True, pooled: Optional[str] = "evaluate", summarise=True):
    """``evaluate``'s dict from an evaluation's host values ``host``, one flat array per device part; each family's
    refusal is raised for its first non-zero fault count.  Without ``summarise`` the pair ``(points, {m: replicates})``
    instead, the replicates not turned into their spread (what ``delta_dict`` takes)."""
    host, points, columns = iter(host), {}, {}
    for _, decode, names in _families(req, users, pooled):
        if names is None:
            points.update(decode(next(host)))
        else:
            values, faults = next(host), next(host)
            decode(faults)
            columns.update(_columns(values, names))
    return {**points, **_spread_dict(columns, _check_level(req.level))} if summarise else (points, columns)


def enqueue_evaluation(req: Evaluation, labels, scores, user_ids=None, num_users: Optional[int] = None, slice_ids=None,
                       num_slices: Optional[int] = None, unit_ids=None, pooled: Optional[str] = "evaluate"):
    """Enqueue every family that ``req`` asks for on the float32 device vectors (labels, scores) and the int64 device id
    columns (the per-user metrics' users, the calibration's slices, the pooled bootstrap's units) without synchronising.
    Returns ``(device parts, their decode_evaluation, the calibration's device tables {"bins", "slices"} or None)``."""
    users = user_ids is not None
    d = SimpleNamespace(y=labels, s=scores, uid=user_ids, num_users=num_users, sid=slice_ids, num_slices=num_slices,
                        bid=unit_ids, tables=None, prepared=None)
    if users and req.group_auc:                # gauc / uauc and their replicates start from the same sorted keys
        d.prepared = grouped_auc_sorted(user_ids, labels, scores, num_users)
    parts = [part for enqueue, _, _ in _families(req, users, pooled) for part in enqueue(d)]
    return parts, lambda host, summarise=True: decode_evaluation(req, host, users, pooled, summarise), d.tables


def read_evaluations(enqueued, summarise: bool = True) -> List:
    """The one host read of any number of ``enqueue_evaluation`` results (one ``torch.cat``, one ``.cpu()``): what the
    decoder of each gives, in order."""
    host = iter(_read_parts([part for parts, _, _ in enqueued for part in parts]))
    return [decode([next(host) for _ in parts], summarise) for parts, decode, _ in enqueued]


def compute_bootstrap(labels, scores, replicates: int = 200, seed: int = 0, unit_ids=None,
                      level: float = 0.95) -> Dict[str, float]:
    """Pooled ``auc`` and ``logloss`` of device tensors or numpy arrays (``metrics_device``: ``auc`` is NaN when a class
    is empty) with the standard errors and percentile intervals of ``bootstrap_dict`` from ``replicates`` Poisson
    replicates over the samples, or over whole units with ``unit_ids`` (``bootstrap_device``); one host read."""
    level = _check_level(level)
    y, s = _device_pair(labels, scores)
    req = Evaluation(replicates=_check_replicates(replicates), seed=seed, level=level)
    return read_evaluations([enqueue_evaluation(req, y, s, unit_ids=unit_ids, pooled="nan")])[0]


def compare_bootstrap(labels, scores_a, scores_b, replicates: int = 200, seed: int = 0, unit_ids=None,
                      level: float = 0.95) -> Dict[str, float]:
    """Two score vectors of the same samples under the same resampling (one seed: replicate ``r`` weighs every unit
    alike in both runs): ``delta_dict`` per metric ``m`` in (``auc``, ``logloss``), ``m_b_better`` the share of the
    non-NaN replicates in which b is better (a higher AUC, a lower log loss); one host read."""
    level = _check_level(level)
    y, sa = _device_pair(labels, scores_a)
    _, sb = _device_pair(y, scores_b)
    req = Evaluation(replicates=_check_replicates(replicates), seed=seed, level=level)
    runs = read_evaluations([enqueue_evaluation(req, y, s, unit_ids=unit_ids, pooled="nan") for s in (sa, sb)], False)
    return delta_dict(("auc", "logloss"), (1.0, -1.0), *runs, level)


def compute_bootstrap_ranking(user_ids, labels, scores, ks=(1, 5, 10, 20), replicates: int = 200, seed: int = 0,
                              num_users: Optional[int] = None, group_auc: bool = False,
                              level: float = 0.95) -> Dict[str, float]:
    """``HR@k`` / ``NDCG@k`` (``compute_ranking_metrics``) and with ``group_auc`` ``gauc`` / ``uauc``
    (``compute_gauc``) of device tensors or numpy arrays, with the standard errors and percentile intervals of
    ``bootstrap_grouped_dict`` from ``replicates`` Poisson replicates over whole users (``bootstrap_grouped_device``);
    one host read (one more for ``num_users=None``)."""
    level = _check_level(level)
    y, s, uid, _, num_users = _open(labels, scores, user_ids, "user", num_users)
    req = Evaluation([int(k) for k in ks] or None, group_auc, None, _check_replicates(replicates), seed, True, level)
    return read_evaluations([enqueue_evaluation(req, y, s, uid, num_users, pooled=None)])[0]


def compare_bootstrap_ranking(user_ids, labels, scores_a, scores_b, ks=(1, 5, 10, 20), replicates: int = 200,
                              seed: int = 0, num_users: Optional[int] = None, group_auc: bool = False,
                              level: float = 0.95) -> Dict[str, float]:
    """Two score vectors of the same samples on the per-user metrics, under one resampling of the users: ``delta_dict``
    per metric ``m`` of ``grouped_metric_names`` (a point is NaN when no user qualifies), ``m_b_better`` the share of
    the non-NaN replicates in which b is higher; one host read (one more for ``num_users=None``)."""
    level = _check_level(level)
    y, sa, uid, _, num_users = _open(labels, scores_a, user_ids, "user", num_users)
    _, sb = _device_pair(y, scores_b)
    req = Evaluation([int(k) for k in ks] or None, group_auc, None, _check_replicates(replicates), seed, True, level)
    runs = read_evaluations([enqueue_evaluation(req, y, s, uid, num_users, pooled=None) for s in (sa, sb)], False)
    names = grouped_metric_names(req.ks or [], req.group_auc)
    return delta_dict(names, [1.0] * len(names), *runs, level)


def downsampling_correction(scores: torch.Tensor, keep_rate: float) -> torch.Tensor:
    """The usual correction for a model trained on a fraction ``keep_rate`` of the negatives (and every positive):
    ``q = p / (p + (1 - p) / keep_rate)``, on the tensor's device and in its dtype.  A helper for the caller:
    ``evaluate`` does not apply it."""
    if not 0.0 < keep_rate <= 1.0:
        raise ValueError(f"keep_rate = {keep_rate} outside (0, 1]")
    return scores / (scores + (1.0 - scores) / keep_rate)
