"""Score calibrators fitted and applied on the device (``csrc/calibrator.hip``; ``include/deepfm_hip.h`` states the
formulas, the Platt state block and the isotonic knot table).

``evaluate(..., calibration_bins=...)`` says that the probabilities are off (``copc``, ``ne``, ``ece``); a ``Calibrator``
fits the map that repairs them, from the (label, logit) buffers an evaluation leaves on the device, and the predictors
apply it inside their one graph launch (``FusedPredictor(..., calibrator=cal)``):

    labels, logits = predictor.collect_logits(val_columns)
    cal = Calibrator("platt").fit(labels, logits)          # enqueued: no host synchronisation
    print(cal.report())                                     # the one host read

``"platt"`` fits ``q = sigmoid(a z + b)`` by a damped Newton iteration on fp64 sums (``fit_slope=False``: ``a = 1``, the
prior shift of ``downsampling_correction`` learnt from data; ``smooth=True``: Platt's targets); ``"isotonic"`` fits a
non-decreasing piecewise-linear map by pool-adjacent-violators over ``bins`` equal-width logit bins.  The parameter
buffer is allocated once and only ever written in place: a refit, or ``load_state_dict``, changes what predictors that
were captured with this calibrator compute at their next launch, as ``QuantizedTables.refresh()`` does.
"""

from __future__ import annotations

import warnings
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from deepfm_amd import _lib

KINDS = {"platt": _lib.CAL_PLATT, "isotonic": _lib.CAL_ISOTONIC}
STATUS = {_lib.CAL_RUNNING: "max_rounds", _lib.CAL_CONVERGED: "converged", _lib.CAL_SINGLE_CLASS: "single_class",
          _lib.CAL_BAD_INPUT: "bad_input"}
MAX_ROUNDS = 1024
Z_LIMIT = 64.0


def check_kind(kind) -> str:
    if kind not in KINDS:
        raise ValueError(f"calibrator kind {kind!r}: one of {sorted(KINDS)}")
    return kind


class Calibrator:
    """A Platt or isotonic calibrator of logits.  Every argument is checked here, before any device call."""

    def __init__(self, kind: str = "platt", *, fit_slope: bool = True, smooth: bool = False, max_rounds: int = 32,
                 gtol: float = 1e-9, bins: int = 1024, z_range: Tuple[float, float] = (-16.0, 16.0),
                 device="cuda") -> None:
        self.kind = check_kind(kind)
        bins, max_rounds, gtol = int(bins), int(max_rounds), float(gtol)
        if not 1 <= bins <= _lib.ISOTONIC_MAX_BINS:
            raise ValueError(f"bins = {bins}: between 1 and {_lib.ISOTONIC_MAX_BINS} bins are supported")
        lo, hi = (float(np.float32(v)) for v in z_range)
        if not (-Z_LIMIT <= lo < hi <= Z_LIMIT):
            raise ValueError(f"z_range = {tuple(z_range)}: needs -{Z_LIMIT:g} <= z_lo < z_hi <= {Z_LIMIT:g}")
        if not 1 <= max_rounds <= MAX_ROUNDS:
            raise ValueError(f"max_rounds = {max_rounds} outside [1, {MAX_ROUNDS}]")
        if not gtol >= 0.0:
            raise ValueError(f"gtol = {gtol}: a number >= 0")
        self.fit_slope, self.smooth, self.max_rounds, self.gtol = bool(fit_slope), bool(smooth), max_rounds, gtol
        self.bins, self.z_range = bins, (lo, hi)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        lib = _lib.load()
        # the parameters: a Platt state block at the identity (1, 0), or a knot table with no knot (the plain sigmoid)
        if self.kind == "platt":
            host = torch.zeros(_lib.PLATT_STATE_DOUBLES, dtype=torch.float64)
            host[0] = 1.0
            self.params = host.to(self.device)
            self._ws = None
        else:
            self.params = torch.zeros(_lib.ISOTONIC_KNOT_BYTES, dtype=torch.uint8, device=self.device)
            self._ws = torch.zeros(lib.dfm_isotonic_workspace_bytes(bins), dtype=torch.uint8, device=self.device)
        _lib.require_device(self.params, "calibrator")
        self._code = KINDS[self.kind]

    # ------------------------------------------------------------------ fit / apply
    def _vector(self, x, what: str) -> torch.Tensor:
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        elif not isinstance(x, torch.Tensor):
            raise TypeError(f"{what}: expected a device tensor or a numpy array, got {type(x).__name__}")
        _lib.require_device(x, what)
        x = x.reshape(-1)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        return x

    def fit(self, labels, logits) -> "Calibrator":
        """Enqueue the fit on (labels, logits): device tensors, or numpy arrays that are copied once.  No host
        synchronisation; ``report()`` reads the outcome."""
        y, z = self._vector(labels, "labels"), self._vector(logits, "logits")
        n = z.numel()
        if y.numel() != n:
            raise ValueError(f"labels ({y.numel()}) and logits ({n}) differ in length")
        if not 1 <= n < 1 << 31:
            raise ValueError(f"{n} samples: a fit takes between 1 and 2^31 - 1")
        lib, st = _lib.load(), _lib.stream_handle()
        if self.kind == "platt":
            nbytes = lib.dfm_platt_workspace_bytes(n)
            if self._ws is None or self._ws.numel() < nbytes:
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(lib.dfm_platt_fit(y.data_ptr(), z.data_ptr(), n, int(self.fit_slope), int(self.smooth),
                                         self.max_rounds, self.gtol, self._ws.data_ptr(), self.params.data_ptr(), st))
        else:
            _lib.check(lib.dfm_isotonic_fit(y.data_ptr(), z.data_ptr(), n, self.bins, self.z_range[0], self.z_range[1],
                                            self._ws.data_ptr(), self.params.data_ptr(), st))
        return self

    def apply_into(self, logits_ptr: int, n: int, probs_ptr: int, at=None) -> None:
        """The apply launch on raw pointers: enqueued on the current stream, or re-pointing the node ``at``."""
        _lib.check(_lib.load().dfm_calibrate_apply(self._code, self.params.data_ptr(), logits_ptr, n, probs_ptr,
                                                   at or _lib.stream_handle()))

    def apply(self, logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Calibrated probabilities of a float32 device tensor of logits, in its shape (``out``: a contiguous float32
        device tensor of as many elements that aliases nothing else)."""
        _lib.require_device(logits, "logits")
        if logits.dtype != torch.float32:
            raise TypeError("logits must be float32")
        z = logits if logits.is_contiguous() else logits.contiguous()
        if out is None:
            out = torch.empty(z.shape, dtype=torch.float32, device=z.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != z.numel() or \
                out.device != z.device:
            raise ValueError("out must be a contiguous float32 tensor of the logits' size on their device")
        if z.numel():
            self.apply_into(z.data_ptr(), z.numel(), out.data_ptr())
        return out

    # ------------------------------------------------------------------ the host read
    def bin_table(self) -> torch.Tensor:
        """Isotonic: the (bins, 3) int64 device table ``[count, positives, sum of llrint(z_c * 2^24)]`` of the last
        fit (a view of the fit's workspace)."""
        if self.kind != "isotonic":
            raise ValueError("the bin table belongs to the isotonic calibrator")
        return self._ws.view(torch.int64)[8:].view(self.bins, 3)

    def report(self) -> Dict:
        """The outcome of the last fit; the one host read.  ``ValueError`` for ``bad_input`` (with the fault counts),
        a warning for ``single_class`` and ``slope_unidentified``."""
        if self.kind == "platt":
            s = self.params.cpu().tolist()
            status = STATUS[int(s[6])]
            rounds = int(s[5])
            out = {"kind": "platt", "a": s[0], "b": s[1], "status": status, "rounds": rounds,
                   "slope_unidentified": bool(int(s[7]) & _lib.CAL_FLAG_SLOPE_UNIDENTIFIED),
                   "logloss_before": s[3] if rounds else None, "logloss_after": s[2] if rounds else None,
                   "max_gradient": s[4] if rounds else None, "positives": int(s[8]), "negatives": int(s[9]),
                   "nonfinite_logits": int(s[10]), "bad_labels": int(s[11])}
        else:
            host = self.params.cpu()
            hdr = host[:64].view(torch.int64).tolist()
            m = hdr[0]
            x = host[64 + 8 * _lib.ISOTONIC_MAX_BINS:64 + 16 * _lib.ISOTONIC_MAX_BINS].view(torch.float64)[:m]
            v = host[64 + 16 * _lib.ISOTONIC_MAX_BINS:].view(torch.float64)[:m]
            bad = hdr[2] or hdr[3]
            out = {"kind": "isotonic", "knots_x": x.numpy().copy(), "knots_v": v.numpy().copy(), "knots": m,
                   "blocks": hdr[6], "bins": hdr[1] or self.bins,
                   "status": "bad_input" if bad else ("single_class" if m and hdr[5] in (0, hdr[4]) else "converged"),
                   "samples": hdr[4], "positives": hdr[5], "nonfinite_logits": hdr[2], "bad_labels": hdr[3]}
        if out["status"] == "bad_input":
            raise ValueError(f"calibrator fit: {out['nonfinite_logits']} non-finite logits, {out['bad_labels']} labels "
                             "other than 0 and 1")
        if out["status"] == "single_class":
            warnings.warn("calibrator fit: the labels hold a single class" +
                          ("; the parameters stay (1, 0)" if self.kind == "platt" else "; the map is constant"))
        if out.get("slope_unidentified"):
            warnings.warn("calibrator fit: the logits do not identify a slope (all equal?); only the bias was fitted")
        return out

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> Dict:
        return {"kind": self.kind, "params": self.params.detach().cpu().clone(),
                "config": torch.tensor([float(self.fit_slope), float(self.smooth), float(self.max_rounds), self.gtol,
                                        float(self.bins), self.z_range[0], self.z_range[1]], dtype=torch.float64)}

    def load_state_dict(self, state: Dict) -> "Calibrator":
        """Copies the saved parameters into this calibrator's buffer, in place (live graphs follow)."""
        if state.get("kind") != self.kind:
            raise ValueError(f"a state of kind {state.get('kind')!r} for a {self.kind!r} calibrator")
        params = state["params"]
        if params.dtype != self.params.dtype or params.numel() != self.params.numel():
            raise ValueError("the saved parameters do not have this calibrator's layout")
        self.params.copy_(params.to(self.device))
        return self
