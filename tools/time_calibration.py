#!/usr/bin/env python3
"""Time of the calibration pass (``training/metrics.py:calibration_device``, csrc/calibration.hip), two groups:
  * ``compute_calibration`` on 1 M samples and 20 bins, without slices and with 10 K slices (device tensors in, the
    dict with its tables out on the host): wall clock of whole calls, and the device time of the pass's own launches
    (the clearing of the workspace, the pass, the finish) by device events over back-to-back calls, beside its byte
    floor (8 or 16 bytes per sample over ``--bandwidth``); against a host pass of ``np.bincount`` over the same arrays
    and against ``sklearn.calibration.calibration_curve`` + ``brier_score_loss``, both with the copy to the host;
  * ``evaluate_loader(..., ranking_ks=[1, 5, 10, 20])`` with and without ``calibration_bins=20`` on the MovieLens
    schema (DeepFM of configs/deepfm_movielens.yaml, B = 4096) over 943 users x 1000 candidates: wall clock of whole
    calls (each ends in its one host read), alternating the two.
Medians and ranges over ``--reps`` repetitions; one JSON line per case.
usage: python tools/time_calibration.py [--reps 15] [--bandwidth 6.3e12]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.time_predict_mixed import B, C, U, build, split  # noqa: E402

BINS = 20


def stats(xs, scale=1e3, digits=3):
    xs = np.asarray(xs) * scale
    return dict(median=round(float(np.median(xs)), digits), min=round(float(xs.min()), digits),
                max=round(float(xs.max()), digits))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def host_bincount(d_y, d_p, d_sid, slices):
    """The same numbers on the host: copy, one ``np.bincount`` per column."""
    y, p = d_y.cpu().numpy(), d_p.cpu().numpy()
    b = np.minimum(BINS - 1, (p * np.float32(BINS)).astype(np.int64))
    p64, y64 = p.astype(np.float64), y.astype(np.float64)
    pc = np.clip(p64, 1e-7, 1 - 1e-7)
    ll = -(y64 * np.log(pc) + (1 - y64) * np.log(1 - pc))
    cnt = np.bincount(b, minlength=BINS)
    pos = np.bincount(b, weights=y64, minlength=BINS)
    sp = np.bincount(b, weights=p64, minlength=BINS)
    gap = np.abs(sp - pos)
    out = dict(mean_pred=float(p64.mean()), brier=float(np.mean((p64 - y64) ** 2)), logloss=float(ll.mean()),
               ece=float(gap.sum() / y.size), mce=float(np.max(gap[cnt > 0] / cnt[cnt > 0])))
    if d_sid is not None:
        sid = d_sid.cpu().numpy()
        out["slices"] = [np.bincount(sid, weights=w, minlength=slices) for w in (None, y64, p64, ll)]
    return out


def host_sklearn(d_y, d_p):
    from sklearn.calibration import calibration_curve
    from sklearn.metrics import brier_score_loss
    y, p = d_y.cpu().numpy(), d_p.cpu().numpy().astype(np.float64)
    frac_pos, mean_pred = calibration_curve(y, p, n_bins=BINS, strategy="uniform")
    return dict(brier=float(brier_score_loss(y, p)), mce=float(np.max(np.abs(frac_pos - mean_pred))))


def pass_case(reps, slices, bandwidth):
    from deepfm_amd.training import calibration_device, compute_calibration
    n = 1_000_000
    rng = np.random.default_rng(2)
    p = rng.beta(1.2, 8.0, n).astype(np.float32)
    y = (rng.random(n) < 0.7 * p).astype(np.float32)                  # over-predicting by construction
    sid = rng.integers(0, slices, n) if slices else None
    d_y, d_p = torch.from_numpy(y).cuda(), torch.from_numpy(p).cuda()
    d_sid = torch.from_numpy(sid).cuda() if slices else None
    call = lambda: compute_calibration(d_y, d_p, BINS, d_sid, slices or None)  # noqa: E731
    for _ in range(3):
        got = call()
    device = [wall(call)[0] for _ in range(reps)]
    calls, events = 20, []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            calibration_device(d_y, d_p, BINS, d_sid, slices or None)
        b.record()
        b.synchronize()
        events.append(a.elapsed_time(b) / calls)                      # ms
    host_bincount(d_y, d_p, d_sid, slices)
    bincount, ref = [], None
    for _ in range(reps):
        t, ref = wall(lambda: host_bincount(d_y, d_p, d_sid, slices))
        bincount.append(t)
    host_sklearn(d_y, d_p)
    sk, ref_sk = [], None
    for _ in range(reps):
        t, ref_sk = wall(lambda: host_sklearn(d_y, d_p))
        sk.append(t)
    bytes_read = n * (16 if slices else 8)
    print(json.dumps(dict(case="compute_calibration", samples=n, bins=BINS, slices=slices, reps=reps,
                          device_ms=stats(device), pass_device_ms=stats(events, scale=1.0, digits=4),
                          bytes_read=bytes_read, byte_floor_ms=round(bytes_read / bandwidth * 1e3, 4),
                          host_bincount_ms=stats(bincount), host_sklearn_ms=stats(sk),
                          brier=got["brier"], brier_host=ref["brier"], brier_sklearn=ref_sk["brier"],
                          ece=got["ece"], ece_host=ref["ece"], mce=got["mce"], mce_host=ref["mce"],
                          mce_sklearn=ref_sk["mce"], ne=got["ne"], copc=got["copc"])), flush=True)


def evaluation_case(reps):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import MixedSchemaPredictor
    rng = np.random.default_rng(0)
    model = build("deepfm")
    feats, labels = split(rng)
    loader = DeviceEpochLoader(DeviceColumns(PackedColumns(model.schema, feats, labels), "cuda"), B, shuffle=False)
    pred = MixedSchemaPredictor(model, B)
    ks = [1, 5, 10, 20]
    for bins in (None, BINS, None, BINS):                         # warm-up of both forms
        m = pred.evaluate_loader(loader, ranking_ks=ks, calibration_bins=bins)
    plain, with_bins, sliced = [], [], []
    for _ in range(reps):                                         # alternating: the same neighbours for all
        plain.append(wall(lambda: pred.evaluate_loader(loader, ranking_ks=ks))[0])
        with_bins.append(wall(lambda: pred.evaluate_loader(loader, ranking_ks=ks, calibration_bins=BINS))[0])
        sliced.append(wall(lambda: pred.evaluate_loader(loader, ranking_ks=ks, calibration_bins=BINS,
                                                        slice_field="movie_id"))[0])
    print(json.dumps(dict(case="evaluate_loader", split=f"{U}x{C}", B=B, bins=BINS, reps=reps,
                          without_ms=stats(plain), with_bins_ms=stats(with_bins), with_slices_ms=stats(sliced),
                          difference_of_medians_ms=round(float(np.median(with_bins) - np.median(plain)) * 1e3, 3),
                          ece=m["ece"], mce=m["mce"], ne=m["ne"], copc=m["copc"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--bandwidth", type=float, default=6.3e12, help="achievable HBM bytes per second")
    ap.add_argument("--only", choices=["evaluate_loader", "compute_calibration"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_calibration.py measures on the device: no GPU found")
    if args.only != "evaluate_loader":
        pass_case(args.reps, 0, args.bandwidth)
        pass_case(args.reps, 10_000, args.bandwidth)
    if args.only != "compute_calibration":
        evaluation_case(args.reps)


if __name__ == "__main__":
    main()
