#!/usr/bin/env python3
"""Time of the grouped AUC (``training/metrics.py:grouped_auc_device``, csrc/grouped_auc.hip), two cases:
  * ``evaluate_loader(..., ranking_ks=[1, 5, 10, 20], group_auc=True)`` against the same call without the flag, on
    the MovieLens schema (DeepFM of configs/deepfm_movielens.yaml, B = 4096) over 943 users x 1000 candidates: wall
    clock of whole calls (each ends in its one host read), alternating the two, and the device time of the metric's
    own launches (prepare, ``torch.sort``, finish) by device events over back-to-back calls;
  * ``compute_gauc`` on 1 M samples in 10 K groups (device tensors in, dict out on the host) against a host loop of
    ``sklearn.metrics.roc_auc_score`` per group, the copy of ids, labels and scores to the host included.
Medians and ranges over ``--reps`` repetitions; one JSON line per case.
usage: python tools/time_gauc.py [--reps 15] [--host-reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.time_predict_mixed import B, C, U, build, split  # noqa: E402


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


def evaluation_case(reps):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import MixedSchemaPredictor, grouped_auc_device
    rng = np.random.default_rng(0)
    model = build("deepfm")
    feats, labels = split(rng)
    loader = DeviceEpochLoader(DeviceColumns(PackedColumns(model.schema, feats, labels), "cuda"), B, shuffle=False)
    pred = MixedSchemaPredictor(model, B)
    ks = [1, 5, 10, 20]
    for flag in (False, True, False, True):                       # warm-up of both forms
        m = pred.evaluate_loader(loader, ranking_ks=ks, group_auc=flag)
    plain, grouped = [], []
    for _ in range(reps):                                         # alternating: the same neighbours for both
        plain.append(wall(lambda: pred.evaluate_loader(loader, ranking_ks=ks))[0])
        grouped.append(wall(lambda: pred.evaluate_loader(loader, ranking_ks=ks, group_auc=True))[0])
    uid = torch.from_numpy(feats["user_id"]).cuda()
    y, s = pred.last_labels, pred.last_scores
    calls, dev = 10, []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            grouped_auc_device(uid, y, s, 944)
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b) / calls)                     # ms
    print(json.dumps(dict(case="evaluate_loader", split=f"{U}x{C}", B=B, reps=reps,
                          without_flag_ms=stats(plain), with_flag_ms=stats(grouped),
                          difference_of_medians_ms=round(float(np.median(grouped) - np.median(plain)) * 1e3, 3),
                          metric_device_ms=stats(dev, scale=1.0), gauc=m["gauc"], uauc=m["uauc"])), flush=True)


def large_case(reps, host_reps):
    from sklearn.metrics import roc_auc_score
    from deepfm_amd.training import compute_gauc
    n, groups = 1_000_000, 10_000
    rng = np.random.default_rng(1)
    g = rng.integers(0, groups, n)
    y = (rng.random(n) < 0.3).astype(np.float32)
    s = (rng.random(n) * 0.5 + 0.2 * y).astype(np.float32)
    d_g, d_y, d_s = (torch.from_numpy(x).cuda() for x in (g, y, s))
    for _ in range(3):
        got = compute_gauc(d_g, d_y, d_s, groups)
    device = [wall(lambda: compute_gauc(d_g, d_y, d_s, groups))[0] for _ in range(reps)]

    def host_loop():
        hg, hy, hs = d_g.cpu().numpy(), d_y.cpu().numpy(), d_s.cpu().numpy()
        order = np.argsort(hg, kind="stable")
        bounds = np.flatnonzero(np.diff(hg[order])) + 1
        aucs, weights = [], []
        for idx in np.split(order, bounds):
            yu = hy[idx]
            if 0 < yu.sum() < yu.size:
                aucs.append(roc_auc_score(yu, hs[idx]))
                weights.append(idx.size)
        return {"gauc": float(np.average(aucs, weights=weights)), "uauc": float(np.mean(aucs))}

    host, ref = [], None
    for _ in range(host_reps):
        t, ref = wall(host_loop)
        host.append(t)
    print(json.dumps(dict(case="compute_gauc", samples=n, groups=groups, reps=reps, host_reps=host_reps,
                          device_ms=stats(device), host_loop_s=stats(host, scale=1.0),
                          gauc=got["gauc"], gauc_host=ref["gauc"], uauc=got["uauc"], uauc_host=ref["uauc"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--only", choices=["evaluate_loader", "compute_gauc"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gauc.py measures on the device: no GPU found")
    if args.only != "compute_gauc":
        evaluation_case(args.reps)
    if args.only != "evaluate_loader":
        large_case(args.reps, args.host_reps)


if __name__ == "__main__":
    main()
