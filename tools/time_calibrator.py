#!/usr/bin/env python3
"""Time of the score calibrators (``training/calibrator.py``, csrc/calibrator.hip), medians and ranges over ``--reps``:
  * ``fit``: Platt and isotonic (1024 bins) on 1 M (label, logit) samples on the device: the device time of one fit's
    launches by device events over back-to-back fits, and the wall clock of ``fit(...).report()`` (the host read
    included), with the rounds the Platt iteration used; against sklearn's ``LogisticRegression`` (one feature,
    ``C=1e12``) and ``IsotonicRegression`` on the same data on the host, the copies included, where sklearn is there;
  * ``apply``: both kinds on 4096 and on 1 M logits, device events over back-to-back launches, beside the byte floor
    (8 bytes per sample over ``--bandwidth``) and an empty launch;
  * ``predict_from``: one launch of the captured predictor with and without a calibrator for DeepFM, xDeepFM and
    AttentionDeepFM at the headline shape (tools/time_predict.py), alternating the two, and the head launch alone.
One JSON line per case.
usage: python tools/time_calibrator.py [--reps 15] [--bandwidth 8e12] [--only fit|apply|predict]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.time_predict import B, ND, S, SHAPES, V, build  # noqa: E402

N = 1_000_000


def stats(xs, digits=3):
    xs = np.asarray(xs, np.float64)
    return dict(median=round(float(np.median(xs)), digits), min=round(float(xs.min()), digits),
                max=round(float(xs.max()), digits))


def events_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def data():
    """A model that over-predicts after negative down-sampling: true logit u, the model's z = 1.3 u + 1.5."""
    rng = np.random.default_rng(4)
    u = rng.normal(-3.0, 1.5, N)
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-u))).astype(np.float32)
    return y, (1.3 * u + 1.5).astype(np.float32)


def fit_case(reps):
    from deepfm_amd.training import Calibrator
    y, z = data()
    d_y, d_z = torch.from_numpy(y).cuda(), torch.from_numpy(z).cuda()
    for kind in ("platt", "isotonic"):
        cal = Calibrator(kind)
        for _ in range(3):
            rep = cal.fit(d_y, d_z).report()
        device = [events_us(lambda i: cal.fit(d_y, d_z), 5) for _ in range(reps)]
        whole = [wall_ms(lambda: cal.fit(d_y, d_z).report())[0] for _ in range(reps)]
        out = dict(case="fit", kind=kind, samples=N, reps=reps, fit_device_us=stats(device), fit_report_wall_ms=stats(whole),
                   status=rep["status"])
        if kind == "platt":
            # the same fit with max_rounds = the rounds used: what the launches that return at once cost
            tight = Calibrator(kind, max_rounds=rep["rounds"])
            assert tight.fit(d_y, d_z).report()["status"] == "converged"
            exact = [events_us(lambda i: tight.fit(d_y, d_z), 5) for _ in range(reps)]
            out.update(rounds=rep["rounds"], max_rounds=cal.max_rounds, fit_device_us_max_rounds_as_used=stats(exact),
                       a=rep["a"], b=rep["b"], logloss_before=rep["logloss_before"], logloss_after=rep["logloss_after"])
        else:
            out.update(bins=cal.bins, knots=rep["knots"], blocks=rep["blocks"])
        try:
            if kind == "platt":
                from sklearn.linear_model import LogisticRegression
                host = lambda: LogisticRegression(C=1e12).fit(d_z.cpu().numpy().astype(np.float64)[:, None],  # noqa: E731
                                                              d_y.cpu().numpy())
            else:
                from sklearn.isotonic import IsotonicRegression
                host = lambda: IsotonicRegression(out_of_bounds="clip").fit(d_z.cpu().numpy(), d_y.cpu().numpy())  # noqa: E731
            host()
            out["host_sklearn_ms"] = stats([wall_ms(host)[0] for _ in range(min(reps, 5))])
        except ImportError:
            pass
        print(json.dumps(out), flush=True)


def apply_case(reps, bandwidth):
    from deepfm_amd import _lib
    from deepfm_amd.training import Calibrator
    y, z = data()
    d_y, d_z = torch.from_numpy(y).cuda(), torch.from_numpy(z).cuda()
    lib = _lib.load()
    empty = [events_us(lambda i: lib.dfm_debug_empty_launch(_lib.stream_handle()), 200) for _ in range(reps)]
    for kind in ("platt", "isotonic"):
        cal = Calibrator(kind).fit(d_y, d_z)
        for n in (4096, N):
            src, dst = d_z[:n], torch.empty(n, device="cuda")
            cal.apply(src, out=dst)
            us = [events_us(lambda i: cal.apply_into(src.data_ptr(), n, dst.data_ptr()), 200) for _ in range(reps)]
            print(json.dumps(dict(case="apply", kind=kind, samples=n, reps=reps, apply_us=stats(us),
                                  empty_launch_us=stats(empty), byte_floor_us=round(8 * n / bandwidth * 1e6, 3))),
                  flush=True)


def predict_case(reps):
    from deepfm_amd import _lib
    from deepfm_amd.training import Calibrator, FusedPredictor
    y, z = data()
    cal = Calibrator("platt").fit(y[:100_000], z[:100_000])
    iso = Calibrator("isotonic").fit(y[:100_000], z[:100_000])
    lib = _lib.load()
    for kind in SHAPES:
        model = build(kind)
        model.eval()
        g = torch.Generator(device="cuda").manual_seed(1)
        nrec = 4
        ids = torch.randint(1, V, (nrec, S, B), generator=g, device="cuda", dtype=torch.int64)
        dense = torch.rand((nrec, ND, B), generator=g, device="cuda")
        records = torch.cat([ids.view(nrec, -1).view(torch.uint8), dense.view(nrec, -1).view(torch.uint8),
                             torch.zeros(nrec, B * 4, dtype=torch.uint8, device="cuda")], 1).contiguous()
        preds = {"without": FusedPredictor(model, B), "platt": FusedPredictor(model, B, calibrator=cal),
                 "isotonic": FusedPredictor(model, B, calibrator=iso)}
        times = {k: [] for k in preds}
        launch = lambda p: (lambda i: p._launch(records[i % nrec].data_ptr(), B, p.probs, None, p.st_labels))  # noqa: E731
        for p in preds.values():
            events_us(launch(p), 10)
        for _ in range(reps):                                  # alternating: the same neighbours for all
            for k, p in preds.items():
                times[k].append(events_us(launch(p), 50))
        p = preds["without"]
        head = [events_us(lambda i: lib.dfm_predict_head(*p._head_args(B, p.probs, None), _lib.stream_handle()), 200)
                for _ in range(reps)]
        print(json.dumps(dict(case="predict_from", kind=kind, B=B, reps=reps,
                              **{f"{k}_us": stats(v) for k, v in times.items()}, head_launch_us=stats(head),
                              platt_minus_without_us=round(float(np.median(times["platt"]) -
                                                                 np.median(times["without"])), 3),
                              isotonic_minus_without_us=round(float(np.median(times["isotonic"]) -
                                                                    np.median(times["without"])), 3))), flush=True)
        del preds, model, p
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--bandwidth", type=float, default=8e12, help="HBM bytes per second of the byte floor")
    ap.add_argument("--only", choices=["fit", "apply", "predict"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_calibrator.py measures on the device: no GPU found")
    if args.only in (None, "fit"):
        fit_case(args.reps)
    if args.only in (None, "apply"):
        apply_case(args.reps, args.bandwidth)
    if args.only in (None, "predict"):
        predict_case(args.reps)


if __name__ == "__main__":
    main()
