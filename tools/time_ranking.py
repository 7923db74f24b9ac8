#!/usr/bin/env python3
"""Device time of the ranking pass (``ranking_metrics_device``: one memset and four launches of csrc/ranking.hip)
on leave-one-out splits: 943 users x 1000 candidates (ML-100k's eval shape) contiguous and shuffled, and
138 493 users x 100 (ML-20M's user count) contiguous and shuffled.  Each repetition brackets ``--calls``
back-to-back calls with device events; the median over ``--reps`` repetitions, per call, is reported, with the
wall time of one ``compute_ranking_metrics`` call (device tensors in, dict out on the host).
One JSON line per shape.
usage: python tools/time_ranking.py [--reps 25] [--calls 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("ml100k_contiguous", 943, 1000, False), ("ml100k_shuffled", 943, 1000, True),
          ("ml20m_contiguous", 138_493, 100, False), ("ml20m_shuffled", 138_493, 100, True)]
KS = [1, 5, 10, 20]


def split(users, cands, shuffled, seed=0):
    rng = np.random.default_rng(seed)
    uid = np.repeat(np.arange(users, dtype=np.int64), cands)
    y = np.zeros(uid.size, np.float32)
    y[np.arange(users) * cands + rng.integers(0, cands, users)] = 1.0
    s = rng.random(uid.size).astype(np.float32)
    if shuffled:
        p = rng.permutation(uid.size)
        uid, y, s = uid[p], y[p], s[p]
    return [torch.from_numpy(x).cuda() for x in (uid, y, s)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    from deepfm_amd.training import compute_ranking_metrics, ranking_metrics_device
    for name, users, cands, shuffled in SHAPES:
        uid, y, s = split(users, cands, shuffled)
        for _ in range(3):
            ranking_metrics_device(uid, y, s, KS, users)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                ranking_metrics_device(uid, y, s, KS, users)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / args.calls)
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            m = compute_ranking_metrics(uid, y, s, KS, users)
            walls.append((time.perf_counter() - t0) * 1e6)
        print(json.dumps(dict(shape=name, users=users, candidates=cands, samples=users * cands,
                              device_us_median=round(float(np.median(times)), 2),
                              device_us_min=round(float(np.min(times)), 2), reps=args.reps, calls=args.calls,
                              wall_us_median=round(float(np.median(walls)), 1),
                              hr20=m["HR@20"])), flush=True)


if __name__ == "__main__":
    main()
