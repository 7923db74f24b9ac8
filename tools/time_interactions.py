#!/usr/bin/env python3
"""Time the interaction log on the device (``deepfm_amd/data/interactions.py``) against its host
counterparts on the same data, in one process.

Shapes: the ML-100K shape (100 000 rows, 943 users, 1682 items) and one large shape inside the 1 GiB seen-set limit
(``--rows`` 10^7, ``--users`` 10^5, ``--items`` 10^4: 239 MiB of bitmap + prefix).  The columns start on the device.

  seen_sets      ``log.seen_sets()``                 vs  the two columns copied to the host, ``SeenSets.from_interactions``
                                                         and ``upload``
  counts         ``log.counts("item", train)``       vs  the columns and the index copied to the host, ``np.bincount``,
                                                         the counts copied back
  temporal       ``log.temporal_split(0.1, 0.1)``    vs  the columns copied to the host, a vectorised numpy statement of
                 (its ``torch.sort`` included)           the same split (stable argsort, masks, ``np.unique``), the three
                                                         index arrays copied back
  leave_one_out  ``log.leave_one_out_split(3)``      vs  the same for the leave-one-out split
                 (its two sorts and the counts)

Every device result is compared with the host one before anything is timed.  Wall clock around work that ends in a
device synchronise; medians of ``--reps`` (15) with min-max, ``--host-reps`` for the host side of the large shape (a
repeat takes seconds).  The byte floor of each pass is what its kernels must move (the sorts left out) over 8 TB/s.
One JSON object.  Needs the GPU: there is no fallback.

    python tools/time_interactions.py [--rows N --users U --items I] [--reps 15] [--host-reps 3] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def stats(xs, scale=1.0):
    xs = sorted(x * scale for x in xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


def host_temporal(user, ts, labels, n_users, val_ratio, test_ratio):
    from tests.interactions_reference import quantile
    order = np.argsort(ts, kind="stable")
    st = ts[order]
    floors = [math.floor(quantile(st, q)) for q in (1 - val_ratio - test_ratio, 1 - test_ratio)]
    n_train, n_trainval = (int(np.searchsorted(st, f, side="right")) for f in floors)
    train = order[:n_train]
    in_train = np.zeros(n_users, bool)
    in_train[user[train]] = True

    def first_positive_per_user(rows):
        rows = rows[(labels[rows] == 1.0) & in_train[user[rows]]]
        return rows[np.unique(user[rows], return_index=True)[1]]

    return train, first_positive_per_user(order[n_train:n_trainval]), first_positive_per_user(order[n_trainval:])


def host_leave_one_out(user, ts, n_users, min_interactions):
    by_time = np.argsort(ts, kind="stable")
    order = by_time[np.argsort(user[by_time], kind="stable")]
    su = user[order]
    last = np.ones(len(su), bool)
    last[:-1] = su[1:] != su[:-1]
    before_last = np.zeros(len(su), bool)
    before_last[:-1] = last[1:] & ~last[:-1]
    eligible = np.bincount(user, minlength=n_users)[su] >= min_interactions
    return order[~((last | before_last) & eligible)], order[before_last & eligible], order[last & eligible]


def measure(n, n_users, n_items, reps, host_reps):
    from deepfm_amd.data import DeviceInteractionLog, SeenSets
    dev = torch.device("cuda")
    rng = np.random.default_rng(n)
    user = np.minimum(rng.zipf(1.2, n) - 1, n_users - 1).astype(np.int64)       # a few heavy users, a long tail
    user = rng.permutation(n_users)[user]
    item = np.minimum(rng.zipf(1.1, n) - 1, n_items - 1).astype(np.int64)
    ts = rng.integers(0, 10 * n, n).astype(np.int64) + 874724710
    labels = (rng.random(n) < 0.55).astype(np.float32)
    log = DeviceInteractionLog(user, item, ts, labels, n_users, n_items, dev)
    W = (n_items + 31) // 32
    out = {"rows": n, "n_users": n_users, "n_items": n_items, "seen_set_bytes": 4 * n_users * (2 * W + 1),
           "reps": reps, "host_reps": host_reps}

    def cpu(*tensors):
        return [t.cpu().numpy() for t in tensors]

    def done(key, res):
        out[key] = res
        print(f"[{n} rows] {key}: device {res['device_ms']['median']:.3f} ms" +
              (f", host {res['host_ms']['median']:.1f} ms" if "host_ms" in res else ""), file=sys.stderr, flush=True)

    # ---- seen-sets
    def host_seen():
        u, i = cpu(log.user_rows, log.item_rows)
        return SeenSets.from_interactions(u, i, n_users, n_items).upload(dev)
    want, got = host_seen(), log.seen_sets().upload(dev)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "device and host seen-sets differ"
    del want, got
    res = {"device_ms": stats(wall(log.seen_sets, reps), 1e3), "host_ms": stats(wall(host_seen, host_reps), 1e3)}
    res["byte_floor_ms"] = (16.0 * n + 12.0 * n_users * W + 4.0 * n_users) / HBM_BYTES_PER_S * 1e3
    done("seen_sets", res)

    # ---- temporal split
    def host_split(fn):
        parts = fn(*cpu(log.user_rows, log.timestamps, log.labels))
        return [torch.from_numpy(p).to(dev) for p in parts]
    temporal_host = lambda: host_split(lambda u, t, lab: host_temporal(u, t, lab, n_users, 0.1, 0.1))   # noqa: E731
    split = log.temporal_split(0.1, 0.1)
    for g, w in zip(split, temporal_host()):
        assert torch.equal(g, w), "device and host temporal splits differ"
    res = {"device_ms": stats(wall(lambda: log.temporal_split(0.1, 0.1), reps), 1e3),
           "of_which_torch_sort_ms": stats(wall(lambda: torch.sort(log.timestamps, stable=True), reps), 1e3),
           "host_ms": stats(wall(temporal_host, host_reps), 1e3),
           "parts": [int(p.numel()) for p in split]}
    res["byte_floor_ms"] = (16.0 * n + 4.0 * (n - split.train.numel()) + 17.0 * n_users) / HBM_BYTES_PER_S * 1e3
    done("temporal_split", res)

    # ---- counts over the train part
    train = split.train
    def host_counts():
        i, lab, rows = cpu(log.item_rows, log.labels, train)
        return torch.from_numpy(np.bincount(i[rows][lab[rows] == 1.0], minlength=n_items)).to(dev)
    assert torch.equal(log.counts("item", train), host_counts()), "device and host counts differ"
    from deepfm_amd import _lib
    res = {"route": "lds" if n_items <= _lib.COUNTS_LDS_ENTITIES else "global",
           "device_ms": stats(wall(lambda: log.counts("item", train), reps), 1e3),
           "host_ms": stats(wall(host_counts, host_reps), 1e3)}
    res["byte_floor_ms"] = (20.0 * train.numel() + 8.0 * n_items) / HBM_BYTES_PER_S * 1e3
    done("counts_item_over_train", res)
    res = {"route": "lds" if n_users <= _lib.COUNTS_LDS_ENTITIES else "global",
           "device_ms": stats(wall(lambda: log.counts("user", train), reps), 1e3)}
    res["byte_floor_ms"] = (20.0 * train.numel() + 8.0 * n_users) / HBM_BYTES_PER_S * 1e3
    done("counts_user_over_train", res)

    # ---- leave-one-out split
    loo_host = lambda: host_split(lambda u, t, lab: host_leave_one_out(u, t, n_users, 3))               # noqa: E731
    loo = log.leave_one_out_split(3)
    for g, w in zip(loo, loo_host()):
        assert torch.equal(g, w), "device and host leave-one-out splits differ"
    res = {"device_ms": stats(wall(lambda: log.leave_one_out_split(3), reps), 1e3),
           "host_ms": stats(wall(loo_host, host_reps), 1e3), "parts": [int(p.numel()) for p in loo]}
    res["byte_floor_ms"] = (8.0 * n + 8.0 * n_users + 17.0 * n + 8.0 * n_users) / HBM_BYTES_PER_S * 1e3
    done("leave_one_out_split", res)
    for key in ("seen_sets", "temporal_split", "counts_item_over_train", "leave_one_out_split"):
        out[key]["host_over_device"] = out[key]["host_ms"]["median"] / out[key]["device_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_interactions.py needs the GPU")
    out = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}
    measure(2000, 50, 40, 2, 2)                                                   # warm-up: code objects, allocator
    out["ml100k_shape"] = measure(100_000, 943, 1682, args.reps, args.reps)
    out["large_shape"] = measure(args.rows, args.users, args.items, args.reps, args.host_reps)
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
