#!/usr/bin/env python3
"""Time the user histories on the device (``deepfm_amd/data/interactions.py``, ``csrc/history.hip``, DESIGN.md §7b
"User histories on the device") against the host path they replace, on the same data, in one process.

Shapes: the ML-100K shape (100 000 rows, 943 users, 1682 items) and a large one (``--rows`` 10^7, ``--users`` 10^5,
``--items`` 10^4) with users and items drawn Zipf as ``tools/time_interactions.py`` draws them; bags of ``--length`` 20
ids for every row of the log.  The columns start on the device.

  history_index    ``log.history_index()``: two stable ``torch.sort``, the counts, the scan, one kernel launch; the
                   sorts alone and the rest are also timed apart
  lookup           ``index.lookup(all rows, L, ties)`` for both ``ties``: one launch and its status read
  latest           ``index.latest(all users, L)``
  host             the yardstick: the four columns copied to the host, the vectorised numpy restatement
                   (``tests/history_reference.py:histories``) and the upload of its (n, L) int64 bag, count and gap

Every device result is compared with the host one.  Wall clock around work that ends in a device synchronise; medians
of ``--reps`` (15) with min-max, ``--host-reps`` for the host side of the large shape (a repeat takes many seconds).
The byte floor of a launch is what it must move over 8 TB/s, from the shapes and the counts.  ``longest_user`` is what
the one-wavefront-per-user index kernel serialises: its rows and its trips of 64.  One JSON object.  Needs the GPU.

    python tools/time_history.py [--rows N --users U --items I --length L] [--reps 15] [--host-reps 1] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
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


def index_floor_bytes(n, n_users, events, masked):
    """dfm_history_index_build: order, user, item, timestamp, label (and mask) in; pos_of, rank, sorted_ts out; one
    int32 per event; start in and event_count out per user."""
    return (36.0 + (1.0 if masked else 0.0)) * n + 16.0 * n + 4.0 * events + 12.0 * n_users


def gather_floor_bytes(m, L, filled, mode):
    """dfm_history_gather: per query its row (or user), user, pos_of, start pair, rank (or event_count), the two
    timestamps of the gap, count and gap out; per filled slot the event and its item row; every slot stored."""
    per_query = {"position": 8 + 8 + 4 + 16 + 4 + 16 + 16, "exclude": 8 + 8 + 4 + 16 + 4 + 8 + 16 + 16,
                 "latest": 8 + 16 + 4 + 16}[mode]
    return float(per_query) * m + 12.0 * filled + 8.0 * m * L


def measure(n, n_users, n_items, L, reps, host_reps):
    from deepfm_amd.data import DeviceInteractionLog
    from tests.history_reference import histories
    dev = torch.device("cuda")
    rng = np.random.default_rng(n)
    user = np.minimum(rng.zipf(1.2, n) - 1, n_users - 1).astype(np.int64)       # a few heavy users, a long tail
    user = rng.permutation(n_users)[user]
    item = np.minimum(rng.zipf(1.1, n) - 1, n_items - 1).astype(np.int64)
    ts = rng.integers(0, 10 * n, n).astype(np.int64) + 874724710
    labels = (rng.random(n) < 0.55).astype(np.float32)
    log = DeviceInteractionLog(user, item, ts, labels, n_users, n_items, dev)
    longest = int(np.bincount(user, minlength=n_users).max())
    out = {"rows": n, "n_users": n_users, "n_items": n_items, "length": L, "reps": reps, "host_reps": host_reps,
           "longest_user": {"rows": longest, "trips_of_64": (longest + 63) // 64}}
    del user, item, ts, labels
    rows = torch.arange(n, device=dev)
    users = torch.arange(n_users, device=dev)

    def done(key, res):
        out[key] = res
        print(f"[{n} rows] {key}: " + ", ".join(f"{k[:-3]} {v['median']:.3f} ms" for k, v in res.items()
                                                if k.endswith("_ms") and isinstance(v, dict)), file=sys.stderr, flush=True)

    def sorts():
        by_time = torch.sort(log.timestamps, stable=True)[1]
        return by_time[torch.sort(log.user_rows[by_time], stable=True)[1]]

    index = log.history_index()
    events = int(index.event_count.sum())
    total = wall(log.history_index, reps)
    sort_only = wall(sorts, reps)
    res = {"device_ms": stats(total, 1e3), "of_which_torch_sorts_ms": stats(sort_only, 1e3), "events": events,
           "byte_floor_ms": index_floor_bytes(n, n_users, events, False) / HBM_BYTES_PER_S * 1e3}
    res["rest_ms_by_difference"] = res["device_ms"]["median"] - res["of_which_torch_sorts_ms"]["median"]
    done("history_index", res)

    def host(ties, queries):
        cols = [t.cpu().numpy() for t in (log.user_rows, log.item_rows, log.timestamps, log.labels)]
        return [torch.from_numpy(a).to(dev) for a in histories(*cols, queries.cpu().numpy(), L, ties=ties)]

    for ties in ("position", "exclude", "latest"):
        queries = users if ties == "latest" else rows
        call = (lambda: index.latest(queries, L)) if ties == "latest" else (lambda: index.lookup(queries, L, ties))
        got = call()
        filled = int(torch.clamp(got.count, max=L).sum())
        res = {"queries": int(queries.numel()), "filled_slots": filled, "device_ms": stats(wall(call, reps), 1e3),
               "byte_floor_ms": gather_floor_bytes(queries.numel(), L, filled, ties) / HBM_BYTES_PER_S * 1e3}
        want, times = None, []
        for _ in range(host_reps):
            del want
            torch.cuda.synchronize()
            t = time.perf_counter()
            want = host(ties, queries)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        for g, w, name in zip((got.bag, got.count, got.gap), want, ("bag", "count", "gap")):
            assert torch.equal(g, w), f"device and host {name} differ ({ties})"
        del got, want
        res["host_ms"] = stats(times, 1e3)
        # the host path has no index to keep: it is compared with the index and the lookup together
        res["host_over_index_plus_lookup"] = res["host_ms"]["median"] / (out["history_index"]["device_ms"]["median"] +
                                                                        res["device_ms"]["median"])
        done("latest" if ties == "latest" else f"lookup_{ties}", res)
    return out


def measure_lazy(n, n_users, n_items, L, batch, reps):
    """``--lazy``: the history column of a ``DeviceEpochLoader`` bound to the index (``HistoryBag``) against the same
    column materialised by ``lookup``, over every row of the log: one assemble launch (the mean of a run of
    consecutive batches, one synchronise behind the run) and one epoch (``set_epoch``, every batch, the tail), the two
    loaders alternating inside every repeat, and the bytes each keeps for the column."""
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, DeviceInteractionLog, HistoryBag, history_field
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    dev = torch.device("cuda")
    rng = np.random.default_rng(n)
    user = np.minimum(rng.zipf(1.2, n) - 1, n_users - 1).astype(np.int64)       # as measure() draws them
    user = rng.permutation(n_users)[user]
    item = np.minimum(rng.zipf(1.1, n) - 1, n_items - 1).astype(np.int64)
    ts = rng.integers(0, 10 * n, n).astype(np.int64) + 874724710
    labels = (rng.random(n) < 0.55).astype(np.float32)
    log = DeviceInteractionLog(user, item, ts, labels, n_users, n_items, dev)
    del user, item, ts, labels
    index = log.history_index()
    schema = DatasetSchema(fields={
        "user_id": FieldSchema("user_id", FeatureType.SPARSE, n_users + 1, 16, "user"),
        "item_id": FieldSchema("item_id", FeatureType.SPARSE, n_items + 1, 16, "item"),
        "hist": history_field("hist", L, n_items, 16)})
    ids = torch.stack([log.user_rows + 1, log.item_rows + 1]).contiguous()
    dense = torch.empty(0, n, dtype=torch.float32, device=dev)
    bag = HistoryBag(index, torch.arange(n, device=dev), L)
    whole = bag.materialize()
    filled = int(torch.clamp(whole.count, max=L).sum())
    loaders = {"bound": DeviceEpochLoader(DeviceColumns.from_device(schema, ids, dense, log.labels, bags=[bag]),
                                          batch, shuffle=True, seed=1),
               "materialised": DeviceEpochLoader(DeviceColumns.from_device(schema, ids, dense, log.labels,
                                                                           bags=[whole.bag]), batch, shuffle=True, seed=1)}
    run = min(64, len(loaders["bound"]))
    for loader in loaders.values():
        loader.set_epoch(1)
    assert all(torch.equal(loaders["bound"].record(k), loaders["materialised"].record(k)) for k in (0, run - 1))

    def launches(loader):
        for k in range(run):
            loader.record(k)

    def epoch(loader):
        loader.set_epoch(2)
        for _ in loader:
            pass
        loader.tail()

    times = {(what, name): [] for what in ("launch", "epoch") for name in loaders}
    for fn, what in ((launches, "launch"), (epoch, "epoch")):
        for loader in loaders.values():                      # warm-up of this shape
            fn(loader)
        for _ in range(reps):                                # alternating: both see the same neighbours
            for name, loader in loaders.items():
                times[what, name] += wall(lambda: fn(loader), 1)
    index_bytes = sum(t.numel() * t.element_size() for t in (index.start, index.pos_of, index.rank, index.events,
                                                             index.sorted_ts, index.event_count))
    out = {"rows": n, "n_users": n_users, "n_items": n_items, "length": L, "batch_size": batch, "reps": reps,
           "batches_per_epoch": len(loaders["bound"]), "launches_per_timed_run": run, "filled_slots": filled,
           "bytes_held": {"bound_queries": 8 * n, "index_shared_with_every_bag": index_bytes,
                          "materialised_bag": 8 * n * L}}
    for name in loaders:
        out[name] = {"launch_us": stats(times["launch", name], 1e6 / run), "epoch_ms": stats(times["epoch", name], 1e3)}
    out["bound_over_materialised"] = {
        "launch": out["bound"]["launch_us"]["median"] / out["materialised"]["launch_us"]["median"],
        "epoch": out["bound"]["epoch_ms"]["median"] / out["materialised"]["epoch_ms"]["median"]}
    print(f"[{n} rows, L = {L}] " + ", ".join(
        f"{name}: launch {out[name]['launch_us']['median']:.2f} us, epoch {out[name]['epoch_ms']['median']:.2f} ms"
        for name in loaders), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--length", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--json")
    ap.add_argument("--lazy", action="store_true",
                    help="time the bag bound to the index at record assembly against the materialised bag, instead of "
                         "the measurements above")
    ap.add_argument("--lazy-length", type=int, default=50, help="--lazy: bag length of the large shape")
    ap.add_argument("--batch", type=int, default=4096, help="--lazy: the loaders' batch size")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_history.py needs the GPU")
    out = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}
    if args.lazy:
        measure_lazy(2000, 50, 40, args.length, 256, 2)                           # warm-up: code objects, allocator
        out["lazy"] = {"ml100k_shape": measure_lazy(100_000, 943, 1682, args.length, args.batch, args.reps),
                       "large_shape": measure_lazy(args.rows, args.users, args.items, args.lazy_length, args.batch,
                                                   args.reps)}
    else:
        measure(2000, 50, 40, args.length, 2, 1)                                  # warm-up: code objects, allocator
        out["ml100k_shape"] = measure(100_000, 943, 1682, args.length, args.reps, args.reps)
        out["large_shape"] = measure(args.rows, args.users, args.items, args.length, args.reps, args.host_reps)
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
