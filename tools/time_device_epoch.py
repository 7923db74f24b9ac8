#!/usr/bin/env python3
"""Time an epoch's input side on a synthetic ML-100K-shaped set (943 users, 1 682 items, P = 90 000 positives,
K = 4 negatives each, B = 4096, the MovieLens schema; ``FusedMixedDeepFMStep`` as a graph, Adam, tower
[256, 128, 64]), in one process:

  a  the host path: ``PackedBatchLoader(shuffle=True)`` + ``DeviceBatchRing`` -> ``run_from`` over the 450 000
     pre-materialised rows (one fixed draw of negatives; the host path has no resampler to time);
  b  the same epoch through ``DeviceEpochLoader``, its ``set_epoch`` (negatives + permutation) included;
  c  ``set_epoch`` alone;
  d  one ``dfm_record_assemble`` launch (device events around a block of launches).

One warm-up epoch, then ``--epochs`` timed ones, a and b alternating, synchronised at epoch end only; prints the
median and the min-max spread as one JSON object.  Needs the GPU: there is no fallback.

    python tools/time_device_epoch.py [--epochs 5] [--json out.json]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N_USERS, N_ITEMS, P, K, B = 943, 1682, 90_000, 4, 4096
GROUPS = {"user_id": "user", "movie_id": "item", "gender": "user", "age": "user", "occupation": "user",
          "zip_prefix": "user", "genres": "item", "release_year_bucket": "item", "movie_age_at_rating": "context",
          "num_genres": "item", "dow_sin": "context", "dow_cos": "context", "hour_sin": "context", "hour_cos": "context",
          "user_rating_count": "user", "item_rating_count": "item"}


def dataset(rng):
    from deepfm_amd.data import BucketDifference, ItemTable, SeenSets
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.synthetic import random_fields_batch, schema_from_fields
    from time_train_mixed import movielens_fields
    fields = movielens_fields()
    schema = schema_from_fields(fields)
    for name, spec in schema.fields.items():
        spec.group = GROUPS[name]
    feats = random_fields_batch(fields, P, rng, zero_frac=0.0)
    user_of = rng.integers(0, N_USERS, P).astype(np.int32)
    item_of = rng.integers(0, N_ITEMS, P)
    items = {f["name"]: random_fields_batch([f], N_ITEMS, rng, zero_frac=0.0)[f["name"]]
             for f in fields if GROUPS[f["name"]] == "item"}
    items["movie_id"] = np.arange(N_ITEMS, dtype=np.int64) + 1
    feats["user_id"], feats["movie_id"] = user_of.astype(np.int64) + 1, item_of + 1
    for name, col in items.items():                       # a positive carries its own item's features
        feats[name] = col[item_of]
    rated = rng.uniform(20.0, 30.0, P).astype(np.float32)                  # years: rating time, release time
    released = rng.uniform(0.0, 28.0, N_ITEMS).astype(np.float32)
    bd = BucketDifference(rated, released, np.array([1, 2, 5, 10, 20, 40], np.float32), np.arange(8, dtype=np.int64))
    cols = PackedColumns(schema, feats, np.ones(P, np.float32))
    seen = SeenSets.from_interactions(user_of, item_of, N_USERS, N_ITEMS)
    return fields, schema, cols, user_of, ItemTable(schema, items), {"movie_age_at_rating": bd}, seen


def materialise(dcols, sampler, schema):
    """The 450 000 rows of epoch 0's draw as host columns: what the host path trains on."""
    from deepfm_amd.data import DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    rows = P * (1 + K)
    chunk = 4500
    loader = DeviceEpochLoader(dcols, chunk, shuffle=False, negatives=sampler, depth=2)
    feats, labels = {n: [] for n in schema.fields}, []
    for rec in loader:
        batch, lab = loader.layout.unpack(rec.cpu().numpy().copy())
        for n, v in batch.items():
            feats[n].append(v.copy())
        labels.append(lab.copy())
    assert len(loader) * chunk == rows
    return PackedColumns(schema, {n: np.concatenate(v) for n, v in feats.items()}, np.concatenate(labels))


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_device_epoch.py needs the GPU (no fallback)")
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, NegativeSampler
    from deepfm_amd.data.packed import DeviceBatchRing, PackedBatchLoader
    from deepfm_amd.training import DenseTableAdam, FusedMixedDeepFMStep
    from time_train_mixed import make_model
    dev = torch.device("cuda")
    fields, schema, cols, user_of, table, derived, seen = dataset(np.random.default_rng(0))
    dcols = DeviceColumns(cols, dev)
    sampler = NegativeSampler(dcols, seen, user_of, table, K, derived=derived, seed=0)
    host_cols = materialise(dcols, sampler, schema)
    model = make_model(fields)
    opt = DenseTableAdam(model, lr=1e-3, l2=1e-5, max_grad_norm=1.0)
    step = FusedMixedDeepFMStep(model, opt, B, use_graph=True)
    step.capture()
    host_loader = PackedBatchLoader(host_cols, B, shuffle=True, seed=0)
    ring = DeviceBatchRing(host_loader, dev, depth=4)
    dev_loader = DeviceEpochLoader(dcols, B, shuffle=True, seed=0, negatives=sampler, depth=4)
    assert len(host_loader) == len(dev_loader) == P * (1 + K) // B

    def epoch_a(e):
        host_loader.set_epoch(e)
        for rec in ring:
            step.run_from(rec)

    def epoch_b(e):
        dev_loader.set_epoch(e)
        for rec in dev_loader:
            step.run_from(rec)

    def wall(fn, e):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(e)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    wall(epoch_a, 0); wall(epoch_b, 0); wall(dev_loader.set_epoch, 0)      # the warm-up epoch of each
    ta, tb, tc = [], [], []
    for e in range(1, args.epochs + 1):
        ta.append(wall(epoch_a, e))
        tb.append(wall(epoch_b, e))
        tc.append(wall(dev_loader.set_epoch, e))
    model.embedding.raise_on_bad_index()
    # d: one assemble launch; and the sampler launch, the same way
    n, rec = 200, dev_loader.ring[0][:dev_loader.record_bytes]
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    td, ts = [], []
    for _ in range(args.epochs + 1):
        start.record()
        for i in range(n):
            dev_loader.assemble_into(rec, (i % len(dev_loader)) * B, B)
        stop.record(); stop.synchronize()
        td.append(start.elapsed_time(stop) / n * 1e3)
        start.record()
        for i in range(20):
            sampler.sample(i)
        stop.record(); stop.synchronize()
        ts.append(start.elapsed_time(stop) / 20 * 1e3)
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "users": N_USERS, "items": N_ITEMS, "positives": P, "negatives_per_positive": K,
           "batch": B, "steps_per_epoch": len(dev_loader), "record_bytes": dev_loader.record_bytes, "epochs": args.epochs,
           "a_host_ring_epoch_ms": stats(ta), "b_device_loader_epoch_ms": stats(tb), "c_set_epoch_ms": stats(tc),
           "d_record_assemble_us": stats(td[1:]), "sample_negatives_us": stats(ts[1:])}
    out["b_minus_a_ms"] = out["b_device_loader_epoch_ms"]["median"] - out["a_host_ring_epoch_ms"]["median"]
    out["a_spread_ms"] = out["a_host_ring_epoch_ms"]["max"] - out["a_host_ring_epoch_ms"]["min"]
    out["b_within_a_spread"] = bool(out["b_minus_a_ms"] <= out["a_spread_ms"])
    out["c_share_of_b"] = out["c_set_epoch_ms"]["median"] / out["b_device_loader_epoch_ms"]["median"]
    print(json.dumps(out, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
