#!/usr/bin/env python
"""Time the device-side evaluation candidates on the ML-100K shape: 943 queries x 1682 items,
B = 4096, DeepFM / xDeepFM / AttentionDeepFM.

  a  ``CatalogueScorer.evaluate`` end to end (assemble + score 943 x 1682 rows, select, rank, metrics)
     vs ``MixedSchemaPredictor.evaluate(columns)`` over the same rows as host ``PackedColumns``
  b  ``evaluate_loader`` over 943 x (1 + 999) weighted candidates, the draw included
     vs ``evaluate(columns)`` over the host-materialised rows of the same draw
  the host materialisation of either row set is timed once and stated apart (it is the parent's only way to get the
  rows); ``dfm_catalogue_topk`` and ``dfm_sample_weighted`` launches alone, by device events, and one
  ``dfm_record_assemble`` launch over 4096 candidate rows, in row order and shuffled.

``--short-users N`` gives N users a seen-set that leaves fewer than 999 unseen rows (0 .. 998, evenly spread), so that
(b) runs over a truncating ``WeightedNegatives`` (DESIGN.md §7b "Ragged candidate lists"); the ragged draw and the
ragged assemble launch are then timed beside the rectangular ones, which keep the data set nobody is short in.

Wall times around a synchronise, one warm-up run of each, then ``--runs`` runs: medians with min / max.  Records
nothing but what it measured; no threshold."""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N_USERS, N_ITEMS, C, B = 943, 1682, 999, 4096


def dataset(rng, short_users=0):
    from deepfm_amd.data import BucketDifference, ItemTable, SeenSets
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.synthetic import movielens_fields, random_fields_batch, schema_from_fields
    fields = movielens_fields(N_USERS, N_ITEMS)
    schema = schema_from_fields(fields)
    items = {f["name"]: random_fields_batch([f], N_ITEMS, rng, zero_frac=0.0)[f["name"]]
             for f in fields if f["group"] == "item"}
    items["movie_id"] = np.arange(N_ITEMS, dtype=np.int64) + 1
    feats = random_fields_batch(fields, N_USERS, rng, zero_frac=0.0)
    user_of = np.arange(N_USERS, dtype=np.int32)
    target = rng.integers(0, N_ITEMS, N_USERS)
    feats["user_id"] = user_of.astype(np.int64) + 1
    for name, col in items.items():
        feats[name] = col[target]
    hist_u, hist_i = rng.integers(0, N_USERS, 100_000), rng.integers(0, N_ITEMS, 100_000)     # ML-100K's ratings
    seen = SeenSets.from_interactions(np.concatenate([hist_u, user_of]), np.concatenate([hist_i, target]), N_USERS,
                                      N_ITEMS)
    bd = BucketDifference(rng.uniform(20.0, 30.0, N_USERS).astype(np.float32),
                          rng.uniform(0.0, 28.0, N_ITEMS).astype(np.float32),
                          np.array([1, 2, 5, 10, 20, 40], np.float32), np.arange(8, dtype=np.int64))
    counts = np.bincount(np.concatenate([hist_i, target]), minlength=N_ITEMS)
    cols = PackedColumns(schema, feats, np.ones(N_USERS, np.float32))
    seen_short = None
    if short_users:
        # user u of the first N keeps `left[u]` unseen rows, its target not among them; the popularity counts stay
        left = np.linspace(0, C - 1, short_users).astype(np.int64)
        more_u, more_i = [], []
        for u, n in enumerate(left):
            fresh = np.setdiff1d(np.arange(N_ITEMS), np.append(hist_i[hist_u == u], target[u]))
            keep = rng.permutation(fresh)[:n]
            rows = np.setdiff1d(np.arange(N_ITEMS), keep)
            more_u.append(np.full(rows.size, u, np.int64)); more_i.append(rows)
        seen_short = SeenSets.from_interactions(np.concatenate([hist_u, user_of] + more_u),
                                                np.concatenate([hist_i, target] + more_i), N_USERS, N_ITEMS)
        assert (seen_short.unseen[:short_users] == left).all()
    return (fields, schema, cols, user_of, target, ItemTable(schema, items), {"movie_age_at_rating": bd}, seen, counts,
            seen_short)


def materialise(dcols, source, schema, first, chunk):
    """The loader's rows from ``first`` on as host columns, read back in records of ``chunk`` rows."""
    from deepfm_amd.data import DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    loader = DeviceEpochLoader(dcols, chunk, shuffle=False, negatives=source, depth=2)
    feats, labels = {n: [] for n in schema.fields}, []
    for s in range(first, loader.rows, chunk):
        cnt = min(chunk, loader.rows - s)
        batch, lab = loader.layout.unpack(loader.rows_into_next(s, cnt).cpu().numpy().copy())
        for n, v in batch.items():
            feats[n].append(v[:cnt].copy())
        labels.append(lab[:cnt].copy())
    return PackedColumns(schema, {n: np.concatenate(v) for n, v in feats.items()}, np.concatenate(labels))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def runs(fn, n):
    wall(fn)
    return stats([wall(fn)[0] for _ in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--short-users", type=int, default=0,
                    help="users with fewer than 999 unseen rows: (b) and the launch timings use a truncating source")
    args = ap.parse_args()
    if not 0 <= args.short_users <= N_USERS:
        raise SystemExit(f"--short-users must be in [0, {N_USERS}]")
    if not torch.cuda.is_available():
        raise SystemExit("time_catalogue.py needs the GPU (no fallback)")
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data import (CatalogueCandidates, DeviceColumns, DeviceEpochLoader, WeightedNegatives,
                                 item_weights)
    from deepfm_amd.models import create_model
    from deepfm_amd.training import CatalogueScorer, MixedSchemaPredictor
    dev = torch.device("cuda")
    fields, schema, cols, user_of, target, table, derived, seen, counts, seen_short = dataset(
        np.random.default_rng(0), args.short_users)
    dcols = DeviceColumns(cols, dev)
    cand = CatalogueCandidates(dcols, seen, user_of, table, derived=derived)
    rect = WeightedNegatives(dcols, seen, user_of, table, item_weights(counts, 0.75), C, derived=derived, seed=0)
    weighted = rect
    if args.short_users:
        weighted = WeightedNegatives(dcols, seen_short, user_of, table, item_weights(counts, 0.75), C, derived=derived,
                                     seed=0, short_users="truncate")
        assert weighted.counts is not None
    ks = [1, 5, 10, 20]
    t_mat_a, host_a = wall(lambda: materialise(dcols, cand, schema, N_USERS, 1682 * 41))
    weighted.sample(0)
    t_mat_b, host_b = wall(lambda: materialise(dcols, weighted, schema, 0, 23_575))
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "date": datetime.date.today().isoformat(), "queries": N_USERS, "items": N_ITEMS,
           "weighted_candidates": C, "batch": B, "runs": args.runs, "short_users": args.short_users,
           "total_candidates": weighted.total_candidates,
           "host_materialise_catalogue_rows_ms": t_mat_a, "host_materialise_weighted_rows_ms": t_mat_b, "models": {}}
    for kind in ("deepfm", "xdeepfm", "attention_deepfm"):
        cfg = ExperimentConfig()
        cfg.feature.fm_embed_dim = 16
        cfg.dnn.hidden_units, cfg.dnn.dropout = [256, 128, 64], 0.0
        if kind == "xdeepfm":
            cfg.cin.layer_sizes, cfg.cin.split_half = [64], True
        if kind == "attention_deepfm":
            cfg.attention.num_heads, cfg.attention.attention_dim = 4, 64
            cfg.attention.num_layers, cfg.attention.use_residual = 1, True
        torch.manual_seed(0)
        model = create_model(kind, schema, cfg).cuda()
        pred = MixedSchemaPredictor(model, B)
        scorer = CatalogueScorer(pred, cand)
        loader = DeviceEpochLoader(dcols, B, shuffle=False, negatives=weighted, depth=4)

        def device_b():
            loader.set_epoch(0)                            # the draw is part of the device path
            return pred.evaluate_loader(loader, ranking_ks=ks)

        r = {"a_catalogue_evaluate_ms": runs(lambda: scorer.evaluate(target, ks), args.runs),
             "a_host_fed_evaluate_ms": runs(lambda: pred.evaluate(host_a), args.runs),
             "b_evaluate_loader_ms": runs(device_b, args.runs),
             "b_host_fed_evaluate_ms": runs(lambda: pred.evaluate(host_b, ranking_ks=ks), args.runs)}
        r["b_same_metrics"] = device_b() == pred.evaluate(host_b, ranking_ks=ks)
        r["full_metrics"] = scorer.evaluate(target, ks)
        out["models"][kind] = r
    # the two new launches alone
    sc = scorer.scores()
    t = torch.from_numpy(target.astype(np.int32)).to(dev)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tk, ts = [], []
    for _ in range(args.runs + 1):
        start.record()
        for _ in range(20):
            scorer._topk(sc, t, 10, True)
        stop.record(); stop.synchronize()
        tk.append(start.elapsed_time(stop) / 20 * 1e3)
        start.record()
        for e in range(20):
            rect.sample(e)
        stop.record(); stop.synchronize()
        ts.append(start.elapsed_time(stop) / 20 * 1e3)
    out["catalogue_topk_k10_us"] = stats(tk[1:])           # with the output allocations of one call
    out["sample_weighted_us"] = stats(ts[1:])

    def launches(fns, reps):
        """us per call of each ``fns[name](i)``: events around ``reps`` back-to-back calls, the functions alternating,
        one warm-up round then ``--runs`` rounds."""
        us = {name: [] for name in fns}
        for _ in range(args.runs + 1):
            for name, fn in fns.items():
                start.record()
                for i in range(reps):
                    fn(i)
                stop.record(); stop.synchronize()
                us[name].append(start.elapsed_time(stop) / reps * 1e3)
        return {name: stats(v[1:]) for name, v in us.items()}

    sources = {"rectangular": rect}
    if args.short_users:
        sources["ragged"] = weighted
    out["sample_weighted_by_shape_us"] = launches({name: src.sample for name, src in sources.items()}, 20)
    # one assemble launch over the same 4096 candidate rows (from row Q on), in row order and shuffled
    for shuffle in (False, True):
        fns = {}
        for name, src in sources.items():
            ld = DeviceEpochLoader(dcols, B, shuffle=shuffle, seed=0, negatives=src, depth=2)
            fns[name] = (lambda ld, rec: lambda i: ld.assemble_into(rec, N_USERS, B))(ld, ld.ring[0][:ld.record_bytes])
        out[f"assemble_{'shuffled' if shuffle else 'ordered'}_us"] = launches(fns, 200)
    print(json.dumps(out, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
