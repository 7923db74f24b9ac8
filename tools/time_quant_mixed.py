#!/usr/bin/env python3
"""Quantised tables for mixed schemas (``QuantizedMixedTables`` / ``QuantizedMixedPredictor``,
``dfm_embedding_forward_record_quant``) against the fp32 record gather (``MixedSchemaPredictor``,
``dfm_embedding_forward_record``): fp32, int8 and uint4 of the same checkout in the same run, alternating, at B = 4096:
  (a) ``movielens``: the MovieLens schema (tools/time_train_mixed.py:movielens_fields, DeepFM 256-128-64); only the two
      width-16 fields are quantised and every table sits in cache;
  (b) ``history``: user_id and item_id at width 16 with 10^6 rows each, a history bag of L earlier items over a
      10^6-row table of its own at width 16 (mean), two narrow SPARSE fields of widths 4 and 8 and two DENSE fields; ids
      uniform and Zipf (log-uniform rank, exponent 1: a head that stays in cache), L = 50 and 200, every bag full.
Per case:
  * the gather alone, as the predictors launch it: 16 launches over 4 different records captured into one graph and
    replayed (device events; no host time);
  * a ``predict_from`` launch (graph mode, the launch alone as tools/time_predict.py times it);
  * the byte floor of each gather at 8 TB/s: the ids, values and table bytes it must read (a record or an fp32 row and
    first-order weight per id, no reuse assumed) and the outputs it writes, over the HBM peak;
  * ``tables.nbytes`` against ``fp32_nbytes``.
Medians and ranges over ``--reps`` repetitions; one JSON line per case.
usage: python tools/time_quant_mixed.py [--reps 15] [--iters 50] [--only movielens|history]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.time_quant_predict import GATHERS_PER_GRAPH, events_us, gather_graph, stats  # noqa: E402
from tools.time_train_mixed import B, movielens_fields  # noqa: E402

HBM_BYTES_PER_S = 8e12
ROWS = 10 ** 6


def history_fields(L):
    f = lambda name, kind, V, d, ml=1: dict(name=name, type=kind, vocab=V, dim=d, max_len=ml, combiner="mean")
    return [f("user_id", "sparse", ROWS, 16), f("item_id", "sparse", ROWS, 16), f("hist", "sequence", ROWS, 16, L),
            f("device", "sparse", 64, 4), f("region", "sparse", 1024, 8), f("hour", "dense", 0, 4),
            f("recency", "dense", 0, 8)]


def make_model(fields):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.synthetic import schema_from_fields
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = 16
    cfg.dnn.hidden_units, cfg.dnn.dropout = [256, 128, 64], 0.0
    torch.manual_seed(0)
    model = create_model("deepfm", schema_from_fields(fields), cfg).cuda().eval()
    with torch.no_grad():                      # trained-like tables; the padding rows stay 0
        for f in fields:
            if f["type"] != "dense":
                model.embedding.second_order_embeddings[f["name"]].weight[1:].uniform_(-0.5, 0.5)
                model.embedding.first_order_embeddings[f["name"]].weight[1:].uniform_(-0.5, 0.5)
    return model


def draw(dist, V, shape, gen):
    if dist == "uniform":
        return torch.randint(1, V, shape, generator=gen, device="cuda", dtype=torch.int64)
    u = torch.rand(shape, generator=gen, device="cuda", dtype=torch.float64)      # rank = V^u: Zipf, exponent 1
    return torch.exp(u * float(np.log(V))).long().clamp_(1, V - 1)


def make_records(layout, fields, dist, nrec, gen):
    out = []
    for _ in range(nrec):
        rec = torch.zeros(layout.record_bytes, dtype=torch.uint8, device="cuda")
        ids, dense, _, bags = layout.views(rec)
        si = bi = 0
        for f in fields:
            if f["type"] == "sparse":
                ids[si].copy_(draw(dist, f["vocab"], (B,), gen)); si += 1
            elif f["type"] == "sequence":
                bags[bi].copy_(draw(dist, f["vocab"], (B, f["max_len"]), gen)); bi += 1
        dense.copy_(torch.rand(dense.shape, generator=gen, device="cuda"))
        out.append(rec)
    return out


def floor_us(fields, tables):
    """Bytes a gather of B samples must move, over the HBM peak: per id its 8 bytes and a record (quantised field) or
    an fp32 row and first-order weight; a DENSE value; the labels; first_order, fm and flat written."""
    per = 4 + 4 + 4                                            # label read, first_order and fm written
    for f in fields:
        d, n = f["dim"], f["max_len"]
        per += 4 * d                                           # its flat columns
        if f["type"] == "dense":
            per += 4
        elif tables is not None and f["name"] in tables.records:
            per += n * (8 + tables.row_bytes(f["name"]))
        else:
            per += n * (8 + 4 * d + 4)
    return round(B * per / HBM_BYTES_PER_S * 1e6, 3)


def case(name, fields, dists, reps, iters, extra):
    from deepfm_amd.training import MixedSchemaPredictor, QuantizedMixedPredictor
    model = make_model(fields)
    preds = {"fp32": MixedSchemaPredictor(model, B, use_graph=True)}
    for fmt in ("int8", "uint4"):
        preds[fmt] = QuantizedMixedPredictor(model, B, use_graph=True, fmt=fmt)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for dist in dists:
        records = make_records(preds["fp32"].layout, fields, dist, 4, gen)
        res = dict(case=name, batch=B, ids=dist, reps=reps, **extra)
        graphs = {k: gather_graph(p, records) for k, p in preds.items()}
        times = {k: [] for k in graphs}
        for g in graphs.values():                    # warm-up
            g.replay()
        for _ in range(reps):                        # alternating: the same neighbours for all three
            for k, g in graphs.items():
                times[k].append(events_us(g.replay, GATHERS_PER_GRAPH))
        res.update({f"gather_{k}_us": stats(t) for k, t in times.items()})
        res.update({f"gather_{k}_floor_us": floor_us(fields, getattr(p, "tables", None)) for k, p in preds.items()})

        def run(p):
            for i in range(iters):
                p._launch(records[i % 4].data_ptr(), B, p.probs, None, p.st_labels)
        times = {k: [] for k in preds}
        for p in preds.values():
            run(p)
        for _ in range(reps):
            for k, p in preds.items():
                times[k].append(events_us(lambda: run(p), iters))
        res.update({f"predict_{k}_us": stats(t) for k, t in times.items()})
        for p in preds.values():
            p.emb.raise_on_bad_index()
        print(json.dumps(res), flush=True)
    t8, t4 = preds["int8"].tables, preds["uint4"].tables
    print(json.dumps(dict(case=f"{name}_bytes", quantised=list(t8.records), fp32_fields=t8.fp32_fields,
                          int8_table_bytes=t8.nbytes, uint4_table_bytes=t4.nbytes, fp32_table_bytes=t8.fp32_nbytes,
                          **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default=None, choices=["movielens", "history"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_quant_mixed.py measures on the device: no GPU found")
    if args.only in (None, "movielens"):
        case("movielens", movielens_fields(), ["uniform"], args.reps, args.iters, {})
        torch.cuda.empty_cache()
    if args.only in (None, "history"):
        for L in (50, 200):
            case("history", history_fields(L), ["uniform", "zipf"], args.reps, args.iters, dict(L=L))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
