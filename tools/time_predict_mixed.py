#!/usr/bin/env python3
"""Evaluation on the MovieLens schema (tests/golden/model_deepfm_movielens.npz fields: a ``genres`` bag, widths 4 / 8 /
16, six DENSE fields) with the reference's configs/*_movielens.yaml models, B = 4096:
  * per batch: ``model.predict`` against ``MixedSchemaPredictor`` eager and graph, device events over back-to-back
    batches from device records, for DeepFM, xDeepFM and AttentionDeepFM;
  * a split of 943 users x 1000 candidates: ``evaluate(..., ranking_ks=[1, 5, 10, 20])`` against a ``model.predict``
    loop + ``compute_auc`` / ``compute_logloss`` / ``compute_ranking_metrics`` (wall clock, both ending on the host);
  * ``--trace``: only the gather launches (the record gather, then emb_fwd_general + first_order_sum + the FM kernel
    of ``model.predict``) for a ``rocprofv3 --kernel-trace --stats`` run of their own.
One JSON line per measurement.
usage: python tools/time_predict_mixed.py [--iters 50] [--only deepfm] [--trace]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepfm_amd.data.synthetic import random_fields_batch, schema_from_fields  # noqa: E402

B, U, C = 4096, 943, 1000
# the golden MovieLens schema (reference deepfm/data/movielens.py:360-416); the golden file is not read here
_S = [("user_id", "sparse", 944, 16), ("movie_id", "sparse", 1683, 16), ("gender", "sparse", 3, 4),
      ("age", "sparse", 8, 4), ("occupation", "sparse", 22, 8), ("zip_prefix", "sparse", 400, 8),
      ("genres", "sequence", 20, 8), ("release_year_bucket", "sparse", 16, 4),
      ("movie_age_at_rating", "sparse", 8, 4), ("num_genres", "sparse", 8, 4), ("dow_sin", "dense", 0, 4),
      ("dow_cos", "dense", 0, 4), ("hour_sin", "dense", 0, 4), ("hour_cos", "dense", 0, 4),
      ("user_rating_count", "dense", 0, 8), ("item_rating_count", "dense", 0, 8)]
FIELDS = [dict(name=n, type=t, vocab=v, dim=d, max_len=6 if t == "sequence" else 1, combiner="mean")
          for n, t, v, d in _S]


def build(kind):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = 16
    cfg.dnn.hidden_units, cfg.dnn.dropout = [256, 128, 64], 0.1
    if kind == "xdeepfm":
        cfg.cin.layer_sizes, cfg.cin.split_half = [64], True
    if kind == "attention_deepfm":
        cfg.attention.num_heads, cfg.attention.attention_dim = 4, 64
        cfg.attention.num_layers, cfg.attention.use_residual = 1, True
    torch.manual_seed(0)
    with torch.device("cuda"):
        return create_model(kind, schema_from_fields(FIELDS), cfg)


def event_us(fn, iters):
    for _ in range(3):
        fn(0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def records(model, n, rng):
    """n device records and the same batches as dicts."""
    from deepfm_amd.data.packed import PackedColumns, mixed_record_layout, write_mixed_record
    out, dicts = [], []
    size = mixed_record_layout(model.schema, B)[-1]
    for _ in range(n):
        hb = random_fields_batch(FIELDS, B, rng, zero_frac=0.05)
        cols = PackedColumns(model.schema, hb, (rng.random(B) < 0.25).astype(np.float32))
        rec = np.zeros(size, np.uint8)
        write_mixed_record(rec, cols, B, 0, B)
        out.append(torch.from_numpy(rec).cuda())
        dicts.append({k: torch.from_numpy(v).cuda() for k, v in hb.items()})
    return out, dicts


def split(rng):
    feats = random_fields_batch(FIELDS, U * C, rng, zero_frac=0.05)
    feats["user_id"] = np.repeat(np.arange(1, U + 1, dtype=np.int64), C)
    labels = np.zeros(U * C, np.float32)
    labels[np.arange(U) * C + rng.integers(0, C, U)] = 1.0
    return feats, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default=None)
    ap.add_argument("--trace", action="store_true", help="gather launches only (for a kernel trace)")
    args = ap.parse_args()
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import (MixedSchemaPredictor, compute_auc, compute_logloss,
                                     compute_ranking_metrics)
    rng = np.random.default_rng(0)
    kinds = [args.only] if args.only else ["deepfm", "xdeepfm", "attention_deepfm"]
    if args.trace:
        model = build("deepfm")
        model.eval()
        emb = model.embedding
        recs, dicts = records(model, 4, rng)
        T = model.schema.total_embedding_dim
        fo, fm, flat = torch.empty(B, 1, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, T, device="cuda")
        with torch.no_grad():
            for i in range(args.iters):
                emb.forward_record(recs[i % 4].data_ptr(), B, fo, None, flat.data_ptr(), T, fm)
                fo_g, fe_g, flat_g = emb(dicts[i % 4])
                model.fm(fe_g)
        torch.cuda.synchronize()
        print(json.dumps({"trace": "gather", "iters": args.iters}))
        return
    for kind in kinds:
        model = build(kind)
        recs, dicts = records(model, 8, rng)
        model.eval()
        with torch.no_grad():
            t_ref = event_us(lambda i: model.predict(dicts[i % 8]), args.iters)
        model.train()
        row = {"model": kind, "B": B, "model_predict_us": round(t_ref, 1)}
        for graph in (False, True):
            pred = MixedSchemaPredictor(model, B, use_graph=graph)
            t = event_us(lambda i: pred._launch(recs[i % 8].data_ptr(), B, pred.probs, pred.logits, pred.st_labels),
                         args.iters)
            row["mixed_graph_us" if graph else "mixed_eager_us"] = round(t, 1)
            del pred
        print(json.dumps(row), flush=True)
    # the 943 x 1000 evaluation split, DeepFM
    model = build("deepfm")
    feats, labels = split(rng)
    cols = PackedColumns(model.schema, feats, labels)
    ks = [1, 5, 10, 20]
    pred = MixedSchemaPredictor(model, B)
    pred.evaluate(cols, ranking_ks=ks)                  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = pred.evaluate(cols, ranking_ks=ks)
    t_new = time.perf_counter() - t0
    uid = torch.from_numpy(feats["user_id"]).cuda()
    lab = torch.from_numpy(labels).cuda()
    dev = {k: torch.from_numpy(v) for k, v in feats.items()}

    def loop():
        model.eval()
        out = []
        with torch.no_grad():
            for s in range(0, U * C, B):
                out.append(model.predict({k: v[s:s + B].cuda(non_blocking=True) for k, v in dev.items()}).view(-1))
        model.train()
        scores = torch.cat(out)
        r = {"auc": compute_auc(lab, scores), "logloss": compute_logloss(lab, scores)}
        r.update(compute_ranking_metrics(uid, lab, scores, ks, num_users=944))
        return r
    loop()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = loop()
    t_old = time.perf_counter() - t0
    print(json.dumps({"split": f"{U}x{C}", "B": B, "evaluate_s": round(t_new, 4), "predict_loop_s": round(t_old, 4),
                      "auc": m["auc"], "auc_loop": ref["auc"], "HR@10": m["HR@10"], "HR@10_loop": ref["HR@10"]}))


if __name__ == "__main__":
    main()
