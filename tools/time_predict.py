#!/usr/bin/env python3
"""Inference throughput: samples/s of a ``model.predict`` loop, ``FusedPredictor`` eager and ``FusedPredictor`` graph at
BASELINE.json's three shapes (26 x 10^6 + 13 fields, B = 4096: DeepFM D = 16; xDeepFM CIN [128]*3 D = 16;
AttentionDeepFM D = 32), timed with device events over back-to-back batches from device records; then
``evaluate()`` of ~1 M samples against ``model.predict`` + sklearn (wall clock, both ending on the host).
One JSON line per measurement.
usage: python tools/time_predict.py [--iters 50] [--eval-samples 1048576] [--only deepfm] [--graph-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepfm_amd.data.synthetic import criteo_fields, schema_from_fields  # noqa: E402

V, B, S, ND = 1_000_000, 4096, 26, 13
SHAPES = {"deepfm": 16, "xdeepfm": 16, "attention_deepfm": 32}


def build(kind):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    D = SHAPES[kind]
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = D
    if kind == "xdeepfm":
        cfg.cin.layer_sizes, cfg.cin.split_half = [128, 128, 128], True
    if kind == "attention_deepfm":
        cfg.attention.num_heads, cfg.attention.attention_dim = 4, 64
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = create_model(kind, schema_from_fields(criteo_fields(V, D)), cfg)
    model.embedding.pack_tables_()
    model.embedding.set_grad_mode("rowsparse")
    return model


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--eval-samples", type=int, default=1 << 20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--graph-only", action="store_true", help="the predictor graph only (for a kernel trace)")
    args = ap.parse_args()
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FusedPredictor, compute_auc, compute_logloss  # noqa: F401
    kinds = [args.only] if args.only else list(SHAPES)
    for kind in kinds:
        model = build(kind)
        model.eval()
        g = torch.Generator(device="cuda").manual_seed(1)
        nrec = 4
        ids = torch.randint(1, V, (nrec, S, B), generator=g, device="cuda", dtype=torch.int64)
        dense = torch.rand((nrec, ND, B), generator=g, device="cuda")
        batches = [{**{f"C{j + 1}": ids[r, j] for j in range(S)}, **{f"I{j + 1}": dense[r, j] for j in range(ND)}}
                   for r in range(nrec)]
        graph = FusedPredictor(model, B, use_graph=True)
        records = torch.cat([ids.view(nrec, -1).view(torch.uint8), dense.view(nrec, -1).view(torch.uint8),
                             torch.zeros(nrec, B * 4, dtype=torch.uint8, device="cuda")], 1).contiguous()
        res = {"kind": kind, "batch": B}
        res["graph_us"] = event_us(lambda i: graph._launch(records[i % nrec].data_ptr(), B, graph.probs, None,
                                                           graph.st_labels), args.iters)
        if not args.graph_only:
            eager = FusedPredictor(model, B, use_graph=False)
            res["eager_us"] = event_us(lambda i: eager._launch(records[i % nrec].data_ptr(), B, eager.probs, None,
                                                               eager.st_labels), args.iters)
            with torch.no_grad():
                res["model_predict_us"] = event_us(lambda i: model.predict(batches[i % nrec]), args.iters)
        for k in ("graph_us", "eager_us", "model_predict_us"):
            if k in res:
                res[k.replace("_us", "_samples_per_s")] = B / (res[k] * 1e-6)
        print(json.dumps(res), flush=True)
        if kind != "deepfm" or args.graph_only or args.eval_samples <= 0:
            del model, graph
            torch.cuda.empty_cache()
            continue
        # ---- evaluate() of ~1 M samples against model.predict + sklearn
        from sklearn.metrics import log_loss, roc_auc_score
        n = args.eval_samples
        rng = np.random.default_rng(0)
        feats = {f"C{j + 1}": rng.integers(1, V, n) for j in range(S)}
        feats.update({f"I{j + 1}": rng.random(n).astype(np.float32) for j in range(ND)})
        cols = PackedColumns(model.schema, feats, (rng.random(n) < 0.25).astype(np.float32))
        graph.evaluate(cols)                           # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = graph.evaluate(cols)
        t_eval = time.perf_counter() - t0
        t0 = time.perf_counter()
        scores = []
        with torch.no_grad():
            for s in range(0, n, B):
                e = min(n, s + B)
                batch = {k: torch.from_numpy(v[s:e]).cuda(non_blocking=True) for k, v in feats.items()}
                scores.append(model.predict(batch).squeeze(1).cpu().numpy())
        sc = np.concatenate(scores)
        ref = {"auc": roc_auc_score(cols.labels, sc), "logloss": log_loss(cols.labels, np.clip(sc, 1e-7, 1 - 1e-7))}
        t_ref = time.perf_counter() - t0
        print(json.dumps({"kind": "evaluate", "samples": n, "evaluate_s": t_eval, "evaluate_samples_per_s": n / t_eval,
                          "model_predict_sklearn_s": t_ref, "model_predict_sklearn_samples_per_s": n / t_ref,
                          "auc": m["auc"], "auc_ref": ref["auc"], "logloss": m["logloss"],
                          "logloss_ref": ref["logloss"]}), flush=True)
        del model, graph
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
