#!/usr/bin/env python3
"""Row-wise quantised tables (``training/quantized.py``, csrc/quant.hip; ``--format int8`` or ``uint4``) against the
fp32 path, and with ``--format uint4`` against the int8 tables as well, all of the same checkout and the same run, at
BASELINE.json's shapes (26 x 10^6 + 13 fields, B = 4096: DeepFM D = 16; xDeepFM CIN [128]*3 D = 16; AttentionDeepFM
D = 32), with uniform ids and with Zipf ids (log-uniform rank, exponent 1: a head that stays in cache):
  * the gather alone: ``dfm_embedding_forward_quant`` against ``dfm_embedding_forward_staged``, as the predictors
    launch them, 16 launches over different records captured into one graph and replayed (device events; no host time);
  * ``QuantizedPredictor.predict_from`` against ``FusedPredictor.predict_from`` (graph mode, the launch alone as
    tools/time_predict.py times it), alternating the two;
  * the quantise pass (``QuantizedTables.refresh`` over all 26 tables, without its host read of the flags);
  * bytes per id and per model.
Medians and ranges over ``--reps`` repetitions; one JSON line per case.
``--quality``: DeepFM on the learnable synthetic task (tools_shared_auc.py) after the 4 epochs of
tests/test_gpu_auc_parity.py: AUC and log loss of the test split through both predictors, and the largest |d logit|.
The keys of the JSON lines carry the format's name.
usage: python tools/time_quant_predict.py [--format int8] [--reps 15] [--iters 50] [--only deepfm] [--quality]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.time_predict import B, ND, S, SHAPES, V, build  # noqa: E402

GATHERS_PER_GRAPH = 16


def stats(xs, digits=2):
    xs = np.asarray(xs, dtype=np.float64)
    return dict(median=round(float(np.median(xs)), digits), min=round(float(xs.min()), digits),
                max=round(float(xs.max()), digits))


def events_us(fn, calls=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def make_records(dist, nrec, gen):
    if dist == "uniform":
        ids = torch.randint(1, V, (nrec, S, B), generator=gen, device="cuda", dtype=torch.int64)
    else:       # rank = V^u, u uniform: P(rank <= r) = log r / log V, the density of Zipf with exponent 1
        u = torch.rand((nrec, S, B), generator=gen, device="cuda", dtype=torch.float64)
        ids = torch.exp(u * float(np.log(V))).long().clamp_(1, V - 1)
    dense = torch.rand((nrec, ND, B), generator=gen, device="cuda")
    return torch.cat([ids.view(nrec, -1).view(torch.uint8), dense.view(nrec, -1).view(torch.uint8),
                      torch.zeros(nrec, B * 4, dtype=torch.uint8, device="cuda")], 1).contiguous()


def gather_graph(pred, records):
    """One graph of GATHERS_PER_GRAPH gather launches of ``pred`` over ``records`` in turn."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pred._gather(records[0].data_ptr(), pred.st_labels)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for i in range(GATHERS_PER_GRAPH):
            pred._gather(records[i % len(records)].data_ptr(), pred.st_labels)
    return g


def speed(kind, reps, iters, fmt):
    from deepfm_amd.training import FusedPredictor, QuantizedPredictor, QuantizedTables
    model = build(kind)
    model.eval()
    D = SHAPES[kind]
    fp32 = FusedPredictor(model, B, use_graph=True)
    # the format under test last, so that `tables` and `quant` below are its; int8 stays the second comparator
    preds = {"fp32": fp32}
    for f in dict.fromkeys(["int8", fmt]):
        tables = QuantizedTables.from_model(model, fmt=f)
        preds[f] = quant = QuantizedPredictor(model, B, tables=tables, use_graph=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for dist in ("uniform", "zipf"):
        records = make_records(dist, 4, gen)
        res = dict(case="speed", kind=kind, D=D, batch=B, ids=dist, reps=reps)
        if kind == "deepfm":        # the gather does not depend on the model around it
            graphs = {k: gather_graph(p, records) for k, p in preds.items()}
            times = {k: [] for k in graphs}
            for g in graphs.values():
                g.replay()
            for _ in range(reps):                        # alternating: the same neighbours for both
                for k, g in graphs.items():
                    times[k].append(events_us(g.replay, GATHERS_PER_GRAPH))
            res.update({f"gather_{k}_us": stats(t) for k, t in times.items()})
        times = {k: [] for k in preds}

        def run(p):
            for i in range(iters):
                p._launch(records[i % 4].data_ptr(), B, p.probs, None, p.st_labels)
        for p in preds.values():
            run(p)
        for _ in range(reps):
            for k, p in preds.items():
                times[k].append(events_us(lambda: run(p), iters))
        res.update({f"predict_{k}_us": stats(t) for k, t in times.items()})
        print(json.dumps(res), flush=True)
    if kind == "deepfm":
        tables.refresh(check=False)
        t = [events_us(lambda: tables.refresh(check=False)) for _ in range(reps)]
        rows = sum(tables.vocab.values())
        print(json.dumps(dict(case="quantize", format=fmt, tables=len(tables.vocab), rows=rows, D=D,
                              layout="packed row records",
                              refresh_ms=stats(np.asarray(t) / 1e3, 3),
                              bytes_moved=rows * (4 * D + 4 + tables.row_bytes))), flush=True)
    sizes = {}
    for k, p in preds.items():
        if k != "fp32":
            sizes[f"{k}_bytes_per_id"], sizes[f"{k}_table_bytes"] = p.tables.row_bytes, p.tables.nbytes
    print(json.dumps(dict(case="bytes", kind=kind, D=D, **sizes,
                          fp32_bytes_per_id=4 * D + 4, fp32_table_bytes=tables.fp32_nbytes,
                          packed_training_bytes=sum(b["buffer"].numel() * 4 for b in model.embedding.packed.values()),
                          ratio=round(tables.fp32_nbytes / tables.nbytes, 3))), flush=True)


def quality(fmt):
    import tools_shared_auc as T
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.synthetic import criteo_fields, schema_from_fields
    from deepfm_amd.models import create_model
    from deepfm_amd.training import FusedPredictor, QuantizedPredictor
    from deepfm_amd.training.fused_step import FusedDeepFMStep
    from deepfm_amd.training.rowsparse import RowSparseAdam
    ids, dense, labels = T.make_task()
    cfg = ExperimentConfig()
    torch.manual_seed(0)
    model = create_model("deepfm", schema_from_fields(criteo_fields(T.VOCAB, T.DIM)), cfg).cuda().train()
    model.embedding.pack_tables_()
    model.embedding.set_grad_mode("rowsparse")
    opt = RowSparseAdam(model, lr=cfg.training.lr, l2=cfg.feature.embedding_l2_reg,
                        max_grad_norm=cfg.training.gradient_clip_norm)
    step = FusedDeepFMStep(model, opt, T.BATCH, use_graph=True)
    d_ids = torch.from_numpy(ids).cuda().t().contiguous()
    d_dense = torch.from_numpy(dense).cuda().t().contiguous()
    d_labels = torch.from_numpy(labels).cuda()
    step.load_batch(d_ids[:, :T.BATCH], d_dense[:, :T.BATCH], d_labels[:T.BATCH])
    step.capture()
    for epoch in range(T.EPOCHS):
        order = torch.from_numpy(T.epoch_order(epoch)).cuda()
        for k in range(T.N_TRAIN // T.BATCH):
            idx = order[k * T.BATCH:(k + 1) * T.BATCH]
            step.load_batch(d_ids[:, idx], d_dense[:, idx], d_labels[idx])
            step.run()
    torch.cuda.synchronize()
    test = slice(T.N_TRAIN, T.N_TRAIN + T.N_TEST)
    feats = {f"C{j + 1}": ids[test, j] for j in range(T.N_SPARSE)}
    feats.update({f"I{j + 1}": dense[test, j] for j in range(T.N_DENSE)})
    cols = PackedColumns(model.schema, feats, labels[test])
    fp32 = FusedPredictor(model, T.BATCH)
    quants = {f: QuantizedPredictor(model, T.BATCH, fmt=f) for f in dict.fromkeys(["int8", fmt])}
    m32 = fp32.evaluate(cols)
    res = dict(case="quality", task="tools_shared_auc", epochs=T.EPOCHS, test_samples=T.N_TEST,
               auc_fp32=m32["auc"], logloss_fp32=m32["logloss"])
    rec = np.zeros(fp32.record_bytes, np.uint8)
    for f, quant in quants.items():
        mq = quant.evaluate(cols)
        worst = 0.0
        for s in range(0, T.N_TEST, T.BATCH):
            fp32.layout.write(rec, cols, s, s + T.BATCH)
            d_rec = torch.from_numpy(rec).cuda()
            fp32.predict_from(d_rec)
            quant.predict_from(d_rec)
            worst = max(worst, float((fp32.last_logits() - quant.last_logits()).abs().max()))
        res.update({f"auc_{f}": mq["auc"], f"logloss_{f}": mq["logloss"], f"max_abs_dlogit_{f}": worst,
                    f"table_error_bound_{f}": max(quant.tables.error_bound().values())})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default=None, choices=list(SHAPES))
    ap.add_argument("--format", default="int8", choices=["int8", "uint4"],
                    help="the quantised format under test; uint4 is timed beside int8")
    ap.add_argument("--quality", action="store_true", help="the accuracy comparison only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_quant_predict.py measures on the device: no GPU found")
    if args.quality:
        quality(args.format)
        return
    for kind in ([args.only] if args.only else list(SHAPES)):
        speed(kind, args.reps, args.iters, args.format)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
