#!/usr/bin/env python3
"""Time one training step of DeepFM (default), xDeepFM or AttentionDeepFM (``--model``) on the MovieLens schema (the
reference's configs/deepfm_movielens.yaml model: tower [256, 128, 64], dropout 0.1; CIN and attention blocks at the
reference's defaults) at B = 4096, interleaved in one process, device events around blocks of steps:

  A  the dense autograd path: model(batch) + BCE + get_l2_reg_loss() + clip_grad_norm_ + torch.optim.Adam
  B  the model's fused mixed step (``mixed_step_class``), eager
  C  the same step as a HIP graph, G = 1 and G = 4 steps per graph

    python tools/time_train_mixed.py [--model deepfm|xdeepfm|attention_deepfm] [--steps 240] [--rounds 3] [--json out.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_train_mixed.py --profile      (kernel table: C only)

Prints ms per step (median over rounds, and the spread), the ratio A / C and the embedding backward's traffic floor.
Needs the GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B = 4096


def movielens_fields():
    sp = [("user_id", 944, 16), ("movie_id", 1683, 16), ("gender", 3, 4), ("age", 8, 4), ("occupation", 22, 8),
          ("zip_prefix", 400, 8)]
    fs = [dict(name=n, type="sparse", vocab=v, dim=d, max_len=1, combiner="mean") for n, v, d in sp]
    fs.append(dict(name="genres", type="sequence", vocab=20, dim=8, max_len=6, combiner="mean"))
    for n, v in (("release_year_bucket", 16), ("movie_age_at_rating", 8), ("num_genres", 8)):
        fs.append(dict(name=n, type="sparse", vocab=v, dim=4, max_len=1, combiner="mean"))
    for n in ("dow_sin", "dow_cos", "hour_sin", "hour_cos"):
        fs.append(dict(name=n, type="dense", vocab=0, dim=4, max_len=1, combiner="mean"))
    for n in ("user_rating_count", "item_rating_count"):
        fs.append(dict(name=n, type="dense", vocab=0, dim=8, max_len=1, combiner="mean"))
    return fs


def make_model(fields, seed=0, kind="deepfm"):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.synthetic import schema_from_fields
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = 16
    cfg.feature.embedding_l2_reg = 1e-5
    cfg.dnn.hidden_units = [256, 128, 64]
    cfg.dnn.dropout = 0.1
    torch.manual_seed(seed)
    return create_model(kind, schema_from_fields(fields), cfg).cuda().train()


def timed(fn, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn(steps)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--model", default="deepfm", choices=["deepfm", "xdeepfm", "attention_deepfm"])
    ap.add_argument("--profile", action="store_true", help="graph variant only, 50 steps (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_train_mixed.py needs the GPU (no fallback)")
    from deepfm_amd.data.synthetic import random_fields_batch
    from deepfm_amd.training import DenseTableAdam, mixed_step_class, mixed_step_ineligible_reason
    fields = movielens_fields()
    rng = np.random.default_rng(0)
    batches = [(random_fields_batch(fields, B, rng, zero_frac=0.05), (rng.random(B) < 0.3).astype(np.float32))
               for _ in range(8)]
    dev = [({k: torch.from_numpy(v).cuda() for k, v in b.items()}, torch.from_numpy(l).cuda()) for b, l in batches]

    variants = {}
    if not args.profile:
        ref = make_model(fields, kind=args.model)
        topt = torch.optim.Adam(ref.parameters(), lr=1e-3)

        def run_a(n):
            for i in range(n):
                b, lab = dev[i % len(dev)]
                loss = torch.nn.functional.binary_cross_entropy_with_logits(ref(b).squeeze(1), lab) + ref.get_l2_reg_loss()
                topt.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
                topt.step()
        variants["A dense autograd + torch Adam"] = run_a

    def fused(use_graph, G):
        model = make_model(fields, kind=args.model)
        cls = mixed_step_class(model)
        if cls is None:
            raise SystemExit(mixed_step_ineligible_reason(model, B))
        opt = DenseTableAdam(model, lr=1e-3, l2=1e-5, max_grad_norm=1.0)
        step = cls(model, opt, B, use_graph=use_graph)
        recs = [step.pack_record(b, lab) for b, lab in dev]
        if use_graph:
            step.capture(steps_per_graph=G)

        def run(n):
            for i in range(0, n, G):
                if G == 1:
                    step.run_from(recs[i % len(recs)])
                else:
                    step.run_group([recs[(i + k) % len(recs)] for k in range(G)])
        return run, step

    keep = []
    for name, (g, G) in {"B fused eager": (False, 1), "C fused graph G=1": (True, 1), "C fused graph G=4": (True, 4)}.items():
        if args.profile and name != "C fused graph G=1":
            continue
        run, step = fused(g, G)
        keep.append(step)
        variants[name] = run
    steps = 48 if args.profile else args.steps // 4 * 4
    for fn in variants.values():            # warm every variant
        fn(16)
    torch.cuda.synchronize()
    if args.profile:
        variants["C fused graph G=1"](steps)
        torch.cuda.synchronize()
        return
    times = {k: [] for k in variants}
    for _ in range(args.rounds):            # interleaved: A B C C A B C C ...
        for k, fn in variants.items():
            times[k].append(timed(fn, steps))
    F, T = len(fields), sum(f["dim"] for f in fields)
    rec_bytes = keep[0].packed_bytes
    floor_bytes = rec_bytes + 4 * (2 * B * T + B * F * 16 + B) + 4 * keep[0].opt.n_l2 * keep[0]._dense_parts
    out = {"model": args.model, "step": type(keep[0]).__name__, "batch": B, "steps": steps, "rounds": args.rounds,
           "ms_per_step": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()},
           "embedding_backward_bytes": int(floor_bytes),
           "embedding_backward_floor_us_at_8TBs": floor_bytes / 8e12 * 1e6}
    a = out["ms_per_step"]["A dense autograd + torch Adam"]["median"]
    for k in variants:
        if k.startswith("C"):
            out.setdefault("ratio_A_over", {})[k] = a / out["ms_per_step"][k]["median"]
    print(json.dumps(out, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    if not all(out["ms_per_step"][k]["median"] < a for k in variants if k.startswith("C")):
        raise SystemExit("the graph-captured fused step is not faster than the dense autograd path")


if __name__ == "__main__":
    main()
