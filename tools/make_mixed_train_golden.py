#!/usr/bin/env python3
"""Generate tests/golden/train_steps_deepfm_movielens{,_l2clip}.npz: three reference training steps on the
MovieLens schema, for the fused mixed-schema step (``training/mixed_step.py``).

Runs on the CPU where the reference implementation is installed (see tools/make_golden.py, whose loaders, schema
and composite model this tool imports: the reference's layer classes by file path, DeepFM composed per
deepfm.py:30-42).  Each step is the body of ``Trainer._train_epoch`` (trainer.py:212-240): BCEWithLogits +
``lambda * sum ||p||^2`` over ``embedding.parameters()``, ``clip_grad_norm_``, ``torch.optim.Adam``; dropout 0, B = 64.

What these vectors pin that the Criteo ones cannot: DENSE Adam.  Ids are drawn from the lower part of every
vocabulary, so the upper rows of EVERY table are named by no sample of any step; the reference still moves them
(L2 gradient 2 lambda w, then stale moments).  The tool checks that every table has such rows and that the reference
moves them by more than the tests' bar of 1e-3 * lr.  Some bags are short or empty, some ids are 0.

The schema is make_golden.movielens_fields() with the vocabularies of user_id and movie_id cut to 96 and 128: 64
samples cannot name more rows anyway, and the full tables would put each file (initial state, three steps of
gradients and parameters, final moments) over the repository's 1 MiB limit.  Keys follow train_steps_*.npz
(``adam_param_bound`` of tests/test_oracle_golden.py reads them) plus ``untouched/<table>``: the row mask.
Fixtures are data only.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as G  # noqa: E402

B, STEPS, HIDDEN = 64, 3, [32, 32]
SMALL = {"user_id": 96, "movie_id": 128}


def fields():
    fs = G.movielens_fields()
    for f in fs:
        if f["name"] in SMALL:
            f["vocab"] = SMALL[f["name"]]
    return fs


def draw_batch(fs, rng):
    """Ids from rows [1, hi) with hi = max(2, 0.6 V): rows >= hi are never named."""
    batch = {}
    for f in fs:
        if f["type"] == "dense":
            batch[f["name"]] = rng.random(B).astype(np.float32) * 2 - 1
            continue
        hi = max(2, int(0.6 * f["vocab"]))
        if f["type"] == "sparse":
            x = rng.integers(1, hi, size=B, dtype=np.int64)
            x[rng.random(B) < 0.1] = 0
        else:
            L = f["max_len"]
            x = rng.integers(1, hi, size=(B, L), dtype=np.int64)
            lens = rng.integers(0, L + 1, size=B)
            for b in range(B):
                x[b, lens[b]:] = 0
            x[0, :] = 0                         # an empty bag
            x[2, :] = x[2, 0]                   # one id repeated inside a bag
        batch[f["name"]] = x
    return batch


def case(name, seed, lr, l2, clip):
    fs = fields()
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = G._RefComposite("deepfm", G.to_schema(fs), 16, HIDDEN)
    G.randomize_(model, rng, scale=0.25)
    model.train()
    criterion = nn.BCEWithLogitsLoss()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    cfg = dict(kind="deepfm", fm_dim=16, hidden_units=HIDDEN)
    arrays = dict(fields=G.fields_meta(fs), cfg=np.array(json.dumps(cfg)), steps=np.int64(STEPS), lr=np.float64(lr),
                  l2=np.float64(l2), clip=np.float64(clip))
    arrays.update(G.sd_np(model, "init/"))
    named = {f["name"]: np.zeros(f["vocab"], bool) for f in fs if f["type"] != "dense"}
    for t in range(STEPS):
        batch = draw_batch(fs, rng)
        for k, hit in named.items():
            hit[np.unique(batch[k])] = True
        labels = (rng.random(B) < 0.3).astype(np.float32)
        logits = model(G.tb(batch)).squeeze(1)
        bce = criterion(logits, torch.from_numpy(labels))
        l2_loss = torch.tensor(0.0)
        for p in model.embedding.parameters():
            l2_loss = l2_loss + p.norm(2).pow(2)
        l2_term = l2 * l2_loss
        loss = bce + l2_term
        opt.zero_grad()
        loss.backward()
        arrays.update(G.grads_np(model, f"step{t}/grad/"))          # before clipping
        total_norm = nn.utils.clip_grad_norm_(model.parameters(), clip)
        opt.step()
        arrays.update({f"step{t}/batch/" + k: v for k, v in batch.items()})
        arrays[f"step{t}/labels"] = labels
        arrays[f"step{t}/logits"] = logits.detach().numpy().copy()
        arrays[f"step{t}/bce"] = np.float32(bce.item())
        arrays[f"step{t}/l2_term"] = np.float32(l2_term.item())
        arrays[f"step{t}/loss"] = np.float32(loss.item())
        arrays[f"step{t}/grad_norm"] = np.float32(float(total_norm))
        arrays.update(G.sd_np(model, f"step{t}/param/"))
    for i, (k, _) in enumerate(model.named_parameters()):
        st = opt.state_dict()["state"][i]
        arrays["adam_m/" + k] = st["exp_avg"].numpy().copy()
        arrays["adam_v/" + k] = st["exp_avg_sq"].numpy().copy()
    # every table has rows no sample named (row 0, the zero padding row, does not count), and the reference moves
    # them by more than the tests' bar on them
    for k, hit in named.items():
        free = ~hit
        free[0] = False
        assert free.any(), f"{name}: every row of {k} was named"
        arrays["untouched/" + k] = free
        for order in ("second", "first"):
            key = f"embedding.{order}_order_embeddings.{k}.weight"
            moved = np.abs(arrays[f"step{STEPS - 1}/param/" + key] - arrays["init/" + key])[free]
            assert moved.min() > 1e-3 * lr, f"{name}: {key}: an untouched row moved {moved.min():.2e} <= {1e-3 * lr:.1e}"
    G.save(name, **arrays)
    size = os.path.getsize(os.path.join(G.OUT, name + ".npz"))
    assert size < 900 * 1024, f"{name}: {size} bytes"


def main():
    case("train_steps_deepfm_movielens", 811, lr=1e-3, l2=1e-5, clip=1.0)              # reference defaults
    case("train_steps_deepfm_movielens_l2clip", 812, lr=1e-2, l2=1e-2, clip=0.25)      # L2 and the clip bite


if __name__ == "__main__":
    main()
