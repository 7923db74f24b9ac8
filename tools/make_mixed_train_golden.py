#!/usr/bin/env python3
"""Generate tests/golden/train_steps_{deepfm,xdeepfm,attention_deepfm}_movielens{,_l2clip}.npz: three reference
training steps on the MovieLens schema, for the fused mixed-schema steps (``training/mixed_step.py``).

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

xDeepFM and AttentionDeepFM cases (same schema, batch draw, masks and keys) are additionally checked for ReLU kinks:
in every step, the smallest |pre-activation| of every tower layer (the BatchNorm output in front of the ReLU) and of
every CIN layer (the convolution's output) must be at least 1e-5 of that layer's largest |pre-activation|.  A unit
closer to 0 than that can fall on the other side of the kink under another summation order (DESIGN.md section 2
records a flipped column at that distance) and would spend the tests' outlier allowance on the reference's side.  A
case that fails the check (or whose untouched rows the reference moves by less than the tests' bar) is drawn again
from the next seed; the seed used is stored under ``seed``.  The
AttentionDeepFM cases keep their ``step<t>/grad/`` keys in ``<name>_grads.npz`` (every file stays under 900 KiB).
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


KINK = 1e-5         # smallest |pre-activation| allowed, as a fraction of the layer's largest


class Kink(Exception):
    """This draw cannot serve as a fixture (a unit on a ReLU kink, an untouched row the reference barely moves)."""


def watch_preactivations(model):
    """Forward hooks that collect, per call, (layer name, min |pre-activation|, max |pre-activation|) of every tower
    ReLU's input and every CIN convolution's output (cin.py applies torch.relu to it)."""
    seen = []
    for i, m in enumerate(model.dnn.mlp):
        if isinstance(m, nn.ReLU):
            m.register_forward_hook(lambda _m, inp, _out, i=i: seen.append(
                (f"dnn.mlp.{i}", float(inp[0].abs().min()), float(inp[0].abs().max()))))
    if hasattr(model, "cin"):
        for i, conv in enumerate(model.cin.conv_layers):
            conv.register_forward_hook(lambda _m, _inp, out, i=i: seen.append(
                (f"cin.conv_layers.{i}", float(out.abs().min()), float(out.abs().max()))))
    return seen


def case(name, seed, lr, l2, clip, kind="deepfm", **kw):
    if kind == "deepfm":                 # the original pair, byte for byte
        return _case(name, seed, lr, l2, clip, kind, **kw)
    while True:
        try:
            return _case(name, seed, lr, l2, clip, kind, **kw)
        except Kink as e:
            print(f"{name}: seed {seed}: {e}; next seed")
            seed += 1


def _case(name, seed, lr, l2, clip, kind, **kw):
    fs = fields()
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = G._RefComposite(kind, G.to_schema(fs), 16, HIDDEN, **kw)
    G.randomize_(model, rng, scale=0.25)
    model.train()
    criterion = nn.BCEWithLogitsLoss()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    cfg = dict(kind=kind, fm_dim=16, hidden_units=HIDDEN, **kw)
    arrays = dict(fields=G.fields_meta(fs), cfg=np.array(json.dumps(cfg)), steps=np.int64(STEPS), lr=np.float64(lr),
                  l2=np.float64(l2), clip=np.float64(clip))
    seen = []
    if kind != "deepfm":
        arrays["seed"] = np.int64(seed)
        seen = watch_preactivations(model)
    arrays.update(G.sd_np(model, "init/"))
    named = {f["name"]: np.zeros(f["vocab"], bool) for f in fs if f["type"] != "dense"}
    for t in range(STEPS):
        batch = draw_batch(fs, rng)
        for k, hit in named.items():
            hit[np.unique(batch[k])] = True
        labels = (rng.random(B) < 0.3).astype(np.float32)
        logits = model(G.tb(batch)).squeeze(1)
        for layer, lo, hi in seen:
            if lo < KINK * hi:
                raise Kink(f"step {t} {layer}: min |pre-activation| {lo:.3e} < {KINK:g} x {hi:.3e}")
        seen.clear()
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
            if kind != "deepfm" and moved.min() <= 1e-3 * lr:        # a draw property as well: the next seed
                raise Kink(f"{key}: an untouched row moved {moved.min():.2e} <= {1e-3 * lr:.1e}")
            assert moved.min() > 1e-3 * lr, f"{name}: {key}: an untouched row moved {moved.min():.2e} <= {1e-3 * lr:.1e}"
    files = {name: arrays}
    if kind == "attention_deepfm":
        # the tower's first Linear reads F D + T = 364 columns: nine copies of it (initial state, three steps of
        # gradients and parameters, two moments) put one file over the limit, so the ``step<t>/grad/`` keys go to
        # a sibling file ``<name>_grads.npz`` under the same keys; a reader merges the two
        grads = {k: v for k, v in arrays.items() if "/grad/" in k}
        files = {name: {k: v for k, v in arrays.items() if k not in grads}, name + "_grads": grads}
    for fname, content in files.items():
        G.save(fname, **content)
        size = os.path.getsize(os.path.join(G.OUT, fname + ".npz"))
        assert size < 900 * 1024, f"{fname}: {size} bytes"


def main():
    case("train_steps_deepfm_movielens", 811, lr=1e-3, l2=1e-5, clip=1.0)              # reference defaults
    case("train_steps_deepfm_movielens_l2clip", 812, lr=1e-2, l2=1e-2, clip=0.25)      # L2 and the clip bite
    case("train_steps_xdeepfm_movielens", 813, lr=1e-3, l2=1e-5, clip=1.0, kind="xdeepfm",
         cin_sizes=[16, 16, 8], cin_split=True)
    case("train_steps_xdeepfm_movielens_l2clip", 814, lr=1e-2, l2=1e-2, clip=0.25, kind="xdeepfm",
         cin_sizes=[24, 12], cin_split=True)
    case("train_steps_attention_deepfm_movielens", 815, lr=1e-3, l2=1e-5, clip=1.0, kind="attention_deepfm",
         heads=4, A=64, layers=1, residual=True)
    case("train_steps_attention_deepfm_movielens_l2clip", 816, lr=1e-2, l2=1e-2, clip=0.25, kind="attention_deepfm",
         heads=4, A=64, layers=2, residual=True)


if __name__ == "__main__":
    main()
