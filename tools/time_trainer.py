#!/usr/bin/env python3
"""Time what ``Trainer._train_epoch`` adds to the device epoch, at the shape of DESIGN.md §7b (943 users, 1 682 items,
P = 90 000 positives, K = 4, B = 4096: 109 whole batches and a trailing batch of 3 536 rows; the MovieLens schema,
``FusedMixedDeepFMStep`` as a graph, Adam, tower [256, 128, 64]), in one process:

  b  loop (b) of tools/time_device_epoch.py as it was before the Trainer: ``set_epoch`` and ``run_from`` over the
     loader's whole batches, no loss tracking, the trailing batch dropped;
  t  ``Trainer._train_epoch``: the same, plus the loss accumulator launch in every step, the trailing batch through
     the tail step, and the one host read of the mean loss;
  the tail step alone and ``dfm_loss_accumulate`` alone, by device events around a block of launches.

One warm-up epoch of each, then ``--epochs`` timed ones, b and t alternating, synchronised at epoch end only; prints
median and min-max as one JSON object.  The yardstick is b's own spread.  Needs the GPU: there is no fallback.

    python tools/time_trainer.py [--epochs 5] [--json out.json]

``--uniform``: the same question for the uniform, row-sparse family at the headline shape (26 tables of ``--vocab`` rows,
13 DENSE fields, packed tables, ``FusedDeepFMStep``, 100 batches of 4096 and a trailing batch of 1000 rows):

  t  ``Trainer._train_epoch`` with ``steps_per_graph`` = 4;
  a  the same groups of 4 without the tail step and without tracking;
  g  ``Trainer._train_epoch`` with ``steps_per_graph`` = 1;
  the tail step alone, the three tracking launches alone (two ``dfm_rows_sqnorm`` and ``dfm_loss_accumulate_tables``
  against ``dfm_loss_accumulate``) and the per-epoch ``dfm_tables_sqnorm`` (``reset_loss``), by device events.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_device_epoch import B, K, P, dataset, stats  # noqa: E402


def uniform(args):
    """The ``--uniform`` mode (see the module text)."""
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.data.synthetic import criteo_fields, schema_from_fields
    from deepfm_amd.models import create_model
    from deepfm_amd.training import RowSparseAdam, Trainer
    from deepfm_amd.training.fused_step import FusedDeepFMStep
    dev, Bu, G = torch.device("cuda"), 4096, 4
    rows = 100 * Bu + 1000
    fields = criteo_fields(args.vocab, 16)
    schema = schema_from_fields(fields)
    rng = np.random.default_rng(0)
    feats = {f["name"]: (rng.integers(1, f["vocab"], rows, dtype=np.int64) if f["type"] == "sparse"
                         else rng.random(rows).astype(np.float32)) for f in fields}
    labels = (rng.random(rows) < 0.25).astype(np.float32)
    dcols = DeviceColumns(PackedColumns(schema, feats, labels), dev)
    small = PackedColumns(schema, {k: v[:Bu] for k, v in feats.items()}, labels[:Bu])

    def model():
        cfg = ExperimentConfig()
        cfg.training.batch_size, cfg.training.scheduler = Bu, "none"
        torch.manual_seed(0)
        with torch.device(dev):
            m = create_model("deepfm", schema, cfg)
        m.train()
        m.embedding.pack_tables_()
        m.embedding.set_grad_mode("rowsparse")
        return m, cfg

    def loader(depth):
        return DeviceEpochLoader(dcols, Bu, shuffle=True, seed=0, depth=depth)

    trainers = {}
    with tempfile.TemporaryDirectory() as tmp:
        for key, g in (("t", G), ("g", 1)):
            m, cfg = model()
            cfg.output_dir = tmp
            trainers[key] = Trainer(m, schema, cfg, loader(g + 2), small, small, steps_per_graph=g)
    m_a, cfg_a = model()
    opt_a = RowSparseAdam(m_a, lr=cfg_a.training.lr, l2=cfg_a.feature.embedding_l2_reg,
                          max_grad_norm=cfg_a.training.gradient_clip_norm)
    step_a = FusedDeepFMStep(m_a, opt_a, Bu)
    step_a.capture(timed_variant=True, steps_per_graph=G)
    loader_a = loader(G + 2)

    def epoch_a(e):
        loader_a.set_epoch(e - 1)
        for first in range(0, len(loader_a), G):
            step_a.run_group([loader_a.record(first + k) for k in range(G)])

    def wall(fn, e):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(e)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    fns = {"a": epoch_a, "t": trainers["t"]._train_epoch, "g": trainers["g"]._train_epoch}
    times = {k: [] for k in fns}
    for k, fn in fns.items():
        wall(fn, 1)
    for e in range(2, args.epochs + 2):
        for k, fn in fns.items():
            times[k].append(wall(fn, e))
    tr = trainers["g"]
    step, tail_step, opt = tr.step, tr.tail_step, tr.optimizer
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def events(fn, n):
        start.record()
        for _ in range(n):
            fn()
        stop.record(); stop.synchronize()
        return start.elapsed_time(stop) / n * 1e3

    rec, main_rec = tr.train_ds.tail(), tr.train_ds.record(0)
    lib, st = _lib_and_stream()
    S, old, new, _ = step._table_sq
    tabs = opt._table_struct()

    def tracking_launches():
        opt._rows_sqnorm(tabs, old)
        opt._rows_sqnorm(tabs, new)
        lib.dfm_loss_accumulate_tables(step.loss.data_ptr(), opt.l2, opt.flat_param.data_ptr(), opt.n_l2, S.data_ptr(),
                                       old.data_ptr(), new.data_ptr(), old.numel(), step._loss_acc.data_ptr(), st())

    t_tail, t_main, t_plain, t_track, t_reset = [], [], [], [], []
    for _ in range(args.epochs + 1):
        t_tail.append(events(lambda: tail_step.run_from(rec), 50))
        t_main.append(events(lambda: step.run_from(main_rec), 50))
        t_plain.append(events(lambda: step_a.run_from(main_rec, eager_gather=True), 50))
        t_track.append(events(tracking_launches, 100))
        t_reset.append(events(step.reset_loss, 5))
    n_tab = sum(t.numel() for t in opt._tables)
    out = {"device": torch.cuda.get_device_properties(0).name, "mode": "uniform", "vocab": args.vocab, "batch": Bu,
           "whole_batches": len(loader_a), "tail_rows": tr.train_ds.tail_rows, "table_floats": n_tab,
           "epochs": args.epochs, "t_trainer_G4_epoch_ms": stats(times["t"]), "a_groups_only_epoch_ms": stats(times["a"]),
           "g_trainer_G1_epoch_ms": stats(times["g"]), "tail_step_us": stats(t_tail[1:]),
           "tracked_main_step_G1_us": stats(t_main[1:]), "untracked_eager_gather_step_us": stats(t_plain[1:]),
           "three_tracking_launches_eager_us": stats(t_track[1:]), "reset_loss_tables_sqnorm_us": stats(t_reset[1:])}
    out["t_minus_a_ms"] = out["t_trainer_G4_epoch_ms"]["median"] - out["a_groups_only_epoch_ms"]["median"]
    out["a_spread_ms"] = out["a_groups_only_epoch_ms"]["max"] - out["a_groups_only_epoch_ms"]["min"]
    print(json.dumps(out, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def _lib_and_stream():
    from deepfm_amd import _lib
    return _lib.load(), _lib.stream_handle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--uniform", action="store_true", help="the uniform, row-sparse family at the headline shape")
    ap.add_argument("--vocab", type=int, default=1_000_000, help="--uniform: rows per table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_trainer.py needs the GPU (no fallback)")
    if args.uniform:
        return uniform(args)
    from deepfm_amd import _lib
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, NegativeSampler
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import DenseTableAdam, FusedMixedDeepFMStep, Trainer
    from time_train_mixed import make_model
    dev = torch.device("cuda")
    fields, schema, cols, user_of, table, derived, seen = dataset(np.random.default_rng(0))
    dcols = DeviceColumns(cols, dev)

    def loader():
        sampler = NegativeSampler(dcols, seen, user_of, table, K, derived=derived, seed=0)
        return DeviceEpochLoader(dcols, B, shuffle=True, seed=0, negatives=sampler, depth=4)

    # b: the loop as it was
    model_b = make_model(fields)
    opt_b = DenseTableAdam(model_b, lr=1e-3, l2=1e-5, max_grad_norm=1.0)
    step_b = FusedMixedDeepFMStep(model_b, opt_b, B, use_graph=True)
    step_b.capture()
    loader_b = loader()

    def epoch_b(e):
        loader_b.set_epoch(e - 1)
        for rec in loader_b:
            step_b.run_from(rec)

    # t: the Trainer (Adam, lr 1e-3, l2 1e-5, clip 1.0 are the configuration's defaults)
    model_t = make_model(fields)
    cfg = model_t.config
    cfg.training.batch_size, cfg.training.scheduler = B, "none"
    small = PackedColumns(schema, {n: c[:B] for n, c in zip(schema.fields, _host_columns(cols))}, cols.labels[:B])
    with tempfile.TemporaryDirectory() as tmp:
        cfg.output_dir = tmp
        trainer = Trainer(model_t, schema, cfg, loader(), small, small)
    assert len(trainer.train_ds) == len(loader_b) == P * (1 + K) // B and trainer.train_ds.tail_rows == P * (1 + K) % B
    losses = []

    def epoch_t(e):
        losses.append(trainer._train_epoch(e))

    def wall(fn, e):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(e)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    wall(epoch_b, 1); wall(epoch_t, 1)                    # the warm-up epoch of each
    tb, tt = [], []
    for e in range(2, args.epochs + 2):
        tb.append(wall(epoch_b, e))
        tt.append(wall(epoch_t, e))
    model_b.embedding.raise_on_bad_index()
    # the two additions alone, by events
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tail_step, step, opt = trainer.tail_step, trainer.step, trainer.optimizer
    rec = trainer.train_ds.tail()
    t_tail, t_acc, t_main = [], [], []
    main_rec = trainer.train_ds.record(0)
    for _ in range(args.epochs + 1):
        start.record()
        for _i in range(50):
            tail_step.run_from(rec)
        stop.record(); stop.synchronize()
        t_tail.append(start.elapsed_time(stop) / 50 * 1e3)
        start.record()
        for _i in range(50):
            step.run_from(main_rec)
        stop.record(); stop.synchronize()
        t_main.append(start.elapsed_time(stop) / 50 * 1e3)
        start.record()
        for _i in range(200):
            _lib.check(_lib.load().dfm_loss_accumulate(step.loss.data_ptr(), opt.l2, opt.flat_param.data_ptr(), opt.n_l2,
                                                       step._loss_acc.data_ptr(), _lib.stream_handle()))
        stop.record(); stop.synchronize()
        t_acc.append(start.elapsed_time(stop) / 200 * 1e3)
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "positives": P, "negatives_per_positive": K, "batch": B,
           "steps_per_epoch": len(loader_b), "tail_rows": trainer.train_ds.tail_rows, "n_l2": int(opt.n_l2),
           "epochs": args.epochs, "b_parent_loop_epoch_ms": stats(tb), "t_trainer_epoch_ms": stats(tt),
           "tail_step_us": stats(t_tail[1:]), "tracked_main_step_us": stats(t_main[1:]),
           "loss_accumulate_us": stats(t_acc[1:]), "mean_loss_last_epoch": losses[-1]}
    out["t_minus_b_ms"] = out["t_trainer_epoch_ms"]["median"] - out["b_parent_loop_epoch_ms"]["median"]
    out["b_spread_ms"] = out["b_parent_loop_epoch_ms"]["max"] - out["b_parent_loop_epoch_ms"]["min"]
    out["t_median_within_b_max"] = bool(out["t_trainer_epoch_ms"]["median"] <= out["b_parent_loop_epoch_ms"]["max"])
    out["accumulator_share_ms"] = out["loss_accumulate_us"]["median"] * (len(loader_b) + 1) / 1e3
    out["tail_share_ms"] = out["tail_step_us"]["median"] / 1e3
    print(json.dumps(out, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def _host_columns(cols):
    """Per field, schema order: its host column."""
    from deepfm_amd.data.schema import FeatureType
    its = {FeatureType.SPARSE: iter(cols.ids), FeatureType.DENSE: iter(cols.dense), FeatureType.SEQUENCE: iter(cols.bags)}
    return [next(its[s.feature_type]) for s in cols.schema.fields.values()]


if __name__ == "__main__":
    main()
