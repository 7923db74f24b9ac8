#!/usr/bin/env python3
"""Time of the permutation field importance (``training/importance.py``, csrc/importance.hip).
At the Criteo shape (26 SPARSE + 13 DENSE fields, DeepFM, B = 4096, ``--samples`` = 10^6 samples):
  * the whole report, every field at 5 repeats (196 passes over the set), wall clock (``--report-reps`` repetitions);
  * one variant alone (half of a one-field, one-repeat run, which is a baseline pass and a permuted pass) against one
    plain ``evaluate_loader`` of the same rows, alternating, and their ratio;
  * the permute launch alone by device events over back-to-back launches, beside an empty launch and the time its
    byte floor (2 x record_bytes) takes at 8 TB/s;
  * a host loop (``np.random.permutation`` of one column, ``PackedColumns``, ``predictor.evaluate``) at 2 fields x 1
    repeat, scaled linearly to every field at 5 repeats.
At the ML-100K evaluation shape (943 users x 1000 candidates, ``MixedSchemaPredictor``, ``ranking_ks=[5, 10]``): the
whole report of every field at 5 repeats and one plain ``evaluate_loader`` with the same keywords.
Medians and ranges over ``--reps`` repetitions; one JSON line per case.
usage: python tools/time_importance.py [--reps 15] [--report-reps 15] [--samples 1000000] [--only criteo|movielens]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.time_bootstrap import device_ms  # noqa: E402
from tools.time_gauc import stats, wall  # noqa: E402

REPEATS = 5
HBM_BYTES_PER_S = 8.0e12


def criteo_case(reps, report_reps, n):
    from deepfm_amd import _lib
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FieldImportance, FusedPredictor, RecordSet
    from deepfm_amd.training.importance import permutation_keys, permute_into, record_fields
    from tools.time_predict import B, V, build
    model = build("deepfm")
    rng = np.random.default_rng(0)
    feats = {name: (rng.integers(0, V, n) if spec.feature_type.name == "SPARSE" else rng.random(n).astype(np.float32))
             for name, spec in model.schema.fields.items()}
    cols = PackedColumns(model.schema, feats, (rng.random(n) < 0.3).astype(np.float32))
    pred = FusedPredictor(model, B)
    names = list(model.schema.fields)
    rs = RecordSet.from_columns(pred, cols)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    fi = FieldImportance(pred)
    for _ in range(2):                                            # warm-up of every form
        fi.run(rs, fields=names[:2], repeats=1)
        pred.evaluate_loader(loader)
    whole = [wall(lambda: fi.run(rs, repeats=REPEATS))[0] for _ in range(report_reps)]
    build_set = [wall(lambda: RecordSet.from_columns(pred, cols))[0] for _ in range(3)]
    variant, plain = [], []
    for _ in range(reps):                                         # alternating: the same neighbours for both
        # a run of one field and one repeat is two passes (the baseline and the variant): the variant is half of it
        variant.append(wall(lambda: fi.run(rs, fields=names[:1], repeats=1))[0] / 2)
        plain.append(wall(lambda: pred.evaluate_loader(loader))[0])
    # the permute launch alone
    lay = pred.layout
    ordered = torch.sort(permutation_keys(0, 0, n, pred.device)).values
    fields = record_fields(lay)
    out = torch.zeros(rs.stride, dtype=torch.uint8, device=pred.device)
    lib = _lib.load()
    one = device_ms(lambda: permute_into(rs, fields, ordered, 1, B, B, out), reps, calls=200)
    every = device_ms(lambda: permute_into(rs, fields, ordered, (1 << len(names)) - 1, B, B, out), reps, calls=200)
    empty = device_ms(lambda: _lib.check(lib.dfm_debug_empty_launch(_lib.stream_handle())), reps, calls=200)

    def host_loop():
        out = []
        for name in names[:2]:
            shuffled = dict(feats)
            shuffled[name] = feats[name][np.random.permutation(n)]
            out.append(pred.evaluate(PackedColumns(model.schema, shuffled, cols.labels)))
        return out
    host = [wall(host_loop)[0] * len(names) * REPEATS / 2 for _ in range(3)]
    print(json.dumps(dict(
        case="criteo", samples=n, B=B, fields=len(names), repeats=REPEATS, reps=reps, report_reps=report_reps,
        whole_report_s=stats(whole, scale=1.0), passes=1 + len(names) * REPEATS,
        record_set_from_columns_s=stats(build_set, scale=1.0), record_set_bytes=rs.records.numel(),
        one_variant_ms=stats(variant), plain_evaluate_loader_ms=stats(plain),
        variant_over_plain=round(float(np.median(variant) / np.median(plain)), 3),
        permute_one_field_us=stats(one), permute_every_field_us=stats(every), empty_launch_us=stats(empty),
        record_bytes=lay.record_bytes, byte_floor_us=round(2 * lay.record_bytes / HBM_BYTES_PER_S * 1e6, 3),
        host_loop_s_scaled=stats(host, scale=1.0), host_fields_timed=2)), flush=True)


def movielens_case(reps, report_reps):
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FieldImportance, MixedSchemaPredictor, RecordSet
    from tools.time_predict_mixed import B, C, U, build, split
    rng = np.random.default_rng(0)
    model = build("deepfm")
    feats, labels = split(rng)
    cols = PackedColumns(model.schema, feats, labels)
    loader = DeviceEpochLoader(DeviceColumns(cols, "cuda"), B, shuffle=False)
    pred = MixedSchemaPredictor(model, B)
    kw = dict(ranking_ks=[5, 10])
    rs = RecordSet.from_loader(pred, loader)
    fi = FieldImportance(pred)
    for _ in range(2):
        fi.run(rs, fields=["user_id"], repeats=1, **kw)
        pred.evaluate_loader(loader, **kw)
    whole = [wall(lambda: fi.run(rs, repeats=REPEATS, **kw)) for _ in range(report_reps)]
    report = whole[-1][1]
    variant, plain = [], []
    for _ in range(reps):
        variant.append(wall(lambda: fi.run(rs, fields=["genres"], repeats=1, **kw))[0] / 2)
        plain.append(wall(lambda: pred.evaluate_loader(loader, **kw))[0])
    print(json.dumps(dict(
        case="movielens", split=f"{U}x{C}", B=B, fields=len(report.groups), repeats=REPEATS, reps=reps,
        report_reps=report_reps, whole_report_s=stats([t for t, _ in whole], scale=1.0),
        passes=1 + len(report.groups) * REPEATS, one_variant_ms=stats(variant), plain_evaluate_loader_ms=stats(plain),
        variant_over_plain=round(float(np.median(variant) / np.median(plain)), 3),
        top_logloss=report.ranking("logloss")[:3], top_ndcg10=report.ranking("NDCG@10")[:3])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--report-reps", type=int, default=15)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--only", choices=["criteo", "movielens"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_importance.py measures on the device: no GPU found")
    if args.only != "movielens":
        criteo_case(args.reps, args.report_reps, args.samples)
    if args.only != "criteo":
        movielens_case(args.reps, args.report_reps)


if __name__ == "__main__":
    main()
