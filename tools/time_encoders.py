#!/usr/bin/env python3
"""Time the device-side feature encoders (``deepfm_amd/data/encoders.py``) in one process.

  fit / transform   26 id columns of ``--rows`` raw int64 keys (default 2^21 = 2 097 152 rows: 416 MiB of raw keys and
                    as much of ids, beside the sort's temporaries), keys drawn from 10^6 values, uniform and Zipf(1.1);
                    ``DeviceFeatureEncoder.fit`` and ``.transform`` with the raw columns on the device, and again from
                    host arrays (the upload included);
  host              ``np.unique`` + ``np.searchsorted`` over the same columns, plus the copy of the ids to the device
                    (``--host-reps`` repeats: a repeat takes seconds);
  dict              the reference's dict loop (``tests/encoders_reference.py``) on a 100 000-value subsample of one column;
  encode_into       one batch record at B = 4096 of the 26 SPARSE + 13 DENSE schema (40 jobs, one launch), beside an
                    empty launch, ``dfm_record_assemble`` of the same record from already encoded device columns, and
                    the ``dfm_encode_columns`` launch alone from a job table built once: device events around a block
                    of ``--block`` calls, and the host's own time per call;
  floor             bytes the lookups must move (8 raw + 8 id + one 16-byte slot per value) over 8 TB/s.

Medians of ``--reps`` (15) with min-max, one JSON object.  Needs the GPU: there is no fallback.

    python tools/time_encoders.py [--rows N] [--reps 15] [--host-reps 3] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
NS, ND, B, VOCAB = 26, 13, 4096, 1_000_000


def stats(xs, scale=1.0):
    xs = sorted(x * scale for x in xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


def block_us(fn, block, reps):
    """Device time per call of a block of back-to-back calls (events), and the host's time per call to enqueue them."""
    dev, host = [], []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        a.record()
        for _ in range(block):
            fn()
        b.record()
        host.append((time.perf_counter() - t) / block * 1e6)
        torch.cuda.synchronize()
        dev.append(a.elapsed_time(b) / block * 1e3)
    return stats(dev[1:]), stats(host[1:])                      # the first block is the warm-up


def draw(kind, rng, rows):
    """One raw column: keys spread over int64 (a multiplicative scramble of the drawn rank)."""
    if kind == "uniform":
        rank = rng.integers(0, VOCAB, rows)
    else:
        rank = np.minimum(rng.zipf(1.1, rows), VOCAB) - 1
    return (rank.astype(np.int64) * np.int64(0x9E3779B97F4A7C15 - (1 << 64))) ^ np.int64(0x5851F42D4C957F2D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_encoders.py needs the GPU")
    from deepfm_amd import _lib
    from deepfm_amd.data import DeviceEpochLoader, DeviceFeatureEncoder
    from deepfm_amd.data.packed import RecordLayout
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    from tests import encoders_reference as R
    dev, rows = torch.device("cuda"), args.rows
    names = [f"C{i}" for i in range(NS)]
    ids_schema = DatasetSchema(fields={n: FieldSchema(n, FeatureType.SPARSE, 0, 16) for n in names})
    labels_h = np.zeros(rows, np.float32)
    labels_d = torch.from_numpy(labels_h).to(dev)
    out = {"rows": rows, "id_columns": NS, "key_space": VOCAB, "reps": args.reps, "host_reps": args.host_reps,
           "device": torch.cuda.get_device_name(0)}
    with np.errstate(over="ignore"):
        for kind in ("uniform", "zipf"):
            rng = np.random.default_rng(1)
            raw_h = {n: draw(kind, rng, rows) for n in names}
            raw_d = {n: torch.from_numpy(v).to(dev) for n, v in raw_h.items()}
            enc = DeviceFeatureEncoder(ids_schema)
            res = {}
            enc.fit(raw_d), enc.transform(raw_d, labels_d)                                   # warm-up
            res["fit_device_input_ms"] = stats(wall(lambda: enc.fit(raw_d), args.reps), 1e3)
            res["transform_device_input_ms"] = stats(wall(lambda: enc.transform(raw_d, labels_d), args.reps), 1e3)
            res["fit_host_input_ms"] = stats(wall(lambda: enc.fit(raw_h), args.reps), 1e3)
            res["transform_host_input_ms"] = stats(wall(lambda: enc.transform(raw_h, labels_h), args.reps), 1e3)
            res["vocabulary_sizes"] = [enc.encoders[names[0]].vocabulary_size, enc.encoders[names[-1]].vocabulary_size]
            floor = 32.0 * rows * NS / HBM_BYTES_PER_S
            res["transform_byte_floor_ms"] = floor * 1e3
            res["transform_over_floor"] = res["transform_device_input_ms"]["median"] / (floor * 1e3)

            def host_fit():
                return {n: np.unique(v) for n, v in raw_h.items()}

            def host_transform(keys):
                ids = np.empty((NS, rows), np.int64)
                for i, n in enumerate(names):
                    pos = np.minimum(np.searchsorted(keys[n], raw_h[n]), len(keys[n]) - 1)
                    ids[i] = np.where(keys[n][pos] == raw_h[n], pos + 1, 0)
                return torch.from_numpy(ids).to(dev)

            kept = {}                                            # the timed repeats' own results are the ones compared
            res["numpy_unique_ms"] = stats(wall(lambda: kept.update(keys=host_fit()), args.host_reps), 1e3)
            keys = kept["keys"]
            res["numpy_searchsorted_and_upload_ms"] = stats(
                wall(lambda: kept.update(ids=host_transform(keys)), args.host_reps), 1e3)
            got = enc.transform(raw_d, labels_d).ids
            assert torch.equal(got, kept["ids"]), "device and host encodings differ"
            sub = raw_h[names[0]][:100_000]
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                R.label_transform(keys[names[0]], sub)
                t.append(time.perf_counter() - t0)
            res["dict_loop_100k_values_ms"] = stats(t, 1e3)
            res["dict_loop_26_columns_extrapolated_s"] = stats(t)["median"] * NS * rows / sub.size
            out[kind] = res
            del raw_d, got, kept

    # ---- one serving batch: 26 SPARSE + 13 DENSE, B = 4096
    fields = {n: FieldSchema(n, FeatureType.SPARSE, 0, 16) for n in names}
    fields.update({f"I{i}": FieldSchema(f"I{i}", FeatureType.DENSE, embedding_dim=16) for i in range(ND)})
    schema = DatasetSchema(fields=fields)
    rng = np.random.default_rng(2)
    n_fit = 1 << 18
    raw = {n: torch.from_numpy(draw("zipf", rng, n_fit)).to(dev) for n in names}
    raw.update({f"I{i}": torch.from_numpy(rng.lognormal(0, 2, n_fit).astype(np.float32)).to(dev) for i in range(ND)})
    labels = torch.zeros(n_fit, device=dev)
    enc = DeviceFeatureEncoder(schema).fit(raw)
    cols = enc.transform(raw, labels)
    lay = RecordLayout.of(enc.schema, B)
    batch = {k: v[:B] for k, v in raw.items()}
    rec_a = torch.zeros(lay.record_bytes, dtype=torch.uint8, device=dev)
    rec_b = torch.zeros_like(rec_a)
    loader = DeviceEpochLoader(cols, B, shuffle=False)
    enc.encode_into(rec_a, batch, labels[:B])
    loader.assemble_into(rec_b, 0, B)
    assert torch.equal(rec_a, rec_b), "encode_into and dfm_record_assemble disagree on the record"
    lib, stream = _lib.load(), _lib.stream_handle()
    serving = {"batch": B, "jobs": NS + ND + 1, "record_bytes": lay.record_bytes}
    # the launch alone, from a job table built once: what encode_into costs without its per-call host work
    _, cols_b, labels_b = enc._inputs(batch, labels[:B])
    outs = {name: rec_a.data_ptr() + off for name, off in zip(lay.names, lay.field_offsets)}
    jobs = enc._jobs(cols_b, labels_b, outs, rec_a.data_ptr() + lay.labels_offset)
    table = (_lib.EncodeJob * len(jobs))(*jobs)
    for key, fn in (("empty_launch", lambda: lib.dfm_debug_empty_launch(stream)),
                    ("record_assemble", lambda: loader.assemble_into(rec_b, 0, B)),
                    ("encode_columns_prebuilt_jobs", lambda: lib.dfm_encode_columns(table, len(jobs), B, B, stream)),
                    ("encode_into", lambda: enc.encode_into(rec_a, batch, labels[:B]))):
        d, h = block_us(fn, args.block, args.reps)
        serving[key + "_device_us"], serving[key + "_host_us"] = d, h
    serving["encode_into_byte_floor_us"] = (32.0 * NS + 8.0 * (ND + 1)) * B / HBM_BYTES_PER_S * 1e6
    out["serving_batch"] = serving
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
