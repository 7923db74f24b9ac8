#!/usr/bin/env python3
"""Generate tests/golden/encoders_reference.npz from the REFERENCE's feature transforms.

Run in the build container only, like tools/make_golden.py (needs the reference checkout; it never travels to the GPU
box):   python tools/make_encoders_golden.py REFERENCE_ROOT

``deepfm/data/transforms.py`` is loaded by file path (it imports numpy only).  The fixture is data only: raw integer
columns, token lists as a padded matrix plus lengths, float columns, a held-out split with unseen values, and what the
reference's LabelEncoder / MultiHotEncoder / MinMaxScaler make of them (fitted on the train split).

Two field sets share the file (the tests build the schemas around them):
  mixed    user_id, movie_id SPARSE; genres SEQUENCE (max_length 4, rows of up to 7 raw tokens); age (float32),
           timestamp (float64, a span float32 cannot hold) DENSE
  uniform  C0..C3 SPARSE; I0 (float32), I1 (float64) DENSE
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "encoders_reference.npz")

spec = importlib.util.spec_from_file_location("_ref_transforms", f"{REF}/deepfm/data/transforms.py")
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)

N_TRAIN, N_HELD = 300, 100
MAX_LENGTH, RAW_WIDTH = 4, 7
SPLITS = (("train", N_TRAIN), ("heldout", N_HELD))


def main() -> None:
    rng = np.random.default_rng(20240607)
    out = {"max_length": np.int64(MAX_LENGTH)}

    # raw key pools: the held-out split draws from a wider pool, so it holds unseen keys
    i64 = np.iinfo(np.int64)
    pools = {
        "user_id": np.concatenate([np.arange(-5, 60), [i64.min, i64.max]]).astype(np.int64),
        "movie_id": (np.arange(120, dtype=np.int64) * 7919 - 400000),
        "C0": np.arange(40, dtype=np.int64),
        "C1": rng.integers(-2**62, 2**62, 80),
        "C2": np.arange(1000, 1003, dtype=np.int64),
        "C3": (np.arange(200, dtype=np.int64) << 33) + 1,
    }
    sparse = {}
    for name, pool in pools.items():
        seen = pool[: max(2, (2 * len(pool)) // 3)]
        zipf = 1.0 / np.arange(1, len(seen) + 1)
        sparse[name] = {"train": rng.choice(seen, N_TRAIN, p=zipf / zipf.sum()),
                        "heldout": rng.choice(pool, N_HELD)}
    for name, cols in sparse.items():
        enc = T.LabelEncoder().fit(cols["train"].tolist())
        out[f"vocab/{name}"] = np.int64(enc.vocabulary_size)
        for split, _ in SPLITS:
            out[f"raw/{name}/{split}"] = cols[split].astype(np.int64)
            got = enc.transform(cols[split].tolist())
            assert got.dtype == np.int64
            out[f"ref/{name}/{split}"] = got
        assert (out[f"ref/{name}/train"] > 0).all()
    assert any((out[f"ref/{n}/heldout"] == 0).any() for n in sparse)

    # token lists: lengths 0 .. RAW_WIDTH (some above max_length), unseen tokens in the middle of held-out rows
    genre_pool = np.arange(100, 130, dtype=np.int64) * 3
    lists = {}
    for split, n in SPLITS:
        pool = genre_pool[:20] if split == "train" else genre_pool
        lengths = rng.integers(0, RAW_WIDTH + 1, n).astype(np.int32)
        lengths[:5] = [0, 1, MAX_LENGTH - 1, MAX_LENGTH, RAW_WIDTH]
        tokens = rng.choice(pool, (n, RAW_WIDTH)).astype(np.int64)        # the tail past `lengths` is junk on purpose
        lists[split] = [tokens[i, :lengths[i]].tolist() for i in range(n)]
        out[f"raw/genres/{split}/tokens"], out[f"raw/genres/{split}/lengths"] = tokens, lengths
    enc = T.MultiHotEncoder(max_length=MAX_LENGTH).fit(lists["train"])
    out["vocab/genres"] = np.int64(enc.vocabulary_size)
    for split, _ in SPLITS:
        out[f"ref/genres/{split}"] = enc.transform(lists[split])
    held = out["ref/genres/heldout"]
    assert ((held[:, :-1] == 0) & (held[:, 1:] > 0)).any(), "no OOV token in the middle of a held-out row"

    # float columns; the held-out split leaves the fitted range
    dense = {
        "age": lambda n, wide: (rng.uniform(18, 70, n) + (rng.normal(0, 40, n) if wide else 0)).astype(np.float32),
        "timestamp": lambda n, wide: 1.0e9 + rng.integers(0, 2**34, n).astype(np.float64) / 1024.0 * (2 if wide else 1),
        "I0": lambda n, wide: rng.lognormal(0, 2, n).astype(np.float32) * (3 if wide else 1),
        "I1": lambda n, wide: rng.normal(0, 1e-3, n) * (2 if wide else 1),
    }
    for name, draw in dense.items():
        cols = {"train": draw(N_TRAIN, False), "heldout": draw(N_HELD, True)}
        sc = T.MinMaxScaler().fit(cols["train"])
        out[f"min/{name}"], out[f"max/{name}"] = np.float64(sc._min), np.float64(sc._max)
        for split, _ in SPLITS:
            out[f"raw/{name}/{split}"] = cols[split]
            got = sc.transform(cols[split])
            assert got.dtype == np.float64
            out[f"ref/{name}/{split}"] = got
        h = out[f"ref/{name}/heldout"]
        assert (h < 0).any() or (h > 1).any()
    for split, n in SPLITS:
        out[f"labels/{split}"] = (rng.random(n) < 0.3).astype(np.float32)

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
