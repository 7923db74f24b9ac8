#!/usr/bin/env python3
"""Generate tests/golden/interactions_reference.npz from the REFERENCE's adapter methods.

Run in the build container only, like tools/make_trainer_golden.py (needs the reference checkout and pandas; neither
travels to the GPU box):   python tools/make_interactions_golden.py REFERENCE_CHECKOUT

The reference is imported, not copied; ``dacite``, which ``deepfm.config`` imports and nothing here needs, is replaced
by a stand-in in ``sys.modules``.  Its own ``_temporal_split``, ``_leave_one_out_split``, ``_build_popularity_weights``,
``_fit_encoders`` and ``_transform`` run on one small synthetic frame (400 rows, 25 users, 60 items; placeholder
values in the columns this fixture does not concern) that carries a ``row`` column, so the fixture stores row indices.

The fixture is data only:
  user_rows, item_rows, timestamps, ratings, labels, label_threshold, n_users, n_items       the log
  temporal/<k>/{val_ratio, test_ratio, train, val, test}                                     k = 0 .. 3
  loo/<m>/{train, val, test}                                                                 min_interactions m = 2, 3
  user_items                                                (pairs, 2) sorted (user row, item row): ``_user_items``
  <strategy>/{user_counts, item_counts}                     training positives per entity (0 where there is none)
  <strategy>/pop_weights_alpha1                             ``_build_popularity_weights`` at alpha = 1: max(count, 1)
  <strategy>/{user_rating_count, item_rating_count}         ``_transform`` of the whole frame, float32 per row
for the strategies temporal/0 and loo/3.

The inputs are ones on which the reference's answer is unique: no user has two rows with equal timestamps.  Ties
between users are many, and both cutoffs of every temporal case fall inside a run of equal timestamps.  The order of a
temporal ``train`` within such a run is pandas' and unspecified; the tests compare that part as a set.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "interactions_reference.npz")

sys.path.insert(0, REF)
sys.modules.setdefault("dacite", types.SimpleNamespace(from_dict=None))
import pandas as pd  # noqa: E402
from deepfm.config import DataConfig  # noqa: E402
from deepfm.data.movielens import MovieLensAdapter  # noqa: E402

N, N_USERS, N_ITEMS, N_TIMES = 400, 25, 60, 90
TEMPORAL = [(0.1, 0.1), (0.15, 0.05), (0.2, 0.2), (0.0, 0.1)]
LOO = [2, 3]
THRESHOLD = 4.0


def user_key(rows):
    return 10 + 3 * np.asarray(rows)          # ascending in the row, so "ascending user_id" is "ascending user row"


def item_key(rows):
    return 100 + 7 * np.asarray(rows)


def draw(rng):
    """Users 0..2 have 1, 2 and 3 rows (below, at and above the leave-one-out thresholds), the others share the
    rest; a user's timestamps are distinct, drawn from N_TIMES values so that users tie with each other."""
    sizes = np.array([1, 2, 3] + [0] * (N_USERS - 3))
    rest = rng.multinomial(N - 6 - 4 * (N_USERS - 3), np.ones(N_USERS - 3) / (N_USERS - 3)) + 4
    sizes[3:] = rest
    user = np.repeat(np.arange(N_USERS), sizes)
    ts = np.concatenate([rng.choice(N_TIMES, s, replace=False) for s in sizes]).astype(np.int64) * 3600 + 874724710
    perm = rng.permutation(N)
    user, ts = user[perm], ts[perm]
    item = rng.integers(0, N_ITEMS - 2, N)    # the last two items are never rated; duplicated (user, item) pairs occur
    rating = rng.integers(1, 6, N)
    return user.astype(np.int64), item.astype(np.int64), ts, rating.astype(np.int64)


def cutoffs_inside_ties(ts):
    s, n = np.sort(ts), len(ts)
    for v, t in TEMPORAL:
        for q in (1 - v - t, 1 - t):
            lo = int(np.floor(q * (n - 1)))
            if lo + 1 >= n or lo < 1 or not s[lo - 1] == s[lo] == s[lo + 1]:
                return False
    return True


def frame(user, item, ts, rating):
    n = len(user)
    rng = np.random.default_rng(1)
    weekday = rng.integers(0, 7, n)
    return pd.DataFrame({
        "row": np.arange(n), "user_id": user_key(user), "movie_id": item_key(item), "timestamp": ts, "rating": rating,
        "label": (rating >= THRESHOLD).astype(np.float32),
        # placeholders: the columns _fit_encoders / _transform walk over but this fixture does not store
        "gender": "F", "age": 25, "occupation": "none", "zip_prefix": "000", "genres": [["Drama"]] * n,
        "release_year_bucket": "1990-1994", "movie_age_at_rating": "1-3yr", "num_genres": "1",
        "dow_sin": np.sin(2 * np.pi * weekday / 7).astype(np.float32), "dow_cos": np.float32(0),
        "hour_sin": np.float32(0), "hour_cos": np.float32(0),
    })


def dense(series, keys):
    """A pandas count series indexed by raw key as a vector over the rows, 0 where the key is absent."""
    return np.array([int(series.get(k, 0)) for k in keys], np.int64)


def main() -> None:
    rng = np.random.default_rng(20240611)
    for attempt in range(10000):
        user, item, ts, rating = draw(rng)
        if cutoffs_inside_ties(ts):
            break
    else:
        sys.exit("no draw has every cutoff inside a run of equal timestamps")
    df = frame(user, item, ts, rating)
    assert not df.duplicated(["user_id", "timestamp"]).any()
    out = {"user_rows": user, "item_rows": item, "timestamps": ts, "ratings": rating,
           "labels": df["label"].to_numpy(), "label_threshold": np.float64(THRESHOLD),
           "n_users": np.int64(N_USERS), "n_items": np.int64(N_ITEMS)}

    def adapter(**kw):
        a = MovieLensAdapter(DataConfig(data_dir=".", label_threshold=THRESHOLD, neg_sampling_alpha=1.0, **kw))
        a._all_movie_ids = set(item_key(np.arange(N_ITEMS)).tolist())
        return a

    def rows_of(parts):
        return {k: p["row"].to_numpy().astype(np.int64) for k, p in zip(("train", "val", "test"), parts)}

    def features(a, prefix, train_df):
        weights = a._build_popularity_weights(train_df)
        a._fit_encoders(train_df)
        ds = a._transform(df)
        out[f"{prefix}/user_counts"] = dense(a._user_counts, user_key(np.arange(N_USERS)))
        out[f"{prefix}/item_counts"] = dense(a._item_counts, item_key(np.arange(N_ITEMS)))
        out[f"{prefix}/pop_weights_alpha1"] = np.array([weights[k] for k in item_key(np.arange(N_ITEMS))], np.float64)
        for name in ("user_rating_count", "item_rating_count"):
            col = ds.features[name]
            assert col.dtype == np.float32 and col.shape == (N,)
            out[f"{prefix}/{name}"] = col

    user_items = None
    for k, (v, t) in enumerate(TEMPORAL):
        a = adapter(split_strategy="temporal", temporal_val_ratio=v, temporal_test_ratio=t)
        parts = a._temporal_split(df)
        out[f"temporal/{k}/val_ratio"], out[f"temporal/{k}/test_ratio"] = np.float64(v), np.float64(t)
        for name, rows in rows_of(parts).items():
            out[f"temporal/{k}/{name}"] = rows
        assert list(parts[1]["user_id"]) == sorted(parts[1]["user_id"])
        print(f"temporal {v}, {t}: {[len(p) for p in parts]} rows")
        user_items = a._user_items
        if k == 0:
            features(a, "temporal/0", parts[0])
    for m in LOO:
        a = adapter(split_strategy="leave_one_out", min_interactions=m)
        parts = a._leave_one_out_split(df)
        for name, rows in rows_of(parts).items():
            out[f"loo/{m}/{name}"] = rows
        print(f"leave one out, min {m}: {[len(p) for p in parts]} rows")
        assert a._user_items == user_items
        if m == 3:
            features(a, "loo/3", parts[0])
    to_user = {int(k): r for r, k in enumerate(user_key(np.arange(N_USERS)))}
    to_item = {int(k): r for r, k in enumerate(item_key(np.arange(N_ITEMS)))}
    out["user_items"] = np.array(sorted((to_user[u], to_item[i]) for u, s in user_items.items() for i in s), np.int64)

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes (draw {attempt})")


if __name__ == "__main__":
    main()
