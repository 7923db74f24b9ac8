"""The Poisson-bootstrap contract restated in numpy (the yardstick of tests/test_*_bootstrap.py), from the definitions in
include/deepfm_hip.h.

A sample is used when its score is not NaN, its label is exactly 0 or 1 and its unit id lies in [0, 2^40); each failure is
counted on its own and a sample with any of them enters nothing else.  Without unit ids the unit of sample i is i.

    h = mix32(seed * 0x9E3779B97F4A7C15 + 0x426F6F7453747261 + (r << 40) + unit)        wrapping uint64
    w = #{k : h >= T[k]},  T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!)                   Poisson(1) truncated at 12

Per replicate, over the used samples (float32 score order, -0.0 == +0.0):

    P = sum_{y = 1} w,  N = sum_{y = 0} w,  S = P + N
    U = sum_{y_i = 1, y_j = 0} w_i w_j (2 [s_i > s_j] + [s_i == s_j])
    L = sum w_i rint(l_i * 2^27),  l_i the per-sample log loss of the pooled metric
    auc_r = float64(U) / float64(2 P N),  logloss_r = float64(L) * 2^-27 / float64(S)     (NaN for a zero denominator)

U comes from ``searchsorted`` on the sorted order keys of the negatives and the prefix sums of their weights.
"""
import numpy as np

from tests.grouped_auc_reference import ord_bits

GOLDEN = 0x9E3779B97F4A7C15
SALT = 0x426F6F7453747261
MASK = (1 << 64) - 1
T = np.array([1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291,
              4294609777, 4294923276, 4294962463, 4294966817, 4294967252, 4294967292], np.uint64)
UNIT_LIMIT = 1 << 40
L_UNIT = 2.0 ** -27


def mix32(x):
    """The counter hash of the dropout masks: uint64 array -> its low 32 bits after two multiply-xorshift rounds."""
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x & np.uint64(0xFFFFFFFF)


def weights(seed, r, units):
    """int64 weights of the units (any integer array below 2^40) in replicate r."""
    base = (int(seed) * GOLDEN + SALT + (int(r) << 40)) & MASK
    with np.errstate(over="ignore"):
        h = mix32(np.uint64(base) + np.asarray(units).astype(np.uint64))
    return np.searchsorted(T, h, side="right").astype(np.int64)


def logloss_terms(scores, positive):
    """rint(l * 2^27) as int64: the scores clipped to [1e-7, 1 - 1e-7] in float32, [1 - p, p] formed in float32 and
    clipped to [eps, 1 - eps] with eps = 2^-23, the logarithm in float64."""
    s = np.asarray(scores, np.float32)
    p = np.minimum(np.maximum(s, np.float32(1e-7)), np.float32(1.0 - 1e-7))
    t = np.where(positive, p, np.float32(1.0) - p).astype(np.float32)
    eps = np.float32(2.0 ** -23)
    t = np.minimum(np.maximum(t, eps), np.float32(1.0) - eps)
    return np.rint(-np.log(t.astype(np.float64)) * 2.0 ** 27).astype(np.int64)


def used_samples(labels, scores, unit_ids=None):
    """(mask of the used samples, units, [NaN scores, labels other than 0 / 1, bad unit ids])."""
    y = np.asarray(labels, np.float32).reshape(-1)
    s = np.asarray(scores, np.float32).reshape(-1)
    u = np.arange(s.size, dtype=np.int64) if unit_ids is None else np.asarray(unit_ids, np.int64).reshape(-1)
    nan = np.isnan(s)
    bad_label = (y != 0) & (y != 1)
    bad_unit = (u < 0) | (u >= UNIT_LIMIT)
    return ~(nan | bad_label | bad_unit), u, [int(nan.sum()), int(bad_label.sum()), int(bad_unit.sum())]


def bootstrap(labels, scores, replicates, seed=0, unit_ids=None):
    """dict(counts (R, 5) int64 [U, P, N, L, S], values (R, 2) float64 [auc_r, logloss_r], faults (3) int64)."""
    ok, u, faults = used_samples(labels, scores, unit_ids)
    y = np.asarray(labels, np.float32).reshape(-1)[ok]
    s = np.asarray(scores, np.float32).reshape(-1)[ok]
    u = u[ok]
    pos = y == 1
    k = ord_bits(s).astype(np.int64)
    lt = logloss_terms(s, pos)
    order = np.argsort(k[~pos], kind="stable")
    kneg, kpos = k[~pos][order], k[pos]
    below, upto = np.searchsorted(kneg, kpos, side="left"), np.searchsorted(kneg, kpos, side="right")
    counts = np.zeros((replicates, 5), np.int64)
    values = np.full((replicates, 2), np.nan)
    for r in range(replicates):
        w = weights(seed, r, u)
        cw = np.concatenate([[0], np.cumsum(w[~pos][order])])
        # 2 * (weight below) + (weight at the same score)
        U = int((w[pos] * (cw[below] + cw[upto])).sum())
        P, N, L = int(w[pos].sum()), int(w[~pos].sum()), int((w * lt).sum())
        counts[r] = [U, P, N, L, P + N]
        if P and N:
            values[r, 0] = float(U) / float(2 * P * N)          # int -> float rounds to nearest, once each
        if P + N:
            values[r, 1] = float(L) * L_UNIT / float(P + N)
    return dict(counts=counts, values=values, faults=np.array(faults, np.int64))


def brute_force_u(labels, scores, w):
    """U of one replicate by the O(P N) double loop over the used samples, comparing as float32."""
    y = np.asarray(labels, np.float32)
    s = np.asarray(scores, np.float32)
    total = 0
    for i in np.flatnonzero(y == 1):
        for j in np.flatnonzero(y == 0):
            total += int(w[i]) * int(w[j]) * (2 if s[i] > s[j] else (1 if s[i] == s[j] else 0))
    return total


def summary(values, level=0.95):
    """The spread the package's ``bootstrap_dict`` gives for ``values`` (R, 2), written out independently."""
    q = (1.0 - level) / 2.0
    out = {}
    for j, name in enumerate(("auc", "logloss")):
        x = np.asarray(values, np.float64).reshape(-1, 2)[:, j]
        kept = x[~np.isnan(x)]
        out[f"{name}_se"] = float(np.std(kept, ddof=1)) if kept.size > 1 else float("nan")
        out[f"{name}_lo"] = float(np.nanquantile(x, q)) if kept.size else float("nan")
        out[f"{name}_hi"] = float(np.nanquantile(x, 1.0 - q)) if kept.size else float("nan")
        out[f"{name}_replicates"] = int(kept.size)
    return out
