"""The bootstrap of the per-user metrics restated in numpy (the yardstick of tests/test_*_bootstrap_units.py), from the
definitions in include/deepfm_hip.h.

HR@k, NDCG@k, uauc and gauc are means over users, so under integer user weights w_u (``bootstrap_reference.weights``
with the user id as the unit: the pooled bootstrap's resampling by user) a replicate is a quotient of two weighted sums
of per-user integers:

    rank_u     position of the user's first positive in np.argsort(-s, kind="stable"); NOT_COUNTED (-1) for a user
               that does not count, MISS (-2) for one that counts without a positive
    columns    counted | [rank < k] per k | (rank < k ? G[rank] : 0) per k,   G[i] = rint(2^30 / log2(i + 2))
               qual | qual q | qual size | qual size q,   size = P + N,  q = rint(auc_g 2^30)   (grouped_auc_reference)
    sums       S[r][m] = sum_u w_u(seed, r) columns[m][u]                               wrapping uint64
    HR@k_r = S hit / S counted,  NDCG@k_r = S gain 2^-30 / S counted,
    uauc_r = S (qual q) 2^-30 / S qual,  gauc_r = S (qual size q) 2^-30 / S (qual size)   (NaN for a zero denominator)

``brute_force_replicate`` does not use the sums: it materialises the resample, user u repeated w_u times as distinct
users, and evaluates the plain metrics on it.
"""
import numpy as np

from tests.bootstrap_reference import weights
from tests.grouped_auc_reference import group_integers

NOT_COUNTED, MISS = -1, -2
UNIT = 2.0 ** -30


def user_ranks(user_ids, labels, scores, num_users, require_both_classes=True):
    """(rank (num_users) int64, users counted, [bad ids, NaN scores, labels other than 0 / 1]).  A sample with a bad id
    enters nothing; NaN scores and other labels are only counted (the ranks are then meaningless)."""
    u = np.asarray(user_ids, np.int64).reshape(-1)
    y = np.asarray(labels, np.float32).reshape(-1)
    s = np.asarray(scores, np.float32).reshape(-1)
    ok = (u >= 0) & (u < num_users)
    faults = [int((~ok).sum()), int(np.isnan(s).sum()), int(((y != 0) & (y != 1)).sum())]
    rank = np.full(num_users, NOT_COUNTED, np.int64)
    for user in range(num_users):
        idx = np.flatnonzero(ok & (u == user))                    # dataset order
        pos = y[idx] == 1
        npos = int(pos.sum())
        keep = (0 < npos < idx.size) if require_both_classes else idx.size > 0
        if not keep:
            continue
        rank[user] = MISS
        order = np.argsort(-s[idx], kind="stable")
        for place, j in enumerate(order):
            if pos[j]:
                rank[user] = place
                break
    return rank, int((rank != NOT_COUNTED).sum()), faults


def gain_table(length):
    return np.rint(2.0 ** 30 / np.log2(np.arange(length, dtype=np.float64) + 2.0)).astype(np.int64)


def rank_columns(rank, ks):
    """(1 + 2 len(ks), users) int64: counted, hits per k, fixed-point gains per k."""
    rank = np.asarray(rank, np.int64)
    gain = gain_table(max(ks))
    cols = [(rank != NOT_COUNTED).astype(np.int64)]
    hits = [((rank >= 0) & (rank < k)) for k in ks]
    cols += [h.astype(np.int64) for h in hits]
    cols += [np.where(h, gain[np.clip(rank, 0, gain.size - 1)], 0) for h in hits]
    return np.stack(cols)


def group_columns(user_ids, labels, scores, num_users):
    """(4, users) int64: qual, qual q, qual size, qual size q."""
    num, P, N, _ = group_integers(user_ids, labels, scores, num_users)
    qual = (P > 0) & (N > 0)
    q = np.zeros(num_users, np.int64)
    for g in np.flatnonzero(qual):
        q[g] = int(np.rint(float(num[g]) / float(2 * int(P[g]) * int(N[g])) * 2.0 ** 30))
    size = np.where(qual, P + N, 0)
    return np.stack([qual.astype(np.int64), q, size, size * q])


def weighted_sums(cols, replicates, seed=0):
    """(replicates, num_cols) uint64: sum_u w_u cols[m][u] mod 2^64, unit u the column index."""
    cols = np.asarray(cols).astype(np.uint64)
    units = np.arange(cols.shape[1], dtype=np.int64)
    out = np.zeros((replicates, cols.shape[0]), np.uint64)
    with np.errstate(over="ignore"):
        for r in range(replicates):
            w = weights(seed, r, units).astype(np.uint64)
            out[r] = (cols * w[None, :]).sum(axis=1, dtype=np.uint64)
    return out


def _quotient(num, den, scale=1.0):
    num, den = np.asarray(num).astype(np.float64), np.asarray(den).astype(np.float64)     # rounded to nearest, once each
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num * scale / np.where(den > 0, den, 1.0), np.nan)


def names(ks, group_auc):
    return [f"HR@{k}" for k in ks] + [f"NDCG@{k}" for k in ks] + (["gauc", "uauc"] if group_auc else [])


def replicate_values(sums, num_ks, group_auc):
    """(replicates, 2 num_ks [+ 2]) float64 from the sums of [ranking columns | group columns], in ``names`` order."""
    m = num_ks
    out = []
    if m:
        out += [_quotient(sums[:, 1 + j], sums[:, 0]) for j in range(m)]
        out += [_quotient(sums[:, 1 + m + j], sums[:, 0], UNIT) for j in range(m)]
    if group_auc:
        g = sums[:, (1 + 2 * m if m else 0):]
        out += [_quotient(g[:, 3], g[:, 2], UNIT), _quotient(g[:, 1], g[:, 0], UNIT)]
    return np.stack(out, axis=1)


def columns(user_ids, labels, scores, ks, num_users, group_auc=False, require_both_classes=True):
    parts = []
    if len(ks):
        parts.append(rank_columns(user_ranks(user_ids, labels, scores, num_users, require_both_classes)[0], ks))
    if group_auc:
        parts.append(group_columns(user_ids, labels, scores, num_users))
    return np.concatenate(parts)


def bootstrap_grouped(user_ids, labels, scores, ks, replicates, seed=0, num_users=None, group_auc=False,
                      require_both_classes=True):
    """(replicates, 2 len(ks) [+ 2]) float64 replicate values, in ``names`` order."""
    if num_users is None:
        num_users = int(np.max(user_ids)) + 1
    cols = columns(user_ids, labels, scores, ks, num_users, group_auc, require_both_classes)
    return replicate_values(weighted_sums(cols, replicates, seed), len(ks), group_auc)


def brute_force_replicate(user_ids, labels, scores, ks, w, num_users, group_auc=False, require_both_classes=True):
    """One replicate with the resample written out: user u appears w[u] times, each copy a user of its own, and the
    plain metrics run on that population.  dict(counted, hits (per k), HR, NDCG (per k, plain float sums of 1 /
    log2(rank + 2)), and with group_auc qual, size, gauc, uauc); quotients NaN for an empty population."""
    u = np.asarray(user_ids, np.int64).reshape(-1)
    y = np.asarray(labels, np.float32).reshape(-1)
    s = np.asarray(scores, np.float32).reshape(-1)
    new_u, new_y, new_s, copies = [], [], [], 0
    for user in range(num_users):
        idx = np.flatnonzero(u == user)
        for _ in range(int(w[user])):
            new_u.append(np.full(idx.size, copies, np.int64))
            new_y.append(y[idx])
            new_s.append(s[idx])
            copies += 1
    U = max(copies, 1)
    cat = (lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype))
    ru, ry, rs = cat(new_u, np.int64), cat(new_y, np.float32), cat(new_s, np.float32)
    rank, counted, _ = user_ranks(ru, ry, rs, U, require_both_classes)
    out = dict(counted=counted, hits=[int(((rank >= 0) & (rank < k)).sum()) for k in ks])
    nan = float("nan")
    out["HR"] = [h / counted if counted else nan for h in out["hits"]]
    out["NDCG"] = [float(sum(1.0 / np.log2(r + 2.0) for r in rank if 0 <= r < k)) / counted if counted else nan
                   for k in ks]
    if group_auc:
        num, P, N, _ = group_integers(ru, ry, rs, U)
        qual = np.flatnonzero((P > 0) & (N > 0))
        auc = np.array([float(num[g]) / float(2 * int(P[g]) * int(N[g])) for g in qual])
        size = (P + N)[qual].astype(np.float64)
        out.update(qual=int(qual.size), size=int(size.sum()),
                   uauc=float(auc.mean()) if qual.size else nan,
                   gauc=float((size * auc).sum() / size.sum()) if qual.size else nan)
    return out


def summary(values, metric_names, level=0.95):
    """The spread the package's ``bootstrap_grouped_dict`` gives for ``values`` (R, len(names)), written out
    independently."""
    q = (1.0 - level) / 2.0
    v = np.asarray(values, np.float64).reshape(-1, len(metric_names))
    out = {}
    for j, name in enumerate(metric_names):
        kept = v[:, j][~np.isnan(v[:, j])]
        out[f"{name}_se"] = float(np.std(kept, ddof=1)) if kept.size > 1 else float("nan")
        out[f"{name}_lo"] = float(np.nanquantile(v[:, j], q)) if kept.size else float("nan")
        out[f"{name}_hi"] = float(np.nanquantile(v[:, j], 1.0 - q)) if kept.size else float("nan")
        out[f"{name}_replicates"] = int(kept.size)
    return out
