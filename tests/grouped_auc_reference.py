"""The grouped-AUC contract restated in numpy (the yardstick of tests/test_*_grouped_auc.py).

For a group g with P_g labels 1 and N_g labels 0 (it qualifies when both are > 0):

    W_g, T_g = its (positive, negative) pairs with s_pos > s_neg, s_pos == s_neg   (float32 order, -0.0 == +0.0)
    auc_g    = float64(2 W_g + T_g) / float64(2 P_g N_g)                           (integers, converted once each)
    gauc     = sum (P_g + N_g) auc_g / sum (P_g + N_g),   uauc = mean auc_g         over the qualifying groups

The integers come from ``searchsorted`` on the order keys of the scores.  The two fp64 sums run over the group ids in
the fixed tree that ``csrc/grouped_auc.hip`` documents (``tree_sum``), so the results can be compared bit for bit.
Samples with an id outside [0, num_groups), a NaN score or a label other than 0 / 1 are counted and not used.
"""
import numpy as np

LEAVES = 256           # leaves per workgroup
BLOCKS = 1024          # workgroups, whatever the number of groups


def ord_bits(scores):
    """Order-preserving uint32 keys of float32 scores: a < b <=> ord(a) < ord(b); -0.0 maps as +0.0."""
    s = np.asarray(scores, np.float32).copy()
    s[s == 0] = 0.0
    b = s.view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _halving(x):
    """x (rows, 256) float64 -> (rows,): x[t] += x[t + s] for s = 128 .. 1."""
    x = x.copy()
    s = LEAVES // 2
    while s:
        x[:, :s] = x[:, :s] + x[:, s:2 * s]
        s //= 2
    return x[:, 0]


def _strided(v, leaves):
    """Leaf l adds v[l], v[l + leaves], ... in that order, starting from 0.0."""
    rounds = -(-v.size // leaves)
    padded = np.zeros(rounds * leaves, np.float64)
    padded[:v.size] = v
    acc = np.zeros(leaves, np.float64)
    for row in padded.reshape(rounds, leaves):
        acc = acc + row
    return acc


def tree_sum(terms):
    """The fixed fp64 tree over per-group terms (0.0 for a group that does not qualify)."""
    terms = np.asarray(terms, np.float64)
    per_block = _halving(_strided(terms, BLOCKS * LEAVES).reshape(BLOCKS, LEAVES))
    return float(_halving(_strided(per_block, LEAVES).reshape(1, LEAVES))[0])


def group_integers(group_ids, labels, scores, num_groups):
    """(numerator 2W + T, P, N) per group as Python-int object arrays / int64 arrays, and the three invalid counts."""
    g = np.asarray(group_ids, np.int64).reshape(-1)
    y = np.asarray(labels, np.float32).reshape(-1)
    s = np.asarray(scores, np.float32).reshape(-1)
    bad_id = (g < 0) | (g >= num_groups)
    nan = np.isnan(s)
    bad_label = (y != 0) & (y != 1)
    ok = ~(bad_id | nan | bad_label)
    g, y, k = g[ok], y[ok], ord_bits(s[ok]).astype(np.int64)
    num = np.zeros(num_groups, object)
    num[:] = 0
    P = np.zeros(num_groups, np.int64)
    N = np.zeros(num_groups, np.int64)
    order = np.argsort(g, kind="stable")
    bounds = np.flatnonzero(np.diff(g[order])) + 1
    for idx in np.split(order, bounds) if g.size else []:
        gid = int(g[idx[0]])
        neg = np.sort(k[idx][y[idx] == 0])
        pos = k[idx][y[idx] == 1]
        below = np.searchsorted(neg, pos, side="left")
        upto = np.searchsorted(neg, pos, side="right")
        num[gid] = int(2 * below.sum(dtype=np.int64) + (upto - below).sum(dtype=np.int64))
        P[gid], N[gid] = pos.size, neg.size
    return num, P, N, (int(bad_id.sum()), int(nan.sum()), int(bad_label.sum()))


def grouped_auc(group_ids, labels, scores, num_groups=None):
    """dict(groups, gauc, uauc, samples, per_group (NaN where a group does not qualify), bad_id, nan, bad_label)."""
    if num_groups is None:
        num_groups = int(np.max(group_ids)) + 1
    num, P, N, (bad_id, nan, bad_label) = group_integers(group_ids, labels, scores, num_groups)
    keep = (P > 0) & (N > 0)
    per_group = np.full(num_groups, np.nan)
    for gid in np.flatnonzero(keep):
        per_group[gid] = float(num[gid]) / float(2 * int(P[gid]) * int(N[gid]))   # int -> float rounds to nearest
    auc0 = np.where(keep, per_group, 0.0)
    weight = np.where(keep, P + N, 0).astype(np.float64)
    groups, samples = int(keep.sum()), int(weight.sum())
    out = dict(groups=groups, samples=samples, per_group=per_group, bad_id=bad_id, nan=nan, bad_label=bad_label,
               gauc=float("nan"), uauc=float("nan"))
    if groups:
        out["gauc"] = tree_sum(weight * auc0) / float(samples)
        out["uauc"] = tree_sum(auc0) / float(groups)
    return out


def brute_force_numerator(labels, scores):
    """2W + T of one group by the O(P N) double loop, comparing as float32."""
    y = np.asarray(labels, np.float32)
    s = np.asarray(scores, np.float32)
    total = 0
    for sp in s[y == 1]:
        for sn in s[y == 0]:
            total += 2 if sp > sn else (1 if sp == sn else 0)
    return total
