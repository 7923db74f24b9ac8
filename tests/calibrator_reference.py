"""numpy restatement of the score calibrators (``csrc/calibrator.hip``), written from their specification in
``include/deepfm_hip.h`` and sharing no code with the package: an fp64 Newton for Platt scaling, the integer logit
histogram, an integer pool-adjacent-violators, and the float32 apply written operation by operation."""
import numpy as np

F32 = np.float32


# ----------------------------------------------------------------------------- data
# (base rate, true a, true b, seed): the model's logits z are such that sigmoid(a z + b) is the true probability
CASES = [(0.005, 0.2, 0.0, 11), (0.02, 0.5, -0.5, 12), (0.3, 1.5, 0.25, 13), (0.4, 2.0, -1.0, 14), (0.5, 3.0, 1.0, 15)]


def synthetic(case, n):
    """(labels, logits) float32 of one of CASES: true logits u ~ N(logit(rate), 1.5), y ~ Bernoulli(sigmoid(u)), and
    the model's logit z = (u - b) / a, so that the fit should find about (a, b)."""
    rate, a, b, seed = case
    rng = np.random.default_rng(seed)
    u = rng.normal(np.log(rate / (1.0 - rate)), 1.5, n)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-u))).astype(F32)
    return y, ((u - b) / a).astype(F32)


SEPARABLE = (np.array([0, 0, 1, 1], F32), np.array([-2.0, -1.0, 1.0, 2.0], F32))


def faults(y, z):
    """(non-finite logits, labels other than 0 / 1, mask of the usable samples)."""
    z_bad = ~np.isfinite(z)
    y_bad = ~((y == 0) | (y == 1))
    return int(z_bad.sum()), int(y_bad.sum()), ~(z_bad | y_bad)


# ----------------------------------------------------------------------------- Platt
def platt_targets(y, smooth):
    y = np.asarray(y, np.float64)
    if not smooth:
        return y
    npos, nneg = float((y == 1).sum()), float((y == 0).sum())
    return np.where(y == 1, (npos + 1.0) / (npos + 2.0), 1.0 / (nneg + 2.0))


def platt_terms(a, b, z, t):
    """(F, g (2,), H (2, 2)) of the mean objective at (a, b), fp64."""
    z = np.asarray(z, np.float64)
    s = a * z + b
    e = np.exp(-np.abs(s))
    q = np.where(s >= 0, 1.0, e) / (1.0 + e)
    w = e / (1.0 + e) ** 2
    F = np.mean(np.log1p(e) + np.maximum(s, 0.0) - t * s)
    r = q - t
    g = np.array([np.mean(r * z), np.mean(r)])
    H = np.array([[np.mean(w * z * z), np.mean(w * z)], [np.mean(w * z), np.mean(w)]])
    return F, g, H


def platt_logloss(a, b, z, y):
    return platt_terms(a, b, z, np.asarray(y, np.float64))[0]


def platt_newton(y, z, fit_slope=True, smooth=False, gtol=1e-13, max_iter=200):
    """(a, b, iterations): Newton with step halving in fp64 from (1, 0) until max |g| <= gtol."""
    t = platt_targets(y, smooth)
    p = np.array([1.0, 0.0])
    F, g, H = platt_terms(p[0], p[1], z, t)
    for it in range(max_iter):
        if (np.abs(g).max() if fit_slope else abs(g[1])) <= gtol:
            return p[0], p[1], it
        d = -np.linalg.solve(H, g) if fit_slope else np.array([0.0, -g[1] / H[1, 1]])
        step = 1.0
        while True:
            cand = p + step * d
            Fc, gc, Hc = platt_terms(cand[0], cand[1], z, t)
            if Fc <= F or step < 1e-10:
                break
            step *= 0.5
        p, F, g, H = cand, Fc, gc, Hc
    return p[0], p[1], max_iter


def platt_apply_fp64(a, b, z):
    return 1.0 / (1.0 + np.exp(-(np.float64(a) * np.asarray(z, np.float64) + np.float64(b))))


# ----------------------------------------------------------------------------- isotonic
def histogram(y, z, bins, z_lo=-16.0, z_hi=16.0):
    """The (bins, 3) int64 table [count, positives, sum of rint(z_c * 2^24)] over the usable samples, and the header
    [used, positives, non-finite logits, labels other than 0 / 1]."""
    y, z = np.asarray(y, F32), np.asarray(z, F32)
    z_bad, y_bad, ok = faults(y, z)
    y, z = y[ok], z[ok]
    lo, hi = F32(z_lo), F32(z_hi)
    scale = F32(np.float64(bins) / (np.float64(hi) - np.float64(lo)))
    zc = np.minimum(np.maximum(z, lo), hi)                    # float32
    prod = (zc - lo) * scale                                  # two float32 roundings
    assert prod.dtype == F32
    idx = np.minimum(prod.astype(np.int64), bins - 1)         # truncation, as (int)
    zfix = np.rint(zc.astype(np.float64) * 16777216.0).astype(np.int64)
    table = np.zeros((bins, 3), np.int64)
    np.add.at(table[:, 0], idx, 1)
    np.add.at(table[:, 1], idx, (y == 1).astype(np.int64))
    np.add.at(table[:, 2], idx, zfix)
    return table, [int(ok.sum()), int((y == 1).sum()), z_bad, y_bad]


def pav(table):
    """(x, v, blocks): fp64 knots of the non-empty bins and their fitted values, by pool-adjacent-violators over exact
    integers: neighbours are pooled only on a strict decrease, decided by cross-multiplication."""
    rows = [(int(c), int(p), int(s)) for c, p, s in table if c > 0]
    stack = []                                                # [positives, count, knots]
    for c, p, _ in rows:
        blk = [p, c, 1]
        while stack and stack[-1][0] * blk[1] > blk[0] * stack[-1][1]:
            top = stack.pop()
            blk = [top[0] + blk[0], top[1] + blk[1], top[2] + blk[2]]
        stack.append(blk)
    v = np.array([float(p) / float(c) for p, c, k in stack for _ in range(k)], np.float64)
    x = np.array([(float(s) * 2.0 ** -24) / float(c) for c, _, s in rows], np.float64)
    return x, v, len(stack)


def isotonic_apply(x, v, z):
    """The float32 apply, operation by operation, on the float32 roundings of the fp64 knots."""
    x32, v32, z = np.asarray(x).astype(F32), np.asarray(v).astype(F32), np.asarray(z, F32)
    m = x32.size
    if m == 0:
        with np.errstate(over="ignore"):
            return (F32(1) / (F32(1) + np.exp(-z))).astype(F32)
    lo = np.clip(np.searchsorted(x32, z, side="right") - 1, 0, max(m - 2, 0))
    hi = np.minimum(lo + 1, m - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (z - x32[lo]) / (x32[hi] - x32[lo])               # float32 throughout
        q = np.minimum(v32[lo] + t * (v32[hi] - v32[lo]), v32[hi])
    assert q.dtype == F32
    q = np.where(z <= x32[0], v32[0], q)
    q = np.where(z >= x32[m - 1], v32[m - 1], q)
    return np.where(np.isnan(z), F32(np.nan), q).astype(F32)
