"""The calibration contract restated in numpy (the yardstick of tests/test_*_calibration.py), from the definitions in
include/deepfm_hip.h.

A sample is used unless its slice id is outside [0, num_slices) (with slices), its score is NaN, its score is outside
[0, 1] (-0.0 is inside) or its label is other than exactly 0 or 1; each of the four is counted on its own and a sample
with any of them enters nothing else.  For a used sample with float32 score p and label y, K bins:

    bin = min(K - 1, int(float32(p) * float32(K)))          float32 product
    P   = rint(float64(p) * 2^32)
    Q   = rint((float64(p) - y)^2 * 2^32)
    L   = rint(l * 2^27),  l = -log(float64(clip(t, eps, 1 - eps))), t = p' or float32(1) - p' for y = 1 / 0,
          p' = clip(p, float32(1e-7), float32(1 - 1e-7)), eps = 2^-23: all float32 up to the logarithm

Every sum is an int64 sum; the finish is fp64 in the stated order (``ece`` adds the gaps one by one, ascending).
"""
import numpy as np

P_UNIT = 2.0 ** -32
L_UNIT = 2.0 ** -27


def sample_logloss(scores, positive):
    """fp64 per-sample log loss of float32 scores, as the pooled log loss of the device metrics forms it."""
    s = np.asarray(scores, np.float32)
    lo, hi = np.float32(1e-7), np.float32(1.0 - 1e-7)
    eps = np.float32(1.1920928955078125e-07)
    p = np.minimum(np.maximum(s, lo), hi)
    q = np.float32(1.0) - p
    t = np.where(positive, p, q).astype(np.float32)
    t = np.minimum(np.maximum(t, eps), np.float32(1.0) - eps)
    return -np.log(t.astype(np.float64))


def integers(labels, scores, bins, slice_ids=None, num_slices=0):
    """The integer sums: dict(glob = [N, positives, sum P, sum Q, sum L], bins (K, 3), slices (S, 4) or None, faults =
    [bad ids, NaN scores, out-of-range scores, bad labels]), all int64."""
    y = np.asarray(labels, np.float32).reshape(-1)
    p = np.asarray(scores, np.float32).reshape(-1)
    K = int(bins)
    with np.errstate(invalid="ignore"):
        nan = np.isnan(p)
        out_of_range = ~nan & ~((p >= 0) & (p <= 1))
        bad_label = ~((y == 0) | (y == 1))
    bad_id = np.zeros(p.size, bool)
    if slice_ids is not None:
        sid = np.asarray(slice_ids, np.int64).reshape(-1)
        bad_id = (sid < 0) | (sid >= num_slices)
    ok = ~(bad_id | nan | out_of_range | bad_label)
    y, p = y[ok], p[ok]
    pos = y == 1
    pd = p.astype(np.float64)
    d = pd - pos.astype(np.float64)
    P = np.rint(pd * 2.0 ** 32).astype(np.int64)
    Q = np.rint(d * d * 2.0 ** 32).astype(np.int64)
    L = np.rint(sample_logloss(p, pos) * 2.0 ** 27).astype(np.int64)
    b = np.minimum(K - 1, (p * np.float32(K)).astype(np.int32)).astype(np.int64)
    assert (p * np.float32(K)).dtype == np.float32
    ones = np.ones(p.size, np.int64)
    posi = pos.astype(np.int64)

    def table(index, size, columns):
        t = np.zeros((size, len(columns)), np.int64)
        for j, col in enumerate(columns):
            np.add.at(t[:, j], index, col)
        return t

    out = dict(glob=np.array([p.size, posi.sum(), P.sum(), Q.sum(), L.sum()], np.int64),
               bins=table(b, K, [ones, posi, P]), slices=None,
               faults=np.array([bad_id.sum(), nan.sum(), out_of_range.sum(), bad_label.sum()], np.int64))
    if slice_ids is not None:
        out["slices"] = table(sid[ok], int(num_slices), [ones, posi, P, L])
    return out


def calibration(labels, scores, bins=10, slice_ids=None, num_slices=None):
    """dict(out (12,), bins (K, 3), slices (S, 4) or None) as float64, as ``dfm_calibration`` writes them; ``ints``
    holds the integer sums."""
    if slice_ids is not None and num_slices is None:
        num_slices = int(np.max(slice_ids)) + 1
    ints = integers(labels, scores, bins, slice_ids, num_slices or 0)
    N, npos, sp, sq, sl = (int(v) for v in ints["glob"])
    bt = ints["bins"].astype(np.float64)                  # int64 -> float64 rounds to nearest even
    bt[:, 2] = bt[:, 2] * P_UNIT
    gap = np.abs(bt[:, 2] - bt[:, 1])
    total, worst = 0.0, -1.0
    for g, c in zip(gap.tolist(), bt[:, 0].tolist()):
        total = total + g
        if c > 0:
            worst = max(worst, g / c)
    nan = float("nan")
    fn = np.float64(N)
    out = np.array([N, npos,
                    np.float64(sp) * P_UNIT / fn if N else nan, np.float64(sq) * P_UNIT / fn if N else nan,
                    np.float64(sl) * L_UNIT / fn if N else nan, np.float64(total) / fn if N else nan,
                    worst if N else nan, *ints["faults"].tolist(), 0.0], np.float64)
    st = None
    if ints["slices"] is not None:
        st = ints["slices"].astype(np.float64)
        st[:, 2] = st[:, 2] * P_UNIT
        st[:, 3] = st[:, 3] * L_UNIT
    return dict(out=out, bins=bt, slices=st, ints=ints)


def summary(result):
    """The floats the package's ``calibration_dict`` gives for ``result["out"]`` (written out independently)."""
    N, npos, mean_pred, brier, logloss, ece, mce = result["out"][:7].tolist()
    rate = npos / N
    d = {"mean_pred": mean_pred, "base_rate": rate, "brier": brier, "ece": ece, "mce": mce}
    if npos:
        d["copc"] = mean_pred * N / npos
    if 0 < npos < N:
        d["ne"] = logloss / -(rate * np.log(rate) + (1 - rate) * np.log(1 - rate))
    return d
