"""numpy / dict restatement of the reference's three feature transforms (``deepfm/data/transforms.py``), of the
``min_count`` / ``max_vocab`` pruning and of the 64-bit mixer of ``include/deepfm_hip.h``, written from their
specification and sharing no code with the package.  ``tests/golden/encoders_reference.npz`` holds what the
reference's own classes give on the same inputs (``tools/make_encoders_golden.py``)."""
from __future__ import annotations

from collections import Counter

import numpy as np

_M64 = (1 << 64) - 1


def mix64(x: int) -> int:
    """The mixer of include/deepfm_hip.h on one value, in Python integers."""
    x &= _M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & _M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & _M64
    x ^= x >> 33
    return x


def mix64_array(keys: np.ndarray) -> np.ndarray:
    """The same over an int64 array, in wrapping uint64 arithmetic."""
    x = np.asarray(keys, np.int64).view(np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return x


def hashed(keys: np.ndarray, num_buckets: int) -> np.ndarray:
    return (np.uint64(1) + mix64_array(keys) % np.uint64(num_buckets)).astype(np.int64)


def fit_vocabulary(values, min_count: int = 1, max_vocab=None):
    """(kept keys ascending, their counts): keys seen at least ``min_count`` times, of those the ``max_vocab`` most
    frequent, ties to the smaller key.  With the defaults: ``sorted(set(values))`` (transforms.py:15)."""
    counts = Counter(int(v) for v in np.asarray(values).reshape(-1))
    kept = [k for k, c in counts.items() if c >= min_count]
    if max_vocab is not None and len(kept) > max_vocab:
        kept = sorted(kept, key=lambda k: (-counts[k], k))[:max_vocab]
    kept = sorted(kept)
    return np.array(kept, np.int64), np.array([counts[k] for k in kept], np.int64)


def label_transform(keys: np.ndarray, values) -> np.ndarray:
    """transforms.py:17 and :20-23: key i of the ascending ``keys`` is i + 1, anything else 0."""
    mapping = {int(k): i + 1 for i, k in enumerate(keys)}
    return np.array([mapping.get(int(v), 0) for v in np.asarray(values).reshape(-1)], np.int64)


def valid_tokens(tokens: np.ndarray, lengths) -> list:
    """The token lists a padded matrix + lengths stands for."""
    tokens = np.asarray(tokens)
    n, w = tokens.shape
    lengths = np.full(n, w) if lengths is None else np.clip(np.asarray(lengths), 0, w)
    return [[int(t) for t in tokens[i, :lengths[i]]] for i in range(n)]


def multihot_transform(keys: np.ndarray, tokens: np.ndarray, lengths, max_length: int) -> np.ndarray:
    """transforms.py:65-71."""
    mapping = {int(k): i + 1 for i, k in enumerate(keys)}
    lists = valid_tokens(tokens, lengths)
    out = np.zeros((len(lists), max_length), np.int64)
    for i, toks in enumerate(lists):
        idx = [mapping.get(t, 0) for t in toks]
        m = min(len(idx), max_length)
        out[i, :m] = idx[:m]
    return out


def minmax_fit(values):
    v = np.asarray(values, np.float64)
    return float(v.min()), float(v.max())


def minmax_transform(lo: float, hi: float, values) -> np.ndarray:
    """transforms.py:44-49, in float64."""
    v = np.asarray(values, np.float64)
    denom = hi - lo
    if denom == 0:
        return np.zeros_like(v)
    with np.errstate(over="ignore", invalid="ignore"):
        return (v - lo) / denom
