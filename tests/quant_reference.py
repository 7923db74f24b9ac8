"""numpy float32 restatement of the row-wise int8 record format (``include/deepfm_hip.h``: DFM_QUANT_INT8_ROWWISE),
written from its specification and sharing no code with the package: quantise, pack, unpack, dequantise.  Every step
is one float32 operation on float32 operands, so the kernels' results can be compared bit for bit."""
import numpy as np

HEADER = 16
F32 = np.float32


def row_bytes(dim: int) -> int:
    return HEADER + dim


def quantize(x):
    """x (rows, D) float32 -> (scale (rows,), lo (rows,), q (rows, D) uint8).  Rows must be finite."""
    x = np.ascontiguousarray(x, dtype=F32)
    lo = x.min(axis=1)
    hi = x.max(axis=1)
    with np.errstate(over="ignore"):
        scale = ((hi - lo).astype(F32) / F32(255.0)).astype(F32)
    safe = np.where(scale == 0, F32(1), scale).astype(F32)
    t = ((x - lo[:, None]).astype(F32) / safe[:, None]).astype(F32)
    q = np.minimum(np.rint(t), F32(255.0))                 # np.rint rounds half to even
    q = np.where(scale[:, None] == 0, F32(0), q)
    return scale, lo.astype(F32), q.astype(np.uint8)


def dequantize(scale, lo, q):
    """x' = fl(fl(q * scale) + lo): two float32 roundings."""
    prod = (q.astype(F32) * np.asarray(scale, F32)[:, None]).astype(F32)
    return (prod + np.asarray(lo, F32)[:, None]).astype(F32)


def pack(scale, lo, w1, q):
    """(rows, 16 + D) uint8 records: [scale | lo | w1 | 0 | q]."""
    rows, dim = q.shape
    rec = np.zeros((rows, HEADER + dim), np.uint8)
    head = np.zeros((rows, 4), F32)
    head[:, 0], head[:, 1], head[:, 2] = scale, lo, np.asarray(w1, F32).reshape(rows)
    rec[:, :HEADER] = head.view(np.uint8)
    rec[:, HEADER:] = q
    return rec


def unpack(rec):
    """(scale, lo, w1, pad, q) of (rows, 16 + D) uint8 records."""
    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    head = rec[:, :HEADER].copy().view(F32)
    return head[:, 0], head[:, 1], head[:, 2], head[:, 3], rec[:, HEADER:]


def quantize_table(w2, w1):
    """Records of a table (V, D) with its first-order weights (V,) or (V, 1)."""
    scale, lo, q = quantize(w2)
    return pack(scale, lo, w1, q)


def dequantize_table(rec):
    """(w2' (V, D), w1 (V, 1)) of records."""
    scale, lo, w1, _, q = unpack(rec)
    return dequantize(scale, lo, q), w1.reshape(-1, 1).copy()


def bound(x):
    """Per row: scale / 2 + 2**-21 * max(|lo|, |hi|) in float64, from the row's own float32 scale."""
    x = np.asarray(x, dtype=F32)
    scale, lo, _ = quantize(x)
    hi = x.max(axis=1)
    return scale.astype(np.float64) / 2 + 2.0 ** -21 * np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64)
