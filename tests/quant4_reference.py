"""numpy restatement of the row-wise 4-bit record format (``include/deepfm_hip.h``: DFM_QUANT_UINT4_ROWWISE), written
from its specification and sharing no code with the package: quantise, pack, unpack, dequantise.  Every step is one
float32 operation on float32 operands, the two header fields are binary16 by a round-to-nearest conversion and
``np.nextafter`` steps (one exact float64 comparison decides the last), so the kernels' results can be compared bit
for bit."""
import numpy as np

HEADER = 8
LEVELS = 15
F32 = np.float32
F16 = np.float16


def row_bytes(dim: int) -> int:
    return HEADER + dim // 2


def half_floor(v):
    """The largest binary16 value <= v (float32 array); -inf where there is none."""
    v = np.asarray(v, F32)
    with np.errstate(over="ignore"):
        h = v.astype(F16)
        return np.where(h.astype(F32) > v, np.nextafter(h, F16(-np.inf)), h).astype(F16)


def half_ceil(v):
    """The smallest binary16 value >= v (float32 array); +inf where there is none."""
    v = np.asarray(v, F32)
    with np.errstate(over="ignore"):
        h = v.astype(F16)
        return np.where(h.astype(F32) < v, np.nextafter(h, F16(np.inf)), h).astype(F16)


def quantize(x):
    """x (rows, D) float32 -> (scale (rows,) float16, lo (rows,) float16, q (rows, D) uint8 in 0..15, bad (rows,)).
    ``bad`` marks the rows the format refuses: a non-finite element, a minimum or a scale beyond binary16; their
    other outputs mean nothing."""
    x = np.ascontiguousarray(x, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lo_h = half_floor(x.min(axis=1))
        lo = lo_h.astype(F32)
        rng = (x.max(axis=1) - lo).astype(F32)
        scale_h = half_ceil((rng / F32(LEVELS)).astype(F32))
        # both float32 roundings can go down: where lo + 15 scale < hi, exactly (float64 holds the terms), one step up
        short = lo.astype(np.float64) + LEVELS * scale_h.astype(np.float64) < x.max(axis=1).astype(np.float64)
        scale_h = np.where(short, np.nextafter(scale_h, F16(np.inf)), scale_h).astype(F16)
        scale = scale_h.astype(F32)
        bad = ~np.isfinite(x).all(axis=1) | np.isinf(lo_h) | np.isinf(scale_h)
        safe = np.where(scale == 0, F32(1), scale).astype(F32)
        t = ((x - lo[:, None]).astype(F32) / safe[:, None]).astype(F32)
        q = np.minimum(np.rint(t), F32(LEVELS))                # np.rint rounds half to even
        q = np.where((scale[:, None] == 0) | bad[:, None], F32(0), q)
    return scale_h, lo_h, q.astype(np.uint8), bad


def dequantize(scale, lo, q):
    """x' = fl(fl(q * scale) + lo): two float32 roundings on the widened binary16 header."""
    s = np.asarray(scale, F16).astype(F32)[:, None]
    prod = (q.astype(F32) * s).astype(F32)
    return (prod + np.asarray(lo, F16).astype(F32)[:, None]).astype(F32)


def pack(scale, lo, w1, q):
    """(rows, 8 + D / 2) uint8 records: [scale f16 | lo f16 | w1 f32 | q, element j in byte j / 2, low nibble first]."""
    rows, dim = q.shape
    rec = np.zeros((rows, HEADER + dim // 2), np.uint8)
    rec[:, 0:2] = np.asarray(scale, F16).reshape(rows, 1).view(np.uint8)
    rec[:, 2:4] = np.asarray(lo, F16).reshape(rows, 1).view(np.uint8)
    rec[:, 4:8] = np.ascontiguousarray(np.asarray(w1, F32).reshape(rows, 1)).view(np.uint8)
    q = q.astype(np.uint8)
    rec[:, HEADER:] = (q[:, 0::2] & 15) | ((q[:, 1::2] & 15) << 4)
    return rec


def unpack(rec):
    """(scale f16, lo f16, w1 f32, q (rows, D) uint8) of (rows, 8 + D / 2) uint8 records."""
    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    rows = rec.shape[0]
    scale = rec[:, 0:2].copy().view(F16)[:, 0]
    lo = rec[:, 2:4].copy().view(F16)[:, 0]
    w1 = rec[:, 4:8].copy().view(F32)[:, 0]
    pay = rec[:, HEADER:]
    q = np.empty((rows, 2 * pay.shape[1]), np.uint8)
    q[:, 0::2] = pay & 15
    q[:, 1::2] = pay >> 4
    return scale, lo, w1, q


def quantize_table(w2, w1):
    """Records of a table (V, D) with its first-order weights (V,) or (V, 1).  Rows must be quantisable."""
    scale, lo, q, bad = quantize(w2)
    assert not bad.any(), "quantize_table: a row the format refuses"
    return pack(scale, lo, w1, q)


def dequantize_table(rec):
    """(w2' (V, D), w1 (V, 1)) of records."""
    scale, lo, w1, q = unpack(rec)
    return dequantize(scale, lo, q), w1.reshape(-1, 1).copy()


def bound(x):
    """Per row: scale / 2 + 2**-21 * max(|lo|, |lo + 15 scale|) in float64, from the row's own binary16 header."""
    scale, lo, _, _ = quantize(np.asarray(x, dtype=F32))
    scale, lo = scale.astype(np.float64), lo.astype(np.float64)
    return scale / 2 + 2.0 ** -21 * np.maximum(np.abs(lo), np.abs(lo + LEVELS * scale))
