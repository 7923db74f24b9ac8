"""Cases, seeded inputs and fp64 references of the d-input epilogues of dfm_linear_backward (csrc/tower.hip:
bn_mask_tile and the FM branch of dx_tile_epilogue), shared by tests/test_cpu_linear_bwd_epilogue_reference.py (which
holds a plain fp32 restatement of the epilogues to the same bars on the host) and
tests/test_gpu_linear_bwd_epilogue.py (which runs the kernels).  Plain numpy; no GPU and no library needed.

The epilogues read their operands (z; g_fm, S, e; the addend) for all 16 accumulator rows of a lane from addresses
whose row is clamped to M - 1, then compute and store under the row test.  So the cases walk the last tile's row
count rather than the contraction: N = 8 (one short k slice), M = 1 (every clamped row is row 0), 2, 33 (1 valid row
in the second 32-row MFMA tile), 63, 65 and 129 (a second / third workgroup row with one valid row), on widths of
the fast operand route (4, 60, 68: one lane quad, a partly and a fully filled second column tile) and of the
checked route (1, 33, 67)."""
from __future__ import annotations

import functools

import numpy as np

from tests import tower_cases as TC
from tests.helpers import tower_bn_relu_fp64, tower_linear_backward_fp64, tower_masked_grad_fp64

N_UP = 8                                   # out_features of the Linear above: the d-input contraction
M_ALL = (1, 2, 33, 63, 65, 129)
K_FAST = (4, 60, 68)
K_CHECKED = (1, 33, 67)
K_DIM16 = 64                               # 16 divides none of K_FAST: one more fast width for the FM dim = 16 cases
DROPOUT_P = 0.25
SEED, SALT = 20240607, 3

SHAPES = [(M, K) for K in K_FAST + K_CHECKED + (K_DIM16,) for M in M_ALL]


def fm_dims(K):
    if K % 2:
        return (1,)
    return tuple(d for d in (4, 16) if K % d == 0)


def epilogues(K):
    """(name, FM dim, dropout p) of every epilogue variant run at width K."""
    out = [] if K == K_DIM16 else [("bn", 0, 0.0), ("bn", 0, DROPOUT_P), ("fm_a", 1, 0.0)]
    for d in fm_dims(K):
        if K == K_DIM16 or d != 16:
            out += [("fm_g", d, 0.0), ("fm_ga", d, 0.0)]
    return out


def route(K) -> str:
    return "fast" if K % 4 == 0 else "checked"          # N_UP % 4 == 0; gemm::operand_fast restated


@functools.lru_cache(maxsize=None)
def fm_sum(M, dim):
    """S (M, dim): the FM layer's sum over the fields."""
    return np.random.default_rng([6, M, dim]).standard_normal((M, dim)).astype(np.float32)


def keep_mask(seed, salt, count, p):
    """dropout.h restated: element i is kept when mix32(seed * golden + (salt << 40) + i) >= p * 2^32."""
    if p <= 0.0:
        return np.ones(count, dtype=bool)
    m = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        x = (np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + (np.uint64(salt) << np.uint64(40))
             + np.arange(count, dtype=np.uint64)) & m
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return (x & np.uint64(0xFFFFFFFF)) >= np.uint64(int(p * 4294967296.0))


def reference(M, K, epi, dim, p):
    """fp64: the d-input result (M, K) and, for bn, the [T][2][K] per-tile column sums of dy and dy * xhat."""
    i = TC.backward_inputs(M, N_UP, K)
    g, a = epi in ("fm_g", "fm_ga"), epi in ("fm_a", "fm_ga")
    _, dx = tower_linear_backward_fp64(i["dz"], i["x"], i["w"], i["g_fm"] if g else None,
                                       fm_sum(M, dim) if g else None, i["x"] if g else None,
                                       i["addend"] if a else None)
    if epi != "bn":
        return dx, None
    bn = TC.bn_inputs(M, K)
    mean, rstd = bn["stats"].astype(np.float64)
    xhat, y, _ = tower_bn_relu_fp64(bn["z"], mean, rstd, bn["gamma"], bn["beta"])
    dy = tower_masked_grad_fp64(dx, y) * keep_mask(SEED, SALT, M * K, p).reshape(M, K) / (1.0 - p)
    T = (M + 31) // 32
    part = np.zeros((T, 2, K))
    for t in range(T):
        rows = slice(32 * t, min(32 * t + 32, M))
        part[t, 0], part[t, 1] = dy[rows].sum(0), (dy[rows] * xhat[rows]).sum(0)
    return dy, part
