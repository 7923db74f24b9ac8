"""Cases and seeded inputs of the tower matrix, shared by tests/test_cpu_tower_reference.py (which proves on the
host that each case reaches the loop phase it claims and keeps its distance from the ReLU kink) and
tests/test_gpu_tower_matrix.py (which runs them).  Plain numpy; no GPU and no library needed to import this."""
from __future__ import annotations

import functools

import numpy as np

from tests.helpers import tower_column_stats_fp64, tower_dw_split_plan

# Contraction lengths of gemm::mainloop (32-deep slices; prologue slices 0-3 then 4-5; the unchecked steady loop
# runs while k0 + 320 <= ke; checked tail in groups of four).  Fast route: multiples of 4.  What each length pins:
#   4, 28          less than one slice                     32 .. 192   exactly 1 .. 6 slices (prologue slots)
#   36, 100, 132, 196   partial last slice at tail position 1, 3, 0 (second group), 2
#   224, 288       7 and 9 slices: the checked loop alone, three groups
#   316 / 320 / 324    last length without, first lengths with one steady iteration
#   352            steady + 1 tail group                   448 / 452   two steady iterations (+ a 4-wide tail)
K_FAST = (4, 28, 32, 36, 64, 96, 100, 128, 132, 160, 192, 196, 224, 288, 316, 320, 324, 352, 448, 452)
K_CHECKED = (1, 31, 33, 65, 127, 129, 161, 319, 321, 449)
KINK_MARGIN = 1e-4               # min |gamma xhat + beta| of every case that pushes a gradient through a ReLU mask
EPS, MOMENTUM = 1e-5, 0.1

# ---- forward: (M, N, K, variant, bias).  variant: plain | x_off | w_off (pointer + 4 bytes) | ldx4 | ldx1 -------
FWD_CASES = (
    [(70, 68, k, "plain", True) for k in K_FAST + K_CHECKED]
    + [(70, 68, k, v, True) for k in (64, 320) for v in ("x_off", "ldx4", "ldx1")]
    + [(70, 68, 64, "w_off", True), (70, 68, 64, "plain", False), (70, 68, 33, "plain", False),
       (70, 68, 320, "plain", False)]
    + [(m, n, 36, "plain", True) for m in (2, 63, 64, 65, 70) for n in (4, 63, 64, 68) if (m, n) != (70, 68)]
)


def fwd_route(case) -> str:
    """The operand route the case must take (gemm::operand_fast restated: alignment, ld % 4, K % 4)."""
    M, N, K, variant, _ = case
    ldx = K + {"ldx4": 4, "ldx1": 1}.get(variant, 0)
    return "fast" if (K % 4 == 0 and ldx % 4 == 0 and variant not in ("x_off", "w_off")) else "checked"


# ---- apply kernels: column tiles of 64 (okc lanes), row-lane merge trip counts T = ceil(M / 32) ----------------
APPLY_N = (4, 60, 64, 68, 132)
APPLY_M = (2, 31, 32, 33, 512, 513, 1056)          # T = 1, 1, 1, 2, 16, 17, 33; M % 32 = 2, 31, 0, 1, 0, 1, 0
APPLY_UP = 8                                        # out_features of the Linear above (the dx contraction)

# ---- head: features / 32 = 1 .. 8 ---------------------------------------------------------------------------
HEAD_CH = tuple(range(1, 9))
HEAD_M = (1, 31, 32, 33, 545)


def head_nulls(ch: int, M: int):
    """Which optional pointers a head case passes: (d_b, d_first_order, d_fm, g_b, g_b2) as booleans.  Over the
    matrix each is null and non-null several times per flavour; M = 33 rows have everything, M = 31 nothing."""
    i = ch + HEAD_M.index(M)
    if M == 33:
        return (True,) * 5
    if M == 31:
        return (False,) * 5
    return (i % 2 == 0, i % 3 != 0, i % 3 != 1, i % 2 == 1, i % 4 < 2)


# ---- backward, mode 0: (M, N, K, epi, variant, dw_phase) -------------------------------------------------------
# epi: plain | bn | fm_g | fm_a | fm_ga;  variant: plain | dz_off | x_off | w_off.
# dw_phase (proved from the restated plan by the CPU test):
#   one       one split, the whole batch            ragged    >= 2 splits, last one shorter, not a multiple of 32
#   sub32     a split of fewer than 32 rows         steady    >= 320 rows per split and >= 2 splits
#   sliceN    one split of exactly N full slices
BWD_STEADY = (1377, 8, 1156)      # cheapest M N K found with >= 320 rows per split and >= 2 splits: 352 x 3 + 321
BWD_CASES = (
    [(70, n, 68, "plain", "plain", "one") for n in K_FAST + K_CHECKED]
    + [(70, 64, 68, e, "plain", "one") for e in ("bn", "fm_g", "fm_a", "fm_ga")]
    + [(70, 33, 68, e, "plain", "one") for e in ("bn", "fm_ga")]                       # checked route, each epilogue
    + [(70, 64, 68, "plain", v, "one") for v in ("dz_off", "x_off", "w_off")]
    + [(70, 64, 67, "plain", "plain", "one"), (70, 64, 67, "bn", "plain", "one")]      # odd in_features: checked
    + [(32 * s, 8, 12, "plain", "plain", f"slice{s}") for s in range(1, 7)]
    + [(300, 8, 12, "plain", "plain", "ragged"), (300, 8, 12, "bn", "plain", "ragged"),
       (641, 8, 12, "plain", "plain", "sub32"), (20, 8, 12, "fm_ga", "plain", "sub32"),
       (250, 130, 68, "plain", "plain", "one"),        # 6 dW blocks (identity branch), 8 dx blocks (mapped from 6)
       (300, 130, 130, "bn", "plain", "ragged"),       # 18 dW blocks (16 mapped + 2), 15 dx blocks (8 mapped + 7)
       (*BWD_STEADY, "plain", "plain", "steady")]
)


def bwd_route(case) -> str:
    M, N, K, epi, variant, _ = case
    return "fast" if (N % 4 == 0 and K % 4 == 0 and variant == "plain") else "checked"


def dw_phase_holds(case) -> bool:
    M, N, K, _, _, phase = case
    splits, kps, rows = tower_dw_split_plan(N, K, M)
    if phase == "one":
        return splits == 1
    if phase == "ragged":
        return splits >= 2 and rows[-1] < kps and rows[-1] % 32 != 0
    if phase == "sub32":
        return min(rows) < 32
    if phase == "steady":
        return splits >= 2 and min(rows) >= 320
    if phase.startswith("slice"):
        return splits == 1 and rows[0] == 32 * int(phase[5:])
    raise ValueError(phase)


# ---- finish: splits through the one-output Linear (M = 64 s rows give s slabs) ---------------------------------
FINISH_SPLITS = (1, 7, 8, 9, 17)
FINISH_TOWER_SHAPE = (300, 4, 257)        # dW of 257 float4 in two splits: one float4 spills into a second workgroup

# ---- mode 1 (bf16 x 3): (M, N, K, epi) on the route; fallbacks (M, N, K, variant) must be mode 0 bit for bit ----
X3_CASES = [(2, 8, 68, "plain"), (62, 56, 68, "plain"), (64, 64, 68, "plain"), (66, 72, 68, "bn"),
            (130, 120, 68, "fm_ga"), (778, 128, 68, "plain"), (64, 136, 68, "plain"), (130, 200, 68, "plain")]
X3_FALLBACK = [(66, 60, 68, "plain"), (65, 64, 68, "plain"), (66, 64, 68, "w_off"), (66, 64, 68, "dz_off")]


def all_backward_shapes():
    """Every (M, N, K) the matrix hands to dfm_linear_backward (any mode)."""
    s = {c[:3] for c in BWD_CASES} | {c[:3] for c in X3_CASES} | {c[:3] for c in X3_FALLBACK}
    s |= {(m, APPLY_UP, n) for m in APPLY_M for n in APPLY_N} | {FINISH_TOWER_SHAPE}
    return sorted(s)


# ---- seeded inputs ------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


@functools.lru_cache(maxsize=None)
def linear_inputs(M, N, K):
    """x (M, K), w (N, K), b (N), gamma, beta (N) in fp32, seeded from the shape alone."""
    r = _rng(1, M, N, K)
    return dict(x=(r.standard_normal((M, K)) * 1.5 + 0.3).astype(np.float32),
                w=(r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32),
                b=r.standard_normal(N).astype(np.float32),
                gamma=r.uniform(0.5, 1.5, N).astype(np.float32),
                beta=(r.standard_normal(N) * 0.3).astype(np.float32))


@functools.lru_cache(maxsize=None)
def bn_inputs(M, N, tag=0):
    """A BatchNorm layer as its backward sees it: z (M, N), stats (2, N) = (mean, rstd) as the forward would have
    left them in fp32, gamma, beta.  Elements of z whose y = gamma xhat + beta falls within 2e-4 of the ReLU kink
    are moved to |y| = 1e-3 (the statistics are an input of the backward kernels and stay as they are), so the mask
    is the same in any arithmetic: the CPU test asserts min |y| >= KINK_MARGIN in fp64 for every such case."""
    r = _rng(2, M, N, tag)
    # Two rows: xhat = +-sigma / sqrt(sigma^2 + eps) and dz = gamma rstd (d1 - d2) / 2 * eps / (sigma^2 + eps).  At unit
    # variance that is a 1e-5 cancellation which fp32 cannot hold to 1e-4 (tower matrix findings);
    # a spread of the order of sqrt(eps) keeps the same code path well conditioned.
    spread = 3e-3 if M == 2 else 1.3
    z = (r.standard_normal((M, N)) * spread + 0.2).astype(np.float32)
    gamma = r.uniform(0.5, 1.5, N).astype(np.float32)
    beta = (r.standard_normal(N) * 0.3).astype(np.float32)
    mean, var = tower_column_stats_fp64(z)
    stats = np.stack([mean, 1.0 / np.sqrt(var + EPS)]).astype(np.float32)
    m64, r64, g64, b64 = (a.astype(np.float64) for a in (stats[0], stats[1], gamma, beta))
    for _ in range(4):
        y = g64 * (z.astype(np.float64) - m64) * r64 + b64
        near = np.abs(y) < 2e-4
        if not near.any():
            break
        target = np.where(y >= 0, 1e-3, -1e-3)
        moved = m64 + (target - b64) / (g64 * r64)
        z = np.where(near, moved, z.astype(np.float64)).astype(np.float32)
    return dict(z=z, stats=stats, gamma=gamma, beta=beta)


def bn_y_fp64(bn):
    z, (mean, rstd) = bn["z"].astype(np.float64), bn["stats"].astype(np.float64)
    return bn["gamma"].astype(np.float64) * (z - mean) * rstd + bn["beta"].astype(np.float64)


@functools.lru_cache(maxsize=None)
def backward_inputs(M, N, K):
    """dz (M, N), x (M, K), w (N, K) and the FM epilogue's g_fm (M), S (M, 4), addend (M, K); e is x."""
    r = _rng(3, M, N, K)
    return dict(dz=(r.standard_normal((M, N)) * 1e-2).astype(np.float32),
                x=r.standard_normal((M, K)).astype(np.float32),
                w=(r.standard_normal((N, K)) / np.sqrt(N)).astype(np.float32),
                g_fm=(r.standard_normal(M) * 1e-2).astype(np.float32),
                S=r.standard_normal((M, 4)).astype(np.float32),
                addend=(r.standard_normal((M, K)) * 1e-2).astype(np.float32))


@functools.lru_cache(maxsize=None)
def head_inputs(M, K):
    """Head weights, first-order / FM terms with both signs and a few |logit| > 20 rows (agreeing and disagreeing
    with their label), labels."""
    r = _rng(4, M, K)
    fo = r.standard_normal(M).astype(np.float32)
    fm = r.standard_normal(M).astype(np.float32)
    labels = (r.uniform(size=M) < 0.3).astype(np.float32)
    for i, v in enumerate((27.0, -31.0, 23.5, -22.0)):      # rows 0, 3 agree with their label, rows 6, 9 do not
        for term, row in ((fo, 3 * i), (fm, 3 * i + 1)):
            if row < M and M >= 31:                          # a lone row keeps a d logit that fp32 can represent
                term[row] = v
                labels[row] = float(v > 0) if i < 2 else float(v < 0)
    return dict(w=(r.standard_normal(K) / np.sqrt(K)).astype(np.float32), b=r.standard_normal(1).astype(np.float32),
                fo=fo, fm=fm, labels=labels)
