"""Cases, seeded inputs, fp64 references, float32 restatements and bars of the layer matrix: the kernels the models'
own layers call (csrc/fm.hip: dfm_fm_forward, dfm_fm_backward, dfm_embedding_grad_combine, dfm_copy_2d;
csrc/dnn_fused.hip: dfm_bn_relu_dropout_forward / _backward; csrc/loss.hip: dfm_bce_with_logits) and the predictor's
two tower kernels (csrc/predict.hip: dfm_linear_bn_eval, dfm_predict_head).  Shared by
tests/test_cpu_layer_reference.py (which proves on the host that the case lists reach every branch they name, that the
integer family is exact, that a float32 restatement stays inside every bar and that the listed mistakes show) and
tests/test_gpu_layer_matrix.py (which runs them).  Plain numpy; importing this needs neither a GPU nor the library.

Two input families, as in tests/gemm_cases.py.

  int    every operand is a nonzero integer in [-3, 3] held as float32.  Every sum stays below 2^24 (int_bound), so
         it is exact in float32 in any order: where a kernel only adds and multiplies (FM forward / backward,
         grad_combine, copy_2d, the logits of predict_head, the z of linear_bn_eval) the result equals the fp64
         reference bit for bit, and a dropped, doubled or misplaced term moves it.  This family carries the indexing.
  float  N(0, 1)-scaled operands, held to

             |got - fp64| <= C[kind] * EPS32 * sqrt(n) * A

         A = the fp64 sum of |terms| of the element, n = the longest chain of additions that reaches it, restated
         from the launch geometry (*_chain).  For the BatchNorm statistics A is taken about the TRUE column mean
         (sum (z - mean)^2 / M for the variance), never about a kernel's shift: a bar that grew with the shift would
         hide the cancellation the row-0 family is there to show.

C[kind] is measured, not chosen: 4 x the worst ratio a numpy float32 restatement reaches over all float cases of the
kind, in the kernel's own order and in pairwise order, rounded up (the factor 4 pays for fma contraction and the fixed
order: the margin of tests/gemm_cases.py).  Transcendental outputs have no sum to bound: their bar is T[name] * EPS32
* |ref| (+ TINY = 2^-126, the smallest normal float32: below it expf flushes), T = 4 x the worst error of a numpy
float32 evaluation of the same formula against fp64 over the cases.  Composite outputs add the parts (bars below).
`python -m tests.layer_cases` prints the measured ratios:

    kind       worst ratio   x 4     C
    fm_fwd     0.485         1.94    2.0      (dfm_fm_forward; A = 0.5 sum_d ((sum_f |e|)^2 + sum_f e^2))
    fm_bwd     0.647         2.59    2.75     (dfm_fm_backward)
    combine    0.645         2.58    2.75     (dfm_embedding_grad_combine)
    bn_stats   0.679         2.72    2.75     (mean and variance of dfm_bn_relu_dropout_forward: every statistics family)
    bn_out     1.669         6.68    6.75     (its apply pass and running statistics, given float32 statistics)
    bn_bwd     0.289         1.16    1.25     (d gamma, d beta, dz of dfm_bn_relu_dropout_backward)
    bce_loss   0.165         0.66    0.75     (the loss's sum, given the per-sample terms)
    bce_dz     1.244         4.98    5.0      (d logits, given the sigmoid)
    eval_z     0.346         1.38    1.5      (the contraction of dfm_linear_bn_eval)
    eval_epi   1.648         6.59    6.75     (its epilogue, given z and rsqrt)
    head       0.287         1.15    1.25     (the logits of dfm_predict_head)

    transcendental   worst / (EPS32 |ref|)   x 4    T (host)   device                                  T (used)
    rsqrt            0.75                    3.0    3.5        inside: rstd 0.17, eval out 0.18 x the bar    3.5
    log1p            2.29                    9.2    9.5        inside: bce loss 0.12 x the bar            9.5
    sigmoid          2.24                    8.9    9.0        inside: bce dz 0.19 x the bar              9.0
    prob             1.27                    5.1    5.5        0.88 EPS32 |ref| against its own logits    5.5

(log1p and sigmoid take a float32-rounded exp(-|z|), whose half-ulp error they pass on.  The device column is what
tests/test_gpu_layer_matrix.py printed on an MI355X: the probability's error is measured alone; the other three reach
the device only inside a composite bar, and the worst ratio to that bar is given.  No bar needed widening.)

All three statistics families (plain, common mean 50 at sigma 0.1, row 0 displaced by 10 and by 100 sigma) share the
one measured bar.  "kernel" is dnn_fused.hip's order: per 16-row slice the mean and M2 of z - shift, shift = the first
slice's mean, merged by Chan's formula.  Restated with the sums about row 0 that the file formed before this matrix
(order "shifted": var = E[(z - z0)^2] - E[z - z0]^2), the statistics reach, with C = 1,

    family / rows          shifted   kernel   two-pass pairwise
    row 0 10 sigma, 512    13.3      0.18     0.01
    row 0 100 sigma, 512   172       0.68     0.52
    row 0 10 sigma, 4096   22.9      0.13     0.04
    row 0 100 sigma, 4096  621       0.61     0.39
    common, 17             0.10      0.10     0.04
    common, 257            0.37      0.27     0.12
    common, 4115           1.30      0.23     0.11

so the shifted sums miss the bar (C = 2.75) in all four row-0 cases, by a factor 226 at the last, and hold the common
family; the kernel's order holds both.  Slice means of z itself (no shift) would hold the row-0 family and lose the
common one: the float32 rounding of a slice mean, eps |mean|, enters the merged variance to first order, 9.0 at 17
rows.  tests/test_cpu_layer_reference.py holds the kernel's order to the bar at |mean| / sigma = 5e4 as well.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from tests import tower_cases as TC
from tests.gemm_cases import tiled_f32
from tests.helpers import tower_bn_backward_fp64, tower_bn_relu_fp64, tower_masked_grad_fp64
from tests.linear_bwd_epilogue_cases import keep_mask

EPS32 = 2.0 ** -23
TINY = 2.0 ** -126
F32, F64 = np.float32, np.float64
MARGIN = 4.0
C = dict(fm_fwd=2.0, fm_bwd=2.75, combine=2.75, bn_stats=2.75, bn_out=6.75, bn_bwd=1.25, bce_loss=0.75,
         bce_dz=5.0, eval_z=1.5, eval_epi=6.75, head=1.25)
T_HOST = dict(rsqrt=3.5, log1p=9.5, sigmoid=9.0, prob=5.5)         # 4 x the host measurement, rounded up to 0.5
T = dict(T_HOST)                                                   # the bars in use (widened to 2 x the device's where it exceeds)
BN_EPS = F32(1e-5)
BN_MOMENTUM = F32(0.1)


def ceil_div(a, b):
    return -(-a // b)


def pow2_at_least(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def seed_of(key: str) -> int:
    return zlib.crc32(key.encode()) & 0x7FFFFFFF


def _rng(key: str):
    return np.random.default_rng(seed_of(key))


def values(rng, shape, family: str) -> np.ndarray:
    if family == "float":
        return rng.standard_normal(shape).astype(F32)
    v = rng.integers(-3, 3, shape)
    return np.where(v >= 0, v + 1, v).astype(F32)


def bar(A, n, c):
    return c * EPS32 * np.sqrt(np.asarray(n, dtype=F64)) * np.asarray(A, dtype=F64)


def worst(got, want, b) -> float:
    """Worst |got - want| / bar over the elements; a non-finite element fails, a zero bar demands equality."""
    err = np.abs(np.asarray(got, dtype=F64) - np.asarray(want, dtype=F64))
    if not err.size:
        return 0.0
    if not np.isfinite(err).all():
        return float("inf")
    b = np.broadcast_to(np.asarray(b, dtype=F64), err.shape)
    return float(np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0)).max())


def _seq_sum(x, axis):
    """Sum along `axis` one term after the other, in x's dtype."""
    x = np.moveaxis(x, axis, 0)
    acc = np.zeros(x.shape[1:], dtype=x.dtype)
    for i in range(x.shape[0]):
        acc = acc + x[i]
    return acc


def _pair_sum(x, axis):
    """numpy's pairwise sum along `axis` (made the contiguous one), in x's dtype."""
    return np.ascontiguousarray(np.moveaxis(x, axis, -1)).sum(-1, dtype=x.dtype)


def _sum(x, axis, order):
    return _seq_sum(x, axis) if order == "kernel" else _pair_sum(x, axis)


def _butterfly(a):
    """acc += shfl_xor(acc, m) over the last axis (a power of two), m = 1, 2, ...: every lane ends with the tree's sum."""
    n = a.shape[-1]
    lane = np.arange(n)
    m = 1
    while m < n:
        a = a + a[..., lane ^ m]
        m <<= 1
    return a


def sigmoid64(z):
    z = np.asarray(z, dtype=F64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# =====================================================================================================================
# FMInteraction: dfm_fm_forward / dfm_fm_backward
# =====================================================================================================================
FM_D_SCALAR = (1, 2, 3, 5, 7, 63)
FM_D_VEC = (4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 252, 256)
FM_F = (1, 2, 3, 4, 5, 39)                    # the field loop is unrolled by 4
FM_F_FULL_AT = (3, 16, 132)
FM_SHIFT_D = (4, 16, 64)                      # multiples of 4 on a base one float off 16 bytes: the scalar route
FM_REFUSED_D = (65, 67, 260)


def fm_vec(D: int, aligned: bool = True) -> int:
    return 4 if D % 4 == 0 and D // 4 <= 64 and aligned else 1


def fm_lps(D: int, aligned: bool = True) -> int:
    """Lanes per sample."""
    return pow2_at_least(D // fm_vec(D, aligned))


def fm_refused(D: int, aligned: bool = True) -> bool:
    return D // fm_vec(D, aligned) > 64


def fm_batches(D: int, aligned: bool = True) -> Tuple[int, ...]:
    """1, the last sample of a workgroup's, the first of the next, a ragged last workgroup."""
    per = 256 // fm_lps(D, aligned)
    return tuple(sorted({1, per - 1, per + 1, 3 * per + 5} - {0}))


@dataclass(frozen=True)
class Fm:
    D: int
    F: int
    B: int
    shift: int = 0

    @property
    def name(self):
        return f"D{self.D}_F{self.F}_B{self.B}" + ("_shift" if self.shift else "")

    @property
    def vec(self):
        return fm_vec(self.D, not self.shift)

    @property
    def lps(self):
        return fm_lps(self.D, not self.shift)


def _fm_cases() -> List[Fm]:
    cs = [Fm(D, 5, B) for D in FM_D_SCALAR + FM_D_VEC for B in fm_batches(D)]
    cs += [Fm(D, F, 256 // fm_lps(D) + 1) for D in FM_F_FULL_AT for F in FM_F if F != 5]
    cs += [Fm(D, F, B, 1) for D in FM_SHIFT_D for F, B in ((5, 256 // fm_lps(D, False) + 1), (39, 3 * (256 // fm_lps(D, False)) + 5))]
    return cs


FM_CASES: Dict[str, Fm] = {c.name: c for c in _fm_cases()}


def fm_inputs(c: Fm, family: str) -> dict:
    r = _rng(f"fm:{c.name}:{family}")
    return dict(e=values(r, (c.B, c.F, c.D), family), g=values(r, (c.B,), family))


def fm_int_bound(c: Fm) -> int:
    """Largest |partial sum| of the integer family: sum_d (sum_f e)^2 + sum_d sum_f e^2."""
    return 9 * c.F * c.F * c.D + 9 * c.F * c.D


def fm_fwd_chain(c: Fm) -> int:
    return c.F + c.vec + (c.lps.bit_length() - 1) + 1


def fm_bwd_chain(c: Fm) -> int:
    return c.F + 2


def fm_fwd_ref(e):
    e = np.asarray(e, dtype=F64)
    S, a = e.sum(1), np.abs(e).sum(1)
    return 0.5 * (S * S - (e * e).sum(1)).sum(-1), 0.5 * (a * a + (e * e).sum(1)).sum(-1)


def fm_bwd_ref(e, g):
    e, g = np.asarray(e, dtype=F64), np.asarray(g, dtype=F64)[:, None, None]
    S = e.sum(1)[:, None, :]
    return g * (S - e), np.abs(g) * (np.abs(e).sum(1)[:, None, :] + np.abs(e))


def fm_fwd_restate(e, vec: int, lps: int, dt=F32, order: str = "kernel", mistake: Optional[str] = None):
    """fm_fwd_kernel<VEC> in `dt`: a sample's lanes sweep the fields (S += v, SQ += v v), each adds its VEC columns'
    S^2 - SQ, a butterfly over the sample's lps lanes, out = 0.5 acc.  Mistakes: "drop_last_field"; "idle_lane" (the
    lanes behind D / VEC read on: the next field's first columns)."""
    e = np.asarray(e, dtype=dt)
    B, F, D = e.shape
    if order == "pair":
        S = _pair_sum(e, 1)
        return dt(0.5) * _pair_sum(S * S - _pair_sum(e * e, 1), -1)
    W = lps * vec
    if mistake == "idle_lane":
        flat = np.concatenate([e.reshape(-1), np.ones(W, dtype=dt)])
        idx = (np.arange(B)[:, None, None] * F + np.arange(F)[None, :, None]) * D + np.arange(W)[None, None, :]
        x = flat[idx]
    else:
        x = np.zeros((B, F, W), dtype=dt)
        x[:, :, :D] = e
    if mistake == "drop_last_field":
        x = x[:, :F - 1]
    S, SQ = _seq_sum(x, 1), _seq_sum(x * x, 1)
    acc = _seq_sum((S * S - SQ).reshape(B, lps, vec), 2)
    return dt(0.5) * _butterfly(acc)[:, 0]


def fm_bwd_restate(e, g, dt=F32, order: str = "kernel", mistake: Optional[str] = None):
    e, g = np.asarray(e, dtype=dt), np.asarray(g, dtype=dt)[:, None, None]
    S = _sum(e[:, :-1] if mistake == "drop_last_field" else e, 1, order)[:, None, :]
    return g * (S - e)


# =====================================================================================================================
# dfm_embedding_grad_combine, dfm_copy_2d
# =====================================================================================================================
COMBINE_D = (4, 8, 12, 16, 32)                # at 12, c % dim is not a mask
COMBINE_F = (1, 3, 39)
COMBINE_THREADS = (255, 256, 257, 3 * 256 + 5)


@dataclass(frozen=True)
class Combine:
    D: int
    F: int
    rows: int
    ld_pad: int            # floats added to the row stride of g_flat
    extra: bool
    fm: bool

    @property
    def width(self):
        return self.F * self.D

    @property
    def ld(self):
        return self.width + self.ld_pad

    @property
    def name(self):
        return f"D{self.D}_F{self.F}_R{self.rows}_ld{self.ld}_x{int(self.extra)}f{int(self.fm)}"


def combine_rows(D, F) -> Tuple[int, ...]:
    """Row counts whose rows * width / 4 lanes end just below, on, just above a workgroup's 256 and in a ragged
    fourth workgroup (exactly 255, 256, 257 and 773 where width / 4 divides them)."""
    w4 = F * D // 4
    return tuple(sorted({max(1, 255 // w4), ceil_div(256, w4), ceil_div(257, w4), ceil_div(3 * 256 + 5, w4)}))


def _combine_cases() -> List[Combine]:
    nulls = ((True, True), (False, True), (True, False), (False, False))
    cs, i = [], 0
    for D in COMBINE_D:
        for F in COMBINE_F:
            x, f = nulls[i % 4]
            cs.append(Combine(D, F, ceil_div(257, F * D // 4), 0, x, f))
            i += 1
    for D, F in ((4, 1), (12, 3), (16, 39)):
        for rows in combine_rows(D, F):
            for pad in (0, 4, F * D):
                x, f = nulls[i % 2]                       # the FM term always: it is the one that indexes by c % dim
                cs.append(Combine(D, F, rows, pad, x, f))
                i += 1
    for D in (12, 16):
        cs += [Combine(D, 3, 65, 4, x, f) for x, f in nulls]
    return cs


COMBINE_CASES: Dict[str, Combine] = {c.name: c for c in _combine_cases()}


def combine_inputs(c: Combine, family: str) -> dict:
    r = _rng(f"combine:{c.name}:{family}")
    return dict(g_flat=values(r, (c.rows, c.ld), family), g_extra=values(r, (c.rows, c.width), family),
                g_fm=values(r, (c.rows,), family), fm_sum=values(r, (c.rows, c.D), family),
                e=values(r, (c.rows, c.width), family))


def combine_ref(c: Combine, inp, dt=F64, mistake: Optional[str] = None):
    """(out, A): g_flat[:, :width] + g_extra + g_fm[:, None] (fm_sum tiled over the fields - e); in float32 this is
    the kernel's own order.  Mistake "mask": c & (dim - 1) in place of c % dim."""
    k = {n: np.asarray(v, dtype=dt) for n, v in inp.items()}
    out = k["g_flat"][:, :c.width]
    A = np.abs(out).astype(F64)
    if c.extra:
        out, A = out + k["g_extra"], A + np.abs(k["g_extra"])
    if c.fm:
        col = np.arange(c.width)
        idx = ((col // 4 * 4) & (c.D - 1)) + col % 4 if mistake == "mask" else col % c.D
        s, g = k["fm_sum"][:, idx], k["g_fm"][:, None]
        out, A = out + g * (s - k["e"]), A + np.abs(g) * (np.abs(s) + np.abs(k["e"]))
    return out, A


COMBINE_CHAIN = 3
COPY_WIDTH = (4, 12, 624)
COPY_ROWS = (0, 1, 63, 65, 257)


def copy_lds(width):
    return (width, width + 4, 2 * width)


# =====================================================================================================================
# dfm_bn_relu_dropout_forward / _backward
# =====================================================================================================================
BN_ROWS_PER_SLICE = 16
BN_FIN_LANES = 16
BN_M = (1, 2, 15, 16, 17, 33, 255, 257, 16 * 257 + 3)
BN_N = (1, 3, 15, 16, 17, 255, 257, 300)
BN_SHAPES = tuple(sorted({(M, N) for M in BN_M for N in (3, 17)} | {(M, N) for M in (17, 257) for N in BN_N}))
P_TINY = float(np.nextafter(F32(2.0 ** -32), F32(1)))        # the smallest p whose threshold is 1
BN_P = (0.0, 0.25, 0.5, P_TINY)
BN_SALTS = (3, 11)
BN_SEEDS = (20240607, -77)


def bn_slices(M):
    return ceil_div(M, BN_ROWS_PER_SLICE)


def bn_slices_per_lane(M):
    """(fewest, most) slices a finalize lane folds."""
    s = bn_slices(M)
    return s // BN_FIN_LANES, ceil_div(s, BN_FIN_LANES)


def bn_chain(M):
    return BN_ROWS_PER_SLICE + bn_slices_per_lane(M)[1] + BN_FIN_LANES


def dropout_thresh(p) -> int:
    p = float(F32(p))
    return 0 if p <= 0 else min(int(p * 4294967296.0), 4294967295)


def inv_keep_of(p) -> float:
    return float(F32(1) / (F32(1) - F32(p)))


@dataclass(frozen=True)
class Bn:
    M: int
    N: int
    stats: str             # plain | common | row0_10 | row0_100
    p: float
    salt: int
    seed: Optional[int]    # None: a NULL seed pointer (p == 0 only)
    running: bool          # the three running pointers given or all NULL

    @property
    def name(self):
        p = {0.0: "0", 0.25: "q", 0.5: "h"}.get(self.p, "tiny")
        return f"M{self.M}_N{self.N}_{self.stats}_p{p}_s{self.salt}_{'null' if self.seed is None else self.seed % 100}_r{int(self.running)}"


def _bn_cases() -> List[Bn]:
    cs = []
    for i, (M, N) in enumerate(BN_SHAPES):
        p = BN_P[i % 4]
        cs.append(Bn(M, N, "plain", p, BN_SALTS[(i // 4) % 2], None if (p == 0 and i % 8 == 0) else BN_SEEDS[(i // 2) % 2],
                     i % 5 != 4))
    cs += [Bn(M, N, "common", 0.25, 3, BN_SEEDS[0], True) for M, N in ((17, 3), (257, 17), (16 * 257 + 3, 3))]
    cs += [Bn(M, 3, f"row0_{k}", 0.0 if k == 10 else 0.25, 11, BN_SEEDS[1], True) for M in (512, 4096) for k in (10, 100)]
    return cs


BN_CASES: Dict[str, Bn] = {c.name: c for c in _bn_cases()}
BN_BWD_CASES: Dict[str, Bn] = {c.name: c for c in _bn_cases() if c.stats == "plain"}


@functools.lru_cache(maxsize=None)
def bn_fwd_inputs(name: str) -> dict:
    c = BN_CASES[name]
    r = _rng("bnf:" + name)
    z = r.standard_normal((c.M, c.N)) * 1.3 + 0.2
    if c.stats == "common":
        z = r.standard_normal((c.M, c.N)) * 0.1 + 50.0
    elif c.stats.startswith("row0_"):
        z[0] = 0.2 + 1.3 * float(c.stats[5:]) * np.where(np.arange(c.N) % 2 == 0, 1.0, -1.0)
    return dict(z=z.astype(F32), gamma=r.uniform(0.5, 1.5, c.N).astype(F32), beta=(r.standard_normal(c.N) * 0.3).astype(F32),
                running_mean=r.standard_normal(c.N).astype(F32), running_var=r.uniform(0.5, 2.0, c.N).astype(F32),
                num_batches=7)


def bn_mask(c: Bn, count: int):
    """(kept, scale): the restated hash mask of dropout.h and inv_keep as the host forms it in float32."""
    th = dropout_thresh(c.p)
    if th == 0:
        return np.ones(count, dtype=bool), 1.0
    return keep_mask(c.seed % 2 ** 64, c.salt, count, th / 4294967296.0), inv_keep_of(c.p)      # int64 seen as uint64


@functools.lru_cache(maxsize=None)
def bn_fwd_ref(name: str) -> dict:
    """fp64 results and their bars.  bar_mean = C sqrt(n) EPS sum|z| / M; bar_var = C sqrt(n) EPS var (A about the
    true mean); rstd = (var + eps)^-1/2 moves by half the relative change of var + eps, plus the rsqrt's own error;
    out = gamma (z - mean) rstd + beta moves by |gamma| rstd d mean + |gamma xhat| d rstd / rstd, plus its own
    roundings C_out EPS (|gamma xhat| + |beta|); ReLU is 1-Lipschitz, the dropout scale multiplies everything."""
    c, i = BN_CASES[name], bn_fwd_inputs(name)
    z = i["z"].astype(F64)
    M, n = c.M, bn_chain(c.M)
    eps, mom = float(BN_EPS), float(BN_MOMENTUM)
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat, y, a = tower_bn_relu_fp64(z, mean, rstd, i["gamma"], i["beta"])
    kept, scale = bn_mask(c, M * c.N)
    kept = kept.reshape(M, c.N)
    ga, be = np.abs(i["gamma"].astype(F64)), np.abs(i["beta"].astype(F64))
    b_mean = bar(np.abs(z).mean(0), n, C["bn_stats"])
    b_var = bar(var, n, C["bn_stats"])
    b_rstd = rstd * (0.5 * b_var / (var + eps) + T["rsqrt"] * EPS32)
    A_out = ga * np.abs(xhat) + be
    b_out = scale * (ga * rstd * b_mean + ga * np.abs(xhat) * b_rstd / rstd + C["bn_out"] * EPS32 * A_out)
    unb = M / (M - 1.0) if M > 1 else 1.0
    rm0, rv0 = i["running_mean"].astype(F64), i["running_var"].astype(F64)
    rm, rv = (1 - mom) * rm0 + mom * mean, (1 - mom) * rv0 + mom * var * unb
    b_rm = mom * b_mean + C["bn_out"] * EPS32 * (np.abs((1 - mom) * rm0) + np.abs(mom * mean))
    b_rv = mom * unb * b_var + C["bn_out"] * EPS32 * (np.abs((1 - mom) * rv0) + mom * var * unb)
    return dict(mean=mean, var=var, rstd=rstd, xhat=xhat, y=y, out=a * kept * scale, kept=kept, scale=scale,
                running_mean=rm, running_var=rv, A_out=A_out, bar_mean=b_mean, bar_var=b_var, bar_rstd=b_rstd,
                bar_out=b_out, bar_running_mean=b_rm, bar_running_var=b_rv)


def _merge(na, ma, qa, nb, mb, qb):
    """merge_moments of dnn_fused.hip on float32 column vectors (nb a scalar count)."""
    if nb == 0:
        return na, ma, qa
    nb = F32(nb)
    n = na + nb
    d, f = mb - ma, nb / n
    return n, ma + d * f, (qa + qb) + d * d * (na * f)


def bn_stats_restate(z, order: str = "kernel", mistake: Optional[str] = None):
    """(mean, biased var) of the columns in float32.  "kernel": per 16-row slice the mean and M2 about it, 16 lanes
    fold every 16th slice by Chan's formula, lane 0 folds the lanes; "pair": two passes, pairwise sums; "shifted": the
    sums about row 0 (var = E[(z - z0)^2] - E[z - z0]^2) in the same slice and lane order.  Mistake
    "skip_last_slice"."""
    z = np.asarray(z, dtype=F32)
    M, N = z.shape
    Mf = F32(M)
    if order == "pair":
        mean = _pair_sum(z, 0) / Mf
        d = z - mean
        return mean, _pair_sum(d * d, 0) / Mf
    S, L = bn_slices(M), BN_FIN_LANES
    live = S - 1 if mistake == "skip_last_slice" else S
    cnt = [min(BN_ROWS_PER_SLICE, M - BN_ROWS_PER_SLICE * s) for s in range(S)]
    zero = np.zeros(N, dtype=F32)
    if order == "shifted":
        lanes = [[zero, zero] for _ in range(L)]
        for s in range(live):
            v = z[16 * s:16 * s + cnt[s]] - z[0]
            lanes[s % L][0] = lanes[s % L][0] + _seq_sum(v, 0)
            lanes[s % L][1] = lanes[s % L][1] + _seq_sum(v * v, 0)
        s1, s2 = zero, zero
        for a, b in lanes:
            s1, s2 = s1 + a, s2 + b
        ms = s1 / Mf
        return z[0] + ms, np.maximum(s2 / Mf - ms * ms, F32(0))
    shift = _seq_sum(z[:cnt[0]], 0) / F32(cnt[0])          # the first slice's mean: every workgroup forms the same bits
    lanes = [(F32(0), zero, zero) for _ in range(L)]
    for s in range(live):
        rows = z[16 * s:16 * s + cnt[s]] - shift
        m = _seq_sum(rows, 0) / F32(cnt[s])
        d = rows - m
        lanes[s % L] = _merge(*lanes[s % L], cnt[s], m, _seq_sum(d * d, 0))
    n, m, q = lanes[0]
    for nb, mb, qb in lanes[1:]:
        n, m, q = _merge(n, m, q, float(nb), mb, qb)
    return shift + m, q / Mf


def bn_apply_restate(c: Bn, inp, mean, var, salt: Optional[int] = None):
    """bn_fwd_finalize's tail and bn_relu_dropout_fwd in float32 from float32 (mean, var): rstd, out, running
    statistics.  `salt`: build the mask with another salt (the mistake of the CPU test)."""
    z, ga, be = inp["z"], inp["gamma"], inp["beta"]
    mean, var = np.asarray(mean, dtype=F32), np.asarray(var, dtype=F32)
    rstd = (F32(1) / np.sqrt(var + BN_EPS)).astype(F32)
    y = ga * ((z - mean) * rstd) + be
    kept, scale = bn_mask(c if salt is None else Bn(c.M, c.N, c.stats, c.p, salt, c.seed, c.running), z.size)
    out = np.maximum(y, F32(0)) * np.where(kept.reshape(z.shape), F32(scale), F32(0))
    M = F32(c.M)
    unb = var * M / (M - F32(1)) if c.M > 1 else var
    one = F32(1) - BN_MOMENTUM
    return dict(rstd=rstd, out=out, running_mean=one * inp["running_mean"] + BN_MOMENTUM * mean,
                running_var=one * inp["running_var"] + BN_MOMENTUM * unb)


# ---- backward -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bn_bwd_inputs(name: str) -> dict:
    c = BN_BWD_CASES[name]
    bn = TC.bn_inputs(c.M, c.N)                      # z moved off the ReLU kink; stats as the forward left them
    r = _rng("bnb:" + name)
    return dict(bn, g=r.standard_normal((c.M, c.N)).astype(F32), d_gamma0=(r.standard_normal(c.N) + 3.0).astype(F32),
                d_beta0=(r.standard_normal(c.N) - 3.0).astype(F32))


@functools.lru_cache(maxsize=None)
def bn_bwd_ref(name: str) -> dict:
    """fp64 (d gamma, d beta, dz) of one call WITHOUT the initial values, A of each, and min |y|."""
    c, i = BN_BWD_CASES[name], bn_bwd_inputs(name)
    mean, rstd = i["stats"].astype(F64)
    xhat, y, _ = tower_bn_relu_fp64(i["z"], mean, rstd, i["gamma"], i["beta"])
    kept, scale = bn_mask(c, c.M * c.N)
    dy = tower_masked_grad_fp64(i["g"], y) * kept.reshape(c.M, c.N) * scale
    dgamma, dbeta, dz = tower_bn_backward_fp64(dy, xhat, i["gamma"], rstd)
    A_gamma, A_beta = np.abs(dy * xhat).sum(0), np.abs(dy).sum(0)
    A_dz = np.abs(i["gamma"].astype(F64) * rstd) * (np.abs(dy) + A_beta / c.M + np.abs(xhat) * A_gamma / c.M)
    return dict(d_gamma=dgamma, d_beta=dbeta, dz=dz, A_gamma=A_gamma, A_beta=A_beta, A_dz=A_dz, min_abs_y=float(np.abs(y).min()),
                dy=dy)


def bn_bwd_chain(M):
    return bn_chain(M) + 3


def bn_bwd_restate(c: Bn, inp, order: str = "kernel", mistake: Optional[str] = None):
    """bn_bwd_partials / bn_bwd_finalize / bn_relu_dropout_bwd in float32: (sum dy zhat, sum dy, dz)."""
    z, g, ga, be = inp["z"], inp["g"], inp["gamma"], inp["beta"]
    mu, rs = inp["stats"]
    M, N = z.shape
    zh = (z - mu) * rs
    y = ga * zh + be
    kept, scale = bn_mask(c, M * N)
    dy = np.where(y > 0, g * np.where(kept.reshape(M, N), F32(scale), F32(0)), F32(0)).astype(F32)
    if order == "pair":
        s, q = _pair_sum(dy, 0), _pair_sum(dy * zh, 0)
    else:
        S, L = bn_slices(M), BN_FIN_LANES
        pad = np.zeros((ceil_div(S, L) * L * 16, N, 2), dtype=F32)
        pad[:M, :, 0], pad[:M, :, 1] = dy, dy * zh
        if mistake == "skip_last_slice":
            pad[16 * (S - 1):] = 0
        part = _seq_sum(pad.reshape(-1, 16, N, 2), 1)                       # (slices padded, N, 2)
        s, q = np.moveaxis(_seq_sum(_seq_sum(part.reshape(-1, L, N, 2), 0), 0), -1, 0)
    Mf = F32(M)
    return q, s, ga * rs * (dy - s / Mf - zh * (q / Mf))


# =====================================================================================================================
# dfm_bce_with_logits
# =====================================================================================================================
BCE_PER_BLOCK = 1024
BCE_N = (1, 3, 4, 5, 1023, 1024, 1025, 2049, 256 * 1024 + 7)
BCE_FIXED = (0.0, 1e-8, -1e-8, 20.0, -20.0, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0)
BCE_CASES = tuple(("normal", n) for n in BCE_N) + tuple(("soft", n) for n in (5, 1025, 256 * 1024 + 7)) + \
    (("fixed", 2 * len(BCE_FIXED)),)


def bce_partials(n):
    return ceil_div(n, BCE_PER_BLOCK)


def bce_chain(n):
    """12 additions per thread, 6 + 2 across the workgroup, the finalize's strided sum, 6 + 2 again, the mean."""
    return 12 + 8 + ceil_div(bce_partials(n), 256) + 8 + 1


@functools.lru_cache(maxsize=None)
def bce_inputs(family: str, n: int) -> dict:
    r = _rng(f"bce:{family}:{n}")
    if family == "fixed":
        z = np.repeat(np.asarray(BCE_FIXED, dtype=F32), 2)
        return dict(z=z, y=np.tile(np.asarray([0.0, 1.0], dtype=F32), len(BCE_FIXED)))
    z = (r.standard_normal(n) * 6.0).astype(F32)
    y = (r.uniform(size=n) < 0.3).astype(F32) if family == "normal" else r.uniform(0.0, 1.0, n).astype(F32)
    return dict(z=z, y=y)


@functools.lru_cache(maxsize=None)
def bce_ref(family: str, n: int) -> dict:
    i = bce_inputs(family, n)
    z, y = i["z"].astype(F64), i["y"].astype(F64)
    soft = np.log1p(np.exp(-np.abs(z)))
    sig = sigmoid64(z)
    A_loss = (np.maximum(z, 0) + np.abs(z * y) + soft).sum() / n
    b_loss = EPS32 * (C["bce_loss"] * np.sqrt(bce_chain(n)) * A_loss + T["log1p"] * soft.sum() / n) + TINY
    b_dz = EPS32 * (C["bce_dz"] * (sig + y) + T["sigmoid"] * sig) / n + TINY
    return dict(loss=float((np.maximum(z, 0) - z * y + soft).mean()), dz=(sig - y) / n, soft=soft, sig=sig, A_loss=A_loss,
                A_dz=(sig + y) / n, bar_loss=float(b_loss), bar_dz=b_dz)


def _block_sum(v):
    """v (blocks, 256) -> (blocks,): a butterfly inside each wave of 64, then (w0 + w1) + (w2 + w3)."""
    w = _butterfly(v.reshape(v.shape[0], 4, 64))[:, :, 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def bce_restate(inp, order: str = "kernel", exact_terms: Optional[dict] = None, mistake: Optional[str] = None):
    """(loss, dz, partials) in float32.  exact_terms: the fp64 log1p(exp(-|z|)) and sigmoid rounded to float32 in
    place of float32 evaluations (the calibration of the sums alone).  Mistake "skip_partial_256": the finalize
    stops at 256 partials."""
    z, y = inp["z"], inp["y"]
    n = z.size
    e = np.exp(-np.abs(z))
    soft = np.log1p(e) if exact_terms is None else exact_terms["soft"].astype(F32)
    sig = np.where(z >= 0, F32(1) / (F32(1) + e), e / (F32(1) + e)) if exact_terms is None else exact_terms["sig"].astype(F32)
    inv_n = F32(1) / F32(n)
    dz = (sig - y) * inv_n
    term = (np.maximum(z, F32(0)) - z * y) + soft
    if order == "pair":
        return np.sum(term, dtype=F32) * inv_n, dz, None
    P = bce_partials(n)
    t = np.zeros(P * BCE_PER_BLOCK, dtype=F32)
    t[:n] = term
    partial = _block_sum(_seq_sum(t.reshape(P, 256, 4), 2))
    live = partial[:256] if mistake == "skip_partial_256" else partial
    p2 = np.zeros(ceil_div(live.size, 256) * 256, dtype=F32)
    p2[:live.size] = live
    return _block_sum(_seq_sum(p2.reshape(-1, 256), 0)[None])[0] * inv_n, dz, partial


# =====================================================================================================================
# dfm_linear_bn_eval
# =====================================================================================================================
EVAL_BK = 32
EVAL_M = (1, 63, 64, 65, 130)
EVAL_N = (1, 7, 64, 65, 100)
EVAL_K = (1, 4, 10, 31, 32, 33, 64, 100)
EVAL_EPS = F32(1e-5)


def operand_fast(shift, ld, kc, rows, kdim) -> bool:
    """gemm::operand_fast restated; a pointer is given as its distance in floats from a 16-byte boundary."""
    return shift % 4 == 0 and ld % 4 == 0 and (kdim % 4 == 0 if kc else rows % 4 == 0)


@dataclass(frozen=True)
class Eval:
    M: int
    N: int
    K: int
    x_pad: int = 0
    x_shift: int = 0
    w_shift: int = 0
    bias: bool = True

    @property
    def ldx(self):
        return self.K + self.x_pad

    @property
    def fast(self):
        return operand_fast(self.x_shift, self.ldx, True, self.M, self.K) and operand_fast(self.w_shift, self.K, True, self.N, self.K)

    @property
    def name(self):
        return f"M{self.M}_N{self.N}_K{self.K}_p{self.x_pad}_xs{self.x_shift}_ws{self.w_shift}_b{int(self.bias)}"


def _eval_cases() -> List[Eval]:
    cs = []
    fast = (dict(), dict(x_pad=4))
    slow = (dict(x_pad=1), dict(x_shift=1), dict(w_shift=1))
    odd = (dict(), dict(x_pad=1), dict(x_pad=3))                    # K % 4 != 0 is the checked route whatever the rest

    def add(M, N, K, how):
        cs.append(Eval(M, N, K, bias=(len(cs) // 2) % 2 == 0, **how[len(cs) % len(how)]))

    for M in EVAL_M:                                                 # every tile edge: a fast K with a tail, a checked K
        for N in EVAL_N:
            add(M, N, 100, fast + slow + fast)
            add(M, N, 33, odd)
    for M, N in ((65, 100), (1, 1), (130, 7)):                       # every K: on both routes where K % 4 == 0
        for K in EVAL_K:
            if K % 4 == 0:
                add(M, N, K, fast)
                add(M, N, K, slow)
            elif K != 33:
                add(M, N, K, odd)
    return list({c.name: c for c in cs}.values())


EVAL_CASES: Dict[str, Eval] = {c.name: c for c in _eval_cases()}


def eval_chain(K):
    return ceil_div(K, EVAL_BK) * EVAL_BK // 2 + 2


def eval_inputs(c: Eval, family: str) -> dict:
    r = _rng(f"eval:{c.name}:{family}")
    w = values(r, (c.N, c.K), family)
    if family == "float":
        w = (w / np.sqrt(c.K)).astype(F32)
    return dict(x=values(r, (c.M, c.K), family), w=w, b=values(r, (c.N,), family),
                gamma=r.uniform(0.5, 1.5, c.N).astype(F32), beta=(r.standard_normal(c.N) * 0.3).astype(F32),
                running_mean=(r.standard_normal(c.N) * (3.0 if family == "int" else 1.0)).astype(F32),
                running_var=(10.0 ** r.uniform(-6.0, 1.0, c.N)).astype(F32))


def eval_ref(c: Eval, inp, family: str) -> dict:
    """fp64 z, out and the bar of out: the epilogue's own (rsqrt and its roundings) and, in the float family, the
    contraction's C sqrt(n) EPS A_z carried through |gamma| rstd.  The integer family has z exact."""
    k = {n: v.astype(F64) for n, v in inp.items()}
    z, A_z = k["x"] @ k["w"].T, np.abs(k["x"]) @ np.abs(k["w"]).T
    if c.bias:
        z, A_z = z + k["b"], A_z + np.abs(k["b"])
    rs = 1.0 / np.sqrt(k["running_var"] + float(EVAL_EPS))
    t = k["gamma"] * ((z - k["running_mean"]) * rs)
    A_epi = np.abs(t) + np.abs(k["beta"])
    b = EPS32 * (T["rsqrt"] * np.abs(t) + C["eval_epi"] * A_epi)
    if family == "float":
        b = b + np.abs(k["gamma"] * rs) * bar(A_z, eval_chain(c.K), C["eval_z"])
    return dict(z=z, A_z=A_z, out=np.maximum(t + k["beta"], 0.0), A_epi=A_epi, bar_out=b, rs=rs)


def eval_restate(c: Eval, inp, order: str = "kernel", z=None, rs=None, mistake: Optional[str] = None):
    """(z, out) in float32: the tile loop's order (tests/gemm_cases.tiled_f32, one split) and eval_tile_epilogue.
    z / rs: given float32 values in place of the computed ones (the epilogue's calibration).  Mistake
    "drop_k_tail": the k slices behind the last whole 32 are left out."""
    K = c.K // EVAL_BK * EVAL_BK if mistake == "drop_k_tail" else c.K
    if z is None:
        z = tiled_f32(dict(a=inp["x"][:, :K], b=inp["w"][:, :K], bias=inp["b"] if c.bias else None, c0=None), 1,
                      ceil_div(K, EVAL_BK) * EVAL_BK, order)
    if rs is None:
        rs = (F32(1) / np.sqrt(inp["running_var"] + EVAL_EPS)).astype(F32)
    return z, np.maximum(inp["gamma"] * ((z - inp["running_mean"]) * rs) + inp["beta"], F32(0))


# =====================================================================================================================
# dfm_predict_head
# =====================================================================================================================
HEAD_LANES, HEAD_ROWS = 8, 32
HEAD_M = (1, 31, 32, 33, 100)
HEAD_K = (4, 8, 28, 32, 36, 64, 256)
HEAD_EXTREME = (25.0, -25.0, 95.0, -95.0)


@dataclass(frozen=True)
class Head:
    M: int
    K: int
    valid: int
    b: bool
    fo: bool
    extra: bool
    logits: bool

    @property
    def name(self):
        return f"M{self.M}_K{self.K}_v{self.valid}_{int(self.b)}{int(self.fo)}{int(self.extra)}{int(self.logits)}"


def head_valids(M):
    return tuple(sorted({0, 1, M - 1, M}))


def _head_cases() -> List[Head]:
    cs, i = [], 0
    for M in HEAD_M:
        for K in HEAD_K:
            v = head_valids(M)
            cs.append(Head(M, K, v[(i + 1) % len(v)], *(bool((i * 7 + 5) >> j & 1) for j in range(4))))
            i += 1
    cs += [Head(M, 36, v, True, True, True, True) for M in (1, 33, 100) for v in head_valids(M)]
    cs += [Head(33, 36, 33, *(bool(m >> j & 1) for j in range(4))) for m in range(16)]
    return cs


HEAD_CASES: Dict[str, Head] = {c.name: c for c in _head_cases()}


def head_chain(K):
    return 4 * ceil_div(K, 4 * HEAD_LANES) + 3 + 3


def head_inputs(c: Head, family: str) -> dict:
    r = _rng(f"head:{c.M}:{c.K}:{family}")
    w = values(r, (c.K,), family)
    fo = values(r, (c.M,), family)
    if family == "float":
        w = (w / np.sqrt(c.K)).astype(F32)
        k = min(c.M, len(HEAD_EXTREME))
        fo[:k] = HEAD_EXTREME[:k]                    # logits near +-25 and +-95: expf overflows at the upper end
    return dict(a=values(r, (c.M, c.K), family), w=w, b=values(r, (1,), family), fo=fo, extra=values(r, (c.M,), family))


def head_ref(c: Head, inp, family: str) -> dict:
    """fp64 logits = (fo + extra) + (a . w + b), probs and their bars.  |d sigmoid| <= sigmoid |d logit|."""
    k = {n: v.astype(F64) for n, v in inp.items()}
    zl, A = k["a"] @ k["w"], np.abs(k["a"]) @ np.abs(k["w"])
    for given, name in ((c.b, "b"), (c.fo, "fo"), (c.extra, "extra")):
        if given:
            zl, A = zl + k[name], A + np.abs(k[name])
    b_logit = bar(A, head_chain(c.K), C["head"]) if family == "float" else np.zeros(c.M)
    p = sigmoid64(zl)
    return dict(logits=zl, A=A, probs=p, bar_logits=b_logit, bar_probs=p * (T["prob"] * EPS32 + b_logit) + TINY)


def head_restate(c: Head, inp, order: str = "kernel", mistake: Optional[str] = None):
    """(logits, probs) in float32 with NaN in the rows the kernel leaves alone: lane l of a row's 8 takes the float4s
    at 4 l + 32 i, one fma chain; a butterfly over the 8; (fo + extra) + (dot + b); 1 / (1 + exp(-logit)).  Mistake
    "valid_ignored"."""
    a, w = inp["a"], inp["w"]
    if order == "pair":
        dot = _pair_sum(a * w, 1)
    else:
        it = ceil_div(c.K, 4 * HEAD_LANES)
        p = np.zeros((c.M, it * 4 * HEAD_LANES), dtype=F32)
        p[:, :c.K] = a * w
        lanes = _seq_sum(p.reshape(c.M, it, HEAD_LANES, 4).transpose(0, 2, 1, 3).reshape(c.M, HEAD_LANES, it * 4), 2)
        dot = _butterfly(lanes)[:, 0]
    zero = np.zeros(c.M, dtype=F32)
    zl = ((inp["fo"] if c.fo else zero) + (inp["extra"] if c.extra else zero)) + (dot + (inp["b"][0] if c.b else F32(0)))
    with np.errstate(over="ignore"):
        pr = F32(1) / (F32(1) + np.exp(-zl))
    live = np.arange(c.M) < (c.M if mistake == "valid_ignored" else c.valid)
    return np.where(live, zl, F32(np.nan)), np.where(live, pr, F32(np.nan))


# =====================================================================================================================
# the measurement behind C and T
# =====================================================================================================================
ORDERS = ("kernel", "pair")


def rel_error(got, want):
    """Worst |got - want| in units of EPS32 |want|, with an absolute TINY forgiven first."""
    want = np.asarray(want, dtype=F64)
    err = np.maximum(np.abs(np.asarray(got, dtype=F64) - want) - TINY, 0.0)
    return float((err / (EPS32 * np.maximum(np.abs(want), TINY))).max()) if err.size else 0.0


@functools.lru_cache(maxsize=None)
def measure() -> Tuple[Dict[str, float], Dict[str, float], Dict[str, float]]:
    """(worst ratio per kind with C = 1, worst transcendental error per name in EPS32 |ref|, the row-0 families'
    bn_stats ratio per (order, case))."""
    w = {k: 0.0 for k in C}
    t = {k: 0.0 for k in T}

    def up(d, k, v):
        d[k] = max(d[k], v)

    for c in FM_CASES.values():
        i = fm_inputs(c, "float")
        ref, A = fm_fwd_ref(i["e"])
        rb, Ab = fm_bwd_ref(i["e"], i["g"])
        for o in ORDERS:
            up(w, "fm_fwd", worst(fm_fwd_restate(i["e"], c.vec, c.lps, F32, o), ref, bar(A, fm_fwd_chain(c), 1)))
            up(w, "fm_bwd", worst(fm_bwd_restate(i["e"], i["g"], F32, o), rb, bar(Ab, fm_bwd_chain(c), 1)))
    for c in COMBINE_CASES.values():
        i = combine_inputs(c, "float")
        ref, A = combine_ref(c, i)
        up(w, "combine", worst(combine_ref(c, i, F32)[0], ref, bar(A, COMBINE_CHAIN, 1)))
    row0 = {}
    for name, c in BN_CASES.items():
        i, r = bn_fwd_inputs(name), bn_fwd_ref(name)
        n = bn_chain(c.M)
        for o in ORDERS + ("shifted",):
            m, v = bn_stats_restate(i["z"], o)
            ratio = max(worst(m, r["mean"], bar(np.abs(i["z"].astype(F64)).mean(0), n, 1)), worst(v, r["var"], bar(r["var"], n, 1)))
            if o != "shifted":
                up(w, "bn_stats", ratio)
            if c.stats.startswith("row0"):
                row0[(o, name)] = ratio
        ap = bn_apply_restate(c, i, r["mean"].astype(F32), r["var"].astype(F32))
        up(t, "rsqrt", rel_error(ap["rstd"], 1.0 / np.sqrt(r["var"].astype(F32).astype(F64) + float(BN_EPS))))
        # the apply pass alone: the float32 statistics are its inputs, so the reference takes the same numbers
        m32, rs32 = r["mean"].astype(F32).astype(F64), ap["rstd"].astype(F64)
        _, _, a = tower_bn_relu_fp64(i["z"], m32, rs32, i["gamma"], i["beta"])
        A = np.abs(i["gamma"].astype(F64) * (i["z"].astype(F64) - m32) * rs32) + np.abs(i["beta"].astype(F64))
        up(w, "bn_out", worst(ap["out"], a * r["kept"] * r["scale"], r["scale"] * EPS32 * A))
        mom, v32 = float(BN_MOMENTUM), r["var"].astype(F32).astype(F64)
        unb = c.M / (c.M - 1.0) if c.M > 1 else 1.0
        rm0, rv0 = i["running_mean"].astype(F64), i["running_var"].astype(F64)
        up(w, "bn_out", worst(ap["running_mean"], (1 - mom) * rm0 + mom * m32, EPS32 * (np.abs((1 - mom) * rm0) + np.abs(mom * m32))))
        up(w, "bn_out", worst(ap["running_var"], (1 - mom) * rv0 + mom * v32 * unb, EPS32 * ((1 - mom) * rv0 + mom * v32 * unb)))
    for name, c in BN_BWD_CASES.items():
        i, r = bn_bwd_inputs(name), bn_bwd_ref(name)
        n = bn_chain(c.M)
        for o in ORDERS:
            q, s, dz = bn_bwd_restate(c, i, o)
            up(w, "bn_bwd", max(worst(q, r["d_gamma"], bar(r["A_gamma"], n, 1)), worst(s, r["d_beta"], bar(r["A_beta"], n, 1)),
                                worst(dz, r["dz"], bar(r["A_dz"], bn_bwd_chain(c.M), 1))))
    for fam, n in BCE_CASES:
        i, r = bce_inputs(fam, n), bce_ref(fam, n)
        for o in ORDERS:
            loss, dz, _ = bce_restate(i, o, exact_terms=r)
            up(w, "bce_loss", worst(loss, r["loss"], bar(r["A_loss"], bce_chain(n), 1)))
            up(w, "bce_dz", worst(dz, r["dz"], EPS32 * r["A_dz"] + TINY))
        z = i["z"]
        e = np.exp(-np.abs(z))
        up(t, "log1p", rel_error(np.log1p(e), r["soft"]))
        up(t, "sigmoid", rel_error(np.where(z >= 0, F32(1) / (F32(1) + e), e / (F32(1) + e)), r["sig"]))
    for c in EVAL_CASES.values():
        i = eval_inputs(c, "float")
        r = eval_ref(c, i, "float")
        for o in ORDERS:
            up(w, "eval_z", worst(eval_restate(c, i, o)[0], r["z"], bar(r["A_z"], eval_chain(c.K), 1)))
        for fam in ("int", "float"):
            i = eval_inputs(c, fam)
            r = eval_ref(c, i, fam)
            z32 = r["z"].astype(F32)
            rs32 = r["rs"].astype(F32)
            k = {n: v.astype(F64) for n, v in i.items()}
            tt = k["gamma"] * ((z32.astype(F64) - k["running_mean"]) * rs32.astype(F64))
            up(w, "eval_epi", worst(eval_restate(c, i, z=z32, rs=rs32)[1], np.maximum(tt + k["beta"], 0), EPS32 * (np.abs(tt) + np.abs(k["beta"]))))
            up(t, "rsqrt", rel_error(F32(1) / np.sqrt(i["running_var"] + EVAL_EPS), 1.0 / np.sqrt((i["running_var"] + EVAL_EPS).astype(F64))))
    for c in HEAD_CASES.values():
        i = head_inputs(c, "float")
        r = head_ref(c, i, "float")
        full = Head(c.M, c.K, c.M, c.b, c.fo, c.extra, True)
        for o in ORDERS:
            zl, pr = head_restate(full, i, o)
            up(w, "head", worst(zl, r["logits"], bar(r["A"], head_chain(c.K), 1)))
            up(t, "prob", rel_error(pr, sigmoid64(zl)))
    return w, t, row0


def round_up(x, step=0.25):
    return float(np.ceil(x / step - 1e-9) * step)


if __name__ == "__main__":
    w, t, row0 = measure()
    print(f"{'kind':10s} {'worst':>8s} {'x 4':>8s} {'C':>6s}")
    for k in C:
        print(f"{k:10s} {w[k]:8.3f} {MARGIN * w[k]:8.2f} {C[k]:6.2f}")
    print(f"{'transc.':10s} {'worst':>8s} {'x 4':>8s} {'T':>6s}")
    for k in T:
        print(f"{k:10s} {t[k]:8.2f} {MARGIN * t[k]:8.1f} {T[k]:6.1f}")
    for (o, name), r in sorted(row0.items()):
        print(f"bn_stats ratio (C = 1) {o:8s} {name}: {r:.3f}")
