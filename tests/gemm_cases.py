"""Cases, seeded inputs, bars and host restatements of the GEMM matrix: ``dfm_gemm_f32`` on its four routes (the tiled
kernel gemm_f32_kernel<A_KC, B_KC, FAST, FAST> of csrc/gemm_f32.hip with its split reduction gemm_f32_reduce, the rows
kernel gemm_rows_kernel<NT, K> and the streamed weight gradient gemm_wgrad_kernel<T1, T2> of csrc/gemm_skinny.hip),
``dfm_weight_grad_f32`` with its deferred forms, and ``dfm_partials_finish`` (csrc/partial_reduce.h).  Shared by
tests/test_cpu_gemm_reference.py (which proves on the host that every case takes the route, the split count and the
launch plan it claims, that the integer family is exact, that a plain float32 evaluation stays inside every float bar
and that the listed mistakes change the result) and tests/test_gpu_gemm_matrix.py (which runs them).  Plain numpy;
importing this needs neither a GPU nor the library.

Two input families.

  int    every operand, bias and initial C is a nonzero integer in [-3, 3] held as float32.  Every product is at most
         9 and every partial sum at most 9 * 131 077 + 6 < 2^24, so each sum is exact in float32 in ANY order: the
         result must equal the float64 reference bit for bit, and since no term is zero, a (row, k) term that is
         dropped, doubled or fetched from another address moves the output.  This family carries the coverage.
  float  N(0, 1) operands, held to

             |got - fp64| <= C[kind] * EPS32 * sqrt(n) * A

         with A = the fp64 sum of |terms| of the element and n = the longest chain of additions that reaches it,
         restated from the launch plan (chain_length):
             rows    K (+ 1 for the bias, + 1 for accumulate)
             wgrad   32 * chunks_per_wave + 2 + ceil(blocks / 4) + 3
             tiled   k_per_split / 2 + 1 + splits
         This family is there to see a loss of precision, not an indexing error.

C[kind] is measured, not chosen: 4 x the worst ratio |float32 restatement - fp64| / (EPS32 sqrt(n) A) that a numpy
float32 restatement of the same blocking reaches over ALL float cases, in the kernel's own order and in pairwise order
(np.sum over the contiguous axis); the factor 4 pays for fma contraction and for the fixed order of the kernels (the
margin of tests/record_cases.py), rounded up.  `python -m tests.gemm_cases` prints the ratios:

    kind     worst ratio   x 4     C
    rows     0.519         2.08    2.25     (dfm_gemm_f32 on the rows kernel)
    wgrad    0.013         0.052   0.1      (dfm_weight_grad_f32, and dfm_gemm_f32 on the streamed weight gradient)
    tiled    0.193         0.77    1.0      (dfm_gemm_f32 on the tiled kernel, one split or several)

The worst rows ratio sits in the shortest chain (K = 16, where one rounding is a visible share of the bar).  The weight
gradient's is small because its n counts the longest chain of the launch plan (54 additions at 8197 rows) while A sums
all 8197 |terms|: the bar is loose against rounding by construction, which is why the integer family, not this one,
carries the coverage.  Its 131 077-row case reaches 0.002.
"""
from __future__ import annotations

import functools
import re
import zlib
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

EPS32 = 2.0 ** -23
F32 = np.float32
C = dict(rows=2.25, wgrad=0.1, tiled=1.0)
MARGIN = 4.0

# the kernels' constants
BM = BN = 64
BK = 32                              # gemm_core.h
WAVES = 4                            # kWaves
MAX_RESIDENT_WAVES = 2 * 256 * WAVES   # kMaxResidentWaves, kWgradWaves
SKINNY_MIN_ROWS = 8192               # kSkinnyMinRows
MAX_PARTIAL_JOBS = 8                 # kMaxPartialJobs
TILED_SLOW, TILED_FAST, ROWS, WGRAD = 0, 1, 2, 3     # DFM_GEMM_ROUTE_*

# (N, K) of gemm_rows_kernel<N / 32, K>; (192, 32) is two launches of <3, 32>
ROWS_SHAPES = ((32, 16), (32, 32), (32, 64), (32, 96), (32, 192), (64, 32), (64, 64), (96, 16), (96, 32), (192, 32))
ROWS_SPECIAL = (192, 32)
# (N1, N2) of gemm_wgrad_kernel<N1 / 32, N2 / 32>; the pair kernel is <6, 1> + <1, 2>
WGRAD_SHAPES = ((192, 32), (32, 64), (32, 32), (64, 32), (96, 32), (64, 64), (32, 96))
WGRAD_PAIR = ((192, 32), (32, 64))
M_BASE = SKINNY_MIN_ROWS + 5
M_SWEEP = (8192, 8193, 8223, 65569, 131077)


def ceil_div(a, b):
    return -(-a // b)


# =====================================================================================================================
# host restatements of the launch plans and of the route
# =====================================================================================================================
def rows_plan(M: int) -> dict:
    """gemm_rows_try: 32-row tiles, tiles per wave, live waves, workgroups."""
    ntiles = ceil_div(M, 32)
    tpw = ceil_div(ntiles, MAX_RESIDENT_WAVES)
    waves = ceil_div(ntiles, tpw)
    return dict(ntiles=ntiles, tpw=tpw, waves=waves, grid=ceil_div(waves, WAVES))


def wgrad_plan(M: int) -> dict:
    """wgrad_blocks: 32-row chunks, chunks per wave, live waves, workgroups (= partial rows)."""
    nchunks = ceil_div(M, 32)
    cpw = ceil_div(nchunks, MAX_RESIDENT_WAVES)
    waves = ceil_div(nchunks, cpw)
    return dict(nchunks=nchunks, cpw=cpw, waves=waves, blocks=ceil_div(waves, WAVES))


def wgrad_supported(M, n1, n2) -> bool:
    return M >= SKINNY_MIN_ROWS and (n1, n2) in WGRAD_SHAPES


def wgrad_workspace_bytes(M, n1, n2) -> int:
    return 4 * wgrad_plan(M)["blocks"] * (n1 * n2 + n1) if wgrad_supported(M, n1, n2) else 0


def pick_splits(m, n, k) -> int:
    tiles = ceil_div(m, BM) * ceil_div(n, BN)
    if tiles >= 96 or k <= 8 * BK:
        return 1
    return max(1, min(ceil_div(256, tiles), k // (4 * BK)))


def split_plan(m, n, k, has_workspace) -> Tuple[int, int]:
    """(splits launched, k per split): pick_splits, then whole 32-deep slices per split."""
    s = pick_splits(m, n, k) if has_workspace else 1
    kps = ceil_div(ceil_div(k, s), BK) * BK
    return ceil_div(k, kps), kps


def operand_fast(shift, ld, kc, rows, kdim) -> bool:
    return shift % 4 == 0 and ld % 4 == 0 and (kdim % 4 == 0 if kc else rows % 4 == 0)


def route(a_shift, lda, a_kc, b_shift, ldb, b_kc, m, n, k, has_bias, has_workspace) -> int:
    """dfm_gemm_route restated; a pointer is given as its distance in floats from a 16-byte boundary."""
    if a_kc and m >= SKINNY_MIN_ROWS and a_shift % 4 == 0 and lda % 4 == 0 and \
            not (b_kc and (b_shift % 4 != 0 or ldb % 4 != 0)) and (n, k) in ROWS_SHAPES:
        return ROWS
    if not a_kc and not b_kc and not has_bias and has_workspace and wgrad_supported(k, m, n):
        return WGRAD
    fast = operand_fast(a_shift, lda, a_kc, m, k) and operand_fast(b_shift, ldb, b_kc, n, k)
    return TILED_FAST if fast else TILED_SLOW


def parse_instantiations() -> Tuple[set, set]:
    """The DFM_ROWS(NT, K) and DFM_WG(T1, T2) uses of csrc/gemm_skinny.hip as {(N, K)} and {(N1, N2)}."""
    src = (Path(__file__).resolve().parent.parent / "deepfm_amd" / "csrc" / "gemm_skinny.hip").read_text()
    rows = {(32 * int(a), int(b)) for a, b in re.findall(r"DFM_ROWS\((\d+), (\d+)\)", src)}
    wg = {(32 * int(a), 32 * int(b)) for a, b in re.findall(r"DFM_WG\((\d+), (\d+)\)", src)}
    return rows, wg


# =====================================================================================================================
# cases
# =====================================================================================================================
@dataclass(frozen=True)
class Gemm:
    """One dfm_gemm_f32 call: C[m, n] (+)= sum_k A(m, k) B(n, k) (+ bias).  *_pad: floats added to the leading
    dimension; *_shift: floats the pointer sits behind a 16-byte boundary; ws: a workspace is passed."""
    name: str
    m: int
    n: int
    k: int
    a_kc: bool
    b_kc: bool
    bias: bool
    acc: bool
    ws: bool
    route: int
    splits: int = 1
    a_pad: int = 0
    b_pad: int = 0
    c_pad: int = 0
    a_shift: int = 0
    b_shift: int = 0
    families: Tuple[str, ...] = ("int",)
    why: str = ""

    @property
    def lda(self):
        return (self.k if self.a_kc else self.m) + self.a_pad

    @property
    def ldb(self):
        return (self.k if self.b_kc else self.n) + self.b_pad

    @property
    def ldc(self):
        return self.n + self.c_pad

    @property
    def kind(self):
        return {ROWS: "rows", WGRAD: "wgrad"}.get(self.route, "tiled")

    def route_args(self):
        return (self.a_shift, self.lda, self.a_kc, self.b_shift, self.ldb, self.b_kc, self.m, self.n, self.k,
                self.bias, self.ws)


@dataclass(frozen=True)
class WGrad:
    """One dfm_weight_grad_f32 call: dW[n1, n2] (+)= g^T x, db[n1] (+)= column sums of g over M rows."""
    name: str
    M: int
    n1: int
    n2: int
    g_pad: int = 0
    x_pad: int = 0
    dw_pad: int = 0
    db: bool = True
    acc: bool = False
    families: Tuple[str, ...] = ("int",)
    why: str = ""

    kind = "wgrad"


def _flags(j):
    """(bias, accumulate) of the j-th member of a group: both values of each within any two neighbours."""
    return j % 2 == 0, ((j + 1) // 2) % 2 == 0


def _gemm(name, m, n, k, a_kc, b_kc, bias, acc, ws, **kw) -> Gemm:
    """A case whose route and split count are the restated ones (the CPU test holds the library to them)."""
    g = Gemm(name, m, n, k, a_kc, b_kc, bias, acc, ws, route=-1, **kw)
    r = route(*g.route_args())
    s = split_plan(m, n, k, ws)[0] if r in (TILED_SLOW, TILED_FAST) else 1
    return Gemm(name, m, n, k, a_kc, b_kc, bias, acc, ws, route=r, splits=s, **kw)


def _rows_cases() -> List[Gemm]:
    cs, seen = [], {}
    for N, K in ROWS_SHAPES:                       # every instantiation, both weight layouts
        for w_kc in (False, True):
            j = seen.get(N, 0)
            seen[N] = j + 1
            bias, acc = _flags(j)
            cs.append(_gemm(f"rows_N{N}_K{K}_kc{int(w_kc)}", M_BASE, N, K, True, w_kc, bias, acc, False,
                            families=("int", "float"), why=f"gemm_rows_kernel<{N // 32 if N < 192 else 3}, {K}>, w_kc {int(w_kc)}"))
    for i, (N, K) in enumerate(((32, 32), (32, 192), (192, 32))):      # prefetch | no prefetch | two launches
        for j, M in enumerate(M_SWEEP):
            bias, acc = _flags(i + j)
            cs.append(_gemm(f"rows_N{N}_K{K}_M{M}", M, N, K, True, (i + j) % 2 == 0, bias or N == 192, acc, False,
                            families=("int", "float") if (N, K) == (32, 32) else ("int",),
                            why=f"{rows_plan(M)['ntiles']} tiles, {rows_plan(M)['tpw']} per wave, last tile {(M - 1) % 32 + 1} rows"))
    for i, (N, K) in enumerate(((64, 32), (32, 96))):                  # padded strides, the padding left alone
        for w_kc in (False, True):
            bias, acc = _flags(2 * i + int(w_kc))
            cs.append(_gemm(f"rows_strides_N{N}_K{K}_kc{int(w_kc)}", 8193, N, K, True, w_kc, bias, acc, False, a_pad=4,
                            b_pad=4 if w_kc else 1, c_pad=3, why="lda = K + 4, ldw = K + 4 / N + 1, ldc = N + 3"))
    off = dict(lda1=dict(a_pad=1), a_shift=dict(a_shift=1), w_shift=dict(b_shift=1), ldw1=dict(b_pad=1))
    for j, (tag, kw) in enumerate(off.items()):                        # falling off the route: tiled, still exact
        bias, acc = _flags(j)
        cs.append(_gemm(f"rows_off_{tag}", 8193, 64, 32, True, True, bias, acc, False, c_pad=3, why="not the rows kernel", **kw))
    cs.append(_gemm("rows_off_M8191", 8191, 64, 32, True, True, True, True, False, c_pad=3, why="one row short of the rows kernel"))
    return cs


TILED_MN = ((1, 65), (63, 130), (64, 1), (65, 64), (130, 63), (1, 130))
TILED_K = (1, 15, 16, 17, 31, 32, 33, 65)
LAYOUTS = ((True, True), (True, False), (False, True), (False, False))
SPLIT_K = {896: 7, 1024: 8, 1152: 9, 2176: 17, 1000: 7, 1100: 7}      # K -> splits launched at M = N <= 64


def _tiled_cases() -> List[Gemm]:
    cs = []
    # the eight instantiations: each layout on the fast form and on the slow one, forced four ways
    how = dict(fast=dict(a_pad=4, b_pad=4), a_shift=dict(a_shift=1), a_ld=dict(a_pad=1), b_shift=dict(b_shift=1),
               b_ld=dict(b_pad=2))
    for li, (a_kc, b_kc) in enumerate(LAYOUTS):
        for j, (tag, kw) in enumerate(how.items()):
            bias, acc = _flags(li + j)
            cs.append(_gemm(f"tiled_inst_a{int(a_kc)}b{int(b_kc)}_{tag}", 68, 72, 36, a_kc, b_kc, bias, acc, False, c_pad=3,
                            families=("int", "float") if not (bias or acc) else ("int",),
                            why=f"gemm_f32_kernel<{int(a_kc)}, {int(b_kc)}, {tag == 'fast'}>", **kw))
    # tile and slice edges
    for pi, (m, n) in enumerate(TILED_MN):
        for ki, k in enumerate(TILED_K):
            layouts = LAYOUTS if (m, n) == (63, 130) else (LAYOUTS[(pi + ki) % 4],)
            for a_kc, b_kc in layouts:
                i = pi + ki + 2 * int(a_kc) + int(b_kc)
                bias, acc = _flags(i)
                cs.append(_gemm(f"tiled_edge_M{m}_N{n}_K{k}_a{int(a_kc)}b{int(b_kc)}", m, n, k, a_kc, b_kc, bias, acc,
                                i % 3 == 0, a_pad=(0, 4, 1)[i % 3], b_pad=(4, 0, 3)[i % 3], c_pad=(3, 0, 5)[ki % 3]))
    # split reduction: the slabs of gemm_f32_reduce around its unroll of 8, a short last split, the one-split twin
    for si, (mn, (a_kc, b_kc)) in enumerate(((64, (False, False)), (40, (True, True)))):
        for ki, (k, s) in enumerate(SPLIT_K.items()):
            bias, acc = _flags(si + ki)
            for ws in (True, False):
                g = _gemm(f"tiled_split_MN{mn}_K{k}_{'ws' if ws else 'nows'}", mn, mn, k, a_kc, b_kc, bias, acc, ws,
                          c_pad=4 * si, families=("int", "float") if not (bias or acc) else ("int",),
                          why=f"{s if ws else 1} split(s)")
                assert g.splits == (s if ws else 1), (g.name, g.splits)
                cs.append(g)
    # the weight-gradient product through dfm_gemm_f32: streamed with a workspace, tiled without one or with a bias
    cs.append(_gemm("dispatch_wgrad_ws", 64, 32, M_BASE, False, False, False, True, True, why="route 3, accumulating"))
    cs.append(_gemm("dispatch_wgrad_nows", 64, 32, M_BASE, False, False, False, True, False, why="tiled, one split of 8197"))
    cs.append(_gemm("dispatch_wgrad_bias", 64, 32, M_BASE, False, False, True, False, True, why="a bias: tiled, 52 splits of 160"))
    cs.append(_gemm("dispatch_wgrad_pad", 32, 96, 8193, False, False, False, False, True, a_pad=1, b_pad=3, c_pad=5,
                    families=("int", "float"), why="route 3, padded"))
    return cs


def _wgrad_cases() -> List[WGrad]:
    cs = [WGrad(f"wgrad_{a}x{b}", M_BASE, a, b, families=("int", "float"), why=f"gemm_wgrad_kernel<{a // 32}, {b // 32}>")
          for a, b in WGRAD_SHAPES]
    for a, b in ((32, 32), (192, 32), (64, 64)):
        for M in M_SWEEP:
            p = wgrad_plan(M)
            cs.append(WGrad(f"wgrad_{a}x{b}_M{M}", M, a, b, families=("int", "float") if (a, b) == (32, 32) else ("int",),
                            why=f"{p['cpw']} chunk(s) per wave, {p['blocks']} blocks"))
    for a, b in ((64, 32), (32, 96)):
        cs.append(WGrad(f"wgrad_{a}x{b}_strides", M_BASE, a, b, g_pad=1, x_pad=3, dw_pad=5, why="ldg = N1 + 1, ldx = N2 + 3, lddw = N2 + 5"))
        cs.append(WGrad(f"wgrad_{a}x{b}_nodb", M_BASE, a, b, db=False, why="db = NULL"))
        cs.append(WGrad(f"wgrad_{a}x{b}_acc", M_BASE, a, b, acc=True, dw_pad=5, why="accumulate onto nonzero dW and db"))
    return cs


GEMM_CASES: Dict[str, Gemm] = {c.name: c for c in _rows_cases() + _tiled_cases()}
WGRAD_CASES: Dict[str, WGrad] = {c.name: c for c in _wgrad_cases()}
ROWS_NAMES = [n for n in GEMM_CASES if n.startswith("rows_")]
TILED_NAMES = [n for n in GEMM_CASES if not n.startswith("rows_")]
PAIR_REFUSED = (((64, 32), (32, 64)), ((192, 32), (32, 32)), ((32, 64), (192, 32)))   # pairs without a joint kernel

# dfm_partials_finish alone
FINISH_BLOCKS = (1, 2, 3, 4, 5, 7, 8, 28, 29, 31, 32, 33, 35, 36, 37, 61, 64, 65, 157, 416)
FINISH_SHAPES = ((32, 32), (5, 3), (192, 32))
LN_FINISH_BLOCKS = (1, 255, 256, 257, 513)
LN_FINISH_DIMS = (1, 10, 64)


def finish_flags(si: int, bi: int) -> Tuple[int, bool, bool]:
    """(ldw padding, out_b given, accumulate) of kind-0 finish case (shape si, block count bi)."""
    return 5 * ((bi + si) & 1), bool(((bi >> 1) + si) & 1), bool((bi >> 2) & 1)


# one launch of eight jobs: (kind, blocks, n1, n2, ldw padding, out_b given, accumulate)
MIXED_JOBS = ((0, 5, 32, 32, 0, True, False), (1, 257, 10, 0, 0, True, True), (0, 1, 5, 3, 2, False, True),
              (1, 1, 64, 0, 0, True, True), (0, 33, 192, 32, 5, True, True), (1, 513, 1, 0, 0, True, True),
              (0, 65, 64, 64, 0, False, False), (1, 256, 64, 0, 0, True, True))


def finish_grid(jobs) -> List[int]:
    """first_block of dfm_partials_finish: 64 elements per workgroup (kind 0), one column per workgroup (kind 1)."""
    first = [0]
    for kind, blocks, n1, n2, *_ in jobs:
        first.append(first[-1] + (ceil_div(n1 * n2 + n1, 64) if kind == 0 else n1))
    return first


# =====================================================================================================================
# inputs (numpy; the GPU test draws the same families on the device)
# =====================================================================================================================
def seed_of(name: str) -> int:
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def values(rng, shape, family: str) -> np.ndarray:
    if family == "float":
        return rng.standard_normal(shape).astype(F32)
    v = rng.integers(-3, 3, shape)                    # -3 .. 2
    return np.where(v >= 0, v + 1, v).astype(F32)       # -3 .. -1, 1 .. 3


def input_key(case, family: str) -> str:
    """What a case's inputs are seeded from: the split cases and their one-split twins share theirs."""
    name = case.name
    for suffix in ("_ws", "_nows"):
        if name.startswith("tiled_split_") and name.endswith(suffix):
            name = name[:-len(suffix)]
    return name + ":" + family


def gemm_inputs(case: Gemm, family: str, rows: Optional[np.ndarray] = None) -> dict:
    """Logical operands of a case: a (m, k), b (n, k), bias (n,), c0 (m, n); `rows`: only these rows of a and c0."""
    rng = np.random.default_rng(seed_of(input_key(case, family)))
    a = values(rng, (case.m, case.k), family)
    b = values(rng, (case.n, case.k), family)
    bias = values(rng, (case.n,), family)
    if rows is not None:
        a = a[rows]
    c0 = values(rng, (a.shape[0], case.n), family)
    return dict(a=a, b=b, bias=bias if case.bias else None, c0=c0 if case.acc else None)


def wgrad_inputs(case: WGrad, family: str) -> dict:
    rng = np.random.default_rng(seed_of(input_key(case, family)))
    return dict(g=values(rng, (case.M, case.n1), family), x=values(rng, (case.M, case.n2), family),
                dw0=values(rng, (case.n1, case.n2), family) if case.acc else None,
                db0=values(rng, (case.n1,), family) if case.acc else None)


def max_abs_sum(case) -> int:
    """Upper bound of |any partial sum| of the integer family: 9 per term, 3 for the bias, 3 for the initial C."""
    return 9 * (case.M if isinstance(case, WGrad) else case.k) + 6


# =====================================================================================================================
# bars
# =====================================================================================================================
def chain_length(case) -> int:
    if isinstance(case, WGrad) or case.route == WGRAD:
        p = wgrad_plan(case.M if isinstance(case, WGrad) else case.k)
        return 32 * p["cpw"] + 2 + ceil_div(p["blocks"], 4) + 3
    if case.route == ROWS:
        return case.k + int(case.bias) + int(case.acc)
    splits, kps = split_plan(case.m, case.n, case.k, case.ws)
    return kps // 2 + 1 + splits


def bar(A, n, c):
    return c * EPS32 * np.sqrt(float(n)) * np.asarray(A, dtype=np.float64)


def ratio(got, want, A, n, c=1.0) -> float:
    """Worst |got - want| / bar; a non-finite element fails."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    if not np.isfinite(err).all():
        return float("inf")
    b = np.broadcast_to(bar(A, n, c), err.shape)
    return float(np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0)).max()) if err.size else 0.0


# =====================================================================================================================
# references and float32 restatements
# =====================================================================================================================
def gemm_ref(inp, dt=np.float64):
    """(result, A = sum of |terms|) in `dt` arithmetic by one matmul."""
    a, b = inp["a"].astype(dt), inp["b"].astype(dt)
    out, A = a @ b.T, np.abs(a) @ np.abs(b).T
    for t in (inp["bias"], inp["c0"]):
        if t is not None:
            out, A = out + t.astype(dt), A + np.abs(t.astype(dt))
    return out, A


def _pairwise_dot(a, b):
    """float32 sum_k a[m, k] b[n, k], each sum by numpy's pairwise np.sum over the contiguous axis."""
    out = np.empty((a.shape[0], b.shape[0]), dtype=F32)
    for j in range(b.shape[0]):
        out[:, j] = np.sum(a * b[j], axis=1, dtype=F32)
    return out


def rows_f32(inp, order: str):
    """gemm_rows_kernel: the accumulators start at the bias, one chain over k in the lane-half order
    k = 8 (i / 4) + i % 4, then + 4; an accumulating store adds the chain to C."""
    a, b = inp["a"], inp["b"]
    bias = inp["bias"] if inp["bias"] is not None else np.zeros(b.shape[0], dtype=F32)
    if order == "pair":
        acc = _pairwise_dot(a, b) + bias
    else:
        acc = np.broadcast_to(bias, (a.shape[0], b.shape[0])).astype(F32)
        for i in range(a.shape[1] // 2):
            for k in (8 * (i // 4) + i % 4, 8 * (i // 4) + i % 4 + 4):
                acc = acc + a[:, k, None] * b[None, :, k]
    return acc + inp["c0"] if inp["c0"] is not None else acc


def tiled_f32(inp, splits, kps, order: str):
    """gemm_f32_kernel: per split, the two k-halves of every 32-deep slice are separate chains, added half 0 + half 1;
    one split: + bias, then + C; several: (C or 0) + bias + (the slabs in order)."""
    a, b = inp["a"], inp["b"]
    K = a.shape[1]
    zero = np.zeros((a.shape[0], b.shape[0]), dtype=F32)
    slabs = []
    for s in range(splits):
        kb, ke = s * kps, min(K, (s + 1) * kps)
        if order == "pair":
            slabs.append(_pairwise_dot(a[:, kb:ke], b[:, kb:ke]))
            continue
        half = [zero.copy(), zero.copy()]
        for k in range(kb, ke):
            h = ((k - kb) % BK) // (BK // 2)
            half[h] = half[h] + a[:, k, None] * b[None, :, k]
        slabs.append(half[0] + half[1])
    bias = inp["bias"] if inp["bias"] is not None else F32(0)
    if splits == 1:
        v = slabs[0] + bias
        return inp["c0"] + v if inp["c0"] is not None else v
    t = zero.copy()
    for sl in slabs:
        t = t + sl
    return ((inp["c0"] if inp["c0"] is not None else zero) + bias) + t


def wgrad_partials(g, x, M: int, dt=F32, skip_chunk: Optional[int] = None, db_even_only: bool = False):
    """gemm_wgrad_kernel in `dt`: per-workgroup partials (blocks, n1 * n2 + n1).  A wave adds its 32 * cpw rows in row
    order (db: each lane half its alternate rows, then half 0 + half 1); the waves of a workgroup are added
    (0 + 2) + (1 + 3).  skip_chunk / db_even_only: the mistakes of the CPU test."""
    p = wgrad_plan(M)
    rpw, nw = 32 * p["cpw"], 4 * p["blocks"]
    n1, n2 = g.shape[1], x.shape[1]
    gp = np.zeros((nw * rpw, n1), dtype=dt)
    xp = np.zeros((nw * rpw, n2), dtype=dt)
    gp[:M], xp[:M] = g, x
    if skip_chunk is not None:
        gp[32 * skip_chunk:32 * skip_chunk + 32] = 0
    gp, xp = gp.reshape(nw, rpw, n1), xp.reshape(nw, rpw, n2)
    acc = np.zeros((nw, n1, n2), dtype=dt)
    col = np.zeros((2, nw, n1), dtype=dt)
    for j in range(rpw):
        acc = acc + gp[:, j, :, None] * xp[:, j, None, :]
        col[j % 2] = col[j % 2] + gp[:, j]
    col = col[0] if db_even_only else col[0] + col[1]
    full = np.concatenate([acc.reshape(nw, n1 * n2), col], axis=1).reshape(p["blocks"], 4, -1)
    return (full[:, 0] + full[:, 2]) + (full[:, 1] + full[:, 3])


def finish_kind0(partial, skip_block: Optional[int] = None):
    """wgrad_reduce_body: thread group g adds blocks g, g + 4, ... in order; then ((p0 + p1) + p2) + p3."""
    blocks = partial.shape[0]
    part = []
    for gi in range(4):
        t = np.zeros(partial.shape[1], dtype=partial.dtype)
        for s in range(gi, blocks, 4):
            if s != skip_block:
                t = t + partial[s]
        part.append(t)
    return ((part[0] + part[1]) + part[2]) + part[3]


def finish_kind1(partial):
    """layernorm_finalize_body: thread t adds rows t, t + 256, ...; a binary tree over the 256 sums.  partial
    (blocks, 2, D) -> (2, D)."""
    blocks = partial.shape[0]
    red = np.zeros((256,) + partial.shape[1:], dtype=partial.dtype)
    for i in range(blocks):
        red[i % 256] = red[i % 256] + partial[i]
    w = 128
    while w > 0:
        red[:w] = red[:w] + red[w:2 * w]
        w //= 2
    return red[0]


def wgrad_f32(inp, M: int, order: str):
    """(dW, db) of dfm_weight_grad_f32 in float32 (accumulate = 0)."""
    g, x = inp["g"], inp["x"]
    n1, n2 = g.shape[1], x.shape[1]
    if order == "pair":
        dw = _pairwise_dot(np.ascontiguousarray(g.T), np.ascontiguousarray(x.T))
        return dw, np.sum(np.ascontiguousarray(g.T), axis=1, dtype=F32)
    out = finish_kind0(wgrad_partials(g, x, M))
    return out[:n1 * n2].reshape(n1, n2), out[n1 * n2:]


def wgrad_ref(inp):
    """fp64 (dW, db, A of dW, A of db) without the initial values."""
    g, x = inp["g"].astype(np.float64), inp["x"].astype(np.float64)
    return g.T @ x, g.sum(0), np.abs(g).T @ np.abs(x), np.abs(g).sum(0)


RESTATE_ROWS = 40          # the rows kernel's outputs are independent per row: the restatement takes the first and last 40


def restate_rows(m: int) -> np.ndarray:
    return np.arange(m) if m <= 2 * RESTATE_ROWS else np.r_[0:RESTATE_ROWS, m - RESTATE_ROWS:m]


def f32_ratio(name: str, order: str) -> Tuple[str, float]:
    """(kind, worst |float32 restatement - fp64| / (EPS32 sqrt(n) A)) of a float case."""
    if name in WGRAD_CASES:
        case = WGRAD_CASES[name]
        inp = wgrad_inputs(case, "float")
        dw, db = wgrad_f32(inp, case.M, order)
        rdw, rdb, Adw, Adb = wgrad_ref(inp)
        n = chain_length(case)
        return "wgrad", max(ratio(dw, rdw, Adw, n), ratio(db, rdb, Adb, n))
    case = GEMM_CASES[name]
    n = chain_length(case)
    if case.route == WGRAD:
        inp = gemm_inputs(case, "float")
        w = dict(g=np.ascontiguousarray(inp["a"].T), x=np.ascontiguousarray(inp["b"].T))
        dw, _ = wgrad_f32(w, case.k, order)
        ref, A = gemm_ref(inp)
        return "wgrad", ratio(dw + inp["c0"] if inp["c0"] is not None else dw, ref, A, n)
    if case.route == ROWS:
        inp = gemm_inputs(case, "float", rows=restate_rows(case.m))
        got = rows_f32(inp, order)
    else:
        inp = gemm_inputs(case, "float")
        got = tiled_f32(inp, *split_plan(case.m, case.n, case.k, case.ws), order)
    ref, A = gemm_ref(inp)
    return case.kind, ratio(got, ref, A, n)


def float_cases() -> List[str]:
    return [n for n, c in {**GEMM_CASES, **WGRAD_CASES}.items() if "float" in c.families]


@functools.lru_cache(maxsize=None)
def worst_ratios() -> Dict[str, float]:
    worst = dict(rows=0.0, wgrad=0.0, tiled=0.0)
    for nm in float_cases():
        for order in ("kernel", "pair"):
            kind, r = f32_ratio(nm, order)
            worst[kind] = max(worst[kind], r)
    return worst


if __name__ == "__main__":
    for nm in float_cases():
        print(nm, {o: round(f32_ratio(nm, o)[1], 3) for o in ("kernel", "pair")})
    print("worst", {k: round(v, 3) for k, v in worst_ratios().items()}, "x 4",
          {k: round(MARGIN * v, 2) for k, v in worst_ratios().items()})
