"""Cases, seeded inputs, bars and mutations of the record-kernel matrix: ``dfm_embedding_forward_record`` (emb_fwd_record<D>)
and ``dfm_embedding_backward_record`` (emb_bwd_record<D>, emb_bwd_record_fm<D>) of csrc/embedding.hip, shared by
tests/test_cpu_record_reference.py (which proves on the host that every case fits the kernels' caps and reaches the
branch it claims, that a plain float32 evaluation stays inside every bar and that the listed mistakes land outside)
and tests/test_gpu_record_matrix.py (which runs them).  Plain numpy; importing this needs neither a GPU nor the library.

Bars.  An output element that is a float32 sum is held to

    |got - fp64| <= C[kind] * EPS32 * sqrt(n) * A

with A = the fp64 sum of the absolute values of the terms that make it up and n = the length of the longest chain of
additions that reaches it, both from the fp64 restatement (tests/helpers.py: record_forward_fp64 /
record_backward_fp64).  sqrt(n) and not n: the rounding errors of a sum are independent to first order, and n would
open the bar of a 4096-term row to one whole dropped sample (c * 2^-23 * 4096 A = c * 4.9e-4 A against a term of
A / 4096 = 2.4e-4 A), which is what the matrix exists to catch.  C[kind] is 4 x the worst ratio the float32 restatement
(the same numpy statements with dt = float32) reaches over ALL cases in two summation orders, sequential and pairwise;
the factor 4 pays for fma contraction and for the kernels' own fixed order (slices of stages, the atomics of the dense
path).  Measured worst ratios (max over the cases and both orders; `python -m tests.record_cases` prints them) and
the constants derived from them:

    kind       worst ratio   x 4     C
    forward    0.563         2.25    2.5      (first_order, field_embeddings, flat_embeddings, fm, fm_sum)
    table      0.647         2.59    3.0      (the (V, d) and (V, 1) tables of SPARSE and SEQUENCE fields)
    dense      0.369         1.48    1.5      (Linear(1, d) and Linear(1, 1) of DENSE fields)
    proj       0.402         1.61    2.0      (projection weights)

The worst ratios sit in the short sums (n of 2 to 20, where one rounding is a visible share of the bar); the 4096-term
sums of the B = 4097 cases reach 0.27 (table), 0.011 (dense) and 0.016 (proj).

An element whose A is 0 (a row nobody names) has bar 0: it must be exactly 0.
"""
from __future__ import annotations

import functools
import types
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from tests import helpers as H

EPS32 = 2.0 ** -23
F32 = np.float32
C = dict(forward=2.5, table=3.0, dense=1.5, proj=2.0)
MARGIN = 4.0
FM_FLOOR = 0.05            # |FM value| / A of every sample of every case with two fields or more

BWD_THREADS = 256          # kBwdThreads
BWD_STAGE = 256            # kBwdStage
BWD_MAX_PARTS = 16         # kBwdMaxParts
BWD_ROWS = 2               # kBwdRows
RECORD_THREADS = 512       # kRecordThreads
FM_DIMS = (4, 8, 16, 32, 64)

LD_PAD_FLAT = 8            # the gather's flat rows: ld = T + 8, pointer 16 bytes into its buffer
LD_PAD_G = 4               # g_flat: ld = T + 4
LD_PAD_SAVED = 12          # the saved flat handed to the backward: ld = T + 12


def bar(A, n, c):
    return c * EPS32 * np.sqrt(np.maximum(np.asarray(n, dtype=np.float64), 1.0)) * np.asarray(A, dtype=np.float64)


def ratio(got, want, A, n, c) -> float:
    """Worst |got - want| / bar; an element with bar 0 must be met exactly; a non-finite element fails."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    b = np.broadcast_to(bar(A, n, c), err.shape)
    if err.size == 0:
        return 0.0
    if not np.isfinite(err).all():
        return float("inf")
    r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def kind_of(key: str, fields) -> str:
    """Which constant a gradient is held to."""
    if key.startswith("projections."):
        return "proj"
    name = key.split(".")[1]
    spec = next(f for f in fields if f["name"] == name)
    return "dense" if spec["type"] == "dense" else "table"


# =====================================================================================================================
# schemas
# =====================================================================================================================
def sp(name, V, d):
    return dict(name=name, type="sparse", vocab=V, dim=d, max_len=1, combiner="mean")


def seq(name, V, d, L, comb):
    return dict(name=name, type="sequence", vocab=V, dim=d, max_len=L, combiner=comb)


def de(name, d):
    return dict(name=name, type="dense", vocab=0, dim=d, max_len=1, combiner="mean")


@dataclass(frozen=True)
class Case:
    name: str
    D: int
    fields: Tuple[dict, ...]
    B: int
    why: str                      # the branch the case exists for
    fwd: bool = True              # the record gather takes it
    bwd: bool = True              # the record backward takes it
    refusal: Optional[str] = None   # which documented refusal it is a case of

    @property
    def T(self):
        return sum(f["dim"] for f in self.fields)

    @property
    def F(self):
        return len(self.fields)


def fwd_sb(F, D):
    """describe_record: whole samples per workgroup."""
    per = F * (D // 4)
    return 1 if per >= RECORD_THREADS else RECORD_THREADS // per


def row_tile(d):
    """describe_bwd_record: table rows per workgroup, R = 2 * (256 // (d/4 + 1))."""
    return BWD_ROWS * (BWD_THREADS // (d // 4 + 1))


def bwd_slices(B):
    """(parts, rows per part): bwd_parts and rows_per_part of describe_bwd_record."""
    stages = -(-B // BWD_STAGE)
    parts = max(1, min(BWD_MAX_PARTS, stages))
    return parts, -(-B // parts)


def _mixed3(D):
    return (sp("a", 11, D), seq("g", 9, D, 3, "mean"), de("x", D))


def _wide(F, D):
    """F fields of width D: SPARSE but for two bags and two DENSE fields."""
    fs = [sp(f"s{i}", 5 + i % 3, D) for i in range(F)]
    if F >= 8:
        fs[1], fs[F // 2] = seq("g1", 6, D, 3, "mean"), seq("g2", 7, D, 1, "sum")
        fs[2], fs[F - 1] = de("x1", D), de("x2", D)
    return tuple(fs)


def _widths(D, ds, extra=()):
    """Every width of `ds` as a SPARSE, a SEQUENCE and a DENSE field (d != D: projected)."""
    fs, Ls, combs = [], (3, 6, 1), ("mean", "sum")
    for i, d in enumerate(ds):
        fs += [sp(f"s{d}", 23 + i, d), seq(f"g{d}", 13 + i, d, Ls[i % 3], combs[i % 2]), de(f"x{d}", d)]
    return tuple(fs) + tuple(extra)


def _narrow(D, dp):
    """The schema of the batch-size cases: one field of each kind at d == D and one projected at d = dp; `hot` is the
    field whose id 3 most samples name."""
    return (sp("u", 300, D), sp("hot", 9, dp), seq("g", 40, D, 3, "mean"), seq("h", 12, dp, 1, "sum"), de("x", D),
            de("y", dp))


def _build_cases() -> List[Case]:
    cs: List[Case] = []
    for D in FM_DIMS:
        sb = fwd_sb(3, D)
        ok = D < 64               # d = 64 is over the backward's LDS cap
        cs.append(Case(f"small_b5_D{D}", D, _mixed3(D), 5, f"emb_fwd_record<{D}> with SB = {sb} > B: dead lanes read sample B - 1", bwd=ok))
        cs.append(Case(f"small_tail_D{D}", D, _mixed3(D), 2 * sb + 3, f"SB = {sb}, B = 2 SB + 3: a partial last workgroup", bwd=ok))
        cs.append(Case(f"single_D{D}", D, (sp("only", 7, D),), 3, "a single field (F = 1)", bwd=ok,
                       refusal=None if ok else "bwd_d64"))
    for D, Fs in ((4, (64,)), (8, (64,)), (16, (64,)), (32, (63, 64)), (64, (31, 33, 64))):
        for F in Fs:
            cs.append(Case(f"wide_F{F}_D{D}", D, _wide(F, D), 9, f"F * D / 4 = {F * D // 4}: SB = {fwd_sb(F, D)}, "
                           f"{fwd_sb(F, D) * F * D // 4} threads", bwd=D < 64))
    cs.append(Case("widths_D4", 4, _widths(4, (4, 8, 12, 32)), 37, "d == D, d > D, d not a power of two at D = 4"))
    cs.append(Case("widths_D8", 8, _widths(8, (8, 4, 12, 32), (sp("s48", 17, 48),)), 37, "d == D, d < D, d > D, 12 and 48 at D = 8"))
    cs.append(Case("widths_D16", 16, _widths(16, (16, 4, 32, 12), (sp("s20", 17, 20), seq("g20", 9, 20, 3, "mean"),
                                                                 sp("s48", 19, 48))), 37,
                   "d == D, d = 4 < D, d = 32 > D, 12 / 20 / 48 at D = 16; projection jobs of 1, 2 and 3 chunks"))
    cs.append(Case("widths_D32", 32, _widths(32, (32, 4, 12, 20)), 37, "d == D, d < D, 12 and 20 at D = 32"))
    cs.append(Case("widths_D64", 64, (sp("s64", 23, 64), sp("s4", 24, 4), seq("g12", 13, 12, 3, "mean"), de("x32", 32),
                                      sp("s48", 25, 48), de("x64", 64), seq("g64", 14, 64, 6, "sum")), 37,
                   "d == D and projections from 4, 12, 32, 48 at D = 64 (gather only: no backward exists at D = 64)", bwd=False))
    v16 = [sp(f"v16_{V}", V, 16) for V in (2, 52, 101, 102, 103, 250)]
    v4 = [sp(f"v4_{V}", V, 4) for V in (129, 255, 256, 257, 600)]
    v32 = [sp(f"v32_{V}", V, 32) for V in (29, 55, 56, 57, 173)]
    cs.append(Case("vocab_D16", 16, tuple(v16 + v4 + v32 + [seq("vg12", 129, 12, 3, "mean")]), 48,
                   "V in {2, R/2 + 1, R - 1, R, R + 1, several tiles} for R = 102 (d = 16), 256 (d = 4), 56 (d = 32, 4 idle "
                   "threads), 128 (d = 12); ids on the tile edges"))
    cs.append(Case("vocab_D4", 4, tuple(sp(f"v{V}", V, 4) for V in (2, 129, 255, 256, 257, 600)), 48,
                   "the row tiles of d = 4 without a projection"))
    for B in (1, 7, 256, 257, 513, 4097):
        parts, rpp = bwd_slices(B)
        cs.append(Case(f"batch_B{B}", 8, _narrow(8, 4), B, f"B = {B}: {parts} slice(s) of {rpp}, "
                       f"{-(-rpp // BWD_STAGE)} stage(s), the last of {(rpp - 1) % BWD_STAGE + 1} sample(s)"))
    cs.append(Case("batch_B4097_D4", 4, _narrow(4, 8), 4097, "sixteen slices of 257 at D = 4, d = 8 projected"))
    cs.append(Case("batch_B4097_D16", 16, _narrow(16, 4), 4097, "sixteen slices of 257 at D = 16"))
    cs.append(Case("batch_B513_D32", 32, _narrow(32, 12), 513, "three slices of 171 at D = 32"))
    bags = [seq(f"b{L}{c[0]}", 15, 16, L, c) for L in (1, 3, 6) for c in ("mean", "sum")]
    cs.append(Case("bags_D16", 16, tuple(bags + [seq("b3p", 15, 4, 3, "mean"), sp("s", 9, 16), de("x", 16)]), 21,
                   "L in {1, 3, 6}, mean and sum; an empty bag, one id repeated, padding in the middle"))
    cs.append(Case("max_D16", 16, (seq("m6", 15, 16, 6, "max"), seq("m3p", 11, 4, 3, "max"), seq("m1w", 9, 32, 1, "max"),
                                   sp("s", 9, 16), de("x", 16)), 19,
                   "max bags in the gather; the backward refuses them (dense-autograd path only)", bwd=False, refusal="bwd_max"))
    cs.append(Case("refuse_D12", 12, (sp("s12", 9, 12), sp("s4", 9, 4), seq("g16", 9, 16, 3, "mean"), de("x12", 12),
                                      seq("m12", 9, 12, 3, "max")), 19,
                   "fm_embed_dim 12: refused by both record kernels", fwd=False, bwd=False, refusal="D"))
    cs.append(Case("refuse_D20", 20, (sp("s20", 9, 20), sp("s8", 9, 8), seq("g20", 9, 20, 6, "sum"), de("x4", 4)), 19,
                   "fm_embed_dim 20: refused by both record kernels", fwd=False, bwd=False, refusal="D"))
    cs.append(Case("refuse_d6", 16, (sp("s16", 9, 16), sp("s6", 9, 6), de("x6", 6)), 19,
                   "embedding_dim 6 is not a multiple of 4; on the dense-autograd path, a narrow field BEHIND one of width "
                   "fm_dim (the order in which plan creation used to refuse it)", fwd=False, bwd=False, refusal="d%4"))
    cs.append(Case("refuse_lds", 64, tuple(sp(f"s{i}", 9, 32) for i in range(5)), 19,
                   "five 64 x 32 projections: 40960 bytes, over DFM_RECORD_PARAM_LDS_BYTES", fwd=False, bwd=False, refusal="param_lds"))
    return cs


CASES: Dict[str, Case] = {c.name: c for c in _build_cases()}
FWD_CASES = [n for n, c in CASES.items() if c.fwd]
BWD_CASES = [n for n, c in CASES.items() if c.bwd]
DENSE_CASES = list(CASES)            # the dense-autograd path takes every schema
REFUSALS = [n for n, c in CASES.items() if c.refusal]


def model_shim(case: Case):
    """What training/eligibility.py reads of a model: embedding.fm_embed_dim and schema.fields."""
    return types.SimpleNamespace(embedding=types.SimpleNamespace(fm_embed_dim=case.D), schema=H.schema_from_fields(list(case.fields)))


# =====================================================================================================================
# inputs
# =====================================================================================================================
def edge_rows(spec) -> List[int]:
    """Rows of a table on the edges of the backward's row tiles: 1, V - 1, the last row of every tile and the first of
    the next."""
    V, R = spec["vocab"], row_tile(spec["dim"]) if spec["dim"] % 4 == 0 else 0
    rows = {1, V - 1}
    if R:
        rows |= {R // 2, R // 2 + 1}
        for k in range(1, V // R + 2):
            rows |= {k * R - 1, k * R}
    return sorted(r for r in rows if 1 <= r < V)


def _pos(a, b, shape, rng):
    return rng.uniform(a, b, shape).astype(F32)


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """params (state_dict keys of FeatureEmbedding, float32), batch, labels and the upstream gradients of a case, seeded
    from its position in the list.  Every forward operand is positive (tables, row 0 included, and DENSE / projection
    weights in [0.25, 1] (projections / d), x in (0, 1)): every field embedding is positive, so the FM value 0.5 (S^2 -
    sum e^2) keeps |value| / A >= FM_FLOOR and no output has to be left out of a comparison.  The gradients are
    standard normal."""
    case = CASES[name]
    rng = np.random.default_rng([7, list(CASES).index(name)])
    B, D, F, T = case.B, case.D, case.F, case.T
    params, batch = {}, {}
    held = {B // 2, B - 1}
    for spec in case.fields:
        n, d, V, L = spec["name"], spec["dim"], spec["vocab"], spec["max_len"]
        k2, k1, kb2, kb1, kp = H._rec_keys(n)
        if spec["type"] == "dense":
            params[k2], params[kb2] = _pos(0.25, 1, (d, 1), rng), _pos(0.25, 1, (d,), rng)
            params[k1], params[kb1] = _pos(0.25, 1, (1, 1), rng), _pos(0.25, 1, (1,), rng)
            batch[n] = rng.uniform(0.05, 1.0, B).astype(F32)
        else:
            params[k2], params[k1] = _pos(0.25, 1, (V, d), rng), _pos(0.25, 1, (V, 1), rng)
            ids = rng.integers(0, V, (B, L), dtype=np.int64)
            if n == "hot":
                ids[rng.random((B, L)) < 0.85] = 3
            p = 1
            for r in edge_rows(spec):             # ids on the tile edges, past the samples the bag patterns hold
                while p in held:
                    p += 1
                if p >= B:
                    break
                ids[p, 0] = r
                p += 1
            if spec["type"] == "sequence":
                if L >= 3:
                    ids[0] = [max(1, V - 2), 0] + [1] * (L - 2)      # padding in the middle
                ids[B // 2] = min(2, V - 1)                          # one id repeated
                ids[B - 1] = 0                                        # an empty bag
            else:
                ids[B - 1] = 0                                        # id 0
            batch[n] = ids if spec["type"] == "sequence" else np.ascontiguousarray(ids[:, 0])
        if d != D:
            params[kp] = (_pos(0.25, 1, (D, d), rng) / F32(d)).astype(F32)
    g_flat_ld = rng.standard_normal((B, T + LD_PAD_G)).astype(F32)
    return dict(params=params, batch=batch, labels=(rng.random(B) < 0.3).astype(F32),
                g_first=rng.standard_normal(B).astype(F32), g_field=rng.standard_normal((B, F, D)).astype(F32),
                g_flat_ld=g_flat_ld, g_flat=g_flat_ld[:, :T], g_fm=rng.standard_normal(B).astype(F32))


def _fl(case):
    return [dict(f) for f in case.fields]


@functools.lru_cache(maxsize=None)
def forward_ref(name: str) -> dict:
    case, inp = CASES[name], inputs(name)
    return H.record_forward_fp64(_fl(case), inp["params"], inp["batch"], case.D)


def saved_f32(name: str) -> dict:
    """The forward's outputs as float32 arrays: what the backward kernels are handed (and the reference with them)."""
    r = forward_ref(name)
    return {k: r[k].astype(F32) for k in ("field_embeddings", "fm_sum", "flat_embeddings")}


BWD_MODES = ("plain", "fm_field", "fm_only")       # g_field alone | g_field + the FM trio | the trio alone


@functools.lru_cache(maxsize=None)
def backward_ref(name: str, mode: str = "plain") -> dict:
    case, inp = CASES[name], inputs(name)
    return H.record_backward_fp64(_fl(case), inp["params"], inp["batch"], case.D, inp["g_first"],
                                  None if mode == "fm_only" else inp["g_field"], inp["g_flat"],
                                  None if mode == "plain" else inp["g_fm"], saved=saved_f32(name))


# =====================================================================================================================
# what a case reaches
# =====================================================================================================================
def reach(name: str) -> dict:
    case = CASES[name]
    D = case.D
    r = dict(kernels=set(), jobs=set(), proj_chunks=set(), proj_partial=False, tiles=set())
    if case.fwd:
        r["kernels"].add(f"emb_fwd_record<{D}>")
    if case.bwd:
        r["kernels"] |= {f"emb_bwd_record<{D}>", f"emb_bwd_record_fm<{D}>"}
        for f in case.fields:
            r["jobs"].add("dense" if f["type"] == "dense" else "table")
            if f["type"] != "dense":
                r["tiles"].add(-(-f["vocab"] // row_tile(f["dim"])))
            if f["dim"] != D:
                r["jobs"].add("proj")
                n = D * f["dim"]
                r["proj_chunks"].add(-(-n // BWD_THREADS))
                r["proj_partial"] |= n > BWD_THREADS and n % BWD_THREADS != 0
    return r


# =====================================================================================================================
# the float32 restatement and its ratios
# =====================================================================================================================
def f32_ratios(name: str, order: str) -> Dict[str, float]:
    """Worst |float32 restatement - fp64| / (EPS32 sqrt(n) A) per kind of output (c = 1)."""
    case, inp = CASES[name], inputs(name)
    out = dict(forward=0.0, table=0.0, dense=0.0, proj=0.0)
    ref = forward_ref(name)
    got = H.record_forward_fp64(_fl(case), inp["params"], inp["batch"], case.D, dt=F32, order=order)
    for k in ("first_order", "field_embeddings", "flat_embeddings", "fm", "fm_sum"):
        out["forward"] = max(out["forward"], ratio(got[k], ref[k], ref["A"][k], ref["n"][k], 1.0))
    for mode in BWD_MODES:
        want = backward_ref(name, mode)
        g = H.record_backward_fp64(_fl(case), inp["params"], inp["batch"], case.D, inp["g_first"],
                                   None if mode == "fm_only" else inp["g_field"], inp["g_flat"],
                                   None if mode == "plain" else inp["g_fm"], saved=saved_f32(name), dt=F32, order=order)
        for k, v in want["grads"].items():
            kd = kind_of(k, case.fields)
            out[kd] = max(out[kd], ratio(g["grads"][k], v, want["A"][k], want["n"][k], 1.0))
    return out


# =====================================================================================================================
# mutations: mistakes a kernel of this family could make, applied to the fp64 reference's inputs or outputs.  Each
# returns {key: mutated gradient} for the keys the mistake must move outside their bars in the case named with it.
# =====================================================================================================================
def _bwd(case, inp, mode="plain", **over):
    a = dict(params=inp["params"], batch=inp["batch"], g_first=inp["g_first"], g_field=inp["g_field"], g_flat=inp["g_flat"],
             g_fm=inp["g_fm"], saved=saved_f32(case.name))
    a.update(over)
    return H.record_backward_fp64(_fl(case), a["params"], a["batch"], case.D, a["g_first"],
                                  None if mode == "fm_only" else a["g_field"], a["g_flat"],
                                  None if mode == "plain" else a["g_fm"], saved=a["saved"])["grads"]


def _drop_sample(name, b):
    """Every gradient without sample b's contribution; the keys sample b contributes to."""
    case, inp = CASES[name], inputs(name)
    z = {k: inp[k].copy() for k in ("g_first", "g_field", "g_flat")}
    for v in z.values():
        v[b] = 0
    got = _bwd(case, inp, **z)
    keys = []
    for spec in case.fields:
        k2, k1, kb2, kb1, kp = H._rec_keys(spec["name"])
        named = spec["type"] == "dense" or np.any(inp["batch"][spec["name"]][b] != 0)
        if named:
            keys += [k2, k1] + ([kb2, kb1] if spec["type"] == "dense" else [])
        if spec["dim"] != case.D:
            keys.append(kp)
    return {k: got[k] for k in keys}


def mut_drop_last_of_slice(name):
    parts, rpp = bwd_slices(CASES[name].B)
    assert parts > 1
    return _drop_sample(name, rpp - 1)


def mut_drop_second_stage(name):
    parts, rpp = bwd_slices(CASES[name].B)
    assert rpp == BWD_STAGE + 1
    return _drop_sample(name, BWD_STAGE)


def mut_skip_row(name):
    """The last row of the first tile (or row V - 1 of a table of one tile) is never stored."""
    case = CASES[name]
    want = backward_ref(name)["grads"]
    out = {}
    for spec in case.fields:
        if spec["type"] == "dense":
            continue
        k2, k1 = H._rec_keys(spec["name"])[:2]
        row = min(row_tile(spec["dim"]), spec["vocab"]) - 1
        for k in (k2, k1):
            out[k] = want[k].copy()
            out[k][row] = 0
    return out


def mut_mean_counts_padding(name):
    """A mean bag divides by L, padding included."""
    case, inp = CASES[name], inputs(name)
    gf, gl = inp["g_field"].copy(), inp["g_flat"].copy()
    keys, off = [], 0
    for f, spec in enumerate(case.fields):
        d = spec["dim"]
        if spec["type"] == "sequence" and spec["combiner"] == "mean" and spec["max_len"] > 1:
            s = ((inp["batch"][spec["name"]] != 0).sum(axis=1) / spec["max_len"]).astype(F32)
            gf[:, f] *= s[:, None]
            gl[:, off:off + d] *= s[:, None]
            keys.append(H._rec_keys(spec["name"])[0])
        off += d
    got = _bwd(case, inp, g_field=gf, g_flat=gl)
    return {k: got[k] for k in keys}


def mut_repeat_once(name):
    """An id a sum bag holds twice is added once."""
    case, inp = CASES[name], inputs(name)
    batch, keys = dict(inp["batch"]), []
    for spec in case.fields:
        if spec["type"] == "sequence" and spec["combiner"] == "sum" and spec["max_len"] > 1:
            ids = batch[spec["name"]].copy()
            for l in range(1, ids.shape[1]):
                ids[:, l] = np.where((ids[:, :l] == ids[:, l:l + 1]).any(axis=1), 0, ids[:, l])
            batch[spec["name"]] = ids
            keys += list(H._rec_keys(spec["name"])[:2])
    got = _bwd(case, inp, batch=batch)
    return {k: got[k] for k in keys}


def mut_ld_is_T(name):
    """g_flat read with a row stride of T inside a buffer whose stride is T + LD_PAD_G."""
    case, inp = CASES[name], inputs(name)
    wrong = inp["g_flat_ld"].reshape(-1)[:case.B * case.T].reshape(case.B, case.T)
    got = _bwd(case, inp, g_flat=wrong)
    return {k: v for k, v in got.items() if k.startswith("second_order")}


def _transposed(case, inp):
    params, keys = dict(inp["params"]), []
    for spec in case.fields:
        kp = H._rec_keys(spec["name"])[4]
        if kp in params:
            params[kp] = np.ascontiguousarray(params[kp].reshape(spec["dim"], case.D).T)
            keys.append(H._rec_keys(spec["name"])[0])
    return params, keys


def mut_transpose_projection(name):
    """P (fm_dim, d) walked as (d, fm_dim)."""
    case, inp = CASES[name], inputs(name)
    params, keys = _transposed(case, inp)
    got = _bwd(case, inp, params=params)
    return {k: got[k] for k in keys}


def mut_omit_minus_e(name):
    """d e = g_fm * S in place of g_fm * (S - e)."""
    case, inp = CASES[name], inputs(name)
    saved = dict(saved_f32(name))
    saved["field_embeddings"] = np.zeros_like(saved["field_embeddings"])
    got = _bwd(case, inp, mode="fm_field", saved=saved)
    return {k: v for k, v in got.items() if k.startswith("second_order") or k.startswith("projections.")}


def mut_dense_bias_unscaled(name):
    """The two sums of a DENSE field's Linear(1, d) confused: the weight gradient left as the unscaled sum of g (what the
    bias gets), and the bias gradient given the sum scaled by x."""
    case = CASES[name]
    want = backward_ref(name)["grads"]
    out = {}
    for spec in case.fields:
        if spec["type"] == "dense":
            k2, k1, kb2, kb1, _ = H._rec_keys(spec["name"])
            out[k2], out[kb2] = want[kb2].reshape(want[k2].shape), want[k2].reshape(want[kb2].shape)
            out[k1], out[kb1] = want[kb1].reshape(want[k1].shape), want[k1].reshape(want[kb1].shape)
    return out


# (mutation, the case that claims to cover it, the reference mode it is compared with)
MUTATIONS = [
    (mut_drop_last_of_slice, "batch_B257", "plain"), (mut_drop_last_of_slice, "batch_B513", "plain"),
    (mut_drop_last_of_slice, "batch_B4097", "plain"), (mut_drop_last_of_slice, "batch_B4097_D16", "plain"),
    (mut_drop_second_stage, "batch_B4097", "plain"), (mut_drop_second_stage, "batch_B4097_D4", "plain"),
    (mut_drop_second_stage, "batch_B4097_D16", "plain"),
    (mut_skip_row, "vocab_D16", "plain"), (mut_skip_row, "vocab_D4", "plain"),
    (mut_mean_counts_padding, "bags_D16", "plain"), (mut_mean_counts_padding, "widths_D16", "plain"),
    (mut_repeat_once, "bags_D16", "plain"), (mut_repeat_once, "widths_D8", "plain"),
    (mut_ld_is_T, "widths_D16", "plain"), (mut_ld_is_T, "batch_B7", "plain"),
    (mut_transpose_projection, "widths_D16", "plain"), (mut_transpose_projection, "widths_D4", "plain"),
    (mut_transpose_projection, "widths_D32", "plain"),
    (mut_omit_minus_e, "widths_D16", "fm_field"), (mut_omit_minus_e, "batch_B4097_D16", "fm_field"),
    (mut_dense_bias_unscaled, "widths_D16", "plain"), (mut_dense_bias_unscaled, "batch_B4097", "plain"),
]


def forward_mutations(name: str) -> Dict[str, dict]:
    """The two mistakes of the list that the gather can make too: {mutation: forward outputs}."""
    case, inp = CASES[name], inputs(name)
    params, _ = _transposed(case, inp)
    out = {"transpose_projection": H.record_forward_fp64(_fl(case), params, inp["batch"], case.D)}
    ref = forward_ref(name)
    flat, off = ref["flat_embeddings"].copy(), 0
    for spec in case.fields:
        d = spec["dim"]
        if spec["type"] == "sequence" and spec["combiner"] == "mean" and spec["max_len"] > 1:
            s = (inp["batch"][spec["name"]] != 0).sum(axis=1) / spec["max_len"]
            flat[:, off:off + d] *= s[:, None]
        off += d
    out["mean_counts_padding"] = dict(flat_embeddings=flat)
    return out


if __name__ == "__main__":
    worst = dict(forward=0.0, table=0.0, dense=0.0, proj=0.0)
    for nm in CASES:
        for order in ("seq", "pair"):
            r = f32_ratios(nm, order)
            print(nm, order, {k: round(v, 3) for k, v in r.items()})
            worst = {k: max(worst[k], r[k]) for k in worst}
    print("worst", worst)
