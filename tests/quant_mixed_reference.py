"""numpy float32 restatement of the quantised record gather (``dfm_embedding_forward_record_quant``,
include/deepfm_hip.h), written from its specification and sharing no code with the package, and the cases that
tests/test_cpu_quant_mixed.py and tests/test_gpu_quant_mixed.py run it on.  Plain numpy; importing this needs neither a
GPU nor the library.

The restatement: a quantised field's records are dequantised through tests/quant_reference.py or
tests/quant4_reference.py (x' = fl(fl(q * scale) + lo), w1 copied).  A SPARSE field is row ``id`` of that.  A SEQUENCE
field is pooled over l = 0 .. L-1 in float32, one addition (or comparison) per non-padding id: id 0 is skipped wherever
it stands, an id outside [0, V) counts as id 0, ``mean`` divides by the count of non-padding ids (one float32 divide),
``max`` works per column and on the first-order weight, an all-padding bag gives zeros.  That is, for every quantised
field, its columns of flat_embeddings, its first-order value and, without a projection, its columns of
field_embeddings."""
from __future__ import annotations

import functools
from typing import Dict, List

import numpy as np

from tests import helpers as H
from tests import quant4_reference, quant_reference
from tests import record_cases as R

F32 = np.float32
REFS = {"int8": quant_reference, "uint4": quant4_reference}
QUANT_DIMS = (16, 32, 64)


def quantised(spec) -> bool:
    """Whether a field of a case is served from records: SPARSE or SEQUENCE of width 16, 32 or 64."""
    return spec["type"] != "dense" and spec["dim"] in QUANT_DIMS


def pool(w2, w1, ids, combiner):
    """(pooled rows (B, d), pooled first-order weights (B,)) of bags ids (B, L) over the float32 table (w2 (V, d),
    w1 (V,)), sequentially in float32."""
    B, L = ids.shape
    V, d = w2.shape
    ids = np.where((ids < 0) | (ids >= V), 0, ids)
    acc, fo = np.zeros((B, d), F32), np.zeros(B, F32)
    count = np.zeros(B, np.int64)
    for l in range(L):
        on = ids[:, l] != 0
        rows, w = w2[ids[:, l]], w1[ids[:, l]]
        if combiner == "max":
            first = count == 0
            new_a = np.where(first[:, None], rows, np.maximum(acc, rows))
            new_w = np.where(first, w, np.maximum(fo, w))
        else:
            new_a, new_w = (acc + rows).astype(F32), (fo + w).astype(F32)
        acc = np.where(on[:, None], new_a, acc).astype(F32)
        fo = np.where(on, new_w, fo).astype(F32)
        count += on
    if combiner == "mean":
        c = np.maximum(count, 1).astype(F32)
        some = count > 0
        acc = np.where(some[:, None], (acc / c[:, None]).astype(F32), acc)
        fo = np.where(some, (fo / c).astype(F32), fo)
    return acc, fo


def field(fmt: str, records, spec, x):
    """(flat columns (B, d), first-order value (B,)) of one quantised field from its host records (V, row bytes)."""
    w2, w1 = REFS[fmt].dequantize_table(np.asarray(records))
    w2, w1 = w2.astype(F32), w1.reshape(-1).astype(F32)
    if spec["type"] == "sparse":
        ids = np.where((x < 0) | (x >= spec["vocab"]), 0, x)
        return w2[ids], w1[ids]
    return pool(w2, w1, x, spec["combiner"])


def dequantised_params(fmt: str, fields, params, records) -> Dict[str, np.ndarray]:
    """``params`` with the tables of the quantised fields replaced by what their records dequantise to."""
    out = dict(params)
    for spec in fields:
        if spec["name"] in records:
            k2, k1 = H._rec_keys(spec["name"])[:2]
            w2, w1 = REFS[fmt].dequantize_table(np.asarray(records[spec["name"]]))
            out[k2], out[k1] = w2.astype(F32), w1.reshape(-1, 1).astype(F32)
    return out


def host_records(fmt: str, fields, params) -> Dict[str, np.ndarray]:
    """The restatement's records of every quantised field, each at its own width."""
    out = {}
    for spec in fields:
        if quantised(spec):
            k2, k1 = H._rec_keys(spec["name"])[:2]
            out[spec["name"]] = REFS[fmt].quantize_table(params[k2], params[k1])
    return out


# =====================================================================================================================
# cases
# =====================================================================================================================
sp, seq, de = R.sp, R.seq, R.de

# every forward case of the record matrix that has something to quantise
MATRIX = [n for n in R.FWD_CASES if any(quantised(f) for f in R.CASES[n].fields)]


def _bags(D):
    """L in 1, 2, 5, 50 under every combiner at d == D, beside a SPARSE field, narrow fp32 fields and a DENSE one."""
    fs = [seq(f"b{L}{c[:2]}", 40, D, L, c) for L in (1, 2, 5, 50) for c in ("mean", "sum", "max")]
    return tuple(fs + [sp("s", 9, D), sp("n4", 7, 4), sp("n8", 8, 8), de("x", D)])


_EDGE = (sp("u", 30, 16), seq("h", 25, 16, 5, "mean"), sp("n4", 7, 4), sp("n8", 8, 8), de("x", 16),
         seq("m", 12, 16, 2, "max"))                      # F = 6 at D = 16: SB = 512 // 24 = 21
_SB = R.fwd_sb(len(_EDGE), 16)

EXTRA: List[R.Case] = [
    R.Case("q_bags_D16", 16, _bags(16), 23, "L in 1, 2, 5, 50 x mean, sum, max at d == D = 16; narrow fp32 fields of "
           "widths 4 and 8 and a DENSE field in the same launch", bwd=False),
    R.Case("q_bags_D32", 32, (seq("h", 33, 32, 5, "mean"), seq("m", 21, 32, 50, "max"), sp("s", 19, 32), de("x", 32),
                              sp("n8", 8, 8)), 11, "d == D = 32: two payload dwords per uint4 lane pair", bwd=False),
    R.Case("q_bags_D64", 64, (seq("h", 33, 64, 5, "sum"), seq("m", 21, 64, 2, "max"), sp("s", 19, 64), de("x", 64),
                              sp("n4", 6, 4)), 11, "d == D = 64", bwd=False),
    R.Case("q_proj_D16", 16, (sp("s32", 23, 32), seq("g32", 17, 32, 5, "mean"), sp("s64", 19, 64),
                              seq("g64", 15, 64, 50, "sum"), seq("m64", 15, 64, 2, "max"), sp("s16", 9, 16),
                              sp("n4", 7, 4), sp("n8", 8, 8), de("x", 16), de("y", 8)), 13,
           "projections 32 into 16 and 64 into 16, SPARSE and bags", bwd=False),
    R.Case("q_proj_D32", 32, (sp("s16", 23, 16), seq("g16", 17, 16, 5, "mean"), seq("m16", 17, 16, 50, "max"),
                              sp("s32", 9, 32), sp("n4", 7, 4), de("x", 32)), 13,
           "projection 16 into 32: the uint4 record of one aligned 16 bytes, every lane walking all its pieces",
           bwd=False),
    R.Case("q_proj_D8", 8, (sp("s16", 23, 16), seq("g32", 17, 32, 5, "sum"), sp("n8", 8, 8), de("x", 8)), 9,
           "fm_embed_dim 8: quantised fields are wider than D", bwd=False),
] + [R.Case(f"q_edge_B{B}", 16, _EDGE, B, f"SB = {_SB}, B = {B}", bwd=False)
     for B in (1, _SB - 1, _SB, _SB + 1, 2 * _SB + 1)]
EXTRA_CASES: Dict[str, R.Case] = {c.name: c for c in EXTRA}
ALL_CASES = MATRIX + list(EXTRA_CASES)


def case_of(name: str) -> R.Case:
    return EXTRA_CASES[name] if name in EXTRA_CASES else R.CASES[name]


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """params (state_dict keys of FeatureEmbedding, float32), batch and labels of a case; the record matrix's own for
    its cases.  An extra case: tables, DENSE and projection weights in (-1, 1) (projections / d), x in (0, 1), ids
    uniform with, in every bag field and as far as B goes, sample 0: padding in the middle, 1: all padding, 2: one id,
    3: full, 4: one id repeated, 5: padding in front."""
    if name in R.CASES:
        return R.inputs(name)
    case = EXTRA_CASES[name]
    rng = np.random.default_rng([11, list(EXTRA_CASES).index(name)])
    B, D = case.B, case.D
    params, batch = {}, {}
    u = lambda shape: rng.uniform(-1.0, 1.0, shape).astype(F32)
    for spec in case.fields:
        n, d, V, L = spec["name"], spec["dim"], spec["vocab"], spec["max_len"]
        k2, k1, kb2, kb1, kp = H._rec_keys(n)
        if spec["type"] == "dense":
            params[k2], params[kb2], params[k1], params[kb1] = u((d, 1)), u((d,)), u((1, 1)), u((1,))
            batch[n] = rng.uniform(0.05, 1.0, B).astype(F32)
        else:
            params[k2], params[k1] = u((V, d)), u((V, 1))
            ids = rng.integers(0, V, (B, L), dtype=np.int64)
            if spec["type"] == "sequence":
                pat = [np.r_[V - 1, 0, np.full(L - 2, 1)] if L >= 3 else np.r_[np.zeros(L - 1), V - 1],
                       np.zeros(L), np.r_[2, np.zeros(L - 1)], rng.integers(1, V, L), np.full(L, 3),
                       np.r_[np.zeros(L - 1), 4]]
                for b, row in enumerate(pat[:B]):
                    ids[b] = row
                batch[n] = ids
            else:
                ids[B - 1] = 0
                batch[n] = np.ascontiguousarray(ids[:, 0])
        if d != D:
            params[kp] = (u((D, d)) / F32(d)).astype(F32)
    return dict(params=params, batch=batch, labels=(rng.random(B) < 0.3).astype(F32))


def fields_of(name: str) -> List[dict]:
    return [dict(f) for f in case_of(name).fields]
