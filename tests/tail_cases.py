"""Cases, seeded inputs, bars and fp32 emulations of the step-tail matrix (csrc/step_tail.hip, csrc/tail_bodies.h, the
row-gradient half of csrc/rowplan.hip), shared by tests/test_cpu_tail_reference.py (which proves on the host that
every case reaches the branch it claims and that a correct fp32 implementation stays inside every bar) and
tests/test_gpu_tail_matrix.py (which runs them).  Plain numpy; no GPU and no library needed to import this.

Every bar below is derived from the operation chain, in units of U = 2^-24 (half an ulp: the relative error of one
correctly rounded fp32 operation).  A check returns the worst |error| / bar of an output: <= 1 passes."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from tests import helpers as H

CH = 4096                 # DFM_ROWPLAN_CHUNK
THREADS = 256             # kTailThreads
K_RUN_BATCH = 8           # kRunBatch: contributions in flight per lane group
K_LONG = 64               # kLongRun: longer runs are summed by the whole workgroup (coop widths)
K_SPLIT = 2048            # kSplitRun: longer runs are summed by several workgroups (coop widths)
MAX_SPLIT_RUNS = 2        # kMaxSplitRuns
MAX_SLICES = 64           # kMaxSlices
PREP_PER_BLOCK = 1024     # kTailThreads * kStepPrepPerThread: floats of the dense buffer per prepare workgroup
U = 2.0 ** -24
F32 = np.float32


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def fma32(a, b, c):
    """fmaf in numpy: the float64 product (exact for fp32 operands) plus c, rounded once to fp32."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def ratio(err, bar):
    """Worst |err| / bar over the elements; an element with bar 0 must have err 0."""
    err, bar = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(bar, dtype=np.float64)
    if err.size == 0:
        return 0.0
    if not np.isfinite(err).all():
        return float("inf")
    r = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


# =====================================================================================================================
# a. row gradients: (D, kind).  Two chunks (4096 + an odd tail of 37); field 0's first chunk is the list of the kind.
#   mixed      runs of 300, 65, 64, 9, 8 contributions, singles, three padding ids
#   split2049  one run of 2049 + 2047 distinct ids: num_uniq == CH - kSplitRun exactly, the run is split
#   run2048    one run of 2048 + 2048 distinct ids: not split (summed by one workgroup)
#   run4096    one run of 4096: split, num_uniq == 1
# Bars: a sum that the kernel forms sequentially (runs of <= 64 contributions; every run of a non-coop width) is
# bit-equal to the float32 sum in sample order.  Any other summation order of n fp32 terms has
# |err| <= (n - 1) U sum|g_i| to first order; n U sum|g_i| covers the higher orders for n <= 4096.
# =====================================================================================================================
COOP_D = (4, 8, 16, 32, 64, 128, 256)
NONCOOP_D = (12, 20, 24, 40)
ROWGRAD_KINDS = ("mixed", "split2049", "run2048", "run4096")
MIXED_RUNS = (300, 65, 64, 9, 8)
ROWGRAD_B = CH + 37
ROWGRAD_CASES = [(D, k) for D in COOP_D for k in ROWGRAD_KINDS] + [(D, "mixed") for D in NONCOOP_D]


def is_coop(D: int) -> bool:
    """rowgrad_body: the D/4 lanes of an entry tile the 256-thread workgroup."""
    return THREADS % (D // 4) == 0


def run_class(n: int) -> str:
    return "<=8" if n <= K_RUN_BATCH else "<=64" if n <= K_LONG else "<=2048" if n <= K_SPLIT else ">2048"


@functools.lru_cache(maxsize=None)
def rowgrad_inputs(D, kind):
    """ids (S, B) int64, vocab, field map (F > S, not the identity), g_field (B, F, D), g_first (B,)."""
    rng = _rng(11, D, ROWGRAD_KINDS.index(kind))
    S = 1 if D == 256 else 2
    F = S + 2
    if kind == "mixed":
        head = np.repeat(np.arange(5, 5 + len(MIXED_RUNS)), MIXED_RUNS)
        c0 = np.concatenate([head, np.arange(20, 20 + CH - head.size - 3), np.zeros(3, dtype=np.int64)])
    elif kind == "split2049":
        c0 = np.concatenate([np.full(K_SPLIT + 1, 3), np.arange(10, 10 + CH - K_SPLIT - 1)])
    elif kind == "run2048":
        c0 = np.concatenate([np.full(K_SPLIT, 3), np.arange(10, 10 + CH - K_SPLIT)])
    else:
        c0 = np.full(CH, 3)
    ids = [np.concatenate([rng.permutation(c0), rng.integers(1, 20, ROWGRAD_B - CH)]).astype(np.int64)]
    vocab = [8192]
    if S == 2:
        ids.append(rng.integers(0, 50, ROWGRAD_B).astype(np.int64))
        vocab.append(50)
    return dict(S=S, F=F, B=ROWGRAD_B, ids=np.stack(ids), vocab=tuple(vocab),
                fmap=tuple(F - 1 - 2 * s for s in range(S)),
                g_field=rng.standard_normal((ROWGRAD_B, F, D)).astype(F32),
                g_first=rng.standard_normal(ROWGRAD_B).astype(F32))


def rowgrad_reach(D, kind) -> dict:
    """What the case's lists make rowgrad_body do, from the ids alone."""
    inp = rowgrad_inputs(D, kind)
    classes, split, split_exact, unsplit_2048 = set(), False, False, False
    for c, s in itertools.product(range(2), range(inp["S"])):
        ids = inp["ids"][s, c * CH:(c + 1) * CH]
        rows, count = np.unique(ids[ids != 0], return_counts=True)
        classes |= {run_class(int(n)) for n in count}
        listed = rows.size <= CH - K_SPLIT            # the row plan lists split runs only then
        if is_coop(D) and listed and count.max() > K_SPLIT:
            split = True
            split_exact |= rows.size == CH - K_SPLIT
        unsplit_2048 |= int(count.max()) == K_SPLIT
    return dict(coop=is_coop(D), classes=classes, split=split, split_exact=split_exact, unsplit_2048=unsplit_2048,
                chunks=2, tail=inp["B"] - CH, map_identity=inp["fmap"] == tuple(range(inp["S"])))


def seq_sum_f32(ids, g_rows, g_first, max_len=None):
    """float32 sums in sample order per distinct non-zero id: (g2 (U, D), g1 (U,)); runs longer than max_len: NaN."""
    ids = np.asarray(ids)
    order = np.argsort(ids, kind="stable")
    order = order[ids[order] != 0]
    sid = ids[order]
    starts = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]]) if sid.size else np.zeros(0, dtype=np.int64)
    count = np.diff(np.r_[starts, sid.size])
    g_rows, g_first = _f32(g_rows), _f32(g_first).reshape(-1)
    g2 = np.zeros((starts.size, g_rows.shape[1]), dtype=F32)
    g1 = np.zeros(starts.size, dtype=F32)
    todo = count <= (max_len if max_len is not None else count.max(initial=0))
    for k in range(int(count[todo].max(initial=0))):
        sel = todo & (count > k)
        pos = order[starts[sel] + k]
        g2[sel] = g2[sel] + g_rows[pos]
        g1[sel] = g1[sel] + g_first[pos]
    g2[~todo] = np.nan
    g1[~todo] = np.nan
    return g2, g1


@functools.lru_cache(maxsize=None)
def rowgrad_expect(D, kind):
    """Per list (chunk c, sparse field s): the fp64 reference, the float32 sequential sums where the kernel's sum is
    sequential (`exact`), and the bars elsewhere."""
    inp = rowgrad_inputs(D, kind)
    out = []
    for c, s in itertools.product(range(2), range(inp["S"])):
        sl = slice(c * CH, min((c + 1) * CH, inp["B"]))
        ids, g2, g1 = inp["ids"][s, sl], inp["g_field"][sl, inp["fmap"][s]], inp["g_first"][sl]
        ref = H.tail_rowgrad_fp64(ids, g2, g1)
        exact = (ref["count"] <= K_LONG) | (not is_coop(D))
        seq2, seq1 = seq_sum_f32(ids, g2, g1, K_LONG if is_coop(D) else None)
        out.append(dict(c=c, s=s, exact=exact, seq2=seq2, seq1=seq1, ref=ref,
                        bar2=ref["count"][:, None] * U * ref["abs2"], bar1=ref["count"] * U * ref["abs1"]))
    return out


def rowgrad_check(e, got2, got1) -> float:
    """got2 (num_uniq, D), got1 (num_uniq,) float32 of one list against rowgrad_expect's entry `e`: bit equality
    where the sum is sequential, the bar elsewhere.  Returns the worst error / bar."""
    got2, got1 = _f32(got2), _f32(got1)
    ex = e["exact"]
    assert np.array_equal(got2[ex].view(np.int32), e["seq2"][ex].view(np.int32)), "sequential rows are not bit-equal"
    assert np.array_equal(got1[ex].view(np.int32), e["seq1"][ex].view(np.int32)), "sequential g1 is not bit-equal"
    return max(ratio(got2[~ex] - e["ref"]["g2"][~ex], e["bar2"][~ex]), ratio(got1[~ex] - e["ref"]["g1"][~ex], e["bar1"][~ex]))


def emu_rowgrad(D, kind):
    """A correct fp32 implementation: every run summed one contribution after the other."""
    inp = rowgrad_inputs(D, kind)
    out = []
    for e in rowgrad_expect(D, kind):
        sl = slice(e["c"] * CH, min((e["c"] + 1) * CH, inp["B"]))
        out.append(seq_sum_f32(inp["ids"][e["s"], sl], inp["g_field"][sl, inp["fmap"][e["s"]]], inp["g_first"][sl]))
    return out


# =====================================================================================================================
# b. DENSE-field gradients: (D, B); inside a case num_dense in {1, 3}, alone and beside two sparse fields, in place
# (buffers pre-filled with 1.0) and sliced into dense_parts partial buffers.  B = 100 is the 64-slice case (rows per
# slice = 2, slices 50 .. 63 are empty).
# Bar: every product x g enters through one fmaf, so a slice's sum of n terms is n rounded operations in some order
# (a term passes through its own fmaf and at most n - 1 further additions): n U sum|term|.  In place the 1.0 already
# in the buffer is one more term.
# =====================================================================================================================
DENSE_D = (4, 12, 16)
DENSE_B = (1, 255, 256, 257, 1000)
DENSE_ND = (1, 3)
DENSE_F = 6
DENSE_POS = (4, 0, 2)             # schema positions of the DENSE fields (position 3 is nobody's)
DENSE_SPARSE_POS = (5, 1)
DENSE_FIELD_CASES = [(D, B) for D in DENSE_D for B in DENSE_B] + [(D, 100) for D in DENSE_D]


def dense_modes(B):
    """"inplace" or the number of batch slices."""
    return (64,) if B == 100 else ("inplace", 1, 3)


def dense_grad_layout(D, nd):
    """Offsets (w2, b2, w1, b1) of each DENSE field's gradients inside one buffer, with unused floats between them."""
    per = 2 * D + 8
    return nd * per + 5, [(3 + k * per, 3 + k * per + D, 3 + k * per + 2 * D + 1, 3 + k * per + 2 * D + 3) for k in range(nd)]


@functools.lru_cache(maxsize=None)
def dense_field_inputs(D, B):
    rng = _rng(12, D, B)
    return dict(x=rng.standard_normal((len(DENSE_POS), B)).astype(F32), ids=rng.integers(0, 30, (2, B)).astype(np.int64),
                g_field=rng.standard_normal((B, DENSE_F, D)).astype(F32), g_first=rng.standard_normal(B).astype(F32))


def dense_field_expect(D, B, nd, mode):
    """want / bar (slices, elems) in fp64; NaN in `want` = an address that is no gradient (must keep its bits).
    mode "inplace": one slice, want = 1 + sum."""
    inp = dense_field_inputs(D, B)
    elems, lay = dense_grad_layout(D, nd)
    parts = 1 if mode == "inplace" else mode
    rows = -(-B // parts)
    want, bar = np.full((parts, elems), np.nan), np.zeros((parts, elems))
    for p in range(parts):
        lo, hi = min(p * rows, B), min((p + 1) * rows, B)
        for k in range(nd):
            x = inp["x"][k, lo:hi]
            cols = np.concatenate([inp["g_field"][lo:hi, DENSE_POS[k]], inp["g_first"][lo:hi, None]], axis=1)
            sw, sb, aw, ab = H.tail_dense_field_fp64(x, cols)
            o_w2, o_b2, o_w1, o_b1 = lay[k]
            for off, val, ab_ in ((o_w2, sw[:D], aw[:D]), (o_b2, sb[:D], ab[:D]), (o_w1, sw[D:], aw[D:]), (o_b1, sb[D:], ab[D:])):
                n = hi - lo
                if mode == "inplace":
                    want[p, off:off + val.size], bar[p, off:off + val.size] = 1.0 + val, (n + 1) * U * (1.0 + ab_)
                else:
                    want[p, off:off + val.size], bar[p, off:off + val.size] = val, n * U * ab_
    return want, bar


def emu_dense_field(D, B, nd, mode):
    """fp32: fmaf / additions over the slice's rows one after the other."""
    inp = dense_field_inputs(D, B)
    elems, lay = dense_grad_layout(D, nd)
    parts = 1 if mode == "inplace" else mode
    rows = -(-B // parts)
    out = np.full((parts, elems), np.nan, dtype=F32)
    for p in range(parts):
        lo, hi = min(p * rows, B), min((p + 1) * rows, B)
        for k in range(nd):
            cols = np.concatenate([inp["g_field"][lo:hi, DENSE_POS[k]], inp["g_first"][lo:hi, None]], axis=1)
            sw, sb = np.zeros(D + 1, dtype=F32), np.zeros(D + 1, dtype=F32)
            for b in range(hi - lo):
                sw = fma32(inp["x"][k, lo + b], cols[b], sw)
                sb = sb + cols[b]
            o_w2, o_b2, o_w1, o_b1 = lay[k]
            for off, val in ((o_w2, sw[:D]), (o_b2, sb[:D]), (o_w1, sw[D:]), (o_b1, sb[D:])):
                out[p, off:off + val.size] = (F32(1.0) + val) if mode == "inplace" else val
    return out


def dense_field_check(want, bar, got) -> float:
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    live = ~np.isnan(want)
    assert np.isfinite(got[live]).all(), "a gradient address is not finite"
    return ratio(got[live] - want[live], bar[live])


# =====================================================================================================================
# c. prepare, merge half: (L, S, D, packed, l2, scale_by_L).  Lists per field s (V rows per table):
#   s = 0   rows 0 and V - 1 (first / last row of the table) in list 0, V - 1 also in the last list; row 7 in every
#           list; row 11 in the last list only; row 13 in lists 0 and 2 only, row 17 in lists 1 and 3 only (0-based:
#           an owner with a gap behind it, an owner that is not list 0); the last list is FULL (4096 rows) for L >= 2
#   s = 1   list min(1, L - 1) is EMPTY
#   s = 2   random overlapping lists only
# Bar of an owner's merged gradient (issue: (L + 3) U sum|term|): L - 1 additions, one product with grad_scale,
# one fmaf -> L + 1 roundings of partial results, each bounded by the sum of |term|; terms = |scale g_l|, |2 l2 w|.
# =====================================================================================================================
MERGE_L = (1, 2, 3, 5)
MERGE_D = (4, 12, 16, 256)
PACKED_STRIDE2 = 64


def _merge_cases():
    cases = []
    for i, (D, L) in enumerate(itertools.product((4, 12, 16), MERGE_L)):
        a, b = (3, bool(i % 2), 0.01 if (i // 2) % 2 else 0.0, True), (1, not i % 2, 0.0 if (i // 2) % 2 else 0.01, False)
        cases += [(L, a[0], D, a[1], a[2], a[3]), (L, b[0], D, b[1], b[2], b[3])]
    # D = 256: one field, at most two lists
    cases += [(1, 1, 256, False, 0.01, False), (2, 1, 256, True, 0.0, True), (2, 1, 256, False, 0.01, True)]
    return cases


MERGE_CASES = _merge_cases()


def table_rows(D):
    return 6000


def packed_layout(D):
    """One (V, RS) record buffer [w2 | w1 m1 v1 pad | m2 | v2 | pad]: (RS, offsets of w2, w1, m1, v1, m2, v2).
    RS = 64 floats (stride2 = 64) wherever a record fits, which is D <= 16."""
    rs = PACKED_STRIDE2 if 3 * D + 4 <= PACKED_STRIDE2 else 3 * D + 64
    return rs, dict(w2=0, w1=D, m1=D + 1, v1=D + 2, m2=D + 4, v2=2 * D + 4)


@functools.lru_cache(maxsize=None)
def merge_inputs(case):
    L, S, D, packed, l2, by_l = case
    rng = _rng(13, L, S, D, int(packed), int(l2 > 0), int(by_l))
    V = table_rows(D)
    rows = np.full((L, S, CH), 0x7FFFFFF0, dtype=np.int32)          # behind num: never a valid row
    num = np.zeros((L, S), dtype=np.int32)
    for s, l in itertools.product(range(S), range(L)):
        pick = set(rng.choice(np.arange(20, 1500), size=int(rng.integers(200, 600)), replace=False).tolist())
        if s == 0:
            pick |= {7}
            if l == 0:
                pick |= {0, V - 1}
            if l == L - 1:
                pick |= {11, V - 1}
            if l in (0, 2) and L >= 3:
                pick |= {13}
            if l in (1, 3) and L >= 5:
                pick |= {17}
            if l == L - 1 and L >= 2:
                pick |= set(rng.choice(np.arange(1500, V - 1), size=CH - len(pick), replace=False).tolist())
        if s == 1 and l == min(1, L - 1):
            pick = set()
        r = np.array(sorted(pick), dtype=np.int32)
        rows[l, s, :r.size], num[l, s] = r, r.size
    g2 = rng.standard_normal((L, S, CH, D)).astype(F32)
    g1 = rng.standard_normal((L, S, CH)).astype(F32)
    w2 = [(rng.standard_normal((V, D)) * 0.1).astype(F32) for _ in range(S)]
    w1 = [(rng.standard_normal(V) * 0.1).astype(F32) for _ in range(S)]
    return dict(L=L, S=S, D=D, V=V, packed=packed, l2=F32(l2), grad_scale=F32(1.0 / L) if by_l else F32(1.0),
                rows=rows, num=num, g2=g2, g1=g1, w2=w2, w1=w1)


def merge_reach(case) -> dict:
    """Features of the case's lists, from the lists alone."""
    m = merge_inputs(case)
    L, S, V, rows, num = m["L"], m["S"], m["V"], m["rows"], m["num"]
    held = lambda s, r: tuple(l for l in range(L) if r in rows[l, s, :num[l, s]])        # noqa: E731
    every = [r for r in range(20) if S and held(0, r) == tuple(range(L))]
    return dict(every_list=bool(every), last_only=held(0, 11) == (L - 1,) and L >= 2,
                lists_0_2_only=held(0, 13) == (0, 2), lists_1_3_only=held(0, 17) == (1, 3),
                empty_list=bool((num == 0).any()), full_list=bool((num == CH).any()),
                first_row=0 in held(0, 0), last_row=0 in held(0, V - 1) and L - 1 in held(0, V - 1),
                search=L >= 2, match=L >= 3, sorted=all((np.diff(rows[l, s, :num[l, s]]) > 0).all()
                                                       for l in range(L) for s in range(S)))


@functools.lru_cache(maxsize=None)
def merge_expect(case):
    m = merge_inputs(case)
    ref = H.tail_merge_fp64(m["rows"], m["num"], m["g2"], m["g1"], m["w2"], m["w1"], m["grad_scale"], m["l2"])
    ref["bar2"], ref["bar1"] = (m["L"] + 3) * U * ref["abs2"], (m["L"] + 3) * U * ref["abs1"]
    return ref


def emu_merge(case):
    """fp32: the owner adds the other lists' rows in list order, then fmaf(2 l2, w, scale * g).  Returns (owner, g2, g1)
    with non-owners' rows as they were."""
    m = merge_inputs(case)
    L, S = m["L"], m["S"]
    own = merge_expect(case)["owner"]
    g2, g1 = m["g2"].copy(), m["g1"].copy()
    k = F32(2.0) * m["l2"]
    for s in range(S):
        where = [{int(r): u for u, r in enumerate(m["rows"][l, s, :m["num"][l, s]])} for l in range(L)]
        for l in range(L):
            us = np.flatnonzero(own[l, s] == 1)
            r = m["rows"][l, s, us]
            a2, a1 = m["g2"][l, s, us].copy(), m["g1"][l, s, us].copy()
            for ln in range(l + 1, L):
                hit = np.array([where[ln].get(int(x), -1) for x in r], dtype=np.int64)
                a2[hit >= 0] = a2[hit >= 0] + m["g2"][ln, s, hit[hit >= 0]]
                a1[hit >= 0] = a1[hit >= 0] + m["g1"][ln, s, hit[hit >= 0]]
            g2[l, s, us] = fma32(k, m["w2"][s][r], m["grad_scale"] * a2)
            g1[l, s, us] = fma32(k, m["w1"][s][r], m["grad_scale"] * a1)
    return own, g2, g1


def merge_check(case, owner, g2, g1):
    """owner (L, S, CH) int, g2, g1 float32 after the merge.  Asserts the exact parts (owner flags, non-owners' bits);
    returns the worst error / bar of (g2, g1) over the owners."""
    m, ref = merge_inputs(case), merge_expect(case)
    live = ref["owner"] >= 0
    assert np.array_equal(np.asarray(owner)[live], ref["owner"][live]), "owner_flag"
    own = ref["owner"] == 1
    g2, g1 = _f32(g2).reshape(m["g2"].shape), _f32(g1).reshape(m["g1"].shape)
    assert np.array_equal(g2[~own].view(np.int32), m["g2"][~own].view(np.int32)), "a non-owner's row_g2 changed"
    assert np.array_equal(g1[~own].view(np.int32), m["g1"][~own].view(np.int32)), "a non-owner's row_g1 changed"
    return ratio(g2[own] - ref["g2"][own], ref["bar2"][own]), ratio(g1[own] - ref["g1"][own], ref["bar1"][own])


# =====================================================================================================================
# c. prepare, dense half: dict(n, n_l2, slabs = ((offset, elems, splits), ...), world, pad).  world = 0: no gathered
# buffer; pad: gathered_stride - n.  Slabs need n % 4 == 0 to end on the last float4; gathered buffers need n % 4 == 0.
# Bar of g: every term joins by one addition (the L2 term by fmaf, the rank mean by one product more):
# (terms + 1) U sum|term| (tail_dense_prepare_fp64 counts the terms).
# |g|^2 of n elements: n products and n additions of non-negative numbers in any order: relative error n U to first
# order; the bar is taken against the fp64 sum of squares of the gradient the kernel itself wrote.
# =====================================================================================================================
DENSE_N = (4, 1023, 1024, 1025, 1027, 4112)
SLAB_SPLITS = (1, 7, 8, 9, 17)


def _dense_prepare_cases():
    cases = []
    for n in DENSE_N:
        for n_l2 in sorted({0, 16 if n >= 16 else 0, n // 16 * 16}):
            cases.append(dict(n=n, n_l2=n_l2, slabs=(), world=0, pad=0))
    for i, sp in enumerate(SLAB_SPLITS):                       # one slab at offset 0; odd n: beside the scalar tail
        n = (1024, 1027, 4112, 1025, 1023)[i]
        cases.append(dict(n=n, n_l2=(0, 16, n // 16 * 16)[i % 3], slabs=((0, 64, sp),), world=0, pad=0))
    for i, (sa, sb) in enumerate(((7, 8), (9, 1), (17, 7), (8, 17), (1, 9))):      # two: offset 0, and up to the last float4
        n = (1024, 4112)[i % 2]
        cases.append(dict(n=n, n_l2=(n // 16 * 16, 0, 16)[i % 3], slabs=((0, 32, sa), (n - 48, 48, sb)), world=0, pad=0))
    for world, pad, n in itertools.product((1, 2, 3), (0, 4), (4, 1024, 4112)):
        if (world + pad // 4 + n) % 2 == 0 or n == 4:
            cases.append(dict(n=n, n_l2=0, slabs=(), world=world, pad=pad))                 # alone
    for i, (world, pad) in enumerate(itertools.product((1, 2, 3), (0, 4))):                 # with slabs and L2
        n = (4112, 1024)[i % 2]
        cases.append(dict(n=n, n_l2=(16, n // 16 * 16)[i % 2], slabs=((0, 32, SLAB_SPLITS[i % 5]), (n - 48, 48, 8)),
                          world=world, pad=pad))
    return cases


DENSE_PREPARE_CASES = _dense_prepare_cases()


def dense_case_id(c):
    return "n{n}-l2_{n_l2}-slabs{k}-w{world}p{pad}".format(k="_".join(str(s[2]) for s in c["slabs"]) or "0", **c)


def dense_prepare_reach(c) -> dict:
    n = c["n"]
    full = n // 4                                    # float4s that take the vector branch
    return dict(vector=full > 0, scalar_tail=n % 4 != 0, blocks=-(-n // PREP_PER_BLOCK),
                unrolled=any(s[2] >= 8 for s in c["slabs"]), unrolled_exact=any(s[2] == 8 for s in c["slabs"]),
                remainder=any(s[2] % 8 for s in c["slabs"]), remainder_only=any(s[2] < 8 for s in c["slabs"]),
                slab_at_0=any(s[0] == 0 for s in c["slabs"]), slab_at_end=any(s[0] + s[1] == n for s in c["slabs"]),
                gathered=c["world"] > 0, l2_all=c["n_l2"] == n // 16 * 16 and c["n_l2"] > 0)


def _dense_key(c):
    return (c["n"], c["n_l2"], c["slabs"], c["world"], c["pad"])


@functools.lru_cache(maxsize=None)
def _dense_prepare_inputs(key):
    n, n_l2, slabs, world, pad = key
    rng = _rng(14, n, n_l2, world, pad, *[v for s in slabs for v in s])
    d = dict(g=rng.standard_normal(n).astype(F32), p=(rng.standard_normal(n) * 0.1).astype(F32), l2=F32(0.01),
             slabs=[(off, rng.standard_normal((sp, el)).astype(F32)) for off, el, sp in slabs], gathered=None,
             scale=F32(1.0))
    if world:
        ga = np.full((world, n + pad), np.nan, dtype=F32)                # NaN in the gap between two ranks
        ga[:, :n] = rng.standard_normal((world, n))
        d.update(gathered=ga, scale=F32(1.0 / world))
    return d


def dense_prepare_inputs(c):
    return _dense_prepare_inputs(_dense_key(c))


def dense_prepare_expect(c, l2=None, scale=None):
    """(g, bar); l2 / scale: the launch's own values where it shares them with a merge half (default: the inputs')."""
    d = dense_prepare_inputs(c)
    ga = None if d["gathered"] is None else d["gathered"][:, :c["n"]]
    g, absum, terms = H.tail_dense_prepare_fp64(d["g"], d["p"], c["n_l2"], d["l2"] if l2 is None else F32(l2), d["slabs"],
                                                ga, d["scale"] if scale is None else F32(scale))
    return g, (terms + 1) * U * absum


def emu_dense_prepare(c, l2=None, scale=None):
    d = dict(dense_prepare_inputs(c))
    if l2 is not None:
        d["l2"] = F32(l2)
    if scale is not None:
        d["scale"] = F32(scale)
    n = c["n"]
    g = d["g"].copy()
    if d["gathered"] is not None:
        g = np.zeros(n, dtype=F32)
        for r in range(c["world"]):
            g = g + d["gathered"][r, :n]
        g = g * d["scale"]
    for off, sl in d["slabs"]:
        for q in range(sl.shape[0]):
            g[off:off + sl.shape[1]] = g[off:off + sl.shape[1]] + sl[q]
    g[:c["n_l2"]] = fma32(F32(2.0) * d["l2"], d["p"][:c["n_l2"]], g[:c["n_l2"]])
    return g


def sq_bar(values) -> float:
    """Bar of an fp32 sum of squares against the fp64 one: n U relative."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    return max(v.size, 1) * U * float((v ** 2).sum())


def emu_sq(values) -> float:
    """fp32: squares added one after the other."""
    v = _f32(values).reshape(-1)
    v = v[~np.isnan(v)]
    return float(np.cumsum(v * v, dtype=F32)[-1]) if v.size else 0.0


# =====================================================================================================================
# d. dfm_grad_norm_finalize: n partials.
# total: n - 1 additions of non-negative numbers in any order: n U relative.
# clip = min(1, max_norm / (sqrt(total) + 1e-6)): the square root halves total's error and rounds once, the
# addition and the division round once each: (n / 2 + 3) U relative (+ 1 U of slack for the second order).
# =====================================================================================================================
FINALIZE_N = (0, 1, 1023, 1024, 1025, 5000)


def finalize_inputs(n):
    return (_rng(15, n).uniform(0.0, 2.0, n) ** 2).astype(F32)


def finalize_expect(n, max_norm):
    """(total, its bar, clip, its bar) for the fp32 max_norm the kernel receives."""
    total = float(finalize_inputs(n).astype(np.float64).sum())
    clip = H.tail_clip_fp64(total, F32(max_norm))
    return total, n * U * total, clip, (0.0 if clip == 1.0 else (n / 2 + 4) * U * clip)


def finalize_max_norms(n):
    """0 (no clipping), above the norm (clip == 1 exactly), below it."""
    norm = float(np.sqrt(finalize_inputs(n).astype(np.float64).sum()))
    return (0.0, 2.0 * norm + 1.0, 0.37 * norm if n else 0.5)


def emu_finalize(n, max_norm):
    p = finalize_inputs(n)
    tot = np.cumsum(p, dtype=F32)[-1] if n else F32(0)
    c = F32(1.0)
    if F32(max_norm) > 0:
        c = min(F32(1.0), F32(max_norm) / (np.sqrt(tot, dtype=F32) + F32(1e-6)))
    return float(tot), float(c)


# =====================================================================================================================
# e. apply.  One launch = one optimizer step at step count t on given state (m, v random: any history).
#
# Hyper-parameters are float32 (the kernel's arguments); 1 - b1 and 1 - b2 are exact in fp32 (Sterbenz, b >= 0.5).
# gc = g * clip rounds once when a clip coefficient is given; without one gc = g * 1.f is exact.  Roundings per chain
# (ROUNDINGS[output] = (without, with a clip coefficient)):
#   m' = fmaf(b1, m, (1 - b1) gc)            [gc,] the product, the fmaf                  -> 2 | 3 U (|b1 m| + |(1 - b1) gc|)
#   v' = fmaf(b2, v, (1 - b2) gc gc)         [gc, which enters squared: 2,] two products, the fmaf -> 3 | 5 U v'   (all terms >= 0)
#   SGD buf' = fmaf(momentum, buf, gc)       [gc,] the fmaf                               -> 1 | 2 U (|momentum buf| + |gc|)
# The Adam update  upd = step_size * (m' / denom):
#   step_size = lr / (1 - powf(b1, t)).  powf is accurate to 1 ulp (HIP math API) = at most 2 U relative = POW_ULP U;
#       an error of c U in b^t appears as c U b^t / (1 - b^t) in 1 - b^t: about 3e-5 per U-unit at t = 2 for
#       b2 = 0.999.  Then the subtraction and the division round: eps_ss = POW_ULP U r1 + 2 U,  r = b^t / (1 - b^t).
#   inv = 1 / sqrtf(1 - powf(b2, t)): the square root halves what it receives:  eps_inv = (POW_ULP U r2 + U) / 2 + 2 U.
#   denom = sqrtf(v') * inv + eps: v' carries its 3 | 5 U, halved; sqrtf, the product and the addition round (the eps term
#       only dilutes the relative error):  eps_denom = (1.5 | 2.5) U + eps_inv + 3 U.
#   the quotient and the product with step_size round:  + 2 U.
#   m' enters with its absolute error: (step_size / denom) * bar(m').
# w' = decay w - upd: the subtraction rounds once (U |w'|); AdamW also rounds decay = 1 - lr wd (U) and decay * w (U).
# The test holds  w' - decay w  (decay in fp64 from the fp32 lr and wd) to
#       |upd| eps_total + (step_size / denom) bar(m') + W_ULPS[rule] ulp(w),   ulp(w) = 2 U max(|w|, |w'|):
# one ulp of w for Adam and SGD; two for AdamW, whose two extra roundings are of the size of w.
# SGD: w' = fmaf(-lr, buf', w): lr bar(buf') + one ulp of w.
# =====================================================================================================================
POW_ULP = 2.0
W_ULPS = {"adam": 1.0, "adamw": 2.0, "sgd": 1.0}
ROUNDINGS = {"m": (2.0, 3.0), "v": (3.0, 5.0), "sgd": (1.0, 2.0)}         # (clip NULL, clip given)
RULES = ("adam", "adamw", "sgd")
RULE_KIND = {"adam": 0, "adamw": 1, "sgd": 2}       # DFM_OPT_*
APPLY_T = (1, 2, 10, 1000, 100000)
APPLY_D = (4, 12, 16, 256)
APPLY_N = (1, 255, 256, 257, 1025)
APPLY_CLIP = 0.37
HYPER = dict(b1=F32(0.9), b2=F32(0.999), eps=F32(1e-8), wd=F32(0.01), momentum=F32(0.9))
LR, LR2 = F32(1e-3), F32(3e-3)


APPLY_ENTRIES = ("dfm_step_apply", "dfm_step_dense_apply", "dfm_step_apply_plan")      # the first sets the bits


def _apply_cases():
    """dict(rule, t, D, n, clip, zero_grad, packed, batch, wide, entries): test_apply launches the entries listed."""
    cases = []
    for i, (rule, t) in enumerate(itertools.product(RULES, APPLY_T)):
        cases.append(dict(rule=rule, t=t, D=(4, 12, 16)[i % 3], n=APPLY_N[(i + i // 5) % 5], clip=bool(i % 2),
                          zero_grad=(i // 2) % 2, packed=bool((i // 3) % 2), batch=(1000, 4133)[i % 2], wide=False))
    for i, rule in enumerate(RULES):
        cases.append(dict(rule=rule, t=10, D=256, n=APPLY_N[i + 1], clip=bool(i % 2), zero_grad=(i + 1) % 2,
                          packed=i == 1, batch=1000, wide=False))
        cases.append(dict(rule=rule, t=2, D=4, n=APPLY_N[(i + 3) % 5], clip=not i % 2, zero_grad=i % 2, packed=False,
                          batch=(4133, 1000, 4133)[i], wide=True))
    return [dict(c, entries=APPLY_ENTRIES) for c in cases]


APPLY_CASES = _apply_cases()
NARROW_VOCAB, WIDE_VOCAB = 1000, (1 << 20) - 1


def apply_case_id(c):
    return "{rule}-t{t}-D{D}-n{n}-clip{clip:d}-zg{zero_grad}-{lay}-{key}{batch}".format(
        lay="packed" if c["packed"] else "separate", key="wide" if c["wide"] else "narrow", **c)


def apply_shape(c):
    """(S, L, V): sparse fields, lists, rows per table.  The plan half of dfm_step_apply_plan touches row id of every
    next id below the field's vocabulary, so the tables have max_vocab rows."""
    if c["wide"]:
        return 1, 2, WIDE_VOCAB
    return (1 if c["D"] == 256 else 2), 2, NARROW_VOCAB


def apply_key_is_narrow(c) -> bool:
    return (WIDE_VOCAB if c["wide"] else NARROW_VOCAB) < (1 << 20) - 1


def _apply_key(c):
    return tuple(sorted(c.items()))


@functools.lru_cache(maxsize=None)
def _apply_inputs(key):
    c = dict(key)
    S, L, V = apply_shape(c)
    D, n = c["D"], c["n"]
    rng = _rng(16, RULES.index(c["rule"]), c["t"], D, n, int(c["wide"]))
    rows = np.zeros((L, S, CH), dtype=np.int32)
    num = np.zeros((L, S), dtype=np.int32)
    flag = np.zeros((L, S, CH), dtype=np.int32)
    for s in range(S):
        pick = rng.choice(np.arange(1, V - 1), size=600, replace=False)
        pick[:2] = (0, V - 1)
        at = 0
        for l in range(L):
            k = 250 + 50 * l
            r = np.sort(pick[at:at + k])
            at += k
            rows[l, s, :k], num[l, s] = r, k
            flag[l, s, :k] = rng.uniform(size=k) < 0.7          # the rest: rows another list owns
            rows[l, s, k:] = r[rng.integers(0, k, CH - k)]      # behind num_uniq: valid rows, flagged as owned
            flag[l, s, k:] = 1
        flag[0, s, :5] = (1, 0, 1, 0, 1)
    g2 = rng.standard_normal((L, S, CH, D)).astype(F32)
    g1 = rng.standard_normal((L, S, CH)).astype(F32)
    g2[0, :, 2], g1[0, :, 2] = 0.0, 0.0                         # an owned row with g = m = v = 0
    g2[0, :, 4], g1[0, :, 4] = 0.0, 0.0                         # ... and one with g = v = 0, m = 1e-6: denom == eps
    tabs = []
    for s in range(S):
        t = dict(w2=(rng.standard_normal((V, D)) * 0.1).astype(F32), m2=(rng.standard_normal((V, D)) * 0.1).astype(F32),
                 v2=(rng.standard_normal((V, D)) ** 2 * 0.01).astype(F32), w1=(rng.standard_normal(V) * 0.1).astype(F32),
                 m1=(rng.standard_normal(V) * 0.1).astype(F32), v1=(rng.standard_normal(V) ** 2 * 0.01).astype(F32))
        z = rows[0, s, 2]
        t["m2"][z], t["v2"][z], t["m1"][z], t["v1"][z] = 0.0, 0.0, 0.0, 0.0
        z = rows[0, s, 4]
        t["m2"][z], t["v2"][z], t["m1"][z], t["v1"][z] = 1e-6, 0.0, -1e-6, 0.0
        tabs.append(t)
    dense = dict(p=(rng.standard_normal(n) * 0.1).astype(F32), m=(rng.standard_normal(n) * 0.1).astype(F32),
                 v=(rng.standard_normal(n) ** 2 * 0.01).astype(F32), g=rng.standard_normal(n).astype(F32))
    dense["g"][n - 1] = dense["m"][n - 1] = dense["v"][n - 1] = 0.0
    if n >= 3:                                                  # g = v = 0, m = 1e-6: the denominator is eps alone
        dense["g"][n - 2], dense["m"][n - 2], dense["v"][n - 2] = 0.0, 1e-6, 0.0
    vocab = (V,) + ((50,) if S == 2 else ())
    B, stride = c["batch"], c["batch"] + 24
    nxt = np.zeros((S, stride), dtype=np.int64)
    for s in range(S):
        nxt[s, :B] = rng.integers(0, vocab[s], B)
        nxt[s, :4] = (vocab[s] - 1, 0, 1, vocab[s] - 1)
    return dict(S=S, L=L, V=V, rows=rows, num=num, flag=flag, g2=g2, g1=g1, tables=tabs, dense=dense, vocab=vocab,
                next_ids=nxt, ids_stride=stride)


def apply_inputs(c):
    return _apply_inputs(_apply_key(c))


def apply_owned(c):
    """Per field: (rows, list, entry) of the entries the launch must update, rows distinct."""
    a = apply_inputs(c)
    out = []
    for s in range(a["S"]):
        ls, us = np.nonzero((np.arange(CH)[None, :] < a["num"][:, s, None]) & (a["flag"][:, s] != 0))
        r = a["rows"][ls, s, us]
        assert np.unique(r).size == r.size
        out.append((r.astype(np.int64), ls, us))
    return out


def pow_ratio(b, t):
    bt = float(b) ** float(t)
    return bt / (1.0 - bt)


def adam_update_eps(t, clip: bool) -> float:
    """eps_total of the derivation above, in absolute terms (not U units)."""
    r1, r2 = pow_ratio(HYPER["b1"], t), pow_ratio(HYPER["b2"], t)
    eps_ss = POW_ULP * U * r1 + 2 * U
    eps_inv = (POW_ULP * U * r2 + U) / 2 + 2 * U
    eps_denom = ROUNDINGS["v"][bool(clip)] / 2 * U + eps_inv + 3 * U
    return eps_ss + eps_denom + 2 * U


def rule_expect(rule, w, m, v, g, t, lr, clip):
    """fp64 (w', m', v') of one step and the bars of (w' - decay w, m', v'); clip: None or the fp32 coefficient."""
    cl = 1.0 if clip is None else float(F32(clip))
    w64, m64, g64 = (np.asarray(a, dtype=np.float64) for a in (w, m, g))
    wn, mn, vn = H.tail_rule_fp64(rule, w, m, v, g, t, lr, HYPER, cl)
    lr64 = float(F32(lr))
    decay = 1.0 - lr64 * float(HYPER["wd"]) if rule == "adamw" else 1.0
    ulp_w = W_ULPS[rule] * 2 * U * np.maximum(np.abs(w64), np.abs(wn))
    if rule == "sgd":
        bar_m = ROUNDINGS["sgd"][clip is not None] * U * (np.abs(float(HYPER["momentum"]) * m64) + np.abs(g64 * cl))
        return (wn, mn, None), decay, (lr64 * bar_m + ulp_w, bar_m, None)
    b1, b2 = float(HYPER["b1"]), float(HYPER["b2"])
    bar_m = ROUNDINGS["m"][clip is not None] * U * (np.abs(b1 * m64) + np.abs((1 - b1) * g64 * cl))
    bar_v = ROUNDINGS["v"][clip is not None] * U * vn
    gain = (lr64 / (1.0 - b1 ** float(t))) / (np.sqrt(vn) / np.sqrt(1.0 - b2 ** float(t)) + float(HYPER["eps"]))
    upd = np.abs(wn - decay * w64)
    return (wn, mn, vn), decay, (upd * adam_update_eps(t, clip is not None) + gain * bar_m + ulp_w, bar_m, bar_v)


def rule_check(rule, w, m, v, g, t, lr, clip, got_w, got_m, got_v) -> dict:
    """Worst error / bar of the update (w' - decay w), m' and v' (Adam family)."""
    (wn, mn, vn), decay, (bar_w, bar_m, bar_v) = rule_expect(rule, w, m, v, g, t, lr, clip)
    w64 = np.asarray(w, dtype=np.float64)
    r = dict(update=ratio((np.asarray(got_w, dtype=np.float64) - decay * w64) - (wn - decay * w64), bar_w),
             m=ratio(np.asarray(got_m, dtype=np.float64) - mn, bar_m))
    if rule != "sgd":
        r["v"] = ratio(np.asarray(got_v, dtype=np.float64) - vn, bar_v)
    return r


def emu_rule(rule, w, m, v, g, t, lr, clip):
    """The rule in numpy float32, operation by operation as csrc/tail_bodies.h::rule1 writes it."""
    w, m, g, lr = _f32(w), _f32(m), _f32(g), F32(lr)
    g = g * F32(1.0 if clip is None else clip)
    h = HYPER
    if rule == "sgd":
        m = fma32(h["momentum"], m, g)
        return fma32(-lr, m, w), m, None
    v = _f32(v)
    if rule == "adamw":
        w = w * (F32(1.0) - lr * h["wd"])
    m = fma32(h["b1"], m, (F32(1.0) - h["b1"]) * g)
    v = fma32(h["b2"], v, (F32(1.0) - h["b2"]) * g * g)
    pw = lambda b: F32(float(b) ** float(t))          # noqa: E731   (powf, correctly rounded)
    step_size = lr / (F32(1.0) - pw(h["b1"]))
    inv = F32(1.0) / np.sqrt(F32(1.0) - pw(h["b2"]), dtype=F32)
    denom = np.sqrt(v, dtype=F32) * inv + h["eps"]
    return w - step_size * (m / denom), m, v
