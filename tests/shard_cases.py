"""Cases, seeded inputs, host restatements of the layouts, fp32 emulations and bars of the field-sharded exchange
matrix (csrc/shard.hip: dfm_shard_gather, dfm_shard_pack, dfm_shard_rowgrad, dfm_sum_floats, dfm_stage_record), shared
by tests/test_cpu_shard_reference.py (which proves on the host that every case reaches the branch it claims, that every
planted mistake is caught and that a correct fp32 implementation passes every check) and tests/test_gpu_shard_matrix.py
(which runs them).  Plain numpy; no GPU and no library needed to import this.

Two statements of every layout live here.  An `*_expect` function restates the documented layout
(include/deepfm_hip.h, "Field-sharded embedding tables") with array operations on the logical tables and gradients.
An `emu_*` function walks the buffers as they lie in memory with the address arithmetic of one item at a time, in
float32 where something is added, and accepts a planted `mistake`; with mistake=None it must satisfy every check.

Bars.  Copies are compared bit for bit.  A sum whose order is fixed is bit-equal to its float32 emulation.  Any
summation of n float32 terms is within n U sum|term| of the float64 sum (tests/tail_cases.py derives it), U = 2^-24."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from tests import helpers as H
from tests.tail_cases import (CH, F32, K_LONG, K_RUN_BATCH, K_SPLIT, MAX_SLICES, MAX_SPLIT_RUNS, THREADS, U, is_coop, ratio,
                              run_class, seq_sum_f32)

MAX_RANKS = 64            # DFM_MAX_RANKS
MAX_FIELDS = 64           # DFM_MAX_FIELDS
MAX_SLABS = 16            # kMaxSlabs
NEG_ZERO = F32(-0.0)
DENORMAL = np.array([0x00000123], dtype=np.uint32).view(F32)[0]
INF = F32(np.inf)

MISTAKES = ("neighbour_first_order", "stride1_ignored", "gids_rank_major", "segment_forgets_first", "segment_index_b_plus_1",
            "field_map_twice", "slab_tail_dropped", "split_last_slice_dropped", "id_truncated_32", "butterfly_first_step")


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.int32)


def same_bits(a, b) -> bool:
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def field_blocks(num_sparse: int, world: int):
    """FieldShards' split, restated: contiguous blocks in rank order, sizes differ by at most one.  (first, count)."""
    base, extra = divmod(num_sparse, world)
    count = [base + (1 if r < extra else 0) for r in range(world)]
    return [sum(count[:r]) for r in range(world)], count


# =====================================================================================================================
# a. dfm_shard_gather: (D, (world, nf, B), stride kind[, out-of-range ids]).
# Planted: -0.0 and a denormal in row vocab - 1 (which ids select), inf in row vocab - 2 (which no id selects).
# =====================================================================================================================
GATHER_D = (4, 8, 12, 16, 32, 64)
GATHER_SHAPES = ((1, 1, 4), (3, 3, 36), (8, 2, 4))
GATHER_STRIDES = ("default", "padded", "packed")
GATHER_VOCAB = {1: (70000,), 2: (3, 70000), 3: (3, 50, 70000)}
GATHER_CASES = list(itertools.product(GATHER_D, GATHER_SHAPES, GATHER_STRIDES))
OOR_WIDE = 2 ** 32 + 1


def gather_case_id(c):
    return "D{}-w{}f{}B{}-{}".format(c[0], *c[1], c[2])


def table_layout(D: int, stride: str):
    """(floats per row of the w2 buffer, floats per row of the w1 buffer, float offset of w1 inside the w2 buffer or
    None when it has a buffer of its own, dfm_table.stride2, dfm_table.stride1).  "packed" is what
    FeatureEmbedding.pack_tables_() makes: one record of roundup(3 D + 4, 32) floats per row, w1 behind w2."""
    if stride == "default":
        return D, 1, None, 0, 0
    if stride == "padded":
        return D + 4, 2, None, D + 4, 2
    rs = (3 * D + 4 + 31) // 32 * 32
    return rs, rs, D, rs, rs


@functools.lru_cache(maxsize=4)
def _gather_inputs(D, shape, stride):
    world, nf, B = shape
    rng = _rng(21, D, *shape, GATHER_STRIDES.index(stride))
    vocab = GATHER_VOCAB[nf]
    w2 = [rng.standard_normal((V, D)).astype(F32) for V in vocab]
    w1 = [rng.standard_normal(V).astype(F32) for V in vocab]
    ids = np.empty((world, nf, B), dtype=np.int64)
    for j, V in enumerate(vocab):
        w2[j][V - 1, 0], w2[j][V - 1, 1], w1[j][V - 1] = NEG_ZERO, DENORMAL, (NEG_ZERO, DENORMAL)[j % 2]
        w2[j][V - 2], w1[j][V - 2] = INF, INF
        pick = rng.integers(0, V, (world, B))
        pick[pick == V - 2] = V - 1
        ids[:, j] = pick
    ids[0, :, 0] = 0                                  # padding: reads row 0
    ids[0, :, 1] = np.asarray(vocab) - 1
    ids[0, :, 3] = ids[0, :, 2]                       # a duplicate next to its twin
    ids[-1, :, B - 1] = ids[0, :, 1]                  # ... and the last row again in the last item of all
    bad = ids.copy()                                  # the separate sub-case: the same tables, three ids out of range
    bad[-1, nf - 1, 0], bad[-1, 0, 1], bad[-1, nf - 1, 2] = -1, vocab[0], OOR_WIDE
    base = dict(D=D, world=world, nf=nf, B=B, stride=stride, vocab=vocab, w2=w2, w1=w1)
    return dict(base, ids=ids, oor=False), dict(base, ids=bad, oor=True)


def gather_inputs(case, oor=False):
    return _gather_inputs(*case)[int(bool(oor))]


def gather_buffers(inp):
    """Per owned field the float32 buffers as they lie in memory, NaN in every float that is no weight:
    dict(buf2 (V * row2,), buf1 (V * row1,) or None when w1 lives in buf2, off1)."""
    D = inp["D"]
    row2, row1, off1, _, _ = table_layout(D, inp["stride"])
    out = []
    for w2, w1 in zip(inp["w2"], inp["w1"]):
        b2 = np.full((w2.shape[0], row2), np.nan, dtype=F32)
        b2[:, :D] = w2
        if off1 is None:
            b1 = np.full((w2.shape[0], row1), np.nan, dtype=F32)
            b1[:, 0] = w1
            out.append(dict(buf2=b2.reshape(-1), buf1=b1.reshape(-1), off1=0))
        else:
            b2[:, off1] = w1
            out.append(dict(buf2=b2.reshape(-1), buf1=None, off1=off1))
    return out


def gather_reach(case, oor=False) -> dict:
    inp = gather_inputs(case, oor)
    D, world, nf, B, ids = inp["D"], inp["world"], inp["nf"], inp["B"], inp["ids"]
    lpr = D // 4
    threads = world * B * nf * lpr
    v = np.asarray(inp["vocab"])[None, :, None]
    flat = [ids[:, j].reshape(-1) for j in range(nf)]
    return dict(lanes=lpr, threads=threads, mod256=threads % THREADS, blocks=-(-threads // THREADS),
                straddle=THREADS % lpr != 0 and threads > THREADS, vocab=inp["vocab"],
                zero=bool((ids == 0).any()), last=bool((ids == v - 1).any()),
                dup=all(np.unique(f).size < f.size for f in flat), inf_row_selected=bool((ids == v - 2).any()),
                negative=bool((ids < 0).any()), at_vocab=bool((ids == v).any()), wide=bool((ids == OOR_WIDE).any()),
                strides=table_layout(D, inp["stride"])[3:])


def gather_expect(inp):
    """The documented layout from the logical tables: send = [p][e (B, nf, D) | w (B, nf)], gids (nf, world * B), the
    error flag.  An id outside [0, vocab) counts as 0."""
    ids, nf = inp["ids"], inp["nf"]
    v = np.asarray(inp["vocab"], dtype=np.int64)[None, :, None]
    bad = (ids < 0) | (ids >= v)
    idc = np.where(bad, 0, ids)
    e = np.stack([inp["w2"][j][idc[:, j]] for j in range(nf)], axis=2)            # (world, B, nf, D)
    w = np.stack([inp["w1"][j][idc[:, j]] for j in range(nf)], axis=2)            # (world, B, nf)
    send = np.concatenate([e.reshape(inp["world"], -1), w.reshape(inp["world"], -1)], axis=1).reshape(-1)
    return send, np.ascontiguousarray(idc.transpose(1, 0, 2)).reshape(nf, -1), int(bad.any())


def emu_gather(inp, mistake=None):
    """One (p, b, j) item after the other over the memory buffers.  Returns (send, gids flat, error flag); floats and
    ids nobody wrote stay NaN / -7."""
    D, world, nf, B, vocab = inp["D"], inp["world"], inp["nf"], inp["B"], inp["vocab"]
    row2, row1, _, a2, a1 = table_layout(D, inp["stride"])
    s2, s1 = (a2 or D), (a1 or 1)
    if mistake == "stride1_ignored":
        s1 = 1
    bufs = gather_buffers(inp)
    seg = B * nf * (D + 1)
    send = np.full(world * seg, np.nan, dtype=F32)
    gids = np.full(nf * world * B, -7, dtype=np.int64)
    err = 0
    for p, b, j in itertools.product(range(world), range(B), range(nf)):
        i = int(inp["ids"][p, j, b])
        if mistake == "id_truncated_32":
            i &= 0xFFFFFFFF
        if i < 0 or i >= vocab[j]:
            err, i = 1, 0
        send[p * seg + (b * nf + j) * D:p * seg + (b * nf + j + 1) * D] = bufs[j]["buf2"][i * s2:i * s2 + D]
        jw = j - 1 if (mistake == "neighbour_first_order" and j > 0) else j
        src = bufs[jw]["buf1"] if bufs[jw]["buf1"] is not None else bufs[jw]["buf2"]
        send[p * seg + B * nf * D + b * nf + j] = src[bufs[jw]["off1"] + min(i, vocab[jw] - 1) * s1]
        gids[(p * nf + j) * B + b if mistake == "gids_rank_major" else j * world * B + p * B + b] = i
    return send, gids, err


def gather_check(inp, send, gids, err):
    """Asserts bit equality with the restated layout; every word written."""
    want_send, want_gids, want_err = gather_expect(inp)
    assert not np.isnan(want_send).any()
    assert same_bits(send, want_send), "send differs from [p][e (B, nf, D) | w (B, nf)]"
    assert np.array_equal(np.asarray(gids).reshape(want_gids.shape), want_gids), "gids differs from ids.transpose"
    assert int(err) == want_err, "error flag"


# =====================================================================================================================
# b. dfm_shard_pack: dict(world, S, D, B, n, slabs).  F = S + 3 schema positions; field_of_sparse is a seeded
# permutation that is not the identity and (S >= 3) not monotone; the three positions that are nobody's hold inf.
# Slabs (float offset, out_features, in_features, splits) of the dense gradient: n = 1028 only.
# Bar of the dense part: splits additions -> (splits + 1) U (|g| + sum|s_q|); bit-equal to ((g + s_0) + s_1) + ...
# =====================================================================================================================
PACK_WORLD_S = ((1, 1), (2, 2), (3, 5), (8, 11))
PACK_D = (4, 12, 64)
PACK_B = (4, 36, 260)
PACK_N = (0, 4, 1028)
PACK_SLABS = {"none": (), "one": ((16, 4, 8, 3),), "two": ((16, 4, 8, 8), (64, 12, 4, 11))}
_PACK_DENSE = ((0, "none"), (4, "none"), (1028, "none"), (1028, "one"), (1028, "two"))


def _pack_cases():
    out = []
    for i, ((world, S), D, B) in enumerate(itertools.product(PACK_WORLD_S, PACK_D, PACK_B)):
        n, slabs = _PACK_DENSE[i % 5]
        out.append(dict(world=world, S=S, D=D, B=B, n=n, slabs=slabs))
    return out


PACK_CASES = _pack_cases()


def pack_case_id(c):
    return "w{world}S{S}-D{D}-B{B}-n{n}-{slabs}".format(**c)


def _pack_key(c):
    return (c["world"], c["S"], c["D"], c["B"], c["n"], c["slabs"])


def field_map(S: int, key) -> tuple:
    """field_of_sparse over F = S + 3 positions: distinct, not the identity, not monotone when S >= 3."""
    rng = _rng(22, S, key)
    while True:
        fos = tuple(int(x) for x in rng.permutation(S + 3)[:S])
        d = np.diff(fos)
        if fos != tuple(range(S)) and fos[0] != 0 and (S < 3 or ((d > 0).any() and (d < 0).any())):
            return fos


@functools.lru_cache(maxsize=None)
def _pack_inputs(key):
    world, S, D, B, n, slabs = key
    rng = _rng(23, world, S, D, B, n, len(PACK_SLABS[slabs]))
    F = S + 3
    fos = field_map(S, 1)
    first, count = field_blocks(S, world)
    g_field = rng.standard_normal((B, F, D)).astype(F32)
    g_first = rng.standard_normal(B).astype(F32)
    dense = rng.standard_normal(n).astype(F32)
    for f in set(range(F)) - set(fos):
        g_field[:, f] = INF
    g_field[0, fos[0], 0], g_field[B - 1, fos[S - 1], D - 1], g_first[1] = NEG_ZERO, DENORMAL, NEG_ZERO
    if n:
        dense[0], dense[1] = NEG_ZERO, DENORMAL
    sl = [(off, o, i, sp, rng.standard_normal((sp, o * i)).astype(F32)) for off, o, i, sp in PACK_SLABS[slabs]]
    return dict(world=world, S=S, F=F, D=D, B=B, n=n, fos=fos, first=first, count=count, g_field=g_field, g_first=g_first,
                dense=dense, slabs=sl)


def pack_inputs(c):
    return _pack_inputs(_pack_key(c))


def pack_segment(B, nf, D, n):
    return B * nf * D + B + n


def pack_reach(c) -> dict:
    p = pack_inputs(c)
    rows4, first4, dense4 = p["B"] * p["S"] * p["D"] // 4, p["B"] // 4 * p["world"], p["n"] // 4
    fos, d = p["fos"], np.diff(p["fos"])
    return dict(blocks=tuple(p["count"]), rows_end_inside=rows4 % THREADS != 0,
                first_end_inside=(rows4 + first4) % THREADS != 0,
                dense_end_inside=dense4 > 0 and (rows4 + first4 + dense4) % THREADS != 0,
                workgroups=-(-(rows4 + first4 + dense4) // THREADS),
                map_identity=fos == tuple(range(p["S"])), map_monotone=bool((d > 0).all() or (d < 0).all()),
                unrolled_no_tail=any(s[3] >= 8 and s[3] % 8 == 0 for s in p["slabs"]),
                unrolled_tail3=any(s[3] >= 8 and s[3] % 8 == 3 for s in p["slabs"]),
                tail_only=any(s[3] < 8 for s in p["slabs"]),
                unslabbed_between=_gaps(p["slabs"], p["n"]))


def _gaps(slabs, n):
    """Un-slabbed floats before the first, between every two and after the last slab-backed weight."""
    if not slabs:
        return False
    edges = [0] + [x for off, o, i, _, _ in slabs for x in (off, off + o * i)] + [n]
    return all(edges[k] < edges[k + 1] for k in range(0, len(edges), 2))


def dense_sum_f32(p, mistake=None):
    """((g + s_0) + s_1) + ... in float32, slab order."""
    g = p["dense"].copy()
    for off, o, i, sp, data in p["slabs"]:
        for q in range(sp // 8 * 8 if mistake == "slab_tail_dropped" else sp):
            g[off:off + o * i] = g[off:off + o * i] + data[q]
    return g


def dense_sum_fp64(p):
    """(sum, bar): (splits + 1) U (|g| + sum|s_q|)."""
    g, a = p["dense"].astype(np.float64), np.abs(p["dense"].astype(np.float64))
    k = np.ones(p["n"])
    for off, o, i, sp, data in p["slabs"]:
        g[off:off + o * i] += data.astype(np.float64).sum(0)
        a[off:off + o * i] += np.abs(data.astype(np.float64)).sum(0)
        k[off:off + o * i] += sp
    return g, k * U * a


def pack_expect(p):
    """Per peer q the restated segment [d e of q's fields (B, nf_q, D) | d first (B) | dense + slabs (n)]."""
    fos, dense = np.asarray(p["fos"]), dense_sum_f32(p)
    return [np.concatenate([p["g_field"][:, fos[lo:lo + c]].reshape(-1), p["g_first"], dense])
            for lo, c in zip(p["first"], p["count"])]


def emu_pack(p, mistake=None):
    """The send buffer (NaN where nobody wrote) filled one (q, b, j) row at a time through segment offsets."""
    B, D, n, fos = p["B"], p["D"], p["n"], p["fos"]
    start = [0]
    for c in p["count"]:
        start.append(start[-1] + B * c * D + (0 if mistake == "segment_forgets_first" else B) + n)
    send = np.full(sum(pack_segment(B, c, D, n) for c in p["count"]), np.nan, dtype=F32)
    dense = dense_sum_f32(p, mistake)
    for q, (lo, c) in enumerate(zip(p["first"], p["count"])):
        for b, j in itertools.product(range(B), range(c)):
            f = fos[lo + j]
            if mistake == "field_map_twice":
                f = fos[f % p["S"]]
            o = start[q] + (b * c + j) * D
            send[o:o + D] = p["g_field"][b, f]
        o = start[q] + B * c * D
        send[o:o + B] = p["g_first"]
        send[o + B:o + B + n] = dense
    return send


def pack_check(p, send) -> float:
    """Bit equality of every segment with the restatement (which holds the fp32 slab sum); the dense part of the first
    segment against fp64.  Returns the worst error / bar of the dense part."""
    want = np.concatenate(pack_expect(p))
    send = np.asarray(send, dtype=F32).reshape(-1)
    assert send.size == want.size and not np.isnan(want).any()
    assert same_bits(send, want), "send differs from [d e (B, nf_q, D) | d first (B) | dense (n)] per peer"
    at, dense = 0, []
    for c in p["count"]:
        at += pack_segment(p["B"], c, p["D"], p["n"])
        dense.append(send[at - p["n"]:at])
    assert all(same_bits(d, dense[0]) for d in dense), "the peers' dense parts differ"
    ref, bar = dense_sum_fp64(p)
    return ratio(dense[0].astype(np.float64) - ref, bar)


# =====================================================================================================================
# c. dfm_shard_rowgrad: dict(world, B, nf, D, kind, n).  d_recv = world segments [d e (B, nf, D) | d first (B) | NaN (n)].
#   spans      (3, 20): id 7 in all three segments, id 9 only in the last sample of segment 0 and the first of
#              segment 1, padding ids
#   mixed / split2049 / run4096   (8, 516): field 0's first chunk as tests/tail_cases.py::rowgrad_inputs
# =====================================================================================================================
ROWGRAD_BIG = (8, 516, 2)
ROWGRAD_KINDS = ("mixed", "split2049", "run4096")
MIXED_RUNS = (300, 65, 64, 9, 8)


def _rowgrad_cases():
    out = [dict(world=3, B=20, nf=3, D=16, kind="spans", n=n) for n in (0, 12)]
    for i, (D, kind) in enumerate(itertools.product((4, 16, 64), ROWGRAD_KINDS)):
        out.append(dict(world=8, B=516, nf=2, D=D, kind=kind, n=(0, 12)[i % 2]))
    out.append(dict(world=8, B=516, nf=2, D=12, kind="mixed", n=12))
    return out


ROWGRAD_CASES = _rowgrad_cases()


def rowgrad_case_id(c):
    return "w{world}B{B}-D{D}-{kind}-n{n}".format(**c)


def _rowgrad_key(c):
    return (c["world"], c["B"], c["nf"], c["D"], c["kind"], c["n"])


def segment_recv(g2, g1, world, B, n_dense):
    """(world * B, nf, D), (world * B,) -> the receive buffer: one segment per source rank, NaN in the dense tail."""
    nf, D = g2.shape[1:]
    seg = pack_segment(B, nf, D, n_dense)
    recv = np.full((world, seg), np.nan, dtype=F32)
    recv[:, :B * nf * D] = g2.reshape(world, -1)
    recv[:, B * nf * D:B * nf * D + B] = g1.reshape(world, B)
    return recv.reshape(-1)


def read_segments(recv, world, B, nf, D, segment, mistake=None):
    """Every sample's gradients back out of the segments with the kernel's address arithmetic: sample b of the plan is
    sample b - sg B of segment sg = b / B."""
    b = np.arange(world * B)
    sg = b // (B + 1) if mistake == "segment_index_b_plus_1" else b // B
    loc = b - sg * B
    i2 = (sg * segment)[:, None, None] + (loc[:, None, None] * nf + np.arange(nf)[None, :, None]) * D + np.arange(D)[None, None, :]
    i1 = sg * segment + B * nf * D + loc
    return recv[np.minimum(i2, recv.size - 1)], recv[np.minimum(i1, recv.size - 1)]


@functools.lru_cache(maxsize=None)
def _rowgrad_inputs(key):
    world, B, nf, D, kind, n_dense = key
    n = world * B
    rng = _rng(24, world, B, nf, D, (("spans",) + ROWGRAD_KINDS).index(kind))
    if kind == "spans":
        f0 = rng.integers(10, 30, n)
        f0[[3, 4, 25, 47, 59]] = 7
        f0[[B - 1, B]] = 9
        f0[[0, 21, 58]] = 0
        ids = [f0] + [rng.integers(0, 15, n) for _ in range(nf - 1)]
        vocab = (40,) + (15,) * (nf - 1)
    else:
        if kind == "mixed":
            head = np.repeat(np.arange(5, 5 + len(MIXED_RUNS)), MIXED_RUNS)
            c0 = np.concatenate([head, np.arange(20, 20 + CH - head.size - 3), np.zeros(3, dtype=np.int64)])
        elif kind == "split2049":
            c0 = np.concatenate([np.full(K_SPLIT + 1, 3), np.arange(10, 10 + CH - K_SPLIT - 1)])
        else:
            c0 = np.full(CH, 3)
        ids = [np.concatenate([rng.permutation(c0), rng.integers(1, 20, n - CH)])] + [rng.integers(0, 50, n) for _ in range(nf - 1)]
        vocab = (8192,) + (50,) * (nf - 1)
    g2 = rng.standard_normal((n, nf, D)).astype(F32)
    g1 = rng.standard_normal(n).astype(F32)
    g2[0, 0, 0], g2[n - 1, nf - 1, D - 1], g1[B] = NEG_ZERO, DENORMAL, NEG_ZERO
    return dict(world=world, B=B, nf=nf, D=D, n_dense=n_dense, segment=pack_segment(B, nf, D, n_dense), vocab=vocab,
                gids=np.stack(ids).astype(np.int64), g2=g2, g1=g1, recv=segment_recv(g2, g1, world, B, n_dense))


def rowgrad_inputs(c):
    return _rowgrad_inputs(_rowgrad_key(c))


def rowgrad_reach(c) -> dict:
    """From the ids alone: per run class whether a run has contributions in more than one segment, the chunk
    boundary, and whether the plan lists the split runs."""
    inp = rowgrad_inputs(c)
    world, B, nf, D = inp["world"], inp["B"], inp["nf"], inp["D"]
    n = world * B
    crossing, split_listed, split_runs, prefetch = {}, True, 0, False
    for ch, s in itertools.product(range(-(-n // CH)), range(nf)):
        ids = inp["gids"][s, ch * CH:(ch + 1) * CH]
        sample = np.arange(ch * CH, ch * CH + ids.size)
        rows, count = np.unique(ids[ids != 0], return_counts=True)
        for r, k in zip(rows, count):
            segs = np.unique(sample[ids == r] // B).size
            cl = run_class(int(k))
            crossing[cl] = crossing.get(cl, False) or segs > 1
            if 1 < k <= K_LONG:         # two neighbours of one batch of kRunBatch loads come from different segments
                at = sample[ids == r] // B
                k0 = np.flatnonzero(at[1:] != at[:-1])
                prefetch |= bool((k0 // K_RUN_BATCH == (k0 + 1) // K_RUN_BATCH).any())
            if k > K_SPLIT and is_coop(D):
                split_runs += 1
                split_listed &= rows.size <= CH - K_SPLIT
                crossing["all_segments"] = crossing.get("all_segments", False) or segs == world
    f0 = inp["gids"][0]
    where = lambda r: tuple(np.flatnonzero(f0 == r) // B)            # noqa: E731
    return dict(coop=is_coop(D), chunks=-(-n // CH), boundary_segment=CH // B if n > CH else None,
                boundary_sample=CH % B if n > CH else None, crossing=crossing, split_runs=split_runs,
                prefetch_crossing=prefetch, partial_rows=MAX_SPLIT_RUNS * MAX_SLICES,
                split_listed=split_listed and split_runs > 0, padding=bool((inp["gids"] == 0).any()),
                spans_all=set(where(7)) == set(range(world)), seam_only=tuple(np.flatnonzero(f0 == 9)) == (B - 1, B),
                nan_tail=inp["n_dense"] > 0 and bool(np.isnan(inp["recv"].reshape(world, -1)[:, B * nf * D + B:]).all()))


def lists_expect(gids, g2, g1, D):
    """Per list (chunk c, field s), as tests/tail_cases.py::rowgrad_expect: the fp64 reference, the float32 sequential
    sums where the kernel's sum is sequential (`exact`) and the bars n U sum|g_i| elsewhere."""
    nf, n = gids.shape
    out = []
    for c, s in itertools.product(range(-(-n // CH)), range(nf)):
        sl = slice(c * CH, min((c + 1) * CH, n))
        ids, a2, a1 = gids[s, sl], g2[sl, s], g1[sl]
        ref = H.tail_rowgrad_fp64(ids, a2, a1)
        exact = (ref["count"] <= K_LONG) | (not is_coop(D))
        seq2, seq1 = seq_sum_f32(ids, a2, a1, K_LONG if is_coop(D) else None)
        out.append(dict(c=c, s=s, exact=exact, seq2=seq2, seq1=seq1, ref=ref,
                        bar2=ref["count"][:, None] * U * ref["abs2"], bar1=ref["count"] * U * ref["abs1"]))
    return out


@functools.lru_cache(maxsize=None)
def _rowgrad_expect(key):
    inp = _rowgrad_inputs(key)
    return lists_expect(inp["gids"], inp["g2"], inp["g1"], inp["D"])


def rowgrad_expect(c):
    return _rowgrad_expect(_rowgrad_key(c))


def split_slices(D):
    """Workgroups that share a split run: min(CH / (256 / (D/4)), kMaxSlices)."""
    return min(CH // (THREADS // (D // 4)), MAX_SLICES)


def emu_lists(gids, recv, world, B, D, segment, mistake=None):
    """A correct fp32 implementation over the segments: per list, every run summed one contribution after the other,
    the contributions fetched through read_segments.  Returns [(g2, g1)] in list order."""
    nf, n = gids.shape
    g2, g1 = read_segments(recv, world, B, nf, D, segment, mistake)
    out = []
    for c, s in itertools.product(range(-(-n // CH)), range(nf)):
        sl = slice(c * CH, min((c + 1) * CH, n))
        ids = gids[s, sl].copy()
        if mistake == "split_last_slice_dropped" and is_coop(D):
            rows, count = np.unique(ids[ids != 0], return_counts=True)
            if rows.size <= CH - K_SPLIT:
                for r in rows[count > K_SPLIT]:
                    at = np.flatnonzero(ids == r)
                    per = -(-at.size // split_slices(D))
                    ids[at[(at.size - 1) // per * per:]] = 0          # the last slice that holds anything
        out.append(seq_sum_f32(ids, g2[sl, s], g1[sl]))
    return out


# =====================================================================================================================
# d. the chain, N virtual ranks: dict(N, S, B, D).  An all-to-all between virtual ranks is a slice and a concatenate.
# Field s has vocabulary CHAIN_VOCAB[s % 3]; the 50-row fields put 60 % of their samples on id 5 (with N B > 4096 a
# split run fed by every segment).  `ops` (gather, pack, rowgrad) are the emulations above on the host and the
# kernels on the GPU; chain_rows_in / chain_grads_out do the exchanges and return what is to be checked.
# =====================================================================================================================
CHAIN_CASES = (dict(N=3, S=5, B=36, D=8), dict(N=8, S=11, B=516, D=16))
CHAIN_VOCAB = (3, 50, 5000)
CHAIN_N_DENSE = 1028


def chain_case_id(c):
    return "N{N}-S{S}-B{B}-D{D}".format(**c)


@functools.lru_cache(maxsize=None)
def _chain_inputs(key):
    N, S, B, D = key
    rng = _rng(25, N, S, B, D)
    F = S + 3
    vocab = tuple(CHAIN_VOCAB[s % 3] for s in range(S))
    ids = np.stack([rng.integers(0, V, (N, B)) for V in vocab], axis=1).astype(np.int64)          # (N, S, B)
    for s in range(S):
        if vocab[s] == 50:
            ids[:, s][rng.uniform(size=(N, B)) < 0.6] = 5
    first, count = field_blocks(S, N)
    packs = []
    for r in range(N):
        p = dict(_pack_inputs((N, S, D, B, CHAIN_N_DENSE, "two")))
        rr = _rng(26, N, S, B, D, r)
        p["g_field"] = rr.standard_normal((B, F, D)).astype(F32)
        p["g_first"] = rr.standard_normal(B).astype(F32)
        p["dense"] = rr.standard_normal(CHAIN_N_DENSE).astype(F32)
        p["slabs"] = [(off, o, i, sp, rr.standard_normal((sp, o * i)).astype(F32)) for off, o, i, sp, _ in p["slabs"]]
        packs.append(p)
    return dict(N=N, S=S, B=B, D=D, F=F, vocab=vocab, ids=ids, first=first, count=count, fos=packs[0]["fos"], packs=packs,
                w2=[rng.standard_normal((V, D)).astype(F32) for V in vocab],
                w1=[rng.standard_normal(V).astype(F32) for V in vocab])


def chain_inputs(c):
    return _chain_inputs((c["N"], c["S"], c["B"], c["D"]))


def chain_owner_gather_inputs(ch, r):
    """What owner r's dfm_shard_gather sees: the ids "received" = every rank's (nf_r, B) block of its (S, B) ids."""
    lo, c = ch["first"][r], ch["count"][r]
    return dict(D=ch["D"], world=ch["N"], nf=c, B=ch["B"], stride="packed", vocab=ch["vocab"][lo:lo + c],
                w2=ch["w2"][lo:lo + c], w1=ch["w1"][lo:lo + c], ids=np.ascontiguousarray(ch["ids"][:, lo:lo + c]), oor=False)


def chain_reassemble(ch, sends):
    """sends[r] = owner r's send buffer.  The rows all-to-all, then every rank's (B, S, D) / (B, S)."""
    N, S, B, D = ch["N"], ch["S"], ch["B"], ch["D"]
    fe, fo = np.full((N, B, S, D), np.nan, dtype=F32), np.full((N, B, S), np.nan, dtype=F32)
    for r, send in enumerate(sends):
        lo, c = ch["first"][r], ch["count"][r]
        seg = np.asarray(send, dtype=F32).reshape(N, B * c * (D + 1))
        for p in range(N):                                   # segment p of owner r goes to rank p
            fe[p, :, lo:lo + c] = seg[p, :B * c * D].reshape(B, c, D)
            fo[p, :, lo:lo + c] = seg[p, B * c * D:].reshape(B, c)
    return fe, fo


def chain_check_rows(ch, fe, fo):
    for p, s in itertools.product(range(ch["N"]), range(ch["S"])):
        i = ch["ids"][p, s]
        assert same_bits(fe[p, :, s], ch["w2"][s][i]) and same_bits(fo[p, :, s], ch["w1"][s][i]), (p, s)


def chain_received(ch, sends):
    """sends[p] = rank p's gradient send buffer.  The gradient all-to-all: owner r's receive buffer = segment r of
    every rank, source-rank major."""
    seg = [pack_segment(ch["B"], c, ch["D"], CHAIN_N_DENSE) for c in ch["count"]]
    start = np.r_[0, np.cumsum(seg)]
    return [np.concatenate([np.asarray(sends[p], dtype=F32).reshape(-1)[start[r]:start[r + 1]] for p in range(ch["N"])])
            for r in range(ch["N"])]


@functools.lru_cache(maxsize=None)
def _chain_global(key):
    """The whole batch: gids (S, N B), the gradients of the SPARSE fields (N B, S, D) and (N B,), and per owner the
    lists' expectations."""
    ch = _chain_inputs(key)
    gids = np.concatenate([ch["ids"][p] for p in range(ch["N"])], axis=1)
    fos = np.asarray(ch["fos"])
    g2 = np.concatenate([p["g_field"][:, fos] for p in ch["packs"]], axis=0)
    g1 = np.concatenate([p["g_first"] for p in ch["packs"]])
    per_owner = [lists_expect(gids[lo:lo + c], g2[:, lo:lo + c], g1, ch["D"]) for lo, c in zip(ch["first"], ch["count"])]
    return gids, g2, g1, per_owner


def chain_global(c):
    return _chain_global((c["N"], c["S"], c["B"], c["D"]))


def chain_check_dense(ch, r, recv):
    """Every dense part owner r received equals its sender's dense + slabs bit for bit."""
    c = ch["count"][r]
    seg = np.asarray(recv, dtype=F32).reshape(ch["N"], -1)
    for p in range(ch["N"]):
        assert same_bits(seg[p, ch["B"] * c * ch["D"] + ch["B"]:], dense_sum_f32(ch["packs"][p])), (r, p)


# =====================================================================================================================
# e. dfm_sum_floats: thread t of 1024 adds x[t], x[t + 1024], ... in order; six xor-butterfly steps 32 .. 1 inside each
# 64-lane wave; the 16 wave sums are added one after the other.  Bar against fp64: n U sum|x|.
# =====================================================================================================================
SUM_N = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4099)


def sum_inputs(n):
    rng = _rng(27, n)
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(F32)


def sum_reach(n) -> dict:
    """Strided rounds of the 1024 threads, whether the last one is partial, whether some wave has idle lanes."""
    return dict(rounds=-(-n // 1024), partial_round=n % 1024 != 0, idle_lanes=0 < n < 1024 and n % 64 != 0,
                idle_waves=n <= 1024 - 64, one_wave=0 < n <= 64)


def emu_sum_floats(x, mistake=None):
    x = np.asarray(x, dtype=F32)
    acc = np.zeros(1024, dtype=F32)
    for k in range(0, x.size, 1024):
        part = x[k:k + 1024]
        acc[:part.size] = acc[:part.size] + part
    w = acc.reshape(16, 64)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1)[1 if mistake == "butterfly_first_step" else 0:]:
        w = w + w[:, lane ^ m]
    tot = F32(0.0)
    for i in range(16):
        tot = tot + w[i, 0]
    return F32(tot)


def sum_check(x, got) -> float:
    """Bit equality with the emulation; returns the error against fp64 / (n U sum|x|)."""
    x = np.asarray(x, dtype=F32)
    assert same_bits([got], [emu_sum_floats(x)]), "not the fixed order"
    x64 = x.astype(np.float64)
    return ratio(float(got) - x64.sum(), x.size * U * np.abs(x64).sum())


# =====================================================================================================================
# f. dfm_stage_record: 255, 256 and 257 sixteen-byte words (and one)
# =====================================================================================================================
STAGE_NBYTES = (16, 4080, 4096, 4112)


def stage_reach(nbytes) -> dict:
    words = nbytes // 16
    return dict(words=words, workgroups=-(-words // THREADS), last_partial=words % THREADS != 0)


def stage_inputs(nbytes):
    return _rng(28, nbytes).integers(0, 2 ** 32, nbytes // 4, dtype=np.uint32).view(np.int32)
