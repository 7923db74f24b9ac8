"""GPU: the five device entries of the field-sharded step (csrc/shard.hip) entry by entry, and chained as N virtual
ranks in one process, against the restated layouts, float32 emulations and fp64 references of tests/shard_cases.py.
Copies are compared bit for bit, fixed-order sums with their emulation bit for bit, everything else with the bar
n U sum|term|.  Every input, output and workspace is a guarded buffer, outputs NaN- or pattern-filled, and the guards
are checked after every launch.  tests/test_cpu_shard_reference.py proves on the host that each case reaches the
branch it claims and that every planted mistake fails a check used here.  Lines starting with SHARD-RATIO carry the
worst error / bar of each bar-checked test."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import shard_cases as S
from tests import tail_cases as T
from tests.helpers import GuardedBuffer as G, npy
from tests.test_gpu_tail_matrix import IG, NAN_BITS, PATTERN, Plan, _all_bits, _intact, _same_bits

pytestmark = pytest.mark.gpu

CH = T.CH


def _libs():
    from deepfm_amd import _lib
    return _lib, _lib.load()


def _note(name, r):
    print(f"SHARD-RATIO gpu {name}: {r:.3f}")
    assert r <= 1.0, (name, r)


def _i32(values):
    return (C.c_int32 * len(values))(*[int(v) for v in values])


def _wide(array):
    """int64 values on a guarded buffer."""
    a = np.ascontiguousarray(array, dtype=np.int64).reshape(-1)
    b = IG(a.size, 0, wide=True)
    b.i.copy_(torch.from_numpy(a))
    return b


class Kept:
    """A float32 input on a guarded buffer that a launch must leave as it is."""

    def __init__(self, array):
        self.g = G.of(array)
        self.was = self.g.t.clone()

    def ptr(self):
        return self.g.whole.data_ptr() + 4 * self.g.lo        # (also where the payload is empty: n_dense = 0)

    def unchanged(self):
        return _same_bits(self.g.t, self.was)


# =====================================================================================================================
# a. dfm_shard_gather
# =====================================================================================================================
class DeviceTables:
    """The owned tables of a gather case, each exactly `vocab` rows on a guarded buffer, and their dfm_table array."""

    def __init__(self, _l, inp):
        _, _, off1, a2, a1 = S.table_layout(inp["D"], inp["stride"])
        self.c = (_l.Table * inp["nf"])()
        self.bufs = []
        for j, b in enumerate(S.gather_buffers(inp)):
            b2 = Kept(b["buf2"])
            b1 = Kept(b["buf1"]) if b["buf1"] is not None else None
            self.c[j].w2, self.c[j].w1 = b2.ptr(), (b1.ptr() if b1 else b2.ptr() + 4 * off1)
            self.c[j].stride2, self.c[j].stride1 = a2, a1
            self.bufs += [b2] + ([b1] if b1 else [])
        self.vocab = _i32(inp["vocab"])


def _gather(_l, lib, inp, tabs):
    """One launch; returns (send, gids, flag) after the guard and input checks."""
    world, nf, B, D = inp["world"], inp["nf"], inp["B"], inp["D"]
    ids = _wide(inp["ids"])
    send, gids, err = G(world * B * nf * (D + 1)), IG(nf * world * B, PATTERN, wide=True), IG(1, 0)
    _l.check(lib.dfm_shard_gather(tabs.c, tabs.vocab, nf, D, world, B, ids.ptr(), send.ptr(), gids.ptr(), err.ptr(),
                                  _l.stream_handle()))
    _intact(send, gids, err, ids, *[b.g for b in tabs.bufs])
    assert all(b.unchanged() for b in tabs.bufs), "a table changed"
    assert np.array_equal(npy(ids.i), inp["ids"].reshape(-1)), "the ids changed"
    return send, gids, int(err.i[0])


@pytest.mark.parametrize("case", S.GATHER_CASES, ids=S.gather_case_id)
def test_gather(case):
    _l, lib = _libs()
    tabs = DeviceTables(_l, S.gather_inputs(case))
    for oor in (False, True):
        inp = S.gather_inputs(case, oor)
        send, gids, err = _gather(_l, lib, inp, tabs)
        assert bool(torch.isfinite(send.t).all()), "a float of send was not written (or row vocab - 2 was read)"
        assert not bool((gids.i == PATTERN).any()), "an id of gids was not written"
        S.gather_check(inp, npy(send.t), npy(gids.i), err)
        assert err == int(oor)


# =====================================================================================================================
# b. dfm_shard_pack
# =====================================================================================================================
def _pack(_l, lib, p):
    """One launch of a pack input set; returns the send buffer as numpy after the guard and input checks."""
    B, D, n, S_, F = p["B"], p["D"], p["n"], p["S"], p["F"]
    g_field, g_first, dense = Kept(p["g_field"]), Kept(p["g_first"]), Kept(p["dense"])
    works = [Kept(data) for *_, data in p["slabs"]]
    refs = (_l.SlabRef * max(len(works), 1))()
    for r, w, (off, o, i, sp, _) in zip(refs, works, p["slabs"]):
        r.workspace, r.g_w = w.ptr(), dense.ptr() + 4 * off
        r.batch, r.out_features, r.in_features, r.splits = 64, o, i, sp
    seg = [lib.dfm_shard_pack_segment(B, c, D, n) for c in p["count"]]
    assert seg == [S.pack_segment(B, c, D, n) for c in p["count"]]
    send = G(sum(seg))
    _l.check(lib.dfm_shard_pack(_i32(p["first"]), _i32(p["count"]), p["world"], _i32(p["fos"]), S_, F, D, B, g_field.ptr(),
                                g_first.ptr(), dense.ptr(), n, refs if works else None, len(works), send.ptr(),
                                _l.stream_handle()))
    kept = [g_field, g_first, dense, *works]
    _intact(send, *[k.g for k in kept])
    assert all(k.unchanged() for k in kept), "d_dense, g_field, g_first or a slab workspace changed"
    assert bool(torch.isfinite(send.t).all()), "a float of send was not written (or a field that is nobody's was read)"
    return npy(send.t)


@pytest.mark.parametrize("case", S.PACK_CASES, ids=S.pack_case_id)
def test_pack(case):
    _l, lib = _libs()
    p = S.pack_inputs(case)
    _note("pack dense part", S.pack_check(p, _pack(_l, lib, p)))


# =====================================================================================================================
# c. dfm_shard_rowgrad
# =====================================================================================================================
def _shard_rowgrad(_l, lib, plan, recv, world, B, nf, D, segment, expect, what):
    """dfm_shard_rowgrad over the received segments on `plan`, twice: rows, bits / bars per list, the rows behind
    num_uniq, the re-armed arrival counter.  Returns (worst error / bar, row_g2, row_g1, lists)."""
    lists = plan.lists()
    nl = len(lists)
    assert nl == len(expect)
    g2, g1 = G(nl * CH * D), G(nl * CH)

    def launch():
        _l.check(lib.dfm_shard_rowgrad(nf, D, world, B, recv.ptr(), segment, plan.sorted_pos.ptr(), plan.seg.ptr(),
                                       plan.num.ptr(), g2.ptr(), g1.ptr(), _l.stream_handle()))
        _intact(g2, g1, recv.g, *plan.bufs())

    launch()
    r2, r1 = g2.view(nl, CH, D), g1.view(nl, CH)
    worst = 0.0
    free = lambda n: slice(n, CH - T.MAX_SPLIT_RUNS * T.MAX_SLICES)            # noqa: E731
    for i, ((n, rows, _, _), e) in enumerate(zip(lists, expect)):
        assert n == e["ref"]["rows"].size and np.array_equal(rows, e["ref"]["rows"]), f"{what}: rows of list {i}"
        assert bool(torch.isfinite(r2[i, :n]).all()) and bool(torch.isfinite(r1[i, :n]).all()), \
            f"{what}: list {i}: an element below num_uniq is not finite (never written, or read from a dense tail)"
        worst = max(worst, T.rowgrad_check(e, npy(r2[i, :n]), npy(r1[i, :n])))
        assert _all_bits(r2[i, free(n)], NAN_BITS) and _all_bits(r1[i, free(n)], NAN_BITS), f"{what}: list {i}: a row behind num_uniq"
    first2, first1 = r2.clone(), r1.clone()
    launch()
    for i, (n, *_) in enumerate(lists):
        assert _same_bits(r2[i, :n], first2[i, :n]) and _same_bits(r1[i, :n], first1[i, :n]), f"{what}: second launch"
    assert recv.unchanged(), "the receive buffer changed"
    return worst, r2, r1, lists


@pytest.mark.parametrize("case", S.ROWGRAD_CASES, ids=S.rowgrad_case_id)
def test_rowgrad(case):
    _l, lib = _libs()
    inp = S.rowgrad_inputs(case)
    world, B, nf, D = inp["world"], inp["B"], inp["nf"], inp["D"]
    n = world * B
    plan = Plan(nf, n).build(_l, lib, torch.from_numpy(inp["gids"]).cuda(), inp["vocab"])
    recv = Kept(inp["recv"])
    worst, r2, r1, lists = _shard_rowgrad(_l, lib, plan, recv, world, B, nf, D, inp["segment"], S.rowgrad_expect(case),
                                          S.rowgrad_case_id(case))
    _note("row gradients", worst)
    # segmenting changes addresses only: dfm_rowgrad_build on the same plan over the concatenated arrays, the same bits
    nl = len(lists)
    g_field, g_first = Kept(inp["g2"]), Kept(inp["g1"])
    w2, w1 = G(nl * CH * D), G(nl * CH)
    _l.check(lib.dfm_rowgrad_build(_i32(range(nf)), nf, nf, D, n, g_first.ptr(), g_field.ptr(), plan.sorted_pos.ptr(),
                                   plan.seg.ptr(), plan.num.ptr(), w2.ptr(), w1.ptr(), _l.stream_handle()))
    _intact(w2, w1, g_field.g, g_first.g, *plan.bufs())
    for i, (k, *_) in enumerate(lists):
        assert _same_bits(r2[i, :k], w2.view(nl, CH, D)[i, :k]) and _same_bits(r1[i, :k], w1.view(nl, CH)[i, :k]), \
            f"list {i}: dfm_shard_rowgrad differs from dfm_rowgrad_build over the concatenated batch"


# =====================================================================================================================
# d. the chain: N virtual ranks, the all-to-alls done by slicing
# =====================================================================================================================
@pytest.mark.parametrize("case", S.CHAIN_CASES, ids=S.chain_case_id)
def test_chain_of_virtual_ranks(case):
    _l, lib = _libs()
    ch = S.chain_inputs(case)
    N, B, D = ch["N"], ch["B"], ch["D"]
    all_gids, _, _, per_owner = S.chain_global(case)
    # forward: ids -> owners (a slice), rows of the owned tables -> the batches (a slice)
    sends, gids = [], []
    for r in range(N):
        inp = S.chain_owner_gather_inputs(ch, r)
        send, gid, err = _gather(_l, lib, inp, DeviceTables(_l, inp))
        assert err == 0
        S.gather_check(inp, npy(send.t), npy(gid.i), err)
        lo, c = ch["first"][r], ch["count"][r]
        assert np.array_equal(npy(gid.i).reshape(c, N * B), all_gids[lo:lo + c]), "gids is not the global batch, field-major"
        sends.append(npy(send.t))
        gids.append(gid)
    S.chain_check_rows(ch, *S.chain_reassemble(ch, sends))
    # backward: every rank packs, the segments go to their owners (a slice), the owners reduce
    packed = [_pack(_l, lib, p) for p in ch["packs"]]
    for p, send in zip(ch["packs"], packed):
        S.pack_check(p, send)
    worst = 0.0
    for r, recv_np in enumerate(S.chain_received(ch, packed)):
        lo, c = ch["first"][r], ch["count"][r]
        segment = lib.dfm_shard_pack_segment(B, c, D, S.CHAIN_N_DENSE)
        assert recv_np.size == N * segment
        plan = Plan(c, N * B).build(_l, lib, gids[r].i.view(c, N * B), ch["vocab"][lo:lo + c])
        ratio, *_ = _shard_rowgrad(_l, lib, plan, Kept(recv_np), N, B, c, D, segment, per_owner[r], f"owner {r}")
        worst = max(worst, ratio)
        S.chain_check_dense(ch, r, recv_np)
    _note("chain row gradients", worst)


# =====================================================================================================================
# e. dfm_sum_floats
# =====================================================================================================================
@pytest.mark.parametrize("n", S.SUM_N)
def test_sum_floats(n):
    _l, lib = _libs()
    x = S.sum_inputs(n)
    buf, out = G(n + 8), G(1)                          # NaN outside [0, n)
    buf.t[:n].copy_(torch.from_numpy(x))
    _l.check(lib.dfm_sum_floats(buf.ptr(), n, out.ptr(), _l.stream_handle()))
    _intact(buf, out)
    got = npy(out.t)[0]
    _note("sum_floats", S.sum_check(x, got))
    if n == 0:
        assert S.same_bits([got], [0.0]), "n = 0 gives +0.0"
    assert S.same_bits(npy(buf.t[:n]), x) and _all_bits(buf.t[n:], NAN_BITS)


# =====================================================================================================================
# f. dfm_stage_record
# =====================================================================================================================
@pytest.mark.parametrize("nbytes", S.STAGE_NBYTES)
def test_stage_record(nbytes):
    _l, lib = _libs()
    words = S.stage_inputs(nbytes)
    src, dst = IG.of(words), IG(nbytes // 4)
    _l.check(lib.dfm_stage_record(src.ptr(), dst.ptr(), nbytes, _l.stream_handle()))
    _intact(src, dst)
    assert np.array_equal(npy(dst.i), words) and np.array_equal(npy(src.i), words)
