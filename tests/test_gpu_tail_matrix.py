"""GPU: the tail of the training step (csrc/step_tail.hip, csrc/tail_bodies.h, the row-gradient half of
csrc/rowplan.hip) entry by entry against plain fp64 restatements (tests/helpers.py::tail_*_fp64): row gradients,
DENSE-field gradients, the row-list merge, the dense prepare with slabs and gathered ranks, the norm finalize and the
three update rules on rows and on the dense buffer.  Every output and workspace is a guarded buffer, NaN-filled
(integers: a pattern) unless a case says otherwise, and the guards are checked after every launch.  The cases, the
bars and their derivations live in tests/tail_cases.py; tests/test_cpu_tail_reference.py proves on the host that each
case reaches the branch it claims and that a plain float32 implementation stays inside every bar, so nothing is
excluded from a comparison here.  Lines starting with TAIL-RATIO carry the worst error / bar of each output."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import tail_cases as T
from tests.helpers import GuardedBuffer as G, npy, tail_sq_fp64

pytestmark = pytest.mark.gpu

CH = T.CH
NAN_BITS = 0x7FC00000             # what fill_(nan) writes
PATTERN = 0x55555555              # integer workspaces start as this


def _libs():
    from deepfm_amd import _lib
    return _lib, _lib.load()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _all_bits(t, pattern):
    return bool((_bits(t) == pattern).all())


def _intact(*bufs):
    torch.cuda.synchronize()
    for b in bufs:
        if b is not None:
            assert (b.g if isinstance(b, IG) else b).guards_intact(), "a word outside a buffer was written"


class IG:
    """Guarded buffer of `n` 32-bit integers (`.i`), or of `n` 64-bit ones with wide=True."""

    def __init__(self, n, fill=PATTERN, wide=False):
        self.g = G(n * (2 if wide else 1), 0.0)
        self.i = self.g.t.view(torch.int64 if wide else torch.int32)
        self.i.fill_(fill)

    @classmethod
    def of(cls, array):
        a = np.ascontiguousarray(array, dtype=np.int32)
        b = cls(a.size, 0)
        b.i.copy_(torch.from_numpy(a.reshape(-1)))
        return b

    def ptr(self):
        return self.i.data_ptr()


def _note(name, r):
    print(f"TAIL-RATIO gpu {name}: {r:.3f}")
    assert r <= 1.0, (name, r)


class Plan:
    """dfm_rowplan_build's four outputs (+ the error flag) on guarded, pattern-filled buffers."""

    def __init__(self, S, B):
        self.S, self.B, self.chunks = S, B, (B + CH - 1) // CH
        n = self.chunks * S
        self.sorted_pos, self.uniq, self.seg, self.num = IG(n * CH), IG(n * CH), IG(n * (CH + 1)), IG(n)
        self.err = IG(1, 0)

    def bufs(self):
        return self.sorted_pos, self.uniq, self.seg, self.num, self.err

    def build(self, _l, lib, d_ids, vocab):
        """d_ids: (S, >= B) int64 device tensor, one row per field."""
        S = self.S
        ptrs = (C.c_void_p * S)(*[d_ids[s].data_ptr() for s in range(S)])
        _l.check(lib.dfm_rowplan_build(ptrs, (C.c_int32 * S)(*vocab), S, self.B, self.sorted_pos.ptr(), self.uniq.ptr(),
                                       self.seg.ptr(), self.num.ptr(), self.err.ptr(), None, 0, _l.stream_handle()))
        _intact(*self.bufs())
        assert int(self.err.i[0]) == 0
        return self

    def lists(self):
        """Per list: (num_uniq, rows, seg_start[: num + 1], sorted_pos[: valid])."""
        num = npy(self.num.i)
        uniq, seg, pos = npy(self.uniq.i).reshape(-1, CH), npy(self.seg.i).reshape(-1, CH + 1), npy(self.sorted_pos.i).reshape(-1, CH)
        return [(int(n), uniq[i, :n], seg[i, :n + 1], pos[i, :seg[i, n]] if n else pos[i, :0]) for i, n in enumerate(num)]


def _fmap(positions):
    return (C.c_int32 * len(positions))(*positions)


# =====================================================================================================================
# a. row gradients: dfm_rowgrad_build, and the same through dfm_step_embedding_backward with num_dense = 0
# =====================================================================================================================
@pytest.mark.parametrize("case", T.ROWGRAD_CASES, ids=lambda c: f"D{c[0]}-{c[1]}")
def test_row_gradients(case):
    _l, lib = _libs()
    D, kind = case
    inp = T.rowgrad_inputs(D, kind)
    S, F, B = inp["S"], inp["F"], inp["B"]
    plan = Plan(S, B).build(_l, lib, torch.from_numpy(inp["ids"]).cuda(), inp["vocab"])
    lists = plan.lists()
    nl = len(lists)
    g_field, g_first = G.of(inp["g_field"]), G.of(inp["g_first"])
    fmap = _fmap(inp["fmap"])

    def standalone(g2, g1):
        _l.check(lib.dfm_rowgrad_build(fmap, S, F, D, B, g_first.ptr(), g_field.ptr(), plan.sorted_pos.ptr(),
                                       plan.seg.ptr(), plan.num.ptr(), g2.ptr(), g1.ptr(), _l.stream_handle()))

    def grouped(g2, g1):
        _l.check(lib.dfm_step_embedding_backward(None, 0, None, None, fmap, S, F, D, B, g_first.ptr(), g_field.ptr(),
                                                 plan.sorted_pos.ptr(), plan.seg.ptr(), plan.num.ptr(), g2.ptr(),
                                                 g1.ptr(), None, 0, None, 0, _l.stream_handle()))

    def launch(entry):
        g2, g1 = G(nl * CH * D), G(nl * CH)
        entry(g2, g1)
        _intact(g2, g1, g_field, g_first, *plan.bufs())
        return g2, g1

    g2, g1 = launch(standalone)
    r2, r1 = g2.view(nl, CH, D), g1.view(nl, CH)
    expect = T.rowgrad_expect(D, kind)
    unwritten = sum(int((~torch.isfinite(r2[i, :n])).sum()) + int((~torch.isfinite(r1[i, :n])).sum())
                    for i, (n, *_) in enumerate(lists))
    print(f"TAIL-UNWRITTEN D={D} {kind}: {unwritten} elements of row_g2 / row_g1 below num_uniq are not finite")
    worst = 0.0
    for i, ((n, rows, _, _), e) in enumerate(zip(lists, expect)):
        assert n == e["ref"]["rows"].size and np.array_equal(rows, e["ref"]["rows"])
        assert bool(torch.isfinite(r2[i, :n]).all()) and bool(torch.isfinite(r1[i, :n]).all()), \
            f"list {i}: an element below num_uniq was never written"
        worst = max(worst, T.rowgrad_check(e, npy(r2[i, :n]), npy(r1[i, :n])))
        free = slice(n, CH - T.MAX_SPLIT_RUNS * T.MAX_SLICES)
        assert _all_bits(r2[i, free], NAN_BITS) and _all_bits(r1[i, free], NAN_BITS), f"list {i}: a row behind num_uniq was written"
    _note("row gradients", worst)
    # a second launch on the same plan (the arrival counter re-arms itself) and the grouped entry: the same bits
    first2, first1 = r2.clone(), r1.clone()
    standalone(g2, g1)
    _intact(g2, g1, *plan.bufs())
    h2, h1 = launch(grouped)
    for i, (n, *_) in enumerate(lists):
        assert _same_bits(r2[i, :n], first2[i, :n]) and _same_bits(r1[i, :n], first1[i, :n]), "second launch"
        assert _same_bits(h2.view(nl, CH, D)[i, :n], first2[i, :n]) and _same_bits(h1.view(nl, CH)[i, :n], first1[i, :n]), \
            "dfm_step_embedding_backward differs from dfm_rowgrad_build"
        free = slice(n, CH - T.MAX_SPLIT_RUNS * T.MAX_SLICES)
        assert _all_bits(h2.view(nl, CH, D)[i, free], NAN_BITS) and _all_bits(h1.view(nl, CH)[i, free], NAN_BITS)


# =====================================================================================================================
# b. DENSE-field gradients through dfm_step_embedding_backward
# =====================================================================================================================
@pytest.mark.parametrize("case", T.DENSE_FIELD_CASES, ids=lambda c: f"D{c[0]}-B{c[1]}")
def test_dense_field_gradients(case):
    _l, lib = _libs()
    D, B = case
    inp = T.dense_field_inputs(D, B)
    F, S = T.DENSE_F, len(T.DENSE_SPARSE_POS)
    g_field, g_first = G.of(inp["g_field"]), G.of(inp["g_first"])
    xs = [G.of(x) for x in inp["x"]]
    plan = Plan(S, B).build(_l, lib, torch.from_numpy(inp["ids"]).cuda(), (30, 30))
    fmap = _fmap(T.DENSE_SPARSE_POS)
    alone2, alone1 = G(S * CH * D), G(S * CH)
    _l.check(lib.dfm_rowgrad_build(fmap, S, F, D, B, g_first.ptr(), g_field.ptr(), plan.sorted_pos.ptr(), plan.seg.ptr(),
                                   plan.num.ptr(), alone2.ptr(), alone1.ptr(), _l.stream_handle()))
    _intact(alone2, alone1)
    nums = [n for n, *_ in plan.lists()]
    worst = 0.0
    for nd, sparse, mode in itertools.product(T.DENSE_ND, (False, True), T.dense_modes(B)):
        elems, lay = T.dense_grad_layout(D, nd)
        parts = 1 if mode == "inplace" else mode
        grads = G(elems, 1.0)
        partial = None if mode == "inplace" else G(parts * elems)
        dense_x, dense_g = (C.c_void_p * F)(), (_l.FieldGrad * F)()
        for k in range(nd):
            f = T.DENSE_POS[k]
            dense_x[f] = xs[k].ptr()
            dense_g[f].w2, dense_g[f].b2, dense_g[f].w1, dense_g[f].b1 = (grads.ptr() + 4 * o for o in lay[k])
        d_list = torch.tensor(T.DENSE_POS[:nd], dtype=torch.int32, device="cuda")
        row2, row1 = G(S * CH * D), G(S * CH)
        sp = (fmap, S) if sparse else (None, 0)
        _l.check(lib.dfm_step_embedding_backward(
            d_list.data_ptr(), nd, dense_x, dense_g, sp[0], sp[1], F, D, B, g_first.ptr(), g_field.ptr(),
            plan.sorted_pos.ptr() if sparse else None, plan.seg.ptr() if sparse else None,
            plan.num.ptr() if sparse else None, row2.ptr() if sparse else None, row1.ptr() if sparse else None,
            partial.ptr() if partial else None, parts if partial else 0, grads.ptr() if partial else None,
            elems if partial else 0, _l.stream_handle()))
        _intact(grads, partial, row2, row1, g_field, g_first, *xs, *plan.bufs())
        want, bar = T.dense_field_expect(D, B, nd, mode)
        live = torch.from_numpy(~np.isnan(want)).cuda()
        what = f"nd={nd} sparse={sparse} mode={mode}"
        if mode == "inplace":
            got = grads.view(1, elems)
            assert bool((got[~live] == 1.0).all()), what + ": a float between the gradients changed"
        else:
            got = partial.view(parts, elems)
            assert _all_bits(got[~live], NAN_BITS), what + ": a float of the partial buffer that is no gradient was written"
            assert bool((grads.t == 1.0).all()), what + ": sliced runs do not touch the gradient buffers"
            rows = -(-B // parts)
            for p in range(parts):
                if p * rows >= B:
                    assert bool((got[p][live[p]] == 0).all()), what + f": empty slice {p} is not zero"
        worst = max(worst, T.dense_field_check(want, bar, npy(got)))
        if sparse:
            for i, n in enumerate(nums):
                assert _same_bits(row2.view(S, CH, D)[i, :n], alone2.view(S, CH, D)[i, :n]), what + ": row gradients"
                assert _same_bits(row1.view(S, CH)[i, :n], alone1.view(S, CH)[i, :n]), what + ": row gradients"
        else:
            assert _all_bits(row2.t, NAN_BITS) and _all_bits(row1.t, NAN_BITS)
    _note("DENSE-field gradients", worst)


# =====================================================================================================================
# tables on the device: separate tensors (strides 0) or packed records (stride2 = 64 where a record fits)
# =====================================================================================================================
FIELDS = ("w2", "m2", "v2", "w1", "m1", "v1")


class Tables:
    """`arrays`: per field a dict of (V, D) / (V,) float32 arrays under some of FIELDS; absent ones are NULL in the
    dfm_table (separate layout) or NaN-filled (packed)."""

    def __init__(self, _l, arrays, D, packed):
        self.D, self.packed, self.S = D, packed, len(arrays)
        self.V = arrays[0]["w2"].shape[0]
        self.c = (_l.Table * self.S)()
        self.bufs = []
        self.rs, self.off = T.packed_layout(D)
        for s, a in enumerate(arrays):
            t = self.c[s]
            if packed:
                rec = np.full((self.V, self.rs), np.nan, dtype=np.float32)
                for k, v in a.items():
                    rec[:, self.off[k]:self.off[k] + (D if k.endswith("2") else 1)] = v.reshape(self.V, -1)
                b = G.of(rec)
                for k in FIELDS:
                    setattr(t, k, b.ptr() + 4 * self.off[k])
                t.stride2 = t.stride1 = self.rs
                self.bufs.append(b)
            else:
                d = {k: G.of(v) for k, v in a.items()}
                for k in FIELDS:
                    setattr(t, k, d[k].ptr() if k in d else None)
                t.stride2 = t.stride1 = 0
                self.bufs.append(d)

    def guarded(self):
        return [b for x in self.bufs for b in (x.values() if isinstance(x, dict) else [x])]

    def read(self, s):
        """Everything the field's buffers hold, as numpy: a dict of arrays (separate) or the (V, RS) records."""
        if self.packed:
            return npy(self.bufs[s].view(self.V, self.rs)).copy()
        return {k: npy(b.t).reshape(self.V, -1).copy() for k, b in self.bufs[s].items()}

    def field(self, state, k):
        """(V, D) or (V,) view of field k inside what read() returned; None if the table has no such array."""
        if self.packed:
            o = self.off[k]
            return state[:, o:o + self.D] if k.endswith("2") else state[:, o]
        if k not in state:
            return None
        return state[k] if k.endswith("2") else state[k][:, 0]


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _same_outside(tabs, before, after, rows, what):
    """Rows outside `rows` — and in a packed record the floats between the arrays — keep their bits."""
    if tabs.packed:
        keep = np.ones(before.shape, dtype=bool)
        for k in FIELDS:
            keep[np.ix_(rows, np.arange(tabs.off[k], tabs.off[k] + (tabs.D if k.endswith("2") else 1)))] = False
        assert _bits_equal(before[keep], after[keep]), what + ": a float outside the owned rows changed"
        return
    other = np.ones(tabs.V, dtype=bool)
    other[rows] = False
    for k in before:
        assert _bits_equal(before[k][other], after[k][other]), what + f": {k} changed outside the owned rows"


# =====================================================================================================================
# c. prepare: dfm_step_prepare (merge half + dense half), dfm_step_dense_prepare
# =====================================================================================================================
class DenseSide:
    """The dense half's inputs on guarded buffers, and the slab descriptors."""

    def __init__(self, _l, c):
        d = T.dense_prepare_inputs(c)
        self.c, self.n = c, c["n"]
        self.g, self.p = G.of(d["g"]), G.of(d["p"])
        self.slab_bufs = [G.of(sl) for _, sl in d["slabs"]]
        self.slabs = (_l.SlabRef * max(len(d["slabs"]), 1))()
        for i, (off, sl) in enumerate(d["slabs"]):
            r = self.slabs[i]
            r.workspace, r.g_w = self.slab_bufs[i].ptr(), self.g.ptr() + 4 * off
            r.batch, r.out_features, r.in_features, r.splits = 64, sl.shape[1] // 4, 4, sl.shape[0]
        self.num_slabs = len(d["slabs"])
        self.gathered = G.of(d["gathered"]) if d["gathered"] is not None else None
        self.world, self.stride = c["world"], c["n"] + c["pad"]

    def bufs(self):
        return [self.g, self.p, self.gathered, *self.slab_bufs]

    def check(self, partials, l2=None, scale=None):
        """g against fp64, the partial sums against the |g|^2 of the g the kernel wrote."""
        want, bar = T.dense_prepare_expect(self.c, l2, scale)
        got = npy(self.g.t)
        _note("dense prepare g", T.ratio(got - want, bar))
        _note("dense |g|^2", T.ratio(float(partials.astype(np.float64).sum()) - tail_sq_fp64(got), T.sq_bar(got)))


def _prepare(_l, lib, tabs, L, S, D, rows, num, g2, g1, flag, scale, l2, dense, partials, offset, match):
    return lib.dfm_step_prepare(tabs.c, S, D, L, rows.ptr(), num.ptr(), g2.ptr(), g1.ptr(), flag.ptr(), float(scale),
                                float(l2), dense.g.ptr(), dense.p.ptr(), dense.n, dense.c["n_l2"], dense.slabs,
                                dense.num_slabs, dense.gathered.ptr() if dense.gathered else None, dense.world,
                                dense.stride if dense.gathered else 0, partials.ptr(), offset,
                                match.ptr() if match else None, _l.stream_handle())


@pytest.mark.parametrize("idx", range(len(T.MERGE_CASES)), ids=lambda i: "-".join(map(str, T.MERGE_CASES[i])))
def test_prepare_merge(idx):
    _l, lib = _libs()
    case = T.MERGE_CASES[idx]
    m = T.merge_inputs(case)
    L, S, D, packed = m["L"], m["S"], m["D"], m["packed"]
    dcase = T.DENSE_PREPARE_CASES[idx % len(T.DENSE_PREPARE_CASES)]
    tabs = Tables(_l, [dict(w2=m["w2"][s], w1=m["w1"][s]) for s in range(S)], D, packed)
    before = [tabs.read(s) for s in range(S)]
    rows, num = IG.of(m["rows"]), IG.of(m["num"])
    mb = lib.dfm_rowadam_num_partials(S, D, L)
    npart = lib.dfm_step_prepare_num_partials(S, D, L, dcase["n"])
    pb = -(-dcase["n"] // T.PREP_PER_BLOCK)
    assert mb == -(-L * S * CH * (D // 4) // T.THREADS) and npart == mb + pb
    shift = 3 if packed else 0                    # packed cases: the dense partials start behind a gap
    offset = mb + shift if shift else 0
    results = []
    for use_match in ((False, True) if L >= 3 else (False,)):
        g2, g1, flag = G.of(m["g2"]), G.of(m["g1"]), IG(L * S * CH)
        dense = DenseSide(_l, dcase)
        partials = G(npart + shift + 5)
        match = G(lib.dfm_step_match_bytes(S, L) // 4 + 1) if use_match else None
        if not results:
            # dense partials that would overlap the row partials: refused, nothing launched
            assert _prepare(_l, lib, tabs, L, S, D, rows, num, g2, g1, flag, m["grad_scale"], m["l2"], dense, partials,
                            mb - 1, match) != 0
            torch.cuda.synchronize()
            assert _all_bits(partials.t, NAN_BITS) and _all_bits(flag.i, PATTERN) and _bits_equal(npy(g2.t), m["g2"].reshape(-1))
        _l.check(_prepare(_l, lib, tabs, L, S, D, rows, num, g2, g1, flag, m["grad_scale"], m["l2"], dense, partials,
                          offset, match))
        _intact(g2, g1, flag, partials, match, rows, num, *dense.bufs(), *tabs.guarded())
        results.append((g2, g1, flag, partials, dense))
    g2, g1, flag, partials, dense = results[0]
    owner = npy(flag.i).reshape(L, S, CH)
    behind = np.arange(CH)[None, None, :] >= m["num"][:, :, None]
    assert (owner[behind] == PATTERN).all(), "owner_flag behind num_uniq was written"
    got2, got1 = npy(g2.t).reshape(L, S, CH, D), npy(g1.t).reshape(L, S, CH)
    r2, r1 = T.merge_check(case, owner, got2, got1)
    _note("merged row_g2", r2)
    _note("merged row_g1", r1)
    for s in range(S):
        after = tabs.read(s)
        assert _bits_equal(before[s], after) if packed else all(_bits_equal(before[s][k], after[k]) for k in after), "tables"
    part = npy(partials.t)
    own = T.merge_expect(case)["owner"] == 1
    mine = np.concatenate([got2[own].reshape(-1), got1[own]])
    _note("row |g|^2", T.ratio(float(part[:mb].astype(np.float64).sum()) - tail_sq_fp64(mine), T.sq_bar(mine)))
    dense.check(part[mb + shift:npart + shift], m["l2"], m["grad_scale"])
    assert _all_bits(partials.t[mb:mb + shift], NAN_BITS) and _all_bits(partials.t[npart + shift:], NAN_BITS), \
        "a float outside the partial sums was written"
    if len(results) == 2:       # the match workspace changes how memberships are found, not one bit of the result
        for a, b in zip(results[0][:4], results[1][:4]):
            assert _same_bits(a.i if isinstance(a, IG) else a.t, b.i if isinstance(b, IG) else b.t), "match vs search"
        assert _same_bits(results[0][4].g.t, results[1][4].g.t)


@pytest.mark.parametrize("idx", range(len(T.DENSE_PREPARE_CASES)), ids=lambda i: T.dense_case_id(T.DENSE_PREPARE_CASES[i]))
def test_prepare_dense(idx):
    """The dense half beside one EMPTY row list (its 16 row partials are exact zeros), and the same inputs through
    dfm_step_dense_prepare: bit-identical g and partial sums."""
    _l, lib = _libs()
    c = T.DENSE_PREPARE_CASES[idx]
    d = T.dense_prepare_inputs(c)
    n, D = c["n"], 4
    tabs = Tables(_l, [dict(w2=np.ones((8, D), dtype=np.float32), w1=np.ones(8, dtype=np.float32))], D, False)
    rows, num, flag = IG(CH), IG.of([0]), IG(CH)
    g2, g1 = G(CH * D), G(CH)
    mb, pb = lib.dfm_rowadam_num_partials(1, D, 1), -(-n // T.PREP_PER_BLOCK)
    assert lib.dfm_step_prepare_num_partials(1, D, 1, n) == mb + pb and lib.dfm_step_dense_num_partials(n) == pb
    dense, partials = DenseSide(_l, c), G(mb + pb + 5)
    _l.check(_prepare(_l, lib, tabs, 1, 1, D, rows, num, g2, g1, flag, d["scale"], d["l2"], dense, partials, 0, None))
    _intact(g2, g1, flag, partials, rows, num, *dense.bufs(), *tabs.guarded())
    assert _all_bits(g2.t, NAN_BITS) and _all_bits(g1.t, NAN_BITS) and _all_bits(flag.i, PATTERN)
    part = npy(partials.t)
    assert (part[:mb] == 0).all() and _all_bits(partials.t[mb + pb:], NAN_BITS)
    dense.check(part[mb:mb + pb])
    if d["gathered"] is not None:
        assert np.isnan(npy(dense.gathered.view(c["world"], -1))[:, n:]).all()
        return
    alone, p2 = DenseSide(_l, c), G(pb + 5)
    _l.check(lib.dfm_step_dense_prepare(float(d["l2"]), alone.g.ptr(), alone.p.ptr(), n, c["n_l2"], alone.slabs,
                                        alone.num_slabs, p2.ptr(), _l.stream_handle()))
    _intact(p2, *alone.bufs())
    assert _same_bits(alone.g.t, dense.g.t) and _same_bits(p2.t[:pb], partials.t[mb:mb + pb]), "the two dense halves differ"
    assert _all_bits(p2.t[pb:], NAN_BITS)


# =====================================================================================================================
# d. dfm_grad_norm_finalize
# =====================================================================================================================
@pytest.mark.parametrize("n", T.FINALIZE_N)
def test_grad_norm_finalize(n):
    _l, lib = _libs()
    partials = G.of(np.r_[T.finalize_inputs(n), np.full(3, np.nan, dtype=np.float32)])       # (NaN behind the n partials)
    worst_t = worst_c = 0.0
    for max_norm, with_clip, with_ticks in itertools.product(T.finalize_max_norms(n), (False, True), (False, True)):
        sq, clip = G(1), G(1) if with_clip else None
        step, seed = IG.of([41]), IG(1, (1 << 40) + 5, wide=True)
        _l.check(lib.dfm_grad_norm_finalize(partials.ptr(), n, float(np.float32(max_norm)), sq.ptr(),
                                            clip.ptr() if clip else None, step.ptr() if with_ticks else None,
                                            seed.ptr() if with_ticks else None, _l.stream_handle()))
        _intact(partials, sq, clip, step, seed)
        total, bar_t, want_c, bar_c = T.finalize_expect(n, max_norm)
        worst_t = max(worst_t, T.ratio(float(sq.t[0]) - total, bar_t))
        if clip:
            got = float(clip.t[0])
            assert got == 1.0 if (max_norm == 0.0 or want_c == 1.0) else got < 1.0
            worst_c = max(worst_c, T.ratio(got - want_c, bar_c))
        assert int(step.i[0]) == (42 if with_ticks else 41) and int(seed.i[0]) == (1 << 40) + 5 + int(with_ticks)
    _note("norm total", worst_t)
    _note("clip coefficient", worst_c)


# =====================================================================================================================
# e. apply: dfm_step_apply, dfm_step_dense_apply, dfm_step_apply_plan
# =====================================================================================================================
class ApplyState:
    """Tables, dense buffers and the read-only lists of one apply case, fresh on the device.  SGD: every v buffer is
    NaN-filled (it must keep its bits), or absent with null_v."""

    def __init__(self, _l, c, null_v=False):
        a = T.apply_inputs(c)
        self.c, self.a, sgd = c, a, c["rule"] == "sgd"
        arrays = []
        for t in a["tables"]:
            t = dict(t)
            if sgd:
                for k in ("v2", "v1"):
                    if null_v and not c["packed"]:
                        del t[k]
                    else:
                        t[k] = np.full_like(t[k], np.nan)
            arrays.append(t)
        self.tabs = Tables(_l, arrays, c["D"], c["packed"])
        d = a["dense"]
        self.p, self.m, self.g = G.of(d["p"]), G.of(d["m"]), G.of(d["g"])
        self.v = None if (sgd and null_v) else (G(c["n"]) if sgd else G.of(d["v"]))
        self.rows, self.num, self.flag = IG.of(a["rows"]), IG.of(a["num"]), IG.of(a["flag"])
        self.g2, self.g1 = G.of(a["g2"]), G.of(a["g1"])
        self.lr, self.step = G.of([T.LR]), IG.of([c["t"]])
        self.clip = G.of([T.APPLY_CLIP]) if c["clip"] else None
        h = T.HYPER
        self.opt = _l.Optim(T.RULE_KIND[c["rule"]], float(h["b1"]), float(h["b2"]), float(h["eps"]), float(h["wd"]),
                            float(h["momentum"]), self.lr.ptr())

    def bufs(self):
        return [self.p, self.m, self.v, self.g, self.rows, self.num, self.flag, self.g2, self.g1, self.lr, self.step,
                self.clip, *self.tabs.guarded()]

    def list_args(self):
        a, c = self.a, self.c
        return (self.tabs.c, a["S"], c["D"], a["L"], self.rows.ptr(), self.num.ptr(), self.g2.ptr(), self.g1.ptr(),
                self.flag.ptr(), self.clip.ptr() if self.clip else None, C.byref(self.opt), self.step.ptr())

    def dense_args(self):
        return (self.p.ptr(), self.m.ptr(), self.v.ptr() if self.v else None, self.g.ptr(), self.c["n"], self.c["zero_grad"])

    def snapshot(self):
        return dict(tables=[self.tabs.read(s) for s in range(self.a["S"])], p=npy(self.p.t).copy(), m=npy(self.m.t).copy(),
                    v=npy(self.v.t).copy() if self.v else None, g=npy(self.g.t).copy())

    def inputs_unchanged(self):
        a = self.a
        assert _bits_equal(npy(self.g2.t), a["g2"].reshape(-1)) and _bits_equal(npy(self.g1.t), a["g1"].reshape(-1))
        assert np.array_equal(npy(self.rows.i), a["rows"].reshape(-1)) and np.array_equal(npy(self.flag.i), a["flag"].reshape(-1))
        assert int(self.step.i[0]) == self.c["t"]


def _check_apply(st, before, after, lr, what):
    """One launch took the state `before` (snapshots) to `after`: the owned rows and the dense buffer against fp64,
    everything else bit for bit."""
    c, a, tabs = st.c, st.a, st.tabs
    rule, t = c["rule"], c["t"]
    clip = T.APPLY_CLIP if c["clip"] else None
    worst = {}

    def fold(r):
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)

    for s, (rows, ls, us) in enumerate(T.apply_owned(c)):
        b, f = before["tables"][s], after["tables"][s]
        _same_outside(tabs, b, f, rows, f"{what}: field {s}")
        for w, m, v, g in (("w2", "m2", "v2", a["g2"][ls, s, us]), ("w1", "m1", "v1", a["g1"][ls, s, us])):
            vb, vf = tabs.field(b, v), tabs.field(f, v)
            fold(T.rule_check(rule, tabs.field(b, w)[rows], tabs.field(b, m)[rows], None if rule == "sgd" else vb[rows], g,
                              t, lr, clip, tabs.field(f, w)[rows], tabs.field(f, m)[rows], None if rule == "sgd" else vf[rows]))
            if rule == "sgd" and vb is not None:
                assert _bits_equal(vb, vf), f"{what}: SGD touched {v}"
        z = a["rows"][0, s, 2]                         # g = 0 on m = v = 0 (first launch) / on what the first launch left
        if rule in ("adam", "sgd") and not np.any(tabs.field(b, "m2")[z]) and not np.any(tabs.field(b, "m1")[z]):
            assert _bits_equal(tabs.field(b, "w2")[z], tabs.field(f, "w2")[z]), f"{what}: a row with g = m = v = 0 moved"
            assert tabs.field(b, "w1")[z] == tabs.field(f, "w1")[z]
    fold(T.rule_check(rule, before["p"], before["m"], before["v"], before["g"], t, lr, clip, after["p"], after["m"], after["v"]))
    if rule == "sgd" and before["v"] is not None:
        assert _bits_equal(before["v"], after["v"]), f"{what}: SGD touched the dense v"
    if rule in ("adam", "sgd") and before["g"][-1] == 0 and before["m"][-1] == 0:
        assert after["p"][-1] == before["p"][-1], f"{what}: a dense element with g = m = v = 0 moved"
    if c["zero_grad"]:
        assert _bits_equal(after["g"], np.zeros_like(after["g"])), f"{what}: zero_grad leaves +0.0 in g[0 .. n)"
    else:
        assert _bits_equal(after["g"], before["g"]), f"{what}: g changed without zero_grad"
    for k, v in worst.items():
        _note(f"{rule} {k}", v)


def _same_state(a, b, what, skip_v=False):
    for k in ("p", "m", "v", "g"):
        if a[k] is not None and b[k] is not None and not (skip_v and k == "v"):
            assert _bits_equal(a[k], b[k]), f"{what}: dense {k}"
    for ta, tb in zip(a["tables"], b["tables"]):
        if isinstance(ta, dict):
            for k in ta:
                if k in tb:
                    assert _bits_equal(ta[k], tb[k]), f"{what}: {k}"
        else:
            assert _bits_equal(ta, tb), f"{what}: records"


def _run_step_apply(_l, lib, c, ctx):
    """dfm_step_apply, twice: the second launch reads the learning rate that is in d_lr then."""
    st = ApplyState(_l, c)
    ctx["s0"] = s0 = st.snapshot()
    _l.check(lib.dfm_step_apply(*st.list_args(), *st.dense_args(), _l.stream_handle()))
    _intact(*st.bufs())
    ctx["s1"] = s1 = st.snapshot()
    st.inputs_unchanged()
    _check_apply(st, s0, s1, T.LR, "dfm_step_apply")
    st.lr.t.fill_(float(T.LR2))
    _l.check(lib.dfm_step_apply(*st.list_args(), *st.dense_args(), _l.stream_handle()))
    _intact(*st.bufs())
    _check_apply(st, s1, st.snapshot(), T.LR2, "second launch, new learning rate")


def _run_step_dense_apply(_l, lib, c, ctx):
    """The dense half alone (SGD: without a v buffer): the bits of dfm_step_apply's dense half, no table touched."""
    sd = ApplyState(_l, c, null_v=True)
    _l.check(lib.dfm_step_dense_apply(sd.clip.ptr() if sd.clip else None, C.byref(sd.opt), sd.step.ptr(), *sd.dense_args(),
                                      _l.stream_handle()))
    _intact(*sd.bufs())
    got = sd.snapshot()
    for k in ("p", "m", "v", "g"):
        if got[k] is not None:
            assert _bits_equal(got[k], ctx["s1"][k]), f"dfm_step_dense_apply: {k} differs from dfm_step_apply"
    _same_state(dict(got, p=None, m=None, v=None, g=None), ctx["s0"], "dfm_step_dense_apply touched a table")


def _run_step_apply_plan(_l, lib, c, ctx):
    """On the stream: the same update as dfm_step_apply (SGD: v NULL wherever the layout allows), and the plan of the
    next ids equal to dfm_rowplan_build's."""
    a = T.apply_inputs(c)
    S = a["S"]
    sp = ApplyState(_l, c, null_v=True)
    B, stride = c["batch"], a["ids_stride"]
    ids = torch.from_numpy(a["next_ids"]).cuda()
    vocab = torch.tensor(a["vocab"], dtype=torch.int32, device="cuda")
    fused, alone = Plan(S, B), Plan(S, B)
    _l.check(lib.dfm_step_apply_plan(*sp.list_args(), *sp.dense_args(), ids.data_ptr(), stride, vocab.data_ptr(),
                                     max(a["vocab"]), B, fused.sorted_pos.ptr(), fused.uniq.ptr(), fused.seg.ptr(),
                                     fused.num.ptr(), fused.err.ptr(), _l.stream_handle()))
    _intact(*sp.bufs(), *fused.bufs())
    assert int(fused.err.i[0]) == 0
    _same_state(sp.snapshot(), ctx["s1"], "dfm_step_apply_plan vs dfm_step_apply", skip_v=c["rule"] == "sgd")
    sp.inputs_unchanged()
    alone.build(_l, lib, ids, a["vocab"])
    assert T.apply_key_is_narrow(c) == (max(a["vocab"]) < (1 << 20) - 1)
    for (n1, u1, g1, p1), (n2, u2, g2, p2) in zip(fused.lists(), alone.lists()):
        assert n1 == n2 and np.array_equal(u1, u2) and np.array_equal(g1, g2) and np.array_equal(p1, p2), "the fused row plan"
    for s in range(S):            # ... against the ids themselves
        col = a["next_ids"][s, :min(B, CH)]
        want = np.unique(col[(col > 0) & (col < a["vocab"][s])])
        n1, u1, _, _ = fused.lists()[s]
        assert n1 == want.size and np.array_equal(u1, want)


APPLY_ENTRY = {"dfm_step_apply": _run_step_apply, "dfm_step_dense_apply": _run_step_dense_apply,
               "dfm_step_apply_plan": _run_step_apply_plan}


@pytest.mark.parametrize("idx", range(len(T.APPLY_CASES)), ids=lambda i: T.apply_case_id(T.APPLY_CASES[i]))
def test_apply(idx):
    """Every entry the case lists (tests/tail_cases.py::APPLY_ENTRIES; the CPU file asserts that every case of every
    rule lists all three), dfm_step_apply first: the others are held to its bits."""
    _l, lib = _libs()
    c = T.APPLY_CASES[idx]
    ctx = {}
    for entry in c["entries"]:
        APPLY_ENTRY[entry](_l, lib, c, ctx)
