"""The GEMM matrix on the GPU: every case of tests/gemm_cases.py through the C ABI on guarded buffers, against a float64
matmul of the same inputs on the device.  Each test asserts the route first (dfm_gemm_route / dfm_gemm_splits: the
functions dfm_gemm_f32 itself decides with), then bit-for-bit equality (integer family) or the bar (float family), then
the guards and the padding of every padded stride.  Inputs are drawn on the device."""
import ctypes as C

import pytest
import torch

from deepfm_amd import _lib
from tests import gemm_cases as GC
from tests.helpers import TOWER_SENTINEL, GuardedBuffer as G

pytestmark = pytest.mark.gpu

NAN = float("nan")
NAN_BITS = 0x7FC00000


def _gen(key: str):
    g = torch.Generator(device="cuda")
    g.manual_seed(GC.seed_of(key))
    return g


def dev_values(shape, family, gen):
    """The families of gemm_cases.values, drawn on the device."""
    if family == "float":
        return torch.randn(shape, device="cuda", generator=gen)
    v = torch.randint(-3, 3, shape, device="cuda", generator=gen)
    return torch.where(v >= 0, v + 1, v).float()


class Operand:
    """An (r, k) operand in a guarded buffer, K-contiguous (r rows of ld floats) or K-strided (k rows of ld floats).
    The padding of a padded leading dimension holds values of the family too: a fetch from it shows."""

    def __init__(self, r, k, kc, pad, shift, family, gen):
        outer, inner = (r, k) if kc else (k, r)
        self.ld = inner + pad
        self.buf = G(outer * self.ld, 0.0, shift)
        self.buf.t.copy_(dev_values((outer * self.ld,), family, gen))
        v = self.buf.view(outer, self.ld)[:, :inner]
        self.logical = v if kc else v.t()

    def ptr(self):
        return self.buf.ptr()


class Output:
    """A (rows, cols) result with row stride cols + pad: NaN everywhere but where `init` is given."""

    def __init__(self, rows, cols, pad=0, init=None):
        self.rows, self.cols, self.ld = rows, cols, cols + pad
        self.buf = G(rows * self.ld, NAN)
        if init is not None:
            self.buf.view(rows, self.ld)[:, :cols] = init

    def ptr(self):
        return self.buf.ptr()

    @property
    def value(self):
        return self.buf.view(self.rows, self.ld)[:, :self.cols]

    def assert_untouched_outside(self):
        assert self.buf.guards_intact(), "a float outside the buffer was written"
        pad = self.buf.view(self.rows, self.ld)[:, self.cols:]
        assert bool((pad.contiguous().view(torch.int32) == NAN_BITS).all()), "a padding column was written"


def _vec(n, family, gen):
    b = G(n, 0.0)
    b.t.copy_(dev_values((n,), family, gen))
    return b


def _check(got, want, A, n, c, family, what):
    """Integer family: the same bits as the (exact) float64 reference.  Float family: the bar of gemm_cases."""
    if family == "int":
        want = want.float()
        assert bool((want.abs() < 2 ** 24).all())
        assert torch.equal(got, want), f"{what}: {(got != want).sum().item()} of {got.numel()} elements differ"
        return
    err = (got.double() - want).abs()
    bar = c * GC.EPS32 * (float(n) ** 0.5) * A
    worst = (err / bar).max().item()
    print(f"{what}: worst |got - fp64| / bar = {worst:.3f} (n = {n}, C = {c})")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, f"{what}: {worst:.3f} x the bar"


# =====================================================================================================================
# dfm_gemm_f32
# =====================================================================================================================
def run_gemm(case: GC.Gemm, family: str):
    lib = _lib.load()
    gen = _gen(GC.input_key(case, family))
    m, n, k = case.m, case.n, case.k
    a = Operand(m, k, case.a_kc, case.a_pad, case.a_shift, family, gen)
    b = Operand(n, k, case.b_kc, case.b_pad, case.b_shift, family, gen)
    bias = _vec(n, family, gen)
    c0 = dev_values((m, n), family, gen) if case.acc else None
    out = Output(m, n, case.c_pad, c0)
    ws = G(max(lib.dfm_gemm_workspace_bytes(m, n, k) // 4, 4), NAN) if case.ws else None
    assert a.ld == case.lda and b.ld == case.ldb and out.ld == case.ldc
    got_route = lib.dfm_gemm_route(a.ptr(), a.ld, int(case.a_kc), b.ptr(), b.ld, int(case.b_kc), m, n, k, int(case.bias),
                                   int(case.ws))
    assert got_route == case.route, f"route {got_route}, the case is written for {case.route}"
    if case.route in (GC.TILED_SLOW, GC.TILED_FAST):
        assert lib.dfm_gemm_splits(m, n, k, int(case.ws)) == case.splits
    _lib.check(lib.dfm_gemm_f32(a.ptr(), a.ld, int(case.a_kc), b.ptr(), b.ld, int(case.b_kc), out.ptr(), out.ld, m, n, k,
                                bias.ptr() if case.bias else None, int(case.acc), ws.ptr() if ws else None,
                                _lib.stream_handle()))
    torch.cuda.synchronize()
    ad, bd = a.logical.double(), b.logical.double()
    want = ad @ bd.t()
    A = (ad.abs() @ bd.abs().t()) if family == "float" else None
    del ad, bd
    for t in ([bias.t] if case.bias else []) + ([c0] if case.acc else []):
        want += t.double()
        if A is not None:
            A += t.double().abs()
    _check(out.value, want, A, GC.chain_length(case), GC.C[case.kind], family, case.name)
    out.assert_untouched_outside()
    for buf in (a.buf, b.buf, bias) + ((ws,) if ws else ()):
        assert buf.guards_intact()
    return out.value.clone()


def _params(names, table):
    return [pytest.param(n, f, id=f"{n}-{f}") for n in names for f in table[n].families]


@pytest.mark.parametrize("name,family", _params(GC.ROWS_NAMES, GC.GEMM_CASES))
def test_rows_kernel(name, family):
    """gemm_rows_kernel<NT, K>: every instantiation in both weight layouts, the row counts that reach a second and a
    third tile per wave, padded strides, and the shapes that fall off the route (tiled, still exact)."""
    run_gemm(GC.GEMM_CASES[name], family)


@pytest.mark.parametrize("name,family", _params(GC.TILED_NAMES, GC.GEMM_CASES))
def test_tiled_kernel(name, family):
    """gemm_f32_kernel<A_KC, B_KC, FAST, FAST> at its tile and slice edges, its split reduction, and the weight-gradient
    product through dfm_gemm_f32's dispatch."""
    run_gemm(GC.GEMM_CASES[name], family)


@pytest.mark.parametrize("mn", [64, 40])
@pytest.mark.parametrize("k", list(GC.SPLIT_K))
def test_split_equals_one_split(mn, k):
    """Integer family: the slabs of a split reduction add up to the bits of the single pass."""
    split = run_gemm(GC.GEMM_CASES[f"tiled_split_MN{mn}_K{k}_ws"], "int")
    whole = run_gemm(GC.GEMM_CASES[f"tiled_split_MN{mn}_K{k}_nows"], "int")
    assert torch.equal(split, whole)


# =====================================================================================================================
# dfm_weight_grad_f32, its deferred forms
# =====================================================================================================================
class WGradRun:
    def __init__(self, case: GC.WGrad, family: str):
        self.case, self.family = case, family
        self.lib = _lib.load()
        gen = _gen(GC.input_key(case, family))
        M, n1, n2 = case.M, case.n1, case.n2
        self.g = Operand(M, n1, True, case.g_pad, 0, family, gen)        # (M, n1) rows of ldg floats
        self.x = Operand(M, n2, True, case.x_pad, 0, family, gen)
        self.dw0 = dev_values((n1, n2), family, gen) if case.acc else None
        self.db0 = dev_values((n1,), family, gen) if case.acc else None
        self.ws_floats = self.lib.dfm_weight_grad_workspace_bytes(M, n1, n2) // 4
        assert self.ws_floats == GC.wgrad_workspace_bytes(M, n1, n2) // 4 > 0
        self.blocks = self.lib.dfm_weight_grad_partial_blocks(M)

    def outputs(self):
        c = self.case
        dw = Output(c.n1, c.n2, c.dw_pad, self.dw0)
        db = Output(1, c.n1, 0, None if self.db0 is None else self.db0.view(1, -1))
        return dw, db, G(self.ws_floats, NAN)

    def direct(self):
        c = self.case
        dw, db, ws = self.outputs()
        _lib.check(self.lib.dfm_weight_grad_f32(self.g.ptr(), self.g.ld, self.x.ptr(), self.x.ld, c.M, c.n1, c.n2, dw.ptr(),
                                                dw.ld, db.ptr() if c.db else None, int(c.acc), ws.ptr(), _lib.stream_handle()))
        torch.cuda.synchronize()
        return dw, db, ws

    def deferred(self):
        c = self.case
        dw, db, ws = self.outputs()
        _lib.check(self.lib.dfm_weight_grad_partials_f32(self.g.ptr(), self.g.ld, self.x.ptr(), self.x.ld, c.M, c.n1, c.n2,
                                                         ws.ptr(), _lib.stream_handle()))
        job = _lib.PartialJob(0, self.blocks, c.n1, c.n2, int(c.acc), 0, ws.ptr(), dw.ptr(), db.ptr() if c.db else None, dw.ld)
        _lib.check(self.lib.dfm_partials_finish(C.byref(job), 1, _lib.stream_handle()))
        torch.cuda.synchronize()
        return dw, db, ws

    def check(self, dw, db, ws):
        c = self.case
        gd, xd = self.g.logical.double(), self.x.logical.double()
        n, cc = GC.chain_length(c), GC.C["wgrad"]
        want = gd.t() @ xd + (self.dw0.double() if c.acc else 0.0)
        A = gd.abs().t() @ xd.abs() if self.family == "float" else None
        _check(dw.value, want, A, n, cc, self.family, c.name + " dW")
        if c.db:
            want = gd.sum(0) + (self.db0.double() if c.acc else 0.0)
            _check(db.value[0], want, gd.abs().sum(0) if self.family == "float" else None, n, cc, self.family, c.name + " db")
        else:
            assert bool((db.value.contiguous().view(torch.int32) == NAN_BITS).all()), "db = NULL was written"
        dw.assert_untouched_outside()
        db.assert_untouched_outside()
        assert ws.guards_intact() and self.g.buf.guards_intact() and self.x.buf.guards_intact()


def _same_bits(a: Output, b: Output):
    return torch.equal(a.buf.whole.view(torch.int32), b.buf.whole.view(torch.int32))


@pytest.mark.parametrize("name,family", _params(list(GC.WGRAD_CASES), GC.WGRAD_CASES))
def test_weight_gradient(name, family):
    """gemm_wgrad_kernel<T1, T2> + its finish: the reference, two runs bitwise equal, and the deferred form
    (dfm_weight_grad_partials_f32 + dfm_partials_finish) bitwise equal to the direct call."""
    run = WGradRun(GC.WGRAD_CASES[name], family)
    first = run.direct()
    run.check(*first)
    again = run.direct()
    assert _same_bits(first[0], again[0]) and _same_bits(first[1], again[1])
    later = run.deferred()
    run.check(*later)
    assert _same_bits(first[0], later[0]) and _same_bits(first[1], later[1])
    assert torch.equal(first[2].t.view(torch.int32), later[2].t.view(torch.int32))      # the partials themselves


@pytest.mark.parametrize("family", ["int", "float"])
@pytest.mark.parametrize("M", [GC.M_BASE, 65569])
def test_pair_partials_equal_single_launches(M, family):
    """dfm_weight_grad_partials_pair_f32 on (192, 32) + (32, 64): each workspace float for float what the single launch
    leaves."""
    lib = _lib.load()
    gen = _gen(f"pair:{M}:{family}")
    (a1, a2), (b1, b2) = GC.WGRAD_PAIR
    ops = [Operand(M, w, True, p, 0, family, gen) for w, p in ((a1, 0), (a2, 4), (b1, 1), (b2, 0))]
    sizes = [lib.dfm_weight_grad_workspace_bytes(M, *s) // 4 for s in GC.WGRAD_PAIR]
    single = [G(s, NAN) for s in sizes]
    for (g, x), (n1, n2), ws in zip((ops[:2], ops[2:]), GC.WGRAD_PAIR, single):
        _lib.check(lib.dfm_weight_grad_partials_f32(g.ptr(), g.ld, x.ptr(), x.ld, M, n1, n2, ws.ptr(), _lib.stream_handle()))
    pair = [G(s, NAN) for s in sizes]
    _lib.check(lib.dfm_weight_grad_partials_pair_f32(ops[0].ptr(), ops[0].ld, ops[1].ptr(), ops[1].ld, a1, a2, pair[0].ptr(),
                                                     ops[2].ptr(), ops[2].ld, ops[3].ptr(), ops[3].ld, b1, b2, pair[1].ptr(),
                                                     M, _lib.stream_handle()))
    torch.cuda.synchronize()
    for s, p in zip(single, pair):
        assert not bool(torch.isnan(s.t).any())
        assert torch.equal(s.whole.view(torch.int32), p.whole.view(torch.int32))


@pytest.mark.parametrize("shapes", GC.PAIR_REFUSED)
def test_pair_refuses_other_shapes(shapes):
    lib = _lib.load()
    M = GC.M_BASE
    (a1, a2), (b1, b2) = shapes
    gen = _gen("refused")
    ops = [Operand(M, w, True, 0, 0, "int", gen) for w in (a1, a2, b1, b2)]
    ws = [G(lib.dfm_weight_grad_workspace_bytes(M, *s) // 4, TOWER_SENTINEL) for s in shapes]
    rc = lib.dfm_weight_grad_partials_pair_f32(ops[0].ptr(), a1, ops[1].ptr(), a2, a1, a2, ws[0].ptr(), ops[2].ptr(), b1,
                                               ops[3].ptr(), b2, b1, b2, ws[1].ptr(), M, _lib.stream_handle())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED
    for w in ws:
        assert bool((w.whole == TOWER_SENTINEL).all()), "a refused call wrote into its workspace"


# =====================================================================================================================
# dfm_partials_finish alone, on synthetic integer partials
# =====================================================================================================================
class FinishJob:
    """One job on integer partials with its exact expectation."""

    def __init__(self, kind, blocks, n1, n2, ld_pad, has_b, acc, gen):
        self.kind, self.has_b = kind, has_b
        width = n1 * n2 + n1 if kind == 0 else 2 * n1
        part = dev_values((blocks, width), "int", gen)
        self.partial = G(blocks * width, 0.0)
        self.partial.t.copy_(part.view(-1))
        total = part.double().sum(0)
        if kind == 0:
            w0 = dev_values((n1, n2), "int", gen) if acc else None
            b0 = dev_values((1, n1), "int", gen) if acc and has_b else None
            self.out_w, self.out_b = Output(n1, n2, ld_pad, w0), Output(1, n1, 0, b0)
            self.want_w = total[:n1 * n2].view(n1, n2) + (w0.double() if acc else 0.0)
            self.want_b = total[n1 * n2:].view(1, n1) + (b0.double() if b0 is not None else 0.0)
        else:                       # LayerNorm planes [blocks][2][D]: always added onto the outputs
            w0, b0 = dev_values((1, n1), "int", gen), dev_values((1, n1), "int", gen)
            self.out_w, self.out_b = Output(1, n1, 0, w0), Output(1, n1, 0, b0)
            self.want_w, self.want_b = total[:n1].view(1, n1) + w0.double(), total[n1:].view(1, n1) + b0.double()
        self.job = _lib.PartialJob(kind, blocks, n1, n2, int(acc), 0, self.partial.ptr(), self.out_w.ptr(),
                                   self.out_b.ptr() if has_b else None, self.out_w.ld)

    def check(self):
        assert torch.equal(self.out_w.value, self.want_w.float())
        if self.has_b:
            assert torch.equal(self.out_b.value, self.want_b.float())
        else:
            assert bool((self.out_b.value.contiguous().view(torch.int32) == NAN_BITS).all()), "out_b = NULL was written"
        self.out_w.assert_untouched_outside()
        self.out_b.assert_untouched_outside()
        assert self.partial.guards_intact()


def _finish(jobs):
    arr = (_lib.PartialJob * len(jobs))(*[j.job for j in jobs])
    _lib.check(_lib.load().dfm_partials_finish(arr, len(jobs), _lib.stream_handle()))
    torch.cuda.synchronize()
    for j in jobs:
        j.check()


@pytest.mark.parametrize("si", range(len(GC.FINISH_SHAPES)))
@pytest.mark.parametrize("bi", range(len(GC.FINISH_BLOCKS)))
def test_finish_weight_gradient_partials(bi, si):
    """wgrad_reduce_body: block counts around its strides of 32 and 4."""
    pad, has_b, acc = GC.finish_flags(si, bi)
    n1, n2 = GC.FINISH_SHAPES[si]
    _finish([FinishJob(0, GC.FINISH_BLOCKS[bi], n1, n2, pad, has_b, acc, _gen(f"finish0:{si}:{bi}"))])


@pytest.mark.parametrize("n1", GC.LN_FINISH_DIMS)
@pytest.mark.parametrize("blocks", GC.LN_FINISH_BLOCKS)
def test_finish_layernorm_partials(blocks, n1):
    """layernorm_finalize_body: block counts around its stride of 256, added onto nonzero outputs."""
    _finish([FinishJob(1, blocks, n1, 0, 0, True, True, _gen(f"finish1:{blocks}:{n1}"))])


def test_finish_mixed_jobs():
    """Eight jobs of alternating kind and size in one launch: the first_block search."""
    gen = _gen("finish:mixed")
    assert len(GC.MIXED_JOBS) == _lib.MAX_PARTIAL_JOBS
    _finish([FinishJob(*spec, gen) for spec in GC.MIXED_JOBS])


@pytest.mark.parametrize("count", [0, _lib.MAX_PARTIAL_JOBS + 1])
def test_finish_refuses_bad_count(count):
    gen = _gen("finish:count")
    jobs = [FinishJob(0, 3, 5, 3, 0, True, False, gen) for _ in range(_lib.MAX_PARTIAL_JOBS + 1)]
    arr = (_lib.PartialJob * len(jobs))(*[j.job for j in jobs])
    rc = _lib.load().dfm_partials_finish(arr, count, _lib.stream_handle())
    torch.cuda.synchronize()
    assert rc != 0
    for j in jobs:                      # nothing was launched: every output still NaN
        assert bool(torch.isnan(j.out_w.buf.t).all()) and bool(torch.isnan(j.out_b.buf.t).all())
