"""GPU: every kernel route, k-loop phase and tile edge of the DNN tower (csrc/tower.hip, csrc/gemm_core.h) against
plain fp64 restatements (tests/helpers.py), on buffers with guard floats around them and NaN-filled workspaces.
The cases live in tests/tower_cases.py; tests/test_cpu_tower_reference.py proves on the host that each reaches the
phase it claims and stays clear of the ReLU kink, so nothing is excluded from a comparison here.  Bars are the
project's: exact-fp32 GEMM outputs 1e-5 relative + 2e-6 of the scale; statistics and BatchNorm gradients 1e-4;
bf16 x 3 the assert_close defaults with the fp32 kernel beside it.  DESIGN.md section 2 maps instantiations to ids."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tower_cases as TC
from tests.helpers import (GuardedBuffer as G, assert_close, npy, tower_bn_backward_fp64, tower_bn_relu_fp64,
                           tower_column_stats_fp64, tower_dw_split_plan, tower_head_fp64, tower_linear_backward_fp64,
                           tower_linear_fp64, tower_masked_grad_fp64)

pytestmark = pytest.mark.gpu

GEMM = dict(rtol=1e-5, atol_scale=2e-6)          # exact-fp32 GEMM outputs: z, dx, dW, mean, logits, d logits
STAT = dict(rtol=1e-4)                           # rstd, running variance, d gamma, d beta, head dW (atol 1e-5 of scale)
ACT = dict(rtol=1e-4, atol_scale=2e-5)           # relu(bn(z)) and dz, as tests/test_gpu_fused_tower.py
NAN = float("nan")


def _id(c):
    return "-".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


@pytest.fixture
def tower_mode():
    """Set the tower's arithmetic mode explicitly for one test (whatever DFM_TEST_TOWER_MODE chose for the session)
    and restore the previous mode afterwards."""
    from deepfm_amd import _lib
    lib = _lib.load()
    before = lib.dfm_tower_get_mode()

    def set_mode(mode):
        assert lib.dfm_tower_set_mode(mode) == 0
        return _lib, lib
    try:
        yield set_mode
    finally:
        lib.dfm_tower_set_mode(before)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _intact(**bufs):
    torch.cuda.synchronize()
    for k, b in bufs.items():
        if b is not None:
            assert b.guards_intact(), f"{k}: a float outside the buffer was written"


class Bn:
    """A BatchNorm layer's backward context (struct dfm_bn_bwd) on guarded buffers: dy and the partial-sum workspace
    start as NaN, d gamma / d beta as 1.0."""

    def __init__(self, _l, lib, M, N, p=0.0, seed=None, salt=0, stats=True):
        self.M, self.N = M, N
        self.inp = TC.bn_inputs(M, N)
        self.z, self.gamma, self.beta = G.of(self.inp["z"]), G.of(self.inp["gamma"]), G.of(self.inp["beta"])
        self.stats = G.of(self.inp["stats"]) if stats else G(2 * N)
        self.fresh(_l, lib, p, seed, salt)

    def fresh(self, _l, lib, p=0.0, seed=None, salt=0):
        M, N = self.M, self.N
        self.dy, self.gg, self.gb = G(M * N), G(N, 1.0), G(N, 1.0)
        self.ws = G(lib.dfm_bn_bwd_workspace_bytes(M, N) // 4)
        c = _l.BnBwd()
        c.z, c.mean_rstd, c.gamma, c.beta = self.z.ptr(), self.stats.ptr(), self.gamma.ptr(), self.beta.ptr()
        c.dy, c.g_gamma, c.g_beta = self.dy.ptr(), self.gg.ptr(), self.gb.ptr()
        c.seed = seed.data_ptr() if seed is not None else None
        c.workspace, c.p_drop, c.salt = self.ws.ptr(), p, salt
        self.ctx = c
        return self

    def reference(self):
        mean, rstd = self.inp["stats"].astype(np.float64)
        return tower_bn_relu_fp64(self.inp["z"], mean, rstd, self.inp["gamma"], self.inp["beta"])   # xhat, y, a

    def check_apply(self, dz_got, dy_ref, what=""):
        xhat, _, _ = self.reference()
        dgamma, dbeta, dz = tower_bn_backward_fp64(dy_ref, xhat, self.inp["gamma"], self.inp["stats"][1])
        assert_close(npy(dz_got), dz.reshape(-1), what=what + "dz", **ACT)
        assert_close(npy(self.gg.t), 1.0 + dgamma, what=what + "1 + d gamma", **STAT)
        assert_close(npy(self.gb.t), 1.0 + dbeta, what=what + "1 + d beta", **STAT)

    def guards(self):
        return dict(dy=self.dy, g_gamma=self.gg, g_beta=self.gb, partials=self.ws, bn_stats=self.stats)


# =====================================================================================================================
# forward: dfm_linear_bn_forward, and its statistics workspace through dfm_bn_relu_dropout_apply
# =====================================================================================================================
def _merge_tiles_fp64(ws, M, N):
    """Column mean / biased variance from the [T][2][N] tile (mean, M2) workspace, in fp64."""
    T = (M + 31) // 32
    t = npy(ws)[:T * 2 * N].astype(np.float64).reshape(T, 2, N)
    cnt = np.array([min(32, M - 32 * i) for i in range(T)], dtype=np.float64)[:, None]
    mean = (cnt * t[:, 0]).sum(0) / M
    return mean, (t[:, 1] + cnt * (t[:, 0] - mean) ** 2).sum(0) / M


@pytest.mark.parametrize("case", TC.FWD_CASES, ids=_id)
def test_forward_and_statistics_vs_fp64(case, tower_mode):
    _l, lib = tower_mode(0)
    st = _l.stream_handle()
    M, N, K, variant, bias = case
    inp = TC.linear_inputs(M, N, K)
    ldx = K + {"ldx4": 4, "ldx1": 1}.get(variant, 0)
    xh = np.full((M, ldx), NAN, dtype=np.float32)          # the row padding must never reach a product
    xh[:, :K] = inp["x"]
    x, w, b = G.of(xh, shift=int(variant == "x_off")), G.of(inp["w"], shift=int(variant == "w_off")), G.of(inp["b"])
    assert (x.ptr() % 16 == 0) == (variant != "x_off") and (w.ptr() % 16 == 0) == (variant != "w_off")
    z, ws = G(M * N), G(lib.dfm_linear_bn_workspace_bytes(M, N) // 4)
    _l.check(lib.dfm_linear_bn_forward(x.ptr(), ldx, w.ptr(), b.ptr() if bias else None, M, N, K, z.ptr(), ws.ptr(), st))
    _intact(z=z, workspace=ws)
    z_ref = tower_linear_fp64(inp["x"], inp["w"], inp["b"] if bias else None)
    assert_close(npy(z.view(M, N)), z_ref, what="z", **GEMM)
    mean_ref, var_ref = tower_column_stats_fp64(z_ref)
    rstd_ref = 1.0 / np.sqrt(var_ref + TC.EPS)
    if N % 4:                      # the apply kernel wants float4 columns: merge the tile statistics on the host
        mean, var = _merge_tiles_fp64(ws.t, M, N)
        assert_close(mean, mean_ref, what="mean (tiles)", **GEMM)
        assert_close(1.0 / np.sqrt(var + TC.EPS), rstd_ref, what="rstd (tiles)", **STAT)
        return
    gamma, beta = G.of(inp["gamma"]), G.of(inp["beta"])
    stats, out, rm, rv = G(2 * N), G(M * N), G(N, 0.25), G(N, 2.0)
    nb = torch.tensor([7], dtype=torch.int64, device="cuda")
    _l.check(lib.dfm_bn_relu_dropout_apply(z.ptr(), M, N, ws.ptr(), gamma.ptr(), beta.ptr(), stats.ptr(), rm.ptr(),
                                           rv.ptr(), nb.data_ptr(), TC.MOMENTUM, TC.EPS, 0.0, None, 0, out.ptr(), st))
    _intact(z=z, workspace=ws, stats=stats, out=out, running_mean=rm, running_var=rv)
    assert int(nb) == 8
    got = npy(stats.view(2, N))
    assert_close(got[0], mean_ref, what="mean", **GEMM)
    assert_close(got[1], rstd_ref, what="rstd", **STAT)
    unb = var_ref * M / max(M - 1, 1)
    assert_close(npy(rm.t), 0.9 * 0.25 + 0.1 * mean_ref, what="running mean", **GEMM)
    assert_close(npy(rv.t), 0.9 * 2.0 + 0.1 * unb, what="running variance", **STAT)
    _, _, a_ref = tower_bn_relu_fp64(z_ref, mean_ref, rstd_ref, inp["gamma"], inp["beta"])
    assert_close(npy(out.view(M, N)), a_ref, what="relu(bn(z))", **ACT)


# =====================================================================================================================
# apply kernels: column tiles, row-lane merge trip counts, last tile's count
# =====================================================================================================================
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("M", TC.APPLY_M)
@pytest.mark.parametrize("N", TC.APPLY_N)
def test_forward_apply_vs_fp64(N, M, p, tower_mode):
    _l, lib = tower_mode(0)
    st = _l.stream_handle()
    K = 8
    inp = TC.linear_inputs(M, N, K)
    x, w, b, gamma, beta = (G.of(inp[k]) for k in ("x", "w", "b", "gamma", "beta"))
    z, ws = G(M * N), G(lib.dfm_linear_bn_workspace_bytes(M, N) // 4)
    stats, out, rm, rv = G(2 * N), G(M * N), G(N, 0.25), G(N, 2.0)
    nb = torch.tensor([0], dtype=torch.int64, device="cuda")
    seed = torch.tensor([20240607], dtype=torch.int64, device="cuda")
    _l.check(lib.dfm_linear_bn_forward(x.ptr(), K, w.ptr(), b.ptr(), M, N, K, z.ptr(), ws.ptr(), st))
    _l.check(lib.dfm_bn_relu_dropout_apply(z.ptr(), M, N, ws.ptr(), gamma.ptr(), beta.ptr(), stats.ptr(), rm.ptr(),
                                           rv.ptr(), nb.data_ptr(), TC.MOMENTUM, TC.EPS, p, seed.data_ptr(), 5,
                                           out.ptr(), st))
    _intact(z=z, workspace=ws, stats=stats, out=out, running_mean=rm, running_var=rv)
    assert int(nb) == 1
    z_ref = tower_linear_fp64(inp["x"], inp["w"], inp["b"])
    mean_ref, var_ref = tower_column_stats_fp64(z_ref)
    rstd_ref = 1.0 / np.sqrt(var_ref + TC.EPS)
    got = npy(stats.view(2, N))
    assert_close(got[0], mean_ref, what="mean", **GEMM)
    assert_close(got[1], rstd_ref, what="rstd", **STAT)
    assert_close(npy(rm.t), 0.9 * 0.25 + 0.1 * mean_ref, what="running mean", **GEMM)
    assert_close(npy(rv.t), 0.9 * 2.0 + 0.1 * var_ref * M / (M - 1), what="running variance", **STAT)
    _, _, a_ref = tower_bn_relu_fp64(z_ref, mean_ref, rstd_ref, inp["gamma"], inp["beta"])
    a = npy(out.view(M, N)).astype(np.float64)
    if p == 0.0:
        assert_close(a, a_ref, what="relu(bn(z))", **ACT)
    else:                      # as tests/test_gpu_fused_tower.py: keep rate inside its band, kept values / (1 - p)
        kept, on = a != 0, a_ref > 1e-3
        assert abs(float(kept[on].mean()) - (1 - p)) < 0.03 + 2.0 / (on.sum() ** 0.5 + 1)
        assert_close(a[kept], a_ref[kept] / (1 - p), what="kept values / (1 - p)", **ACT)


def _fm_struct(_l, inp, epi, keep):
    if not epi.startswith("fm"):
        return None
    f = _l.FmBwd()
    f.dim = 4
    if "g" in epi[3:]:
        g, S = G.of(inp["g_fm"]), G.of(inp["S"])
        keep += [g, S]
        f.g_fm, f.fm_sum = g.ptr(), S.ptr()
    if "a" in epi[3:]:
        a = G.of(inp["addend"])
        keep.append(a)
        f.addend = a.ptr()
    return f


class Backward:
    """One dfm_linear_backward launch of a case on fresh guarded buffers: slabs, dx (or dy + partial sums) NaN."""

    def __init__(self, _l, lib, M, N, K, epi, variant, parts):
        inp = TC.backward_inputs(M, N, K)
        self.M, self.N, self.K, self.epi, self.inp = M, N, K, epi, inp
        self.dz = G.of(inp["dz"], shift=int(variant == "dz_off"))
        self.x = G.of(inp["x"], shift=int(variant == "x_off"))
        self.w = G.of(inp["w"], shift=int(variant == "w_off"))
        self.keep = []
        self.splits = tower_dw_split_plan(N, K, M)[0]
        self.slabs = G(lib.dfm_linear_backward_workspace_bytes(M, N, K) // 4)
        self.gx = None if epi == "bn" else G(M * K)
        self.bn = Bn(_l, lib, M, K) if epi == "bn" else None
        fm = _fm_struct(_l, inp, epi, self.keep)
        if fm is not None and fm.g_fm:
            fm.e = self.x.ptr()
        _l.check(lib.dfm_linear_backward(self.dz.ptr(), M, N, self.x.ptr(), K, self.w.ptr(),
                                         self.gx.ptr() if self.gx else None, C.byref(self.bn.ctx) if self.bn else None,
                                         C.byref(fm) if fm is not None else None, parts, self.slabs.ptr(),
                                         _l.stream_handle()))
        g = dict(slabs=self.slabs, dx=self.gx)
        if self.bn:
            g.update(self.bn.guards())
        _intact(**g)

    def slab_floats(self):
        return self.slabs.t[:self.splits * self.N * self.K]

    def d_input(self):
        """What the d-input half wrote: dx, or the masked dy and its per-tile column sums."""
        if self.bn is None:
            return [self.gx.t]
        T = (self.M + 31) // 32
        return [self.bn.dy.t, self.bn.ws.t[:T * 2 * self.K]]

    def references(self):
        i = self.inp
        g = "g" in self.epi[3:] if self.epi.startswith("fm") else False
        a = "a" in self.epi[3:] if self.epi.startswith("fm") else False
        dW, dx = tower_linear_backward_fp64(i["dz"], i["x"], i["w"], i["g_fm"] if g else None, i["S"] if g else None,
                                            i["x"] if g else None, i["addend"] if a else None)
        if self.bn:
            dx = tower_masked_grad_fp64(dx, self.bn.reference()[1])
        return dW, dx

    def finish(self, _l, lib, fill=0.0):
        gw = G(self.N * self.K, fill)
        ref = _l.SlabRef()
        ref.workspace, ref.g_w, ref.batch = self.slabs.ptr(), gw.ptr(), self.M
        ref.out_features, ref.in_features = self.N, self.K
        _l.check(lib.dfm_linear_backward_finish(C.byref(ref), 1, _l.stream_handle()))
        _intact(g_w=gw, slabs=self.slabs)
        return npy(gw.view(self.N, self.K))


@pytest.mark.parametrize("M", TC.APPLY_M)
@pytest.mark.parametrize("N", TC.APPLY_N)
def test_bn_backward_apply_from_dx_partials_vs_fp64(N, M, tower_mode):
    """dfm_linear_backward's BatchNorm epilogue leaves dy and [T][2][N] column sums; dfm_bn_backward_apply merges them:
    d gamma / d beta added to 1.0, dz against fp64, and dz written over dy (aliasing) gives the same bits."""
    _l, lib = tower_mode(0)
    run = Backward(_l, lib, M, TC.APPLY_UP, N, "bn", "plain", 2)
    bn = run.bn
    _, dy_ref = run.references()
    assert_close(npy(bn.dy.view(M, N)), dy_ref, what="dy", **GEMM)
    dy_copy, ws_copy = bn.dy.t.clone(), bn.ws.t.clone()
    dz = G(M * N)
    _l.check(lib.dfm_bn_backward_apply(C.byref(bn.ctx), M, N, None, dz.ptr(), _l.stream_handle()))
    _intact(dz=dz, **bn.guards())
    assert _same_bits(bn.dy.t, dy_copy), "dy is an input of the apply launch"
    bn.check_apply(dz.t, dy_ref)
    first = dz.t.clone()
    bn.fresh(_l, lib)
    bn.dy.t.copy_(dy_copy)
    bn.ws.t.copy_(ws_copy)
    _l.check(lib.dfm_bn_backward_apply(C.byref(bn.ctx), M, N, None, bn.dy.ptr(), _l.stream_handle()))
    _intact(**bn.guards())
    assert _same_bits(bn.dy.t, first), "dz aliasing dy"


# =====================================================================================================================
# head: head_bce_kernel<1..8, false / true>, and the head flavour of bn_bwd_apply
# =====================================================================================================================
HEAD_CASES = [(ch, M) for ch in TC.HEAD_CH for M in TC.HEAD_M] + [(2, 512), (2, 513)]      # T = 16, 17 head partials


def _head_flags(ch, M):
    return TC.head_nulls(ch, M) if M in TC.HEAD_M else (True, True, True, M == 512, M == 513)


@pytest.mark.parametrize("ch,M", HEAD_CASES, ids=lambda v: str(v))
def test_head_and_its_backward_apply_vs_fp64(ch, M, tower_mode):
    _l, lib = tower_mode(0)
    st = _l.stream_handle()
    K = 32 * ch
    has_b, has_fo, has_fm, has_gb, has_gb2 = _head_flags(ch, M)
    bn = Bn(_l, lib, M, K)
    xhat, y, a_ref = bn.reference()
    a32 = a_ref.astype(np.float32)
    hi = TC.head_inputs(M, K)
    a, w, b, fo, fm, labels = (G.of(v) for v in (a32, hi["w"], hi["b"], hi["fo"], hi["fm"], hi["labels"]))
    logits, dl = G(M), G(M)
    _l.check(lib.dfm_head_bce(a.ptr(), M, K, w.ptr(), b.ptr() if has_b else None, fo.ptr() if has_fo else None,
                              fm.ptr() if has_fm else None, labels.ptr(), logits.ptr(), dl.ptr(), C.byref(bn.ctx), st))
    _intact(logits=logits, d_logits=dl, **bn.guards())
    ref = tower_head_fp64(a32, hi["w"], hi["b"] if has_b else None, hi["fo"] if has_fo else None,
                          hi["fm"] if has_fm else None, hi["labels"])
    if (has_fo or has_fm) and M >= 31:
        assert (ref["logits"] > 20).any() and (ref["logits"] < -20).any()
    assert_close(npy(logits.t), ref["logits"], what="logits", **GEMM)
    assert_close(npy(dl.t), ref["dlogits"], what="d logits", **GEMM)
    dy_ref = tower_masked_grad_fp64(ref["dlogits"][:, None] * hi["w"].astype(np.float64)[None, :], y)
    assert_close(npy(bn.dy.view(M, K)), dy_ref, what="dy", **GEMM)
    gw, gb, gb2, loss, dz = G(K, 1.0), G(1, 1.0), G(1, 1.0), G(1), G(M * K)
    tail = _l.HeadTail()
    tail.g_w, tail.loss = gw.ptr(), loss.ptr()
    tail.g_b, tail.g_b2 = gb.ptr() if has_gb else None, gb2.ptr() if has_gb2 else None
    _l.check(lib.dfm_bn_backward_apply(C.byref(bn.ctx), M, K, C.byref(tail), dz.ptr(), st))
    _intact(g_w=gw, g_b=gb, g_b2=gb2, loss=loss, dz=dz, **bn.guards())
    bn.check_apply(dz.t, dy_ref)
    assert_close(npy(gw.t), 1.0 + ref["dw"], what="1 + d head weight", **STAT)
    for name, buf, used in (("d b", gb, has_gb), ("d b2", gb2, has_gb2)):
        want = 1.0 + ref["db"] if used else 1.0
        assert abs(float(buf.t[0]) - want) <= 1e-4 * abs(want) + 1e-5 * abs(want), (name, float(buf.t[0]), want)
    # mean BCE: 1e-6 absolute as tests/test_gpu_fused_tower.py, relative once a |logit| > 20 row lifts the loss over 1
    assert abs(float(loss.t[0]) - ref["loss"]) < 1e-6 * max(1.0, abs(ref["loss"])), (float(loss.t[0]), ref["loss"])


@pytest.mark.parametrize("ch,M", [(ch, M) for ch in TC.HEAD_CH for M in TC.HEAD_M], ids=lambda v: str(v))
def test_fused_head_is_bitwise_the_two_launches(ch, M, tower_mode):
    """dfm_head_bn_bce against dfm_bn_relu_dropout_apply + dfm_head_bce at all eight widths: statistics, running
    statistics, counter, logits, d logits, dy and the workgroup partials, bit for bit."""
    _l, lib = tower_mode(0)
    st = _l.stream_handle()
    K, Kin = 32 * ch, 8
    p = 0.25 if ch % 2 else 0.0
    has_b, has_fo, has_fm, _, _ = TC.head_nulls(ch, M)
    inp, hi = TC.linear_inputs(M, K, Kin), TC.head_inputs(M, K)
    x, w, bias, gamma, beta = (G.of(inp[k]) for k in ("x", "w", "b", "gamma", "beta"))
    hw, hb, fo, fm, labels = (G.of(hi[k]) for k in ("w", "b", "fo", "fm", "labels"))
    seed = torch.tensor([987654321], dtype=torch.int64, device="cuda")
    z, wsf = G(M * K), G(lib.dfm_linear_bn_workspace_bytes(M, K) // 4)
    _l.check(lib.dfm_linear_bn_forward(x.ptr(), Kin, w.ptr(), bias.ptr(), M, K, Kin, z.ptr(), wsf.ptr(), st))

    def run(fused):
        r = dict(stats=G(2 * K), rm=G(K, 0.25), rv=G(K, 2.0), logits=G(M), dl=G(M), dy=G(M * K), gg=G(K, 0.0),
                 gb=G(K, 0.0), ws=G(lib.dfm_bn_bwd_workspace_bytes(M, K) // 4))
        nb = torch.tensor([7], dtype=torch.int64, device="cuda")
        c = _l.BnBwd()
        c.z, c.mean_rstd, c.gamma, c.beta = z.ptr(), r["stats"].ptr(), gamma.ptr(), beta.ptr()
        c.dy, c.g_gamma, c.g_beta, c.seed = r["dy"].ptr(), r["gg"].ptr(), r["gb"].ptr(), seed.data_ptr()
        c.workspace, c.p_drop, c.salt = r["ws"].ptr(), p, 2
        opt = (hb.ptr() if has_b else None, fo.ptr() if has_fo else None, fm.ptr() if has_fm else None)
        if fused:
            _l.check(lib.dfm_head_bn_bce(wsf.ptr(), r["stats"].ptr(), r["rm"].ptr(), r["rv"].ptr(), nb.data_ptr(),
                                         TC.MOMENTUM, TC.EPS, M, K, hw.ptr(), *opt, labels.ptr(), r["logits"].ptr(),
                                         r["dl"].ptr(), C.byref(c), st))
        else:
            a = G(M * K)
            _l.check(lib.dfm_bn_relu_dropout_apply(z.ptr(), M, K, wsf.ptr(), gamma.ptr(), beta.ptr(), r["stats"].ptr(),
                                                   r["rm"].ptr(), r["rv"].ptr(), nb.data_ptr(), TC.MOMENTUM, TC.EPS, p,
                                                   seed.data_ptr(), 2, a.ptr(), st))
            _l.check(lib.dfm_head_bce(a.ptr(), M, K, hw.ptr(), *opt, labels.ptr(), r["logits"].ptr(), r["dl"].ptr(),
                                      C.byref(c), st))
            _intact(a=a)
        _intact(**r)
        assert int(nb) == 8
        return r

    two, one = run(False), run(True)
    blocks = (M + 31) // 32
    for k in two:
        a, b = two[k].t, one[k].t
        if k == "ws":
            a, b = a[:blocks * (3 * K + 4)], b[:blocks * (3 * K + 4)]
        assert _same_bits(a, b), k
        if k != "ws":
            assert bool(torch.isfinite(b).all()), f"{k}: not fully written"
    assert bool(torch.isfinite(one["ws"].t[:blocks * (3 * K + 4)]).all())


# =====================================================================================================================
# backward, mode 0: linear_bwd_kernel<FAST, EPI> — both products, block map, parts, slabs
# =====================================================================================================================
@pytest.mark.parametrize("case", TC.BWD_CASES, ids=_id)
def test_backward_vs_fp64(case, tower_mode):
    _l, lib = tower_mode(0)
    M, N, K, epi, variant, _ = case
    both = Backward(_l, lib, M, N, K, epi, variant, 3)
    dW_ref, dx_ref = both.references()
    slabs = npy(both.slab_floats()).astype(np.float64).reshape(both.splits, N, K)
    assert np.isfinite(slabs).all(), "a slab element was not written"
    assert_close(slabs.sum(0), dW_ref, what="dW (slabs summed in fp64)", **GEMM)
    if (N * K) % 4 == 0:
        assert_close(both.finish(_l, lib), dW_ref, what="dW", **GEMM)
    got = npy(both.d_input()[0]).reshape(M, K)
    assert_close(got, dx_ref, what="dy" if epi == "bn" else "dx", **GEMM)
    if epi == "bn" and K % 4 == 0:
        dz = G(M * K)
        _l.check(lib.dfm_bn_backward_apply(C.byref(both.bn.ctx), M, K, None, dz.ptr(), _l.stream_handle()))
        _intact(dz=dz, **both.bn.guards())
        both.bn.check_apply(dz.t, dx_ref)
    # parts: the two halves launched alone give the same bits as the launch that carries both
    only_dw, only_dx = Backward(_l, lib, M, N, K, epi, variant, 1), Backward(_l, lib, M, N, K, epi, variant, 2)
    assert _same_bits(only_dw.slab_floats(), both.slab_floats()), "parts = 1 against parts = 3"
    for a, b in zip(only_dx.d_input(), both.d_input()):
        assert _same_bits(a, b), "parts = 2 against parts = 3"
    for t in only_dw.d_input():
        assert bool(torch.isnan(t).all()), "parts = 1 wrote a d-input value"
    assert bool(torch.isnan(only_dx.slabs.t).all()), "parts = 2 wrote a slab"


# =====================================================================================================================
# dfm_linear_backward_finish: slab_reduce_kernel
# =====================================================================================================================
def _linear1_slabs(_l, lib, s, K, tag):
    """s slabs of a one-output Linear's weight gradient (M = 64 s - 3 rows) and their fp64 sum."""
    M = 64 * s - 3
    assert lib.dfm_linear1_backward_splits(M) == s
    r = np.random.default_rng([5, s, K, tag])
    g, x, w = (r.standard_normal(n).astype(np.float32) for n in (M, (M, K), K))
    gb, xb, wb, gx, ws = G.of(g), G.of(x), G.of(w), G(M * K), G(s * K)
    _l.check(lib.dfm_linear1_backward(gb.ptr(), xb.ptr(), M, K, wb.ptr(), gx.ptr(), ws.ptr(), _l.stream_handle()))
    _intact(g_x=gx, slabs=ws)
    ref = _l.SlabRef()
    ref.workspace, ref.batch, ref.out_features, ref.in_features, ref.splits = ws.ptr(), 1, 1, K, s
    return ref, ws, g.astype(np.float64) @ x.astype(np.float64)


@pytest.mark.parametrize("s", TC.FINISH_SPLITS)
def test_finish_split_counts_vs_fp64(s, tower_mode):
    _l, lib = tower_mode(0)
    K = 200                                     # 50 float4: one partly filled workgroup
    ref, ws, want = _linear1_slabs(_l, lib, s, K, 0)
    gw = G(K, 1.0)
    ref.g_w = gw.ptr()
    _l.check(lib.dfm_linear_backward_finish(C.byref(ref), 1, _l.stream_handle()))
    _intact(g_w=gw, slabs=ws)
    assert_close(npy(gw.t), 1.0 + want, what="1 + dW", **GEMM)


def test_finish_three_refs_in_one_launch(tower_mode):
    """Three references of different sizes and split counts in one call (the first_block search; a 257-float4 entry
    that spills one float4 into a second workgroup comes first): against fp64 and bit for bit against single calls."""
    _l, lib = tower_mode(0)
    st = _l.stream_handle()
    run = Backward(_l, lib, *TC.FINISH_TOWER_SHAPE, "plain", "plain", 1)     # 4 x 257: 257 float4, the tower's own 2 splits
    r1, ws1, want1 = _linear1_slabs(_l, lib, 9, 200, 1)                      # 50 float4, 8 + 1 splits
    r2, ws2, want2 = _linear1_slabs(_l, lib, 17, 96, 2)                      # 24 float4, 8 + 8 + 1 splits
    M, N, K = TC.FINISH_TOWER_SHAPE
    assert run.splits == 2 and (N * K) // 4 == 257
    want0 = run.references()[0].reshape(-1)
    sizes = (N * K, 200, 96)
    fields = ("workspace", "batch", "out_features", "in_features", "splits")
    refs = (_l.SlabRef * 3)()
    refs[0].workspace, refs[0].batch, refs[0].out_features, refs[0].in_features = run.slabs.ptr(), M, N, K
    for i, src in ((1, r1), (2, r2)):
        for f in fields:
            setattr(refs[i], f, getattr(src, f))
    singles, together = [G(n, 0.5) for n in sizes], [G(n, 0.5) for n in sizes]
    for i in range(3):
        refs[i].g_w = together[i].ptr()
    _l.check(lib.dfm_linear_backward_finish(refs, 3, st))
    for i in range(3):
        one = (_l.SlabRef * 1)()
        for f in fields:
            setattr(one[0], f, getattr(refs[i], f))
        one[0].g_w = singles[i].ptr()
        _l.check(lib.dfm_linear_backward_finish(one, 1, st))
    _intact(**{f"g_w{i}": b for i, b in enumerate(singles + together)})
    for i, want in enumerate((want0, want1, want2)):
        assert _same_bits(singles[i].t, together[i].t), f"reference {i}: one launch against its own launch"
        assert_close(npy(together[i].t), 0.5 + want, what=f"reference {i}", **GEMM)


# =====================================================================================================================
# mode 1: bf16 x 3 backward (linear_bwd_kernel<true, EPI, true>) and its fallbacks
# =====================================================================================================================
def _both_modes(tower_mode, M, N, K, epi, variant):
    runs = []
    for mode in (0, 1):
        _l, lib = tower_mode(mode)
        assert lib.dfm_tower_get_mode() == mode
        run = Backward(_l, lib, M, N, K, epi, variant, 3)
        runs.append((run, run.finish(_l, lib)))
    return runs


@pytest.mark.parametrize("case", TC.X3_CASES, ids=_id)
def test_bf16x3_backward_vs_fp64(case, tower_mode):
    M, N, K, epi = case
    (r0, gw0), (r1, gw1) = _both_modes(tower_mode, M, N, K, epi, "plain")
    dW_ref, dx_ref = r0.references()
    for mode, run, gw in ((0, r0, gw0), (1, r1, gw1)):            # the fp32 kernel beside it, held to the same bar
        assert_close(gw, dW_ref, what=f"dW mode {mode}")
        assert_close(npy(run.d_input()[0]).reshape(M, K), dx_ref, what=f"d input mode {mode}")
    assert not _same_bits(r0.slab_floats(), r1.slab_floats()), "mode 1 ran the fp32 kernel"
    if epi == "bn":
        dz = G(M * K)
        _l, lib = tower_mode(1)
        _l.check(lib.dfm_bn_backward_apply(C.byref(r1.bn.ctx), M, K, None, dz.ptr(), _l.stream_handle()))
        _intact(dz=dz, **r1.bn.guards())
        r1.bn.check_apply(dz.t, dx_ref, what="mode 1 ")


@pytest.mark.parametrize("case", TC.X3_FALLBACK, ids=_id)
def test_bf16x3_fallback_is_the_fp32_kernel(case, tower_mode):
    """out_features % 8 != 0, an odd batch, a misaligned operand: mode 1 must run the fp32 kernels, bit for bit."""
    M, N, K, variant = case
    (r0, gw0), (r1, gw1) = _both_modes(tower_mode, M, N, K, "plain", variant)
    assert _same_bits(r0.slab_floats(), r1.slab_floats()) and _same_bits(r0.gx.t, r1.gx.t)
    assert np.array_equal(gw0, gw1)
    dW_ref, dx_ref = r0.references()
    assert_close(gw1, dW_ref, what="dW", **GEMM)
    assert_close(npy(r1.gx.view(M, K)), dx_ref, what="dx", **GEMM)
