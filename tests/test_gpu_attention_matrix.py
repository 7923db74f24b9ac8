"""GPU parity of field self-attention over every kernel instantiation and tile edge, against an fp64 reference.

The attention kernels are template families (csrc/attention_mfma.hip, attention_core.hip, attention.hip).
``MATRIX`` below launches every instantiation at least once, and every case first asserts — with the library's
own predicates — that the module takes the route the case is meant for:

=============  ==============================================  ==============================================
route          kernels                                         grid
=============  ==============================================  ==============================================
whole_block    attn_block_mfma_fwd / _bwd<NT, KD, RES>          F in {1,15,16,17,32,33,47,48} x D in {16,32,48,64}
                                                                x residual: all 24 + 24 instantiations
qkv_inside     attn_qkv_mfma_fwd / _bwd<NT, KD>                 heads in {1,2,8} x F in {1,16,17,32,33,48}, D cycled so
                                                                that all 12 (NT, KD) occur; + 4 heads, block kernel off
mfma_core      attn_mfma_fwd / _bwd<NT> behind the GEMM         D in {8,20,40,60}, F in {1,15,16,17,32,33,48}: NT 1, 2, 3
                                                                each at both of its edges
vector_core    attn_core_fwd / _bwd<HD>                         HD 4, 8, 32 at F in {1,2,39,63,64}; HD 16 at F in {49,63,64}
per_sample     attn_fwd_kernel / attn_bwd_kernel                F in {65,100}, B = 1, head_dim 12, and a block-kernel
                                                                shape with ``gemm_path = False``
=============  ==============================================  ==============================================

The reference is ``tests.helpers.attention_fp64`` (torch CPU float64, autograd gradients; nothing from oracle/).
The bar is ``assert_close`` unchanged (rtol 1e-4, floor 1e-5 x tensor scale).  ``W_k.bias`` has an exactly zero
gradient (softmax is shift-invariant): it keeps the absolute floor 1e-4 of the existing small-batch tests and the
fp64 value is asserted below 1e-12 so that the floor can never hide a real gradient.  (At F = 1 the softmax is the
constant 1 and d W_q, d W_k are identically zero as well; the kernels return exact zeros there — p = 1 and
dP - sum(dP o P) = 0 without rounding — and the unchanged bar holds them to that.)

Batches are 3...9 samples.  Wherever the head count allows it (heads % 4 != 0) ``B * heads % 4 != 0``: the last
four-wave workgroup is partly empty.  With 4 or 8 heads that is impossible; the whole-block kernel has one
workgroup per sample and no such tail.  Of the cases on the three routes that pack four (sample, head) units into
a workgroup, more than half end in a partly empty one (asserted in tests/test_cpu_attention_reference.py).

tests/test_cpu_attention_reference.py ties this file's reference to the attention goldens and to the oracle on the
CPU, and checks there that ``MATRIX`` covers every instantiation.
"""
import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests.helpers import (assert_close, attention_block_fp64, attention_case_inputs, attention_core_fp64,
                           attention_fp64, error_ratio, npy)

pytestmark = pytest.mark.gpu

WKB_FLOOR = 1e-4          # absolute floor of the W_k.bias gradient (identically zero), as in test_gpu_attention.py


def _case(F, D, heads, A, B, residual=True, layers=1):
    return dict(B=B, F=F, D=D, heads=heads, A=A, layers=layers, residual=residual)


def _batch(heads, i):
    """3...9 samples, varied by ``i``; B * heads % 4 != 0 wherever some B allows it."""
    for k in range(7):
        B = 3 + (i + k) % 7
        if heads % 4 == 0 or (B * heads) % 4 != 0:
            return B
    raise AssertionError("unreachable")


def _matrix():
    m = []
    # ---- the whole block in one kernel: 4 heads of 16; all (NT, KD, RES) -------------------------------------
    for F in (1, 15, 16, 17, 32, 33, 47, 48):
        for D in (16, 32, 48, 64):
            for res in (True, False):
                m.append((_case(F, D, 4, 64, _batch(4, F + D // 16), res), "whole_block"))
    # ---- projection inside the matrix-core kernel: heads != 4 (or the block kernel switched off) --------------
    for nt, fs in enumerate(((1, 16), (17, 32), (33, 48))):
        i = nt                                  # D cycles inside a tile count: 6 cases, all four KD
        for F in fs:
            for heads in (1, 2, 8):
                m.append((_case(F, 16 * (1 + i % 4), heads, 16 * heads, _batch(heads, i), i % 2 == 0), "qkv_inside"))
                i += 1
    for F, D in ((17, 32), (48, 64), (1, 48), (33, 16)):
        m.append((_case(F, D, 4, 64, _batch(4, F), F != 48), "qkv_inside"))
    # ---- projection GEMM + matrix-core kernel: embed_dim not a multiple of 16 --------------------------------
    for i, F in enumerate((1, 15, 16, 17, 32, 33, 48)):
        heads = (1, 2, 3, 4)[i % 4]
        m.append((_case(F, (8, 20, 40, 60)[i % 4], heads, 16 * heads, _batch(heads, i), i % 3 != 1), "mfma_core"))
    # ---- projection GEMM + vector core ------------------------------------------------------------------------
    i = 0
    for hd, fs in ((4, (1, 2, 39, 63, 64)), (8, (1, 2, 39, 63, 64)), (32, (1, 2, 39, 63, 64)), (16, (49, 63, 64))):
        for F in fs:
            heads = (1, 2, 3)[i % 3]
            m.append((_case(F, (8, 32, 20, 64, 16)[i % 5], heads, hd * heads, _batch(heads, i), i % 4 != 3),
                      "vector_core"))
            i += 1
    # ---- the per-sample LDS kernel ----------------------------------------------------------------------------
    m.append((_case(65, 16, 4, 32, 5), "per_sample"))                       # F > 64
    m.append((_case(100, 8, 2, 16, 3, residual=False), "per_sample"))
    m.append((_case(23, 10, 3, 36, 1), "per_sample"))                       # B = 1, head_dim 12, embed_dim % 4 != 0
    m.append((_case(64, 24, 2, 24, 7), "per_sample"))                       # head_dim 12 with F <= 64
    m.append((_case(33, 32, 4, 64, _batch(4, 33 + 2)), "per_sample_forced"))  # the whole_block case's inputs
    # ---- two layers: the second block's input is a kernel output ----------------------------------------------
    m.append((_case(33, 32, 4, 64, 6, layers=2), "whole_block"))
    m.append((_case(17, 48, 2, 32, 7, layers=2), "qkv_inside"))
    m.append((_case(32, 40, 2, 32, 5, layers=2), "mfma_core"))
    return m


MATRIX = _matrix()


def case_id(entry):
    c, path = entry
    return (f"{path}-F{c['F']}-D{c['D']}-h{c['heads']}-A{c['A']}-B{c['B']}"
            f"{'' if c['residual'] else '-nores'}{'-2layers' if c['layers'] == 2 else ''}")


# one shape per route, at the largest F of the route: the property tests and the sharp-softmax test
PER_ROUTE = [
    (_case(48, 32, 4, 64, 6), "whole_block"),
    (_case(48, 64, 2, 32, 5), "qkv_inside"),
    (_case(48, 40, 3, 48, 5), "mfma_core"),
    (_case(64, 32, 3, 48, 5), "vector_core"),
    (_case(100, 8, 2, 16, 3), "per_sample"),
]


def expected_route(lib, c, gemm_path, whole_block_kernel):
    """The dispatch of models/layers/attention.py restated on the library's predicates."""
    F, D, A, H = c["F"], c["D"], c["A"], c["heads"]
    core = bool(lib.dfm_attention_core_supported(F, A, H))
    inside = bool(lib.dfm_attention_qkv_core_supported(F, D, A, H))
    block = bool(lib.dfm_attention_block_supported(F, D, A, H))
    assert not block or inside, "the block kernel implies the projection-inside kernel"
    assert not inside or core, "the projection-inside kernel implies the core"
    if not (gemm_path and core and D % 4 == 0 and A % 4 == 0 and D <= 64):
        return "per_sample"
    if whole_block_kernel and block:
        return "whole_block"
    if inside:
        return "qkv_inside"
    return "mfma_core" if (A // H == 16 and F <= 48) else "vector_core"      # attn_mfma_supported


def _module(c, params, path):
    from deepfm_amd import _lib
    from deepfm_amd.models.layers.attention import MultiHeadSelfAttention, block_route
    att = MultiHeadSelfAttention(c["D"], c["heads"], c["A"], c["layers"], c["residual"])
    assert sorted(att.state_dict().keys()) == sorted(params.keys())
    att.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    for blk in att.layers:
        assert blk.gemm_path is True and blk.whole_block_kernel is True            # the switches' defaults
        if path == "per_sample_forced":
            blk.gemm_path = False
        if path == "qkv_inside" and c["heads"] == 4:
            blk.whole_block_kernel = False
        route = expected_route(_lib.load(), c, blk.gemm_path, blk.whole_block_kernel)
        assert route == path.replace("_forced", ""), f"case meant for {path} would run on {route}"
        assert block_route(blk, c["F"]) == ("gemm_core" if route in ("mfma_core", "vector_core") else route)
    if path == "per_sample_forced":                     # ... at a shape the block kernel runs when left alone
        assert expected_route(_lib.load(), c, True, True) == "whole_block"
    return att.cuda()


def _run(att, x, up):
    att.zero_grad(set_to_none=True)
    t = torch.from_numpy(x).cuda().requires_grad_()
    out = att(t)
    assert out.shape == t.shape
    (out * torch.from_numpy(up).cuda()).sum().backward()
    grads = {}
    for k, p in att.named_parameters():
        assert p.grad is not None, k
        grads[k] = npy(p.grad)
    return npy(out), npy(t.grad), grads


def _floor(k):
    return WKB_FLOOR if k.endswith("W_k.bias") else 0.0


def _check_vs_fp64(got, ref, what=""):
    out, d_x, grads = got
    r_out, r_dx, r_grads = ref
    assert_close(out, r_out, what=what + "out")
    assert_close(d_x, r_dx, what=what + "d_x")
    assert sorted(grads) == sorted(r_grads)
    for k in grads:
        if k.endswith("W_k.bias"):
            assert float(np.abs(r_grads[k]).max()) < 1e-12, f"{k}: the fp64 gradient is not zero"
        assert_close(grads[k], r_grads[k], what=what + k, floor=_floor(k))


@pytest.mark.parametrize("entry", MATRIX, ids=case_id)
def test_instantiation_matrix_vs_fp64(entry):
    """out, d_x and every parameter gradient of the module against the fp64 reference, on the asserted route."""
    c, path = entry
    params, x, up = attention_case_inputs(c)
    att = _module(c, params, path)
    ref = attention_fp64(x, params, c["heads"], c["layers"], c["residual"], up)
    _check_vs_fp64(_run(att, x, up), ref)


SHARP_MARGIN = 4.0


@pytest.mark.parametrize("entry", PER_ROUTE, ids=case_id)
def test_sharp_softmax_vs_fp64(entry):
    """x scaled by 6: scores reach the hundreds and the softmax is near one-hot, so a missing max subtraction
    overflows.  Everything must be finite.  The function is ill-conditioned here — the fp32 oracle itself misses the
    project bar against fp64 (by up to about 3.2x on W_q / W_k gradients on the CPU) — so the bar is set per tensor
    from the ORACLE's worst error-to-bound ratio r against fp64, never from the kernel's output: the kernel is held
    to max(1, SHARP_MARGIN * r) times the project bar.  The margin 4 covers a different summation order over the
    same fp32 arithmetic.

    Worst error / project bar per shape as printed by a run on the MI355X (oracle: tensor | kernel: tensor):
      whole_block  F48 D32 h4:  oracle 0.656 W_k.weight | kernel 0.547 W_q.weight
      qkv_inside   F48 D64 h2:  oracle 4.607 d_x, 3.183 W_k.weight, 2.158 W_q.weight, 1.266 out
                                | kernel 1.443 d_x, 1.406 W_q.weight, 1.174 W_k.weight, 0.986 out
      mfma_core    F48 D40 h3:  oracle 0.718 W_q.bias   | kernel 0.386 W_k.weight
      vector_core  F64 D32 h3:  oracle 0.855 W_k.weight | kernel 1.029 W_q.weight (oracle 0.684 there: 2.735 allowed)
      per_sample   F100 D8 h2:  oracle 0.093 W_k.weight | kernel 0.145 W_q.weight
    The kernels mostly sit below the oracle; where a kernel is past the project bar it is at most 1.5x the oracle's
    ratio on that tensor and uses at most 0.38 of what it is allowed.  Margin kept: 4, as first set.
    """
    c, path = entry
    params, x, up = attention_case_inputs(c, x_scale=6.0)
    att = _module(c, params, path)
    out, d_x, grads = _run(att, x, up)
    r_out, r_dx, r_grads = attention_fp64(x, params, c["heads"], c["layers"], c["residual"], up)
    o_out = O.attention_forward(x, params, c["heads"], c["layers"], c["residual"])
    o_dx, o_grads = O.attention_backward(x, params, c["heads"], c["layers"], c["residual"], up)
    rows = [("out", out, o_out, r_out, 0.0), ("d_x", d_x, o_dx, r_dx, 0.0)]
    rows += [(k, grads[k], o_grads[k], r_grads[k], _floor(k)) for k in sorted(grads)]
    failures = []
    for name, got, orc, ref, floor in rows:
        assert np.isfinite(got).all(), f"{name}: not finite"
        kr, orr = error_ratio(got, ref, floor=floor), error_ratio(orc, ref, floor=floor)
        allowed = max(1.0, SHARP_MARGIN * orr)
        print(f"sharp {case_id(entry)} {name}: kernel {kr:.3f} oracle {orr:.3f} allowed {allowed:.3f}")
        if not kr <= allowed:
            failures.append(f"{name}: kernel {kr:.3f} x bar, oracle {orr:.3f} x bar, allowed {allowed:.3f}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("entry", PER_ROUTE, ids=case_id)
def test_sample_zero_is_batch_invariant_bitwise(entry):
    """Sample 0 alone (B = 1) and as sample 0 of the batch: the same bits in out and d_x (cross-wave LDS overlap
    or a wrong unit index would show here)."""
    c, path = entry
    params, x, up = attention_case_inputs(c)
    att = _module(c, params, path)
    out, d_x, _ = _run(att, x, up)
    out1, d_x1, _ = _run(att, x[:1].copy(), up[:1].copy())
    assert np.array_equal(out[:1], out1), "out of sample 0 depends on the batch"
    assert np.array_equal(d_x[:1], d_x1), "d_x of sample 0 depends on the batch"


@pytest.mark.parametrize("entry", PER_ROUTE, ids=case_id)
def test_two_runs_are_bitwise_equal(entry):
    c, path = entry
    params, x, up = attention_case_inputs(c)
    att = _module(c, params, path)
    a, b = _run(att, x, up), _run(att, x, up)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k


# ---- the C ABI directly, outputs carved out of NaN-filled buffers ------------------------------------------------

GUARD = 64          # floats on each side of an output (256 bytes: the carved pointer stays 16-byte aligned)


def _guarded(n, shift=0):
    """(buffer, view of n floats inside it): NaN everywhere; ``shift`` floats move the view off 16-byte alignment."""
    buf = torch.full((GUARD + shift + n + GUARD,), float("nan"), device="cuda")
    return buf, buf[GUARD + shift:GUARD + shift + n]


def _guards_intact(buf, n, shift=0):
    return bool(torch.isnan(buf[:GUARD + shift]).all()) and bool(torch.isnan(buf[GUARD + shift + n:]).all())


def _dev(a, shift=0):
    """fp32 numpy -> a device tensor whose pointer is ``shift`` floats past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1)
    buf = torch.empty(t.numel() + shift, device="cuda")
    buf[shift:].copy_(t)
    v = buf[shift:]
    assert v.data_ptr() % 16 == (4 * shift) % 16
    return v


CORE_CASES = [
    # kernel the dispatcher must pick, F, head_dim, heads, B, floats the (qkv, outputs) are shifted by
    ("mfma", 1, 16, 3, 5, 0, 0), ("mfma", 16, 16, 3, 5, 0, 0), ("mfma", 17, 16, 3, 5, 0, 0),
    ("mfma", 48, 16, 3, 5, 0, 0),
    ("vector", 49, 16, 3, 5, 0, 0), ("vector", 64, 16, 3, 5, 0, 0), ("vector", 64, 4, 1, 6, 0, 0),
    ("vector", 64, 32, 2, 3, 0, 0),
    ("vector", 39, 16, 3, 5, 1, 0),          # the alignment fallback: qkv 4 bytes off
    ("vector", 39, 16, 3, 5, 0, 1),          # ... and the outputs 4 bytes off
]


@pytest.mark.parametrize("kind,F,hd,heads,B,in_shift,out_shift", CORE_CASES)
def test_core_kernels_vs_fp64_with_guard_bands(kind, F, hd, heads, B, in_shift, out_shift):
    """dfm_attention_core_forward / _backward on random qkv against the fp64 core; the floats before and after
    o and d_qkv stay NaN.  head_dim 16 with F <= 48 runs the matrix-core kernel unless a pointer is not 16-byte
    aligned: then, and for every other shape, the vector core."""
    from deepfm_amd import _lib
    lib = _lib.load()
    A = hd * heads
    assert lib.dfm_attention_core_supported(F, A, heads)
    aligned_shape = hd == 16 and F <= 48
    assert (kind == "mfma") == (aligned_shape and not in_shift and not out_shift)
    rng = np.random.default_rng([F, hd, heads, B])
    qkv = rng.standard_normal((B, F, 3 * A)).astype(np.float32)
    d_o = rng.standard_normal((B, F, A)).astype(np.float32)
    r_o, r_dqkv = attention_core_fp64(qkv, heads, d_o)
    q_dev, g_dev = _dev(qkv, in_shift), _dev(d_o)
    o_buf, o = _guarded(B * F * A, out_shift)
    _lib.check(lib.dfm_attention_core_forward(q_dev.data_ptr(), B, F, A, heads, o.data_ptr(), _lib.stream_handle()))
    d_buf, d_qkv = _guarded(B * F * 3 * A, out_shift)
    _lib.check(lib.dfm_attention_core_backward(q_dev.data_ptr(), g_dev.data_ptr(), B, F, A, heads, d_qkv.data_ptr(),
                                               _lib.stream_handle()))
    torch.cuda.synchronize()
    assert _guards_intact(o_buf, B * F * A, out_shift), "o: a float outside the output was written"
    assert _guards_intact(d_buf, B * F * 3 * A, out_shift), "d_qkv: a float outside the output was written"
    assert_close(npy(o).reshape(B, F, A), r_o, what="o")
    assert_close(npy(d_qkv).reshape(B, F, 3 * A), r_dqkv, what="d_qkv")


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("F", [17, 39, 48])
def test_block_kernels_extra_arguments_vs_fp64(F, D, residual):
    """dfm_attention_block_forward / _backward with every optional argument: a grouped output
    (out_group_stride > F * D), an input copy with its own stride, d_g_flat at a row stride, the FM term.
    d_o, d_y, d_stats, d_out, the copy, d_g_qkv and d_g_x against fp64; d_g_x = the block gradient + g_flat +
    g_fm[b] * (fm_sum[b] - x) as include/deepfm_hip.h states; nothing outside the rows is written (the ragged
    last tile included); the grouped call gives the bits of the contiguous one."""
    from deepfm_amd import _lib
    lib = _lib.load()
    B, H, A = 5, 4, 64
    M, FD = B * F, F * D
    assert lib.dfm_attention_block_supported(F, D, A, H)
    c = _case(F, D, H, A, B, residual)
    params, x, g_y = attention_case_inputs(c)
    pre = "layers.0."
    rng = np.random.default_rng([F, D, int(residual)])
    w_qkv = _dev(np.concatenate([params[pre + n + ".weight"] for n in ("W_q", "W_k", "W_v")]))
    b_qkv = _dev(np.concatenate([params[pre + n + ".bias"] for n in ("W_q", "W_k", "W_v")]))
    wo, bo = _dev(params[pre + "W_out.weight"]), _dev(params[pre + "W_out.bias"])
    gamma = _dev(params[pre + "layer_norm.weight"]) if residual else None
    beta = _dev(params[pre + "layer_norm.bias"]) if residual else None
    X, GY = _dev(x), _dev(g_y)
    st = _lib.stream_handle()

    # ---- fp64: the block, and the gradient of sum(g_y * y) (+ sum(g_y * x) through the residual) ----
    p64 = {k: torch.from_numpy(v.astype(np.float64)) for k, v in params.items()}
    x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    r = attention_block_fp64(x64, p64, pre, H, residual)
    r["qkv"].retain_grad()
    g64 = torch.from_numpy(g_y.astype(np.float64))
    ((r["y"] + x64 if residual else r["y"]) * g64).sum().backward()
    ref_dx, ref_dqkv = x64.grad.numpy(), r["qkv"].grad.numpy()

    # ---- forward: contiguous, then grouped with an input copy ----
    o_stride, c_stride = FD + 24, FD + 40
    fwd = []
    for grouped in (False, True):
        bufs = dict(o=_guarded(M * A), y=_guarded(M * D), stats=_guarded(M * 2),
                    out=_guarded(B * o_stride if grouped else M * D),
                    copy=_guarded(B * c_stride))
        _lib.check(lib.dfm_attention_block_forward(
            X.data_ptr(), w_qkv.data_ptr(), b_qkv.data_ptr(), wo.data_ptr(), bo.data_ptr(), _lib.ptr(gamma),
            _lib.ptr(beta), 1e-5 if residual else 0.0, B, F, D, A, H, bufs["o"][1].data_ptr(), bufs["y"][1].data_ptr(),
            bufs["out"][1].data_ptr(), bufs["stats"][1].data_ptr() if residual else None,
            o_stride if grouped else 0, bufs["copy"][1].data_ptr() if grouped else None, c_stride if grouped else 0, st))
        torch.cuda.synchronize()
        for k, (buf, view) in bufs.items():
            assert _guards_intact(buf, view.numel()), f"{k}: a float outside the output was written"
        if not residual:
            assert bool(torch.isnan(bufs["stats"][1]).all()), "statistics written without a LayerNorm"
        if grouped:
            out2 = bufs["out"][1].view(B, o_stride)
            assert bool(torch.isnan(out2[:, FD:]).all()), "out: the gap between grouped samples was written"
            cp2 = bufs["copy"][1].view(B, c_stride)
            assert bool(torch.isnan(cp2[:, FD:]).all()), "x copy: the gap between grouped samples was written"
            assert torch.equal(cp2[:, :FD].reshape(-1), X), "x copy differs from x"
            out = out2[:, :FD].reshape(-1)
        else:
            assert bool(torch.isnan(bufs["copy"][1]).all()), "an input copy nobody asked for"
            out = bufs["out"][1]
        fwd.append(dict(o=bufs["o"][1], y=bufs["y"][1], stats=bufs["stats"][1], out=out.clone()))
    for k in ("o", "y", "out") + (("stats",) if residual else ()):
        assert torch.equal(fwd[0][k], fwd[1][k]), f"{k}: the grouped call differs from the contiguous one"
    assert_close(npy(fwd[1]["o"]).reshape(B, F, A), r["o"].detach().numpy(), what="d_o")
    assert_close(npy(fwd[1]["y"]).reshape(B, F, D), r["y"].detach().numpy(), what="d_y")
    assert_close(npy(fwd[1]["out"]).reshape(B, F, D), r["out"].detach().numpy(), what="d_out")
    if residual:
        stats = npy(fwd[1]["stats"]).reshape(B, F, 2)
        assert_close(stats[..., :1], r["mean"].detach().numpy(), what="d_stats mean")
        assert_close(stats[..., 1:], r["rstd"].detach().numpy(), what="d_stats rstd")

    # ---- backward: alone, then with the gradient tail ----
    ld_flat = FD + 36
    g_flat = rng.standard_normal((B, ld_flat)).astype(np.float32)
    g_fm = rng.standard_normal(B).astype(np.float32)
    fm_sum = rng.standard_normal((B, D)).astype(np.float32)
    GF, GM, FS = _dev(g_flat), _dev(g_fm), _dev(fm_sum)
    bwd = []
    for tail in (False, True):
        q_buf, d_qkv = _guarded(M * 3 * A)
        x_buf, d_x = _guarded(M * D)
        _lib.check(lib.dfm_attention_block_backward(
            X.data_ptr(), w_qkv.data_ptr(), b_qkv.data_ptr(), wo.data_ptr(), GY.data_ptr(), int(residual), B, F, D, A,
            H, d_qkv.data_ptr(), d_x.data_ptr(), GF.data_ptr() if tail else None, ld_flat if tail else 0,
            GM.data_ptr() if tail else None, FS.data_ptr() if tail else None, st))
        torch.cuda.synchronize()
        assert _guards_intact(q_buf, M * 3 * A), "d_g_qkv: a float outside the output was written"
        assert _guards_intact(x_buf, M * D), "d_g_x: a float outside the output was written"
        bwd.append((d_qkv, d_x))
    assert torch.equal(bwd[0][0], bwd[1][0]), "d_g_qkv depends on the gradient tail"
    assert_close(npy(bwd[0][0]).reshape(B, F, 3 * A), ref_dqkv, what="d_g_qkv")
    assert_close(npy(bwd[0][1]).reshape(B, F, D), ref_dx, what="d_g_x")
    x_d = x.astype(np.float64)
    want = (ref_dx + g_flat[:, :FD].astype(np.float64).reshape(B, F, D)
            + g_fm.astype(np.float64)[:, None, None] * (fm_sum.astype(np.float64)[:, None, :] - x_d))
    assert_close(npy(bwd[1][1]).reshape(B, F, D), want, what="d_g_x with the tail")


def _rejected(lib, rc, *untouched):
    assert rc != 0, "the call was accepted"
    assert lib.dfm_last_error().decode("utf-8", "replace").strip(), "no error message"
    torch.cuda.synchronize()
    for t in untouched:
        assert bool(torch.isnan(t).all()), "a rejected call wrote to its output"


@pytest.mark.parametrize("F,A,heads", [(65, 32, 2), (20, 24, 2)], ids=["F65", "head_dim12"])
def test_core_rejects_unsupported_shapes(F, A, heads):
    from deepfm_amd import _lib
    lib = _lib.load()
    B = 2
    assert not lib.dfm_attention_core_supported(F, A, heads)
    qkv, d_o = torch.zeros(B * F * 3 * A, device="cuda"), torch.zeros(B * F * A, device="cuda")
    o = torch.full((B * F * A,), float("nan"), device="cuda")
    d_qkv = torch.full((B * F * 3 * A,), float("nan"), device="cuda")
    _rejected(lib, lib.dfm_attention_core_forward(qkv.data_ptr(), B, F, A, heads, o.data_ptr(), _lib.stream_handle()), o)
    _rejected(lib, lib.dfm_attention_core_backward(qkv.data_ptr(), d_o.data_ptr(), B, F, A, heads, d_qkv.data_ptr(),
                                                   _lib.stream_handle()), d_qkv)


@pytest.mark.parametrize("fault", ["d_g_x_aliases_d_x", "g_fm_without_fm_sum"])
def test_block_backward_rejects_bad_arguments(fault):
    from deepfm_amd import _lib
    lib = _lib.load()
    B, F, D, A, H = 2, 17, 16, 64, 4
    M = B * F
    x = torch.ones(M * D, device="cuda")
    w, b, wo, g_y = (torch.zeros(n, device="cuda") for n in (3 * A * D, 3 * A, D * A, M * D))
    g_fm = torch.zeros(B, device="cuda")
    d_qkv = torch.full((M * 3 * A,), float("nan"), device="cuda")
    d_x = torch.full((M * D,), float("nan"), device="cuda")
    alias = fault == "d_g_x_aliases_d_x"
    rc = lib.dfm_attention_block_backward(
        x.data_ptr(), w.data_ptr(), b.data_ptr(), wo.data_ptr(), g_y.data_ptr(), 1, B, F, D, A, H, d_qkv.data_ptr(),
        x.data_ptr() if alias else d_x.data_ptr(), None, 0, None if alias else g_fm.data_ptr(), None,
        _lib.stream_handle())
    _rejected(lib, rc, d_qkv, d_x)
    assert bool((x == 1.0).all()), "a rejected call wrote to its input"
