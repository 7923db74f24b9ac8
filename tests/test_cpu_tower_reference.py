"""CPU: the fp64 restatements of the DNN tower (tests/helpers.py) agree with torch autograd, the host restatement
of the batch-split plan equals the library's, and every case of the GPU matrix (tests/tower_cases.py) really
reaches the loop phase and operand route it claims and keeps its distance from the ReLU kink — so that
tests/test_gpu_tower_matrix.py needs no exclusions.  No GPU: only host entry points of the library are called."""
import numpy as np
import pytest
import torch

from tests import tower_cases as TC
from tests.helpers import (assert_close, tower_bn_backward_fp64, tower_bn_relu_fp64, tower_column_stats_fp64,
                           tower_dw_split_plan, tower_dw_splits, tower_head_fp64, tower_linear_backward_fp64,
                           tower_linear_fp64, tower_masked_grad_fp64)


@pytest.mark.parametrize("M,N,K", [(7, 5, 3), (33, 12, 9)])
def test_restatements_agree_with_autograd(M, N, K):
    """Linear -> BatchNorm1d(train) -> ReLU -> Linear(1) -> BCEWithLogits in torch float64 autograd against the
    step-by-step restatements chained by hand."""
    rng = np.random.default_rng([M, N, K])
    x, w, b = rng.standard_normal((M, K)), rng.standard_normal((N, K)), rng.standard_normal(N)
    gamma, beta = rng.uniform(0.5, 1.5, N), rng.standard_normal(N) * 0.3
    hw, hb = rng.standard_normal(N), rng.standard_normal(1)
    labels = (rng.uniform(size=M) < 0.4).astype(np.float64)
    t = {k: torch.from_numpy(v).requires_grad_() for k, v in dict(x=x, w=w, b=b, gamma=gamma, beta=beta, hw=hw, hb=hb).items()}
    lin = t["x"] @ t["w"].T + t["b"]
    bn = torch.nn.functional.batch_norm(lin, None, None, t["gamma"], t["beta"], True, 0.1, TC.EPS)
    a = torch.relu(bn)
    logits = a @ t["hw"] + t["hb"]
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(labels))
    lin.retain_grad(); bn.retain_grad(); a.retain_grad(); logits.retain_grad()
    loss.backward()
    # the same, by hand
    z = tower_linear_fp64(x, w, b)
    mean, var = tower_column_stats_fp64(z)
    rstd = 1.0 / np.sqrt(var + TC.EPS)
    xhat, y, act = tower_bn_relu_fp64(z, mean, rstd, gamma, beta)
    head = tower_head_fp64(act, hw, hb, None, None, labels)
    tight = dict(rtol=1e-10, atol_scale=1e-12)
    assert_close(z, lin.detach().numpy(), what="z", **tight)
    assert_close(act, a.detach().numpy(), what="a", **tight)
    assert_close(head["logits"], logits.detach().numpy(), what="logits", **tight)
    assert abs(head["loss"] - float(loss.detach())) < 1e-12
    assert_close(head["dlogits"], logits.grad.numpy(), what="d logits", **tight)
    assert_close(head["dw"], t["hw"].grad.numpy(), what="d head w", **tight)
    assert abs(head["db"] - float(t["hb"].grad)) < 1e-12
    dy = tower_masked_grad_fp64(head["dlogits"][:, None] * hw[None, :], y)
    assert_close(dy, bn.grad.numpy(), what="dy", **tight)
    dgamma, dbeta, dz = tower_bn_backward_fp64(dy, xhat, gamma, rstd)
    assert_close(dgamma, t["gamma"].grad.numpy(), what="d gamma", **tight)
    assert_close(dbeta, t["beta"].grad.numpy(), what="d beta", **tight)
    assert_close(dz, lin.grad.numpy(), what="dz", **tight)
    dW, dx = tower_linear_backward_fp64(dz, x, w)
    assert_close(dW, t["w"].grad.numpy(), what="dW", **tight)
    assert_close(dx, t["x"].grad.numpy(), what="dx", **tight)
    # the FM term and the addend of the first layer's epilogue, against their definition
    g_fm, S, add = rng.standard_normal(M), rng.standard_normal((M, 3)), rng.standard_normal((M, K * 3))
    e, w3 = rng.standard_normal((M, K * 3)), rng.standard_normal((N, K * 3))
    _, dx3 = tower_linear_backward_fp64(dz, e, w3, g_fm, S, e, add)
    want = dz @ w3 + g_fm[:, None] * (np.tile(S, (1, K)) - e) + add
    assert_close(dx3, want, what="dx + fm + addend", **tight)


def test_split_plan_restatement_equals_the_library():
    from deepfm_amd import _lib
    lib = _lib.load()
    shapes = TC.all_backward_shapes() + [(4096, 256, 624), (4096, 128, 256), (4099, 40, 52), (1000, 36, 44)]
    for M, N, K in shapes:
        splits, kps, rows = tower_dw_split_plan(N, K, M)
        assert lib.dfm_linear_backward_splits(M, N, K) == splits, (M, N, K)
        assert sum(rows) == M and all(r > 0 for r in rows) and kps % 32 == 0
        want = (4 * tower_dw_splits(N, K, M) * N * K + 255) // 256 * 256
        assert lib.dfm_linear_backward_workspace_bytes(M, N, K) == want, (M, N, K)
        assert want >= 4 * splits * N * K, "the workspace holds every slab that is launched"
    assert tower_dw_split_plan(256, 624, 4096)[1] == 480
    assert tower_dw_split_plan(8, 12, 300)[2] == [160, 140]


@pytest.mark.parametrize("case", TC.BWD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_backward_case_reaches_its_declared_phase(case):
    assert TC.dw_phase_holds(case), (case, tower_dw_split_plan(case[1], case[2], case[0]))


def test_steady_case_is_the_declared_one_and_lists_cover_the_phases():
    splits, kps, rows = tower_dw_split_plan(TC.BWD_STEADY[1], TC.BWD_STEADY[2], TC.BWD_STEADY[0])
    assert (splits, kps, rows[-1]) == (4, 352, 321)
    phases = {c[5] for c in TC.BWD_CASES}
    assert {"one", "ragged", "sub32", "steady"} | {f"slice{s}" for s in range(1, 7)} <= phases
    ks = set(TC.K_FAST)
    assert all(k % 4 == 0 for k in TC.K_FAST) and all(k % 4 for k in TC.K_CHECKED)
    assert {319, 321} <= set(TC.K_CHECKED) and {316, 320, 324, 448} <= ks                  # the steady boundary
    assert {32 * s for s in range(1, 7)} <= ks and {4, 28} <= ks                           # prologue slots
    assert {k % 128 // 32 for k in ks if k % 32} == {0, 1, 2, 3}                            # partial slice, each tail step
    routes = {TC.fwd_route(c) for c in TC.FWD_CASES}
    assert routes == {"fast", "checked"}
    for k in (64, 320):
        assert TC.fwd_route((70, 68, k, "ldx4", True)) == "fast" and TC.fwd_route((70, 68, k, "ldx1", True)) == "checked"
        assert TC.fwd_route((70, 68, k, "x_off", True)) == "checked"
    assert {(TC.bwd_route(c), c[3][:2]) for c in TC.BWD_CASES} >= {(r, e) for r in ("fast", "checked") for e in ("pl", "bn", "fm")}
    for M, N, K, _ in TC.X3_CASES:
        assert N % 8 == 0 and M % 2 == 0 and K % 4 == 0 and tower_dw_split_plan(N, K, M)[1] % 2 == 0
    assert [(M % 2, N % 8, v) for M, N, K, v in TC.X3_FALLBACK] == [(0, 4, "plain"), (1, 0, "plain"), (0, 0, "w_off"),
                                                                   (0, 0, "dz_off")]
    # every optional head pointer is passed and withheld at least twice
    flags = np.array([TC.head_nulls(ch, M) for ch in TC.HEAD_CH for M in TC.HEAD_M])
    assert (flags.sum(0) >= 2).all() and ((~flags).sum(0) >= 2).all()


def _masked_layers():
    """(M, features, tag) of every BatchNorm layer through whose ReLU mask a matrix case pushes a gradient."""
    s = {(c[0], c[2], 0) for c in TC.BWD_CASES if c[3] == "bn"} | {(c[0], c[2], 0) for c in TC.X3_CASES if c[3] == "bn"}
    s |= {(m, n, 0) for m in TC.APPLY_M for n in TC.APPLY_N}
    s |= {(m, 32 * ch, 0) for m in TC.HEAD_M for ch in TC.HEAD_CH}
    return sorted(s)


def test_kink_margin_of_every_masked_case():
    """min |gamma xhat + beta| >= 1e-4 in fp64 (fp32 evaluation of y moves it by ~1e-6 at most), with live and dead
    elements both present wherever the layer has more than a handful of elements."""
    for M, N, tag in _masked_layers():
        bn = TC.bn_inputs(M, N, tag)
        y = TC.bn_y_fp64(bn)
        assert np.abs(y).min() >= TC.KINK_MARGIN, (M, N, float(np.abs(y).min()))
        if M * N >= 64:
            assert 0.2 < (y > 0).mean() < 0.8, (M, N)
        # the statistics handed to the kernels are those of z to fp32 rounding (the moved elements are few and near)
        mean, var = tower_column_stats_fp64(bn["z"])
        if M >= 31:
            assert_close(bn["stats"][0], mean, rtol=1e-3, atol_scale=1e-3, what="mean")
