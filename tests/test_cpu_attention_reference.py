"""The fp64 attention reference of tests/helpers.py, tied on the CPU to the attention goldens and to the fp32
oracle over every shape of tests/test_gpu_attention_matrix.py; and that matrix's coverage of the kernel
template instantiations, read off its parametrisation."""
import numpy as np
import pytest

from oracle import ctr_oracle as O
from tests.helpers import (assert_close, attention_case_inputs, attention_core_fp64, attention_fp64, error_ratio,
                           group, load)
from tests.test_gpu_attention_matrix import MATRIX, PER_ROUTE, WKB_FLOOR, case_id, expected_route

GOLDENS = ["attn_cfg4", "attn_two_layers", "attn_no_residual", "attn_odd"]


def _floor(k):
    return WKB_FLOOR if k.endswith("W_k.bias") else 0.0


@pytest.mark.parametrize("case", GOLDENS)
def test_fp64_reference_reproduces_golden(case):
    g = load(case)
    params = group(g, "param/")
    out, d_x, grads = attention_fp64(g["x"], params, int(g["num_heads"]), int(g["num_layers"]),
                                     bool(g["use_residual"]), g["upstream"])
    assert_close(out, g["out"], what="out")
    assert_close(d_x, g["d_x"], what="d_x")
    want = group(g, "grad/")
    assert sorted(grads) == sorted(want)
    for k in want:
        if k.endswith("W_k.bias"):
            assert float(np.abs(grads[k]).max()) < 1e-12, f"{k}: the fp64 gradient is not zero"
        assert_close(grads[k], want[k], what=k, floor=_floor(k))


@pytest.mark.parametrize("entry", MATRIX, ids=case_id)
def test_oracle_within_the_bar_of_fp64_on_the_matrix(entry):
    c, _ = entry
    params, x, up = attention_case_inputs(c)
    r_out, r_dx, r_grads = attention_fp64(x, params, c["heads"], c["layers"], c["residual"], up)
    assert_close(O.attention_forward(x, params, c["heads"], c["layers"], c["residual"]), r_out, what="out")
    d_x, grads = O.attention_backward(x, params, c["heads"], c["layers"], c["residual"], up)
    assert_close(d_x, r_dx, what="d_x")
    assert sorted(grads) == sorted(r_grads)
    for k in grads:
        if k.endswith("W_k.bias"):
            assert float(np.abs(r_grads[k]).max()) < 1e-12, f"{k}: the fp64 gradient is not zero"
        assert_close(grads[k], r_grads[k], what=k, floor=_floor(k))


def test_core_reference_agrees_with_block_reference():
    """attention_core_fp64 on the projection of a block equals that block's head outputs."""
    import torch
    from tests.helpers import attention_block_fp64
    c = dict(B=3, F=7, D=12, heads=3, A=24, layers=1, residual=False)
    params, x, _ = attention_case_inputs(c)
    p64 = {k: torch.from_numpy(v.astype(np.float64)) for k, v in params.items()}
    r = attention_block_fp64(torch.from_numpy(x.astype(np.float64)), p64, "layers.0.", 3, False)
    o, _ = attention_core_fp64(r["qkv"].numpy(), 3)
    np.testing.assert_allclose(o, r["o"].numpy(), rtol=1e-12, atol=1e-14)


def test_sharp_regime_is_ill_conditioned_for_fp32():
    """x scaled by 6 (test_sharp_softmax_vs_fp64): the scores reach the hundreds, and the fp32 oracle is finite
    but no longer inside the project bar of fp64 on every tensor — why that test takes its bar from the oracle."""
    worst = 0.0
    for c, _ in PER_ROUTE:
        params, x, up = attention_case_inputs(c, x_scale=6.0)
        _, _, r_grads = attention_fp64(x, params, c["heads"], c["layers"], c["residual"], up)
        d_x, grads = O.attention_backward(x, params, c["heads"], c["layers"], c["residual"], up)
        assert np.isfinite(d_x).all() and all(np.isfinite(v).all() for v in grads.values())
        worst = max(worst, max(error_ratio(grads[k], r_grads[k], floor=_floor(k)) for k in grads))
        q = x.reshape(-1, c["D"]) @ params["layers.0.W_q.weight"].T
        k_ = x.reshape(-1, c["D"]) @ params["layers.0.W_k.weight"].T
        assert float(np.abs(q).max() * np.abs(k_).max()) > 100.0
    assert worst > 1.0


# ---- coverage: every template instantiation is launched by some case of the matrix ----

def _tiles(F):
    return (F + 15) // 16


def test_matrix_covers_every_instantiation():
    by = {}
    for c, path in MATRIX:
        by.setdefault(path, []).append(c)
    block = {(_tiles(c["F"]), c["D"] // 16, c["residual"]) for c in by["whole_block"]}
    assert block == {(nt, kd, res) for nt in (1, 2, 3) for kd in (1, 2, 3, 4) for res in (True, False)}
    for c in by["whole_block"]:
        assert c["heads"] == 4 and c["A"] == 64 and c["D"] % 16 == 0 and c["F"] <= 48
    inside = {(_tiles(c["F"]), c["D"] // 16) for c in by["qkv_inside"] if c["heads"] != 4}
    assert inside == {(nt, kd) for nt in (1, 2, 3) for kd in (1, 2, 3, 4)}
    assert {c["heads"] for c in by["qkv_inside"]} == {1, 2, 4, 8}
    assert {c["F"] for c in by["mfma_core"] if c["layers"] == 1} == {1, 15, 16, 17, 32, 33, 48}
    for c in by["mfma_core"]:
        assert c["A"] // c["heads"] == 16 and c["D"] % 16 != 0 and c["D"] % 4 == 0
    vec = {(c["A"] // c["heads"], c["F"]) for c in by["vector_core"]}
    assert vec == ({(hd, F) for hd in (4, 8, 32) for F in (1, 2, 39, 63, 64)} | {(16, F) for F in (49, 63, 64)})
    assert any(c["heads"] == 1 for c in by["vector_core"])
    assert {c["F"] for c in by["per_sample"]} >= {65, 100}
    assert any(c["B"] == 1 for c in by["per_sample"])
    assert any(c["A"] // c["heads"] not in (4, 8, 16, 32) and c["F"] <= 64 for c in by["per_sample"])
    (forced,) = by["per_sample_forced"]
    assert forced in by["whole_block"]                      # identical inputs on both paths
    assert {path for c, path in MATRIX if c["layers"] == 2} == {"whole_block", "qkv_inside", "mfma_core"}


def test_matrix_batches():
    for c, _ in MATRIX:
        assert 3 <= c["B"] <= 9 or (c["B"] == 1 and c["F"] == 23)
        if c["heads"] % 4 != 0 and c["B"] != 1:
            assert (c["B"] * c["heads"]) % 4 != 0           # a partly empty last workgroup wherever possible
    # the routes whose workgroups hold four (sample, head) units: at least half end in a partly empty workgroup
    units = [c for c, path in MATRIX if path in ("qkv_inside", "mfma_core", "vector_core")]
    assert 2 * sum((c["B"] * c["heads"]) % 4 != 0 for c in units) >= len(units)
    assert len({case_id(e) for e in MATRIX}) == len(MATRIX)


# ---- the module's route decision against the matrix's own restatement of it ----

def _gemm_core(route):
    """``block_route`` leaves the choice between the matrix-core and the vector core to the library."""
    return "gemm_core" if route in ("mfma_core", "vector_core") else route


def test_block_route_agrees_with_expected_route():
    """``block_route`` against ``expected_route`` on every shape of ``MATRIX``, under all four settings of the two
    switches.  Host predicates only."""
    from deepfm_amd import _lib
    from deepfm_amd.models.layers.attention import _AttentionBlock, block_route
    lib = _lib.load()
    seen = set()
    for c, path in MATRIX:
        blk = _AttentionBlock(c["D"], c["heads"], c["A"], c["residual"])
        for gemm_path in (True, False):
            for whole_block_kernel in (True, False):
                blk.gemm_path, blk.whole_block_kernel = gemm_path, whole_block_kernel
                want = _gemm_core(expected_route(lib, c, gemm_path, whole_block_kernel))
                got = block_route(blk, c["F"])
                assert got == want, f"{case_id((c, path))} gemm_path={gemm_path} whole_block={whole_block_kernel}"
                seen.add(got)
    assert seen == {"per_sample", "whole_block", "qkv_inside", "gemm_core"}


def test_block_route_alignment_terms():
    """A whole-block shape: a misaligned W_out alone leaves the projection inside; misaligned x / W_qkv / b_qkv
    put the projection GEMM in front of the core."""
    from deepfm_amd.models.layers.attention import _AttentionBlock, block_route
    blk = _AttentionBlock(32, 4, 64, True)
    assert block_route(blk, 17) == "whole_block"
    assert block_route(blk, 17, w_out_aligned=False) == "qkv_inside"
    assert block_route(blk, 17, aligned=False) == "gemm_core"
    assert block_route(blk, 17, aligned=False, w_out_aligned=False) == "gemm_core"
