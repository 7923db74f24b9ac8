"""The fp64 CIN reference of tests/helpers.py, tied on the CPU to the CIN goldens and to the fp32 oracle; the
kink margin of every kink-free case of tests/test_gpu_cin_matrix.py, measured on the reference alone; that
matrix's coverage of the kernel instantiations, read off its case lists; and the library's route decision against
the matrix's restatement of it (host predicates only)."""
import numpy as np
import pytest

from oracle import ctr_oracle as O
from tests.helpers import (assert_close, bf16_round, cin_bf16_emulation, cin_case_inputs, cin_fp64, cin_full_params,
                           cin_split_layout, group, load)
from tests.test_gpu_cin_matrix import (ACCUMULATE_RUNS, ALL_RUNS, GENERAL_CASES, MFMA_CASES, RAGGED_RUNS, case_id,
                                       expected_route, general_reasons, library_route, reference, run_id)

GOLDENS = ["cin_small_split", "cin_small_nosplit", "cin_single_layer", "cin_odd_split", "cin_criteo_full"]


@pytest.mark.parametrize("case", GOLDENS)
def test_fp64_reference_reproduces_golden(case):
    g = load(case)
    sizes, split = [int(s) for s in g["layer_sizes"]], bool(g["split_half"])
    params = cin_full_params() if bool(g["hashed"]) else group(g, "param/")
    out, d_x, grads, _ = cin_fp64(g["x"], params, sizes, split, g["upstream"])
    assert_close(out, g["out"], what="out")
    assert_close(d_x, g["d_x"], what="d_x")
    assert sorted(grads) == sorted(params)
    for k in grads:
        if bool(g["hashed"]):
            got = grads[k].reshape(-1)
            assert_close(got[::97] if k.endswith("weight") else got, g["grad_sample/" + k], what=k)
        else:
            assert_close(grads[k], g["grad/" + k], what=k)


@pytest.mark.parametrize("c", [MFMA_CASES[2], MFMA_CASES[4]], ids=case_id)
def test_oracle_within_the_bar_of_fp64(c):
    F, D, sizes, split, B = c
    params, x, up, (r_out, r_dx, r_grads, _) = reference(c, True)
    assert_close(O.cin_forward(x, params, list(sizes), split), r_out, what="out")
    d_x, grads = O.cin_backward(x, params, list(sizes), split, up)
    assert_close(d_x, r_dx, what="d_x")
    assert sorted(grads) == sorted(r_grads)
    for k in grads:
        assert_close(grads[k], r_grads[k], what=k)
    params, x, _, (r_out, _, _, _) = reference(c, False)
    assert_close(O.cin_forward(x, params, list(sizes), split), r_out, what="out, ordinary parameters")


@pytest.mark.parametrize("c", sorted({c for c, _ in ALL_RUNS}), ids=case_id)
def test_kink_free_cases_keep_their_margin(c):
    """min |pre-activation| > 1e-2 on the fp64 reference for the seeds the matrix uses, with live and dead channels
    both present; the ordinary parameters of the same case do put pre-activations on both sides of the kink."""
    _, _, _, (_, _, _, pre) = reference(c, True)
    assert min(float(np.abs(a).min()) for a in pre) > 1e-2
    assert min(float(np.abs(a).min()) for a in pre) > 1.0          # in fact the margin is wide: plain bf16 keeps it
    for a in pre:
        if a.shape[1] >= 3:
            assert (a > 0).any() and (a < 0).any()
    _, _, _, (_, _, _, pre) = reference(c, False)
    assert all((a > 0).any() and (a < 0).any() for a in pre)


def test_bf16_round_is_nearest_even():
    import torch
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 3.0,
                        np.array([1.00390625, 1.01171875, -1.00390625, 0.0, 1.0, 3.3895314e38 / 2], dtype=np.float32)])
    assert np.array_equal(bf16_round(a), torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy())
    assert bf16_round(np.float32([1.00390625]))[0] == 1.0 and bf16_round(np.float32([1.01171875]))[0] == np.float32(1.015625)


def test_bf16_emulation_is_the_reference_up_to_bf16():
    """The emulation differs from fp64 by bf16 rounding alone (relative 2^-9 per operand) and not by more."""
    c = MFMA_CASES[2]
    F, D, sizes, split, B = c
    params, x, up, (r_out, r_dx, r_grads, _) = reference(c, True)
    e = cin_bf16_emulation(x, params, list(sizes), split, up)
    for got, want in [(e["out"], r_out), (e["d_x"], r_dx)] + [(e["grads"][k], r_grads[k]) for k in r_grads]:
        err = float(np.abs(got - want).max() / np.abs(want).max())
        assert err < 2e-2, err
    assert float(np.abs(e["out"] - r_out).max()) > 0.0


# ---- coverage: every instantiation is launched by some case of the matrix ----

def test_matrix_covers_every_instantiation():
    on_cores = [c for c in MFMA_CASES if expected_route(c, 0) == "mfma"]
    assert all(expected_route(c, 1) == "mfma" for c in on_cores)            # SPLIT = true and false: both modes run
    assert {(c[1], (c[0] + 7) // 8) for c in on_cores} == {(D, fg) for D in (8, 16, 32) for fg in (1, 2, 3, 4, 5)}
    layers = [(c, ch) for c in on_cores for ch in c[2]]
    padded_mb4 = [ch for _, ch in layers if 97 <= ch < 128]
    padded_ks8 = [ch for _, ch in layers if 113 <= ch < 128]
    assert padded_mb4 and padded_ks8 and 97 in padded_mb4 and 113 in padded_ks8
    assert any(ch == 128 for _, ch in layers)
    assert any(ch <= 96 for _, ch in layers) and any(ch <= 112 for _, ch in layers)          # MB < 4, KS < 8
    assert any(c[0] % 8 == 0 for c in on_cores) and any(c[0] % 8 != 0 for c in on_cores)    # separate / fused bias
    assert any(len(c[2]) == 8 for c in on_cores) and any(len(c[2]) == 1 for c in on_cores)
    assert {1, 40} <= {c[0] for c in on_cores}
    assert any(max(cin_split_layout(c[0], c[2], c[3])[0]) == 128 for c in on_cores)
    assert any(c[1] == 16 and c[4] % 2 for c in on_cores) and any(c[1] == 16 and c[4] % 16 for c in on_cores)
    assert any(c[4] == 1 for c in on_cores)
    assert any(c[1] == 8 and (c[4] * 8) % 32 for c in on_cores)
    assert any(c[4] > 16 * 16 for c in on_cores)                             # more than one workgroup of each kernel


def test_matrix_covers_every_general_route_reason():
    why = set()
    for c, mode in ALL_RUNS:
        why |= general_reasons(c, mode)
    assert why == {"mode 2", "D", "F > 40", "L > 8", "C or H > 128", "LDS"}
    routes = {expected_route(c, mode) for c, mode in ALL_RUNS}
    assert routes == {"mfma", "mfma_fwd+general_bwd", "general"}
    general = [c for c, mode in GENERAL_CASES if expected_route(c, mode) == "general"]
    assert (39, 16, (200, 200, 200), True, 9) in general
    assert any(c[4] < 8 for c in general) and any(c[4] == 1 for c in general)
    # C D 4 bytes of bias partials on both sides of the 64 KB default limit, and the layer kernels' LDS above it
    assert {c[2][0] * c[1] * 4 <= 65536 for c in general if c[1] == 64} == {True, False}
    assert any((c[0] + c[0] + c[2][0]) * c[1] * 4 > 65536 for c in general)
    for runs in (ACCUMULATE_RUNS, RAGGED_RUNS):
        assert {expected_route(c, mode) for c, mode in runs} == {"mfma", "mfma_fwd+general_bwd", "general"}
        assert all((c, mode) in ALL_RUNS or mode == 1 for c, mode in runs)
    assert {c[4] for c, _ in RAGGED_RUNS} >= {1, 3, 5, 17, 257} and ((20, 8, (40, 24), True, 6), 0) in RAGGED_RUNS
    assert len({run_id(r) for r in ALL_RUNS}) == len(ALL_RUNS)


def test_library_route_agrees_with_expected_route():
    from deepfm_amd import _lib
    lib = _lib.load()
    before = lib.dfm_cin_get_mode()
    try:
        for mode in (0, 1, 2):
            assert lib.dfm_cin_set_mode(mode) == 0
            for c in sorted({c for c, _ in ALL_RUNS}):
                assert library_route(lib, c) == expected_route(c, mode), f"{case_id(c)} mode {mode}"
        lib.dfm_cin_set_mode(0)
        # the LDS term on both sides: 16 KB per field group + 1 KB per hidden row against 160 KB
        assert library_route(lib, (16, 16, (128, 128), False, 4)) == "mfma"          # 32 + 128
        assert library_route(lib, (17, 16, (128, 128), False, 4)) == "general"       # 48 + 128
        assert library_route(lib, (40, 16, (80, 80), False, 4)) == "mfma"            # 80 + 80
        assert library_route(lib, (40, 16, (81, 80), False, 4)) == "general"         # 80 + 82
    finally:
        lib.dfm_cin_set_mode(before)
