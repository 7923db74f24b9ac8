"""Host proof for tests/test_gpu_linear_bwd_epilogue.py: the fp64 references of tests/linear_bwd_epilogue_cases.py are
held against a plain fp32 restatement of the two d-input epilogues (a row-by-row numpy transcription of what
bn_mask_tile and dx_tile_epilogue<2> compute, element by element and in the kernels' order of additions) at the very
bars the GPU test uses, for every case.  It also proves what the GPU comparison takes for granted: every BatchNorm
case keeps its distance from the ReLU kink, the dropout restatement keeps 1 - p of the elements, and the shapes reach
the operand route and the last-tile row counts the case list claims."""
import numpy as np
import pytest

from tests import linear_bwd_epilogue_cases as EC
from tests import tower_cases as TC
from tests.helpers import assert_close, tower_bn_relu_fp64

GEMM = dict(rtol=1e-5, atol_scale=2e-6)          # tests/test_gpu_tower_matrix.py::GEMM


def _dx_fp32(i):
    """dz W with fp32 products added in k order (the contraction is 8 long: any order is within the same bound)."""
    acc = np.zeros((i["dz"].shape[0], i["w"].shape[1]), dtype=np.float32)
    for k in range(EC.N_UP):
        acc = (acc + i["dz"][:, k:k + 1] * i["w"][k:k + 1, :]).astype(np.float32)
    return acc


def _emulate(M, K, epi, dim, p):
    f = np.float32
    i = TC.backward_inputs(M, EC.N_UP, K)
    v = _dx_fp32(i)
    if epi != "bn":
        if epi in ("fm_g", "fm_ga"):
            S = np.tile(EC.fm_sum(M, dim), (1, K // dim))
            v = (v + (i["g_fm"][:, None] * (S - i["x"]).astype(f)).astype(f)).astype(f)
        if epi in ("fm_a", "fm_ga"):
            v = (v + i["addend"]).astype(f)
        return v, None
    bn = TC.bn_inputs(M, K)
    mu, rs = bn["stats"]
    zh = ((bn["z"] - mu).astype(f) * rs).astype(f)
    y = (bn["gamma"] * zh).astype(f) + bn["beta"]
    scale = EC.keep_mask(EC.SEED, EC.SALT, M * K, p).reshape(M, K).astype(f) * f(1.0 / (1.0 - p))
    dy = np.where(y > 0, (v * scale).astype(f), f(0))
    T = (M + 31) // 32
    part = np.zeros((T, 2, K), dtype=f)
    for m in range(M):
        part[m // 32, 0] = (part[m // 32, 0] + dy[m]).astype(f)
        part[m // 32, 1] = (part[m // 32, 1] + (dy[m] * zh[m]).astype(f)).astype(f)
    return dy, part


@pytest.mark.parametrize("M,K", EC.SHAPES, ids=lambda v: str(v))
def test_fp32_restatement_meets_the_gpu_bars(M, K):
    for epi, dim, p in EC.epilogues(K):
        what = f"{epi} dim {dim} p {p}: "
        want, want_part = EC.reference(M, K, epi, dim, p)
        got, got_part = _emulate(M, K, epi, dim, p)
        assert_close(got, want, what=what + "d input", **GEMM)
        if epi == "bn":
            assert_close(got_part, want_part, what=what + "column partials", **GEMM)


def test_case_list_covers_what_it_claims():
    assert [((M - 1) % 64) % 32 + 1 for M in EC.M_ALL] == [1, 2, 1, 31, 1, 1]      # rows of the last 32-row MFMA tile
    assert [(M - 1) % 64 + 1 for M in EC.M_ALL] == [1, 2, 33, 63, 1, 1]            # rows of the last workgroup tile
    assert [EC.route(K) for K in EC.K_FAST + (EC.K_DIM16,)] == ["fast"] * 4
    assert [EC.route(K) for K in EC.K_CHECKED] == ["checked"] * 3
    assert [EC.fm_dims(K) for K in EC.K_FAST + EC.K_CHECKED + (EC.K_DIM16,)] == [(4,)] * 3 + [(1,)] * 3 + [(4, 16)]
    for K in EC.K_FAST + EC.K_CHECKED:
        names = [e for e in EC.epilogues(K)]
        assert ("bn", 0, 0.0) in names and ("bn", 0, EC.DROPOUT_P) in names
        assert {n for n, _, _ in names} == {"bn", "fm_g", "fm_a", "fm_ga"}
    assert {d for _, d, _ in EC.epilogues(EC.K_DIM16)} == {4, 16}


@pytest.mark.parametrize("M,K", [s for s in EC.SHAPES if s[1] != EC.K_DIM16], ids=lambda v: str(v))
def test_bn_cases_stay_clear_of_the_relu_kink(M, K):
    bn = TC.bn_inputs(M, K)
    mean, rstd = bn["stats"].astype(np.float64)
    _, y, _ = tower_bn_relu_fp64(bn["z"], mean, rstd, bn["gamma"], bn["beta"])
    assert np.abs(y).min() >= TC.KINK_MARGIN


def test_dropout_restatement_keeps_one_minus_p():
    keep = EC.keep_mask(EC.SEED, EC.SALT, 1 << 16, EC.DROPOUT_P)
    assert abs(keep.mean() - (1 - EC.DROPOUT_P)) < 4 * (EC.DROPOUT_P * (1 - EC.DROPOUT_P) / (1 << 16)) ** 0.5
    assert EC.keep_mask(EC.SEED, EC.SALT, 64, 0.0).all()
    assert not np.array_equal(keep[:4096], EC.keep_mask(EC.SEED, EC.SALT + 1, 4096, EC.DROPOUT_P))
