"""GPU: the d-input epilogues of dfm_linear_backward — the lower layer's BatchNorm mask (with and without dropout) and
the FM backward / addend — at the last-tile row counts and widths of tests/linear_bwd_epilogue_cases.py, on the guarded
buffers of tests/test_gpu_tower_matrix.py.  Both epilogues request the operands of all 16 accumulator rows from
addresses clamped to row M - 1 before they use the first: M = 1 and the one-row last tiles are where a wrong clamp
would read outside the operand (a guard float cannot see a read, so those cases are here to be run, and the clamp
is argued in the kernel).  dx / dy and the per-tile column sums against fp64 at the matrix's GEMM bar (the same
references meet it with a plain fp32 restatement on the host: tests/test_cpu_linear_bwd_epilogue_reference.py);
parts = 2 against parts = 3 bit for bit; every guard float intact."""
import ctypes as C

import pytest
import torch

from tests import linear_bwd_epilogue_cases as EC
from tests import tower_cases as TC
from tests.helpers import GuardedBuffer as G, assert_close, npy
from tests.test_gpu_tower_matrix import GEMM, Bn, _intact, _same_bits, tower_mode  # noqa: F401  (tower_mode: fixture)

pytestmark = pytest.mark.gpu


class Run:
    """One dfm_linear_backward launch of an epilogue case on fresh guarded buffers (outputs start as NaN)."""

    def __init__(self, _l, lib, M, K, epi, dim, p, parts, seed):
        N = EC.N_UP
        inp = TC.backward_inputs(M, N, K)
        self.dz, self.x, self.w = G.of(inp["dz"]), G.of(inp["x"]), G.of(inp["w"])
        self.slabs = G(lib.dfm_linear_backward_workspace_bytes(M, N, K) // 4)
        self.bn = Bn(_l, lib, M, K, p=p, seed=seed if p > 0 else None, salt=EC.SALT) if epi == "bn" else None
        self.gx = None if self.bn else G(M * K)
        self.keep, fm = [], None
        if self.bn is None:
            fm = _l.FmBwd()
            fm.dim = dim
            if epi in ("fm_g", "fm_ga"):
                g, S = G.of(inp["g_fm"]), G.of(EC.fm_sum(M, dim))
                self.keep += [g, S]
                fm.g_fm, fm.fm_sum, fm.e = g.ptr(), S.ptr(), self.x.ptr()
            if epi in ("fm_a", "fm_ga"):
                a = G.of(inp["addend"])
                self.keep.append(a)
                fm.addend = a.ptr()
        _l.check(lib.dfm_linear_backward(self.dz.ptr(), M, N, self.x.ptr(), K, self.w.ptr(),
                                         self.gx.ptr() if self.gx else None, C.byref(self.bn.ctx) if self.bn else None,
                                         C.byref(fm) if fm is not None else None, parts, self.slabs.ptr(),
                                         _l.stream_handle()))
        guards = dict(slabs=self.slabs, dx=self.gx, dz=self.dz, x=self.x, w=self.w)
        guards.update({f"fm{i}": b for i, b in enumerate(self.keep)})
        if self.bn:
            guards.update(self.bn.guards(), z=self.bn.z)
        _intact(**guards)
        T = (M + 31) // 32
        self.out = self.bn.dy.view(M, K) if self.bn else self.gx.view(M, K)
        self.partials = self.bn.ws.t[:T * 2 * K].view(T, 2, K) if self.bn else None


@pytest.mark.parametrize("M,K", EC.SHAPES, ids=lambda v: str(v))
def test_d_input_epilogues_vs_fp64(M, K, tower_mode):
    _l, lib = tower_mode(0)
    seed = torch.tensor([EC.SEED], dtype=torch.int64, device="cuda")
    for epi, dim, p in EC.epilogues(K):
        what = f"{epi} dim {dim} p {p}: "
        want, want_part = EC.reference(M, K, epi, dim, p)
        only_dx, both = (Run(_l, lib, M, K, epi, dim, p, parts, seed) for parts in (2, 3))
        assert_close(npy(both.out), want, what=what + ("dy" if epi == "bn" else "dx"), **GEMM)
        assert _same_bits(only_dx.out, both.out), what + "parts = 2 against parts = 3"
        assert bool(torch.isnan(only_dx.slabs.t).all()), what + "parts = 2 wrote a slab"
        if epi == "bn":
            assert_close(npy(both.partials), want_part, what=what + "column partials", **GEMM)
            assert _same_bits(only_dx.partials, both.partials), what + "partials, parts = 2 against parts = 3"
