"""Host-side proof of the GEMM matrix (tests/gemm_cases.py): the case tables name every instantiation of
csrc/gemm_skinny.hip and csrc/gemm_f32.hip, every case takes the route, the split count and the launch plan it claims
(dfm_gemm_route / dfm_gemm_splits / dfm_weight_grad_partial_blocks / dfm_weight_grad_workspace_bytes: host arithmetic,
no GPU), the integer family is exact, a plain float32 evaluation stays a factor 4 inside every float bar, and the
mistakes the matrix exists for change the result."""
import re
from pathlib import Path

import numpy as np
import pytest

from deepfm_amd import _lib
from tests import gemm_cases as GC

ROOT = Path(__file__).resolve().parent.parent
BASE = 1 << 20                      # a 16-byte aligned address for the route predicate (never read)


def _route(lib, c: GC.Gemm):
    return lib.dfm_gemm_route(BASE + 4 * c.a_shift, c.lda, int(c.a_kc), BASE + 4 * c.b_shift, c.ldb, int(c.b_kc), c.m, c.n,
                              c.k, int(c.bias), int(c.ws))


def test_entry_points_are_declared():
    header = (ROOT / "include" / "deepfm_hip.h").read_text()
    for name in ("dfm_gemm_route", "dfm_gemm_splits"):
        assert re.search(rf"\bint {name}\(", header) and name in _lib.SIGNATURES
    for name, value in (("TILED_SLOW", 0), ("TILED_FAST", 1), ("ROWS", 2), ("WGRAD", 3)):
        assert re.search(rf"#define DFM_GEMM_ROUTE_{name} {value}\b", header)
        assert getattr(GC, name) == getattr(_lib, "GEMM_" + name) == value
    assert _lib.MAX_PARTIAL_JOBS == GC.MAX_PARTIAL_JOBS
    assert re.search(rf"kMaxPartialJobs = {GC.MAX_PARTIAL_JOBS};", (ROOT / "deepfm_amd/csrc/gemm_skinny.hip").read_text())
    assert _lib.load().dfm_abi_version() == _lib.ABI_VERSION


def test_instantiation_lists_equal_the_source():
    rows, wg = GC.parse_instantiations()
    src = (ROOT / "deepfm_amd/csrc/gemm_skinny.hip").read_text()
    assert GC.ROWS_SPECIAL not in rows and re.search(r"N == 192 && K == 32", src)
    assert rows | {GC.ROWS_SPECIAL} == set(GC.ROWS_SHAPES) and len(GC.ROWS_SHAPES) == 10
    assert wg == set(GC.WGRAD_SHAPES) and len(GC.WGRAD_SHAPES) == 7
    pair = re.search(r"gemm_wgrad_pair_kernel<(\d), (\d), (\d), (\d)>\), dim3", src)
    t = [32 * int(v) for v in pair.groups()]
    assert ((t[0], t[1]), (t[2], t[3])) == GC.WGRAD_PAIR
    consts = dict(kWaves=GC.WAVES, kSkinnyMinRows=GC.SKINNY_MIN_ROWS)
    for name, value in consts.items():
        assert re.search(rf"{name} = {value};", src)
    assert re.search(r"kMaxResidentWaves = 2 \* 256 \* kWaves;", src) and re.search(r"kWgradWaves = 2 \* 256 \* kWaves;", src)
    core = (ROOT / "deepfm_amd/csrc/gemm_core.h").read_text()
    assert re.search(rf"BM = {GC.BM}, BN = {GC.BN}, BK = {GC.BK};", core)


def test_every_table_entry_is_named_by_a_case():
    G, W = GC.GEMM_CASES, GC.WGRAD_CASES
    on_rows = {(c.n, c.k, c.b_kc, c.m) for c in G.values() if c.route == GC.ROWS}
    for N, K in GC.ROWS_SHAPES:
        for w_kc in (False, True):
            assert (N, K, w_kc, GC.M_BASE) in on_rows
    for N, K in ((32, 32), (32, 192), (192, 32)):
        assert {M for M in GC.M_SWEEP if any((N, K, kc, M) in on_rows for kc in (False, True))} == set(GC.M_SWEEP)
    for N in (32, 64, 96, 192):        # bias and accumulate: each value with each NT
        group = [c for c in G.values() if c.route == GC.ROWS and c.n == N and c.m == GC.M_BASE]
        assert {c.bias for c in group} == {True, False} == {c.acc for c in group}
    strides = [c for c in G.values() if c.name.startswith("rows_strides_")]
    assert {(c.n, c.k, c.b_kc) for c in strides} == {(64, 32, False), (64, 32, True), (32, 96, False), (32, 96, True)}
    for c in strides:
        assert c.route == GC.ROWS and c.m == 8193 and c.lda == c.k + 4 and c.ldc == c.n + 3
        assert c.ldb == (c.k + 4 if c.b_kc else c.n + 1)
    off = {c.name: c for c in G.values() if c.name.startswith("rows_off_")}
    assert len(off) == 5 and all(c.route in (GC.TILED_SLOW, GC.TILED_FAST) and (c.n, c.k, c.b_kc) == (64, 32, True) for c in off.values())
    assert off["rows_off_M8191"].route == GC.TILED_FAST and off["rows_off_M8191"].m == GC.SKINNY_MIN_ROWS - 1
    assert all(c.route == GC.TILED_SLOW for n, c in off.items() if n != "rows_off_M8191")
    # the tiled kernel: 4 layouts x fast / slow, the slow form forced by a pointer and by a stride of either operand
    inst = [c for c in G.values() if c.name.startswith("tiled_inst_")]
    assert {(c.a_kc, c.b_kc, c.route) for c in inst} == {(a, b, r) for a, b in GC.LAYOUTS for r in (GC.TILED_SLOW, GC.TILED_FAST)}
    for a, b in GC.LAYOUTS:
        slow = [c for c in inst if (c.a_kc, c.b_kc) == (a, b) and c.route == GC.TILED_SLOW]
        assert sorted((c.a_shift, c.a_pad % 4 != 0, c.b_shift, c.b_pad % 4 != 0) for c in slow) == \
            sorted([(1, False, 0, False), (0, True, 0, False), (0, False, 1, False), (0, False, 0, True)])
    edge = [c for c in G.values() if c.name.startswith("tiled_edge_")]
    assert {(c.m, c.n) for c in edge} == set(GC.TILED_MN) and all(m != n for m, n in GC.TILED_MN)
    assert {v for mn in GC.TILED_MN for v in mn} == {1, 63, 64, 65, 130}
    for mn in GC.TILED_MN:
        assert {c.k for c in edge if (c.m, c.n) == mn} == set(GC.TILED_K)
    for lay in GC.LAYOUTS:
        assert {c.k for c in edge if (c.a_kc, c.b_kc) == lay} == set(GC.TILED_K)
    assert {c.bias for c in edge} == {c.acc for c in edge} == {True, False}
    assert any(c.a_pad and c.b_pad and c.c_pad for c in edge)
    split = [c for c in G.values() if c.name.startswith("tiled_split_")]
    assert {c.splits for c in split if c.ws} >= {7, 8, 9, 17} and {c.splits for c in split if not c.ws} == {1}
    assert all(c.m == c.n <= 64 for c in split)
    assert any(c.ws and c.k % GC.split_plan(c.m, c.n, c.k, True)[1] != 0 for c in split)           # a short last split
    assert any(c.ws and c.splits < GC.pick_splits(c.m, c.n, c.k) for c in split)                  # the rounding drops one
    assert any(c.ws and c.bias and c.acc for c in split) and any(c.ws and not c.bias and not c.acc for c in split)
    assert G["dispatch_wgrad_ws"].route == GC.WGRAD and G["dispatch_wgrad_pad"].route == GC.WGRAD
    assert G["dispatch_wgrad_nows"].route == GC.TILED_FAST and G["dispatch_wgrad_nows"].splits == 1
    assert G["dispatch_wgrad_bias"].route == GC.TILED_FAST and G["dispatch_wgrad_bias"].splits == 52 < GC.pick_splits(64, 32, GC.M_BASE) == 64
    # the streamed weight gradient
    assert {(c.n1, c.n2) for c in W.values() if c.M == GC.M_BASE} == set(GC.WGRAD_SHAPES)
    for s in ((32, 32), (192, 32), (64, 64)):
        assert {c.M for c in W.values() if (c.n1, c.n2) == s} >= set(GC.M_SWEEP)
    for s in ((64, 32), (32, 96)):
        mine = [c for c in W.values() if (c.n1, c.n2) == s]
        assert any((c.g_pad, c.x_pad, c.dw_pad) == (1, 3, 5) for c in mine)
        assert any(not c.db for c in mine) and any(c.acc and c.db for c in mine)
    assert all(GC.wgrad_supported(GC.M_BASE, *a) and GC.wgrad_supported(GC.M_BASE, *b) and (a, b) != GC.WGRAD_PAIR
               for a, b in GC.PAIR_REFUSED)
    # the finish
    assert len(GC.FINISH_BLOCKS) == 20 and len(GC.MIXED_JOBS) == GC.MAX_PARTIAL_JOBS
    for si in range(len(GC.FINISH_SHAPES)):
        flags = [GC.finish_flags(si, bi) for bi in range(len(GC.FINISH_BLOCKS))]
        assert {f[0] for f in flags} == {0, 5} and {f[1] for f in flags} == {f[2] for f in flags} == {True, False}
    kinds = [j[0] for j in GC.MIXED_JOBS]
    assert kinds == [0, 1] * 4 and any(j[1] == 1 for j in GC.MIXED_JOBS)
    first = GC.finish_grid(GC.MIXED_JOBS)
    assert first == sorted(set(first)) and first[1] == 17 and first[-1] > 200       # several workgroups per job


def test_row_counts_reach_the_claimed_plans():
    p = {M: GC.rows_plan(M) for M in GC.M_SWEEP}
    assert [p[M]["tpw"] for M in GC.M_SWEEP] == [1, 1, 1, 2, 3]
    assert 8192 % 32 == 0 and 8193 % 32 == 1 and 8223 % 32 == 31
    assert p[65569]["ntiles"] == 2050 and p[65569]["waves"] == 1025 and p[65569]["waves"] % GC.WAVES == 1   # one live wave
    assert p[131077]["ntiles"] == 4097 and p[131077]["waves"] * 3 - 4097 == 1         # the last wave stops after two tiles
    assert GC.rows_plan(GC.M_BASE)["tpw"] == 1 and GC.M_BASE % 32 == 5
    w = {M: GC.wgrad_plan(M) for M in GC.M_SWEEP}
    assert [w[M]["cpw"] for M in GC.M_SWEEP] == [1, 1, 1, 2, 3]
    assert w[131077]["waves"] * 3 > w[131077]["nchunks"] and w[131077]["waves"] % GC.WAVES != 0   # partly empty last wave / workgroup
    assert w[65569]["waves"] * 2 == w[65569]["nchunks"] and w[65569]["waves"] % GC.WAVES == 1


def test_library_agrees_with_every_case():
    lib = _lib.load()
    for c in GC.GEMM_CASES.values():
        assert _route(lib, c) == c.route == GC.route(*c.route_args()), c.name
        for ws in (False, True):
            assert lib.dfm_gemm_splits(c.m, c.n, c.k, int(ws)) == GC.split_plan(c.m, c.n, c.k, ws)[0], c.name
        if c.route in (GC.TILED_SLOW, GC.TILED_FAST):
            assert c.splits == GC.split_plan(c.m, c.n, c.k, c.ws)[0]
        if c.route == GC.WGRAD:
            assert lib.dfm_gemm_workspace_bytes(c.m, c.n, c.k) >= GC.wgrad_workspace_bytes(c.k, c.m, c.n) > 0
        elif c.ws:
            assert lib.dfm_gemm_workspace_bytes(c.m, c.n, c.k) >= 4 * GC.pick_splits(c.m, c.n, c.k) * c.m * c.n * (c.splits > 1)
    for c in GC.WGRAD_CASES.values():
        assert lib.dfm_weight_grad_partial_blocks(c.M) == GC.wgrad_plan(c.M)["blocks"]
        assert lib.dfm_weight_grad_workspace_bytes(c.M, c.n1, c.n2) == GC.wgrad_workspace_bytes(c.M, c.n1, c.n2) > 0
    assert lib.dfm_weight_grad_workspace_bytes(GC.SKINNY_MIN_ROWS - 1, 32, 32) == 0
    assert lib.dfm_gemm_route(BASE, 32, 1, BASE, 32, 1, 0, 32, 32, 0, 0) == -1 and lib.dfm_gemm_splits(64, 64, 0, 1) == 0
    # each condition of the rows predicate on its own (K-contiguous and K-strided weight)
    ok = dict(a=BASE, lda=32, b=BASE, ldb=32, b_kc=1, m=8192)
    def r(**kw):
        v = {**ok, **kw}
        return lib.dfm_gemm_route(v["a"], v["lda"], 1, v["b"], v["ldb"], v["b_kc"], v["m"], 64, 32, 1, 0)
    assert r() == GC.ROWS
    assert r(a=BASE + 4) == r(lda=33) == r(b=BASE + 8) == r(ldb=34) == GC.TILED_SLOW and r(m=8191) == GC.TILED_FAST
    assert r(b_kc=0, b=BASE + 4, ldb=65) == GC.ROWS        # the W conditions do not apply to the K-strided layout


def test_integer_family_is_exact():
    for c in list(GC.GEMM_CASES.values()) + list(GC.WGRAD_CASES.values()):
        assert "int" in c.families and GC.max_abs_sum(c) < 2 ** 24, c.name
    assert 9 * 131077 < 2 ** 24
    small = [c for c in GC.GEMM_CASES.values() if c.m * c.n * c.k <= 1 << 22]
    assert len(small) > 80
    for c in small:
        inp = GC.gemm_inputs(c, "int")
        for v in inp.values():
            assert v is None or (np.all(v != 0) and np.all(np.abs(v) <= 3) and np.all(v == np.round(v)))
        want = inp["a"].astype(np.int64) @ inp["b"].astype(np.int64).T
        for t in (inp["bias"], inp["c0"]):
            want = want + (t.astype(np.int64) if t is not None else 0)
        ref, A = GC.gemm_ref(inp)
        assert np.array_equal(ref, want.astype(np.float64)) and A.max() <= GC.max_abs_sum(c)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    c = GC.WGRAD_CASES["wgrad_64x32_acc"]
    inp = GC.wgrad_inputs(c, "int")
    dw, db, Adw, Adb = GC.wgrad_ref(inp)
    g, x = inp["g"].astype(np.int64), inp["x"].astype(np.int64)
    assert np.array_equal(dw, (g.T @ x).astype(np.float64)) and np.array_equal(db, g.sum(0).astype(np.float64))
    assert max(Adw.max(), Adb.max()) + 3 <= GC.max_abs_sum(c)


@pytest.mark.parametrize("name", ["wgrad_32x32_M8193", "wgrad_64x32", "wgrad_32x32_M65569"])
def test_restated_blocking_is_the_product(name):
    """The integer family through the restated blocking of the kernels (waves, workgroup tree, finish order): exact, so
    equal to the plain product; and the listed mistakes, applied to it, change the result."""
    c = GC.WGRAD_CASES[name]
    inp = GC.wgrad_inputs(c, "int")
    g, x = inp["g"].astype(np.int64), inp["x"].astype(np.int64)
    want = np.concatenate([(g.T @ x).reshape(-1), g.sum(0)])
    part = GC.wgrad_partials(g, x, c.M, dt=np.int64)
    p = GC.wgrad_plan(c.M)
    assert part.shape == (p["blocks"], c.n1 * c.n2 + c.n1)
    assert np.array_equal(GC.finish_kind0(part), want)
    nw = c.n1 * c.n2
    # the last row dropped
    last = np.concatenate([(g[:-1].T @ x[:-1]).reshape(-1), g[:-1].sum(0)])
    assert np.all(last != want)
    # one 32-row chunk dropped (the second chunk of a wave where a wave has several)
    chunk = 1 if p["cpw"] > 1 else p["nchunks"] // 2
    dropped = GC.finish_kind0(GC.wgrad_partials(g, x, c.M, dt=np.int64, skip_chunk=chunk))
    assert np.any(dropped[:nw] != want[:nw]) and np.any(dropped[nw:] != want[nw:])
    # odd rows missing from db
    even = GC.finish_kind0(GC.wgrad_partials(g, x, c.M, dt=np.int64, db_even_only=True))
    assert np.array_equal(even[:nw], want[:nw]) and np.any(even[nw:] != want[nw:])
    # one partial block skipped in the finish: the last one, and one inside the 8-unrolled stretch
    for blk in (p["blocks"] - 1, 9):
        assert np.any(GC.finish_kind0(part, skip_block=blk) != want)


def test_second_half_of_n192_needs_its_own_bias():
    c = GC.GEMM_CASES["rows_N192_K32_kc0"]
    assert c.bias and GC.GEMM_CASES["rows_N192_K32_M131077"].bias
    inp = GC.gemm_inputs(c, "int", rows=GC.restate_rows(c.m))
    ref, _ = GC.gemm_ref(inp)
    wrong = dict(inp, bias=np.concatenate([inp["bias"][:96], inp["bias"][:96]]))
    bad, _ = GC.gemm_ref(wrong)
    assert np.array_equal(bad[:, :96], ref[:, :96]) and np.any(bad[:, 96:] != ref[:, 96:])
    # and the float32 restatement of the integer family is the reference, bit for bit, in both orders
    for order in ("kernel", "pair"):
        assert np.array_equal(GC.rows_f32(inp, order).astype(np.float64), ref)


def test_finish_restatements_on_integer_partials():
    rng = np.random.default_rng(5)
    for blocks in (1, 5, 37, 416):
        part = GC.values(rng, (blocks, 40), "int").astype(np.int64)
        assert np.array_equal(GC.finish_kind0(part), part.sum(0))
    for blocks in GC.LN_FINISH_BLOCKS:
        part = GC.values(rng, (blocks, 2, 10), "int").astype(np.int64)
        assert np.array_equal(GC.finish_kind1(part), part.sum(0))
    assert 3 * max(GC.FINISH_BLOCKS + GC.LN_FINISH_BLOCKS) + 3 < 2 ** 24


def test_float32_restatement_stays_inside_the_bars():
    """C[kind] is 4 x the worst ratio of the float32 restatement, rounded up: the restatement sits at <= 1 / 4 of every
    bar, and the constants are no looser than the measurement makes them."""
    names = GC.float_cases()
    kinds = {GC.f32_ratio.__name__}          # (keeps the import of the function explicit)
    assert kinds and len(names) >= 50
    worst = GC.worst_ratios()
    print("worst float32 ratios", {k: round(v, 3) for k, v in worst.items()})
    for kind, w in worst.items():
        assert 0 < GC.MARGIN * w <= GC.C[kind], (kind, w)
        assert GC.C[kind] <= 2 * GC.MARGIN * w, f"{kind}: C = {GC.C[kind]} is looser than twice 4 x {w:.3f}"
    doc = GC.__doc__
    for kind, w in worst.items():
        row = re.search(rf"\n\s+{kind}\s+{w:.3f}\s+([\d.]+)\s+([\d.]+)\s", doc)
        assert row, f"the docstring's table row of {kind} is stale"
        assert abs(float(row.group(1)) - GC.MARGIN * w) < 0.01 and float(row.group(2)) == GC.C[kind]
    assert {GC.GEMM_CASES[n].kind if n in GC.GEMM_CASES else "wgrad" for n in names} == set(GC.C)
