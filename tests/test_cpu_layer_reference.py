"""Host-side proof of the layer matrix (tests/layer_cases.py): the case lists reach every branch of the kernels'
index arithmetic that they name, the integer family is exact, the recorded C and T are the measured ones, a float32
restatement of every kernel stays inside every bar, the mistakes the matrix exists for show, and every entry point
refuses bad arguments on the host (fake pointers: nothing is dereferenced or launched)."""
import re
from pathlib import Path

import numpy as np
import pytest

from deepfm_amd import _lib
from tests import gemm_cases as GC
from tests import layer_cases as L
from tests import tower_cases as TC

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "deepfm_amd" / "csrc"
F32, F64 = np.float32, np.float64


def test_constants_equal_the_sources():
    fm, dnn, loss, pred = ((CSRC / n).read_text() for n in ("fm.hip", "dnn_fused.hip", "loss.hip", "predict.hip"))
    assert "dim / 4 <= 64" in fm and "__launch_bounds__(256) void fm_fwd_kernel" in fm
    assert re.search(rf"kRowsPerSlice = {L.BN_ROWS_PER_SLICE};", dnn)
    assert re.search(rf"kFinCols = 16, kFinLanes = {L.BN_FIN_LANES};", dnn)
    assert "features <= 65536" in dnn and "N <= 65536" in dnn.split("#include")[0]
    assert re.search(r"kThreads = 256;", loss) and re.search(r"kPerThread = 4;", loss) and L.BCE_PER_BLOCK == 1024
    assert re.search(rf"kPhThreads = 256, kPhLanes = {L.HEAD_LANES}, kPhRows = kPhThreads / kPhLanes;", pred)
    assert L.HEAD_ROWS == 256 // L.HEAD_LANES and L.EVAL_BK == GC.BK
    assert "mainloop<true, true, FAST, FAST>" in pred
    for args in ((0, 8, True, 3, 8), (1, 8, True, 3, 8), (0, 9, True, 3, 8), (0, 12, True, 3, 10), (0, 8, False, 3, 8)):
        assert L.operand_fast(*args) == GC.operand_fast(*args)


def test_fm_cases_reach_every_branch():
    cs = list(L.FM_CASES.values())
    aligned = [c for c in cs if not c.shift]
    assert {c.D for c in aligned} == set(L.FM_D_SCALAR + L.FM_D_VEC)
    assert {(c.vec, c.lps) for c in aligned if c.vec == 1} == {(1, 1), (1, 2), (1, 4), (1, 8), (1, 64)}
    assert {(c.vec, c.lps) for c in aligned if c.vec == 4} == {(4, p) for p in (1, 2, 4, 8, 16, 32, 64)}
    idle = {c.D for c in aligned if c.vec == 4 and c.D // 4 < c.lps}
    assert {12, 20, 132} <= idle and L.fm_lps(256) == 64 == 256 // 4
    for D in L.FM_D_SCALAR + L.FM_D_VEC:
        per = 256 // L.fm_lps(D)
        assert {c.B for c in aligned if c.D == D and c.F == 5} == {1, per - 1, per + 1, 3 * per + 5} - {0}
    for D in L.FM_F_FULL_AT:
        assert {c.F for c in aligned if c.D == D} == set(L.FM_F)
    assert {F % 4 for F in L.FM_F} == {0, 1, 2, 3} and 39 in L.FM_F
    shifted = [c for c in cs if c.shift]
    assert {c.D for c in shifted} == set(L.FM_SHIFT_D) and all(c.vec == 1 and c.D % 4 == 0 and c.lps == L.pow2_at_least(c.D) for c in shifted)
    assert all(L.fm_refused(D) for D in L.FM_REFUSED_D) and L.fm_refused(68, aligned=False) and not any(L.fm_refused(c.D, not c.shift) for c in cs)
    assert max(c.B * c.F * c.D for c in cs) < 1_200_000


def test_combine_and_copy_cases_reach_every_branch():
    cs = list(L.COMBINE_CASES.values())
    assert {(c.D, c.F) for c in cs} >= {(D, F) for D in L.COMBINE_D for F in L.COMBINE_F}
    assert {c.rows * (c.width // 4) for c in cs if (c.D, c.F) == (4, 1)} >= set(L.COMBINE_THREADS)
    for D, F in ((12, 3), (16, 39)):                       # lanes end just below, on or above 256 and in a ragged fourth workgroup
        lanes = sorted({c.rows * (c.width // 4) for c in cs if (c.D, c.F) == (D, F)})
        assert lanes[0] <= 256 < lanes[-1] and any(-(-t // 256) == 4 and t % 256 for t in lanes)
        assert {c.ld for c in cs if (c.D, c.F) == (D, F)} >= {F * D, F * D + 4, 2 * F * D}
    for D in (12, 16):
        assert {(c.extra, c.fm) for c in cs if c.D == D and c.F == 3 and c.rows == 65} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert any(c.D == 12 and c.fm and c.F > 1 for c in cs) and 12 & 11 != 12 % 12 + 11       # 12 is no power of two
    assert L.COPY_WIDTH == (4, 12, 624) and L.COPY_ROWS == (0, 1, 63, 65, 257) and L.copy_lds(12) == (12, 16, 24)


def test_bn_cases_reach_every_branch():
    assert {L.bn_slices(M) for M in L.BN_M} == {1, 2, 3, 16, 17, 258}
    per_lane = {v for M in L.BN_M for v in L.bn_slices_per_lane(M)}
    assert {0, 1, 2, 17} <= per_lane
    for cases in (L.BN_CASES, L.BN_BWD_CASES):
        plain = [c for c in cases.values() if c.stats == "plain"]
        assert {(c.M, c.N) for c in plain} == set(L.BN_SHAPES)
        assert {c.M for c in plain if c.N in (3, 17)} == set(L.BN_M) and {c.N for c in plain if c.M in (17, 257)} == set(L.BN_N)
        assert {c.p for c in plain} == set(L.BN_P) and {c.salt for c in plain} == set(L.BN_SALTS)
        assert {c.seed for c in plain} == set(L.BN_SEEDS) | {None} and all(c.p == 0 for c in plain if c.seed is None)
        assert {c.running for c in plain} == {True, False}
    assert [L.dropout_thresh(p) for p in L.BN_P] == [0, 1 << 30, 1 << 31, 1] and L.dropout_thresh(2.0 ** -33) == 0
    assert any(N % 256 and N > 256 for N in L.BN_N) and {N % 16 for N in L.BN_N} >= {0, 1, 15}
    row0 = {(c.M, c.stats) for c in L.BN_CASES.values() if c.stats.startswith("row0")}
    assert row0 == {(M, f"row0_{k}") for M in (512, 4096) for k in (10, 100)}
    assert {c.M for c in L.BN_CASES.values() if c.stats == "common"} == {17, 257, 4115}
    for name, c in L.BN_CASES.items():
        if c.stats.startswith("row0"):
            z = L.bn_fwd_inputs(name)["z"].astype(F64)
            off = np.abs(z[0] - z[1:].mean(0)) / z[1:].std(0)
            assert np.all(np.abs(off / float(c.stats[5:]) - 1) < 0.15), off


def test_backward_inputs_stay_off_the_relu_kink():
    for name in L.BN_BWD_CASES:
        assert L.bn_bwd_ref(name)["min_abs_y"] >= TC.KINK_MARGIN, name


def test_bce_eval_head_cases_reach_every_branch():
    assert {L.bce_partials(n) for n in L.BCE_N} == {1, 2, 3, 257} and {n % 4 for n in L.BCE_N} == {0, 1, 3}
    assert {L.bce_partials(n) for n in L.BCE_N if n in (1023, 1024, 1025)} == {1, 2}
    assert {f for f, _ in L.BCE_CASES} == {"normal", "soft", "fixed"} and {n for f, n in L.BCE_CASES if f == "normal"} == set(L.BCE_N)
    fixed = L.bce_inputs("fixed", 22)
    assert set(zip(fixed["z"].tolist(), fixed["y"].tolist())) == {(float(F32(z)), y) for z in L.BCE_FIXED for y in (0.0, 1.0)}
    assert np.exp(F32(-104.0)) == 0 and np.exp(F32(-88.0)) > 0
    soft = L.bce_inputs("soft", 1025)["y"]
    assert ((soft > 0) & (soft < 1)).all() and len(np.unique(soft)) > 1000
    ev = list(L.EVAL_CASES.values())
    assert {c.M for c in ev} == set(L.EVAL_M) and {c.N for c in ev} == set(L.EVAL_N) and {c.K for c in ev} == set(L.EVAL_K)
    assert {(c.M, c.N) for c in ev if c.K == 100} == {(c.M, c.N) for c in ev if c.K == 33} == {(M, N) for M in L.EVAL_M for N in L.EVAL_N}
    fast, slow = [c for c in ev if c.fast], [c for c in ev if not c.fast]
    assert all(c.K % 4 == 0 and c.x_pad in (0, 4) and not c.x_shift and not c.w_shift for c in fast) and {c.x_pad for c in fast} == {0, 4}
    assert {c.K for c in fast} == {K for K in L.EVAL_K if K % 4 == 0}
    why = {("K" if c.K % 4 else "") + ("ldx" if c.ldx % 4 else "") + ("x" if c.x_shift else "") + ("w" if c.w_shift else "") for c in slow}
    assert {"K", "Kldx", "ldx", "x", "w"} <= why and {c.K for c in slow} >= {K for K in L.EVAL_K if K % 4}
    assert {c.bias for c in fast} == {c.bias for c in slow} == {True, False}
    assert {L.eval_chain(K) for K in (1, 32)} == {18} and L.eval_chain(33) == 34
    hd = list(L.HEAD_CASES.values())
    assert {(c.M, c.K) for c in hd} >= {(M, K) for M in L.HEAD_M for K in L.HEAD_K}
    for M in (1, 33, 100):
        assert {c.valid for c in hd if c.M == M and c.K == 36} >= {0, 1, M - 1, M}
    assert len({(c.b, c.fo, c.extra, c.logits) for c in hd if (c.M, c.K, c.valid) == (33, 36, 33)}) == 16
    assert {-(-M // L.HEAD_ROWS) for M in L.HEAD_M} == {1, 2, 4} and {-(-K // 32) for K in L.HEAD_K} == {1, 2, 8}


def test_integer_family_is_exact():
    """The 2^24 bound of every case, and the float32 restatement in the kernel's order equal to the fp64 reference."""
    worst = 0
    for c in L.FM_CASES.values():
        worst = max(worst, L.fm_int_bound(c))
        i = L.fm_inputs(c, "int")
        assert np.abs(i["e"]).min() >= 1 and np.abs(i["e"]).max() <= 3 and {np.sign(v) for v in i["g"]} <= {-1.0, 1.0}
        ref, _ = L.fm_fwd_ref(i["e"])
        assert np.abs(ref).max() * 2 <= L.fm_int_bound(c)
        assert np.array_equal(L.fm_fwd_restate(i["e"], c.vec, c.lps).astype(F64), ref)
        rb, _ = L.fm_bwd_ref(i["e"], i["g"])
        assert np.array_equal(L.fm_bwd_restate(i["e"], i["g"]).astype(F64), rb)
        if c.F == 1:
            assert not rb.any()
    assert worst == 9 * 39 * 39 * 132 + 9 * 39 * 132 and 9 * 39 * 39 * 256 + 9 * 39 * 256 < 2 ** 24      # the cases' largest; F = 39 at D = 256
    for c in L.COMBINE_CASES.values():
        i = L.combine_inputs(c, "int")
        ref, A = L.combine_ref(c, i)
        assert A.max() <= 3 + 3 + 3 * 6 and np.array_equal(L.combine_ref(c, i, F32)[0].astype(F64), ref)
    for c in L.EVAL_CASES.values():
        i = L.eval_inputs(c, "int")
        r = L.eval_ref(c, i, "int")
        assert r["A_z"].max() <= 9 * c.K + 3 < 2 ** 24
        assert np.array_equal(L.eval_restate(c, i)[0].astype(F64), r["z"])
    for c in L.HEAD_CASES.values():
        i = L.head_inputs(c, "int")
        r = L.head_ref(c, i, "int")
        assert r["A"].max() <= 9 * c.K + 9 < 2 ** 24 and not r["bar_logits"].any()
        full = L.Head(c.M, c.K, c.M, c.b, c.fo, c.extra, True)
        assert np.array_equal(L.head_restate(full, i)[0].astype(F64), r["logits"])


def test_recorded_constants_are_the_measured_ones():
    w, t, _ = L.measure()
    assert set(w) == set(L.C) and set(t) == set(L.T) == set(L.T_HOST)
    for k in L.C:
        assert L.C[k] == L.round_up(L.MARGIN * w[k]), (k, w[k])
    for k in L.T:
        assert L.T_HOST[k] == L.round_up(L.MARGIN * t[k], 0.5), (k, t[k])
        assert L.T[k] >= L.T_HOST[k]
    doc = L.__doc__
    for k in L.C:
        row = re.search(rf"^\s+{k}\s+{w[k]:.3f}\s+{L.MARGIN * w[k]:.2f}\s+([\d.]+)\s", doc, re.M)
        assert row and float(row.group(1)) == L.C[k], k


def test_float32_restatements_stay_inside_every_bar():
    """The whole float32 pipeline of each kernel (its own transcendental evaluations included) against the bars the
    GPU test applies, in both orders."""
    for name, c in L.BN_CASES.items():
        i, r = L.bn_fwd_inputs(name), L.bn_fwd_ref(name)
        for o in L.ORDERS:
            m, v = L.bn_stats_restate(i["z"], o)
            ap = L.bn_apply_restate(c, i, m, v)
            got = dict(mean=m, var=v, rstd=ap["rstd"], out=ap["out"], running_mean=ap["running_mean"], running_var=ap["running_var"])
            for k, x in got.items():
                assert L.worst(x, r[k], r["bar_" + k]) <= 1.0, (name, o, k)
            assert not ap["out"][~r["kept"]].any() and (ap["out"][r["kept"] & (r["y"] > r["bar_out"])] > 0).all()
    for fam, n in L.BCE_CASES:
        i, r = L.bce_inputs(fam, n), L.bce_ref(fam, n)
        for o in L.ORDERS:
            loss, dz, part = L.bce_restate(i, o)
            assert L.worst(loss, r["loss"], r["bar_loss"]) <= 1.0 and L.worst(dz, r["dz"], r["bar_dz"]) <= 1.0, (fam, n, o)
            assert part is None or part.size == L.bce_partials(n)
    for c in L.EVAL_CASES.values():
        for fam in ("int", "float"):
            i = L.eval_inputs(c, fam)
            r = L.eval_ref(c, i, fam)
            for o in L.ORDERS:
                assert L.worst(L.eval_restate(c, i, o)[1], r["out"], r["bar_out"]) <= 1.0, (c.name, fam, o)
    for c in L.HEAD_CASES.values():
        i = L.head_inputs(c, "float")
        r = L.head_ref(c, i, "float")
        v = c.valid
        for o in L.ORDERS:
            zl, pr = L.head_restate(c, i, o)
            assert np.isnan(zl[v:]).all() and np.isnan(pr[v:]).all()
            assert L.worst(zl[:v], r["logits"][:v], r["bar_logits"][:v]) <= 1.0 and L.worst(pr[:v], r["probs"][:v], r["bar_probs"][:v]) <= 1.0
            assert ((pr[:v] >= 0) & (pr[:v] <= 1)).all()
    big = [r for c in L.HEAD_CASES.values() if c.fo and c.M >= 4 for r in [L.head_ref(c, L.head_inputs(c, "float"), "float")["logits"][:4]]]
    assert big and all(np.all(np.abs(np.abs(z) - np.abs(L.HEAD_EXTREME)) < 12) for z in big)


def test_sums_about_row_0_miss_the_bar():
    """The statistics as dnn_fused.hip formed them before this matrix (sums about row 0) against the plain family's
    bar: outside it in every row-0 case, inside it where row 0 is an ordinary row."""
    _, _, row0 = L.measure()
    for (order, name), ratio in row0.items():
        if order == "shifted":
            assert ratio > L.C["bn_stats"], (name, ratio)
        else:
            assert ratio <= L.C["bn_stats"] / L.MARGIN + 1e-9, (order, name, ratio)
    assert row0[("shifted", "M4096_N3_row0_100_pq_s11_23_r1")] > 100 * L.C["bn_stats"]
    name = next(n for n, c in L.BN_CASES.items() if (c.M, c.N, c.stats) == (257, 17, "plain"))
    i, r = L.bn_fwd_inputs(name), L.bn_fwd_ref(name)
    m, v = L.bn_stats_restate(i["z"], "shifted")
    assert L.worst(m, r["mean"], r["bar_mean"]) <= 1.0 and L.worst(v, r["var"], r["bar_var"]) <= 1.0


def test_statistics_do_not_depend_on_the_size_of_the_mean():
    """The kernel's order (moments of z - the first slice's mean) at |mean| / sigma = 5e2, 5e3 and 5e4 stays inside the
    one statistics bar; slice means of z itself would lose it in proportion."""
    rng = np.random.default_rng(11)
    M, N = 257, 17
    for mean in (50.0, 500.0, 5000.0):
        z = (rng.standard_normal((M, N)) * 0.1 + mean).astype(F32)
        z64 = z.astype(F64)
        mu, var = z64.mean(0), z64.var(0)
        m, v = L.bn_stats_restate(z)
        n = L.bn_chain(M)
        assert L.worst(m, mu, L.bar(np.abs(z64).mean(0), n, L.C["bn_stats"])) <= 1.0 / L.MARGIN, mean
        assert L.worst(v, var, L.bar(var, n, L.C["bn_stats"])) <= 1.0 / L.MARGIN, mean


def _fm(D, F):
    return next(c for c in L.FM_CASES.values() if (c.D, c.F) == (D, F) and not c.shift and c.B > 1)


def test_listed_mistakes_show():
    """Each mistake moves the integer family off equality (the float family, where there is no integer one: outside
    the bar)."""
    c = _fm(16, 5)
    i = L.fm_inputs(c, "int")
    assert not np.array_equal(L.fm_fwd_restate(i["e"], c.vec, c.lps, F64, mistake="drop_last_field"), L.fm_fwd_ref(i["e"])[0])
    assert not np.array_equal(L.fm_bwd_restate(i["e"], i["g"], F64, mistake="drop_last_field"), L.fm_bwd_ref(i["e"], i["g"])[0])
    for D in (12, 20, 132):                                   # a sample's idle-lane chunk read
        c = _fm(D, 5)
        i = L.fm_inputs(c, "int")
        bad = L.fm_fwd_restate(i["e"], c.vec, c.lps, F64, mistake="idle_lane")
        assert (bad != L.fm_fwd_ref(i["e"])[0]).mean() > 0.9
        assert np.array_equal(L.fm_fwd_restate(i["e"], c.vec, c.lps, F64), L.fm_fwd_ref(i["e"])[0])
    c = next(c for c in L.COMBINE_CASES.values() if c.D == 12 and c.F == 3 and c.fm)
    i = L.combine_inputs(c, "int")
    assert not np.array_equal(L.combine_ref(c, i, mistake="mask")[0], L.combine_ref(c, i)[0])
    c16 = next(c for c in L.COMBINE_CASES.values() if c.D == 16 and c.F == 3 and c.fm)
    i16 = L.combine_inputs(c16, "int")
    assert np.array_equal(L.combine_ref(c16, i16, mistake="mask")[0], L.combine_ref(c16, i16)[0])     # a mask at 16
    # a skipped last slice (forward statistics and backward sums), a mask built with the wrong salt
    name = next(n for n, c in L.BN_CASES.items() if (c.M, c.N, c.stats) == (257, 17, "plain"))
    c, i, r = L.BN_CASES[name], L.bn_fwd_inputs(name), L.bn_fwd_ref(name)
    m, v = L.bn_stats_restate(i["z"], mistake="skip_last_slice")
    assert L.worst(m, r["mean"], r["bar_mean"]) > 1.0 and L.worst(v, r["var"], r["bar_var"]) > 1.0
    for p in (0.25, 0.5):
        salted = next(n for n, k in L.BN_CASES.items() if k.p == p and k.M * k.N >= 256)
        cs, si, sr = L.BN_CASES[salted], L.bn_fwd_inputs(salted), L.bn_fwd_ref(salted)
        ok = L.bn_apply_restate(cs, si, sr["mean"], sr["var"])["out"]
        bad = L.bn_apply_restate(cs, si, sr["mean"], sr["var"], salt=cs.salt + 1)["out"]
        assert not ok[~sr["kept"]].any() and bad[~sr["kept"]].any()
    cb, ib, rb = L.BN_BWD_CASES[name], L.bn_bwd_inputs(name), L.bn_bwd_ref(name)
    q, s, dz = L.bn_bwd_restate(cb, ib, mistake="skip_last_slice")
    n = L.bn_chain(cb.M)
    assert L.worst(q, rb["d_gamma"], L.bar(rb["A_gamma"], n, L.C["bn_bwd"])) > 1.0
    assert L.worst(s, rb["d_beta"], L.bar(rb["A_beta"], n, L.C["bn_bwd"])) > 1.0
    assert L.worst(dz, rb["dz"], L.bar(rb["A_dz"], n + 3, L.C["bn_bwd"])) > 1.0
    # a skipped 257th partial
    nb = 256 * 1024 + 7
    for fam in ("normal", "soft"):
        loss, _, _ = L.bce_restate(L.bce_inputs(fam, nb), mistake="skip_partial_256")
        assert L.worst(loss, L.bce_ref(fam, nb)["loss"], L.bce_ref(fam, nb)["bar_loss"]) > 1.0
    # a dropped k tail: z moves by at least 1, which the epilogue's bar cannot hide
    for c in (c for c in L.EVAL_CASES.values() if c.K == 100 and c.M * c.N >= 64):
        i = L.eval_inputs(c, "int")
        r = L.eval_ref(c, i, "int")
        z, out = L.eval_restate(c, i, mistake="drop_k_tail")
        assert not np.array_equal(z.astype(F64), r["z"]) and L.worst(out, r["out"], r["bar_out"]) > 1.0, c.name
    # valid ignored
    c = next(c for c in L.HEAD_CASES.values() if 0 < c.valid < c.M and c.logits)
    zl, pr = L.head_restate(c, L.head_inputs(c, "int"), mistake="valid_ignored")
    assert not np.isnan(zl[c.valid:]).any() and not np.isnan(pr[c.valid:]).any()


# ---- host refusals ----------------------------------------------------------------------------------------------
P, Q = 0x10000, 0x10004                    # a 16-byte aligned fake device address and one a float behind it
REFUSED = {
    "dfm_fm_forward": [(None, 4, 4, 16, P), (P, 4, 4, 16, None), (P, 4, 0, 16, P), (P, 4, 4, 0, P), (P, -1, 4, 16, P),
                       (P, 4, 4, 65, P), (P, 4, 4, 67, P), (P, 4, 4, 260, P), (Q, 4, 4, 68, P), (Q, 4, 4, 256, P)],
    "dfm_fm_backward": [(None, P, 4, 4, 16, P), (P, None, 4, 4, 16, P), (P, P, 4, 4, 16, None), (P, P, 4, 0, 16, P),
                        (P, P, 4, 4, 65, P), (P, P, 4, 4, 67, P), (P, P, 4, 4, 260, P), (Q, P, 4, 4, 68, P), (P, P, 4, 4, 68, Q)],
    "dfm_embedding_grad_combine": [(None, 64, P, P, P, P, 4, 4, 16, P), (P, 64, P, P, P, P, 4, 4, 16, None),
                                   (P, 24, P, P, P, P, 4, 4, 6, P), (P, 60, P, P, P, P, 4, 4, 16, P), (P, 66, P, P, P, P, 4, 4, 16, P),
                                   (P, 64, P, P, None, P, 4, 4, 16, P), (P, 64, P, P, P, None, 4, 4, 16, P),
                                   (P, 64, P, P, P, P, 4, 0, 16, P), (P, 64, P, P, P, P, -1, 4, 16, P),
                                   (Q, 64, P, P, P, P, 4, 4, 16, P), (P, 64, Q, P, P, P, 4, 4, 16, P), (P, 64, P, P, Q, P, 4, 4, 16, P),
                                   (P, 64, P, P, P, Q, 4, 4, 16, P), (P, 64, P, P, P, P, 4, 4, 16, Q)],
    "dfm_copy_2d": [(None, 8, P, 8, 4, 8), (P, 8, None, 8, 4, 8), (P, 8, P, 8, 4, 6), (P, 8, P, 8, 4, 0), (P, 4, P, 8, 4, 8),
                    (P, 8, P, 4, 4, 8), (P, 10, P, 8, 4, 8), (P, 8, P, 10, 4, 8), (Q, 8, P, 8, 4, 8), (P, 8, Q, 8, 4, 8),
                    (P, 8, P, 8, -1, 8)],
    "dfm_bn_relu_dropout_forward": [(None, 8, 4, P, P, P, P, P, 0.1, 1e-5, 0.0, P, 1, P, P, P), (P, 8, 4, P, P, P, P, P, 0.1, 1e-5, 0.0, P, 1, None, P, P),
                                    (P, 8, 4, P, P, P, P, P, 0.1, 1e-5, 0.0, P, 1, P, None, P), (P, 8, 4, P, P, P, P, P, 0.1, 1e-5, 0.0, P, 1, P, P, None),
                                    (P, 8, 4, None, P, P, P, P, 0.1, 1e-5, 0.0, P, 1, P, P, P), (P, 0, 4, P, P, P, P, P, 0.1, 1e-5, 0.0, P, 1, P, P, P),
                                    (P, 8, 0, P, P, P, P, P, 0.1, 1e-5, 0.0, P, 1, P, P, P), (P, 8, 65537, P, P, P, P, P, 0.1, 1e-5, 0.0, P, 1, P, P, P),
                                    (P, 8, 4, P, P, P, P, P, 0.1, 1e-5, -0.1, P, 1, P, P, P), (P, 8, 4, P, P, P, P, P, 0.1, 1e-5, 1.0, P, 1, P, P, P),
                                    (P, 8, 4, P, P, P, P, P, 0.1, 1e-5, 0.5, None, 1, P, P, P)],
    "dfm_bn_relu_dropout_backward": [(None, P, P, P, P, 8, 4, 0.0, P, 1, P, P, P, P), (P, P, None, P, P, 8, 4, 0.0, P, 1, P, P, P, P),
                                     (P, P, P, P, P, 8, 4, 0.0, P, 1, None, P, P, P), (P, P, P, P, P, 8, 4, 0.0, P, 1, P, None, P, P),
                                     (P, P, P, P, P, 8, 4, 0.0, P, 1, P, P, None, P), (P, P, P, P, P, 8, 4, 0.0, P, 1, P, P, P, None),
                                     (P, P, P, P, P, 0, 4, 0.0, P, 1, P, P, P, P), (P, P, P, P, P, 8, 0, 0.0, P, 1, P, P, P, P),
                                     (P, P, P, P, P, 8, 65537, 0.0, P, 1, P, P, P, P), (P, P, P, P, P, 8, 4, 1.0, P, 1, P, P, P, P),
                                     (P, P, P, P, P, 8, 4, -0.1, P, 1, P, P, P, P), (P, P, P, P, P, 8, 4, 1.5, P, 1, P, P, P, P),
                                     (P, P, P, P, P, 8, 4, 0.5, None, 1, P, P, P, P)],
    "dfm_bce_with_logits": [(P, P, 0, P, P, P), (P, P, -3, P, P, P), (None, P, 8, P, P, P), (P, None, 8, P, P, P), (P, P, 8, None, P, P),
                            (P, P, 8, P, None, P), (P, P, 8, P, P, None)],
    "dfm_linear_bn_eval": [(None, 8, P, P, 4, 4, 8, P, P, P, P, 1e-5, P), (P, 8, None, P, 4, 4, 8, P, P, P, P, 1e-5, P),
                           (P, 8, P, P, 4, 4, 8, None, P, P, P, 1e-5, P), (P, 8, P, P, 4, 4, 8, P, P, P, None, 1e-5, P),
                           (P, 8, P, P, 4, 4, 8, P, P, P, P, 1e-5, None), (P, 8, P, P, 0, 4, 8, P, P, P, P, 1e-5, P),
                           (P, 8, P, P, 4, 0, 8, P, P, P, P, 1e-5, P), (P, 8, P, P, 4, 4, 0, P, P, P, P, 1e-5, P),
                           (P, 7, P, P, 4, 4, 8, P, P, P, P, 1e-5, P), (P, 8, P, P, 1 << 30, 4, 8, P, P, P, P, 1e-5, P)],
    "dfm_predict_head": [(None, 8, 8, P, P, P, P, 8, P, P), (P, 8, 8, None, P, P, P, 8, P, P), (P, 8, 8, P, P, P, P, 8, P, None),
                         (P, 0, 8, P, P, P, P, 0, P, P), (P, 8, 8, P, P, P, P, 9, P, P), (P, 8, 8, P, P, P, P, -1, P, P),
                         (P, 8, 6, P, P, P, P, 8, P, P), (P, 8, 0, P, P, P, P, 8, P, P), (Q, 8, 8, P, P, P, P, 8, P, P),
                         (P, 8, 8, Q, P, P, P, 8, P, P)],
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_host_refusals(name):
    lib = _lib.load()
    for k, args in enumerate(REFUSED[name]):
        assert len(args) + 1 == len(_lib.SIGNATURES[name][1]), (name, k)
        # a refusal of another entry point first, so that the message read below is this call's
        if name == "dfm_bce_with_logits":
            assert lib.dfm_copy_2d(P, 8, P, 8, 4, 6, None) == 1
        else:
            assert lib.dfm_bce_with_logits(P, P, 0, P, P, P, None) == 1
        before = lib.dfm_last_error()
        assert getattr(lib, name)(*args, None) == 1, (name, k, args)               # DFM_ERR_INVALID
        assert lib.dfm_last_error() and lib.dfm_last_error() != before, (name, k)


def test_empty_batches_return_ok_without_a_launch():
    lib = _lib.load()
    assert lib.dfm_fm_forward(P, 0, 4, 16, P, None) == 0 and lib.dfm_fm_backward(P, P, 0, 4, 16, P, None) == 0
    assert lib.dfm_embedding_grad_combine(P, 64, P, P, P, P, 0, 4, 16, P, None) == 0
    assert lib.dfm_copy_2d(P, 8, P, 8, 0, 8, None) == 0
