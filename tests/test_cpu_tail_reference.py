"""CPU: the fp64 restatements of the training step's tail (tests/helpers.py::tail_*_fp64) agree with independent
sources (the oracle's row reduction, Adam and clip coefficient; torch.optim on float64 tensors), every case of the GPU
matrix (tests/tail_cases.py) reaches the branch it claims and the lists cover every branch, and a plain float32
implementation of each operation chain stays inside the bar of every output at every case — so that
tests/test_gpu_tail_matrix.py needs no exclusions.  No GPU."""
import itertools

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests import tail_cases as T
from tests.helpers import (assert_close, tail_clip_fp64, tail_dense_prepare_fp64, tail_merge_fp64, tail_rowgrad_fp64,
                           tail_rule_fp64, tail_sq_fp64)

TIGHT = dict(rtol=1e-12, atol_scale=1e-14)


# ---- the references against independent sources --------------------------------------------------------------------
@pytest.mark.parametrize("n,vocab,D", [(300, 40, 8), (1000, 5000, 12)])
def test_rowgrad_reference_against_the_oracle(n, vocab, D):
    rng = np.random.default_rng([n, vocab, D])
    ids = rng.integers(0, vocab, n).astype(np.int64)
    # integers / 8: every partial sum is exact in fp32, so the oracle's fp32 sums equal the fp64 ones
    g2 = (rng.integers(-64, 64, (n, D)) / 8.0).astype(np.float32)
    g1 = (rng.integers(-64, 64, n) / 8.0).astype(np.float32)
    ref = tail_rowgrad_fp64(ids, g2, g1)
    for fn in (O.rowsparse_from_batch, O.rowsparse_reduce_fast):
        u, r2, r1 = fn(ids, g2, g1)
        assert np.array_equal(u, ref["rows"])
        assert np.array_equal(r2.astype(np.float64), ref["g2"]) and np.array_equal(r1.astype(np.float64), ref["g1"])
    assert np.array_equal(ref["count"], np.bincount(ids, minlength=vocab)[ref["rows"]])
    s2, s1 = T.seq_sum_f32(ids, g2, g1)
    assert np.array_equal(s2, r2) and np.array_equal(s1, r1)
    # generic values: within fp32 rounding of the oracle's ordered fp32 sum
    g2 = rng.standard_normal((n, D)).astype(np.float32)
    ref = tail_rowgrad_fp64(ids, g2, g1)
    u, r2, _ = O.rowsparse_from_batch(ids, g2, g1)
    assert (np.abs(r2 - ref["g2"]) <= ref["count"][:, None] * T.U * ref["abs2"]).all()
    assert np.array_equal(T.seq_sum_f32(ids, g2, g1)[0], r2)


def test_merge_reference_against_a_dictionary_merge():
    """tail_merge_fp64 against the definition written with dictionaries: the lowest list owns the row."""
    rng = np.random.default_rng(5)
    L, S, D, V = 4, 2, 4, 60
    rows = np.zeros((L, S, T.CH), dtype=np.int32)
    num = np.zeros((L, S), dtype=np.int32)
    for l, s in itertools.product(range(L), range(S)):
        r = np.sort(rng.choice(V, size=int(rng.integers(0, 30)), replace=False))
        rows[l, s, :r.size], num[l, s] = r, r.size
    g2, g1 = rng.standard_normal((L, S, T.CH, D)), rng.standard_normal((L, S, T.CH))
    w2, w1 = [rng.standard_normal((V, D)) for _ in range(S)], [rng.standard_normal(V) for _ in range(S)]
    ref = tail_merge_fp64(rows, num, g2, g1, w2, w1, 0.25, 0.01)
    for s in range(S):
        total, first = {}, {}
        for l in range(L):
            for u in range(num[l, s]):
                r = int(rows[l, s, u])
                first.setdefault(r, l)
                total[r] = total.get(r, 0.0) + g2[l, s, u]
        for l in range(L):
            for u in range(num[l, s]):
                r = int(rows[l, s, u])
                assert ref["owner"][l, s, u] == int(first[r] == l)
                if first[r] == l:
                    assert_close(ref["g2"][l, s, u], 0.25 * total[r] + 0.02 * w2[s][r], what="merged", **TIGHT)
                else:
                    assert np.isnan(ref["g2"][l, s, u]).all()
            assert (ref["owner"][l, s, num[l, s]:] == -1).all()


def test_dense_prepare_and_norm_references():
    rng = np.random.default_rng(6)
    n = 48
    g, p = rng.standard_normal(n), rng.standard_normal(n)
    ga = rng.standard_normal((3, n))
    slab = rng.standard_normal((5, 16))
    out, absum, terms = tail_dense_prepare_fp64(g, p, 32, 0.01, [(16, slab)], ga, 1.0 / 3)
    want = ga.mean(0)
    want[16:32] += slab.sum(0)
    want[:32] += 0.02 * p[:32]
    assert_close(out, want, what="dense prepare", **TIGHT)
    assert (terms == np.r_[np.full(16, 5), np.full(16, 10), np.full(16, 4)]).all() and (absum >= np.abs(out)).all()
    out, _, terms = tail_dense_prepare_fp64(g, p, 0, 0.01)
    assert np.array_equal(out, g) and (terms == 1).all()
    assert abs(tail_sq_fp64(g, [np.nan, 2.0]) - (float((g ** 2).sum()) + 4.0)) < 1e-12
    for total, max_norm in ((4.0, 1.0), (4.0, 3.0), (0.0, 1.0), (1e-3, 0.5)):
        assert abs(tail_clip_fp64(total, max_norm) - float(O.clip_coef(total, max_norm))) <= 2 * T.U
    assert tail_clip_fp64(4.0, 0.0) == 1.0 and tail_clip_fp64(4.0, 3.0) == 1.0


def _hyper64():
    return {k: float(v) for k, v in T.HYPER.items()}


@pytest.mark.parametrize("rule", T.RULES)
def test_rule_reference_against_torch_optim(rule):
    """t steps from zero state with the same gradients: torch.optim on float64 CPU tensors against t applications of
    tail_rule_fp64, compared at every step count of the matrix (one run of 100000 steps, checked on its way)."""
    h, lr = _hyper64(), float(T.LR)
    rng = np.random.default_rng(7)
    w0, g = rng.standard_normal(8), rng.standard_normal(8)
    g[0] = 0.0
    p = torch.tensor(w0.copy(), dtype=torch.float64, requires_grad=True)
    if rule == "adam":
        opt = torch.optim.Adam([p], lr=lr, betas=(h["b1"], h["b2"]), eps=h["eps"])
    elif rule == "adamw":
        opt = torch.optim.AdamW([p], lr=lr, betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    else:
        opt = torch.optim.SGD([p], lr=lr, momentum=h["momentum"])
    grad = torch.from_numpy(g.copy())
    w, m, v = w0.copy(), np.zeros(8), np.zeros(8)
    assert max(T.APPLY_T) == 100000
    for t in range(1, max(T.APPLY_T) + 1):
        p.grad = grad
        opt.step()
        w, m, v = tail_rule_fp64(rule, w, m, v, g, t, T.LR, T.HYPER)
        if t in T.APPLY_T:
            assert_close(w, p.detach().numpy(), what=f"{rule} t={t}", rtol=1e-11, atol_scale=1e-13)
            if rule in ("adam", "sgd"):
                assert w[0] == w0[0], "g = 0 from zero state does not move the weight"


def test_adam_reference_against_the_oracle():
    rng = np.random.default_rng(8)
    w, m, g = (rng.standard_normal(64).astype(np.float32) for _ in range(3))
    v = (rng.standard_normal(64) ** 2).astype(np.float32)
    for t in T.APPLY_T:
        wo, mo, vo = w.copy(), m.copy(), v.copy()
        O.adam_update(wo, mo, vo, g, t, float(T.LR), float(T.HYPER["b1"]), float(T.HYPER["b2"]), float(T.HYPER["eps"]))
        r = T.rule_check("adam", w, m, v, g, t, T.LR, None, wo, mo, vo)
        assert max(r.values()) <= 1.0, (t, r)


# ---- reach: every case takes the branch it claims, and the lists cover every branch ------------------------------
def test_rowgrad_cases_cover_every_branch():
    reach = {c: T.rowgrad_reach(*c) for c in T.ROWGRAD_CASES}
    assert {D for D, _ in T.ROWGRAD_CASES if T.is_coop(D)} == {4, 8, 16, 32, 64, 128, 256}
    assert {D // 4 for D in T.COOP_D} == {1, 2, 4, 8, 16, 32, 64}
    assert {D for D, _ in T.ROWGRAD_CASES if not T.is_coop(D)} == {12, 20, 24, 40}
    for (D, kind), r in reach.items():
        assert r["coop"] == (256 % (D // 4) == 0) and not r["map_identity"] and r["chunks"] == 2 and r["tail"] == 37
        if kind == "mixed":
            inp = T.rowgrad_inputs(D, kind)
            count = np.bincount(inp["ids"][0, :T.CH])[5:10]
            assert tuple(count) == T.MIXED_RUNS == (300, 65, 64, 9, 8) and (inp["ids"][0, :T.CH] == 0).sum() == 3
            assert {"<=8", "<=64", "<=2048"} <= r["classes"]
        assert r["split_exact"] == (kind == "split2049"), "num_uniq == CH - kSplitRun exactly, with a split run"
        assert r["split"] == (kind in ("split2049", "run4096"))
        assert r["unsplit_2048"] == (kind == "run2048")
    for D in T.COOP_D:        # every run-length class, the exact split boundary and the unsplit 2048 at every coop width
        rs = [reach[(D, k)] for k in T.ROWGRAD_KINDS]
        assert set().union(*[r["classes"] for r in rs]) == {"<=8", "<=64", "<=2048", ">2048"}
        assert any(r["split_exact"] for r in rs) and any(r["unsplit_2048"] for r in rs)
    for D in T.NONCOOP_D:     # the sequential path at every run length it can meet
        assert {"<=8", "<=64", "<=2048"} <= reach[(D, "mixed")]["classes"] and not reach[(D, "mixed")]["split"]
    assert len(T.ROWGRAD_CASES) == 7 * 4 + 4


def test_dense_field_cases_cover_the_issue():
    assert {c for c in T.DENSE_FIELD_CASES if c[1] != 100} == set(itertools.product((4, 12, 16), (1, 255, 256, 257, 1000)))
    assert {c[0] for c in T.DENSE_FIELD_CASES if c[1] == 100} == {4, 12, 16}
    assert T.DENSE_ND == (1, 3) and T.dense_modes(1000) == ("inplace", 1, 3) and T.dense_modes(100) == (64,)
    want, _ = T.dense_field_expect(4, 100, 3, 64)
    live = ~np.isnan(want)
    assert (live == live[0]).all() and (want[50:][live[50:]] == 0).all() and (want[49][live[49]] != 0).all()
    assert sorted(T.DENSE_POS + T.DENSE_SPARSE_POS) != list(range(T.DENSE_F))      # one schema position is nobody's
    for D, nd in itertools.product(T.DENSE_D, T.DENSE_ND):
        elems, lay = T.dense_grad_layout(D, nd)
        used = np.zeros(elems, dtype=int)
        for w2, b2, w1, b1 in lay:
            used[w2:w2 + D] += 1; used[b2:b2 + D] += 1; used[w1] += 1; used[b1] += 1
        assert used.max() == 1 and (used == 0).any()


def test_merge_cases_cover_every_branch():
    cases = T.MERGE_CASES
    for name, idx, values in (("L", 0, {1, 2, 3, 5}), ("S", 1, {1, 3}), ("D", 2, {4, 12, 16, 256}),
                              ("packed", 3, {False, True}), ("l2", 4, {0.0, 0.01}), ("scale 1/L", 5, {False, True})):
        assert {c[idx] for c in cases} == values, name
        for D in (4, 12, 16):            # ... and each value at every width the rows can straddle workgroups at
            if name not in ("D",):
                assert {c[idx] for c in cases if c[2] == D} == values, (name, D)
    assert all(c[1] == 1 and c[0] <= 2 for c in cases if c[2] == 256)
    reach = [T.merge_reach(c) for c in cases]
    assert all(r["sorted"] and r["every_list"] and r["first_row"] and r["last_row"] for r in reach)
    for feature in ("last_only", "lists_0_2_only", "lists_1_3_only", "empty_list", "full_list", "search", "match"):
        assert any(r[feature] for r in reach), feature
        assert any(r[feature] for r, c in zip(reach, cases) if c[2] == 12), (feature, "D = 12")
    for r, c in zip(reach, cases):
        assert r["search"] == (c[0] >= 2) and r["match"] == (c[0] >= 3)            # dfm_step_prepare: match for L > 2
        assert r["lists_0_2_only"] == (c[0] >= 3) and r["lists_1_3_only"] == (c[0] >= 5)
        assert r["full_list"] == (c[0] >= 2) and r["empty_list"] == (c[1] == 3)
        m = T.merge_inputs(c)
        assert (m["grad_scale"] == np.float32(1.0 / c[0])) if c[5] else m["grad_scale"] == 1
        rs, _ = T.packed_layout(c[2])
        assert rs == 64 or c[2] == 256


def test_dense_prepare_cases_cover_every_branch():
    cases = T.DENSE_PREPARE_CASES
    reach = [T.dense_prepare_reach(c) for c in cases]
    assert {c["n"] for c in cases} == {4, 1023, 1024, 1025, 1027, 4112}
    for n in T.DENSE_N:
        assert {c["n_l2"] for c in cases if c["n"] == n} >= {0, 16 if n >= 16 else 0, n // 16 * 16}
    assert all(c["n_l2"] % 16 == 0 and c["n_l2"] <= c["n"] for c in cases)
    assert {len(c["slabs"]) for c in cases} == {0, 1, 2}
    assert {s[2] for c in cases for s in c["slabs"]} == {1, 7, 8, 9, 17}
    for f in ("vector", "scalar_tail", "unrolled", "unrolled_exact", "remainder", "remainder_only", "slab_at_0",
              "slab_at_end", "gathered", "l2_all"):
        assert any(r[f] for r in reach), f
    assert any(r["scalar_tail"] and r["slab_at_0"] for r in reach), "slabs beside the scalar tail"
    assert any(r["unrolled"] and r["remainder"] for r in reach) and any(r["unrolled_exact"] for r in reach)
    assert {r["blocks"] for r in reach} >= {1, 2, 5}
    assert not any(r["scalar_tail"] and not r["vector"] for r in reach if r["blocks"] > 1)
    assert {(c["world"], c["pad"]) for c in cases if c["world"] and not c["slabs"]} == set(itertools.product((1, 2, 3), (0, 4)))
    assert {(c["world"], c["pad"]) for c in cases if c["world"] and c["slabs"] and c["n_l2"]} == set(itertools.product((1, 2, 3), (0, 4)))
    for c in cases:
        for off, elems, splits in c["slabs"]:
            assert off % 16 == 0 and elems % 4 == 0 and off + elems <= c["n"]
        if c["world"]:
            assert c["n"] % 4 == 0 and np.isnan(T.dense_prepare_inputs(c)["gathered"][:, c["n"]:]).all()
    assert len({T.dense_case_id(c) for c in cases}) == len(cases)
    assert T.FINALIZE_N == (0, 1, 1023, 1024, 1025, 5000)


def test_apply_cases_cover_every_rule_and_entry():
    cases = T.APPLY_CASES
    assert {(c["rule"], c["t"]) for c in cases} >= set(itertools.product(("adam", "adamw", "sgd"), (1, 2, 10, 1000, 100000)))
    assert T.APPLY_ENTRIES == ("dfm_step_apply", "dfm_step_dense_apply", "dfm_step_apply_plan")
    assert {(c["rule"], e) for c in cases for e in c["entries"]} == set(itertools.product(T.RULES, T.APPLY_ENTRIES))
    for c in cases:           # test_apply launches what a case lists: every case, all three, the grouped apply first
        assert c["entries"] == T.APPLY_ENTRIES, T.apply_case_id(c)
    for rule in T.RULES:      # ... at every width and both key widths
        mine = [c for c in cases if c["rule"] == rule]
        assert {c["D"] for c in mine} == {4, 12, 16, 256} and {c["n"] for c in mine} >= {1, 255, 256, 257, 1025}
        assert {c["clip"] for c in mine} == {False, True} and {c["zero_grad"] for c in mine} == {0, 1}
        assert {c["packed"] for c in mine} == {False, True} and {c["batch"] for c in mine} == {1000, 4133}
        assert {T.apply_key_is_narrow(c) for c in mine} == {False, True}
    assert {c["n"] for c in cases} == {1, 255, 256, 257, 1025}
    assert T.NARROW_VOCAB == 1000 and T.WIDE_VOCAB == (1 << 20) - 1
    assert T.RULE_KIND == {"adam": 0, "adamw": 1, "sgd": 2}
    for c in cases:
        a = T.apply_inputs(c)
        assert a["ids_stride"] > c["batch"] and max(a["vocab"]) == a["V"]
        assert (a["flag"][:, :, :200] == 0).any() and (a["flag"][np.arange(T.CH)[None, None, :] >= a["num"][:, :, None]] == 1).all()
        T.apply_owned(c)                                       # (asserts that the owned rows are distinct)
    assert len({T.apply_case_id(c) for c in cases}) == len(cases)


# ---- the bars hold for a plain float32 implementation, at every case ---------------------------------------------
def _note(name, r):
    print(f"TAIL-RATIO cpu {name}: {r:.3f}")         # (pytest -s shows the worst error / bar of every output)
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("case", T.ROWGRAD_CASES, ids=lambda c: f"D{c[0]}-{c[1]}")
def test_bars_hold_rowgrad(case):
    for e, (g2, g1) in zip(T.rowgrad_expect(*case), T.emu_rowgrad(*case)):
        _note("row gradients", T.rowgrad_check(e, g2, g1))


@pytest.mark.parametrize("case", T.DENSE_FIELD_CASES, ids=lambda c: f"D{c[0]}-B{c[1]}")
def test_bars_hold_dense_fields(case):
    for nd, mode in itertools.product(T.DENSE_ND, T.dense_modes(case[1])):
        want, bar = T.dense_field_expect(*case, nd, mode)
        _note("DENSE-field gradients", T.dense_field_check(want, bar, T.emu_dense_field(*case, nd, mode)))


@pytest.mark.parametrize("case", T.MERGE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_bars_hold_merge(case):
    own, g2, g1 = T.emu_merge(case)
    r2, r1 = T.merge_check(case, own, g2, g1)
    _note("merged row_g2", r2)
    _note("merged row_g1", r1)
    live = T.merge_expect(case)["owner"] == 1
    got = T.emu_sq(np.concatenate([g2[live].reshape(-1), g1[live]]))
    _note("row |g|^2", T.ratio(got - tail_sq_fp64(g2[live], g1[live]), T.sq_bar(np.concatenate([g2[live].reshape(-1), g1[live]]))))


@pytest.mark.parametrize("case", T.DENSE_PREPARE_CASES, ids=T.dense_case_id)
def test_bars_hold_dense_prepare(case):
    want, bar = T.dense_prepare_expect(case)
    got = T.emu_dense_prepare(case)
    _note("dense prepare g", T.ratio(got - want, bar))
    _note("dense |g|^2", T.ratio(T.emu_sq(got) - tail_sq_fp64(got), T.sq_bar(got)))


@pytest.mark.parametrize("n", T.FINALIZE_N)
def test_bars_hold_finalize(n):
    for max_norm in T.finalize_max_norms(n):
        total, bar_t, clip, bar_c = T.finalize_expect(n, max_norm)
        tot, c = T.emu_finalize(n, max_norm)
        _note("norm total", T.ratio(tot - total, bar_t))
        _note("clip coefficient", T.ratio(c - clip, bar_c))
    assert T.finalize_expect(n, T.finalize_max_norms(n)[1])[2] == 1.0
    if n:
        assert T.finalize_expect(n, T.finalize_max_norms(n)[2])[2] < 0.5


@pytest.mark.parametrize("case", T.APPLY_CASES, ids=T.apply_case_id)
def test_bars_hold_apply(case):
    a = T.apply_inputs(case)
    clip = T.APPLY_CLIP if case["clip"] else None
    d = a["dense"]
    sets = [(d["p"], d["m"], d["v"], d["g"])]
    for s, (rows, ls, us) in enumerate(T.apply_owned(case)):
        t = a["tables"][s]
        sets += [(t["w2"][rows], t["m2"][rows], t["v2"][rows], a["g2"][ls, s, us]),
                 (t["w1"][rows], t["m1"][rows], t["v1"][rows], a["g1"][ls, s, us])]
    for lr in (T.LR, T.LR2):
        for w, m, v, g in sets:
            got = T.emu_rule(case["rule"], w, m, v, g, case["t"], lr, clip)
            for k, r in T.rule_check(case["rule"], w, m, v, g, case["t"], lr, clip, *got).items():
                _note(f"{case['rule']} {k}", r)
    if case["rule"] == "adam":     # g = m = v = 0 does not move the weight
        w, _, _ = T.emu_rule("adam", d["p"], d["m"], d["v"], d["g"], case["t"], T.LR, clip)
        assert w[-1] == d["p"][-1]
