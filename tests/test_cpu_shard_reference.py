"""CPU: the matrix of the field-sharded exchange kernels (tests/shard_cases.py) is sound before it reaches a GPU.
Every case reaches the branch its name claims and the cases together cover every shape, stride, layout edge and run
class; each layout restatement agrees with an independent formulation (the segment formulas of
tests/test_dp_gloo.py::_sharded_worker, plain concatenation); the float32 emulations satisfy every check with every
bar ratio <= 1; each planted mistake, applied to an emulation, fails the check of a named case; and the five entries
refuse bad arguments on the host (dummy pointers, nothing is launched).  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import shard_cases as S
from tests import tail_cases as T
from tests.helpers import tail_rowgrad_fp64


def _note(name, r):
    print(f"SHARD-RATIO cpu {name}: {r:.3f}")          # (pytest -s shows the worst error / bar)
    assert r <= 1.0, (name, r)


def _fails(check, *args):
    try:
        r = check(*args)
    except AssertionError:
        return True
    return r is not None and not r <= 1.0


# ---- branches ------------------------------------------------------------------------------------------------------
def test_field_blocks_are_field_shards_split():
    from deepfm_amd.training.sharded import FieldShards
    for world, num in S.PACK_WORLD_S + tuple((c["N"], c["S"]) for c in S.CHAIN_CASES) + ((3, 3), (4, 26)):
        sh = FieldShards(num, world)
        assert S.field_blocks(num, world) == (sh.first, sh.count)
    assert S.field_blocks(5, 3)[1] == [2, 2, 1] and S.field_blocks(11, 8)[1] == [2, 2, 2, 1, 1, 1, 1, 1]
    assert S.MAX_RANKS == 64 and S.MAX_FIELDS == 64


def test_gather_cases_cover_every_branch():
    cases = S.GATHER_CASES
    assert {c[0] // 4 for c in cases} == {1, 2, 3, 4, 8, 16} and {c[1] for c in cases} == {(1, 1, 4), (3, 3, 36), (8, 2, 4)}
    assert len(cases) == 6 * 3 * 3 == len({S.gather_case_id(c) for c in cases})
    r = S.gather_reach((12, (3, 3, 36), "default"))
    assert r["threads"] == 972 and r["mod256"] == 972 % 256 == 204 and r["blocks"] == 4 and r["straddle"]
    assert any(S.gather_reach(c)["mod256"] == 0 and S.gather_reach(c)["blocks"] > 1 for c in cases), "a full last workgroup"
    assert {S.gather_reach(c)["vocab"] for c in cases} == {(70000,), (3, 70000), (3, 50, 70000)}
    for c in cases:
        r = S.gather_reach(c)
        D = c[0]
        assert r["zero"] and r["last"] and r["dup"] and not r["inf_row_selected"], c
        assert not (r["negative"] or r["at_vocab"] or r["wide"]), c
        assert r["strides"] == {"default": (0, 0), "padded": (D + 4, 2), "packed": ((3 * D + 4 + 31) // 32 * 32,) * 2}[c[2]]
        o = S.gather_reach(c, oor=True)
        assert o["negative"] and o["at_vocab"] and o["wide"] and not o["inf_row_selected"], c
        assert S.gather_expect(S.gather_inputs(c, True))[2] == 1 and S.gather_expect(S.gather_inputs(c))[2] == 0
        inp = S.gather_inputs(c)
        for j, V in enumerate(inp["vocab"]):            # the planted patterns are where the ids do / do not look
            assert np.signbit(inp["w2"][j][V - 1, 0]) and inp["w2"][j][V - 1, 0] == 0 and 0 < inp["w2"][j][V - 1, 1] < 1e-40
            assert np.isinf(inp["w2"][j][V - 2]).all() and np.isinf(inp["w1"][j][V - 2])
    assert S.table_layout(16, "packed")[:3] == (64, 64, 16)


def test_packed_layout_is_pack_tables():
    """table_layout("packed") against what FeatureEmbedding.pack_tables_() makes of a tiny model's tables (CPU tensors)."""
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    from deepfm_amd.models.layers.embedding import FeatureEmbedding
    for D in S.GATHER_D:
        emb = FeatureEmbedding(DatasetSchema(fields={"a": FieldSchema("a", FeatureType.SPARSE, 7, D)}), D).pack_tables_()
        w2, w1 = emb.second_order_embeddings["a"].weight, emb.first_order_embeddings["a"].weight
        row2, row1, off1, s2, s1 = S.table_layout(D, "packed")
        assert (w2.stride(0), w1.stride(0)) == (s2, s1) == (row2, row1)
        assert (w1.data_ptr() - w2.data_ptr()) // 4 == off1 and emb.packed["a"]["buffer"].shape == (7, row2)


def test_pack_cases_cover_every_branch():
    cases = S.PACK_CASES
    reach = [S.pack_reach(c) for c in cases]
    assert {(c["world"], c["S"]) for c in cases} == {(1, 1), (2, 2), (3, 5), (8, 11)}
    assert {c["D"] for c in cases} == {4, 12, 64} and {c["B"] for c in cases} == {4, 36, 260}
    assert {c["n"] for c in cases} == {0, 4, 1028} and {c["slabs"] for c in cases} == {"none", "one", "two"}
    assert {r["blocks"] for r in reach} == {(1,), (1, 1), (2, 2, 1), (2, 2, 2, 1, 1, 1, 1, 1)}
    for key in ("world", "D", "B"):                      # every dense / slab variant at every world, width and batch
        for v in {c[key] for c in cases}:
            assert {(c["n"], c["slabs"]) for c in cases if c[key] == v} == set(S._PACK_DENSE), (key, v)
    for f in ("rows_end_inside", "first_end_inside", "dense_end_inside", "unrolled_no_tail", "unrolled_tail3", "tail_only",
              "unslabbed_between"):
        assert any(r[f] for r in reach), f
    assert {r["workgroups"] > 1 for r in reach} == {False, True}
    assert S.PACK_SLABS["one"] == ((16, 4, 8, 3),) and [s[3] for s in S.PACK_SLABS["two"]] == [8, 11]
    for c, r in zip(cases, reach):
        p = S.pack_inputs(c)
        assert p["F"] == c["S"] + 3 and not r["map_identity"] and (c["S"] < 3 or not r["map_monotone"])
        assert len(set(p["fos"])) == c["S"] and all(0 <= f < p["F"] for f in p["fos"])
        assert r["unslabbed_between"] == (c["slabs"] != "none")
        for off, o, i, sp, data in p["slabs"]:
            assert off % 16 == 0 and off + o * i <= c["n"] and data.shape == (sp, o * i)
        idle = sorted(set(range(p["F"])) - set(p["fos"]))
        assert len(idle) == 3 and np.isinf(p["g_field"][:, idle]).all() and np.isfinite(p["g_field"][:, list(p["fos"])]).all()
    assert len({S.pack_case_id(c) for c in cases}) == len(cases) == 36


def test_rowgrad_cases_cover_every_branch():
    cases = S.ROWGRAD_CASES
    reach = {S.rowgrad_case_id(c): S.rowgrad_reach(c) for c in cases}
    assert len(reach) == len(cases) == 2 + 9 + 1
    assert {(c["world"], c["B"], c["nf"]) for c in cases} == {(3, 20, 3), (8, 516, 2)}
    assert {c["n"] for c in cases if c["B"] == 20} == {0, 12} and {c["n"] for c in cases if c["B"] == 516} == {0, 12}
    assert {(c["D"], c["kind"]) for c in cases if c["B"] == 516} == \
        set(itertools.product((4, 16, 64), ("mixed", "split2049", "run4096"))) | {(12, "mixed")}
    for c in cases:
        r = reach[S.rowgrad_case_id(c)]
        assert r["coop"] == (c["D"] != 12) and r["padding"] and r["nan_tail"] == (c["n"] == 12)
        inp = S.rowgrad_inputs(c)
        assert inp["segment"] == 516 * 2 * c["D"] + 516 + c["n"] if c["B"] == 516 else inp["segment"] == 20 * 3 * 16 + 20 + c["n"]
        if c["kind"] == "spans":
            assert r["chunks"] == 1 and r["spans_all"] and r["seam_only"] and r["prefetch_crossing"]
            continue
        # n = 4128: two chunks, the boundary falls at sample 484 of segment 7
        assert r["chunks"] == 2 and (r["boundary_segment"], r["boundary_sample"]) == (7, 484) and 7 * 516 + 484 == T.CH
        f0 = inp["gids"][0, :T.CH]
        if c["kind"] == "mixed":
            assert tuple(np.bincount(f0)[5:10]) == (300, 65, 64, 9, 8) and (f0 == 0).sum() == 3
            assert all(r["crossing"][k] for k in ("<=8", "<=64", "<=2048")) and r["split_runs"] == 0 and r["prefetch_crossing"]
        else:
            assert r["split_runs"] == 1 and r["split_listed"] and r["crossing"][">2048"] and r["crossing"]["all_segments"]
            assert np.unique(f0[f0 != 0]).size == (T.CH - T.K_SPLIT if c["kind"] == "split2049" else 1)
            assert (f0 == 3).sum() == (T.K_SPLIT + 1 if c["kind"] == "split2049" else T.CH)
    for D in (4, 16, 64):             # every run class with a run fed by more than one segment, at every coop width
        union = {}
        for c in cases:
            if c["D"] == D and c["B"] == 516:
                for k, v in reach[S.rowgrad_case_id(c)]["crossing"].items():
                    union[k] = union.get(k, False) or v
        assert all(union[k] for k in ("<=8", "<=64", "<=2048", ">2048", "all_segments")), (D, union)
    assert S.split_slices(4) == 16 and S.split_slices(16) == 64 and S.split_slices(64) == 64


def test_chain_sum_and_stage_cases():
    assert [(c["N"], c["S"], c["B"], c["D"]) for c in S.CHAIN_CASES] == [(3, 5, 36, 8), (8, 11, 516, 16)]
    for c in S.CHAIN_CASES:
        ch = S.chain_inputs(c)
        assert ch["count"] == S.field_blocks(c["S"], c["N"])[1] and set(ch["vocab"]) == {3, 50, 5000}
        gids, g2, g1, per_owner = S.chain_global(c)
        assert gids.shape == (c["S"], c["N"] * c["B"]) and len(per_owner) == c["N"]
        if c["N"] == 8:
            assert c["N"] * c["B"] > T.CH and set(ch["count"]) == {1, 2}
            hot = [(gids[s, :T.CH] == 5).sum() for s in range(c["S"]) if ch["vocab"][s] == 50]
            assert min(hot) > T.K_SPLIT, "the 50-row fields carry a split run"
    assert S.SUM_N == (0, 1, 63, 64, 65, 1023, 1024, 1025, 4099) and S.STAGE_NBYTES == (16, 4080, 4096, 4112)
    assert [n // 16 for n in S.STAGE_NBYTES] == [1, 255, 256, 257]
    assert [(r["workgroups"], r["last_partial"]) for r in map(S.stage_reach, S.STAGE_NBYTES)] == \
        [(1, True), (1, True), (1, False), (2, True)]
    sums = {n: S.sum_reach(n) for n in S.SUM_N}
    assert [sums[n]["rounds"] for n in S.SUM_N] == [0, 1, 1, 1, 1, 1, 1, 2, 5]
    assert sums[1024]["partial_round"] is False and sums[1025]["partial_round"] and sums[4099]["partial_round"]
    assert sums[63]["idle_lanes"] and sums[63]["one_wave"] and sums[64]["one_wave"] and not sums[64]["idle_lanes"]
    assert sums[65]["idle_waves"] and sums[1023]["idle_lanes"] and not sums[1023]["idle_waves"]
    x = S.sum_inputs(4099)
    assert (x > 0).any() and (x < 0).any() and np.abs(x).max() / np.abs(x[x != 0]).min() > 1e6


# ---- layout restatements against independent formulations ---------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in S.GATHER_CASES if c[0] in (4, 12)], ids=S.gather_case_id)
def test_gather_layout_against_the_worker_formulas(case):
    """send and gids as tests/test_dp_gloo.py::_sharded_worker forms them, one peer at a time."""
    inp = S.gather_inputs(case)
    world, nf, B, D = inp["world"], inp["nf"], inp["B"], inp["D"]
    gid = inp["ids"]
    send = np.zeros((world, B * nf * (D + 1)), np.float32)
    for p in range(world):
        e = np.stack([inp["w2"][j][gid[p, j]] for j in range(nf)], axis=1)
        w = np.stack([inp["w1"][j][gid[p, j]] for j in range(nf)], axis=1)
        send[p] = np.concatenate([e.reshape(-1), w.reshape(-1)])
    want_send, want_gids, err = S.gather_expect(inp)
    assert S.same_bits(send, want_send) and err == 0
    for j in range(nf):
        assert np.array_equal(want_gids[j], gid[:, j].reshape(-1))
    S.gather_check(inp, *S.emu_gather(inp))
    S.gather_check(S.gather_inputs(case, True), *S.emu_gather(S.gather_inputs(case, True)))


@pytest.mark.parametrize("case", S.PACK_CASES[::3], ids=S.pack_case_id)
def test_pack_layout_against_the_worker_formulas(case):
    p = S.pack_inputs(case)
    B, D, n = p["B"], p["D"], p["n"]
    g_fe = p["g_field"][:, list(p["fos"])]                  # (B, S, D): the SPARSE fields in SPARSE order
    dense = S.dense_sum_f32(p)
    gs = np.concatenate([np.concatenate([g_fe[:, lo:lo + c].reshape(-1), p["g_first"], dense])
                         for lo, c in zip(p["first"], p["count"])])
    assert S.same_bits(gs, np.concatenate(S.pack_expect(p)))
    assert [s.size for s in S.pack_expect(p)] == [B * c * D + B + n for c in p["count"]]
    ref, _ = S.dense_sum_fp64(p)
    want = p["dense"].astype(np.float64)
    for off, o, i, sp, data in p["slabs"]:
        want[off:off + o * i] = want[off:off + o * i] + sum(data[q].astype(np.float64) for q in range(sp))
    np.testing.assert_allclose(ref, want, rtol=1e-13)


@pytest.mark.parametrize("case", S.ROWGRAD_CASES, ids=S.rowgrad_case_id)
def test_segments_against_concatenation(case):
    inp = S.rowgrad_inputs(case)
    world, B, nf, D = inp["world"], inp["B"], inp["nf"], inp["D"]
    g2, g1 = S.read_segments(inp["recv"], world, B, nf, D, inp["segment"])
    assert S.same_bits(g2, inp["g2"]) and S.same_bits(g1, inp["g1"])
    seg = inp["recv"].reshape(world, inp["segment"])
    again2 = np.concatenate([seg[p, :B * nf * D].reshape(B, nf, D) for p in range(world)])
    again1 = np.concatenate([seg[p, B * nf * D:B * nf * D + B] for p in range(world)])
    assert S.same_bits(again2, inp["g2"]) and S.same_bits(again1, inp["g1"])
    assert np.isnan(seg[:, B * nf * D + B:]).all() and seg[:, B * nf * D + B:].shape[1] == case["n"]
    for e in S.rowgrad_expect(case):                       # the lists' rows are np.unique of the chunk's non-zero ids
        ids = inp["gids"][e["s"], e["c"] * T.CH:(e["c"] + 1) * T.CH]
        assert np.array_equal(e["ref"]["rows"], np.unique(ids[ids != 0]))
        ref = tail_rowgrad_fp64(ids, again2[e["c"] * T.CH:(e["c"] + 1) * T.CH, e["s"]], again1[e["c"] * T.CH:(e["c"] + 1) * T.CH])
        assert np.array_equal(ref["g2"], e["ref"]["g2"])


# ---- emulations and bars -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.GATHER_CASES, ids=S.gather_case_id)
def test_emulation_passes_gather(case):
    for oor in (False, True):
        inp = S.gather_inputs(case, oor)
        send, gids, err = S.emu_gather(inp)
        assert not np.isnan(send).any() and (gids != -7).all()
        S.gather_check(inp, send, gids, err)


@pytest.mark.parametrize("case", S.PACK_CASES, ids=S.pack_case_id)
def test_emulation_passes_pack(case):
    p = S.pack_inputs(case)
    send = S.emu_pack(p)
    assert not np.isnan(send).any()
    _note("pack dense part", S.pack_check(p, send))


@pytest.mark.parametrize("case", S.ROWGRAD_CASES, ids=S.rowgrad_case_id)
def test_emulation_passes_rowgrad(case):
    inp = S.rowgrad_inputs(case)
    got = S.emu_lists(inp["gids"], inp["recv"], inp["world"], inp["B"], inp["D"], inp["segment"])
    _note("row gradients", max(T.rowgrad_check(e, g2, g1) for e, (g2, g1) in zip(S.rowgrad_expect(case), got)))


@pytest.mark.parametrize("case", S.CHAIN_CASES, ids=S.chain_case_id)
def test_emulation_passes_the_chain(case):
    ch = S.chain_inputs(case)
    sends = [S.emu_gather(S.chain_owner_gather_inputs(ch, r)) for r in range(ch["N"])]
    S.chain_check_rows(ch, *S.chain_reassemble(ch, [s[0] for s in sends]))
    gids, _, _, per_owner = S.chain_global(case)
    recvs = S.chain_received(ch, [S.emu_pack(p) for p in ch["packs"]])
    worst = 0.0
    for r in range(ch["N"]):
        lo, c = ch["first"][r], ch["count"][r]
        assert np.array_equal(sends[r][1].reshape(c, -1), gids[lo:lo + c])
        seg = S.pack_segment(ch["B"], c, ch["D"], S.CHAIN_N_DENSE)
        got = S.emu_lists(gids[lo:lo + c], recvs[r], ch["N"], ch["B"], ch["D"], seg)
        worst = max([worst] + [T.rowgrad_check(e, g2, g1) for e, (g2, g1) in zip(per_owner[r], got)])
        S.chain_check_dense(ch, r, recvs[r])
    _note("chain row gradients", worst)


@pytest.mark.parametrize("n", S.SUM_N)
def test_emulation_passes_sum_floats(n):
    x = S.sum_inputs(n)
    got = S.emu_sum_floats(x)
    _note("sum_floats", S.sum_check(x, got))
    if n == 0:
        assert S.same_bits([got], [0.0])
    seq = np.float32(0) if n == 0 else np.cumsum(x, dtype=np.float32)[-1]          # another correct order: inside the bar
    assert T.ratio(float(seq) - x.astype(np.float64).sum(), max(n, 1) * T.U * np.abs(x.astype(np.float64)).sum()) <= 1.0


# ---- planted mistakes: each fails the check of a named case -------------------------------------------------------
G_STRADDLE = (12, (3, 3, 36), "padded")
G_PACKED = (16, (8, 2, 4), "packed")
P_UNEVEN = next(c for c in S.PACK_CASES if (c["world"], c["S"]) == (3, 5) and c["slabs"] == "two")
P_EIGHT = next(c for c in S.PACK_CASES if (c["world"], c["S"]) == (8, 11))
R_SPANS = S.ROWGRAD_CASES[1]
R_SPLIT = next(c for c in S.ROWGRAD_CASES if c["kind"] == "run4096" and c["D"] == 16)
R_SPLIT2049 = next(c for c in S.ROWGRAD_CASES if c["kind"] == "split2049" and c["D"] == 4)


def _gather_fails(case, mistake, oor=False):
    inp = S.gather_inputs(case, oor)
    return _fails(S.gather_check, inp, *S.emu_gather(inp, mistake))


def _rowgrad_fails(case, mistake):
    inp = S.rowgrad_inputs(case)
    got = S.emu_lists(inp["gids"], inp["recv"], inp["world"], inp["B"], inp["D"], inp["segment"], mistake)
    return any(_fails(T.rowgrad_check, e, g2, g1) for e, (g2, g1) in zip(S.rowgrad_expect(case), got))


def test_planted_mistakes_are_caught():
    caught = {
        "neighbour_first_order": _gather_fails(G_STRADDLE, "neighbour_first_order") and _gather_fails(G_PACKED, "neighbour_first_order"),
        "stride1_ignored": _gather_fails(G_STRADDLE, "stride1_ignored") and _gather_fails(G_PACKED, "stride1_ignored"),
        "gids_rank_major": _gather_fails(G_STRADDLE, "gids_rank_major") and _gather_fails(G_PACKED, "gids_rank_major"),
        "id_truncated_32": _gather_fails(G_STRADDLE, "id_truncated_32", oor=True),
        "segment_forgets_first": _fails(S.pack_check, S.pack_inputs(P_UNEVEN), S.emu_pack(S.pack_inputs(P_UNEVEN), "segment_forgets_first")),
        "field_map_twice": _fails(S.pack_check, S.pack_inputs(P_EIGHT), S.emu_pack(S.pack_inputs(P_EIGHT), "field_map_twice")),
        "slab_tail_dropped": _fails(S.pack_check, S.pack_inputs(P_UNEVEN), S.emu_pack(S.pack_inputs(P_UNEVEN), "slab_tail_dropped")),
        "segment_index_b_plus_1": _rowgrad_fails(R_SPANS, "segment_index_b_plus_1") and _rowgrad_fails(R_SPLIT, "segment_index_b_plus_1"),
        "split_last_slice_dropped": _rowgrad_fails(R_SPLIT, "split_last_slice_dropped") and _rowgrad_fails(R_SPLIT2049, "split_last_slice_dropped"),
        "butterfly_first_step": all(_fails(S.sum_check, S.sum_inputs(n), S.emu_sum_floats(S.sum_inputs(n), "butterfly_first_step"))
                                    for n in (63, 1024, 4099)),
    }
    assert set(caught) == set(S.MISTAKES)
    assert all(caught.values()), [k for k, v in caught.items() if not v]
    # ... and the in-range cases do not depend on the truncation: only the separate sub-case can see it
    assert not _gather_fails(G_STRADDLE, "id_truncated_32")
    # without a slab tail there is nothing to drop: splits = 8 alone passes
    one = dict(P_UNEVEN, slabs="none")
    assert not _fails(S.pack_check, S.pack_inputs(one), S.emu_pack(S.pack_inputs(one), "slab_tail_dropped"))


# ---- host argument checks: DFM_ERR_INVALID, nothing launched ------------------------------------------------------
P = 0x10000
INVALID = 1


def _lib():
    from deepfm_amd import _lib
    return _lib, _lib.load()


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _gather_args(_l, **kw):
    tabs = (_l.Table * 2)()
    for t in tabs:
        t.w2 = t.w1 = P
    a = dict(tables=tabs, vocab=_i32(10, 10), nf=2, dim=16, world=2, batch=8, ids=P, send=P, gids=P, err=P)
    a.update(kw)
    return (a["tables"], a["vocab"], a["nf"], a["dim"], a["world"], a["batch"], a["ids"], a["send"], a["gids"], a["err"], None)


def _pack_args(_l, **kw):
    a = dict(first=_i32(0, 2), count=_i32(2, 1), world=2, fos=_i32(4, 0, 2), S=3, F=5, dim=16, batch=8, g_field=P, g_first=P,
             dense=P, n=64, slabs=None, num_slabs=0, send=P)
    a.update(kw)
    return (a["first"], a["count"], a["world"], a["fos"], a["S"], a["F"], a["dim"], a["batch"], a["g_field"], a["g_first"],
            a["dense"], a["n"], a["slabs"], a["num_slabs"], a["send"], None)


def _rowgrad_args(**kw):
    a = dict(nf=2, dim=16, world=2, batch=8, recv=P, segment=8 * 2 * 16 + 8, pos=P, seg=P, num=P, g2=P, g1=P)
    a.update(kw)
    return (a["nf"], a["dim"], a["world"], a["batch"], a["recv"], a["segment"], a["pos"], a["seg"], a["num"], a["g2"], a["g1"], None)


def _slab(_l, g_w, out=4, inp=8):
    s = _l.SlabRef()
    s.workspace, s.g_w, s.batch, s.out_features, s.in_features, s.splits = P, g_w, 64, out, inp, 3
    return s


def test_host_argument_checks():
    _l, lib = _lib()
    bad = {}
    msg = lambda: lib.dfm_last_error().decode()                               # noqa: E731
    g = lambda **kw: lib.dfm_shard_gather(*_gather_args(_l, **kw))            # noqa: E731
    p = lambda **kw: lib.dfm_shard_pack(*_pack_args(_l, **kw))                # noqa: E731
    r = lambda **kw: lib.dfm_shard_rowgrad(*_rowgrad_args(**kw))              # noqa: E731
    big = (C.c_int32 * 65)(*([0] * 65))
    bad["gather batch % 4"] = (g(batch=6), msg())
    bad["pack batch % 4"] = (p(batch=6), msg())
    bad["gather dim % 4"] = (g(dim=6), msg())
    bad["pack dim % 4"] = (p(dim=6), msg())
    bad["rowgrad dim % 4"] = (r(dim=6, segment=1 << 20), msg())
    bad["gather unaligned send"] = (g(send=P + 4), msg())
    bad["pack unaligned send"] = (p(send=P + 4), msg())
    bad["rowgrad unaligned recv"] = (r(recv=P + 4), msg())
    for name, fn in (("gather", g), ("rowgrad", r)):
        bad[f"{name} world 0"] = (fn(world=0), msg())
        bad[f"{name} world 65"] = (fn(world=S.MAX_RANKS + 1, **({"segment": 1 << 20} if name == "rowgrad" else {})), msg())
        bad[f"{name} batch * world = 2^31"] = (fn(batch=1 << 28, world=8, **({"segment": 1 << 40} if name == "rowgrad" else {})), msg())
    bad["pack world 0"] = (p(world=0), msg())
    bad["pack world 65"] = (p(world=S.MAX_RANKS + 1, first=big, count=big), msg())
    bad["pack blocks overlap"] = (p(first=_i32(0, 1), count=_i32(2, 2)), msg())
    bad["pack blocks leave a gap"] = (p(first=_i32(0, 2), count=_i32(1, 1)), msg())
    bad["pack blocks out of rank order"] = (p(first=_i32(1, 0), count=_i32(2, 1)), msg())
    bad["pack blocks do not cover"] = (p(first=_i32(0, 1), count=_i32(1, 1)), msg())
    bad["pack blocks outside"] = (p(first=_i32(0, 2), count=_i32(2, 2)), msg())
    bad["pack field_of_sparse out of range"] = (p(fos=_i32(4, 5, 2)), msg())
    bad["pack field_of_sparse negative"] = (p(fos=_i32(4, -1, 2)), msg())
    bad["pack n_dense % 4"] = (p(n=62), msg())
    bad["rowgrad segment too short"] = (r(segment=8 * 2 * 16 + 4), msg())
    bad["rowgrad segment % 4"] = (r(segment=8 * 2 * 16 + 8 + 2), msg())
    many = (_l.SlabRef * 17)(*[_slab(_l, P) for _ in range(17)])
    bad["pack 17 slabs"] = (p(slabs=many, num_slabs=S.MAX_SLABS + 1), msg())
    bad["pack slab outside the dense buffer"] = (p(slabs=(_l.SlabRef * 1)(_slab(_l, P + 4 * 48)), num_slabs=1), msg())
    bad["pack slab before the dense buffer"] = (p(slabs=(_l.SlabRef * 1)(_slab(_l, P - 64)), num_slabs=1), msg())
    bad["stage nbytes % 16"] = (lib.dfm_stage_record(P, 2 * P, 24, None), msg())
    bad["stage nbytes 0"] = (lib.dfm_stage_record(P, 2 * P, 0, None), msg())
    bad["stage unaligned src"] = (lib.dfm_stage_record(P + 4, 2 * P, 32, None), msg())
    bad["stage unaligned dst"] = (lib.dfm_stage_record(P, 2 * P + 8, 32, None), msg())
    bad["sum_floats n < 0"] = (lib.dfm_sum_floats(P, -1, P, None), msg())
    bad["sum_floats n = 2^31"] = (lib.dfm_sum_floats(P, 1 << 31, P, None), msg())
    assert {k: v for k, v in bad.items() if v[0] != INVALID or not v[1]} == {}
    # refused for the reason the case names, not for another one that happens to come first
    for k, needle in (("gather world 65", "rank count"), ("rowgrad world 65", "rank count"), ("pack world 65", "rank count"),
                      ("rowgrad batch * world = 2^31", "2^31"), ("pack blocks overlap", "contiguous"),
                      ("pack blocks do not cover", "cover every"), ("pack field_of_sparse out of range", "field_of_sparse"),
                      ("pack 17 slabs", "slab references"), ("pack slab outside the dense buffer", "views of the dense"),
                      ("rowgrad segment too short", "segment too short"), ("stage unaligned dst", "aligned"),
                      ("gather unaligned send", "aligned"), ("pack unaligned send", "aligned")):
        assert needle in bad[k][1], (k, bad[k])
    for B, nf, D, n in ((4, 1, 4, 0), (36, 2, 12, 4), (260, 2, 64, 1028), (516, 3, 16, 12)):
        assert lib.dfm_shard_pack_segment(B, nf, D, n) == S.pack_segment(B, nf, D, n) == B * nf * D + B + n
