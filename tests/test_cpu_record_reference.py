"""Host-side proofs for the record-kernel matrix (tests/record_cases.py, tests/test_gpu_record_matrix.py):

1. every case fits the caps the kernels compute (``training/eligibility.py`` restates them), every refusal case is
   refused for the reason it names, and every case reaches the branch it claims;
2. the case list reaches every instantiation that can be launched at all, all three kinds of backward workgroup and
   projection jobs of one chunk, of several and with a partial last one;
3. the fp64 restatements of tests/helpers.py reproduce the embedding goldens and ``oracle/ctr_oracle.py``;
4. a plain float32 evaluation of the same statements, in two summation orders, stays inside every bar with the margin
   the bars were derived with;
5. the FM value of every case stays clear of cancellation, so no output is left out of a comparison;
6. each mistake of the fixed list lands outside the bar in the case that claims to cover it.
"""
import numpy as np
import pytest

from deepfm_amd import _lib
from deepfm_amd.training import eligibility as E
from oracle import ctr_oracle as O
from tests import helpers as H
from tests import record_cases as R

ALL = list(R.CASES)


# ----------------------------------------------------------------------------- 1. caps, refusals, branches
@pytest.mark.parametrize("name", ALL)
def test_case_fits_the_caps_it_claims(name):
    case = R.CASES[name]
    m = R.model_shim(case)
    gather, backward = E.record_gather_reason(m), E.record_backward_reason(m, case.B)
    assert case.fwd == (gather is None), gather
    assert case.bwd == (gather is None and backward is None), (gather, backward)
    assert case.F <= _lib.MAX_FIELDS and case.why
    if case.fwd:
        assert E.mixed_param_bytes(m) <= _lib.RECORD_PARAM_LDS_BYTES
        sb = R.fwd_sb(case.F, case.D)
        assert sb * case.F * case.D // 4 <= 1024, "over the gather's 1024-thread workgroup"
        assert 4 * (E.mixed_param_bytes(m) // 4 + sb * case.F * (case.D + 1)) <= 65536
    if case.bwd:
        assert E.backward_lds_bytes(m) <= _lib.BWD_RECORD_LDS_BYTES
        assert all(f["type"] != "sequence" or f["combiner"] != "max" for f in case.fields)
    want = {None: None, "bwd_d64": "bytes of LDS", "bwd_max": "pools with max", "D": "fm_embed_dim",
            "d%4": "not a multiple of 4", "param_lds": "over the record gather's cap"}[case.refusal]
    if case.refusal in ("bwd_d64", "bwd_max"):
        assert gather is None and want in backward
    elif case.refusal:
        assert want in gather


def test_refusals_cover_the_documented_list():
    assert {R.CASES[n].refusal for n in R.REFUSALS} == {"bwd_d64", "bwd_max", "D", "d%4", "param_lds"}
    assert {R.CASES[n].D for n in R.REFUSALS if R.CASES[n].refusal == "D"} == {12, 20}


def test_cases_reach_the_branches_they_claim():
    C = R.CASES
    for D in R.FM_DIMS:
        sb = R.fwd_sb(3, D)
        assert sb > 1 and C[f"small_b5_D{D}"].B < sb
        assert C[f"small_tail_D{D}"].B > sb and C[f"small_tail_D{D}"].B % sb
        assert C[f"single_D{D}"].F == 1
    per = {n: C[n].F * C[n].D // 4 for n in C if n.startswith("wide_")}
    assert per["wide_F63_D32"] == 504 and per["wide_F64_D32"] == 512 and per["wide_F31_D64"] == 496
    assert per["wide_F33_D64"] == 528 and per["wide_F64_D64"] == 1024
    assert all(R.fwd_sb(C[n].F, C[n].D) == 1 for n in per if per[n] >= 496) and R.fwd_sb(64, 16) == 2
    # widths: d == D, d < D (4), d > D and a width that is no power of two, each as SPARSE, SEQUENCE and DENSE
    for D, nm in ((4, "widths_D4"), (8, "widths_D8"), (16, "widths_D16"), (32, "widths_D32"), (64, "widths_D64")):
        for kind in ("sparse", "sequence", "dense"):
            ds = {f["dim"] for f in C[nm].fields if f["type"] == kind}
            assert D in ds and any(d != D for d in ds), (nm, kind)
            if nm != "widths_D64":
                assert any(d & (d - 1) for d in ds), (nm, kind)
    assert {4, 32, 12, 20, 48} <= {f["dim"] for f in C["widths_D16"].fields}
    # vocabularies against the row tile, and ids on its edges
    for nm in ("vocab_D16", "vocab_D4"):
        inp = R.inputs(nm)
        by_d = {}
        for f in C[nm].fields:
            by_d.setdefault(f["dim"], set()).add(f["vocab"])
            named = set(np.unique(inp["batch"][f["name"]]).tolist())
            assert set(R.edge_rows(f)) <= named, (nm, f["name"])
            assert len(named) < f["vocab"] or f["vocab"] <= 2, "rows nobody names"
        for d, vs in by_d.items():
            if len(vs) > 1:
                t = R.row_tile(d)
                assert {t - 1, t, t + 1} <= vs and any(v > 2 * t for v in vs), (nm, d, vs)
                assert 2 in vs or t // 2 + 1 in vs
    assert R.row_tile(16) == 102 and R.row_tile(4) == 256 and R.row_tile(32) == 56 and R.row_tile(12) == 128
    # batch sizes against slices and stages
    assert [R.bwd_slices(B) for B in (1, 7, 256, 257, 513, 4097)] == [(1, 1), (1, 7), (1, 256), (2, 129), (3, 171), (16, 257)]
    assert {C[f"batch_B{B}"].B for B in (1, 7, 256, 257, 513, 4097)} == {1, 7, 256, 257, 513, 4097}
    assert {f["max_len"] for f in C["batch_B4097"].fields if f["type"] == "sequence"} == {1, 3}    # n * L odd at n = 1
    hot = R.inputs("batch_B4097")["batch"]["hot"]
    assert (hot == 3).sum() > 3000, "the hot id"
    # bags
    inp, B = R.inputs("bags_D16"), C["bags_D16"].B
    assert {(f["max_len"], f["combiner"]) for f in C["bags_D16"].fields if f["type"] == "sequence"} >= \
        {(L, c) for L in (1, 3, 6) for c in ("mean", "sum")}
    ids = inp["batch"]["b6m"]
    assert not ids[B - 1].any() and len(set(ids[B // 2])) == 1 and ids[B // 2, 0] and ids[0, 1] == 0 and ids[0, 0] and ids[0, 2]
    assert {f["combiner"] for f in C["max_D16"].fields if f["type"] == "sequence"} == {"max"}


def test_plan_create_takes_a_narrow_field_behind_a_field_of_width_fm_dim():
    """The bug the matrix found (case refuse_d6 on the dense-autograd path): dfm_embedding_plan_create held a field's row
    stride to the uniform gather's multiple of 4 while the plan still LOOKED uniform, so a width of 6 was refused with
    "bad row strides" behind a field of width fm_dim and accepted in front of it.  The descriptor check runs before any
    device work: without a GPU the call now gets as far as the upload (a HIP error), with one it succeeds."""
    import ctypes as C
    lib = _lib.load()
    arr = (_lib.Field * 2)()
    for i, d in enumerate((16, 6)):
        fd = arr[i]
        fd.kind, fd.dim, fd.vocab, fd.max_len, fd.combiner = _lib.SPARSE, d, 9, 1, 0
        fd.w2, fd.w1, fd.stride2, fd.stride1 = 4096, 8192, d, 1
        fd.proj = 12288 if d != 16 else None
    handle = C.c_void_p()
    rc = lib.dfm_embedding_plan_create(arr, 2, 16, C.byref(handle))
    msg = lib.dfm_last_error().decode() if rc else ""
    assert rc != 1 and "bad row strides" not in msg, msg
    if rc == 0:
        assert not lib.dfm_embedding_plan_is_uniform(handle)
        lib.dfm_embedding_plan_destroy(handle)
    # a plan that IS uniform still needs 16-byte rows
    arr[1].dim, arr[1].stride2, arr[1].proj = 16, 18, None
    assert lib.dfm_embedding_plan_create(arr, 2, 16, C.byref(handle)) == 1
    assert "bad row strides" in lib.dfm_last_error().decode()


# ----------------------------------------------------------------------------- 2. coverage
def test_every_launchable_instantiation_and_job_kind_is_reached():
    kernels, jobs, chunks, partial = set(), set(), set(), False
    for name in ALL:
        r = R.reach(name)
        kernels |= r["kernels"]
        jobs |= r["jobs"]
        chunks |= r["proj_chunks"]
        partial |= r["proj_partial"]
    print("RECORD-COVERAGE", sorted(kernels))
    want = {f"emb_fwd_record<{D}>" for D in R.FM_DIMS}
    want |= {f"{k}<{D}>" for k in ("emb_bwd_record", "emb_bwd_record_fm") for D in (4, 8, 16, 32)}
    assert kernels == want
    assert jobs == {"table", "dense", "proj"}
    assert 1 in chunks and max(chunks) > 1 and partial
    # emb_bwd_record<64> and emb_bwd_record_fm<64> are compiled but no schema passes describe_bwd_record's LDS cap at
    # fm_embed_dim 64: d == 64 needs 70 672 bytes for its staged vectors, any other d a projection job of
    # 1024 * (64 + d) bytes.  Thirteen of the fifteen instantiations can be launched; the matrix launches thirteen.
    for d in range(4, 257, 4):
        for f in (R.sp("s", 9, d), R.seq("g", 9, d, 1, "mean"), R.de("x", d)):
            m = R.model_shim(R.Case("probe", 64, (f,), 1, "probe"))
            assert E.backward_lds_bytes(m) > _lib.BWD_RECORD_LDS_BYTES, (d, f["type"])


# ----------------------------------------------------------------------------- 3. the restatements against goldens and oracle
def _close_all(got, want, what, rtol=H.RTOL):
    assert set(got) == set(want), what
    for k in want:
        H.assert_close(got[k], want[k], rtol, what=f"{what} {k}")


@pytest.mark.parametrize("golden", ["emb_movielens_mean", "emb_movielens_sum", "emb_movielens_max",
                                    "emb_layers_test_schema", "emb_criteo_d32"])
def test_fp64_restatement_reproduces_the_goldens(golden):
    g = H.load(golden)
    fields, params, batch, D = H.fields_of(g), H.group(g, "param/"), H.group(g, "batch/"), int(g["fm_dim"])
    r = H.record_forward_fp64(fields, params, batch, D)
    H.assert_close(r["first_order"][:, None], g["out/first_order"], 1e-5, what="first_order")
    H.assert_close(r["field_embeddings"], g["out/field_embeddings"], 1e-5, what="field_embeddings")
    H.assert_close(r["flat_embeddings"], g["out/flat_embeddings"], 1e-5, what="flat_embeddings")
    H.assert_close(r["fm"][:, None], O.fm_forward(g["out/field_embeddings"]), 1e-5, what="fm")
    b = H.record_backward_fp64(fields, params, batch, D, g["upstream/first_order"], g["upstream/field_embeddings"],
                               g["upstream/flat_embeddings"])
    _close_all(b["grads"], H.group(g, "grad/"), golden, 1e-5)


@pytest.mark.parametrize("name", [n for n in ALL if R.CASES[n].B <= 600])
def test_fp64_restatement_reproduces_the_oracle(name):
    case, inp = R.CASES[name], R.inputs(name)
    fields = [dict(f) for f in case.fields]
    fo, fe, flat = O.embedding_forward(fields, inp["params"], inp["batch"], case.D)
    r = R.forward_ref(name)
    H.assert_close(r["first_order"][:, None], fo, what="first_order")
    H.assert_close(r["field_embeddings"], fe, what="field_embeddings")
    H.assert_close(r["flat_embeddings"], flat, what="flat_embeddings")
    H.assert_close(r["fm"][:, None], O.fm_forward(fe), what="fm")
    H.assert_close(r["fm_sum"], fe.sum(axis=1), what="fm_sum")
    want = O.embedding_backward(fields, inp["params"], inp["batch"], case.D, inp["g_first"], inp["g_field"], inp["g_flat"])
    _close_all(R.backward_ref(name, "plain")["grads"], want, name)
    # the FM term: the oracle's fm_backward added to g_field
    sv = R.saved_f32(name)
    d_e = O.fm_backward(sv["field_embeddings"], inp["g_fm"])
    want = O.embedding_backward(fields, inp["params"], inp["batch"], case.D, inp["g_first"], inp["g_field"] + d_e, inp["g_flat"])
    _close_all(R.backward_ref(name, "fm_field")["grads"], want, name + " fm")
    want = O.embedding_backward(fields, inp["params"], inp["batch"], case.D, inp["g_first"], d_e, inp["g_flat"])
    _close_all(R.backward_ref(name, "fm_only")["grads"], want, name + " fm alone")


# ----------------------------------------------------------------------------- 4. float32 inside the bars, with the margin
def test_constants_are_the_measured_ratios_times_the_margin():
    worst = dict.fromkeys(R.C, 0.0)
    for name in ALL:
        for order in ("seq", "pair"):
            r = R.f32_ratios(name, order)
            for k, v in r.items():
                assert v * R.MARGIN <= R.C[k], f"{name} {order} {k}: float32 ratio {v:.3f} x {R.MARGIN} over C = {R.C[k]}"
                worst[k] = max(worst[k], v)
    print("RECORD-F32", {k: round(v, 3) for k, v in worst.items()})
    for k, v in worst.items():
        assert R.C[k] <= 1.25 * R.MARGIN * v + 0.25, f"C[{k}] = {R.C[k]} is wider than its derivation ({R.MARGIN} x {v:.3f})"


# ----------------------------------------------------------------------------- 5. nothing cancels
@pytest.mark.parametrize("name", ALL)
def test_fm_value_clear_of_cancellation(name):
    r = R.forward_ref(name)
    if R.CASES[name].F == 1:
        assert not r["fm"].any()            # a single field: 0.5 (e^2 - e^2), exactly 0 with a bar of eps * e^2
        return
    assert (np.abs(r["fm"]) / r["A"]["fm"]).min() >= R.FM_FLOOR
    for k in ("first_order", "field_embeddings", "flat_embeddings", "fm_sum"):
        assert (np.abs(r[k]) == r["A"][k]).all() or np.allclose(np.abs(r[k]), r["A"][k], rtol=1e-12), k


# ----------------------------------------------------------------------------- 6. sensitivity
@pytest.mark.parametrize("mut,name,mode", R.MUTATIONS, ids=[f"{m.__name__[4:]}-{n}" for m, n, _ in R.MUTATIONS])
def test_mutation_lands_outside_the_bar(mut, name, mode):
    case = R.CASES[name]
    assert case.bwd
    want = R.backward_ref(name, mode)
    got = mut(name)
    assert got, "the case does not cover the mutation"
    for k, v in got.items():
        r = R.ratio(v, want["grads"][k], want["A"][k], want["n"][k], R.C[R.kind_of(k, case.fields)])
        print(f"RECORD-MUTATION {mut.__name__[4:]} {name} {k}: {r:.3g}")
        assert r > 1.0, f"{mut.__name__} passes the bar of {k} in {name} (ratio {r:.3g})"


@pytest.mark.parametrize("name", ["widths_D4", "widths_D16", "widths_D64", "bags_D16"])
def test_forward_mutations_land_outside_the_bar(name):
    ref = R.forward_ref(name)
    muts = R.forward_mutations(name)
    fe = muts["transpose_projection"]["field_embeddings"]
    if any(f["dim"] != R.CASES[name].D for f in R.CASES[name].fields):
        assert R.ratio(fe, ref["field_embeddings"], ref["A"]["field_embeddings"], ref["n"]["field_embeddings"], R.C["forward"]) > 1
    flat = muts["mean_counts_padding"]["flat_embeddings"]
    assert R.ratio(flat, ref["flat_embeddings"], ref["A"]["flat_embeddings"], ref["n"]["flat_embeddings"], R.C["forward"]) > 1
