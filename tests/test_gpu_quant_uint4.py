"""GPU: row-wise 4-bit embedding tables (csrc/quant.hip with DFM_QUANT_UINT4_ROWWISE, training/quantized.py and
QuantizedPredictor with ``"uint4"``).

Bars, as tests/test_gpu_quant.py: the quantiser, its inverse and the SPARSE columns of the gather match the numpy
restatement (tests/quant4_reference.py) bit for bit; the DENSE columns match the fp32 gather bit for bit; every sum is
held to the project's 1e-4 bar (helpers.assert_close) against fp64 sums over the dequantised values, and the predictor's
logits to the same bar against ``FusedPredictor`` on a copy of the model that holds the dequantised tables.  The helpers
and the checks shared with the int8 format are tests/quant_cases.py's."""
import numpy as np
import pytest
import torch

from tests import quant4_reference as Q
from tests import quant_cases as QC
from tests.helpers import npy

pytestmark = pytest.mark.gpu

FMT = QC.UINT4
WIDTHS, MIXES, KINDS, PB, PN = QC.WIDTHS, QC.MIXES, QC.KINDS, QC.PB, QC.PN
F16, F32 = np.float16, np.float32


# ---------------------------------------------------------------------------------------------- quantise / dequantise
def _table(rows, D, rng):
    """(w2 (rows, D), w1 (rows, 1)) of trained-like values with, in turn: row 0 all zero; a constant row at a value
    binary16 cannot represent; a row of range 1e-9 above 0 (scale 2^-24, every code 0); a row whose minimum is a tiny
    negative number (lo: -0 stepped to -2^-24); a row whose minimum binary16 represents exactly; a row with
    lo = -1 and hi = 0.875 + 2^-24, whose range rounds down to 1.875 and its fifteenth to the binary16 value 0.125, so
    that the scale needs its extra step to reach hi."""
    w2 = rng.uniform(-0.5, 0.5, (rows, D)).astype(F32)
    for r in range(rows):
        k = r % 6
        if r == 0:
            w2[r] = 0
        elif k == 1:
            v = F32(0.1) * F32(1 + r)
            w2[r] = v if F32(F16(v)) != v else np.nextafter(v, F32(np.inf))
        elif k == 2:
            w2[r] = (1e-9 * rng.random(D)).astype(F32)
        elif k == 3:
            w2[r] = np.abs(w2[r])
            w2[r, r % D] = F32(-1e-9)
        elif k == 4:
            w2[r, (3 * r) % D] = F32(-0.75)
        elif k == 5:
            w2[r, r % D], w2[r, (r + 7) % D] = F32(-1.0), F32(0.875) + F32(2.0 ** -24)
    return w2, rng.standard_normal((rows, 1)).astype(F32)


@pytest.mark.parametrize("packed", [False, True], ids=["contiguous", "packed"])
@pytest.mark.parametrize("rows", [1, 2, 3, 257])
@pytest.mark.parametrize("D", WIDTHS)
def test_quantize_and_dequantize_match_the_restatement(D, rows, packed):
    w2, w1 = _table(rows, D, np.random.default_rng([D, rows]))
    want = Q.quantize_table(w2, w1)
    got, flag = QC.quantize_on_device(FMT, w2, w1, D, packed)
    assert flag == 0
    assert np.array_equal(got, want), f"records differ in rows {np.unique(np.nonzero(got != want)[0])[:8]}"
    scale, lo, _, q = Q.unpack(want)
    if rows == 257:                             # the special rows are what they are meant to be
        assert scale[2] == F16(2.0 ** -24) and not q[2].any()
        assert lo[3].view(np.uint16) == 0x8001
        assert lo[4] == F16(-0.75) and F32(lo[1]) < w2[1, 0] and scale[1] > 0
        assert lo[5] == F16(-1.0) and scale[5] == np.nextafter(F16(0.125), F16(1)) and w2[5].max() > 0.875
    # the inverse, on the restatement's records: a second, independent route
    o2, o1 = QC.dequantize_on_device(FMT, want, D)
    d2, d1 = Q.dequantize_table(want)
    assert np.array_equal(o2.view(np.uint32), d2.view(np.uint32))
    assert np.array_equal(o1, w1) and np.array_equal(d1, w1)
    assert not o2[0].view(np.uint32).any()                                    # the padding row is exactly 0
    err = np.abs(d2.astype(np.float64) - w2.astype(np.float64))
    assert (err <= Q.bound(w2)[:, None]).all()


@pytest.mark.parametrize("mode", ["dense", "rowsparse"])
@pytest.mark.parametrize("D", WIDTHS)
def test_tables_from_model_in_both_grad_modes(D, mode):
    """QuantizedTables.from_model(fmt="uint4") on contiguous tables and on packed row records: the restatement's
    records, bit for bit; dequantized() is the restatement's; error_bound() bounds |dequantized - fp32|."""
    from deepfm_amd.training import QuantizedTables
    fields = QC.pred_fields(D)
    model, _ = QC.small_model("deepfm", fields, D, seed=D, packed=(mode == "rowsparse"))
    emb = model.embedding
    assert emb.grad_mode == mode
    tables = QuantizedTables.from_model(model, fmt="uint4")
    assert tables.format == "uint4" and tables.row_bytes == FMT.row_bytes(D) == 8 + D // 2
    deq = tables.dequantized()
    bounds = tables.error_bound()
    total = 0
    for f in fields:
        if f["type"] != "sparse":
            assert f["name"] not in tables.records
            continue
        name = f["name"]
        w2, w1 = npy(emb.second_order_embeddings[name].weight), npy(emb.first_order_embeddings[name].weight)
        want = Q.quantize_table(w2, w1)
        assert np.array_equal(npy(tables.records[name]), want), name
        d2, d1 = Q.dequantize_table(want)
        assert np.array_equal(npy(deq[name][0]), d2) and np.array_equal(npy(deq[name][1]), w1) and np.array_equal(d1, w1)
        assert not d2[0].any()
        worst = float(np.abs(d2.astype(np.float64) - w2).max())
        assert worst <= bounds[name], (name, worst, bounds[name])
        assert bounds[name] == pytest.approx(float(Q.bound(w2).max()), rel=1e-12)
        total += f["vocab"]
    assert tables.nbytes == total * FMT.row_bytes(D) and tables.fp32_nbytes == total * (4 * D + 4)
    ptrs = {n: r.data_ptr() for n, r in tables.records.items()}
    tables.refresh()
    assert ptrs == {n: r.data_ptr() for n, r in tables.records.items()}
    # the state dict round-trips through host memory into the same buffers
    sd = {k: ({n: t.cpu() for n, t in v.items()} if k == "records" else v) for k, v in tables.state_dict().items()}
    before = {n: r.clone() for n, r in tables.records.items()}
    for r in tables.records.values():
        r.zero_()
    tables.load_state_dict(sd)
    assert all(torch.equal(tables.records[n], before[n]) for n in before)
    with pytest.raises(ValueError, match="format"):
        QuantizedTables.from_model(model).load_state_dict(sd)


@pytest.mark.parametrize("fault", ["nan", "inf", "low", "range"])
def test_unquantisable_tables_are_refused_by_name(fault):
    from deepfm_amd.training import QuantizedPredictor, QuantizedTables
    D = 16
    model, _ = QC.small_model("deepfm", QC.pred_fields(D), D)
    w = model.embedding.second_order_embeddings["s3"].weight
    with torch.no_grad():
        if fault == "low":              # a minimum below -65504: lo has no binary16
            w[96, 3] = -65505.0
        elif fault == "range":          # finite and above -65504, but (hi - lo) / 15 is beyond binary16
            w[96, 9] = 1.0e6
        else:
            w[41, D - 1] = float(fault)
    with pytest.raises(ValueError, match="'s3'"):
        QuantizedTables.from_model(model, fmt="uint4")
    with pytest.raises(ValueError, match="'s3'"):
        QuantizedPredictor(model, 64, fmt="uint4")
    if fault in ("low", "range"):
        QuantizedTables.from_model(model)                       # int8 holds both rows
    with torch.no_grad():
        w[96], w[41] = 0.25, -0.25
        w[96, 3] = -65504.0                                     # the smallest binary16 itself is held
    tables = QuantizedTables.from_model(model, fmt="uint4")     # no stale flag
    with torch.no_grad():
        model.embedding.first_order_embeddings["s1"].weight[1, 0] = float("nan")
    tables.refresh()        # the first-order weight is copied, not quantised: the model's business, as in fp32
    with torch.no_grad():
        model.embedding.second_order_embeddings["user_id"].weight[22, 0] = float("inf")
    with pytest.raises(ValueError, match="'user_id'"):
        tables.refresh()


# ---------------------------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("mix", MIXES, ids=lambda m: f"{m[0]}s{m[1]}d")
@pytest.mark.parametrize("D", WIDTHS)
def test_gather(D, mix):
    QC.check_gather_matrix(FMT, D, mix)


@pytest.mark.parametrize("D", WIDTHS)
def test_gather_dense_columns_are_the_int8_gathers(D):
    """DENSE columns (and, with no SPARSE field, every output) bit for bit those of the int8 gather."""
    for ns, nd in ((0, 4), (3, 2)):
        fields, emb, host, recs, deq = QC.gather_setup(FMT, ns, nd, D)
        rng = np.random.default_rng(D + ns)
        recs8 = {f["name"]: torch.from_numpy(QC.INT8.ref.quantize_table(
            npy(emb.second_order_embeddings[f["name"]].weight), npy(emb.first_order_embeddings[f["name"]].weight))).cuda()
                 for f in fields if f["type"] == "sparse"}
        de = [j for j, f in enumerate(fields) if f["type"] == "dense"]
        for B in (1, 33, 131):
            batch = QC.edge_batch(fields, B, rng)
            inputs = QC.device_inputs(fields, batch)
            got4 = QC.quant_call(FMT, emb, fields, D, recs, inputs, B)
            got8 = QC.quant_call(QC.INT8, emb, fields, D, recs8, inputs, B)
            assert np.array_equal(got4["fe"][:, de].view(np.uint32), got8["fe"][:, de].view(np.uint32))
            if ns == 0:
                assert np.array_equal(got4["fo"].view(np.uint32), got8["fo"].view(np.uint32))


@pytest.mark.parametrize("bad", [-1, "vocab"])
@pytest.mark.parametrize("D,mix", [(16, (26, 13)), (32, (48, 16)), (64, (3, 2))])
def test_gather_out_of_range_id_sets_the_flag_and_scores_as_id_0(D, mix, bad):
    QC.check_out_of_range_id(FMT, D, mix, bad, np.random.default_rng(D))


# ---------------------------------------------------------------------------------------------- the predictor
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", KINDS)
def test_predictor(kind, use_graph):
    QC.check_predictor(FMT, kind, use_graph)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", KINDS)
def test_refresh_after_a_training_step(kind, use_graph):
    QC.check_refresh_after_a_training_step(FMT, kind, use_graph)


@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_returns_the_fp32_predictors_keys(kind):
    QC.check_evaluate_returns_the_fp32_predictors_keys(FMT, kind)


def test_given_tables_decide_the_format():
    """int8 tables passed with fmt="uint4" still serve int8; uint4 tables serve uint4 under the default fmt."""
    from deepfm_amd.training import QuantizedPredictor, QuantizedTables
    D = 16
    fields = QC.pred_fields(D)
    model, _ = QC.small_model("deepfm", fields, D)
    t8 = QuantizedTables.from_model(model)
    pred = QuantizedPredictor(model, PB, tables=t8, use_graph=False, fmt="uint4")
    assert pred.tables is t8 and pred.tables.format == "int8"
    rec = QC.records(pred, fields, np.random.default_rng(0), 1)[0]
    want8 = QuantizedPredictor(model, PB, use_graph=False).predict_from(rec, PN)
    assert torch.equal(pred.predict_from(rec, PN), want8)
    t4 = QuantizedTables.from_model(model, fmt="uint4")
    got4 = QuantizedPredictor(model, PB, tables=t4, use_graph=False).predict_from(rec, PN)
    want4 = QuantizedPredictor(model, PB, use_graph=False, fmt="uint4").predict_from(rec, PN)
    assert torch.equal(got4, want4) and not torch.equal(got4, want8)
    with pytest.raises(ValueError, match="uint5"):
        QuantizedPredictor(model, PB, fmt="uint5")
