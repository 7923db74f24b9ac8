"""GPU: row-wise int8 embedding tables (csrc/quant.hip, training/quantized.py, QuantizedPredictor).

Bars: the quantiser, its inverse and the SPARSE columns of the gather match the numpy float32 restatement
(tests/quant_reference.py) bit for bit; the DENSE columns match the fp32 gather bit for bit; every sum is held to the
project's 1e-4 bar (helpers.assert_close) against fp64 sums over the dequantised values, and the predictor's logits to
the same bar against ``FusedPredictor`` on a copy of the model that holds the dequantised tables, which separates kernel
error from quantisation error.  The helpers and the checks shared with the 4-bit format are tests/quant_cases.py's."""
import numpy as np
import pytest
import torch

from tests import quant_cases as QC
from tests import quant_reference as Q
from tests.helpers import npy

pytestmark = pytest.mark.gpu

FMT = QC.INT8
WIDTHS, MIXES, KINDS, PB, PN = QC.WIDTHS, QC.MIXES, QC.KINDS, QC.PB, QC.PN


# ---------------------------------------------------------------------------------------------- quantise / dequantise
def _table(rows, D, rng):
    """(w2 (rows, D), w1 (rows, 1)): row 0 all zero, then in turn a constant row, a one-signed row, a row spanning
    1e-3 .. 1e3 with mixed sign, a normal row."""
    w2 = rng.standard_normal((rows, D)).astype(np.float32)
    for r in range(rows):
        k = r % 5
        if r == 0:
            w2[r] = 0
        elif k == 1:
            w2[r] = np.float32(rng.standard_normal())
        elif k == 2:
            w2[r] = -np.abs(w2[r]) - np.float32(0.5)
        elif k == 3:
            w2[r] = (np.where(rng.random(D) < 0.5, -1, 1) * 10.0 ** rng.uniform(-3, 3, D)).astype(np.float32)
    return w2, rng.standard_normal((rows, 1)).astype(np.float32)


@pytest.mark.parametrize("packed", [False, True], ids=["contiguous", "packed"])
@pytest.mark.parametrize("rows", [1, 2, 3, 257])
@pytest.mark.parametrize("D", WIDTHS)
def test_quantize_and_dequantize_match_the_restatement(D, rows, packed):
    w2, w1 = _table(rows, D, np.random.default_rng([D, rows]))
    want = Q.quantize_table(w2, w1)
    got, flag = QC.quantize_on_device(FMT, w2, w1, D, packed)
    assert flag == 0
    assert np.array_equal(got, want), f"records differ in rows {np.unique(np.nonzero(got != want)[0])[:8]}"
    # the inverse, on the restatement's records: a second, independent route
    o2, o1 = QC.dequantize_on_device(FMT, want, D)
    d2, d1 = Q.dequantize_table(want)
    assert np.array_equal(o2.view(np.uint32), d2.view(np.uint32))
    assert np.array_equal(o1, w1) and np.array_equal(d1, w1)
    assert not o2[0].view(np.uint32).any()                                    # the padding row is exactly 0
    err = np.abs(d2.astype(np.float64) - w2.astype(np.float64))
    assert (err <= Q.bound(w2)[:, None]).all()
    const = [r for r in range(rows) if r % 5 == 1 or r == 0]
    assert np.array_equal(d2[const], w2[const])                               # constant rows are exact


@pytest.mark.parametrize("mode", ["dense", "rowsparse"])
@pytest.mark.parametrize("D", WIDTHS)
def test_tables_from_model_in_both_grad_modes(D, mode):
    """QuantizedTables.from_model on contiguous tables and on packed row records: the restatement's records, bit for
    bit; dequantized() is the restatement's; error_bound() bounds |dequantized - fp32| for every field."""
    from deepfm_amd.training import QuantizedTables
    fields = QC.pred_fields(D)
    model, _ = QC.small_model("deepfm", fields, D, seed=D, packed=(mode == "rowsparse"))
    emb = model.embedding
    assert emb.grad_mode == mode
    tables = QuantizedTables.from_model(model)
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
        assert bounds[name] <= float(Q.bound(w2).max()) * (1 + 1e-6)      # and it is no looser than the stated one
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


@pytest.mark.parametrize("fault", ["nan", "inf", "overflow"])
def test_unquantisable_tables_are_refused_by_name(fault):
    from deepfm_amd.training import QuantizedPredictor, QuantizedTables
    D = 16
    model, _ = QC.small_model("deepfm", QC.pred_fields(D), D)
    w = model.embedding.second_order_embeddings["s3"].weight
    with torch.no_grad():
        if fault == "overflow":         # finite elements whose range is not
            w[96, 3], w[96, 9] = 3e38, -3e38
        else:
            w[41, D - 1] = float(fault)
    with pytest.raises(ValueError, match="'s3'"):
        QuantizedTables.from_model(model)
    with pytest.raises(ValueError, match="'s3'"):
        QuantizedPredictor(model, 64)
    with torch.no_grad():
        w[96], w[41] = 0.25, -0.25
    tables = QuantizedTables.from_model(model)                  # no stale flag
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


def test_gather_refuses_49_sparse_fields():
    from deepfm_amd import _lib
    fields, emb, host, recs, deq = QC.gather_setup(FMT, 49, 1, 16)
    batch = QC.edge_batch(fields, 5, np.random.default_rng(49))
    rc = QC.quant_call(FMT, emb, fields, 16, recs, QC.device_inputs(fields, batch), 5, check=False)
    assert rc == _lib.ERR_UNSUPPORTED
    assert "at most 48 SPARSE and 32 DENSE" in _lib.load().dfm_last_error().decode()


@pytest.mark.parametrize("bad", [-1, "vocab"])
@pytest.mark.parametrize("D,mix", [(16, (26, 13)), (32, (48, 16)), (64, (3, 2))])
def test_gather_out_of_range_id_sets_the_flag_and_scores_as_id_0(D, mix, bad):
    QC.check_out_of_range_id(FMT, D, mix, bad, np.random.default_rng(D * 1000 + mix[0] * 10 + mix[1]))


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


def test_predictor_refuses_other_tables():
    from deepfm_amd.training import QuantizedPredictor, QuantizedTables
    D = 16
    fields = QC.pred_fields(D)
    model, _ = QC.small_model("deepfm", fields, D)
    other = [dict(f, vocab=98) if f["name"] == "s3" else f for f in fields]
    tables = QuantizedTables.from_model(QC.small_model("deepfm", other, D)[0])
    with pytest.raises(ValueError, match="'s3'"):
        QuantizedPredictor(model, PB, tables=tables)
    host = QuantizedTables.from_records(model.schema, D, {n: r.cpu() for n, r in
                                                          QuantizedTables.from_model(model).records.items()})
    with pytest.raises(ValueError, match="QuantizedTables.to"):
        QuantizedPredictor(model, PB, tables=host)
    pred = QuantizedPredictor(model, PB, tables=host.to("cuda"), use_graph=False)
    rec = QC.records(pred, fields, np.random.default_rng(0), 1)[0]
    assert torch.equal(pred.predict_from(rec, PN), QuantizedPredictor(model, PB).predict_from(rec, PN))
