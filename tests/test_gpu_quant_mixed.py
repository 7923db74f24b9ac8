"""GPU: quantised tables for SEQUENCE, projected and mixed-width schemas (``dfm_embedding_forward_record_quant``,
``QuantizedMixedTables``, ``QuantizedMixedPredictor``), in both record formats.

Every gather case (tests/quant_mixed_reference.py: the record matrix's forward cases that have something to quantise,
and the extra ones) runs three ways: (i) the new gather, (ii) ``dfm_embedding_forward_record`` on a copy of the module
whose quantised fields hold ``tables.dequantized()``, (iii) the numpy restatement.  Bars:
  1. fe, flat, first_order and fm_sum equal (ii) bit for bit; so does fm, because the new kernel lives in
     csrc/embedding.hip and shares the fp32 gather's epilogue under the same contraction;
  2. what the restatement covers equals (iii) bit for bit;
  3. the fp32 fields' columns equal the fp32 gather on the original module bit for bit;
  4. every output is within the record matrix's forward bars of the fp64 gather over the dequantised tables;
  5. some quantised column differs from the fp32 module's: a kernel that ignored the records would not pass.
Outputs live in guarded buffers filled with NaN, as in tests/test_gpu_record_matrix.py."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from deepfm_amd import _lib
from tests import helpers as H
from tests import quant_cases as QC
from tests import quant_mixed_reference as M
from tests import record_cases as R

pytestmark = pytest.mark.gpu

FORMATS = [QC.INT8, QC.UINT4]
FMT_IDS = [f.name for f in FORMATS]
NAN_BITS = 0x7FC00000
OUT = ("first_order", "field_embeddings", "flat_embeddings", "fm", "fm_sum")
F32 = np.float32


# ----------------------------------------------------------------------------- helpers
def _emb(fields, D, params):
    from deepfm_amd.models.layers.embedding import FeatureEmbedding
    emb = FeatureEmbedding(H.schema_from_fields(fields), D)
    emb.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return emb.cuda()


def _shim(emb):
    """What QuantizedMixedTables reads of a model."""
    return types.SimpleNamespace(schema=emb.schema, embedding=emb, parameters=emb.parameters)


def _device_record(fields, B, batch, labels):
    from deepfm_amd.data.packed import RecordLayout
    lay = RecordLayout.of(H.schema_from_fields(fields), B)
    rec = torch.zeros(lay.record_bytes, dtype=torch.uint8, device="cuda")
    views, lab = lay.unpack(rec)
    for k, dst in views.items():
        dst.copy_(torch.from_numpy(batch[k]).to(dst.dtype).view_as(dst))
    lab.copy_(torch.from_numpy(labels))
    assert rec.data_ptr() % 16 == 0
    return rec


def _qrows(emb, records):
    return (C.c_void_p * len(emb.field_names))(*[records[n].data_ptr() if n in records else None
                                                 for n in emb.field_names])


def _is_nan_pattern(t) -> bool:
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gather(emb, rec, B, F, D, T, quant=None, fe=True, fm=True, lab=True, S=True):
    """One launch into guarded buffers; ``quant`` = (qrows, format enum) for the new entry point, None for
    ``dfm_embedding_forward_record``.  Returns numpy outputs and the module's error flag (cleared)."""
    ld = T + R.LD_PAD_FLAT
    b = dict(fo=H.GuardedBuffer(B), fe=H.GuardedBuffer(B * F * D), flat=H.GuardedBuffer(B * ld + 4),
             fm=H.GuardedBuffer(B), lab=H.GuardedBuffer(B), S=H.GuardedBuffer(B * D))
    args = (rec.data_ptr(), B, b["fo"].t, b["fe"].t if fe else None, b["flat"].ptr() + 16, ld,
            b["fm"].t if fm else None, b["lab"].t if lab else None)
    if quant is None:
        emb.forward_record(*args, fm_sum=b["S"].t if S else None)
    else:
        emb.forward_record_quant(quant[0], quant[1], *args, fm_sum=b["S"].t if S else None)
    torch.cuda.synchronize()
    for k, g in b.items():
        assert g.guards_intact(), f"guard band of {k} written"
    assert _is_nan_pattern(b["flat"].t[:4]), "the floats before an offset flat pointer"
    rows = b["flat"].t[4:].view(B, ld)
    assert _is_nan_pattern(rows[:, T:]), "columns of a wider flat row outside the schema"
    for k, on in (("fe", fe), ("fm", fm), ("lab", lab), ("S", S)):
        assert on or _is_nan_pattern(b[k].t), f"{k} written without being asked for"
    flag = int(emb._err.item())
    emb._err.zero_()
    return dict(first_order=H.npy(b["fo"].t), field_embeddings=H.npy(b["fe"].view(B, F, D)),
                flat_embeddings=H.npy(rows[:, :T].contiguous()), fm=H.npy(b["fm"].t), fm_sum=H.npy(b["S"].view(B, D)),
                labels=H.npy(b["lab"].t), flag=flag)


@functools.lru_cache(maxsize=None)
def _setup(name, fmt):
    """Module, tables, the dequantised copy and the device record of a case, built once and left unchanged."""
    from deepfm_amd.training import QuantizedMixedTables
    case, inp, fields = M.case_of(name), M.inputs(name), M.fields_of(name)
    emb = _emb(fields, case.D, inp["params"])
    tables = QuantizedMixedTables.from_model(_shim(emb), fmt.name)
    deq = _emb(fields, case.D, inp["params"])
    with torch.no_grad():
        for n, (w2, w1) in tables.dequantized().items():
            deq.second_order_embeddings[n].weight.copy_(w2)
            deq.first_order_embeddings[n].weight.copy_(w1)
    rec = _device_record(fields, case.B, inp["batch"], inp["labels"])
    return case, inp, fields, emb, tables, deq, rec


# ----------------------------------------------------------------------------- the gather matrix
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name", M.ALL_CASES)
def test_quantised_gather(name, fmt):
    case, inp, fields, emb, tables, deq, rec = _setup(name, fmt)
    B, F, D, T = case.B, case.F, case.D, case.T
    quant = (_qrows(emb, tables.records), fmt.enum)
    host = M.host_records(fmt.name, fields, inp["params"])
    assert list(tables.records) == list(host) and tables.fp32_fields == [
        f["name"] for f in fields if f["type"] != "dense" and f["name"] not in host]
    for n, r in host.items():                  # the device quantiser's records are the restatement's, at each width
        assert fmt.row_bytes(tables.dims[n]) == r.shape[1] == tables.row_bytes(n)
        assert np.array_equal(H.npy(tables.records[n]), r), f"{n}: records"

    got = _gather(emb, rec, B, F, D, T, quant)                       # (i)
    two = _gather(deq, rec, B, F, D, T)                              # (ii)
    orig = _gather(emb, rec, B, F, D, T)                             # the fp32 module, for bars 3 and 5
    assert got["flag"] == 0 and two["flag"] == 0
    assert np.array_equal(got["labels"], inp["labels"])
    for k in OUT:                                                    # bar 1 (and fm: one epilogue, one contraction)
        assert np.array_equal(_bits(got[k]), _bits(two[k])), f"{name} {k}: differs from the gather over dequantised tables"
    ref = H.record_forward_fp64(fields, M.dequantised_params(fmt.name, fields, inp["params"], host), inp["batch"], D)
    for k in OUT:                                                    # bar 4
        r = R.ratio(got[k], ref[k], ref["A"][k], ref["n"][k], R.C["forward"])
        print(f"QUANT-MIXED-RATIO {name} {fmt.name} {k}: {r:.3f}")
        assert r <= 1.0, f"{name} {k}: worst |err| / bar = {r:.3f}"
    off, differs, fo_rest = 0, False, np.zeros(B, np.float64)
    for f, spec in enumerate(fields):
        d = spec["dim"]
        cols = slice(off, off + d)
        if spec["name"] in host:                                     # bar 2
            raw, fo = M.field(fmt.name, host[spec["name"]], spec, inp["batch"][spec["name"]])
            assert np.array_equal(_bits(got["flat_embeddings"][:, cols]), _bits(raw)), f"{spec['name']}: flat vs numpy"
            if d == D:
                assert np.array_equal(_bits(got["field_embeddings"][:, f]), _bits(raw)), f"{spec['name']}: fe vs numpy"
            fo_rest += fo.astype(np.float64)
            differs |= not np.array_equal(got["flat_embeddings"][:, cols], orig["flat_embeddings"][:, cols])
        else:                                                        # bar 3
            assert np.array_equal(_bits(got["flat_embeddings"][:, cols]), _bits(orig["flat_embeddings"][:, cols]))
            assert np.array_equal(_bits(got["field_embeddings"][:, f]), _bits(orig["field_embeddings"][:, f]))
        off += d
    assert differs, "no quantised column differs from the fp32 table's: the records were not read"    # bar 5
    if F == 1:                                                       # a single quantised field: first_order is its w1
        assert np.array_equal(got["first_order"], fo_rest.astype(F32))

    bare = _gather(emb, rec, B, F, D, T, quant, fe=False, fm=False, lab=False, S=False)
    for k in ("first_order", "flat_embeddings"):
        assert np.array_equal(_bits(bare[k]), _bits(got[k])), f"{k} changes bits without fe / fm / fm_sum / labels"
    nosum = _gather(emb, rec, B, F, D, T, quant, S=False)
    for k in ("first_order", "field_embeddings", "flat_embeddings", "fm", "labels"):
        assert np.array_equal(_bits(nosum[k]), _bits(got[k])), f"{k} changes bits with fm_sum off"


def test_first_order_of_quantised_fields_equals_the_restatement():
    """A schema of quantised fields only, summed over the fields in order: first_order bit for bit from numpy."""
    for fmt in FORMATS:
        fields = [M.sp("a", 9, 16), M.seq("h", 17, 16, 5, "mean"), M.seq("m", 11, 16, 2, "max"),
                  M.seq("s", 13, 16, 50, "sum")]
        rng = np.random.default_rng(5)
        params, batch = {}, {}
        for f in fields:
            k2, k1 = H._rec_keys(f["name"])[:2]
            params[k2] = rng.uniform(-1, 1, (f["vocab"], 16)).astype(F32)
            params[k1] = rng.uniform(-1, 1, (f["vocab"], 1)).astype(F32)
            ids = rng.integers(0, f["vocab"], (7, f["max_len"]), dtype=np.int64)
            batch[f["name"]] = ids if f["type"] == "sequence" else ids[:, 0].copy()
        emb = _emb(fields, 16, params)
        host = M.host_records(fmt.name, fields, params)
        recs = {n: torch.from_numpy(r).cuda() for n, r in host.items()}
        rec = _device_record(fields, 7, batch, np.zeros(7, F32))
        got = _gather(emb, rec, 7, 4, 16, 64, (_qrows(emb, recs), fmt.enum))
        want = np.zeros(7, F32)
        for f in fields:
            want = (want + M.field(fmt.name, host[f["name"]], f, batch[f["name"]])[1]).astype(F32)
        assert np.array_equal(_bits(got["first_order"]), _bits(want)), fmt.name


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name", ["widths_D16", "q_bags_D16", "wide_F64_D64", "q_proj_D8"])
def test_without_records_the_entry_point_is_the_fp32_gather(name, fmt):
    """Every quant_rows[f] NULL: every output, fm included (the kernel lives in csrc/embedding.hip), bit for bit."""
    case, inp, fields, emb, tables, deq, rec = _setup(name, fmt)
    B, F, D, T = case.B, case.F, case.D, case.T
    none = (C.c_void_p * F)()
    got = _gather(emb, rec, B, F, D, T, (none, fmt.enum))
    want = _gather(emb, rec, B, F, D, T)
    for k in OUT + ("labels",):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("where", ["u", "h", "m"])          # a SPARSE column, inside a mean bag, inside a max bag
@pytest.mark.parametrize("bad", [-1, "vocab"])
def test_out_of_range_id_sets_the_flag_and_scores_as_id_0(fmt, where, bad):
    sb = R.fwd_sb(6, 16)
    case, inp, fields, emb, tables, deq, _ = _setup(f"q_edge_B{sb + 1}", fmt)      # the ragged tail workgroup
    B, F, D, T = case.B, case.F, case.D, case.T
    spec = next(f for f in fields if f["name"] == where)
    quant = (_qrows(emb, tables.records), fmt.enum)
    outs = []
    for value in (-1 if bad == -1 else spec["vocab"], 0):
        batch = {k: v.copy() for k, v in inp["batch"].items()}
        if spec["type"] == "sparse":
            batch[where][B - 1] = value
        else:
            batch[where][B - 1] = [3] + [1] * (spec["max_len"] - 1)
            batch[where][B - 1, spec["max_len"] // 2] = value
        outs.append(_gather(emb, _device_record(fields, B, batch, inp["labels"]), B, F, D, T, quant))
    assert outs[0]["flag"] == 1 and outs[1]["flag"] == 0
    for k in OUT:
        assert np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])), k


def test_entry_point_refusals():
    """Host-side, with a message, before anything is launched: a quantised narrow field, a quantised DENSE field, a bad
    format, a misaligned base, a plan the record gather refuses."""
    lib = _lib.load()
    sb = R.fwd_sb(6, 16)
    case, inp, fields, emb, tables, deq, rec = _setup(f"q_edge_B{sb}", QC.INT8)
    B, F, D, T = case.B, case.F, case.D, case.T
    fo, flat = torch.full((B,), 7.0, device="cuda"), torch.full((B, T), 7.0, device="cuda")
    names = list(emb.field_names)
    base = tables.records["u"].data_ptr()

    def call(e, rows, fmt=_lib.QUANT_INT8_ROWWISE, nfields=F):
        arr = (C.c_void_p * nfields)(*rows)
        plan = e._ensure_plan(torch.device("cuda", torch.cuda.current_device()))
        return lib.dfm_embedding_forward_record_quant(plan, arr, fmt, C.c_void_p(rec.data_ptr()), B, fo.data_ptr(), None,
                                                      C.c_void_p(flat.data_ptr()), T, None, None, None,
                                                      e._err.data_ptr(), _lib.stream_handle())

    def rows(**at):
        return [at.get(n) for n in names]

    assert call(emb, rows(n8=base)) == _lib.ERR_UNSUPPORTED
    assert "width 8" in lib.dfm_last_error().decode() and "16, 32 and 64" in lib.dfm_last_error().decode()
    assert call(emb, rows(x=base)) == _lib.ERR_UNSUPPORTED and "DENSE" in lib.dfm_last_error().decode()
    assert call(emb, rows(u=base), fmt=2) == _lib.ERR_UNSUPPORTED
    assert "DFM_QUANT_INT8_ROWWISE" in lib.dfm_last_error().decode()
    assert call(emb, rows(u=base + 8)) == 1 and "16-byte aligned" in lib.dfm_last_error().decode()
    bad = R.CASES["refuse_D12"]
    e12 = _emb([dict(f) for f in bad.fields], bad.D, R.inputs("refuse_D12")["params"])
    assert call(e12, [None] * bad.F, nfields=bad.F) == _lib.ERR_UNSUPPORTED
    assert "record gather: fm_embed_dim 12" in lib.dfm_last_error().decode()
    torch.cuda.synchronize()
    assert bool((fo == 7.0).all()) and bool((flat == 7.0).all()), "a refused call wrote its outputs"
    assert call(emb, rows(u=base)) == 0                               # and the same call, well formed, goes through
    torch.cuda.synchronize()
    assert not bool((fo == 7.0).any())


# ----------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_tables_refresh_in_place_and_name_the_table_they_refuse(fmt):
    from deepfm_amd.training import QuantizedMixedTables
    name = "q_proj_D16"                        # SEQUENCE fields, widths 4, 8, 16, 32 and 64
    case, inp, fields = M.case_of(name), M.inputs(name), M.fields_of(name)
    emb = _emb(fields, case.D, inp["params"])
    tables = QuantizedMixedTables.from_model(_shim(emb), fmt.name)
    host = M.host_records(fmt.name, fields, inp["params"])
    assert tables.dims == {"s32": 32, "g32": 32, "s64": 64, "g64": 64, "m64": 64, "s16": 16}
    assert tables.fp32_fields == ["n4", "n8"]
    for n, r in host.items():
        assert np.array_equal(H.npy(tables.records[n]), r), n
    assert tables.nbytes == sum(r.size for r in host.values())
    ptrs = {n: r.data_ptr() for n, r in tables.records.items()}
    with torch.no_grad():
        emb.second_order_embeddings["g64"].weight[3].mul_(2.0)
    assert tables.refresh() is tables and ptrs == {n: r.data_ptr() for n, r in tables.records.items()}
    assert not np.array_equal(H.npy(tables.records["g64"])[3], host["g64"][3])
    assert np.array_equal(H.npy(tables.records["g64"])[:3], host["g64"][:3])
    sub = QuantizedMixedTables.from_model(_shim(emb), fmt.name, fields=["g32", "s16"])
    assert list(sub.records) == ["g32", "s16"] and sub.fp32_fields == ["s32", "s64", "g64", "m64", "n4", "n8"]
    assert np.array_equal(H.npy(sub.records["g32"]), host["g32"])
    # a NaN in a narrow fp32 field's table is not these tables' business
    with torch.no_grad():
        emb.second_order_embeddings["n8"].weight[2, 1] = float("nan")
    tables.refresh()
    with torch.no_grad():
        emb.second_order_embeddings["g32"].weight[5, 7] = float("nan")
    with pytest.raises(ValueError, match="'g32'"):
        tables.refresh()
    with pytest.raises(ValueError, match="'g32'"):
        QuantizedMixedTables.from_model(_shim(emb), fmt.name)


# ----------------------------------------------------------------------------- the predictor
PB, PN = 64, 37
KINDS = ["deepfm", "xdeepfm", "attention_deepfm"]


def _movielens_fields():
    return H.fields_of(H.load("model_deepfm_movielens"))


def _history_fields():
    """A small history schema: user, item, a mean bag of L = 5 earlier items of the same catalogue at width 16, narrow
    SPARSE fields of widths 4 and 8 and two DENSE fields."""
    return [M.sp("user_id", 23, 16), M.sp("item_id", 41, 16), M.seq("hist", 41, 16, 5, "mean"), M.sp("n4", 7, 4),
            M.sp("n8", 9, 8), M.de("x", 4), M.de("y", 8)]


SCHEMAS = {"movielens": _movielens_fields, "history": _history_fields}
QUANTISED = {"movielens": ["user_id", "movie_id"], "history": ["user_id", "item_id", "hist"]}


def _host_record(layout, schema, feats, labels, start, n):
    from deepfm_amd.data.packed import PackedColumns
    host = np.zeros(layout.record_bytes, np.uint8)
    layout.write(host, PackedColumns(schema, feats, labels), start, start + n)
    return torch.from_numpy(host).cuda()


def _records(pred, fields, rng, count, n=PN):
    feats = H.random_fields_batch(fields, count * n, rng, zero_frac=0.15)
    labels = (rng.random(count * n) < 0.3).astype(F32)
    return [_host_record(pred.layout, pred.model.schema, feats, labels, k * n, n) for k in range(count)]


def _overwrite_quantised_tables(model, names, value=None):
    """The fp32 tables of the quantised fields filled with garbage (``value`` None: other finite values)."""
    with torch.no_grad():
        for n in names:
            for which in (model.embedding.second_order_embeddings, model.embedding.first_order_embeddings):
                w = which[n].weight
                w.fill_(value) if value is not None else w.uniform_(-2.0, 2.0)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("schema", list(SCHEMAS))
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_predictor(fmt, schema, kind, use_graph):
    from deepfm_amd.training import MixedSchemaPredictor, QuantizedMixedPredictor, QuantizedMixedTables
    fields = SCHEMAS[schema]()
    model, _ = QC.small_model(kind, fields, 16, seed=3)
    tables = QuantizedMixedTables.from_model(model, **QC.fmt_kw(fmt))
    assert list(tables.records) == QUANTISED[schema]
    other = "int8" if fmt is QC.UINT4 else "uint4"
    pred = QuantizedMixedPredictor(model, PB, tables=tables, use_graph=use_graph, fmt=other)   # the tables decide
    assert pred.tables is tables and pred.tables.format == fmt.name and model.training
    assert isinstance(pred, MixedSchemaPredictor) and bool(pred.slots) == use_graph
    ref = MixedSchemaPredictor(QC.dequantized_copy(kind, fields, 16, model, tables), PB, use_graph=False)
    fp32 = MixedSchemaPredictor(model, PB, use_graph=False)
    rng = np.random.default_rng(len(kind) + len(schema))
    recs = _records(pred, fields, rng, 4)
    first = []
    for k, rec in enumerate(recs):              # four records: both graph slots are re-pointed
        p = pred.predict_from(rec, PN)
        lg = pred.last_logits(PN)
        want_p = ref.predict_from(rec, PN)
        assert p.shape == (PN, 1)
        H.assert_close(H.npy(lg), H.npy(ref.last_logits(PN)), what=f"{kind} record {k} logits")
        H.assert_close(H.npy(p), H.npy(want_p), what=f"{kind} record {k} probabilities")
        fp32.predict_from(rec, PN)
        assert not torch.equal(lg, fp32.last_logits(PN)), "the logits are the fp32 model's: the records were not read"
        first.append((p.clone(), lg.clone()))
    model.embedding.raise_on_bad_index()
    # after construction the fp32 tables of the quantised fields are never read: NaN in all of them changes no bit
    saved = {k: v.clone() for k, v in model.state_dict().items()}
    _overwrite_quantised_tables(model, tables.records, float("nan"))
    for k, rec in enumerate(recs):
        assert torch.equal(pred.predict_from(rec, PN), first[k][0]) and torch.equal(pred.last_logits(PN), first[k][1]), k
    # other finite values: still no bit, until refresh() requantises them into the same buffers
    _overwrite_quantised_tables(model, tables.records)
    assert torch.equal(pred.predict_from(recs[0], PN), first[0][0])
    ptrs = {n: r.data_ptr() for n, r in tables.records.items()}
    tables.refresh()
    assert ptrs == {n: r.data_ptr() for n, r in tables.records.items()}
    assert not torch.equal(pred.predict_from(recs[0], PN), first[0][0])
    model.load_state_dict(saved)
    tables.refresh()
    assert torch.equal(pred.predict_from(recs[0], PN), first[0][0])
    # the dict API agrees with the record API
    batch, _ = pred.layout.unpack(recs[2])
    assert torch.equal(pred.predict({k: v[:PN] for k, v in batch.items()}), first[2][0])


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_refresh_after_a_training_step(fmt, kind, use_graph):
    """One fused mixed-schema training step on every parameter, then refresh(): the predictor, its graphs untouched,
    gives the predictions of freshly built tables."""
    from deepfm_amd.training import (DenseTableAdam, MixedSchemaPredictor, QuantizedMixedPredictor,
                                     QuantizedMixedTables, mixed_step_class)
    fields = _history_fields()
    model, _ = QC.small_model(kind, fields, 16, seed=5)
    opt = DenseTableAdam(model, lr=0.05)                        # re-homes the parameters: before any predictor
    step = mixed_step_class(model)(model, opt, PB, use_graph=True)
    step.capture()
    pred = QuantizedMixedPredictor(model, PB, use_graph=use_graph, **QC.fmt_kw(fmt))      # tables=None: built here
    tables = pred.tables
    assert tables.format == fmt.name and list(tables.records) == QUANTISED["history"]
    rng = np.random.default_rng(11)
    recs = _records(pred, fields, rng, 2)
    before = pred.predict_from(recs[0], PN).clone()
    graphs = [s.graph for s in pred.slots]
    ptrs = {n: r.data_ptr() for n, r in tables.records.items()}
    step.run_from(_records(pred, fields, rng, 1, n=PB)[0])
    model.embedding.raise_on_bad_index()
    tables.refresh()
    assert graphs == [s.graph for s in pred.slots] and ptrs == {n: r.data_ptr() for n, r in tables.records.items()}
    fresh = QuantizedMixedTables.from_model(model, fmt.name)
    assert all(torch.equal(fresh.records[n], tables.records[n]) for n in tables.records)
    ref = MixedSchemaPredictor(QC.dequantized_copy(kind, fields, 16, model, fresh), PB, use_graph=False)
    for k, rec in enumerate(recs):
        p = pred.predict_from(rec, PN)
        want = ref.predict_from(rec, PN)
        H.assert_close(H.npy(pred.last_logits(PN)), H.npy(ref.last_logits(PN)), what=f"{kind} record {k} logits")
        H.assert_close(H.npy(p), H.npy(want), what=f"{kind} record {k} probabilities")
    assert not torch.equal(pred.predict_from(recs[0], PN), before)          # the step did move the scores


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_evaluate_calibrator_and_importance_agree_with_the_dequantised_copy(fmt, kind):
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import Calibrator, MixedSchemaPredictor, QuantizedMixedPredictor
    fields = _movielens_fields()
    model, _ = QC.small_model(kind, fields, 16, seed=7)
    rng = np.random.default_rng(5)
    n = 3 * PB + 11
    feats = H.random_fields_batch(fields, n, rng, zero_frac=0.05)
    cols = PackedColumns(model.schema, feats, (rng.random(n) < 0.4).astype(F32))
    kw = dict(ranking_ks=[1, 5], group_auc=True, calibration_bins=10)
    quant = QuantizedMixedPredictor(model, PB, **QC.fmt_kw(fmt))
    copy = QC.dequantized_copy(kind, fields, 16, model, quant.tables)
    ref = MixedSchemaPredictor(copy, PB)
    got, want = quant.evaluate(cols, **kw), ref.evaluate(cols, **kw)
    assert set(got) == set(want) and {"auc", "logloss", "HR@1", "NDCG@5", "gauc", "ece"} <= set(got)
    H.assert_close(H.npy(quant.last_scores), H.npy(ref.last_scores), what=f"{kind} scores")
    assert torch.equal(quant.last_labels, ref.last_labels)
    # a calibrator rides in the same launches; collect_logits is inherited
    labels, logits = quant.collect_logits(cols)
    H.assert_close(H.npy(logits), H.npy(ref.collect_logits(cols)[1]), what=f"{kind} collected logits")
    cal = Calibrator("platt").fit(labels, logits)
    qc = QuantizedMixedPredictor(model, PB, tables=quant.tables, calibrator=cal)
    rc = MixedSchemaPredictor(copy, PB, calibrator=cal)
    rec = _host_record(qc.layout, model.schema, feats, cols.labels, 0, PB)
    H.assert_close(H.npy(qc.predict_from(rec)), H.npy(rc.predict_from(rec)), what=f"{kind} calibrated probabilities")
    assert torch.equal(qc.predict_from(rec), cal.apply(qc.last_logits()))
    # permutation importance: the same permutations of the same rows.  The quantised gather equals the fp32 gather over
    # the dequantised tables bit for bit (bar 1 of the matrix, fm included) and the rest is the same launches, so the
    # two reports are equal, not merely close
    a = quant.field_importance(cols, fields=["user_id", "genres"], repeats=1, seed=3)
    b = ref.field_importance(cols, fields=["user_id", "genres"], repeats=1, seed=3)
    assert a.groups == b.groups == ["user_id", "genres"] and a.metrics == b.metrics
    assert a == b


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_evaluate_loader_over_history_bags_from_the_index(fmt):
    """The bag column comes from ``index.lookup``; the rows never leave the device.  The quantised gather equals the
    fp32 gather over the dequantised tables bit for bit (bar 1 above, fm included) and everything behind it is the
    same launches, so the scores and with them every metric are equal, not merely close."""
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data import DeviceColumns, DeviceEpochLoader, DeviceInteractionLog, history_field
    from deepfm_amd.data.schema import DatasetSchema, FeatureType, FieldSchema
    from deepfm_amd.models import create_model
    from deepfm_amd.training import MixedSchemaPredictor, QuantizedMixedPredictor
    rng = np.random.default_rng(8)
    n, n_users, n_items, L = 300, 12, 40, 5
    user = rng.integers(0, n_users, n).astype(np.int64)
    item = rng.integers(0, n_items, n).astype(np.int64)
    ts = rng.integers(0, 60, n).astype(np.int64)
    labels = (rng.random(n) < 0.6).astype(F32)
    log = DeviceInteractionLog(user, item, ts, labels, n_users, n_items, "cuda")
    schema = DatasetSchema(fields={
        "user_id": FieldSchema("user_id", FeatureType.SPARSE, n_users + 1, 16, "user"),
        "item_id": FieldSchema("item_id", FeatureType.SPARSE, n_items + 1, 16, "item"),
        "hist": history_field("hist", L, n_items, 16)})
    rows = torch.arange(n, device="cuda")
    hist = log.history_index().lookup(rows, L)
    assert bool((hist.bag != 0).any()) and not bool(hist.bag[:, L - 1].all())
    ids = torch.stack([log.user_rows[rows] + 1, log.item_rows[rows] + 1]).contiguous()
    dense = torch.empty(0, n, dtype=torch.float32, device="cuda")
    dcols = DeviceColumns.from_device(schema, ids, dense, log.labels[rows].contiguous(), bags=[hist.bag])
    loader = DeviceEpochLoader(dcols, PB, shuffle=False)

    def make(seed):
        cfg = ExperimentConfig()
        cfg.feature.fm_embed_dim = 16
        cfg.dnn.hidden_units, cfg.dnn.dropout = [32, 32], 0.0
        torch.manual_seed(seed)
        m = create_model("deepfm", schema, cfg).cuda().train()
        with torch.no_grad():
            for name in schema.fields:
                m.embedding.second_order_embeddings[name].weight[1:].uniform_(-0.5, 0.5)
                m.embedding.first_order_embeddings[name].weight[1:].uniform_(-0.5, 0.5)
        return m
    model = make(3)
    quant = QuantizedMixedPredictor(model, PB, **QC.fmt_kw(fmt))
    assert list(quant.tables.records) == ["user_id", "item_id", "hist"]
    copy = make(4)
    copy.load_state_dict(model.state_dict())
    with torch.no_grad():
        for name, (w2, w1) in quant.tables.dequantized().items():
            copy.embedding.second_order_embeddings[name].weight.copy_(w2)
            copy.embedding.first_order_embeddings[name].weight.copy_(w1)
    ref, fp32 = MixedSchemaPredictor(copy, PB), MixedSchemaPredictor(model, PB)
    kw = dict(ranking_ks=[1, 5], group_auc=True)
    got, want = quant.evaluate_loader(loader, **kw), ref.evaluate_loader(loader, **kw)
    assert list(got) == list(want) and {"auc", "logloss", "HR@5", "gauc"} <= set(got)
    assert torch.equal(quant.last_scores, ref.last_scores)
    assert got == want
    fp32.evaluate_loader(loader, **kw)
    assert not torch.equal(quant.last_scores, fp32.last_scores)
