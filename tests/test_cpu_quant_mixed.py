"""CPU: the numpy restatement of the quantised record gather (tests/quant_mixed_reference.py) against the fp64
restatement of the record gather over the dequantised tables; the new entry point's declaration and binding; the
eligibility of ``QuantizedMixedPredictor`` (reasons before any device work); and what ``QuantizedMixedTables`` refuses by
name."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import quant_mixed_reference as M
from tests import record_cases as R
from tests.helpers import fields_of, load, schema_from_fields
from tests.test_cpu_mixed_predict import movielens_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ["int8", "uint4"]
F32 = np.float32


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", M.ALL_CASES)
def test_restatement_agrees_with_the_fp64_gather_over_the_dequantised_tables(name, fmt):
    case, inp, fields = M.case_of(name), M.inputs(name), M.fields_of(name)
    recs = M.host_records(fmt, fields, inp["params"])
    assert recs, "a case with nothing to quantise"
    ref = H.record_forward_fp64(fields, M.dequantised_params(fmt, fields, inp["params"], recs), inp["batch"], case.D)
    off = 0
    fo_cover = 0
    for f, spec in enumerate(fields):
        d = spec["dim"]
        if spec["name"] in recs:
            raw, fo = M.field(fmt, recs[spec["name"]], spec, inp["batch"][spec["name"]])
            assert raw.dtype == F32 and fo.dtype == F32 and raw.shape == (case.B, d)
            cols = slice(off, off + d)
            r = R.ratio(raw, ref["flat_embeddings"][:, cols], ref["A"]["flat_embeddings"][:, cols],
                        ref["n"]["flat_embeddings"][:, cols], R.C["forward"])
            assert r <= 1.0, f"{name} {spec['name']}: flat columns, worst |err| / bar = {r:.3f}"
            if d == case.D:
                r = R.ratio(raw, ref["field_embeddings"][:, f], ref["A"]["field_embeddings"][:, f],
                            ref["n"]["field_embeddings"][:, f], R.C["forward"])
                assert r <= 1.0, f"{name} {spec['name']}: field_embeddings, worst |err| / bar = {r:.3f}"
            # the field's first-order value against its own fp64 pooling
            w1 = M.REFS[fmt].dequantize_table(recs[spec["name"]])[1].astype(np.float64)
            x = inp["batch"][spec["name"]]
            if spec["type"] == "sparse":
                want, A, n = w1[x, 0], np.abs(w1[x, 0]), np.ones(case.B)
            else:
                want, A, n = H._rec_pool(w1, x, spec["combiner"], np.float64, "seq")
                want, A = want[:, 0], A[:, 0]
            r = R.ratio(fo, want, A, n, R.C["forward"])
            assert r <= 1.0, f"{name} {spec['name']}: first-order value, worst |err| / bar = {r:.3f}"
            fo_cover += 1
        off += d
    assert fo_cover == len(recs)


def _bag_setup(fmt, comb, L=6, V=20, d=16, seed=0):
    rng = np.random.default_rng(seed)
    spec = M.seq("h", V, d, L, comb)
    w2, w1 = rng.uniform(-1, 1, (V, d)).astype(F32), rng.uniform(-1, 1, (V, 1)).astype(F32)
    return spec, M.REFS[fmt].quantize_table(w2, w1)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("comb", ["mean", "sum", "max"])
def test_all_padding_bag_gives_exact_zeros(fmt, comb):
    spec, recs = _bag_setup(fmt, comb)
    ids = np.zeros((3, 6), np.int64)
    ids[1] = [0, 20, -1, 0, 0, 99]                       # out-of-range ids count as id 0
    raw, fo = M.field(fmt, recs, spec, ids)
    assert not raw.any() and not fo.any()
    assert not np.signbit(raw).any() and not np.signbit(fo).any()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("comb", ["sum", "max", "mean"])
def test_padding_may_stand_anywhere_in_a_bag(fmt, comb):
    """Moving the padding ids around, the other ids keeping their order, changes no bit."""
    spec, recs = _bag_setup(fmt, comb, seed=1)
    ids = np.array([[5, 7, 3, 0, 0, 0], [0, 5, 0, 7, 0, 3], [0, 0, 0, 5, 7, 3], [5, 0, 0, 7, 3, 0]], np.int64)
    raw, fo = M.field(fmt, recs, spec, ids)
    assert raw.any()
    for b in range(1, 4):
        assert np.array_equal(raw[b].view(np.uint32), raw[0].view(np.uint32)), b
        assert fo[b].view(np.uint32) == fo[0].view(np.uint32), b


def test_mean_divides_by_the_count_of_non_padding_ids():
    spec, recs = _bag_setup("int8", "mean", seed=2)
    w2, w1 = M.REFS["int8"].dequantize_table(recs)
    raw, fo = M.field("int8", recs, spec, np.array([[4, 0, 9, 0, 0, 4]], np.int64))
    s = ((w2[4] + w2[9]).astype(F32) + w2[4]).astype(F32)
    assert np.array_equal(raw[0], (s / F32(3)).astype(F32))
    assert fo[0] == F32(F32(F32(w1[4, 0] + w1[9, 0]) + w1[4, 0]) / F32(3))


def test_cases_cover_what_they_claim():
    ext = M.EXTRA_CASES
    assert {n for n in M.MATRIX} >= {"widths_D16", "widths_D64", "bags_D16", "max_D16", "wide_F64_D64", "batch_B4097_D16"}
    assert any(R.fwd_sb(R.CASES[n].F, R.CASES[n].D) == 1 for n in M.MATRIX), "a schema with F * D / 4 >= 512"
    Ls = {(f["max_len"], f["combiner"]) for f in ext["q_bags_D16"].fields if f["type"] == "sequence"}
    assert Ls == {(L, c) for L in (1, 2, 5, 50) for c in ("mean", "sum", "max")}
    proj = {(f["dim"], c.D) for c in ext.values() for f in c.fields if M.quantised(f) and f["dim"] != c.D}
    assert {(32, 16), (16, 32), (64, 16)} <= proj
    same = {c.D for c in ext.values() for f in c.fields if M.quantised(f) and f["dim"] == c.D}
    assert same == {16, 32, 64}
    sb = R.fwd_sb(6, 16)
    assert sorted(c.B for n, c in ext.items() if n.startswith("q_edge_B")) == [1, sb - 1, sb, sb + 1, 2 * sb + 1]
    for name in ("q_bags_D16", "q_proj_D16"):
        dims = {f["dim"] for f in ext[name].fields if f["type"] == "sparse"}
        assert {4, 8} <= dims and any(f["type"] == "dense" for f in ext[name].fields)
    ids = M.inputs("q_bags_D16")["batch"]["b5me"]
    assert ids[0, 1] == 0 and ids[0, 0] != 0 and ids[0, 2] != 0        # padding in the middle
    assert not ids[1].any() and (ids[2] != 0).sum() == 1 and ids[3].all() and len(set(ids[4])) == 1


# ----------------------------------------------------------------------------- the C entry point
def test_new_entry_point_is_declared_and_bound_and_the_abi_stays():
    from deepfm_amd import _lib
    import deepfm_amd.training as T
    text = open(os.path.join(ROOT, "include", "deepfm_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "dfm_embedding_forward_record_quant"
    assert name in set(re.findall(r"\b(dfm_[a-z0-9_]+)\s*\(", header)) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES[name][1]) == 14                   # 13 operands + the launch destination
    assert _lib.SIGNATURES[name][1][3:] == _lib.SIGNATURES["dfm_embedding_forward_record"][1][1:]
    assert lib.dfm_abi_version() == _lib.ABI_VERSION == 11
    assert re.search(r"#define DFM_ABI_VERSION 11\b", text)
    listed = re.search(r"Where a re-pointable launch goes\.(.*?)A NULL dfm_launch", text, re.S).group(1)
    assert name in listed
    for n in ("QuantizedMixedPredictor", "QuantizedMixedTables", "quantized_mixed_ineligible_reason"):
        assert hasattr(T, n), n


def test_entry_point_looks_at_the_launch_destination_first():
    from deepfm_amd import _lib
    lib = _lib.load()
    P = 0x1000
    rows = (ctypes.c_void_p * 2)(P, None)
    rc = lib.dfm_embedding_forward_record_quant(None, rows, 99, P, 8, P, None, P, 32, None, None, None, None,
                                                _lib.Launch(None, None, P))
    assert rc == 1 and "launch destination" in lib.dfm_last_error().decode()
    rc = lib.dfm_embedding_forward_record_quant(None, rows, _lib.QUANT_INT8_ROWWISE, P, 8, P, None, P, 32, None, None,
                                                None, None, None)
    assert rc == 1 and "null argument" in lib.dfm_last_error().decode()


# ----------------------------------------------------------------------------- eligibility
def _model(kind="deepfm", fields=None, **dnn):
    from deepfm_amd.models import create_model
    fields = fields or fields_of(load("model_deepfm_movielens"))
    return create_model(kind, schema_from_fields(fields), movielens_cfg(kind, **dnn))


def _narrow_only():
    return [M.sp("a", 9, 4), M.sp("b", 9, 8), M.seq("g", 9, 8, 3, "mean"), M.de("x", 4)]


@pytest.mark.parametrize("kind", ["deepfm", "xdeepfm", "attention_deepfm"])
def test_movielens_schema_is_eligible(kind):
    from deepfm_amd.training import quantized_mixed_ineligible_reason
    assert quantized_mixed_ineligible_reason(_model(kind)) is None


@pytest.mark.parametrize("dnn", [{"activation": "gelu"}, {"use_batch_norm": False}, {"hidden_units": [32, 18]}])
def test_refusals_of_the_fp32_predictor_come_back_verbatim(dnn):
    from deepfm_amd.training import QuantizedMixedPredictor, mixed_ineligible_reason, quantized_mixed_ineligible_reason
    model = _model(**dnn)
    reason = mixed_ineligible_reason(model)
    assert reason is not None and quantized_mixed_ineligible_reason(model) == reason
    with pytest.raises(ValueError, match=re.escape(reason)):          # on the CPU: before any device work
        QuantizedMixedPredictor(model, 64)


def test_record_gather_refusals_come_back_verbatim():
    import json
    from deepfm_amd.training import mixed_ineligible_reason, quantized_mixed_ineligible_reason
    fields = json.loads(json.dumps(fields_of(load("model_deepfm_movielens"))))
    for f in fields:
        if f["name"] == "genres":
            f["dim"] = 6
    model = _model(fields=fields)
    assert "not a multiple of 4" in mixed_ineligible_reason(model)
    assert quantized_mixed_ineligible_reason(model) == mixed_ineligible_reason(model)


def test_a_schema_of_narrow_fields_has_nothing_to_quantise():
    from deepfm_amd.models import create_model
    from deepfm_amd.training import (QuantizedMixedPredictor, mixed_ineligible_reason,
                                     quantized_mixed_ineligible_reason)
    cfg = movielens_cfg("deepfm")
    cfg.feature.fm_embed_dim = 8
    model = create_model("deepfm", schema_from_fields(_narrow_only()), cfg)
    assert mixed_ineligible_reason(model) is None
    want = ("no SPARSE or SEQUENCE field of width 16, 32 or 64: nothing to quantise (MixedSchemaPredictor serves this "
            "model)")
    assert quantized_mixed_ineligible_reason(model) == want
    with pytest.raises(ValueError, match=re.escape(want)):
        QuantizedMixedPredictor(model, 64)


# ----------------------------------------------------------------------------- the tables
_TFIELDS = [M.sp("u", 11, 16), M.seq("h", 13, 32, 4, "mean"), M.sp("n8", 9, 8), M.de("x", 16), M.sp("w", 7, 64),
            M.seq("n4", 6, 4, 2, "sum")]
_ROW = {"int8": {"u": 32, "h": 48, "w": 80}, "uint4": {"u": 16, "h": 24, "w": 40}}


def _trecords(fmt, seed=0, fields=_TFIELDS):
    rng = np.random.default_rng(seed)
    return {f["name"]: M.REFS[fmt].quantize_table(rng.uniform(-1, 1, (f["vocab"], f["dim"])).astype(F32),
                                                  rng.uniform(-1, 1, (f["vocab"], 1)).astype(F32))
            for f in fields if M.quantised(f)}


@pytest.mark.parametrize("fmt", FORMATS)
def test_tables_from_records_and_state_dict_round_trip(fmt):
    import torch
    from deepfm_amd.training import QuantizedMixedTables
    schema = schema_from_fields(_TFIELDS)
    recs = _trecords(fmt)
    tables = QuantizedMixedTables.from_records(schema, recs, fmt)
    assert tables.format == fmt and tables.dims == {"u": 16, "h": 32, "w": 64}
    assert tables.vocab == {"u": 11, "h": 13, "w": 7} and tables.fp32_fields == ["n8", "n4"]
    assert {n: tables.row_bytes(n) for n in recs} == _ROW[fmt]
    assert tables.nbytes == sum(tables.vocab[n] * _ROW[fmt][n] for n in recs)
    assert tables.fp32_nbytes == 11 * 68 + 13 * 132 + 7 * 260
    for n, r in recs.items():
        assert tables.records[n].dtype == torch.uint8 and np.array_equal(tables.records[n].numpy(), r)
    flat = QuantizedMixedTables.from_records(schema, {n: r.reshape(-1) for n, r in recs.items()}, fmt)
    assert all(torch.equal(flat.records[n], tables.records[n]) for n in recs)
    assert set(tables.error_bound()) == set(recs) and all(v > 0 for v in tables.error_bound().values())
    sd = tables.state_dict()
    assert sd["format"] == fmt and sd["dims"] == tables.dims and sd["vocab"] == tables.vocab
    other = QuantizedMixedTables.from_records(schema, _trecords(fmt, seed=1), fmt)
    ptrs = {n: t.data_ptr() for n, t in other.records.items()}
    other.load_state_dict(sd)
    assert all(torch.equal(other.records[n], tables.records[n]) for n in recs)
    assert ptrs == {n: t.data_ptr() for n, t in other.records.items()}
    sub = QuantizedMixedTables.from_records(schema, {"h": recs["h"]}, fmt, fields=["h"])
    assert list(sub.records) == ["h"] and sub.fp32_fields == ["u", "n8", "w", "n4"]
    with pytest.raises(ValueError, match="no model"):
        tables.refresh()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tables.dequantized()


def test_tables_name_their_mismatches():
    from deepfm_amd.training import QuantizedMixedTables
    import types
    schema = schema_from_fields(_TFIELDS)
    recs = _trecords("int8")
    make = QuantizedMixedTables.from_records
    with pytest.raises(ValueError, match="'h'"):                                   # a missing field
        make(schema, {n: r for n, r in recs.items() if n != "h"})
    with pytest.raises(ValueError, match="'zz'"):                                  # an extra field
        make(schema, dict(recs, zz=recs["u"]))
    with pytest.raises(ValueError, match="'n8'"):                                  # records for a narrow field
        make(schema, dict(recs, n8=recs["u"]))
    with pytest.raises(ValueError, match="'w'.*7 x 80"):                           # a wrong byte count
        make(schema, dict(recs, w=recs["w"][:-1]))
    with pytest.raises(ValueError, match="'u'"):
        make(schema, dict(recs, u=recs["u"].astype(np.int8)))
    with pytest.raises(ValueError, match="'u'.*11 x 16"):                          # int8 records read as uint4
        make(schema, recs, "uint4")
    with pytest.raises(ValueError, match="int4"):                                  # a wrong format
        make(schema, recs, "int4")
    with pytest.raises(ValueError, match="'x'.*DENSE"):
        make(schema, recs, fields=["u", "x"])
    with pytest.raises(ValueError, match="'n8'.*width 8"):
        make(schema, recs, fields=["n8"])
    tables = make(schema, recs)
    sd = tables.state_dict()
    with pytest.raises(ValueError, match="format"):
        tables.load_state_dict(dict(sd, format="uint4"))
    with pytest.raises(ValueError, match="'h'.*width 16"):                         # a wrong width per field
        tables.load_state_dict(dict(sd, dims=dict(sd["dims"], h=16)))
    with pytest.raises(ValueError, match="'u'"):
        tables.load_state_dict(dict(sd, vocab=dict(sd["vocab"], u=99)))
    with pytest.raises(ValueError, match="'w'"):
        tables.load_state_dict(dict(sd, records={n: r for n, r in sd["records"].items() if n != "w"}))
    with pytest.raises(ValueError, match="'zz'"):
        tables.load_state_dict(dict(sd, records=dict(sd["records"], zz=sd["records"]["u"])))
    with pytest.raises(ValueError, match="'h'.*13 x 48"):
        tables.load_state_dict(dict(sd, records=dict(sd["records"], h=sd["records"]["h"][:-1])))

    def shim(fields):
        return types.SimpleNamespace(schema=schema_from_fields(fields))
    assert tables.matches(shim(_TFIELDS)) is None
    assert "'h'" in tables.matches(shim([f for f in _TFIELDS if f["name"] != "h"]))                # missing in the model
    assert "'u'" in tables.matches(shim([dict(f, vocab=12) if f["name"] == "u" else f for f in _TFIELDS]))
    wider = tables.matches(shim([dict(f, dim=64) if f["name"] == "h" else f for f in _TFIELDS]))
    assert "'h'" in wider and "width 32" in wider and "width 64" in wider
    assert "DENSE" in tables.matches(shim([M.de("u", 16) if f["name"] == "u" else f for f in _TFIELDS]))
    # a subset serves the model too: the fields without records stay fp32
    assert make(schema, {"u": recs["u"]}, fields=["u"]).matches(shim(_TFIELDS)) is None


def test_from_model_refuses_dense_and_narrow_fields_by_name():
    from deepfm_amd.training import QuantizedMixedPredictor, QuantizedMixedTables
    model = _model()                       # MovieLens, on the CPU: the refusals come before any device work
    with pytest.raises(ValueError, match="'dow_sin'.*DENSE"):
        QuantizedMixedTables.from_model(model, fields=["dow_sin"])
    with pytest.raises(ValueError, match="'genres'.*width 8"):
        QuantizedMixedTables.from_model(model, fields=["user_id", "genres"])
    with pytest.raises(ValueError, match="'nobody'"):
        QuantizedMixedTables.from_model(model, fields=["nobody"])
    with pytest.raises(ValueError, match="int4"):
        QuantizedMixedTables.from_model(model, fmt="int4")
    with pytest.raises(ValueError, match="'genres'.*width 8"):
        QuantizedMixedPredictor(model, 64, fields=["genres"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # an eligible request reaches the device check
        QuantizedMixedTables.from_model(model)
