"""CPU: the row-wise int8 record format by its numpy float32 restatement (tests/quant_reference.py): the error bound
on four row families, exact constant rows, the record layout; the eligibility reasons of ``QuantizedPredictor``;
``QuantizedTables`` from records and through its state dict; the new entry points."""
import os
import re

import numpy as np
import pytest

from tests import quant_reference as Q
from tests.helpers import schema_from_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dfm_quant_row_bytes", "dfm_quantize_rows", "dfm_dequantize_rows", "dfm_embedding_forward_quant"]
WIDTHS = [16, 32, 64]


def _family(name, rows, D, rng):
    if name == "normal":
        return rng.standard_normal((rows, D)).astype(np.float32)
    if name == "scaled":            # whole rows scaled by 10^-6 .. 10^6
        return (rng.standard_normal((rows, D)) * 10.0 ** rng.uniform(-6, 6, (rows, 1))).astype(np.float32)
    if name == "offset":            # +-100 with a spread of 1e-3: one-signed rows, a range far below the magnitude
        sign = np.where(rng.random((rows, 1)) < 0.5, -1.0, 1.0)
        return (sign * 100.0 + 1e-3 * rng.standard_normal((rows, D))).astype(np.float32)
    assert name == "loguniform"     # magnitudes 1e-3 .. 1e3 inside one row, mixed sign
    sign = np.where(rng.random((rows, D)) < 0.5, -1.0, 1.0)
    return (sign * 10.0 ** rng.uniform(-3, 3, (rows, D))).astype(np.float32)


@pytest.mark.parametrize("family", ["normal", "scaled", "offset", "loguniform"])
@pytest.mark.parametrize("D", WIDTHS)
def test_error_bound_of_the_restatement(family, D):
    """|x' - x| <= scale / 2 + 2^-21 max(|lo|, |hi|) for every element; the clamp keeps q within a byte."""
    rng = np.random.default_rng([D, len(family)])
    x = _family(family, 20000, D, rng)
    scale, lo, q = Q.quantize(x)
    xd = Q.dequantize(scale, lo, q)
    err = np.abs(xd.astype(np.float64) - x.astype(np.float64))
    bound = Q.bound(x)[:, None]
    worst = float((err / bound).max())
    print(f"{family} D={D}: worst |err| / bound = {worst:.4f}")
    assert (err <= bound).all(), worst
    # the extremes of every row are hit: lo exactly, hi within the bound, and both ends of the byte range are used
    assert (q.min(axis=1) == 0).all() and (q.max(axis=1) == 255).all()
    assert np.array_equal(xd.min(axis=1), lo)


@pytest.mark.parametrize("D", WIDTHS)
def test_constant_rows_and_the_zero_row_are_exact(D):
    x = np.zeros((5, D), np.float32)
    x[1] = 3.25
    x[2] = -1e-30
    x[3] = 1e30
    x[4] = np.float32(0.1)
    scale, lo, q = Q.quantize(x)
    assert not scale.any() and not q.any()
    xd = Q.dequantize(scale, lo, q)
    assert np.array_equal(xd.view(np.uint32), x.view(np.uint32))
    assert not xd[0].any()


@pytest.mark.parametrize("D", WIDTHS)
def test_record_layout_round_trips(D):
    from deepfm_amd import _lib
    from deepfm_amd.training import quantized
    lib = _lib.load()
    assert Q.row_bytes(D) == 16 + D == lib.dfm_quant_row_bytes(D, _lib.QUANT_INT8_ROWWISE) == quantized.row_bytes(D)
    rng = np.random.default_rng(D)
    w2 = rng.standard_normal((37, D)).astype(np.float32)
    w1 = rng.standard_normal((37, 1)).astype(np.float32)
    rec = Q.quantize_table(w2, w1)
    assert rec.shape == (37, 16 + D) and rec.dtype == np.uint8
    scale, lo, w1b, pad, q = Q.unpack(rec)
    s0, l0, q0 = Q.quantize(w2)
    assert np.array_equal(scale, s0) and np.array_equal(lo, l0) and np.array_equal(q, q0)
    assert np.array_equal(w1b, w1[:, 0]) and not pad.view(np.uint32).any()
    assert np.array_equal(rec[:, 12:16], np.zeros((37, 4), np.uint8))
    assert np.array_equal(rec[:, :4].copy().view(np.float32)[:, 0], s0)           # bytes 0-3: scale
    assert np.array_equal(rec[:, 8:12].copy().view(np.float32)[:, 0], w1[:, 0])   # bytes 8-11: w1
    w2d, w1d = Q.dequantize_table(rec)
    assert np.array_equal(w2d, Q.dequantize(s0, l0, q0)) and np.array_equal(w1d, w1)


def test_row_bytes_of_unsupported_widths_and_formats_is_zero():
    from deepfm_amd import _lib
    from deepfm_amd.training import quantized
    lib = _lib.load()
    for D in (0, 4, 8, 12, 24, 48, 128, 256):
        assert lib.dfm_quant_row_bytes(D, _lib.QUANT_INT8_ROWWISE) == 0
        with pytest.raises(ValueError, match="16, 32 and 64"):
            quantized.row_bytes(D)
    for fmt in (0, 2, -1):
        assert lib.dfm_quant_row_bytes(16, fmt) == 0
    with pytest.raises(ValueError, match="int4"):
        quantized.row_bytes(16, "int4")


# ---------------------------------------------------------------------------------------------- eligibility
def _fields(ns, nd, D):
    fields = [dict(name=f"s{i}", type="sparse", vocab=5 + i, dim=D, max_len=1, combiner="mean") for i in range(ns)]
    return fields + [dict(name=f"d{i}", type="dense", vocab=0, dim=D, max_len=1, combiner="mean") for i in range(nd)]


def _model(fields, D, kind="deepfm", **dnn):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = D
    cfg.dnn.hidden_units = [32, 32]
    for k, v in dnn.items():
        setattr(cfg.dnn, k, v)
    return create_model(kind, schema_from_fields(fields), cfg)


def test_quantized_ineligible_reasons():
    from deepfm_amd.training import QuantizedPredictor, ineligible_reason, quantized_ineligible_reason
    for D in WIDTHS:
        assert quantized_ineligible_reason(_model(_fields(3, 2, D), D)) is None
    for D in (8, 128):
        model = _model(_fields(3, 2, D), D)
        assert ineligible_reason(model) is None            # the fp32 predictor takes it
        reason = quantized_ineligible_reason(model)
        assert f"fm_embed_dim {D}" in reason and "16, 32 and 64" in reason
        with pytest.raises(ValueError, match="16, 32 and 64"):
            QuantizedPredictor(model, 64)                  # on the CPU: refused before any device work
    # past the gather's slot caps
    assert "at most 48 SPARSE" in quantized_ineligible_reason(_model(_fields(49, 1, 16), 16))
    # an fp32-ineligible model keeps the fp32 reason, word for word
    for model in (_model(_fields(3, 2, 16), 16, activation="gelu"),
                  _model(_fields(3, 2, 16), 16, hidden_units=[32, 18]),
                  _model(_fields(2, 1, 16)[:2] + _fields(0, 1, 8), 16)):
        want = ineligible_reason(model)
        assert want is not None and quantized_ineligible_reason(model) == want
        with pytest.raises(ValueError, match=re.escape(want)):
            QuantizedPredictor(model, 64)


# ---------------------------------------------------------------------------------------------- tables on the host
def _records(fields, D, rng):
    out = {}
    for f in fields:
        if f["type"] == "sparse":
            w2 = rng.standard_normal((f["vocab"], D)).astype(np.float32)
            w2[0] = 0
            out[f["name"]] = Q.quantize_table(w2, rng.standard_normal(f["vocab"]).astype(np.float32))
    return out


def test_tables_from_records_and_state_dict_round_trip():
    import torch
    from deepfm_amd.training import QuantizedTables
    D = 32
    fields = _fields(3, 2, D)
    schema = schema_from_fields(fields)
    rng = np.random.default_rng(0)
    recs = _records(fields, D, rng)
    tables = QuantizedTables.from_records(schema, D, recs)
    assert tables.row_bytes == 48 and tables.vocab == {"s0": 5, "s1": 6, "s2": 7}
    assert tables.nbytes == 18 * 48 and tables.fp32_nbytes == 18 * (4 * D + 4)
    for name, r in recs.items():
        assert tables.records[name].dtype == torch.uint8 and np.array_equal(tables.records[name].numpy(), r)
    # flat byte strings are taken as well
    flat = QuantizedTables.from_records(schema, D, {n: r.reshape(-1) for n, r in recs.items()})
    assert all(torch.equal(flat.records[n], tables.records[n]) for n in recs)
    # error_bound() is the restatement's bound, maximised over the rows
    got = tables.error_bound()
    for name, r in recs.items():
        scale, lo, _, _, q = Q.unpack(r)
        hi = lo.astype(np.float64) + 255.0 * scale.astype(np.float64)
        want = (scale.astype(np.float64) / 2 + 2.0 ** -21 * np.maximum(np.abs(lo), np.abs(hi))).max()
        assert got[name] == pytest.approx(want, rel=1e-12)
    # state dict: uint8 tensors plus format, width and vocabularies; loading copies into the same buffers
    sd = tables.state_dict()
    assert sd["format"] == "int8" and sd["dim"] == D and sd["vocab"] == tables.vocab
    assert all(t.dtype == torch.uint8 for t in sd["records"].values())
    other = QuantizedTables.from_records(schema, D, _records(fields, D, np.random.default_rng(1)))
    ptrs = {n: t.data_ptr() for n, t in other.records.items()}
    other.load_state_dict(sd)
    assert all(torch.equal(other.records[n], tables.records[n]) for n in recs)
    assert ptrs == {n: t.data_ptr() for n, t in other.records.items()}
    with pytest.raises(ValueError, match="no model"):
        tables.refresh()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tables.dequantized()


def test_tables_name_their_mismatches():
    from deepfm_amd.training import QuantizedTables
    D = 16
    fields = _fields(3, 1, D)
    schema = schema_from_fields(fields)
    recs = _records(fields, D, np.random.default_rng(2))
    with pytest.raises(ValueError, match="'s1'"):
        QuantizedTables.from_records(schema, D, {n: r for n, r in recs.items() if n != "s1"})
    with pytest.raises(ValueError, match="'zz'"):
        QuantizedTables.from_records(schema, D, dict(recs, zz=recs["s0"]))
    with pytest.raises(ValueError, match="'s2'"):
        QuantizedTables.from_records(schema, D, dict(recs, s2=recs["s2"][:-1]))
    with pytest.raises(ValueError, match="'s0'"):
        QuantizedTables.from_records(schema, D, dict(recs, s0=recs["s0"].astype(np.int8)))
    with pytest.raises(ValueError, match="16, 32 and 64"):
        QuantizedTables.from_records(schema_from_fields(_fields(1, 0, 8)), 8, {})
    with pytest.raises(ValueError, match="'s0'"):                  # the schema's width is not the tables'
        QuantizedTables.from_records(schema, 32, recs)
    tables = QuantizedTables.from_records(schema, D, recs)
    sd = tables.state_dict()
    with pytest.raises(ValueError, match="format"):
        tables.load_state_dict(dict(sd, format="int4"))
    with pytest.raises(ValueError, match="width 32"):
        tables.load_state_dict(dict(sd, dim=32))
    with pytest.raises(ValueError, match="'s1'"):
        tables.load_state_dict(dict(sd, vocab=dict(sd["vocab"], s1=99)))
    with pytest.raises(ValueError, match="'s2'"):
        tables.load_state_dict(dict(sd, records={n: r for n, r in sd["records"].items() if n != "s2"}))
    # a bigger vocabulary in the schema than in the stored tables
    bigger = [dict(f, vocab=f["vocab"] + 1) if f["name"] == "s1" else f for f in fields]
    other = QuantizedTables.from_records(schema_from_fields(bigger), D, _records(bigger, D, np.random.default_rng(3)))
    with pytest.raises(ValueError, match="'s1'"):
        other.load_state_dict(sd)
    # tables of another schema do not serve a model
    assert "'s1'" in other.matches(_model(fields, D))
    assert tables.matches(_model(fields, D)) is None


def test_new_entry_points_are_declared_exported_and_bound():
    from deepfm_amd import _lib
    import deepfm_amd.training as T
    import ctypes
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepfm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dfm_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES["dfm_embedding_forward_quant"][1]) == 14      # 13 operands + the launch destination
    assert ctypes.sizeof(_lib.QuantField) == 48 and _lib.QuantField.rows.offset == 8
    for name in ("QuantizedPredictor", "QuantizedTables", "quantized_ineligible_reason"):
        assert hasattr(T, name), name


def test_gather_refuses_on_the_host():
    """Host-side refusals of dfm_embedding_forward_quant, before anything is dereferenced or launched: the launch
    destination first, then the width, the format and the slot caps (DFM_ERR_UNSUPPORTED with the reason)."""
    import ctypes
    from deepfm_amd import _lib
    lib = _lib.load()
    P = 0x1000

    def call(ns, nd, D, fmt=_lib.QUANT_INT8_ROWWISE, at=None):
        arr = (_lib.QuantField * (ns + nd))()
        for i in range(ns + nd):
            arr[i].kind, arr[i].vocab, arr[i].rows = (_lib.SPARSE, 4, P) if i < ns else (_lib.DENSE, 0, None)
            if i >= ns:
                arr[i].w2 = arr[i].b2 = arr[i].w1 = arr[i].b1 = P
        inputs = (ctypes.c_void_p * (ns + nd))(*([P] * (ns + nd)))
        return lib.dfm_embedding_forward_quant(arr, ns + nd, D, fmt, inputs, None, None, 8, P, P, None, None, None, at)

    assert call(49, 1, 16) == _lib.ERR_UNSUPPORTED
    assert "at most 48 SPARSE and 32 DENSE" in lib.dfm_last_error().decode()
    assert call(5, 33, 16) == _lib.ERR_UNSUPPORTED
    assert call(3, 2, 8) == _lib.ERR_UNSUPPORTED and "16, 32 and 64" in lib.dfm_last_error().decode()
    assert call(3, 2, 16, fmt=2) == _lib.ERR_UNSUPPORTED and "DFM_QUANT_INT8_ROWWISE" in lib.dfm_last_error().decode()
    assert call(3, 2, 8, at=_lib.Launch(None, None, P)) == 1           # DFM_ERR_INVALID: looked at first
    assert "launch destination" in lib.dfm_last_error().decode()
    assert lib.dfm_quantize_rows(P, 8, P, 1, 4, 8, _lib.QUANT_INT8_ROWWISE, P, P, None) == _lib.ERR_UNSUPPORTED
    assert lib.dfm_dequantize_rows(P, 4, 16, 0, P, P, None) == _lib.ERR_UNSUPPORTED
