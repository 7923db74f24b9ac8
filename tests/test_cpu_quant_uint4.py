"""CPU: the row-wise 4-bit record format by its numpy restatement (tests/quant4_reference.py): the error bound in fp64
over widths, magnitudes and row families, monotone codes, the directed header roundings, the exact zero row, refused
rows, the record layout; the host side of the three entry points with format 4; ``QuantizedTables`` in ``"uint4"``
from records and through its state dict."""
import functools

import numpy as np
import pytest

from tests import quant4_reference as Q4
from tests import quant_reference as Q8
from tests.helpers import schema_from_fields

WIDTHS = [16, 32, 64]
MAGNITUDES = [1e-4, 1e-2, 1.0, 100.0, 3e4]
FAMILIES = ["uniform", "offset", "constant", "zero", "tiny_range", "outlier"]
ROWS = 4000


def _family(name, rows, D, mag, rng):
    """``rows`` finite rows of width D around the magnitude ``mag``."""
    if name == "uniform":
        x = rng.uniform(-mag, mag, (rows, D))
    elif name == "offset":           # one-signed rows: a range far below the magnitude
        sign = np.where(rng.random((rows, 1)) < 0.5, -1.0, 1.0)
        x = sign * mag + 0.01 * mag * rng.standard_normal((rows, D))
    elif name == "constant":         # one value per row, which binary16 cannot represent
        x = np.repeat(mag * (1.0 + rng.random((rows, 1))) * (1 + 2.0 ** -13), D, axis=1)
        x *= np.where(rng.random((rows, 1)) < 0.5, -1.0, 1.0)
    elif name == "zero":
        x = np.zeros((rows, D))
    elif name == "tiny_range":       # a range of 1e-9 around +-mag (and around 0 in every fourth row)
        base = mag * rng.uniform(-1, 1, (rows, 1))
        base[::4] = 0.0
        x = base + 1e-9 * rng.random((rows, D))
    else:
        assert name == "outlier"     # small values and one element 100 times as large
        x = 0.01 * mag * rng.standard_normal((rows, D))
        x[np.arange(rows), rng.integers(0, D, rows)] = mag * np.where(rng.random(rows) < 0.5, -1.0, 1.0)
    x = x.astype(np.float32)
    if name == "constant":
        x = np.where(x.astype(np.float16).astype(np.float32) == x, np.nextafter(x, np.float32(np.inf)), x)
        assert (x.astype(np.float16).astype(np.float32) != x).all() and (x == x[:, :1]).all()
    return x


@functools.lru_cache(maxsize=None)
def _cases(family, D):
    """[(magnitude, x, scale_h, lo_h, q)] of one family and width, quantised once and left unchanged."""
    out = []
    for mag in MAGNITUDES:
        rng = np.random.default_rng([D, len(family), int(np.log10(mag) * 10) + 100])
        x = _family(family, ROWS, D, mag, rng)
        scale_h, lo_h, q, bad = Q4.quantize(x)
        assert not bad.any(), (family, mag)
        out.append((mag, x, scale_h, lo_h, q))
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", WIDTHS)
def test_error_bound_and_order_of_the_restatement(family, D):
    """For every finite row: |x' - x| <= scale / 2 + 2^-21 max(|lo|, |lo + 15 scale|) in fp64; x - lo >= 0 and
    (x - lo) / scale <= 15 as the quantiser forms them in float32, before the clamp; codes monotone in x."""
    worst = 0.0
    for mag, x, scale_h, lo_h, q in _cases(family, D):
        xd = Q4.dequantize(scale_h, lo_h, q)
        x64, scale, lo = x.astype(np.float64), scale_h.astype(np.float64), lo_h.astype(np.float64)
        err = np.abs(xd.astype(np.float64) - x64)
        bound = Q4.bound(x)
        assert np.array_equal(bound, scale / 2 + 2.0 ** -21 * np.maximum(np.abs(lo), np.abs(lo + 15 * scale)))
        worst = max(worst, float((err / np.maximum(bound[:, None], 1e-300)).max()))
        assert (err <= bound[:, None]).all(), (family, mag, worst)
        assert q.max() <= 15
        live = scale_h > 0
        t = ((x - lo_h.astype(np.float32)[:, None]).astype(np.float32)[live]
             / scale_h.astype(np.float32)[live, None]).astype(np.float32)
        assert t.size == 0 or (t.min() >= 0 and t.max() <= 15.0)
        # monotone: sorting a row by value sorts its codes
        order = np.argsort(x, axis=1, kind="stable")
        assert (np.diff(np.take_along_axis(q.astype(np.int32), order, axis=1), axis=1) >= 0).all()
        if family == "zero":
            assert not scale_h.any() and not lo_h.view(np.uint16).any() and not q.any()
            assert not xd.view(np.uint32).any()
        if family == "tiny_range":
            assert (scale_h[::4] == np.float16(2.0 ** -24)).all() and not q[::4].any()
    print(f"{family} D={D}: worst |err| / bound = {worst:.5f}")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", WIDTHS)
def test_header_spans_the_row(family, D):
    """lo <= min(x) and lo + 15 scale >= max(x), exactly (fp64), for every row: the two directed roundings of the
    header and, for the rows where the float32 subtract and divide both rounded down onto a binary16 value (1 row in
    20 000 of the uniform families here), the quantiser's extra step of the scale."""
    short, deficit = 0, 0.0
    for mag, x, scale_h, lo_h, q in _cases(family, D):
        x64, scale, lo = x.astype(np.float64), scale_h.astype(np.float64), lo_h.astype(np.float64)
        assert (lo <= x64.min(axis=1)).all(), (family, mag)
        hi, top = x64.max(axis=1), lo + 15 * scale
        short += int((top < hi).sum())
        deficit = max(deficit, float(((hi - top) / np.maximum(hi - lo, 1e-300)).max()))
    print(f"{family} D={D}: {short} rows of {len(MAGNITUDES) * ROWS} with lo + 15 scale < max, "
          f"largest (max - lo - 15 scale) / (max - lo) = {deficit:.3e}")
    assert short == 0, (short, deficit)


def test_directed_roundings_of_the_header():
    f16, f32 = np.float16, np.float32
    v = np.array([0.1, -0.1, 1.0, -1.0, -1e-9, 1e-9, 0.0, -0.0, 65504.0, 65519.0, 1e6, -65504.0, -65505.0, -1e6,
                  2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 6.1e-5, -6.1e-5], f32)
    lo, up = Q4.half_floor(v), Q4.half_ceil(v)
    with np.errstate(over="ignore"):            # the neighbour of +-65504 is infinite
        above, below = np.nextafter(lo, f16(np.inf)).astype(f32), np.nextafter(up, f16(-np.inf)).astype(f32)
    fin = np.isfinite(lo)
    assert (lo[fin].astype(f32) <= v[fin]).all() and (above[fin] > v[fin]).all()
    fin = np.isfinite(up)
    assert (up[fin].astype(f32) >= v[fin]).all() and (below[fin] < v[fin]).all()
    assert lo[4] == f16(-(2.0 ** -24)) and lo[4].view(np.uint16) == 0x8001       # the -0 step
    assert up[5] == f16(2.0 ** -24) and up[5].view(np.uint16) == 0x0001          # the 0 step
    assert lo[6].view(np.uint16) == 0 and up[6].view(np.uint16) == 0             # exact values stay
    assert lo[8] == up[8] == f16(65504.0) and lo[9] == lo[10] == f16(65504.0)
    assert np.isposinf(up[9]) and np.isposinf(up[10])
    assert lo[11] == f16(-65504.0) and np.isneginf(lo[12]) and np.isneginf(lo[13])


@pytest.mark.parametrize("D", WIDTHS)
def test_rows_beyond_binary16_are_reported_bad(D):
    rng = np.random.default_rng(D)
    x = rng.uniform(-1, 1, (8, D)).astype(np.float32)
    x[1] += np.float32(1.5e6)            # offset rows: lo is held at 65504, the scale to reach the row is not
    x[2] -= np.float32(1.5e6)            # lo below -65504
    x[3, 3] = np.float32(-65505.0)
    x[4, 0], x[4, 1] = 0.0, np.float32(15 * 65504.0 * 1.001)     # scale beyond 65504
    x[5, D - 1] = np.nan
    x[6, 0] = np.inf
    x[7, 5] = np.float32(-65504.0)       # exactly the smallest binary16: fine
    bad = Q4.quantize(x)[3]
    assert bad.tolist() == [False, True, True, True, True, True, True, False]


@pytest.mark.parametrize("D", WIDTHS)
def test_record_layout_round_trips(D):
    from deepfm_amd import _lib
    from deepfm_amd.training import quantized
    lib = _lib.load()
    assert Q4.row_bytes(D) == 8 + D // 2 == lib.dfm_quant_row_bytes(D, 4) == quantized.row_bytes(D, "uint4")
    assert _lib.QUANT_UINT4_ROWWISE == 4 == quantized.FORMATS["uint4"] and quantized.HEADER_BYTES == 16
    rng = np.random.default_rng(D)
    w2 = rng.standard_normal((37, D)).astype(np.float32)
    w1 = rng.standard_normal((37, 1)).astype(np.float32)
    rec = Q4.quantize_table(w2, w1)
    assert rec.shape == (37, 8 + D // 2) and rec.dtype == np.uint8
    scale, lo, w1b, q = Q4.unpack(rec)
    s0, l0, q0, _ = Q4.quantize(w2)
    assert np.array_equal(scale, s0) and np.array_equal(lo, l0) and np.array_equal(q, q0)
    assert np.array_equal(w1b, w1[:, 0])
    assert np.array_equal(rec[:, 0:2].copy().view(np.float16)[:, 0], s0)          # bytes 0-1: scale
    assert np.array_equal(rec[:, 2:4].copy().view(np.float16)[:, 0], l0)          # bytes 2-3: lo
    assert np.array_equal(rec[:, 4:8].copy().view(np.float32)[:, 0], w1[:, 0])    # bytes 4-7: w1
    # the low nibble holds the even element
    assert np.array_equal(rec[:, 8] & 15, q0[:, 0]) and np.array_equal(rec[:, 8] >> 4, q0[:, 1])
    assert np.array_equal(rec[:, -1] & 15, q0[:, D - 2]) and np.array_equal(rec[:, -1] >> 4, q0[:, D - 1])
    one = Q4.pack(s0[:1], l0[:1], w1[:1], np.arange(D, dtype=np.uint8)[None, :] % 16)
    assert one[0, 8:12].tolist() == [0x10, 0x32, 0x54, 0x76]
    w2d, w1d = Q4.dequantize_table(rec)
    assert np.array_equal(w2d, Q4.dequantize(s0, l0, q0)) and np.array_equal(w1d, w1)


def test_row_bytes_of_unsupported_widths_is_zero():
    from deepfm_amd import _lib
    from deepfm_amd.training import quantized
    lib = _lib.load()
    for D in (0, 4, 8, 12, 24, 48, 128, 256):
        assert lib.dfm_quant_row_bytes(D, 4) == 0
        with pytest.raises(ValueError, match="16, 32 and 64"):
            quantized.row_bytes(D, "uint4")
    for fmt in (0, 2, 3, 5, 8, -1):
        assert lib.dfm_quant_row_bytes(16, fmt) == 0


def test_entry_points_refuse_an_unsupported_width_on_the_host():
    """With format 4, before anything is dereferenced or launched (the pointers here are not memory)."""
    import ctypes
    from deepfm_amd import _lib
    lib = _lib.load()
    P = 0x1000
    for D in (8, 24, 128):
        assert lib.dfm_quantize_rows(P, D, P, 1, 4, D, 4, P, P, None) == _lib.ERR_UNSUPPORTED
        assert "16, 32 and 64" in lib.dfm_last_error().decode()
        assert lib.dfm_dequantize_rows(P, 4, D, 4, P, P, None) == _lib.ERR_UNSUPPORTED
        assert "16, 32 and 64" in lib.dfm_last_error().decode()
        arr = (_lib.QuantField * 2)()
        arr[0].kind, arr[0].vocab, arr[0].rows = _lib.SPARSE, 4, P
        arr[1].kind = _lib.DENSE
        arr[1].w2 = arr[1].b2 = arr[1].w1 = arr[1].b1 = P
        inputs = (ctypes.c_void_p * 2)(P, P)
        assert lib.dfm_embedding_forward_quant(arr, 2, D, 4, inputs, None, None, 8, P, P, None, None, None,
                                               None) == _lib.ERR_UNSUPPORTED
        assert "16, 32 and 64" in lib.dfm_last_error().decode()
    # an unknown format is refused naming both supported ones
    assert lib.dfm_dequantize_rows(P, 4, 16, 3, P, P, None) == _lib.ERR_UNSUPPORTED
    msg = lib.dfm_last_error().decode()
    assert "DFM_QUANT_INT8_ROWWISE" in msg and "DFM_QUANT_UINT4_ROWWISE" in msg


# ---------------------------------------------------------------------------------------------- tables on the host
def _fields(ns, nd, D):
    fields = [dict(name=f"s{i}", type="sparse", vocab=5 + i, dim=D, max_len=1, combiner="mean") for i in range(ns)]
    return fields + [dict(name=f"d{i}", type="dense", vocab=0, dim=D, max_len=1, combiner="mean") for i in range(nd)]


def _records(fields, D, rng, Q=Q4):
    out = {}
    for f in fields:
        if f["type"] == "sparse":
            w2 = rng.standard_normal((f["vocab"], D)).astype(np.float32)
            w2[0] = 0
            out[f["name"]] = Q.quantize_table(w2, rng.standard_normal(f["vocab"]).astype(np.float32))
    return out


@pytest.mark.parametrize("D", WIDTHS)
def test_tables_from_records_and_state_dict_round_trip(D):
    import torch
    from deepfm_amd.training import QuantizedTables
    fields = _fields(3, 2, D)
    schema = schema_from_fields(fields)
    recs = _records(fields, D, np.random.default_rng(D))
    rb = 8 + D // 2
    tables = QuantizedTables.from_records(schema, D, recs, fmt="uint4")
    assert tables.format == "uint4" and tables.row_bytes == rb and tables.vocab == {"s0": 5, "s1": 6, "s2": 7}
    assert tables.nbytes == 18 * rb and tables.fp32_nbytes == 18 * (4 * D + 4)
    for name, r in recs.items():
        assert tables.records[name].dtype == torch.uint8 and np.array_equal(tables.records[name].numpy(), r)
    flat = QuantizedTables.from_records(schema, D, {n: r.reshape(-1) for n, r in recs.items()}, fmt="uint4")
    assert all(torch.equal(flat.records[n], tables.records[n]) for n in recs)
    # error_bound() is the restatement's bound, maximised over the rows
    got = tables.error_bound()
    for name, r in recs.items():
        w2d, _ = Q4.dequantize_table(r)
        scale, lo, _, _ = Q4.unpack(r)
        scale, lo = scale.astype(np.float64), lo.astype(np.float64)
        want = (scale / 2 + 2.0 ** -21 * np.maximum(np.abs(lo), np.abs(lo + 15 * scale))).max()
        assert got[name] == pytest.approx(want, rel=1e-12) and want > 0
    w2 = np.random.default_rng(1).standard_normal((9, D)).astype(np.float32)
    one = QuantizedTables.from_records(schema_from_fields([dict(_fields(1, 0, D)[0], vocab=9)]), D,
                                       {"s0": Q4.quantize_table(w2, np.zeros(9, np.float32))}, fmt="uint4")
    assert one.error_bound()["s0"] == pytest.approx(float(Q4.bound(w2).max()), rel=1e-12)
    # state dict: uint8 tensors plus format, width and vocabularies; loading copies into the same buffers
    sd = tables.state_dict()
    assert sd["format"] == "uint4" and sd["dim"] == D and sd["vocab"] == tables.vocab
    assert all(t.dtype == torch.uint8 for t in sd["records"].values())
    other = QuantizedTables.from_records(schema, D, _records(fields, D, np.random.default_rng(1)), fmt="uint4")
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
    with pytest.raises(ValueError, match="'s1'"):                  # a missing field
        QuantizedTables.from_records(schema, D, {n: r for n, r in recs.items() if n != "s1"}, fmt="uint4")
    with pytest.raises(ValueError, match="'s2'"):                  # a wrong byte count
        QuantizedTables.from_records(schema, D, dict(recs, s2=recs["s2"][:-1]), fmt="uint4")
    recs8 = _records(fields, D, np.random.default_rng(2), Q8)
    with pytest.raises(ValueError, match="'s0'"):                  # int8 records are not uint4 records, and back
        QuantizedTables.from_records(schema, D, recs8, fmt="uint4")
    with pytest.raises(ValueError, match="'s0'"):
        QuantizedTables.from_records(schema, D, recs)
    with pytest.raises(ValueError, match="16, 32 and 64"):
        QuantizedTables.from_records(schema_from_fields(_fields(1, 0, 8)), 8, {}, fmt="uint4")
    t4 = QuantizedTables.from_records(schema, D, recs, fmt="uint4")
    t8 = QuantizedTables.from_records(schema, D, recs8)
    with pytest.raises(ValueError, match="format"):
        t4.load_state_dict(t8.state_dict())
    with pytest.raises(ValueError, match="format"):
        t8.load_state_dict(t4.state_dict())
    sd = t4.state_dict()
    with pytest.raises(ValueError, match="width 32"):
        t4.load_state_dict(dict(sd, dim=32))
    with pytest.raises(ValueError, match="'s2'"):
        t4.load_state_dict(dict(sd, records={n: r for n, r in sd["records"].items() if n != "s2"}))
    with pytest.raises(ValueError, match="'s1'"):
        t4.load_state_dict(dict(sd, records=dict(sd["records"], s1=sd["records"]["s1"][:-1])))


def test_predictor_takes_a_format_argument():
    import inspect
    from deepfm_amd.training import QuantizedPredictor
    sig = inspect.signature(QuantizedPredictor.__init__)
    assert list(sig.parameters)[1:] == ["model", "batch_size", "tables", "use_graph", "calibrator", "fmt"]
    assert sig.parameters["fmt"].default == "int8"
