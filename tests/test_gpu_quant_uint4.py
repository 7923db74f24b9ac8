"""GPU: row-wise 4-bit embedding tables (csrc/quant.hip with DFM_QUANT_UINT4_ROWWISE, training/quantized.py and
QuantizedPredictor with ``"uint4"``).

Bars, as tests/test_gpu_quant.py: the quantiser, its inverse and the SPARSE columns of the gather match the numpy
restatement (tests/quant4_reference.py) bit for bit; the DENSE columns match the fp32 gather bit for bit; every sum is
held to the project's 1e-4 bar (helpers.assert_close) against fp64 sums over the dequantised values, and the predictor's
logits to the same bar against ``FusedPredictor`` on a copy of the model that holds the dequantised tables."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import quant4_reference as Q
from tests.helpers import GuardedBuffer, assert_close, npy, random_fields_batch, schema_from_fields, to_device_batch
from tests.test_gpu_uniform_gather import _batch, _fields, _fm64, _module

pytestmark = pytest.mark.gpu

WIDTHS = [16, 32, 64]
FMT = 4          # DFM_QUANT_UINT4_ROWWISE
F16, F32 = np.float16, np.float32


def _rb(D):
    return 8 + D // 2


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


def _quantize_on_device(w2, w1, D, packed):
    """(records (rows, 8 + D / 2) uint8, flag) of ``dfm_quantize_rows`` on a contiguous table or on packed row records
    ([w2 (D) | w1, m1, v1, pad | m2 (D) | v2 (D) | pad], as FeatureEmbedding.pack_tables_); the guards are checked."""
    from deepfm_amd import _lib
    lib = _lib.load()
    rows = w2.shape[0]
    if packed:
        rs = ((3 * D + 4 + 31) // 32) * 32
        buf = torch.full((rows, rs), 7.0, device="cuda")          # moments and padding: never read
        buf[:, :D] = torch.from_numpy(w2).cuda()
        buf[:, D] = torch.from_numpy(w1[:, 0]).cuda()
        t2, t1 = buf[:, :D], buf[:, D:D + 1]
    else:
        t2, t1 = torch.from_numpy(w2).cuda(), torch.from_numpy(w1).cuda()
    out = GuardedBuffer(rows * _rb(D) // 4, 0.0)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.dfm_quantize_rows(t2.data_ptr(), t2.stride(0), t1.data_ptr(), t1.stride(0), rows, D, FMT, out.ptr(),
                                     flag.data_ptr(), _lib.stream_handle()))
    torch.cuda.synchronize()
    assert out.guards_intact()
    return npy(out.t).view(np.uint8).reshape(rows, _rb(D)), int(flag.item())


@pytest.mark.parametrize("packed", [False, True], ids=["contiguous", "packed"])
@pytest.mark.parametrize("rows", [1, 2, 3, 257])
@pytest.mark.parametrize("D", WIDTHS)
def test_quantize_and_dequantize_match_the_restatement(D, rows, packed):
    from deepfm_amd import _lib
    lib = _lib.load()
    w2, w1 = _table(rows, D, np.random.default_rng([D, rows]))
    want = Q.quantize_table(w2, w1)
    got, flag = _quantize_on_device(w2, w1, D, packed)
    assert flag == 0
    assert np.array_equal(got, want), f"records differ in rows {np.unique(np.nonzero(got != want)[0])[:8]}"
    scale, lo, _, q = Q.unpack(want)
    if rows == 257:                             # the special rows are what they are meant to be
        assert scale[2] == F16(2.0 ** -24) and not q[2].any()
        assert lo[3].view(np.uint16) == 0x8001
        assert lo[4] == F16(-0.75) and F32(lo[1]) < w2[1, 0] and scale[1] > 0
        assert lo[5] == F16(-1.0) and scale[5] == np.nextafter(F16(0.125), F16(1)) and w2[5].max() > 0.875
    # the inverse, on the restatement's records: a second, independent route
    rec = torch.from_numpy(want).cuda()
    o2, o1 = GuardedBuffer(rows * D), GuardedBuffer(rows)
    _lib.check(lib.dfm_dequantize_rows(rec.data_ptr(), rows, D, FMT, o2.ptr(), o1.ptr(), _lib.stream_handle()))
    torch.cuda.synchronize()
    assert o2.guards_intact() and o1.guards_intact()
    d2, d1 = Q.dequantize_table(want)
    assert np.array_equal(npy(o2.t).view(np.uint32).reshape(rows, D), d2.view(np.uint32))
    assert np.array_equal(npy(o1.t).reshape(rows, 1), w1) and np.array_equal(d1, w1)
    assert not npy(o2.t)[:D].view(np.uint32).any()                            # the padding row is exactly 0
    err = np.abs(d2.astype(np.float64) - w2.astype(np.float64))
    assert (err <= Q.bound(w2)[:, None]).all()


def _small_model(kind, fields, D, seed=0, packed=False):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    cfg.feature.fm_embed_dim = D
    cfg.dnn.hidden_units, cfg.dnn.dropout = [32, 32], 0.0
    cfg.cin.layer_sizes, cfg.cin.split_half = [8, 8], True
    cfg.attention.num_heads, cfg.attention.attention_dim, cfg.attention.num_layers = 2, 16, 1
    torch.manual_seed(seed)
    model = create_model(kind, schema_from_fields(fields), cfg).cuda().train()
    with torch.no_grad():
        for m in model.dnn.mlp:             # non-trivial running statistics
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
        for f in fields:                    # non-zero DENSE biases; tables of trained-like size
            emb = model.embedding
            if f["type"] == "dense":
                for m in (emb.second_order_embeddings[f["name"]], emb.first_order_embeddings[f["name"]]):
                    m.bias.uniform_(-0.5, 0.5)
            else:
                emb.second_order_embeddings[f["name"]].weight[1:].uniform_(-0.5, 0.5)
                emb.first_order_embeddings[f["name"]].weight[1:].uniform_(-0.5, 0.5)
    if packed:
        model.embedding.pack_tables_()
        model.embedding.set_grad_mode("rowsparse")
    model.embedding.strict_indices = True
    return model, cfg


def _pred_fields(D):
    """5 SPARSE (a ``user_id``; vocabularies of 2 and 3) + 3 DENSE fields, interleaved."""
    sp = [("user_id", 23), ("s1", 2), ("s2", 3), ("s3", 97), ("s4", 150)]
    out = []
    for i, (name, V) in enumerate(sp):
        out.append(dict(name=name, type="sparse", vocab=V, dim=D, max_len=1, combiner="mean"))
        if i < 3:
            out.append(dict(name=f"d{i}", type="dense", vocab=0, dim=D, max_len=1, combiner="mean"))
    return out


@pytest.mark.parametrize("mode", ["dense", "rowsparse"])
@pytest.mark.parametrize("D", WIDTHS)
def test_tables_from_model_in_both_grad_modes(D, mode):
    """QuantizedTables.from_model(fmt="uint4") on contiguous tables and on packed row records: the restatement's
    records, bit for bit; dequantized() is the restatement's; error_bound() bounds |dequantized - fp32|."""
    from deepfm_amd.training import QuantizedTables
    fields = _pred_fields(D)
    model, _ = _small_model("deepfm", fields, D, seed=D, packed=(mode == "rowsparse"))
    emb = model.embedding
    assert emb.grad_mode == mode
    tables = QuantizedTables.from_model(model, fmt="uint4")
    assert tables.format == "uint4" and tables.row_bytes == _rb(D)
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
    assert tables.nbytes == total * _rb(D) and tables.fp32_nbytes == total * (4 * D + 4)
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
    model, _ = _small_model("deepfm", _pred_fields(D), D)
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
MIXES = [(1, 0), (3, 2), (0, 4), (26, 13), (48, 16)]
BATCHES = [1, 7, 9, 15, 17, 31, 33, 63, 65, 131]    # one under and one over 8, 16, 32 and 64 samples per workgroup


def _gather_fields(ns, nd, D):
    fields = _fields(ns, nd, D)
    small = iter((2, 3))
    for f in fields:                                   # vocabularies of 2 and 3 on the first two SPARSE fields
        if f["type"] == "sparse":
            f["vocab"] = next(small, f["vocab"])
    return fields


def _quant_call(emb, fields, D, recs, inputs, B, labels=None, fm=True, fmt=FMT):
    """One dfm_embedding_forward_quant launch into guarded buffers: dict(fo, fe, fm, fm_sum, labels, flag)."""
    from deepfm_amd import _lib
    lib = _lib.load()
    F = len(fields)
    arr = (_lib.QuantField * F)()
    for i, f in enumerate(fields):
        if f["type"] == "sparse":
            arr[i].kind, arr[i].vocab, arr[i].rows = _lib.SPARSE, f["vocab"], recs[f["name"]].data_ptr()
        else:
            second, first = emb.second_order_embeddings[f["name"]], emb.first_order_embeddings[f["name"]]
            arr[i].kind = _lib.DENSE
            arr[i].w2, arr[i].b2 = second.weight.data_ptr(), second.bias.data_ptr()
            arr[i].w1, arr[i].b1 = first.weight.data_ptr(), first.bias.data_ptr()
    fo, fe = GuardedBuffer(B), GuardedBuffer(B * F * D)
    fmo, fms, lab = GuardedBuffer(B), GuardedBuffer(B * D), GuardedBuffer(B)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    src = torch.from_numpy(labels).cuda() if labels is not None else None
    _lib.check(lib.dfm_embedding_forward_quant(
        arr, F, D, fmt, (C.c_void_p * F)(*[t.data_ptr() for t in inputs]), _lib.ptr(src),
        lab.ptr() if src is not None else None, B, fo.ptr(), fe.ptr(), fmo.ptr() if fm else None,
        fms.ptr() if fm else None, flag.data_ptr(), _lib.stream_handle()))
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in (fo, fe, fmo, fms, lab))
    return dict(fo=npy(fo.t).reshape(B, 1), fe=npy(fe.t).reshape(B, F, D), fm=npy(fmo.t).reshape(B, 1),
                fm_sum=npy(fms.t).reshape(B, D), labels=npy(lab.t), flag=int(flag.item()))


_SETUPS = {}


def _gather_setup(ns, nd, D):
    """(fields, module, host records, device records, the dequantised tables) of one mix and width, built once."""
    if (ns, nd, D) not in _SETUPS:
        fields = _gather_fields(ns, nd, D)
        emb = _module(fields, D, seed=D + 7 * ns + nd)
        host, recs, deq = {}, {}, {}
        for f in fields:
            if f["type"] == "sparse":
                name = f["name"]
                with torch.no_grad():           # trained-like magnitudes; the padding row stays 0
                    emb.second_order_embeddings[name].weight[1:].uniform_(-1.0, 1.0)
                    emb.first_order_embeddings[name].weight[1:].uniform_(-1.0, 1.0)
                host[name] = Q.quantize_table(npy(emb.second_order_embeddings[name].weight),
                                              npy(emb.first_order_embeddings[name].weight))
                recs[name] = torch.from_numpy(host[name]).cuda()
                deq[name] = Q.dequantize_table(host[name])
        _SETUPS[(ns, nd, D)] = (fields, emb, host, recs, deq)
    return _SETUPS[(ns, nd, D)]


def _edge_batch(fields, B, rng):
    """Random ids with 0 and vocab - 1 present and a padding id in sample 0 of every other SPARSE field."""
    batch = _batch(fields, B, rng)
    for j, f in enumerate(fields):
        if f["type"] == "sparse":
            batch[f["name"]][B - 1] = f["vocab"] - 1
            if B > 2:
                batch[f["name"]][1] = 0 if j % 4 else f["vocab"] - 1
            if B > 3:
                batch[f["name"]][2] = f["vocab"] - 1 if j % 4 else 0
    return batch


def _check_gather(fields, emb, D, deq, batch, got, labels, what):
    B, F = got["fe"].shape[:2]
    db = to_device_batch(batch)
    with torch.no_grad():
        inputs, _ = emb._gather_inputs(db)
        _, fe32, _, _ = emb._launch_forward(inputs, B)
    fe32 = npy(fe32)
    ref = np.zeros((B, F, D), F32)
    fo64 = np.zeros((B, 1))
    for j, f in enumerate(fields):
        name = f["name"]
        if f["type"] == "sparse":
            d2, d1 = deq[name]
            ref[:, j] = d2[batch[name]]
            fo64 += d1[batch[name]].astype(np.float64)
        else:
            ref[:, j] = fe32[:, j]
            w1 = float(npy(emb.first_order_embeddings[name].weight)[0, 0])
            b1 = float(npy(emb.first_order_embeddings[name].bias)[0])
            fo64 += (batch[name].astype(np.float64) * w1 + b1)[:, None]
    sp = [j for j, f in enumerate(fields) if f["type"] == "sparse"]
    de = [j for j, f in enumerate(fields) if f["type"] == "dense"]
    assert got["flag"] == 0, what
    assert np.array_equal(got["fe"][:, sp].view(np.uint32), ref[:, sp].view(np.uint32)), f"{what}: SPARSE columns"
    assert np.array_equal(got["fe"][:, de].view(np.uint32), fe32[:, de].view(np.uint32)), f"{what}: DENSE columns"
    assert_close(got["fo"], fo64, what=f"{what} first_order")
    # 0.5 * sum_d (S_d^2 - SQ_d) cancels: the floor test_gpu_quant._check_gather uses
    floor = 1e-6 * float((ref.astype(np.float64) ** 2).sum(axis=(1, 2)).max())
    assert_close(got["fm"], _fm64(ref), what=f"{what} fm", floor=floor)
    assert_close(got["fm_sum"], ref.astype(np.float64).sum(axis=1), what=f"{what} fm_sum")
    assert np.array_equal(got["labels"], labels), f"{what}: labels"


@pytest.mark.parametrize("mix", MIXES, ids=lambda m: f"{m[0]}s{m[1]}d")
@pytest.mark.parametrize("D", WIDTHS)
def test_gather(D, mix):
    ns, nd = mix
    fields, emb, host, recs, deq = _gather_setup(ns, nd, D)
    rng = np.random.default_rng(D * 1000 + ns * 10 + nd)
    for B in BATCHES:
        batch = _edge_batch(fields, B, rng)
        labels = rng.random(B).astype(F32)
        inputs = [torch.from_numpy(batch[f["name"]]).cuda() for f in fields]
        got = _quant_call(emb, fields, D, recs, inputs, B, labels)
        _check_gather(fields, emb, D, deq, batch, got, labels, f"D={D} {ns}+{nd} B={B}")
        if B in (9, 33, 131):              # the optional outputs change nothing else; a second launch, no other bit
            bare = _quant_call(emb, fields, D, recs, inputs, B, None, fm=False)
            assert np.array_equal(bare["fe"], got["fe"]) and np.array_equal(bare["fo"], got["fo"])
            again = _quant_call(emb, fields, D, recs, inputs, B, labels)
            for k in ("fo", "fe", "fm", "fm_sum", "labels"):
                assert np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)), (B, k)


@pytest.mark.parametrize("D", WIDTHS)
def test_gather_dense_columns_are_the_int8_gathers(D):
    """DENSE columns (and, with no SPARSE field, every output) bit for bit those of the int8 gather."""
    from tests import quant_reference as Q8
    for ns, nd in ((0, 4), (3, 2)):
        fields, emb, host, recs, deq = _gather_setup(ns, nd, D)
        rng = np.random.default_rng(D + ns)
        recs8 = {f["name"]: torch.from_numpy(Q8.quantize_table(npy(emb.second_order_embeddings[f["name"]].weight),
                                                               npy(emb.first_order_embeddings[f["name"]].weight))).cuda()
                 for f in fields if f["type"] == "sparse"}
        de = [j for j, f in enumerate(fields) if f["type"] == "dense"]
        for B in (1, 33, 131):
            batch = _edge_batch(fields, B, rng)
            inputs = [torch.from_numpy(batch[f["name"]]).cuda() for f in fields]
            got4 = _quant_call(emb, fields, D, recs, inputs, B)
            got8 = _quant_call(emb, fields, D, recs8, inputs, B, fmt=1)
            assert np.array_equal(got4["fe"][:, de].view(np.uint32), got8["fe"][:, de].view(np.uint32))
            if ns == 0:
                assert np.array_equal(got4["fo"].view(np.uint32), got8["fo"].view(np.uint32))


@pytest.mark.parametrize("bad", [-1, "vocab"])
@pytest.mark.parametrize("D,mix", [(16, (26, 13)), (32, (48, 16)), (64, (3, 2))])
def test_gather_out_of_range_id_sets_the_flag_and_scores_as_id_0(D, mix, bad):
    """In the LAST SPARSE field at the LAST sample (the ragged tail workgroup; with 48 SPARSE fields, the second
    pass)."""
    ns, nd = mix
    fields, emb, host, recs, deq = _gather_setup(ns, nd, D)
    rng = np.random.default_rng(D)
    B = 64 // (D // 8) + 1
    batch = _edge_batch(fields, B, rng)
    last = [f for f in fields if f["type"] == "sparse"][-1]
    zero = {k: v.copy() for k, v in batch.items()}
    zero[last["name"]][B - 1] = 0
    batch[last["name"]][B - 1] = -1 if bad == -1 else last["vocab"]
    out = [_quant_call(emb, fields, D, recs, [torch.from_numpy(b[f["name"]]).cuda() for f in fields], B)
           for b in (batch, zero)]
    assert out[0]["flag"] == 1 and out[1]["flag"] == 0
    for k in ("fo", "fe", "fm", "fm_sum"):
        assert np.array_equal(out[0][k], out[1][k]), k


# ---------------------------------------------------------------------------------------------- the predictor
KINDS = ["deepfm", "xdeepfm", "attention_deepfm"]
PB, PN = 64, 37          # predictor batch size, samples per record


def _record(layout, fields, batch, labels):
    rec = np.zeros(layout.record_bytes, np.uint8)
    ids, dense, lab, _ = layout.views(rec)
    n = len(labels)
    si = di = 0
    for f in fields:
        if f["type"] == "sparse":
            ids[si, :n] = batch[f["name"]]; si += 1
        else:
            dense[di, :n] = batch[f["name"]]; di += 1
    lab[:n] = labels
    return torch.from_numpy(rec).cuda()


def _dequantized_copy(kind, fields, D, model, tables):
    """A fresh model of the same configuration with ``model``'s state, its SPARSE tables overwritten with
    ``tables.dequantized()``: what the quantised predictor should compute, in fp32."""
    copy, _ = _small_model(kind, fields, D, seed=99)
    copy.load_state_dict(model.state_dict())
    with torch.no_grad():
        for name, (w2, w1) in tables.dequantized().items():
            copy.embedding.second_order_embeddings[name].weight.copy_(w2)
            copy.embedding.first_order_embeddings[name].weight.copy_(w1)
    return copy


def _records(pred, fields, rng, count):
    out = []
    for _ in range(count):
        batch = _edge_batch(fields, PN, rng)
        out.append(_record(pred.layout, fields, batch, (rng.random(PN) < 0.3).astype(F32)))
    return out


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", KINDS)
def test_predictor(kind, use_graph):
    from deepfm_amd.training import FusedPredictor, QuantizedPredictor, QuantizedTables
    D = 16
    fields = _pred_fields(D)
    model, _ = _small_model(kind, fields, D, seed=3)
    tables = QuantizedTables.from_model(model, fmt="uint4")
    pred = QuantizedPredictor(model, PB, tables=tables, use_graph=use_graph)     # fmt is not needed: the tables' holds
    assert pred.tables is tables and pred.tables.format == "uint4" and model.training
    rng = np.random.default_rng(len(kind))
    recs = _records(pred, fields, rng, 4)
    ref = FusedPredictor(_dequantized_copy(kind, fields, D, model, tables), PB, use_graph=False)
    first = []
    for k, rec in enumerate(recs):          # four calls on different records: both graph slots are re-pointed
        p = pred.predict_from(rec, PN)
        lg = pred.last_logits(PN)
        want_p = ref.predict_from(rec, PN)
        assert p.shape == (PN, 1)
        assert_close(npy(lg), npy(ref.last_logits(PN)), what=f"{kind} record {k} logits")
        assert_close(npy(p), npy(want_p), what=f"{kind} record {k} probabilities")
        first.append((p.clone(), lg.clone()))
    assert not torch.equal(first[0][1], first[1][1])
    # the fp32 SPARSE tables are never read again: NaN in every one of them changes no bit
    saved = {}
    with torch.no_grad():
        for f in fields:
            if f["type"] == "sparse":
                for which in (model.embedding.second_order_embeddings, model.embedding.first_order_embeddings):
                    w = which[f["name"]].weight
                    saved[id(w)] = (w, w.detach().clone())
                    w.fill_(float("nan"))
    for k, rec in enumerate(recs):
        p = pred.predict_from(rec, PN)
        assert torch.equal(p, first[k][0]) and torch.equal(pred.last_logits(PN), first[k][1]), k
    with torch.no_grad():
        for w, v in saved.values():
            w.copy_(v)
    # the dict API agrees with the record API
    batch, _ = pred.layout.unpack(recs[2])
    assert torch.equal(pred.predict({k: v[:PN] for k, v in batch.items()}), first[2][0])


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", KINDS)
def test_refresh_after_a_training_step(kind, use_graph):
    """One optimizer step on every parameter, then refresh(): the predictor (its graphs untouched) matches the
    comparator rebuilt from the new tables."""
    from deepfm_amd.training import FusedPredictor, QuantizedPredictor
    D = 32
    fields = _pred_fields(D)
    model, _ = _small_model(kind, fields, D, seed=5)
    pred = QuantizedPredictor(model, PB, use_graph=use_graph, fmt="uint4")       # tables=None: built from the model
    tables = pred.tables
    assert tables.format == "uint4" and tables.row_bytes == _rb(D)
    rng = np.random.default_rng(11)
    recs = _records(pred, fields, rng, 2)
    before = pred.predict_from(recs[0], PN).clone()
    graphs = [s.graph for s in pred.slots]
    ptrs = {n: r.data_ptr() for n, r in tables.records.items()}
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    batch = to_device_batch(_edge_batch(fields, PB, rng))
    labels = torch.from_numpy((rng.random(PB) < 0.3).astype(F32)).cuda()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(model(batch).view(-1), labels)
    loss.backward()
    opt.step()
    tables.refresh()
    assert graphs == [s.graph for s in pred.slots] and ptrs == {n: r.data_ptr() for n, r in tables.records.items()}
    ref = FusedPredictor(_dequantized_copy(kind, fields, D, model, tables), PB, use_graph=False)
    for k, rec in enumerate(recs):
        p = pred.predict_from(rec, PN)
        want = ref.predict_from(rec, PN)
        assert_close(npy(pred.last_logits(PN)), npy(ref.last_logits(PN)), what=f"{kind} record {k} logits")
        assert_close(npy(p), npy(want), what=f"{kind} record {k} probabilities")
    assert not torch.equal(pred.predict_from(recs[0], PN), before)          # the step did move the scores


@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_returns_the_fp32_predictors_keys(kind):
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FusedPredictor, QuantizedPredictor
    D = 16
    fields = _pred_fields(D)
    model, _ = _small_model(kind, fields, D, seed=7)
    rng = np.random.default_rng(5)
    n = 3 * PB + 11
    feats = random_fields_batch(fields, n, rng, zero_frac=0.05)
    cols = PackedColumns(model.schema, feats, (rng.random(n) < 0.4).astype(F32))
    kw = dict(ranking_ks=[1, 5], group_auc=True, calibration_bins=10)
    quant = QuantizedPredictor(model, PB, fmt="uint4")
    got = quant.evaluate(cols, **kw)
    ref = FusedPredictor(_dequantized_copy(kind, fields, D, model, quant.tables), PB)
    want = ref.evaluate(cols, **kw)
    assert set(got) == set(want) and {"auc", "logloss", "HR@1", "NDCG@5", "gauc", "ece"} <= set(got)
    assert_close(npy(quant.last_scores), npy(ref.last_scores), what=f"{kind} scores")
    assert torch.equal(quant.last_labels, ref.last_labels)


def test_given_tables_decide_the_format():
    """int8 tables passed with fmt="uint4" still serve int8; uint4 tables serve uint4 under the default fmt."""
    from deepfm_amd.training import QuantizedPredictor, QuantizedTables
    D = 16
    fields = _pred_fields(D)
    model, _ = _small_model("deepfm", fields, D)
    t8 = QuantizedTables.from_model(model)
    pred = QuantizedPredictor(model, PB, tables=t8, use_graph=False, fmt="uint4")
    assert pred.tables is t8 and pred.tables.format == "int8"
    rec = _records(pred, fields, np.random.default_rng(0), 1)[0]
    want8 = QuantizedPredictor(model, PB, use_graph=False).predict_from(rec, PN)
    assert torch.equal(pred.predict_from(rec, PN), want8)
    t4 = QuantizedTables.from_model(model, fmt="uint4")
    got4 = QuantizedPredictor(model, PB, tables=t4, use_graph=False).predict_from(rec, PN)
    want4 = QuantizedPredictor(model, PB, use_graph=False, fmt="uint4").predict_from(rec, PN)
    assert torch.equal(got4, want4) and not torch.equal(got4, want8)
    with pytest.raises(ValueError, match="uint5"):
        QuantizedPredictor(model, PB, fmt="uint5")
