"""What tests/test_gpu_quant.py (int8) and tests/test_gpu_quant_uint4.py share: a descriptor per record format of
csrc/quant.hip and the helpers that build models, tables, batches and records, launch the kernels into guarded buffers
and hold the gather to its bars, each parametrised by the descriptor.  The numpy restatements
(tests/quant_reference.py, tests/quant4_reference.py) stay separate modules: independent specifications.  Needs torch
and, for everything that launches, the GPU."""
import ctypes as C
import functools
import types
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

from tests import quant4_reference, quant_reference
from tests.helpers import GuardedBuffer, assert_close, npy, schema_from_fields, to_device_batch
from tests.test_gpu_uniform_gather import _batch, _fields, _fm64, _module

F32 = np.float32


@dataclass(frozen=True)
class Format:
    name: str                               # QuantizedTables' and QuantizedPredictor's ``fmt``
    enum: int                               # DFM_QUANT_*
    ref: types.ModuleType                   # the numpy restatement
    row_bytes: Callable[[int], int]         # bytes of a record of width D
    gather_cols: Callable[[int], int]       # columns of a lane of the gather at width D

    def spw(self, D):
        """Samples per workgroup of the gather."""
        return 64 // (D // self.gather_cols(D))


INT8 = Format("int8", 1, quant_reference, lambda D: 16 + D, lambda D: 4)
UINT4 = Format("uint4", 4, quant4_reference, lambda D: 8 + D // 2, lambda D: 4 if D == 16 else 8)

WIDTHS = [16, 32, 64]
MIXES = [(1, 0), (3, 2), (0, 4), (26, 13), (48, 16)]
BATCHES = [1, 7, 9, 15, 17, 31, 33, 63, 65, 131]    # one under and one over 8, 16, 32 and 64 samples per workgroup
KINDS = ["deepfm", "xdeepfm", "attention_deepfm"]
PB, PN = 64, 37          # predictor batch size, samples per record


# ---------------------------------------------------------------------------------------------- quantise / dequantise
def quantize_on_device(fmt, w2, w1, D, packed):
    """(records (rows, row bytes) uint8, flag) of ``dfm_quantize_rows`` on a contiguous table or on packed row records
    ([w2 (D) | w1, m1, v1, pad | m2 (D) | v2 (D) | pad], as FeatureEmbedding.pack_tables_); the guards are checked."""
    from deepfm_amd import _lib
    lib = _lib.load()
    rows, rb = w2.shape[0], fmt.row_bytes(D)
    if packed:
        rs = ((3 * D + 4 + 31) // 32) * 32
        buf = torch.full((rows, rs), 7.0, device="cuda")          # moments and padding: never read
        buf[:, :D] = torch.from_numpy(w2).cuda()
        buf[:, D] = torch.from_numpy(w1[:, 0]).cuda()
        t2, t1 = buf[:, :D], buf[:, D:D + 1]
    else:
        t2, t1 = torch.from_numpy(w2).cuda(), torch.from_numpy(w1).cuda()
    out = GuardedBuffer(rows * rb // 4, 0.0)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.dfm_quantize_rows(t2.data_ptr(), t2.stride(0), t1.data_ptr(), t1.stride(0), rows, D, fmt.enum,
                                     out.ptr(), flag.data_ptr(), _lib.stream_handle()))
    torch.cuda.synchronize()
    assert out.guards_intact()
    return npy(out.t).view(np.uint8).reshape(rows, rb), int(flag.item())


def dequantize_on_device(fmt, records, D):
    """(w2 (rows, D), w1 (rows, 1)) of ``dfm_dequantize_rows`` on host records; the guards are checked."""
    from deepfm_amd import _lib
    rows = records.shape[0]
    rec = torch.from_numpy(records).cuda()
    o2, o1 = GuardedBuffer(rows * D), GuardedBuffer(rows)
    _lib.check(_lib.load().dfm_dequantize_rows(rec.data_ptr(), rows, D, fmt.enum, o2.ptr(), o1.ptr(),
                                               _lib.stream_handle()))
    torch.cuda.synchronize()
    assert o2.guards_intact() and o1.guards_intact()
    return npy(o2.t).reshape(rows, D), npy(o1.t).reshape(rows, 1)


def small_model(kind, fields, D, seed=0, packed=False):
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


def pred_fields(D):
    """5 SPARSE (a ``user_id``; vocabularies of 2 and 3) + 3 DENSE fields, interleaved."""
    sp = [("user_id", 23), ("s1", 2), ("s2", 3), ("s3", 97), ("s4", 150)]
    out = []
    for i, (name, V) in enumerate(sp):
        out.append(dict(name=name, type="sparse", vocab=V, dim=D, max_len=1, combiner="mean"))
        if i < 3:
            out.append(dict(name=f"d{i}", type="dense", vocab=0, dim=D, max_len=1, combiner="mean"))
    return out


# ---------------------------------------------------------------------------------------------- the gather
def gather_fields(ns, nd, D):
    fields = _fields(ns, nd, D)
    small = iter((2, 3))
    for f in fields:                                   # vocabularies of 2 and 3 on the first two SPARSE fields
        if f["type"] == "sparse":
            f["vocab"] = next(small, f["vocab"])
    return fields


def quant_call(fmt, emb, fields, D, recs, inputs, B, labels=None, fm=True, check=True):
    """One dfm_embedding_forward_quant launch into guarded buffers: dict(fo, fe, fm, fm_sum, labels, flag).  The
    return code goes through ``_lib.check``; with ``check=False`` a refusal's code is returned instead."""
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
    rc = lib.dfm_embedding_forward_quant(
        arr, F, D, fmt.enum, (C.c_void_p * F)(*[t.data_ptr() for t in inputs]), _lib.ptr(src),
        lab.ptr() if src is not None else None, B, fo.ptr(), fe.ptr(), fmo.ptr() if fm else None,
        fms.ptr() if fm else None, flag.data_ptr(), _lib.stream_handle())
    if rc and not check:
        return rc
    _lib.check(rc)
    torch.cuda.synchronize()
    assert all(g.guards_intact() for g in (fo, fe, fmo, fms, lab))
    return dict(fo=npy(fo.t).reshape(B, 1), fe=npy(fe.t).reshape(B, F, D), fm=npy(fmo.t).reshape(B, 1),
                fm_sum=npy(fms.t).reshape(B, D), labels=npy(lab.t), flag=int(flag.item()))


@functools.lru_cache(maxsize=None)
def gather_setup(fmt, ns, nd, D):
    """(fields, module, host records, device records, the dequantised tables) of one format, mix and width, built
    once and left unchanged."""
    fields = gather_fields(ns, nd, D)
    emb = _module(fields, D, seed=D + 7 * ns + nd)
    host, recs, deq = {}, {}, {}
    for f in fields:
        if f["type"] == "sparse":
            name = f["name"]
            with torch.no_grad():           # trained-like magnitudes; the padding row stays 0
                emb.second_order_embeddings[name].weight[1:].uniform_(-1.0, 1.0)
                emb.first_order_embeddings[name].weight[1:].uniform_(-1.0, 1.0)
            host[name] = fmt.ref.quantize_table(npy(emb.second_order_embeddings[name].weight),
                                                npy(emb.first_order_embeddings[name].weight))
            recs[name] = torch.from_numpy(host[name]).cuda()
            deq[name] = fmt.ref.dequantize_table(host[name])
    return fields, emb, host, recs, deq


def edge_batch(fields, B, rng):
    """Random ids with vocab - 1 in the last sample and, from sample 1 on, 0 (the padding id) and vocab - 1 in turn
    over the SPARSE fields."""
    batch = _batch(fields, B, rng)
    for j, f in enumerate(fields):
        if f["type"] == "sparse":
            batch[f["name"]][B - 1] = f["vocab"] - 1
            if B > 2:
                batch[f["name"]][1] = 0 if j % 4 else f["vocab"] - 1
            if B > 3:
                batch[f["name"]][2] = f["vocab"] - 1 if j % 4 else 0
    return batch


def device_inputs(fields, batch):
    return [torch.from_numpy(batch[f["name"]]).cuda() for f in fields]


def check_gather(fields, emb, D, deq, batch, got, labels, what):
    """SPARSE columns: the restatement's dequantised rows, bit for bit.  DENSE columns: the fp32 gather's, bit for bit.
    The sums: the project's 1e-4 bar against fp64 sums over those values."""
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
    # 0.5 * sum_d (S_d^2 - SQ_d) cancels: the floor test_gpu_uniform_gather._check_forward uses
    floor = 1e-6 * float((ref.astype(np.float64) ** 2).sum(axis=(1, 2)).max())
    assert_close(got["fm"], _fm64(ref), what=f"{what} fm", floor=floor)
    assert_close(got["fm_sum"], ref.astype(np.float64).sum(axis=1), what=f"{what} fm_sum")
    assert np.array_equal(got["labels"], labels), f"{what}: labels"


def check_gather_matrix(fmt, D, mix):
    """Every batch of BATCHES against check_gather; at B in (9, 33, 131) the optional outputs change nothing else and a
    second launch changes no bit."""
    ns, nd = mix
    fields, emb, host, recs, deq = gather_setup(fmt, ns, nd, D)
    rng = np.random.default_rng(D * 1000 + ns * 10 + nd)
    for B in BATCHES:
        batch = edge_batch(fields, B, rng)
        labels = rng.random(B).astype(F32)
        inputs = device_inputs(fields, batch)
        got = quant_call(fmt, emb, fields, D, recs, inputs, B, labels)
        check_gather(fields, emb, D, deq, batch, got, labels, f"{fmt.name} D={D} {ns}+{nd} B={B}")
        if B in (9, 33, 131):
            bare = quant_call(fmt, emb, fields, D, recs, inputs, B, None, fm=False)
            assert np.array_equal(bare["fe"], got["fe"]) and np.array_equal(bare["fo"], got["fo"])
            again = quant_call(fmt, emb, fields, D, recs, inputs, B, labels)
            for k in ("fo", "fe", "fm", "fm_sum", "labels"):
                assert np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)), (B, k)


def check_out_of_range_id(fmt, D, mix, bad, rng):
    """An id of -1 or vocab in the LAST SPARSE field at the LAST sample (the ragged tail workgroup; with 48 SPARSE
    fields, the second pass) sets the flag and scores as id 0."""
    ns, nd = mix
    fields, emb, host, recs, deq = gather_setup(fmt, ns, nd, D)
    B = fmt.spw(D) + 1
    batch = edge_batch(fields, B, rng)
    last = [f for f in fields if f["type"] == "sparse"][-1]
    zero = {k: v.copy() for k, v in batch.items()}
    zero[last["name"]][B - 1] = 0
    batch[last["name"]][B - 1] = -1 if bad == -1 else last["vocab"]
    out = [quant_call(fmt, emb, fields, D, recs, device_inputs(fields, b), B) for b in (batch, zero)]
    assert out[0]["flag"] == 1 and out[1]["flag"] == 0
    for k in ("fo", "fe", "fm", "fm_sum"):
        assert np.array_equal(out[0][k], out[1][k]), k


# ---------------------------------------------------------------------------------------------- the predictor
def record(layout, fields, batch, labels):
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


def records(pred, fields, rng, count):
    out = []
    for _ in range(count):
        batch = edge_batch(fields, PN, rng)
        out.append(record(pred.layout, fields, batch, (rng.random(PN) < 0.3).astype(F32)))
    return out


def dequantized_copy(kind, fields, D, model, tables):
    """A fresh model of the same configuration with ``model``'s state, its SPARSE tables overwritten with
    ``tables.dequantized()``: what the quantised predictor should compute, in fp32."""
    copy, _ = small_model(kind, fields, D, seed=99)
    copy.load_state_dict(model.state_dict())
    with torch.no_grad():
        for name, (w2, w1) in tables.dequantized().items():
            copy.embedding.second_order_embeddings[name].weight.copy_(w2)
            copy.embedding.first_order_embeddings[name].weight.copy_(w1)
    return copy


def fmt_kw(fmt):
    """The ``fmt`` keyword of QuantizedTables.from_model and QuantizedPredictor; int8 is their default and goes unsaid,
    so that the default stays under test."""
    return {} if fmt is INT8 else dict(fmt=fmt.name)


def check_predictor(fmt, kind, use_graph):
    from deepfm_amd.training import FusedPredictor, QuantizedPredictor, QuantizedTables
    D = 16
    fields = pred_fields(D)
    model, _ = small_model(kind, fields, D, seed=3)
    tables = QuantizedTables.from_model(model, **fmt_kw(fmt))
    pred = QuantizedPredictor(model, PB, tables=tables, use_graph=use_graph)     # fmt is not needed: the tables' holds
    assert pred.tables is tables and pred.tables.format == fmt.name and model.training
    rng = np.random.default_rng(len(kind))
    recs = records(pred, fields, rng, 4)
    ref = FusedPredictor(dequantized_copy(kind, fields, D, model, tables), PB, use_graph=False)
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


def check_refresh_after_a_training_step(fmt, kind, use_graph):
    """One optimizer step on every parameter, then refresh(): the predictor (its graphs untouched) matches the
    comparator rebuilt from the new tables."""
    from deepfm_amd.training import FusedPredictor, QuantizedPredictor
    D = 32
    fields = pred_fields(D)
    model, _ = small_model(kind, fields, D, seed=5)
    pred = QuantizedPredictor(model, PB, use_graph=use_graph, **fmt_kw(fmt))     # tables=None: built from the model
    tables = pred.tables
    assert tables.format == fmt.name and tables.row_bytes == fmt.row_bytes(D)
    rng = np.random.default_rng(11)
    recs = records(pred, fields, rng, 2)
    before = pred.predict_from(recs[0], PN).clone()
    graphs = [s.graph for s in pred.slots]
    ptrs = {n: r.data_ptr() for n, r in tables.records.items()}
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    batch = to_device_batch(edge_batch(fields, PB, rng))
    labels = torch.from_numpy((rng.random(PB) < 0.3).astype(F32)).cuda()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(model(batch).view(-1), labels)
    loss.backward()
    opt.step()
    tables.refresh()
    assert graphs == [s.graph for s in pred.slots] and ptrs == {n: r.data_ptr() for n, r in tables.records.items()}
    ref = FusedPredictor(dequantized_copy(kind, fields, D, model, tables), PB, use_graph=False)
    for k, rec in enumerate(recs):
        p = pred.predict_from(rec, PN)
        want = ref.predict_from(rec, PN)
        assert_close(npy(pred.last_logits(PN)), npy(ref.last_logits(PN)), what=f"{kind} record {k} logits")
        assert_close(npy(p), npy(want), what=f"{kind} record {k} probabilities")
    assert not torch.equal(pred.predict_from(recs[0], PN), before)          # the step did move the scores


def check_evaluate_returns_the_fp32_predictors_keys(fmt, kind):
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import FusedPredictor, QuantizedPredictor
    from tests.helpers import random_fields_batch
    D = 16
    fields = pred_fields(D)
    model, _ = small_model(kind, fields, D, seed=7)
    rng = np.random.default_rng(5)
    n = 3 * PB + 11
    feats = random_fields_batch(fields, n, rng, zero_frac=0.05)
    cols = PackedColumns(model.schema, feats, (rng.random(n) < 0.4).astype(F32))
    kw = dict(ranking_ks=[1, 5], group_auc=True, calibration_bins=10)
    quant = QuantizedPredictor(model, PB, **fmt_kw(fmt))
    got = quant.evaluate(cols, **kw)
    ref = FusedPredictor(dequantized_copy(kind, fields, D, model, quant.tables), PB)
    want = ref.evaluate(cols, **kw)
    assert set(got) == set(want) and {"auc", "logloss", "HR@1", "NDCG@5", "gauc", "ece"} <= set(got)
    assert_close(npy(quant.last_scores), npy(ref.last_scores), what=f"{kind} scores")
    assert torch.equal(quant.last_labels, ref.last_labels)
