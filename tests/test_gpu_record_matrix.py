"""The record gather (``dfm_embedding_forward_record``: emb_fwd_record<D>) and the record backward
(``dfm_embedding_backward_record``: emb_bwd_record<D>, emb_bwd_record_fm<D>) over every launchable instantiation, field
width, row-tile, slice and stage edge of tests/record_cases.py, against the fp64 restatements of tests/helpers.py and
the bars derived there; and the same cases through the kernels of the dense-autograd path (emb_fwd_general,
``dfm_embedding_backward_dense``), which also take the schemas the record kernels refuse.

Every output lives in a guarded buffer filled with NaN: the guards are checked after every launch, the words a launch
must not write are checked for the NaN pattern, and the words it must write for being finite.  Each comparison prints
``RECORD-RATIO <case> <output>: worst |err| / bar`` (<= 1 passes)."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepfm_amd import _lib
from tests import helpers as H
from tests import record_cases as R

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
FWD_OUT = ("first_order", "field_embeddings", "flat_embeddings", "fm", "fm_sum")


def _st():
    return _lib.stream_handle()


def _emb(case, inp):
    from deepfm_amd.models.layers.embedding import FeatureEmbedding
    emb = FeatureEmbedding(H.schema_from_fields(list(case.fields)), case.D)
    emb.load_state_dict({k: torch.from_numpy(v) for k, v in inp["params"].items()}, strict=True)
    return emb.cuda()


def _record(case, inp):
    """The batch and its labels as one device record in the mixed layout."""
    from deepfm_amd.data.packed import RecordLayout
    lay = RecordLayout.of(H.schema_from_fields(list(case.fields)), case.B)
    rec = torch.zeros(lay.record_bytes, dtype=torch.uint8, device="cuda")
    views, labels = lay.unpack(rec)
    for k, dst in views.items():
        dst.copy_(torch.from_numpy(inp["batch"][k]).to(dst.dtype).view_as(dst))
    labels.copy_(torch.from_numpy(inp["labels"]))
    assert rec.data_ptr() % 16 == 0
    return rec


def _is_nan_pattern(t) -> bool:
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _same_bits(a, b) -> bool:
    """Bitwise equality (the NaN pattern of an unwritten word equals itself)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _report(name, what, r):
    print(f"RECORD-RATIO {name} {what}: {r:.3f}")
    assert r <= 1.0, f"{name} {what}: worst |err| / bar = {r:.3f}"


def _check_forward(name, got, ref, keys):
    for k in keys:
        _report(name, k, R.ratio(got[k], ref[k], ref["A"][k], ref["n"][k], R.C["forward"]))


def _sparse_bits(case, inp, flat, fe):
    """SPARSE fields: the flat columns are the table row, bit for bit, and so is field_embeddings without a projection."""
    off = 0
    for f, spec in enumerate(case.fields):
        d = spec["dim"]
        if spec["type"] == "sparse":
            rows = inp["params"][H._rec_keys(spec["name"])[0]][inp["batch"][spec["name"]]]
            assert np.array_equal(flat[:, off:off + d], rows), f"{spec['name']}: flat is not the table row"
            if d == case.D and fe is not None:
                assert np.array_equal(fe[:, f, :], rows), f"{spec['name']}: field_embeddings is not the table row"
        off += d


# ----------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("name", R.FWD_CASES)
def test_record_gather(name):
    case, inp, ref = R.CASES[name], R.inputs(name), R.forward_ref(name)
    B, F, D, T = case.B, case.F, case.D, case.T
    ld = T + R.LD_PAD_FLAT
    emb, rec = _emb(case, inp), _record(case, inp)

    def run(fe=True, fm=True, lab=True, S=True):
        b = dict(fo=H.GuardedBuffer(B), fe=H.GuardedBuffer(B * F * D), flat=H.GuardedBuffer(B * ld + 4),
                 fm=H.GuardedBuffer(B), lab=H.GuardedBuffer(B), S=H.GuardedBuffer(B * D))
        emb.forward_record(rec.data_ptr(), B, b["fo"].t, b["fe"].t if fe else None, b["flat"].ptr() + 16, ld,
                           b["fm"].t if fm else None, b["lab"].t if lab else None, fm_sum=b["S"].t if S else None)
        torch.cuda.synchronize()
        for k, g in b.items():
            assert g.guards_intact(), f"{name}: guard band of {k} written"
        assert _is_nan_pattern(b["flat"].t[:4]), "the floats before an offset flat pointer"
        rows = b["flat"].t[4:].view(B, ld)
        assert _is_nan_pattern(rows[:, T:]), "columns of a wider flat row outside the schema"
        for k, on in (("fe", fe), ("fm", fm), ("lab", lab), ("S", S)):
            assert on or _is_nan_pattern(b[k].t), f"{k} written without being asked for"
        return dict(first_order=b["fo"].t.clone(), field_embeddings=b["fe"].view(B, F, D).clone(),
                    flat_embeddings=rows[:, :T].clone(), fm=b["fm"].t.clone(), fm_sum=b["S"].view(B, D).clone(),
                    labels=b["lab"].t.clone())

    full = run()
    emb.raise_on_bad_index()
    got = {k: H.npy(v) for k, v in full.items()}
    _check_forward(name, got, ref, FWD_OUT)
    _sparse_bits(case, inp, got["flat_embeddings"], got["field_embeddings"])
    assert np.array_equal(got["labels"], inp["labels"]), "labels_out"
    bare = run(fe=False, fm=False, lab=False, S=False)
    for k in ("first_order", "flat_embeddings"):
        assert torch.equal(bare[k], full[k]), f"{k} changes bits without fe / fm"
    nosum = run(S=False)
    for k in ("first_order", "field_embeddings", "flat_embeddings", "fm", "labels"):
        assert torch.equal(nosum[k], full[k]), f"{k} changes bits with fm_sum off"
    assert all(torch.equal(v, full[k]) for k, v in run().items()), "two runs differ bitwise"


# ----------------------------------------------------------------------------- the backward
class _Grads:
    """One flat gradient buffer with every parameter's view at a 64-byte aligned offset (16-element pads), guarded."""

    def __init__(self, emb):
        self.named = dict(emb.named_parameters())
        pad = lambda n: (n + 15) // 16 * 16
        self.n = sum(pad(p.numel()) for p in self.named.values())
        self.buf = H.GuardedBuffer(self.n, 0.0)
        assert self.buf.ptr() % 64 == 0
        self.views, self.extent, off = {}, {}, 0
        for k, p in self.named.items():
            self.views[id(p)] = self.buf.t[off:off + p.numel()].view_as(p)
            self.extent[k] = (off, p.numel(), pad(p.numel()))
            off += pad(p.numel())

    def get(self, flat, k):
        off, n, _ = self.extent[k]
        return flat[..., off:off + n]


def _unnamed_rows(case, inp):
    """{parameter key: bool mask of the table rows no sample names (row 0 among them)}."""
    out = {}
    for spec in case.fields:
        if spec["type"] != "dense":
            free = np.ones(spec["vocab"], dtype=bool)
            ids = np.unique(inp["batch"][spec["name"]])
            free[ids[ids > 0]] = False
            k2, k1 = H._rec_keys(spec["name"])[:2]
            out[k2] = out[k1] = free
    return out


def _compare_grads(name, what, case, got_of, want):
    for k, v in want["grads"].items():
        _report(name, f"{what} {k}", R.ratio(got_of(k).reshape(v.shape), v, want["A"][k], want["n"][k],
                                             R.C[R.kind_of(k, case.fields)]))


@pytest.mark.parametrize("name", R.BWD_CASES)
def test_record_backward(name):
    case, inp = R.CASES[name], R.inputs(name)
    B, F, D, T = case.B, case.F, case.D, case.T
    lib = _lib.load()
    emb, rec = _emb(case, inp), _record(case, inp)
    plan = emb._ensure_plan(torch.device("cuda"))
    gr = _Grads(emb)
    n = gr.n
    parts = lib.dfm_embedding_backward_record_parts(B)
    assert parts == R.bwd_slices(B)[0] and lib.dfm_embedding_backward_record_workspace_bytes(B, n) == 4 * parts * n
    ws = H.GuardedBuffer(parts * n)
    sv = R.saved_f32(name)
    ld_g, ld_s = T + R.LD_PAD_G, T + R.LD_PAD_SAVED
    g_flat = np.full((B, ld_g), np.nan, dtype=np.float32)
    g_flat[:, :T] = inp["g_flat"]
    flat_s = np.full((B, ld_s), np.nan, dtype=np.float32)
    flat_s[:, :T] = sv["flat_embeddings"]
    dev = {k: H.GuardedBuffer.of(v) for k, v in dict(g_first=inp["g_first"], g_field=inp["g_field"], g_flat=g_flat,
                                                     flat=flat_s, g_fm=inp["g_fm"], S=sv["fm_sum"],
                                                     fe=sv["field_embeddings"]).items()}
    grads = emb._grad_struct(gr.views)
    free = _unnamed_rows(case, inp)

    def launch(fold, field, trio):
        ws.t.fill_(float("nan"))
        fm3 = (dev["g_fm"].ptr(), dev["S"].ptr(), dev["fe"].ptr()) if trio else (None, None, None)
        _lib.check(lib.dfm_embedding_backward_record(
            plan, C.c_void_p(rec.data_ptr()), B, dev["g_first"].ptr(), dev["g_field"].ptr() if field else None,
            dev["g_flat"].ptr(), ld_g, dev["flat"].ptr(), ld_s, *fm3, fold, grads, gr.buf.ptr(), n, ws.ptr(), _st()))
        torch.cuda.synchronize()
        assert ws.guards_intact() and gr.buf.guards_intact(), f"{name}: guard band written"
        assert all(g.guards_intact() for g in dev.values())
        slices = ws.view(parts, n)
        for k, (off, numel, padded) in gr.extent.items():
            assert bool(torch.isfinite(slices[:, off:off + numel]).all()), f"{k}: a word of the gradient was not stored"
            assert _is_nan_pattern(slices[:, off + numel:off + padded]), f"{k}: a pad word was written"
            if k in free:
                rows = slices[:, off:off + numel].reshape(parts, len(free[k]), -1)[:, torch.from_numpy(free[k]).cuda()]
                assert bool((rows.contiguous().view(torch.int32) == 0).all()), f"{k}: a row nobody names is not +0"
        parts_copy = ws.t.clone()
        gr.buf.t.zero_()
        ref = _lib.SlabRef()
        ref.workspace, ref.g_w, ref.batch, ref.out_features, ref.in_features, ref.splits = ws.ptr(), gr.buf.ptr(), 1, 1, n, parts
        _lib.check(lib.dfm_linear_backward_finish((_lib.SlabRef * 1)(ref), 1, _st()))
        torch.cuda.synchronize()
        assert gr.buf.guards_intact()
        return parts_copy, gr.buf.t.clone()

    runs = dict(plain=launch(0, True, False), null=launch(1, True, False), fm_field=launch(1, True, True),
                fm_only=launch(1, False, True))
    assert _same_bits(runs["plain"][0], runs["null"][0]) and _same_bits(runs["plain"][1], runs["null"][1]), \
        "fold_fm with a NULL trio differs from the plain kernel"
    for mode, args in (("plain", (0, True, False)), ("fm_field", (1, True, True))):
        again = launch(*args)
        assert _same_bits(again[0], runs[mode][0]) and _same_bits(again[1], runs[mode][1]), f"{mode}: two runs differ bitwise"
    for mode in R.BWD_MODES:
        flat = H.npy(runs[mode][1])
        _compare_grads(name, mode, case, lambda k: gr.get(flat, k), R.backward_ref(name, mode))


# ----------------------------------------------------------------------------- the documented refusals
@pytest.mark.parametrize("name", R.REFUSALS)
def test_refusals_launch_nothing(name):
    case, inp = R.CASES[name], R.inputs(name)
    B, F, D, T = case.B, case.F, case.D, case.T
    lib = _lib.load()
    emb, rec = _emb(case, inp), _record(case, inp)
    plan = emb._ensure_plan(torch.device("cuda"))
    out = dict(fo=H.GuardedBuffer(B), fe=H.GuardedBuffer(B * F * D), flat=H.GuardedBuffer(B * T), fm=H.GuardedBuffer(B),
               S=H.GuardedBuffer(B * D))
    rc = lib.dfm_embedding_forward_record(plan, C.c_void_p(rec.data_ptr()), B, out["fo"].ptr(), out["fe"].ptr(),
                                          out["flat"].ptr(), T, out["fm"].ptr(), out["S"].ptr(), None, emb._err.data_ptr(), _st())
    torch.cuda.synchronize()
    if case.fwd:
        assert rc == 0
    else:
        assert rc == _lib.ERR_UNSUPPORTED, lib.dfm_last_error()
        assert all(_is_nan_pattern(g.t) for g in out.values()), "a refused gather wrote"
    gr = _Grads(emb)
    parts = lib.dfm_embedding_backward_record_parts(B)
    ws = H.GuardedBuffer(parts * gr.n)
    sv = R.saved_f32(name)
    dev = {k: H.GuardedBuffer.of(v) for k, v in dict(g_first=inp["g_first"], g_field=inp["g_field"], g_flat=inp["g_flat"],
                                                     flat=sv["flat_embeddings"]).items()}
    assert not case.bwd
    rc = lib.dfm_embedding_backward_record(plan, C.c_void_p(rec.data_ptr()), B, dev["g_first"].ptr(), dev["g_field"].ptr(),
                                           dev["g_flat"].ptr(), T, dev["flat"].ptr(), T, None, None, None, 0,
                                           emb._grad_struct(gr.views), gr.buf.ptr(), gr.n, ws.ptr(), _st())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED, lib.dfm_last_error()
    assert _is_nan_pattern(ws.t) and ws.guards_intact(), "a refused backward wrote"


# ----------------------------------------------------------------------------- the dense-autograd path
@pytest.mark.parametrize("name", R.DENSE_CASES)
def test_dense_autograd_kernels(name):
    """emb_fwd_general + first_order_sum, then dfm_embedding_backward_dense (atomics), on the same cases with the same
    reference and bars; fm_embed_dim 12 and 20, a width of 6 and max bags (first maximum wins) included."""
    case, inp, ref = R.CASES[name], R.inputs(name), R.forward_ref(name)
    B, F, D, T = case.B, case.F, case.D, case.T
    lib = _lib.load()
    emb = _emb(case, inp)
    plan = emb._ensure_plan(torch.device("cuda"))
    inputs = [torch.from_numpy(np.ascontiguousarray(inp["batch"][f["name"]])).cuda() for f in case.fields]
    out = dict(fo=H.GuardedBuffer(B), fe=H.GuardedBuffer(B * F * D), flat=H.GuardedBuffer(B * T), ws=H.GuardedBuffer(B * F))
    _lib.check(lib.dfm_embedding_forward(plan, emb._ptr_array(inputs), B, out["fo"].ptr(), out["fe"].ptr(), out["flat"].ptr(),
                                         None, None, out["ws"].ptr(), emb._err.data_ptr(), _st()))
    torch.cuda.synchronize()
    emb.raise_on_bad_index()
    assert all(g.guards_intact() for g in out.values())
    got = dict(first_order=H.npy(out["fo"].t), field_embeddings=H.npy(out["fe"].view(B, F, D)),
               flat_embeddings=H.npy(out["flat"].view(B, T)))
    _check_forward(name, got, ref, ("first_order", "field_embeddings", "flat_embeddings"))
    _sparse_bits(case, inp, got["flat_embeddings"], got["field_embeddings"])

    want = R.backward_ref(name, "plain")
    sv = R.saved_f32(name)
    named = dict(emb.named_parameters())
    bufs = {k: H.GuardedBuffer(p.numel(), 0.0) for k, p in named.items()}
    views = {id(named[k]): b.t.view_as(named[k]) for k, b in bufs.items()}
    dev = {k: H.GuardedBuffer.of(v) for k, v in dict(g_first=inp["g_first"], g_field=inp["g_field"], g_flat=inp["g_flat"],
                                                     flat=sv["flat_embeddings"]).items()}
    _lib.check(lib.dfm_embedding_backward_dense(plan, emb._ptr_array(inputs), B, dev["g_first"].ptr(), dev["g_field"].ptr(),
                                                dev["g_flat"].ptr(), emb._grad_struct(views), dev["flat"].ptr(), _st()))
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in bufs.values()) and all(b.guards_intact() for b in dev.values())
    _compare_grads(name, "dense-path", case, lambda k: H.npy(bufs[k].t), want)
    for k, free in _unnamed_rows(case, inp).items():
        rows = H.npy(bufs[k].t).reshape(len(free), -1)[free]
        assert not rows.any(), f"{k}: a row nobody names is not 0"
