"""GPU tests of the fused mixed-schema steps for xDeepFM and AttentionDeepFM (``training/mixed_step.py``) and of the
two kernels under them (``dfm_embedding_forward_record`` with ``d_fm_sum``, ``dfm_embedding_backward_record`` with ``fold_fm``).

1. against REFERENCE train-step vectors on the MovieLens schema (``tools/make_mixed_train_golden.py``), eager, as a
   graph, and as a graph fed from a device ring: logits, loss, total norm, clip coefficient, every parameter after
   every step (``adam_param_bound``; rows no sample names: within 1e-3 of one Adam step and moved, the bar of
   tests/test_gpu_mixed_train.py) and the final Adam moments;
2. against the dense autograd path + torch optimizers, live at B = 512, same bars, at the configuration defaults of
   the interaction layers' shapes (attention: one block, 4 heads over dim 64; measured worst logit error over the
   three steps: 0.20 of ``assert_close``'s bound under Adam / AdamW, 0.005 under SGD; xDeepFM 0.085 / 0.003).  A
   first draft of this test used two blocks over dim 32: SGD passed all three steps and Adam / AdamW the first step
   whole, but their step-1 logits sat at 2.6 x the bound (2.2e-4 against 8.4e-5, 31 of 512 samples) — two fp32
   trajectories one Adam step at lr 1e-2 apart, not a single-step error; the two-block stack is held to the reference's
   own trajectory in 1. (``_l2clip``: lr 1e-2, Adam, every parameter after every step);
3. the kernels alone through the C ABI: S against fe.sum(1) with every other output bit-equal to the existing gather;
   the folded backward against ``dfm_fm_backward`` followed by ``dfm_embedding_backward_record`` (bit-equal: the
   product g (S - e) is rounded before it is added, and S is summed in the field order ``fm_bwd_kernel`` uses), against
   that composition with another gradient already in d fe (``assert_close``), bit-equal to the existing entry with the
   trio NULL, and NaN guard bands around every buffer it writes stay NaN;
4. bitwise: graph == eager, run == run, checkpoint -> resume;
5. learning-rate changes between launches; bad ids raise IndexError.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_close, cfg_of, error_ratio, fields_of, group, npy
from tests.test_cpu_mixed_models_train import CASES, load_case
from tests.test_gpu_mixed_train import (OPTS, _check_params, _check_untouched, _dev, _kernel_case, _model, _movielens,
                                        _records, _state)
from tests.test_oracle_golden import adam_param_bound, assert_adam_moments, zero_grad_param

pytestmark = pytest.mark.gpu

KINDS = {"xdeepfm": ("FusedMixedXDeepFMStep", dict(cin_sizes=[16, 8], cin_split=True)),
         "attention_deepfm": ("FusedMixedAttentionDeepFMStep", dict(heads=4, A=64, layers=1, residual=True))}


# ----------------------------------------------------------------------------- 1. reference vectors
@pytest.mark.parametrize("impl", ["eager", "graph", "ring"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_vs_reference(case, impl):
    import deepfm_amd.training as T
    from deepfm_amd.data.packed import DeviceBatchRing, PackedBatchLoader, PackedColumns
    from deepfm_amd.training.fused_step import fused_step_class
    g = load_case(case)
    fields, steps = fields_of(g), int(g["steps"])
    lr, l2, clip = float(g["lr"]), float(g["l2"]), float(g["clip"])
    init = group(g, "init/")
    model = _model(fields, cfg_of(g), init, l2)
    cls = getattr(T, KINDS[CASES[case]][0])
    assert fused_step_class(model) is cls and T.mixed_step_class(model) is cls
    opt = T.DenseTableAdam(model, lr=lr, l2=l2, max_grad_norm=clip)
    B = g["step0/labels"].shape[0]
    step = cls(model, opt, B, use_graph=impl != "eager")
    if step.use_graph:
        step.capture()
        for k, v in _state(model).items():
            assert np.array_equal(v, init[k]), f"capture() changed {k}"
    if impl == "ring":
        feats = {f["name"]: np.concatenate([g[f"step{t}/batch/{f['name']}"] for t in range(steps)]) for f in fields}
        labels = np.concatenate([g[f"step{t}/labels"] for t in range(steps)])
        loader = PackedBatchLoader(PackedColumns(model.schema, feats, labels), B, shuffle=False)
        records = iter(DeviceBatchRing(loader, torch.device("cuda"), depth=2))
    free = {k: v for k, v in group(g, "untouched/").items()}
    for t in range(steps):
        if impl == "ring":
            step.run_from(next(records))
        else:
            step.run_from(step.pack_record(_dev(group(g, f"step{t}/batch/")), torch.from_numpy(g[f"step{t}/labels"]).cuda()))
        model.embedding.raise_on_bad_index()
        assert_close(npy(step.logits), g[f"step{t}/logits"], what=f"{impl} logits {t}")
        bce = float(g[f"step{t}/bce"])
        print(f"{case} {impl} step {t}: loss {float(step.loss):.7f} / {bce:.7f}  norm {step.total_norm():.7f} / "
              f"{float(g[f'step{t}/grad_norm']):.7f}")
        assert abs(float(step.loss) - bce) < 1e-4 * bce, (t, float(step.loss), bce)
        norm = float(g[f"step{t}/grad_norm"])
        assert abs(step.total_norm() - norm) < 1e-4 * norm, (t, step.total_norm(), norm)
        assert abs(float(opt.clip_coef) - min(1.0, clip / (norm + 1e-6))) < 1e-4
        got, ref = _state(model), group(g, f"step{t}/param/")
        _check_params(got, ref, lambda k: None if zero_grad_param(k, g) else adam_param_bound(g, t, k, lr), f"{impl} step {t}")
        _check_untouched(got, ref, init, free, lr, f"{case} {impl} step {t}")
    osd = opt.state_dict()
    assert osd["step"] == steps
    assert_adam_moments(lambda kind, k: npy(osd["state"][k]["exp_avg" if kind == "m" else "exp_avg_sq"]), g, impl)


# ----------------------------------------------------------------------------- 2. the dense autograd path, live
@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
@pytest.mark.parametrize("model_kind", sorted(KINDS))
def test_steps_vs_dense_autograd_path(model_kind, kind):
    import deepfm_amd.training as T
    B, lr, l2, clip = 512, 1e-2, 1e-3, 0.5
    g, fields, batches = _movielens(B, 5)
    c = dict(kind=model_kind, fm_dim=16, hidden_units=[64, 32], **KINDS[model_kind][1])
    gl_cfg = np.array(__import__("json").dumps(c))
    ref = _model(fields, c, None, l2, seed=3)
    init = _state(ref)
    model = _model(fields, c, init, l2)
    cls_name, torch_cls, kw = OPTS[kind]
    topt = torch_cls(ref.parameters(), lr=lr, **kw)
    opt = getattr(T, cls_name)(model, lr=lr, l2=l2, max_grad_norm=clip)
    step = getattr(T, KINDS[model_kind][0])(model, opt, B, use_graph=True)
    step.capture()
    free = {f["name"]: np.arange(f["vocab"]) >= max(2, int(0.6 * f["vocab"])) for f in fields if f["type"] != "dense"}
    grads, norms = [], []
    for t, (b, labels) in enumerate(batches):
        lab = torch.from_numpy(labels).cuda()
        logits = ref(_dev(b)).squeeze(1)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, lab) + ref.get_l2_reg_loss()
        topt.zero_grad()
        loss.backward()
        grads.append({k: npy(p.grad) for k, p in ref.named_parameters()})
        norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)))
        topt.step()
        step.run_from(step.pack_record(_dev(b), lab))
        model.embedding.raise_on_bad_index()
        print(f"{model_kind} {kind} step {t}: logits worst |err| / bound {error_ratio(npy(step.logits), npy(logits)):.3f}")
        assert_close(npy(step.logits), npy(logits), what=f"{kind} logits {t}")
        print(f"{model_kind} {kind} step {t}: norm {step.total_norm():.7f} / {norms[t]:.7f}")
        assert abs(step.total_norm() - norms[t]) < 1e-4 * norms[t], (t, step.total_norm(), norms[t])
        assert abs(float(opt.clip_coef) - min(1.0, clip / (norms[t] + 1e-6))) < 1e-4
        gl = {"clip": clip, **{f"step{u}/grad_norm": norms[u] for u in range(t + 1)}}
        for u in range(t + 1):
            gl.update({f"step{u}/grad/{k}": v for k, v in grads[u].items()})
        gl["cfg"] = gl_cfg
        got, want = _state(model), _state(ref)
        _check_params(got, want, lambda k: None if zero_grad_param(k, gl) else adam_param_bound(gl, t, k, lr),
                      f"{model_kind} {kind} step {t}")
        _check_untouched(got, want, init, free, lr, f"{model_kind} {kind} step {t}")


# ----------------------------------------------------------------------------- 3. the kernels alone
GUARD = 64          # floats of NaN on both sides of every output


def _guarded(shape, dev="cuda"):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


@pytest.mark.parametrize("B", [1, 7, 4096, 4097])
@pytest.mark.parametrize("combiner", ["mean", "sum"])
def test_gather_emits_fm_sum_and_keeps_every_other_bit(combiner, B):
    _lib, emb, fields, batch, rec, *_ = _kernel_case(combiner, B, 5 + B)
    F, D, T = len(fields), 16, sum(f["dim"] for f in fields)
    ld = T + 8                                  # a row stride wider than the row: the gap must stay NaN

    def run(with_sum):
        bufs = {k: _guarded(s) for k, s in dict(fo=(B, 1), fe=(B, F, D), flat=(B, ld), fm=(B,), lab=(B,),
                                                 S=(B, D)).items()}
        v = {k: b[1] for k, b in bufs.items()}
        emb.forward_record(rec.data_ptr(), B, v["fo"], v["fe"], v["flat"].data_ptr(), ld, v["fm"], v["lab"],
                           fm_sum=v["S"] if with_sum else None)
        torch.cuda.synchronize()
        return bufs, v

    b0, old = run(False)
    b1, new = run(True)
    emb.raise_on_bad_index()
    for k in ("fo", "fe", "fm", "lab"):
        assert torch.equal(old[k], new[k]), f"{k} changed bits"
    assert torch.equal(old["flat"][:, :T], new["flat"][:, :T]) and torch.isnan(new["flat"][:, T:]).all()
    assert torch.isnan(old["S"]).all(), "the existing entry wrote S"
    for k, (buf, _) in b1.items():
        assert _guards_intact(buf), f"{k}: guard band written"
    # S: the sum over the fields in order f = 0 .. F-1 (bit for bit), and fe.sum(1) to rounding
    want = torch.zeros(B, D, device="cuda")
    for f in range(F):
        want = want + new["fe"][:, f, :]
    assert torch.equal(new["S"], want)
    assert_close(npy(new["S"]), npy(new["fe"].double().sum(1)), what="S")


def _flat_views(emb, dev):
    params = list(emb.parameters())
    pad = lambda n: (n + 15) // 16 * 16
    n = sum(pad(p.numel()) for p in params)
    buf, flat_grad = _guarded((n,), dev)
    assert flat_grad.data_ptr() % 64 == 0
    views, off = {}, 0
    for p in params:
        views[id(p)] = flat_grad[off:off + p.numel()].view_as(p)
        off += pad(p.numel())
    return buf, flat_grad, views, n


@pytest.mark.parametrize("B", [1, 7, 4096, 4097])
@pytest.mark.parametrize("combiner", ["mean", "sum"])
def test_folded_backward_vs_fm_backward_then_record_backward(combiner, B):
    _lib, emb, fields, batch, rec, g_first, g_field, g_flat = _kernel_case(combiner, B, 11 + B)
    lib, st, dev = _lib.load(), _lib.stream_handle, torch.device("cuda")
    F, D, T = len(fields), 16, g_flat.shape[1]
    fo, fe, flat = torch.empty(B, 1, device=dev), torch.empty(B, F, D, device=dev), torch.empty(B, T, device=dev)
    S, fm, g_fm = torch.empty(B, D, device=dev), torch.empty(B, device=dev), g_first[:, 0].contiguous() * 0.37
    emb.forward_record(rec.data_ptr(), B, fo, fe, flat.data_ptr(), T, fm, None, fm_sum=S)
    plan = emb._ensure_plan(dev)
    buf, flat_grad, views, n = _flat_views(emb, dev)
    parts = lib.dfm_embedding_backward_record_parts(B)
    ws_buf, ws = _guarded((parts * n,), dev)
    grads = emb._grad_struct(views)

    def finish():
        flat_grad.zero_()
        ref = _lib.SlabRef()
        ref.workspace, ref.g_w, ref.batch, ref.out_features, ref.in_features, ref.splits = \
            ws.data_ptr(), flat_grad.data_ptr(), 1, 1, n, parts
        _lib.check(lib.dfm_linear_backward_finish((_lib.SlabRef * 1)(ref), 1, st()))
        torch.cuda.synchronize()
        return flat_grad.clone(), ws.clone()

    def old(gf):
        ws.zero_()
        _lib.check(lib.dfm_embedding_backward_record(plan, C.c_void_p(rec.data_ptr()), B, g_first.data_ptr(),
                                                     gf.data_ptr(), g_flat.data_ptr(), T, flat.data_ptr(), T, None,
                                                     None, None, 0, grads, flat_grad.data_ptr(), n, ws.data_ptr(), st()))
        return finish()

    def new(gf, trio):
        ws.zero_()
        _lib.check(lib.dfm_embedding_backward_record(
            plan, C.c_void_p(rec.data_ptr()), B, g_first.data_ptr(), None if gf is None else gf.data_ptr(),
            g_flat.data_ptr(), T, flat.data_ptr(), T, *((g_fm.data_ptr(), S.data_ptr(), fe.data_ptr()) if trio else (None,) * 3),
            1, grads, flat_grad.data_ptr(), n, ws.data_ptr(), st()))
        return finish()

    # (a) the trio NULL: the fold_fm == 0 call, bit for bit (slices included)
    a_old, a_new = old(g_field), new(g_field, False)
    assert torch.equal(a_old[0], a_new[0]) and torch.equal(a_old[1], a_new[1])
    # (b) d_g_field NULL + the trio: dfm_fm_backward into a buffer, then the existing entry on it, bit for bit
    g_fe = torch.empty(B, F, D, device=dev)
    _lib.check(lib.dfm_fm_backward(fe.data_ptr(), g_fm.data_ptr(), B, F, D, g_fe.data_ptr(), st()))
    b_old, b_new = old(g_fe), new(None, True)
    assert torch.equal(b_old[0], b_new[0]) and torch.equal(b_old[1], b_new[1])
    assert torch.equal(new(None, True)[0], b_new[0]), "two runs differ bitwise"
    # (c) both: the FM term added to another gradient of fe (torch's add rounds the same way; held to assert_close and
    # reported when it is bit-equal)
    c_old, c_new = old(g_field + g_fe), new(g_field, True)
    named = dict(emb.named_parameters())
    for k, p in named.items():
        lo = views[id(p)].data_ptr() - flat_grad.data_ptr()
        sl = slice(lo // 4, lo // 4 + p.numel())
        assert_close(npy(c_new[0][sl]), npy(c_old[0][sl]), what=f"{combiner} B={B} {k}")
    print(f"{combiner} B={B}: g_field + trio bit-equal to the composition: {torch.equal(c_old[0], c_new[0])}")
    # neither g_field nor the trio: the effective field gradient is 0 -> what g_flat and g_first alone give
    z = new(None, False)
    assert torch.equal(z[0], old(torch.zeros(B, F, D, device=dev))[0])
    # guard bands, and rows nobody names stay exactly 0
    assert _guards_intact(buf) and _guards_intact(ws_buf)
    for f in fields:
        if f["type"] == "dense":
            continue
        ids = np.unique(batch[f["name"]])
        free = np.ones(f["vocab"], bool)
        free[ids[(ids > 0) & (ids < f["vocab"])]] = False
        for order in ("second", "first"):
            p = named[f"{order}_order_embeddings.{f['name']}.weight"]
            lo = (views[id(p)].data_ptr() - flat_grad.data_ptr()) // 4
            gr = npy(c_new[0][lo:lo + p.numel()].view_as(p))
            assert (gr[free] == 0.0).all(), f"{f['name']}: a row nobody names is not exactly 0"
    # the trio comes whole or not at all
    rc = lib.dfm_embedding_backward_record(plan, C.c_void_p(rec.data_ptr()), B, g_first.data_ptr(), None,
                                           g_flat.data_ptr(), T, flat.data_ptr(), T, g_fm.data_ptr(), None, None,
                                           1, grads, flat_grad.data_ptr(), n, ws.data_ptr(), st())
    assert rc != 0


# ----------------------------------------------------------------------------- 4. bitwise
def _fresh(model_kind, kind="adam", B=512, use_graph=True, seed=9):
    import deepfm_amd.training as T
    g, fields, _ = _movielens(8, 1)
    c = dict(kind=model_kind, fm_dim=16, hidden_units=[64, 32], **KINDS[model_kind][1])
    model = _model(fields, c, None, 1e-3, seed=seed)
    model.dnn.mlp[3].p = 0.1                     # dropout on: the seed is part of the state
    opt = getattr(T, OPTS[kind][0])(model, lr=1e-2, l2=1e-3, max_grad_norm=0.5)
    step = getattr(T, KINDS[model_kind][0])(model, opt, B, use_graph=use_graph)
    return model, opt, step


@pytest.mark.parametrize("model_kind", sorted(KINDS))
def test_graph_equals_eager_and_runs_repeat_bitwise(model_kind):
    B = 512
    finals = []
    for mode in ("eager", "graph", "graph", "group"):
        model, opt, step = _fresh(model_kind, B=B, use_graph=mode != "eager")
        seed0 = step.seed.clone()
        recs = _records(step, B, 4, 21)
        if mode != "eager":
            before = [t.clone() for t in step._mutable_state()]
            step.capture(steps_per_graph=2 if mode == "group" else 1)
            for a, b in zip(before, step._mutable_state()):
                assert torch.equal(a, b), "capture() changed training state"
            assert torch.equal(step.seed, seed0) and int(opt.step_count) == 0
        if mode == "group":
            step.run_group(recs[:2]); step.run_group(recs[2:])
        else:
            for r in recs:
                step.run_from(r)
        torch.cuda.synchronize()
        finals.append([opt.flat_param.clone(), opt.flat_m.clone(), opt.flat_v.clone(), step.loss.clone()])
    for other in finals[1:]:
        for a, b in zip(finals[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("model_kind", sorted(KINDS))
def test_checkpoint_resume_is_bitwise(model_kind, tmp_path):
    from deepfm_amd.utils.io import load_checkpoint, save_checkpoint
    B = 256
    model, opt, step = _fresh(model_kind, B=B)
    step.capture()
    recs = _records(step, B, 4, 33)
    for r in recs[:2]:
        step.run_from(r)
    path = os.path.join(tmp_path, "ck.pt")
    save_checkpoint({"epoch": 0, "model_state_dict": model.state_dict(), "optimizer_state_dict": opt.state_dict(),
                     "best_metric": 0.0, "seed": step.seed.clone()}, path)
    for r in recs[2:]:
        step.run_from(r)
    torch.cuda.synchronize()
    want = opt.flat_param.clone()
    model2, opt2, step2 = _fresh(model_kind, B=B, seed=77)
    ck = load_checkpoint(path, device="cuda")
    model2.load_state_dict(ck["model_state_dict"])
    opt2.load_state_dict(ck["optimizer_state_dict"])
    step2.seed.copy_(ck["seed"])
    step2.capture()
    for r in _records(step2, B, 4, 33)[2:]:
        step2.run_from(r)
    torch.cuda.synchronize()
    assert torch.equal(opt2.flat_param, want)


# ----------------------------------------------------------------------------- 5. learning rate, bad ids
@pytest.mark.parametrize("model_kind", sorted(KINDS))
def test_lr_change_takes_effect_at_next_launch_and_bad_id_raises(model_kind):
    B = 256
    outs = []
    for change in (False, True):
        model, opt, step = _fresh(model_kind, kind="sgd", B=B)
        step.capture()
        recs = _records(step, B, 2, 41)
        step.run_from(recs[0])
        p1 = opt.flat_param.clone()
        if change:
            opt.lr = 0.0
        step.run_from(recs[1])
        torch.cuda.synchronize()
        outs.append((p1, opt.flat_param.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert not torch.equal(outs[0][1], outs[0][0])          # lr 1e-2: the second step moved
    assert torch.equal(outs[1][1], outs[1][0])              # lr 0 from the second launch on: it did not
    model, opt, step = _fresh(model_kind, B=B)
    rec = _records(step, B, 1, 43)[0]
    from deepfm_amd.data.packed import RecordLayout
    views, _ = RecordLayout.of(model.schema, B).unpack(rec)
    views["gender"][5] = 3                                   # vocabulary size 3: out of range
    step.run_from(rec)
    with pytest.raises(IndexError):
        model.embedding.raise_on_bad_index()
