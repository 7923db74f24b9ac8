"""GPU tests of the fused mixed-schema training step (``training/mixed_step.py``, ``dfm_embedding_backward_record``,
the dense-table optimizers).

1. against REFERENCE train-step vectors on the MovieLens schema (``tools/make_mixed_train_golden.py``), eager, as a
   graph, and as a graph fed from a device ring.  Rows no sample of any step names get a bar of their own:
   ``adam_param_bound`` opens to its cap where a row's gradient is the small L2 term alone, so it would let a LAZY
   implementation (the row does not move) pass; there the gradient is 2 lambda w times the clip coefficient, which
   this step computes to rounding, so those rows are held to the reference within 1e-3 of one Adam step (1e-3 * lr,
   the bar tests/test_gpu_fullsize.py puts on Adam's formula) and must have moved;
2. against the existing dense autograd path + torch optimizers, live at B = 4096, same bars;
3. the backward kernel alone against ``dfm_embedding_backward_dense``;
4. bitwise: graph == eager, run == run, capture() side-effect free, checkpoint -> resume;
5. learning-rate changes between launches; bad ids raise IndexError.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_close, cfg_of, fields_of, group, load, load_params, npy, schema_from_fields
from tests.test_gpu_models_step import _config
from tests.test_oracle_golden import adam_param_bound, assert_adam_moments, zero_grad_param

pytestmark = pytest.mark.gpu

CASES = ["train_steps_deepfm_movielens", "train_steps_deepfm_movielens_l2clip"]
OPTS = {"adam": ("DenseTableAdam", torch.optim.Adam, {}), "adamw": ("DenseTableAdamW", torch.optim.AdamW, {}),
        "sgd": ("DenseTableSGD", torch.optim.SGD, {"momentum": 0.9})}


def _model(fields, c, params=None, l2=0.0, seed=0):
    from deepfm_amd.models import create_model
    torch.manual_seed(seed)
    model = create_model(c["kind"], schema_from_fields(fields), _config(c))
    if params is not None:
        assert sorted(model.state_dict().keys()) == sorted(params.keys())
        load_params(model, params)
    model = model.cuda()
    model.config.feature.embedding_l2_reg = l2
    model.embedding.strict_indices = True
    return model.train()


def _state(model):
    return {k: npy(v) for k, v in model.state_dict().items()}


def _dev(batch):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}


def _check_params(got, want, bound_of, what):
    """Every element of every parameter inside rtol 1e-4 + bound_of(key); nothing masked."""
    for k, w in want.items():
        if "running_" in k or k.endswith("num_batches_tracked"):
            continue
        b = bound_of(k)
        if b is None:
            continue
        err = np.abs(got[k].astype(np.float64) - w.astype(np.float64))
        bad = err > 1e-4 * np.abs(w.astype(np.float64)) + b
        assert not bad.any(), f"{what} {k}: {bad.sum()} / {bad.size} out; worst |err| {err.max():.3e}"


def _check_untouched(got, ref, init, free, lr, what):
    """Rows no sample names: within 1e-3 * lr of the reference, and moved at all."""
    for name, mask in free.items():
        for order in ("second", "first"):
            k = f"embedding.{order}_order_embeddings.{name}.weight"
            err = np.abs(got[k][mask].astype(np.float64) - ref[k][mask].astype(np.float64))
            print(f"{what} untouched {k}: rows {int(mask.sum())} max |err| {err.max():.3e} bar {1e-3 * lr:.1e}")
            assert err.max() <= 1e-3 * lr, f"{what} {k}: untouched rows off by {err.max():.3e} > {1e-3 * lr:.1e}"
            assert (np.abs(got[k][mask] - init[k][mask]) > 0).all(), f"{what} {k}: an untouched row did not move (lazy?)"


# ----------------------------------------------------------------------------- 1. reference vectors
@pytest.mark.parametrize("impl", ["eager", "graph", "ring"])
@pytest.mark.parametrize("case", CASES)
def test_steps_vs_reference(case, impl):
    from deepfm_amd.data.packed import DeviceBatchRing, PackedBatchLoader, PackedColumns
    from deepfm_amd.training import DenseTableAdam, FusedMixedDeepFMStep
    from deepfm_amd.training.fused_step import fused_step_class
    g = load(case)
    fields, steps = fields_of(g), int(g["steps"])
    lr, l2, clip = float(g["lr"]), float(g["l2"]), float(g["clip"])
    init = group(g, "init/")
    model = _model(fields, cfg_of(g), init, l2)
    assert fused_step_class(model) is FusedMixedDeepFMStep
    opt = DenseTableAdam(model, lr=lr, l2=l2, max_grad_norm=clip)
    B = g["step0/labels"].shape[0]
    step = FusedMixedDeepFMStep(model, opt, B, use_graph=impl != "eager")
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
def _movielens(B, seed):
    from deepfm_amd.data.synthetic import random_fields_batch
    g = load("model_deepfm_movielens")
    fields = fields_of(g)
    rng = np.random.default_rng(seed)
    batches = []
    for _ in range(3):
        b = random_fields_batch(fields, B, rng, zero_frac=0.05)
        for f in fields:                       # ids from the lower 60 % of every table: the rest stays untouched
            if f["type"] != "dense":
                b[f["name"]] = np.where(b[f["name"]] >= max(2, int(0.6 * f["vocab"])), 1, b[f["name"]])
        b["genres"][:7] = 0                    # empty bags
        batches.append((b, (rng.random(B) < 0.3).astype(np.float32)))
    return g, fields, batches


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_steps_vs_dense_autograd_path(kind):
    import deepfm_amd.training as T
    B, lr, l2, clip = 4096, 1e-2, 1e-3, 0.5
    g, fields, batches = _movielens(B, 5)
    c = dict(cfg_of(g), hidden_units=[64, 32])
    ref = _model(fields, c, None, l2, seed=3)
    init = _state(ref)
    model = _model(fields, c, init, l2)
    cls_name, torch_cls, kw = OPTS[kind]
    topt = torch_cls(ref.parameters(), lr=lr, **kw)
    opt = getattr(T, cls_name)(model, lr=lr, l2=l2, max_grad_norm=clip)
    step = T.FusedMixedDeepFMStep(model, opt, B, use_graph=True)
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
        assert_close(npy(step.logits), npy(logits), what=f"{kind} logits {t}")
        assert abs(step.total_norm() - norms[t]) < 1e-4 * norms[t], (t, step.total_norm(), norms[t])
        assert abs(float(opt.clip_coef) - min(1.0, clip / (norms[t] + 1e-6))) < 1e-4
        # adam_param_bound over the live path's own gradients (the keys it reads, as a golden would hold them)
        gl = {"clip": clip, **{f"step{u}/grad_norm": norms[u] for u in range(t + 1)}}
        for u in range(t + 1):
            gl.update({f"step{u}/grad/{k}": v for k, v in grads[u].items()})
        gl["cfg"] = g["cfg"]
        got, want = _state(model), _state(ref)
        _check_params(got, want, lambda k: None if zero_grad_param(k, gl) else adam_param_bound(gl, t, k, lr), f"{kind} step {t}")
        _check_untouched(got, want, init, free, lr, f"{kind} step {t}")


# ----------------------------------------------------------------------------- 3. the kernel alone
def _kernel_case(combiner, B, seed):
    from deepfm_amd import _lib
    from deepfm_amd.data.packed import RecordLayout
    from deepfm_amd.models.layers.embedding import FeatureEmbedding
    fields = [dict(name="u", type="sparse", vocab=700, dim=16, max_len=1, combiner="mean"),
              dict(name="s", type="sparse", vocab=9, dim=4, max_len=1, combiner="mean"),
              dict(name="one", type="sparse", vocab=5, dim=8, max_len=1, combiner="mean"),
              dict(name="g", type="sequence", vocab=20, dim=8, max_len=6, combiner=combiner),
              dict(name="x", type="dense", vocab=0, dim=4, max_len=1, combiner="mean"),
              dict(name="y", type="dense", vocab=0, dim=16, max_len=1, combiner="mean")]
    schema = schema_from_fields(fields)
    torch.manual_seed(seed)
    emb = FeatureEmbedding(schema, 16).cuda()
    rng = np.random.default_rng(seed)
    batch = {"u": rng.integers(0, 600, B), "s": rng.integers(0, 9, B), "one": np.full(B, 3),
             "g": rng.integers(0, 20, (B, 6)), "x": rng.random(B).astype(np.float32),
             "y": rng.random(B).astype(np.float32)}
    batch["u"][0] = 699                        # the maximum id
    batch["u"][B // 2] = 0                     # id 0
    batch["g"][0] = 0                          # an empty bag
    batch["g"][B - 1, 2:] = 0                  # a short one
    batch = {k: np.ascontiguousarray(v) for k, v in batch.items()}
    lay = RecordLayout.of(schema, B)
    rec = torch.zeros(lay.record_bytes, dtype=torch.uint8, device="cuda")
    views, _ = lay.unpack(rec)
    for k, dst in views.items():
        dst.copy_(torch.from_numpy(batch[k]).to(dst.dtype))
    F, D, T = len(fields), 16, schema.total_embedding_dim
    gen = torch.Generator(device="cuda").manual_seed(seed)
    g_first = torch.randn(B, 1, device="cuda", generator=gen)
    g_field = torch.randn(B, F, D, device="cuda", generator=gen)
    g_flat = torch.randn(B, T, device="cuda", generator=gen)
    return _lib, emb, fields, batch, rec, g_first, g_field, g_flat


@pytest.mark.parametrize("B", [1, 7, 4096, 4097])
@pytest.mark.parametrize("combiner", ["mean", "sum"])
def test_backward_kernel_vs_dense_backward(combiner, B):
    _lib, emb, fields, batch, rec, g_first, g_field, g_flat = _kernel_case(combiner, B, 11 + B)
    lib = _lib.load()
    dev = torch.device("cuda")
    inputs, _ = emb._gather_inputs(_dev(batch))
    fo, fe, flat, _ = emb._launch_forward(inputs, B)
    # reference: the atomic dense backward
    want = {id(p): torch.zeros_like(p) for p in emb.parameters()}
    plan = emb._ensure_plan(dev)
    _lib.check(lib.dfm_embedding_backward_dense(plan, emb._ptr_array(inputs), B, g_first.data_ptr(), g_field.data_ptr(),
                                                g_flat.data_ptr(), emb._grad_struct(want), flat.data_ptr(),
                                                _lib.stream_handle()))
    # the record backward into a flat buffer of 64-byte aligned views
    params = list(emb.parameters())
    pad = lambda n: (n + 15) // 16 * 16
    n = sum(pad(p.numel()) for p in params)
    flat_grad = torch.zeros(n, device=dev)
    got, off = {}, 0
    for p in params:
        got[id(p)] = flat_grad[off:off + p.numel()].view_as(p)
        off += pad(p.numel())
    parts = lib.dfm_embedding_backward_record_parts(B)
    assert lib.dfm_embedding_backward_record_workspace_bytes(B, n) == 4 * parts * n
    ws = torch.zeros(parts * n, device=dev)
    runs = []
    for _ in range(2):
        flat_grad.zero_()
        _lib.check(lib.dfm_embedding_backward_record(plan, C.c_void_p(rec.data_ptr()), B, g_first.data_ptr(),
                                                     g_field.data_ptr(), g_flat.data_ptr(), g_flat.shape[1],
                                                     flat.data_ptr(), flat.shape[1], None, None, None, 0,
                                                     emb._grad_struct(got), flat_grad.data_ptr(), n, ws.data_ptr(),
                                                     _lib.stream_handle()))
        ref = _lib.SlabRef()
        ref.workspace, ref.g_w, ref.batch, ref.out_features, ref.in_features, ref.splits = \
            ws.data_ptr(), flat_grad.data_ptr(), 1, 1, n, parts
        _lib.check(lib.dfm_linear_backward_finish((_lib.SlabRef * 1)(ref), 1, _lib.stream_handle()))
        runs.append(flat_grad.clone())
    assert torch.equal(runs[0], runs[1]), "two runs differ bitwise"
    named = dict(emb.named_parameters())
    for k, p in named.items():
        assert_close(npy(got[id(p)]), npy(want[id(p)]), what=f"{combiner} B={B} {k}")
    for f in fields:
        if f["type"] == "dense":
            continue
        ids = np.unique(batch[f["name"]])
        free = np.ones(f["vocab"], bool)
        free[ids[(ids > 0) & (ids < f["vocab"])]] = False
        for order in ("second", "first"):
            gr = npy(got[id(named[f"{order}_order_embeddings.{f['name']}.weight"])])
            assert (gr[free] == 0.0).all(), f"{f['name']}: a row nobody names is not exactly 0"


# ----------------------------------------------------------------------------- 4. bitwise
def _fresh(kind="adam", B=512, use_graph=True, steps_per_graph=1, seed=9):
    import deepfm_amd.training as T
    g, fields, _ = _movielens(8, 1)
    c = dict(cfg_of(g), hidden_units=[64, 32])
    model = _model(fields, c, None, 1e-3, seed=seed)
    model.dnn.mlp[3].p = 0.1                     # dropout on: the seed is part of the state
    opt = getattr(T, OPTS[kind][0])(model, lr=1e-2, l2=1e-3, max_grad_norm=0.5)
    step = T.FusedMixedDeepFMStep(model, opt, B, use_graph=use_graph)
    return model, opt, step


def _records(step, B, n, seed):
    from deepfm_amd.data.synthetic import random_fields_batch
    fields = fields_of(load("model_deepfm_movielens"))
    rng = np.random.default_rng(seed)
    return [step.pack_record(_dev(random_fields_batch(fields, B, rng, zero_frac=0.05)),
                             torch.from_numpy((rng.random(B) < 0.3).astype(np.float32)).cuda()) for _ in range(n)]


def _snapshot(model, opt, step):
    return [t.clone() for t in step._mutable_state()]


def test_graph_equals_eager_and_runs_repeat_bitwise():
    B = 512
    finals = []
    for mode in ("eager", "graph", "graph", "group"):
        model, opt, step = _fresh(B=B, use_graph=mode != "eager")
        seed0 = step.seed.clone()
        recs = _records(step, B, 4, 21)
        if mode != "eager":
            before = _snapshot(model, opt, step)
            step.capture(steps_per_graph=2 if mode == "group" else 1)
            for a, b in zip(before, _snapshot(model, opt, step)):
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


def test_checkpoint_resume_is_bitwise(tmp_path):
    from deepfm_amd.utils.io import load_checkpoint, save_checkpoint
    B = 256
    model, opt, step = _fresh(B=B)
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
    model2, opt2, step2 = _fresh(B=B, seed=77)
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
def test_lr_change_takes_effect_at_next_launch_and_bad_id_raises():
    B = 256
    outs = []
    for change in (False, True):
        model, opt, step = _fresh(kind="sgd", B=B)
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
    model, opt, step = _fresh(B=B)
    rec = _records(step, B, 1, 43)[0]
    from deepfm_amd.data.packed import RecordLayout
    views, _ = RecordLayout.of(model.schema, B).unpack(rec)
    views["gender"][5] = 3                                   # vocabulary size 3: out of range
    step.run_from(rec)
    with pytest.raises(IndexError):
        model.embedding.raise_on_bad_index()
