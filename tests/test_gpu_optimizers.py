"""GPU tests of the AdamW / SGD update rules and the device learning rate of the row-sparse step.

* Reference parity: every fixture of tests/optim_reference.py (torch.optim.AdamW / SGD(momentum=0.9) as
  trainer.py:67-78 builds them, and Adam with an LR change) through ``RowSparseTrainStep`` and the fused step of
  its model, eager and as a graph, packed and unpacked: parameters, logits and final optimizer state.
* LR changes between graph launches reach every capture flavour (look-ahead multi-step graphs, multi-step graphs
  without look-ahead, single-step graphs) bit-identically to the same schedule run eagerly.
* Checkpoints of torch's AdamW / SGD and of the package's own format continue bit-identically; other kinds are
  refused.
* Full size (V = 10^6, B = 4096): untouched rows do not move, touched rows follow the rule.
* The descriptor's node update refuses a node captured for another rule.
"""
import numpy as np
import pytest
import torch

from tests.helpers import cfg_of, group, load, npy
from tests.optim_reference import (ADAMW_CASES, LRSCHED_CASE, OPT_CASES, SGD_CASES, assert_rule_params,
                                   assert_rule_state, kind_of, step_lr)
from tests.test_gpu_models_step import _pool as _rand_pool, _small_deepfm
from tests.test_gpu_train_golden import _model, _pool, _state

pytestmark = pytest.mark.gpu

KINDS = ["adam", "adamw", "sgd"]


def _opt(kind, model, **kw):
    from deepfm_amd.training.rowsparse import OPTIMIZERS
    return OPTIMIZERS[kind](model, **kw)


def _opt_state_getter(opt):
    sd = opt.state_dict()["state"]
    return lambda slot, k: npy(sd[k][slot])


# ------------------------------------------------------------------------------------------- reference parity
@pytest.mark.parametrize("case", OPT_CASES)
@pytest.mark.parametrize("impl", ["autograd", "fused", "fused_graph", "fused_packed_graph"])
def test_rule_steps_vs_reference(case, impl):
    from deepfm_amd.training.fused_step import fused_step_class
    from deepfm_amd.training.step import RowSparseTrainStep
    g = load(case)
    kind = kind_of(g)
    model = _model(g)
    if "packed" in impl:
        model.embedding.pack_tables_()
    model.embedding.set_grad_mode("rowsparse")
    l2, clip = float(g["l2"]), float(g["clip"])
    opt = _opt(kind, model, lr=step_lr(g, 0), l2=l2, max_grad_norm=clip)
    assert opt.kind == kind
    B = g["step0/labels"].shape[0]
    if impl == "autograd":
        step = RowSparseTrainStep(model, opt, B, use_graph=False)
    else:
        cls = fused_step_class(model)
        assert cls is not None and cls.__name__.lower() == "fused" + cfg_of(g)["kind"].replace("_", "") + "step"
        step = cls(model, opt, B, use_graph="graph" in impl)
    if step.use_graph:
        step.load_batch(*_pool(g, 0))
        step.capture()
        for k, v in _state(model).items():
            assert np.array_equal(v, group(g, "init/")[k]), f"capture() changed {k}"
    for t in range(int(g["steps"])):
        opt.param_groups[0]["lr"] = step_lr(g, t)          # the way ReduceLROnPlateau sets it
        assert opt.lr == step_lr(g, t)
        step.load_batch(*_pool(g, t))
        step.run()
        bce = float(g[f"step{t}/bce"])
        assert abs(float(step.loss) - bce) < 1e-4 * bce, (t, float(step.loss), bce)
        norm = float(g[f"step{t}/grad_norm"])
        assert abs(float(opt.sq_norm) ** 0.5 - norm) < 1e-4 * norm
        assert_rule_params(_state(model), g, t, f"{case} {impl}")
    for k, v in _state(model).items():
        if "embeddings.C" in k:
            assert not v[0].any(), "padding row moved"
    assert_rule_state(_opt_state_getter(opt), g, f"{case} {impl}")


@pytest.mark.parametrize("case", ADAMW_CASES[:1] + SGD_CASES[:1])
def test_rule_logits_vs_reference(case):
    """The forward of every step (its parameters came from the previous steps' updates) against the reference's
    logits: the updates feed the next step's forward correctly."""
    from deepfm_amd.training.step import RowSparseTrainStep
    g = load(case)
    model = _model(g)
    model.embedding.set_grad_mode("rowsparse")
    opt = _opt(kind_of(g), model, lr=step_lr(g, 0), l2=float(g["l2"]), max_grad_norm=float(g["clip"]))
    B = g["step0/labels"].shape[0]
    step = RowSparseTrainStep(model, opt, B, use_graph=False)
    for t in range(int(g["steps"])):
        b = {k: torch.from_numpy(v).cuda() for k, v in group(g, f"step{t}/batch/").items()}
        with torch.no_grad():
            was = model.embedding.grad_mode
            logits = npy(model(b).squeeze(1))
        assert was == model.embedding.grad_mode
        want = g[f"step{t}/logits"]
        err = np.abs(logits.astype(np.float64) - want)
        assert (err <= 1e-3 * np.abs(want) + 1e-4 * np.abs(want).max()).all(), (t, float(err.max()))
        step.load_batch(*_pool(g, t))
        step.run()


# ------------------------------------------------------------------------------------------- LR under capture
def _records_run(kind, mode, lrs, n_launch=2, spg=4, seed=21):
    """Train n_launch * spg steps of a small DeepFM with optimizer ``kind``; lrs[i] holds for launch i (a group of
    spg steps).  mode: "eager", "lookahead" (capture(steps_per_graph=spg)), "nolookahead" (the same with
    plan_lookahead False) or "single" (steps_per_graph=1).  Returns (state_dict, optimizer state) on the host."""
    from deepfm_amd.training.fused_step import fused_step_class
    B = 512
    fields, _, model = _small_deepfm(seed=seed)
    model.embedding.pack_tables_()
    model.embedding.set_grad_mode("rowsparse")
    opt = _opt(kind, model, lr=lrs[0], l2=1e-5, max_grad_norm=1.0)
    step = fused_step_class(model)(model, opt, B, use_graph=mode != "eager")
    rng = np.random.default_rng(seed)
    ids, dense, labels = _rand_pool(fields, n_launch * spg, B, rng)
    recs = step.pack_batches(torch.from_numpy(ids).cuda(), torch.from_numpy(dense).cuda(),
                             torch.from_numpy(labels).cuda())
    if mode == "nolookahead":
        step.plan_lookahead = False
    if mode != "eager":
        step.load_packed(recs[0])
        step.capture(steps_per_graph=1 if mode == "single" else spg)
    for i in range(n_launch):
        opt.lr = lrs[i]
        group_recs = [recs[i * spg + k] for k in range(spg)]
        if mode in ("eager", "single"):
            for r in group_recs:
                step.run_from(r)
        else:
            step.run_group(group_recs)
    torch.cuda.synchronize()
    out = {k: npy(v).copy() for k, v in model.state_dict().items()}
    ost = {k: {s: npy(t).copy() for s, t in v.items()} for k, v in opt.state_dict()["state"].items()}
    step.release_graphs()
    return out, ost


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["lookahead", "nolookahead", "single"])
def test_lr_change_between_launches_reaches_the_graph(kind, mode):
    lrs = [1e-2, 2.5e-3]
    want, want_st = _records_run(kind, "eager", lrs)
    got, got_st = _records_run(kind, mode, lrs)
    for k in want:
        assert np.array_equal(want[k], got[k]), f"{kind} {mode}: {k} differs from the eager run"
    for k in want_st:
        for s in want_st[k]:
            assert np.array_equal(want_st[k][s], got_st[k][s]), f"{kind} {mode}: {s} of {k}"
    # and the change mattered: the unchanged schedule ends elsewhere
    same, _ = _records_run(kind, "eager", [lrs[0], lrs[0]])
    assert any(not np.array_equal(same[k], want[k]) for k in want if "embeddings.C" in k)


def test_lr_cannot_be_set_inside_a_capture():
    fields, _, model = _small_deepfm(seed=3)
    opt = _opt("sgd", model, lr=1e-2)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with pytest.raises(RuntimeError, match="capture"):
            with torch.cuda.graph(graph, stream=side):
                opt.lr = 5e-3
    assert opt.lr == 1e-2 and float(opt._lr_dev) == np.float32(1e-2)


def test_lrsched_fixture_through_a_captured_multistep_graph():
    """train_steps_deepfm_lrsched (Adam, LR halved after step 1) through the fused step captured as single-step
    graphs: the LR set between launches is the one each step uses."""
    from deepfm_amd.training.fused_step import fused_step_class
    g = load(LRSCHED_CASE)
    model = _model(g)
    model.embedding.pack_tables_()
    model.embedding.set_grad_mode("rowsparse")
    opt = _opt("adam", model, lr=step_lr(g, 0), l2=float(g["l2"]), max_grad_norm=float(g["clip"]))
    B = g["step0/labels"].shape[0]
    step = fused_step_class(model)(model, opt, B, use_graph=True)
    recs = [step.pack_batches(*(x.unsqueeze(0) for x in _pool(g, t)))[0] for t in range(int(g["steps"]))]
    step.load_packed(recs[0])
    step.capture()                                    # single-step graphs (no look-ahead): steps 0 and 1
    for t in (0, 1):
        opt.lr = step_lr(g, t)
        step.run_from(recs[t])
        assert_rule_params(_state(model), g, t, "lrsched single-step graph")
    step.release_graphs()
    step.load_packed(recs[2])
    step.capture(steps_per_graph=2)                   # steps 2 and 3: one look-ahead launch
    opt.lr = step_lr(g, 2)
    step.run_group([recs[2], recs[3]])
    assert_rule_params(_state(model), g, 3, "lrsched multi-step graph")
    assert_rule_state(_opt_state_getter(opt), g, "lrsched")
    step.release_graphs()


# ------------------------------------------------------------------------------------------- checkpoints
def _ckpt_run(kind, seed=5):
    from deepfm_amd.training.step import RowSparseTrainStep
    B = 384
    fields, _, model = _small_deepfm(seed=seed)
    opt = _opt(kind, model, lr=1e-2, l2=1e-5, max_grad_norm=1.0)
    step = RowSparseTrainStep(model, opt, B, use_graph=False)
    rng = np.random.default_rng(seed)
    ids, dense, labels = _rand_pool(fields, 4, B, rng)
    return model, opt, step, (ids, dense, labels)


def _train(step, opt, pool, ts, lrs):
    ids, dense, labels = pool
    for t in ts:
        opt.lr = lrs[t]
        step.load_batch(torch.from_numpy(ids[t]).cuda(), torch.from_numpy(dense[t]).cuda(),
                        torch.from_numpy(labels[t]).cuda())
        step.run()
    torch.cuda.synchronize()


def _as_torch_state_dict(kind, model, opt):
    """opt's state in the layout torch.optim.AdamW / SGD write (position-keyed state + param_groups)."""
    tmp = [torch.nn.Parameter(torch.zeros(1)) for _ in model.parameters()]
    torch_opt = (torch.optim.AdamW(tmp, lr=opt.lr) if kind == "adamw" else
                 torch.optim.SGD(tmp, lr=opt.lr, momentum=0.9))
    sd = torch_opt.state_dict()
    own = opt.state_dict()
    for i, (name, _) in enumerate(model.named_parameters()):
        st = {k: v.cpu() for k, v in own["state"][name].items()}
        if kind == "adamw":
            st["step"] = torch.tensor(float(own["step"]))
        sd["state"][i] = st
    return sd


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
@pytest.mark.parametrize("fmt", ["torch", "own"])
def test_checkpoint_continues_bit_identically(kind, fmt):
    lrs = [1e-2, 1e-2, 5e-3, 5e-3]                 # the own format also carries a reduced LR
    model, opt, step, pool = _ckpt_run(kind)
    _train(step, opt, pool, range(4), lrs)
    want = {k: npy(v).copy() for k, v in model.state_dict().items()}

    model, opt, step, pool = _ckpt_run(kind)
    _train(step, opt, pool, range(2), lrs)
    opt.lr = lrs[2]
    sd = _as_torch_state_dict(kind, model, opt) if fmt == "torch" else opt.state_dict()
    weights = {k: v.clone() for k, v in model.state_dict().items()}
    fresh, fopt, fstep, _ = _ckpt_run(kind, seed=6)
    fresh.load_state_dict(weights)
    assert fopt.lr == 1e-2
    fopt.load_state_dict(sd)
    assert fopt.lr == lrs[2], "the learning rate is restored from the checkpoint"
    if kind == "adamw":
        assert int(fopt.step_count) == 2
    _train(fstep, fopt, pool, range(2, 4), lrs)
    for k, v in fresh.state_dict().items():
        assert np.array_equal(npy(v), want[k]), f"{kind} {fmt}: resumed run diverged at {k}"


def test_checkpoint_of_another_kind_is_refused():
    model, sgd, _, _ = _ckpt_run("sgd")
    with pytest.raises(ValueError):
        _opt("adamw", model, lr=1e-2).load_state_dict(sgd.state_dict())
    with pytest.raises(ValueError):
        _opt("adam", model, lr=1e-2).load_state_dict(_as_torch_state_dict("sgd", model, sgd))
    adamw = _opt("adamw", model, lr=1e-2)
    with pytest.raises(ValueError):
        _opt("adam", model, lr=1e-2).load_state_dict(_as_torch_state_dict("adamw", model, adamw))
    with pytest.raises(ValueError):
        sgd.load_state_dict(torch.optim.Adam(model.parameters(), lr=1e-3).state_dict())


def test_sharded_step_refuses_other_kinds():
    from deepfm_amd.training.sharded import make_sharded_step
    _, _, model = _small_deepfm(seed=2)
    with pytest.raises(NotImplementedError, match="Adam"):
        make_sharded_step(model, 256, kind="sgd", lr=1e-2)


# ------------------------------------------------------------------------------------------- node refusal
def test_plan_node_update_refuses_another_rule():
    from deepfm_amd.training.fused_step import fused_step_class
    B = 256
    fields, _, model = _small_deepfm(seed=9)
    model.embedding.pack_tables_()
    model.embedding.set_grad_mode("rowsparse")
    opt = _opt("adamw", model, lr=1e-3, l2=1e-5, max_grad_norm=1.0)
    step = fused_step_class(model)(model, opt, B, use_graph=True)
    rng = np.random.default_rng(1)
    ids, dense, labels = _rand_pool(fields, 2, B, rng)
    recs = step.pack_batches(torch.from_numpy(ids).cuda(), torch.from_numpy(dense).cuda(), torch.from_numpy(labels).cuda())
    step.load_packed(recs[0])
    step.capture(steps_per_graph=2)
    slot = step.slots[0]
    _, apply_at, cur, target = slot.at[0]                        # the apply node's launch destination
    assert apply_at is not None and apply_at.node and apply_at.graph_exec == slot.graph.raw_cuda_graph_exec()
    nxt = recs[1].data_ptr() + step._rec_id_offsets[0]
    opt.apply_plan(cur, nxt, target, apply_at)                       # its own rule: accepted
    for other in ("adam", "sgd"):
        opt.kind = other                                             # the descriptor now names another rule
        try:
            with pytest.raises(RuntimeError, match="another kernel"):
                opt.apply_plan(cur, nxt, target, apply_at)
        finally:
            del opt.kind
    step.run_group([recs[0], recs[1]])                               # the graph still runs its own rule
    torch.cuda.synchronize()
    step.release_graphs()


# ------------------------------------------------------------------------------------------- full size
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_fullsize_two_steps_follow_the_rule(kind):
    """Criteo shape (26 x 10^6 rows, d = 16, B = 4096), fused DeepFM as one graph of two steps: rows no batch
    touched keep weights and hold no state (SGD: the v slot is never written); rows touched by step 1 only carry
    exactly one update (lazy: step 2 leaves them alone) that satisfies the rule against the state they hold
    (SGD: w = w0 - lr * buf; AdamW: w = (1 - lr wd) w0 - lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps), step 1)."""
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.synthetic import criteo_fields, schema_from_fields
    from deepfm_amd.models import create_model
    from deepfm_amd.training.fused_step import fused_step_class
    V, B, D, S = 1_000_000, 4096, 16, 26
    fields = criteo_fields(V, D)
    cfg = ExperimentConfig()
    cfg.dnn.dropout = 0.0
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = create_model("deepfm", schema_from_fields(fields), cfg)
    model.train()
    model.embedding.pack_tables_()
    model.embedding.set_grad_mode("rowsparse")
    lr = 1e-2
    opt = _opt(kind, model, lr=lr, l2=cfg.feature.embedding_l2_reg, max_grad_norm=cfg.training.gradient_clip_norm)
    step = fused_step_class(model)(model, opt, B, use_graph=True)
    gen = torch.Generator(device="cuda").manual_seed(7)
    ids = torch.randint(1, V, (2, S, B), generator=gen, device="cuda")
    ids[:, :, :64] = 0                                                   # padding ids
    ids[1, :, 100:200] = ids[0, :, 100:200]                              # rows both steps touch
    dense = torch.rand((2, 13, B), generator=gen, device="cuda")
    labels = (torch.rand((2, B), generator=gen, device="cuda") < 0.25).float()
    recs = step.pack_batches(ids, dense, labels)
    names = [f["name"] for f in fields[:S]]
    step.load_packed(recs[0])
    step.capture(steps_per_graph=2)
    emb = model.embedding
    before = {n: emb.second_order_embeddings[n].weight.detach().clone() for n in names[:4]}
    step.run_group([recs[0], recs[1]])
    torch.cuda.synchronize()
    wd = 1e-2
    for j, n in enumerate(names[:4]):
        rec = emb.packed[n]
        w0, w2, m2 = before[n], emb.second_order_embeddings[n].weight.detach(), rec["m2"]
        t0, t1 = torch.unique(ids[0, j]), torch.unique(ids[1, j])
        t0, t1 = t0[t0 != 0], t1[t1 != 0]
        touched = torch.zeros(V, dtype=torch.bool, device="cuda")
        touched[t0] = True
        touched[t1] = True
        untouched = ~touched
        assert torch.equal(w2[untouched], w0[untouched]), f"{n}: an untouched row moved"
        assert not m2[untouched].any(), f"{n}: untouched rows have optimizer state"
        if kind == "adamw":
            assert not rec["v2"][untouched].any()
        else:
            assert not rec["v2"].any(), "SGD wrote the v slot"
        only1 = torch.zeros(V, dtype=torch.bool, device="cuda")
        only1[t0] = True
        only1[t1] = False
        both = torch.zeros(V, dtype=torch.bool, device="cuda")
        both[t0] = True
        both &= ~only1
        # rows touched by step 1 only: one update from w0 with the state they hold now
        r = only1.nonzero().squeeze(1)
        w0r, w1r, m1r = w0[r].double(), w2[r].double(), m2[r].double()
        if kind == "sgd":
            want = w0r - lr * m1r
        else:
            v1r = rec["v2"][r].double()
            want = (1 - lr * wd) * w0r - (lr / (1 - 0.9)) * m1r / (v1r.sqrt() / np.sqrt(1 - 0.999) + 1e-8)
        err = (w1r - want).abs()
        assert (err <= 1e-6 * w0r.abs() + 1e-3 * lr * (m1r.abs() + 1e-6 if kind == "sgd" else 1.0)).all(), \
            f"{n}: step-1-only rows do not follow the rule (max err {float(err.max()):.3e})"
        assert both.any() and r.numel() > 0
