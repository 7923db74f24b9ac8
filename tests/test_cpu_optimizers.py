"""AdamW / SGD update rules, the learning-rate schedule and the optimizer factory, without a GPU.

* The numpy lazy rules (tests/optim_reference.py), fed with the oracle's gradients, reproduce the
  reference-generated fixtures (torch.optim.AdamW / SGD(momentum=0.9) as trainer.py:67-78 builds them, and an LR
  change through param_groups) at every step: parameters and the final moments / momentum buffers.
* ``deepfm_amd.training.ReduceLROnPlateau`` gives torch's LR sequence.
* ``build_optimizer`` / ``build_scheduler`` map every config value and refuse unknown ones.
* The library exports the descriptor entry points, which refuse bad descriptors before touching a device.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import load
from tests.optim_reference import (ADAMW_CASES, OPT_CASES, assert_rule_params, assert_rule_state, numpy_steps,
                                   rule_update)


def _state_getter(state):
    return lambda slot, k: state[("m/" if slot in ("exp_avg", "momentum_buffer") else "v/") + k]


@pytest.mark.parametrize("case", OPT_CASES)
def test_numpy_rules_vs_reference(case):
    g = load(case)
    state = None
    for t, params, state, _ in numpy_steps(g):
        assert_rule_params(params, g, t, case)
        for k, v in params.items():
            if "embeddings.C" in k:
                assert not v[0].any(), "padding row moved"
    assert_rule_state(_state_getter(state), g, case)


def test_bounds_catch_a_missing_weight_decay(monkeypatch):
    """The parameter bound is tight enough to tell AdamW from Adam (lr 1e-2: 1e-4 of |w| decay per step)."""
    import tests.optim_reference as R
    g = load("train_steps_deepfm_adamw_l2clip")
    monkeypatch.setattr(R, "rule_update", lambda kind, *a: rule_update("adam", *a))
    with pytest.raises(AssertionError):
        for t, params, _, _ in R.numpy_steps(g):
            R.assert_rule_params(params, g, t, "adam rule on an AdamW fixture")


def test_sgd_rule_vs_torch():
    """rule_update("sgd") against torch.optim.SGD(momentum=0.9) on random tensors, with an LR change."""
    rng = np.random.default_rng(3)
    w = rng.standard_normal((9, 4)).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(w.copy()))
    opt = torch.optim.SGD([p], lr=0.05, momentum=0.9)
    m, v = np.zeros_like(w), np.zeros_like(w)
    for step, lr in enumerate([0.05, 0.05, 0.025, 0.025], 1):
        opt.param_groups[0]["lr"] = lr
        gr = rng.standard_normal(w.shape).astype(np.float32)
        p.grad = torch.from_numpy(gr.copy())
        opt.step()
        rule_update("sgd", w, m, v, gr, step, lr)
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(m, opt.state[p]["momentum_buffer"].numpy(), rtol=1e-6, atol=1e-7)
    assert not v.any()


def test_adamw_rule_vs_torch():
    rng = np.random.default_rng(4)
    w = rng.standard_normal((7, 3)).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(w.copy()))
    opt = torch.optim.AdamW([p], lr=3e-3)
    m, v = np.zeros_like(w), np.zeros_like(w)
    for step in range(1, 5):
        gr = rng.standard_normal(w.shape).astype(np.float32)
        p.grad = torch.from_numpy(gr.copy())
        opt.step()
        rule_update("adamw", w, m, v, gr, step, 3e-3)
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------------------------------------- schedule
class _LrHolder:
    """The one attribute ReduceLROnPlateau reads and sets."""

    def __init__(self, lr):
        self.lr = lr


SEQUENCES = {
    "plateau": [0.70, 0.70, 0.70, 0.70, 0.70, 0.70, 0.70, 0.70, 0.70, 0.70],
    "improving": [0.60, 0.62, 0.64, 0.66, 0.68, 0.70, 0.72],
    "below_threshold": [0.7, 0.70001, 0.70002, 0.70003, 0.70004, 0.70005, 0.70006, 0.7001, 0.9, 0.9, 0.9, 0.9],
    "noisy": [0.5, 0.7, 0.65, 0.69, 0.71, 0.70, 0.68, 0.72, 0.60, 0.61, 0.62, 0.63, 0.64, 0.80],
    "min_lr": [0.5] * 30,
}
KWARGS = [dict(), dict(mode="max", factor=0.5, patience=2, cooldown=2), dict(mode="min", factor=0.3, patience=1),
          dict(mode="max", factor=0.5, patience=0, min_lr=2e-4), dict(mode="max", threshold=1e-2, patience=1),
          dict(mode="min", threshold_mode="abs", threshold=0.05, patience=1, cooldown=1),
          dict(mode="max", factor=0.5, patience=0, min_lr=9.9e-4, eps=1e-5)]


@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("kw", range(len(KWARGS)))
def test_reduce_on_plateau_vs_torch(seq, kw):
    from deepfm_amd.training.schedule import ReduceLROnPlateau
    kwargs = KWARGS[kw]
    theirs_opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    defaults = dict(mode="max", factor=0.5, patience=2)       # the reference trainer's (trainer.py:82-84)
    theirs = torch.optim.lr_scheduler.ReduceLROnPlateau(theirs_opt, **{**defaults, **kwargs})
    holder = _LrHolder(1e-3)
    ours = ReduceLROnPlateau(holder, **kwargs)
    for x in SEQUENCES[seq]:
        theirs.step(x)
        ours.step(x)
        assert holder.lr == theirs_opt.param_groups[0]["lr"], (seq, kwargs, x)


def test_reduce_on_plateau_reduces():
    from deepfm_amd.training.schedule import ReduceLROnPlateau
    holder = _LrHolder(1e-3)
    s = ReduceLROnPlateau(holder)
    for _ in range(4):
        s.step(0.7)
    assert holder.lr == 5e-4


# ---------------------------------------------------------------------------------------------- factories
class _FakeOpt:
    def __init__(self, model, **kw):
        self.model, self.kw = model, kw


@pytest.mark.parametrize("name,cls_name", [("adam", "RowSparseAdam"), ("adamw", "RowSparseAdamW"),
                                           ("sgd", "RowSparseSGD")])
@pytest.mark.parametrize("clip", [1.0, 0.0])
def test_build_optimizer_maps_the_config(monkeypatch, name, cls_name, clip):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.training import rowsparse
    cfg = ExperimentConfig()
    cfg.training.optimizer, cfg.training.lr, cfg.training.gradient_clip_norm = name, 0.02, clip
    cfg.feature.embedding_l2_reg = 3e-5
    monkeypatch.setitem(rowsparse.OPTIMIZERS, name, _FakeOpt)
    opt = rowsparse.build_optimizer("model", cfg)
    assert opt.model == "model"
    assert opt.kw == dict(lr=0.02, l2=3e-5, max_grad_norm=clip if clip else None)
    monkeypatch.undo()
    assert rowsparse.OPTIMIZERS[name].__name__ == cls_name and rowsparse.OPTIMIZERS[name].kind == name


def test_optimizer_defaults_match_torch():
    import inspect
    from deepfm_amd.training import RowSparseAdamW, RowSparseSGD
    assert inspect.signature(RowSparseAdamW).parameters["weight_decay"].default == \
        torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults["weight_decay"]
    assert inspect.signature(RowSparseSGD).parameters["momentum"].default == 0.9     # trainer.py:73-76


def test_build_optimizer_rejects_unknown():
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.training import build_optimizer
    cfg = ExperimentConfig()
    cfg.training.optimizer = "rmsprop"
    with pytest.raises(ValueError, match="Unknown optimizer: rmsprop"):
        build_optimizer(None, cfg)


def test_build_scheduler():
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.training import ReduceLROnPlateau, build_scheduler
    cfg = ExperimentConfig()
    assert cfg.training.scheduler == "reduce_on_plateau"
    holder = _LrHolder(1e-3)
    s = build_scheduler(holder, cfg)
    assert isinstance(s, ReduceLROnPlateau)
    assert (s.mode, s.factor, s.patience, s.threshold, s.cooldown, s.min_lr) == ("max", 0.5, 2, 1e-4, 0, 0.0)
    assert s.optimizer is holder
    cfg.training.scheduler = "none"
    assert build_scheduler(holder, cfg) is None
    cfg.training.scheduler = "cosine"
    with pytest.raises(ValueError, match="Unknown scheduler: cosine"):
        build_scheduler(holder, cfg)


# ---------------------------------------------------------------------------------------------- C ABI
NEW_SYMBOLS = ["dfm_step_apply", "dfm_step_apply_plan"]


def test_library_exports_the_descriptor_entry_points():
    from deepfm_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        getattr(lib, name)
    assert len(_lib.SIGNATURES["dfm_step_apply_plan"][1]) == 29      # 28 operands + the launch destination
    assert C.sizeof(_lib.Optim) == 32 and _lib.Optim.d_lr.offset == 24


def _bad_descriptor_calls(optim):
    """The entry points with plausible (never dereferenced) arguments and ``optim``: apply, apply-plan on a stream,
    apply-plan re-pointing a (fake, never touched) graph node."""
    from deepfm_amd import _lib
    lib = _lib.load()
    tabs = (_lib.Table * 1)()
    tabs[0].w2 = tabs[0].w1 = tabs[0].m2 = tabs[0].m1 = tabs[0].v2 = tabs[0].v1 = 0x1000
    P = 0x1000
    o = C.byref(optim) if optim is not None else None
    yield lib.dfm_step_apply(tabs, 1, 16, 1, P, P, P, P, P, P, o, P, P, P, P, P, 64, 1, None)
    yield lib.dfm_step_apply_plan(tabs, 1, 16, 1, P, P, P, P, P, P, o, P, P, P, P, P, 64, 1, P, 64, P, 100, 64,
                                  P, P, P, P, P, None)
    yield lib.dfm_step_apply_plan(tabs, 1, 16, 1, P, P, P, P, P, P, o, P, P, P, P, P, 64, 1, P, 64, P, 100, 64,
                                  P, P, P, P, P, _lib.at_node(P, P))


@pytest.mark.parametrize("bad", ["null_lr", "unknown_kind", "null_descriptor"])
def test_descriptor_entry_points_reject_bad_descriptors(bad):
    from deepfm_amd import _lib
    o = _lib.Optim(kind=_lib.OPT_ADAMW, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, momentum=0.0, d_lr=0x2000)
    if bad == "null_lr":
        o.d_lr = None
    elif bad == "unknown_kind":
        o.kind = 7
    else:
        o = None
    lib = _lib.load()
    for rc in _bad_descriptor_calls(o):
        assert rc == 1, rc                                   # DFM_ERR_INVALID, nothing launched
        msg = lib.dfm_last_error().decode()
        assert ("d_lr" in msg) if bad == "null_lr" else ("kind" in msg if bad == "unknown_kind" else "dfm_optim" in msg)
