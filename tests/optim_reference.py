"""Expected values for the AdamW / SGD update rules and the learning-rate schedule, shared by
test_cpu_optimizers.py and test_gpu_optimizers.py.

The fixtures (``tests/golden/train_steps_*_{adamw,sgd}*.npz``, ``train_steps_deepfm_lrsched.npz``;
tools/make_golden.py::optimizer_cases) hold steps of the reference trainer's body with ``torch.optim.AdamW`` /
``torch.optim.SGD(momentum=0.9)`` (trainer.py:67-78) or an LR change through ``param_groups``.  The oracle's
``train_step_rowsparse`` supplies one step's gradients, clip coefficient and row lists (it applies Adam to the
copy it is given, which is discarded); the rules below apply AdamW or SGD to them in numpy, lazily on the rows.
"""
from __future__ import annotations

import numpy as np

from oracle import ctr_oracle as O
from tests.helpers import cfg_of, fields_of, group
from tests.test_oracle_golden import (ADAM_EPS, _model_cfg, adam_param_bound, train_case_state,
                                      zero_grad_param)

ADAMW_CASES = ["train_steps_deepfm_adamw", "train_steps_deepfm_adamw_l2clip", "train_steps_xdeepfm_adamw",
               "train_steps_attention_deepfm_adamw"]
SGD_CASES = ["train_steps_deepfm_sgd", "train_steps_deepfm_sgd_l2clip", "train_steps_xdeepfm_sgd",
             "train_steps_attention_deepfm_sgd"]
LRSCHED_CASE = "train_steps_deepfm_lrsched"
OPT_CASES = ADAMW_CASES + SGD_CASES + [LRSCHED_CASE]
ADAMW_WD, SGD_MOMENTUM = 1e-2, 0.9         # torch.optim.AdamW's default weight decay; trainer.py:73-76


def kind_of(g) -> str:
    return str(g["optimizer"])


def step_lr(g, t) -> float:
    return float(g[f"step{t}/lr"])


def max_lr(g) -> float:
    return max(step_lr(g, t) for t in range(int(g["steps"])))


def coefs(g):
    return [min(1.0, float(g["clip"]) / (float(g[f"step{t}/grad_norm"]) + 1e-6)) for t in range(int(g["steps"]))]


def rule_update(kind, w, m, v, g, step, lr):
    """One step of ``kind`` on arrays (in place), float32 like torch: AdamW = decay then Adam; SGD with momentum
    0.9, dampening 0 (a zero buffer gives torch's first-step ``buf = g``)."""
    f = np.float32
    if kind == "sgd":
        m *= f(SGD_MOMENTUM)
        m += g
        w -= f(lr) * m
        return
    if kind == "adamw":
        w *= f(1.0 - lr * ADAMW_WD)
    O.adam_update(w, m, v, g, step, lr)


def numpy_steps(g):
    """Yields (t, params, state, info) after each step of the lazy rule of the fixture's kind, with the
    oracle's gradients; state is ``m/<key>`` (Adam moment / SGD buffer) and ``v/<key>``."""
    kind = kind_of(g)
    fields, c = fields_of(g), cfg_of(g)
    ocfg = _model_cfg(c)
    params, state = train_case_state(g)
    for t in range(int(g["steps"])):
        lr = step_lr(g, t)
        hp = dict(lr=lr, l2=float(g["l2"]), max_grad_norm=float(g["clip"]))
        info = {}
        scratch = {k: v.copy() for k, v in params.items()}
        _, scratch_state = train_case_state(g)
        O.train_step_rowsparse(c["kind"], fields, scratch, scratch_state, group(g, f"step{t}/batch/"),
                               g[f"step{t}/labels"], ocfg, hp, t + 1, exact_order=True, info=info)
        coef = np.float32(info["coef"])
        for k, gr in info["grads"].items():
            rule_update(kind, params[k], state["m/" + k], state["v/" + k], gr * coef, t + 1, lr)
        for name, (uniq, r2, r1) in info["rows"].items():
            for key, gr in ((f"embedding.second_order_embeddings.{name}.weight", r2),
                            (f"embedding.first_order_embeddings.{name}.weight", r1[:, None])):
                w, m, v = params[key][uniq], state["m/" + key][uniq], state["v/" + key][uniq]
                rule_update(kind, w, m, v, gr * coef, t + 1, lr)
                params[key][uniq], state["m/" + key][uniq], state["v/" + key][uniq] = w, m, v
        yield t, params, state, info


def sgd_param_bound(g, t, k, r=1e-4, a=1e-5):
    """Per-element bound on |w - w_ref| after step t+1 for SGD with momentum.  Adam's bound (a step of about lr
    per element, whatever the gradient) does not carry over: SGD's step is lr * buf, proportional to the
    gradients.  w_t = w_0 - sum_u lr_u buf_u with buf_u = sum_{k<=u} mu^(u-k) c_k g_k is linear in the clipped
    gradients, so perturbing each gradient by the parity bar — r relative plus a of the tensor's largest, times
    4^k for step k as in adam_param_bound (gradients taken at parameters that already differ; BatchNorm
    amplifies) — moves w by at most sum_u lr_u sum_{k<=u} mu^(u-k) 4^k (r |c_k g_k| + a max |c_k g_k|): a bound
    relative to the update itself."""
    cs = coefs(g)
    bound, buf = 0.0, 0.0
    for u in range(t + 1):
        gu = np.abs(g[f"step{u}/grad/{k}"].astype(np.float64)) * cs[u]
        buf = SGD_MOMENTUM * buf + 4.0 ** u * (r * gu + a * float(gu.max()))
        bound = bound + step_lr(g, u) * buf
    return bound


def assert_rule_params(got, g, t, what="", rtol=1e-4):
    """Parameters after step t+1 against the reference's, every element (parameters with an identically-zero
    gradient skipped, as for Adam): 1e-4 relative plus the rule's perturbation bound."""
    kind = kind_of(g)
    want = group(g, f"step{t}/param/")
    for k, w in want.items():
        if "running_" in k or k.endswith("num_batches_tracked") or zero_grad_param(k, g):
            continue
        extra = sgd_param_bound(g, t, k) if kind == "sgd" else adam_param_bound(g, t, k, max_lr(g))
        bound = rtol * np.abs(w.astype(np.float64)) + extra
        err = np.abs(np.asarray(got[k], dtype=np.float64).reshape(w.shape) - w)
        bad = err > bound
        if bad.any():
            i = np.unravel_index(np.argmax(err - bound), err.shape)
            raise AssertionError(f"{what}: step {t} {k}: {int(bad.sum())}/{bad.size} outside, worst at {i}: "
                                 f"got {np.asarray(got[k]).reshape(w.shape)[i]!r} want {w[i]!r} bound {bound[i]:.3e}")


def assert_rule_state(get, g, what=""):
    """Final optimizer state against torch's (``opt/<slot>/<key>``); ``get(slot, key)`` returns this side's array.
    Adam / AdamW moments as assert_adam_moments bounds them; the SGD buffer (a momentum-weighted sum of the clipped
    gradients) to 1e-4 relative plus 1e-3 of the momentum-weighted largest gradient that went in."""
    steps = int(g["steps"])
    cs = coefs(g)
    for key in list(g):
        if not key.startswith("opt/"):
            continue
        _, slot, k = key.split("/", 2)
        if zero_grad_param(k, g):
            continue
        gmaxes = [float(np.abs(g[f"step{t}/grad/{k}"]).max()) * cs[t] for t in range(steps)]
        if slot == "momentum_buffer":
            bound = 1e-3 * sum(SGD_MOMENTUM ** (steps - 1 - t) * gm for t, gm in enumerate(gmaxes))
        elif slot == "exp_avg":
            bound = 1e-3 * max(gmaxes) + ADAM_EPS
        else:
            bound = 2e-3 * max(gmaxes) ** 2 + ADAM_EPS ** 2
        want = g[key].astype(np.float64)
        err = np.abs(np.asarray(get(slot, k), dtype=np.float64).reshape(want.shape) - want)
        assert (err <= 1e-4 * np.abs(want) + bound + 1e-30).all(), (what, slot, k, float(err.max()))
