"""Shared helpers for the test-suite: golden loading, tolerances, schema glue."""
from __future__ import annotations

import json
import os
from typing import Dict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Floating-point bar of BASELINE.json: logits within 1e-4 relative of the reference
# CPU path.  `assert_close` applies it element-wise with an absolute floor tied to
# the magnitude of the tensor (an element that is ~0 by cancellation cannot be held
# to a relative bound).
RTOL = 1e-4


def load(name: str) -> Dict[str, np.ndarray]:
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def group(d: Dict[str, np.ndarray], prefix: str) -> Dict[str, np.ndarray]:
    n = len(prefix)
    return {k[n:]: v for k, v in d.items() if k.startswith(prefix)}


def fields_of(d) -> list:
    return json.loads(str(d["fields"]))


def cfg_of(d) -> dict:
    return json.loads(str(d["cfg"]))


def assert_close(got, want, rtol: float = RTOL, atol_scale: float = 1e-5, what: str = "", floor: float = 0.0):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-30)
    err = np.abs(got - want)
    bound = rtol * np.abs(want) + atol_scale * scale + floor
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err - bound), err.shape)
        raise AssertionError(
            f"{what}: {bad.sum()} / {bad.size} elements out of tolerance; worst at {i}: "
            f"got {got[i]!r} want {want[i]!r} (|err| {err[i]:.3e}, bound {bound[i]:.3e})")


def hashed_weights(shape, salt: int, scale: float) -> np.ndarray:
    """Same closed form as tools/make_golden.py::hashed_weights (exact integer arithmetic)."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(13))) % np.uint64(1 << 24)
    v = (h.astype(np.float64) / float(1 << 24) - 0.5) * 2.0 * scale
    return v.astype(np.float32).reshape(shape)


def cin_full_params(F=39, layer_sizes=(128, 128, 128), split_half=True):
    """Parameters of the `cin_criteo_full` golden case (not stored: recomputed)."""
    params = {}
    prev = F
    for li, size in enumerate(layer_sizes):
        k = prev * F
        params[f"conv_layers.{li}.weight"] = hashed_weights((size, k, 1), 2 * li + 1, 2.0 / np.sqrt(k))
        params[f"conv_layers.{li}.bias"] = hashed_weights((size,), 2 * li + 2, 0.1)
        prev = size - size // 2 if (split_half and li < len(layer_sizes) - 1) else size
    return params


# ---- glue between the golden "fields" description and the package's schema objects ----

from deepfm_amd.data.synthetic import random_fields_batch, schema_from_fields  # noqa: E402,F401  (package helpers)


def load_params(module, params: Dict[str, np.ndarray], device="cuda"):
    """Copy golden/oracle parameters (state_dict-keyed numpy arrays) into a torch module."""
    import torch
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}
    missing, unexpected = module.load_state_dict(sd, strict=True), None
    return module.to(device)


def to_device_batch(batch: Dict[str, np.ndarray], device="cuda"):
    import torch
    return {k: torch.from_numpy(v).to(device) for k, v in batch.items()}


def npy(t):
    return t.detach().cpu().numpy()


def assert_close_mostly(got, want, max_bad_frac: float, rtol: float = RTOL, atol_scale: float = 1e-5, what: str = ""):
    """assert_close that tolerates a bounded fraction of outliers.  Used only where a ReLU kink
    makes the gradient discontinuous: an activation within rounding distance of 0 may land on the
    other side of the kink in fp32-vs-split-bf16 arithmetic, which flips one (sample, d) column of
    the CIN gradients.  Everything else must still meet the normal bar."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-30)
    bad = np.abs(got - want) > rtol * np.abs(want) + atol_scale * scale
    frac = bad.mean() if bad.size else 0.0
    assert frac <= max_bad_frac, f"{what}: {bad.sum()} / {bad.size} elements ({frac:.2e}) out of tolerance"


# ---- field self-attention: an fp64 reference that shares no code with oracle/ ----

def error_ratio(got, want, rtol: float = RTOL, atol_scale: float = 1e-5, floor: float = 0.0) -> float:
    """Worst |got - want| / bound over the elements, with `assert_close`'s bound: <= 1 is a pass."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"shape {got.shape} vs {want.shape}"
    if not want.size:
        return 0.0
    scale = max(float(np.abs(want).max()), 1e-30)
    ratio = np.abs(got - want) / (rtol * np.abs(want) + atol_scale * scale + floor)
    return float(ratio.max()) if np.isfinite(ratio).all() else float("inf")


def attention_core_fp64(qkv, num_heads: int, d_o=None):
    """softmax(Q_h K_h^T / sqrt(hd)) V_h per head in torch-CPU float64.  qkv (B, F, 3A), rows [q | k | v];
    returns o (B, F, A) and, with an upstream gradient d_o, d_qkv from autograd on (o * d_o).sum()."""
    import torch
    t = torch.from_numpy(np.asarray(qkv, dtype=np.float64)).requires_grad_(d_o is not None)
    B, F, A3 = t.shape
    A = A3 // 3
    hd = A // num_heads
    q, k, v = (t[..., i * A:(i + 1) * A].reshape(B, F, num_heads, hd).transpose(1, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(B, F, A)
    if d_o is None:
        return o.numpy(), None
    (o * torch.from_numpy(np.asarray(d_o, dtype=np.float64))).sum().backward()
    return o.detach().numpy(), t.grad.numpy()


def attention_block_fp64(x, p, prefix: str, num_heads: int, use_residual: bool) -> dict:
    """One _AttentionBlock in torch float64 with its intermediates (all part of one autograd graph):
    qkv (B, F, 3A) the stacked projection, o (B, F, A) the head outputs, y = o W_out^T + b_out and,
    with the residual, mean / rstd of y + x and out = LayerNorm(y + x); without it out is y."""
    import torch
    A = p[prefix + "W_q.weight"].shape[0]
    B, F, _ = x.shape
    hd = A // num_heads
    qkv = torch.cat([x @ p[prefix + n + ".weight"].T + p[prefix + n + ".bias"] for n in ("W_q", "W_k", "W_v")], dim=-1)
    q, k, v = (qkv[..., i * A:(i + 1) * A].reshape(B, F, num_heads, hd).transpose(1, 2) for i in range(3))
    pr = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1)
    o = (pr @ v).transpose(1, 2).reshape(B, F, A)
    y = o @ p[prefix + "W_out.weight"].T + p[prefix + "W_out.bias"]
    r = dict(qkv=qkv, o=o, y=y, out=y)
    if use_residual:
        s = y + x
        mean = s.mean(-1, keepdim=True)
        rstd = (((s - mean) ** 2).mean(-1, keepdim=True) + 1e-5).rsqrt()
        r.update(mean=mean, rstd=rstd,
                 out=(s - mean) * rstd * p[prefix + "layer_norm.weight"] + p[prefix + "layer_norm.bias"])
    return r


def attention_fp64(x, params: Dict[str, np.ndarray], num_heads: int, num_layers: int, use_residual: bool,
                   upstream=None):
    """MultiHeadSelfAttention as stacked blocks in torch-CPU float64; state_dict-keyed arrays in and out like
    the oracle.  Returns (out, d_x, grads); the gradients are autograd's on (out * upstream).sum() and None
    without an upstream."""
    import torch
    p = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).requires_grad_(upstream is not None)
         for k, v in params.items()}
    t = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(upstream is not None)
    h = t
    for li in range(num_layers):
        h = attention_block_fp64(h, p, f"layers.{li}.", num_heads, use_residual)["out"]
    if upstream is None:
        return h.numpy(), None, None
    (h * torch.from_numpy(np.asarray(upstream, dtype=np.float64))).sum().backward()
    return h.detach().numpy(), t.grad.numpy(), {k: v.grad.numpy() for k, v in p.items()}


def attention_case_inputs(c: dict, x_scale: float = 1.0):
    """Parameters (state_dict keys, fp32, uniform in +-0.4, LayerNorm weight in [0.5, 1.5]), x and upstream
    (standard normal, x times `x_scale`) of a matrix case dict(B, F, D, heads, A, layers, residual), seeded
    from the shape alone: every route that runs a shape sees the same numbers."""
    rng = np.random.default_rng([c["F"], c["D"], c["heads"], c["A"], c["layers"], int(c["residual"]), c["B"]])
    D, A = c["D"], c["A"]
    params = {}
    for li in range(c["layers"]):
        pre = f"layers.{li}."
        for n, shape in (("W_q", (A, D)), ("W_k", (A, D)), ("W_v", (A, D)), ("W_out", (D, A))):
            params[pre + n + ".weight"] = rng.uniform(-0.4, 0.4, shape).astype(np.float32)
            params[pre + n + ".bias"] = rng.uniform(-0.4, 0.4, shape[0]).astype(np.float32)
        if c["residual"]:
            params[pre + "layer_norm.weight"] = rng.uniform(0.5, 1.5, D).astype(np.float32)
            params[pre + "layer_norm.bias"] = rng.uniform(-0.4, 0.4, D).astype(np.float32)
    x = (rng.standard_normal((c["B"], c["F"], D)) * x_scale).astype(np.float32)
    up = rng.standard_normal(x.shape).astype(np.float32)
    return params, x, up


# ---- CIN: an fp64 reference that shares no code with oracle/, and the plain-bf16 emulation ----

def cin_split_layout(F: int, layer_sizes, split_half: bool):
    """(H, direct, next_off, out_col) per layer and the output width: the bookkeeping of CIN.__init__."""
    H, direct, next_off, out_col = [], [], [], []
    prev, col, last = F, 0, len(layer_sizes) - 1
    for i, c in enumerate(layer_sizes):
        d = c // 2 if (split_half and i < last) else c
        H.append(prev)
        direct.append(d)
        next_off.append(d if (split_half and i < last) else 0)
        out_col.append(col)
        col += d
        prev = c - d if (split_half and i < last) else c
    return H, direct, next_off, out_col, col


def cin_fp64(x, params: Dict[str, np.ndarray], layer_sizes, split_half: bool, upstream=None):
    """CIN in torch-CPU float64: per layer the outer product hidden (x) x0 over (h, f), the 1x1 convolution,
    ReLU, the [direct | next] split, the sum over d of the direct half; the halves concatenated.  state_dict-keyed
    arrays in and out.  Returns (out, d_x, grads, pre_activations): the gradients are autograd's on
    (out * upstream).sum() (None without an upstream), pre_activations the (B, C_i, D) inputs of every ReLU."""
    import torch
    want_grad = upstream is not None
    p = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).requires_grad_(want_grad) for k, v in params.items()}
    x0 = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(want_grad)
    B, F, D = x0.shape
    hidden, parts, pre = x0, [], []
    last = len(layer_sizes) - 1
    for i, c in enumerate(layer_sizes):
        z = (hidden[:, :, None, :] * x0[:, None, :, :]).reshape(B, -1, D)          # (B, H*F, D), k = h*F + f
        w = p[f"conv_layers.{i}.weight"].reshape(c, -1)
        a = torch.einsum("ck,bkd->bcd", w, z) + p[f"conv_layers.{i}.bias"][None, :, None]
        pre.append(a.detach().numpy())
        y = torch.relu(a)
        if split_half and i < last:
            direct, hidden = y[:, :c // 2], y[:, c // 2:]
        else:
            direct = hidden = y
        parts.append(direct.sum(dim=2))
    out = torch.cat(parts, dim=1)
    if not want_grad:
        return out.numpy(), None, None, pre
    (out * torch.from_numpy(np.asarray(upstream, dtype=np.float64))).sum().backward()
    return out.detach().numpy(), x0.grad.numpy(), {k: v.grad.numpy() for k, v in p.items()}, pre


def cin_case_inputs(case, kink_free: bool):
    """Parameters (state_dict keys, fp32), x and upstream of a matrix case (F, D, layer_sizes, split_half, B),
    seeded from the shape alone: every route and mode that runs a shape sees the same numbers.  Weights and biases
    follow Conv1d's default init, uniform in +-1/sqrt(H*F).  `kink_free`: weights x 0.25, biases +6 and, on every
    third channel, -6, x ~ 0.7 N(0, 1): every pre-activation is far from the ReLU kink (live and dead channels
    both present), so the gradient is continuous around these inputs.  Otherwise x ~ N(0, 1)."""
    F, D, sizes, split, B = case
    rng = np.random.default_rng([F, D, int(split), B, int(kink_free), *sizes])
    H = cin_split_layout(F, sizes, split)[0]
    params = {}
    for i, c in enumerate(sizes):
        k = H[i] * F
        bound = 1.0 / np.sqrt(k)
        w = rng.uniform(-bound, bound, (c, k, 1))
        b = rng.uniform(-bound, bound, c)
        if kink_free:
            w = w * 0.25
            b = np.where(np.arange(c) % 3 == 2, -6.0, 6.0)
        params[f"conv_layers.{i}.weight"] = w.astype(np.float32)
        params[f"conv_layers.{i}.bias"] = b.astype(np.float32)
    x = (rng.standard_normal((B, F, D)) * (0.7 if kink_free else 1.0)).astype(np.float32)
    up = rng.standard_normal((B, cin_split_layout(F, sizes, split)[4])).astype(np.float32)
    return params, x, up


def bf16_round(a) -> np.ndarray:
    """fp32 -> bf16 -> fp32, round to nearest even: what static_cast<__bf16>(float) does in the kernels."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def cin_bf16_emulation(x, params: Dict[str, np.ndarray], layer_sizes, split_half: bool, upstream=None):
    """What the matrix-core CIN kernels compute in plain-bf16 mode (dfm_cin_set_mode(1)), with every sum in
    fp64: both operands of each product are rounded to bf16 (nearest even) — W and Z = fp32(hidden * x0) in the
    forward, W and dY in the data gradient, dY and Z in the weight gradient (and dY times one in the bias
    gradient when it rides in a padding column, F % 8 != 0; the separate bias kernels add fp32 dY) — and whatever
    the kernels keep between two products is fp32: post-ReLU activations, dY, d hidden, the G tile.  Runs layer by
    layer on its own hidden values.  Returns dict(out, y=[(B, C_i, D) fp32], d_x, grads); the last two are None
    without an upstream."""
    x0 = np.asarray(x, dtype=np.float32)
    B, F, D = x0.shape
    H, direct, next_off, out_col, out_dim = cin_split_layout(F, layer_sizes, split_half)
    L = len(layer_sizes)
    wb = [bf16_round(params[f"conv_layers.{i}.weight"].reshape(layer_sizes[i], -1)).astype(np.float64) for i in range(L)]
    hidden, hid, zb, ys = x0, [], [], []
    out = np.zeros((B, out_dim), dtype=np.float64)
    for i, c in enumerate(layer_sizes):
        z = (hidden[:, :, None, :] * x0[:, None, :, :]).astype(np.float32).reshape(B, H[i] * F, D)
        hid.append(hidden)
        zb.append(bf16_round(z).astype(np.float64))
        a = np.einsum("ck,bkd->bcd", wb[i], zb[i]) + params[f"conv_layers.{i}.bias"].astype(np.float64)[None, :, None]
        y = np.maximum(a, 0.0).astype(np.float32)
        ys.append(y)
        out[:, out_col[i]:out_col[i] + direct[i]] = y[:, :direct[i]].astype(np.float64).sum(axis=2)
        hidden = y[:, next_off[i]:]
    r = dict(out=out, y=ys, d_x=None, grads=None)
    if upstream is None:
        return r
    up = np.asarray(upstream, dtype=np.float32)
    d_x = np.zeros((B, F, D), dtype=np.float64)
    grads, d_hidden = {}, None
    for i in reversed(range(L)):
        c = layer_sizes[i]
        g = np.zeros((B, c, D), dtype=np.float32)
        g[:, :direct[i]] = up[:, out_col[i]:out_col[i] + direct[i], None]
        if d_hidden is not None:
            g[:, next_off[i]:] += d_hidden
        dy = np.where(ys[i] > 0, g, np.float32(0))
        dyb = bf16_round(dy).astype(np.float64)
        G = np.einsum("ck,bcd->bkd", wb[i], dyb).astype(np.float32).astype(np.float64).reshape(B, H[i], F, D)
        d_hidden = (x0[:, None, :, :].astype(np.float64) * G).sum(axis=2).astype(np.float32)
        d_x += (hid[i][:, :, None, :].astype(np.float64) * G).sum(axis=1)
        if i == 0:
            d_x += d_hidden
        grads[f"conv_layers.{i}.weight"] = np.einsum("bcd,bkd->ck", dyb, zb[i])[:, :, None]
        grads[f"conv_layers.{i}.bias"] = (dyb if F % 8 else dy.astype(np.float64)).sum(axis=(0, 2))
    r.update(d_x=d_x, grads=grads)
    return r


# ---- DNN tower: fp64 restatements that share no code with the kernels or with oracle/ ----
# Every function takes numpy arrays (any float type), computes in torch-CPU float64 and returns numpy float64.

def _t64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def tower_linear_fp64(x, w, b=None):
    """z = x W^T + b."""
    z = _t64(x) @ _t64(w).T
    if b is not None:
        z = z + _t64(b)
    return z.numpy()


def tower_column_stats_fp64(z):
    """Per-column mean and biased variance."""
    t = _t64(z)
    mean = t.mean(0)
    return mean.numpy(), ((t - mean) ** 2).mean(0).numpy()


def tower_bn_relu_fp64(z, mean, rstd, gamma, beta):
    """(xhat, y, a): xhat = (z - mean) rstd, y = gamma xhat + beta, a = relu(y)."""
    import torch
    xhat = (_t64(z) - _t64(mean)) * _t64(rstd)
    y = _t64(gamma) * xhat + _t64(beta)
    return xhat.numpy(), y.numpy(), torch.relu(y).numpy()


def tower_masked_grad_fp64(g, y):
    """dy: the gradient g of relu(y) pushed through the ReLU mask."""
    return np.where(np.asarray(y, dtype=np.float64) > 0, np.asarray(g, dtype=np.float64), 0.0)


def tower_bn_backward_fp64(dy, xhat, gamma, rstd):
    """(d gamma, d beta, dz) with dz = gamma rstd (dy - mean(dy) - xhat mean(dy xhat))."""
    d, xh = _t64(dy), _t64(xhat)
    dgamma, dbeta = (d * xh).sum(0), d.sum(0)
    dz = _t64(gamma) * _t64(rstd) * (d - d.mean(0) - xh * (d * xh).mean(0))
    return dgamma.numpy(), dbeta.numpy(), dz.numpy()


def tower_linear_backward_fp64(dz, x, w, g_fm=None, fm_sum=None, e=None, addend=None):
    """(dW, dx): dW = dz^T x; dx = dz W, plus the FM term g_fm (S - e) (S repeated over the fields) and the
    addend where given."""
    d = _t64(dz)
    dW = d.T @ _t64(x)
    dx = d @ _t64(w)
    if g_fm is not None:
        S, E = _t64(fm_sum), _t64(e)
        dx = dx + _t64(g_fm)[:, None] * (S.repeat(1, E.shape[1] // S.shape[1]) - E)
    if addend is not None:
        dx = dx + _t64(addend)
    return dW.numpy(), dx.numpy()


def tower_head_fp64(a, w, b, fo, fm, labels):
    """The head: logits = (fo + fm) + (a . w + b), mean BCE-with-logits in its stable form, d logits = (sigmoid -
    y) / M, d w = sum_b d logit_b a_b, d b = sum_b d logit_b.  b, fo, fm may be None (taken as zero)."""
    import torch
    A, W = _t64(a), _t64(w).reshape(-1)
    M = A.shape[0]
    zero = torch.zeros(M, dtype=torch.float64)
    logits = ((_t64(fo) if fo is not None else zero) + (_t64(fm) if fm is not None else zero)) \
        + (A @ W + (float(np.asarray(b).reshape(-1)[0]) if b is not None else 0.0))
    y = _t64(labels)
    li = torch.clamp(logits, min=0) - logits * y + torch.log1p(torch.exp(-logits.abs()))
    dl = (torch.sigmoid(logits) - y) / M
    return dict(logits=logits.numpy(), loss=float(li.mean()), dlogits=dl.numpy(), dw=(dl[:, None] * A).sum(0).numpy(),
                db=float(dl.sum()))


_TOWER_BM = _TOWER_BN = 64
_TOWER_BK = 32


def tower_dw_splits(n_out: int, k_in: int, m: int) -> int:
    """Host restatement of tower.hip::dw_splits: the requested batch splits of the d-weight product."""
    t = -(-n_out // _TOWER_BM) * -(-k_in // _TOWER_BN)
    dx = -(-m // _TOWER_BM) * -(-k_in // _TOWER_BN)
    max_s = max(m // (4 * _TOWER_BK), 1)
    room = (dx // 512 + 1) * 512 - dx
    s = room // t
    if s < 4 and max_s >= 4:
        s = (room + 512) // t
    return max(min(s, max_s), 1)


def tower_dw_split_plan(n_out: int, k_in: int, m: int):
    """(splits, k_per_split, rows per split) actually launched: tower.hip::dw_split_plan."""
    s0 = tower_dw_splits(n_out, k_in, m)
    kps = -(-(-(-m // s0)) // _TOWER_BK) * _TOWER_BK
    splits = -(-m // kps)
    return splits, kps, [min(kps, m - i * kps) for i in range(splits)]


TOWER_GUARD = 64                  # floats on each side: the payload stays 256-byte aligned (before the shift)
TOWER_SENTINEL = -1234.5


class GuardedBuffer:
    """`n` floats on the GPU inside a larger allocation with sentinel floats on both sides.  `shift` floats
    (0 or 1) move the payload off its 16-byte alignment for the misaligned-pointer cases; `.t` is the payload."""

    def __init__(self, n, fill=float("nan"), shift=0):
        import torch
        self.n = int(n)
        self.lo = TOWER_GUARD + shift
        self.whole = torch.full((self.n + 2 * TOWER_GUARD + 4,), TOWER_SENTINEL, dtype=torch.float32, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.t = self.whole[self.lo:self.lo + self.n]
        self.t.fill_(fill)

    @classmethod
    def of(cls, array, shift=0):
        import torch
        a = np.ascontiguousarray(array, dtype=np.float32)
        b = cls(a.size, 0.0, shift)
        b.t.copy_(torch.from_numpy(a.reshape(-1)))
        return b

    def ptr(self):
        return self.t.data_ptr()

    def view(self, *shape):
        return self.t.view(*shape)

    def guards_intact(self):
        import torch
        g = torch.cat([self.whole[:self.lo], self.whole[self.lo + self.n:]]).view(torch.int32)
        want = torch.tensor([TOWER_SENTINEL], dtype=torch.float32).view(torch.int32).item()
        return bool((g == want).all())


# ---- step tail: fp64 restatements that share no code with the kernels or with oracle/ ----
# Hyper-parameters arrive as the float32 values the kernels receive (np.float32(0.999), ...) and are widened.

def tail_rowgrad_fp64(ids, g_rows, g_first):
    """One gradient row per distinct non-zero id: contributions added in sample order.  ids (n,), g_rows (n, D),
    g_first (n,).  Returns dict(rows ascending, count, g2 (U, D), g1 (U,), abs2, abs1 = the sums of |contribution|)."""
    ids = np.asarray(ids)
    keep = ids != 0
    rows, inv, count = np.unique(ids[keep], return_inverse=True, return_counts=True)
    g2 = np.asarray(g_rows, dtype=np.float64)[keep]
    g1 = np.asarray(g_first, dtype=np.float64).reshape(-1)[keep]
    out = dict(rows=rows, count=count)
    for name, src in (("g2", g2), ("abs2", np.abs(g2)), ("g1", g1), ("abs1", np.abs(g1))):
        acc = np.zeros((rows.size,) + src.shape[1:])
        np.add.at(acc, inv, src)
        out[name] = acc
    return out


def tail_dense_field_fp64(x, g):
    """A DENSE field's Linear gradients over a batch slice: x (n,), g (n, k).  Returns (sum x g, sum g, sum |x g|,
    sum |g|), each (k,)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 1)
    g = np.asarray(g, dtype=np.float64)
    g = g.reshape(x.shape[0], g.shape[-1] if g.ndim > 1 else 1)
    return (x * g).sum(0), g.sum(0), np.abs(x * g).sum(0), np.abs(g).sum(0)


def tail_merge_fp64(rows, num, g2, g1, w2, w1, grad_scale, l2):
    """Ownership merge of L lists per field.  rows (L, S, CH) ascending per list, num (L, S), g2 (L, S, CH, D),
    g1 (L, S, CH), w2[s] (V, D), w1[s] (V,).  The lowest list that holds a row owns it; the owner's gradient is
    grad_scale * (sum over the lists, in list order) + 2 l2 w.  Returns dict(owner (L, S, CH) in {0, 1, -1 = behind
    num}, g2, g1 (NaN wherever the entry is no owner), abs2, abs1 = the sums of |term|)."""
    L, S, CH = rows.shape
    D = g2.shape[-1]
    gs, k = float(grad_scale), 2.0 * float(l2)
    owner = np.full((L, S, CH), -1, dtype=np.int64)
    out = {n: np.full((L, S, CH) + ((D,) if n.endswith("2") else ()), np.nan) for n in ("g2", "g1", "abs2", "abs1")}
    for s in range(S):
        cat_rows = np.concatenate([rows[l, s, :num[l, s]] for l in range(L)])
        cat_list = np.concatenate([np.full(num[l, s], l) for l in range(L)])
        cat_g2 = np.concatenate([g2[l, s, :num[l, s]] for l in range(L)]).astype(np.float64)
        cat_g1 = np.concatenate([g1[l, s, :num[l, s]] for l in range(L)]).astype(np.float64)
        uniq, inv = np.unique(cat_rows, return_inverse=True)
        first = np.full(uniq.size, L)
        np.minimum.at(first, inv, cat_list)
        s2, a2 = np.zeros((uniq.size, D)), np.zeros((uniq.size, D))
        s1, a1 = np.zeros(uniq.size), np.zeros(uniq.size)
        np.add.at(s2, inv, cat_g2); np.add.at(a2, inv, np.abs(cat_g2))
        np.add.at(s1, inv, cat_g1); np.add.at(a1, inv, np.abs(cat_g1))
        W2 = np.asarray(w2[s], dtype=np.float64)[uniq]
        W1 = np.asarray(w1[s], dtype=np.float64).reshape(-1)[uniq]
        m2, m1 = gs * s2 + k * W2, gs * s1 + k * W1
        t2, t1 = abs(gs) * a2 + np.abs(k * W2), abs(gs) * a1 + np.abs(k * W1)
        at = 0
        for l in range(L):
            n = int(num[l, s])
            j = inv[at:at + n]
            own = first[j] == l
            owner[l, s, :n] = own
            for name, src in (("g2", m2), ("g1", m1), ("abs2", t2), ("abs1", t1)):
                v = src[j].copy()
                v[~own] = np.nan
                out[name][l, s, :n] = v
            at += n
    out["owner"] = owner
    return out


def tail_dense_prepare_fp64(g, p, n_l2, l2, slabs=(), gathered=None, scale=1.0):
    """The dense buffer's gradient before the norm: the mean over ranks in rank order (`gathered` (world, n) REPLACES
    g by scale * their sum), then every slab (offset, (splits, elems) array) in slab order, then 2 l2 p for i < n_l2.
    Returns (g, sum of |term|, number of terms) per element."""
    g = np.asarray(g, dtype=np.float64).copy()
    terms = np.ones(g.size)
    if gathered is not None:
        ga = np.asarray(gathered, dtype=np.float64)
        g = float(scale) * ga.sum(0)
        absum = abs(float(scale)) * np.abs(ga).sum(0)
        terms = np.full(g.size, float(ga.shape[0]) + 1)          # (+ 1: the product with the scale)
    else:
        absum = np.abs(g)
    for off, slab in slabs:
        sl = np.asarray(slab, dtype=np.float64)
        for q in range(sl.shape[0]):
            g[off:off + sl.shape[1]] += sl[q]
        absum[off:off + sl.shape[1]] += np.abs(sl).sum(0)
        terms[off:off + sl.shape[1]] += sl.shape[0]
    reg = 2.0 * float(l2) * np.asarray(p, dtype=np.float64)[:n_l2]
    g[:n_l2] += reg
    absum[:n_l2] += np.abs(reg)
    terms[:n_l2] += 1
    return g, absum, terms


def tail_sq_fp64(*arrays):
    """|g|^2 over every finite-or-not element handed in (NaN entries = not part of the gradient, skipped)."""
    return float(sum(np.nansum(np.asarray(a, dtype=np.float64) ** 2) for a in arrays))


def tail_clip_fp64(total_sq, max_norm):
    """clip = min(1, max_norm / (sqrt(total) + 1e-6)); max_norm <= 0: no clipping."""
    if not max_norm > 0:
        return 1.0
    return min(1.0, float(max_norm) / (float(np.sqrt(np.float64(total_sq))) + float(np.float32(1e-6))))


def tail_rule_fp64(rule, w, m, v, g, t, lr, hyper, clip=1.0):
    """One optimizer step on arrays, as the comments of csrc/tail_bodies.h state the rules.  rule: "adam"
    (torch.optim.Adam), "adamw" (p *= 1 - lr wd first, then Adam), "sgd" (buf = momentum buf + g, p -= lr buf;
    buf in the m slot, v untouched).  hyper: dict(b1, b2, eps, wd, momentum).  Returns (w, m, v) in fp64."""
    w, m, g = (np.asarray(a, dtype=np.float64) for a in (w, m, g))
    v = None if v is None else np.asarray(v, dtype=np.float64)
    lr, g = float(lr), g * float(clip)
    h = {k: float(x) for k, x in hyper.items()}
    if rule == "sgd":
        m = h["momentum"] * m + g
        return w - lr * m, m, v
    if rule == "adamw":
        w = w * (1.0 - lr * h["wd"])
    m = h["b1"] * m + (1.0 - h["b1"]) * g
    v = h["b2"] * v + (1.0 - h["b2"]) * g * g
    t = float(t)
    denom = np.sqrt(v) / np.sqrt(1.0 - h["b2"] ** t) + h["eps"]
    return w - (lr / (1.0 - h["b1"] ** t)) * (m / denom), m, v


# ---- record gather / record backward: restatements from the operation's definition ----
# FeatureEmbedding of the reference (per field: SPARSE row lookup, DENSE Linear(1, d) and Linear(1, 1), SEQUENCE
# EmbeddingBag with padding id 0; a bias-free projection to fm_dim where d != fm_dim; first_order = sum of the
# first-order parts, field_embeddings stacked, flat_embeddings concatenated) and FMInteraction (0.5 sum_d (S^2 - sum_f
# e^2), d e = g_fm (S - e)).  Plain numpy, no slices, no tiles, nothing of the kernels' bookkeeping.  Beside every
# value the functions return A = the sum of the absolute values of the terms that make it up and n = the length of the
# longest chain of additions that reaches it: the matrix's bars are c * eps32 * sqrt(n) * A (tests/record_cases.py).
# `dt` / `order` exist for the bars' calibration only: the same statements evaluated in float32 with every sum taken
# sequentially ("seq") or pairwise ("pair").

def _rec_sum(x, axis, dt, order):
    if dt == np.float64:
        return x.sum(axis=axis)
    if order == "seq":
        return np.take(np.cumsum(x, axis=axis, dtype=dt), -1, axis=axis)
    return np.ascontiguousarray(np.moveaxis(x, axis, -1)).sum(-1, dtype=dt)


def _rec_scatter(shape, idx, vals, dt=np.float64, order="seq"):
    """out[idx] += vals with repeated indices accumulating, in the order given (one np.add.at); "pair": 16 blocks of
    the contributions summed one by one, the blocks by a tree."""
    if dt == np.float64 or order == "seq" or len(vals) < 32:
        out = np.zeros(shape, dtype=dt)
        np.add.at(out, idx, vals)
        return out
    edges = np.linspace(0, len(vals), 17).astype(np.int64)
    parts = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        p = np.zeros(shape, dtype=dt)
        np.add.at(p, tuple(i[lo:hi] for i in idx), vals[lo:hi])
        parts.append(p)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0]


def _rec_pool(table, ids, combiner, dt, order):
    """EmbeddingBag(mode=combiner, padding_idx=0): (pooled (B, d), A, n (B,)).  id 0 is left out of the reduction and of
    the mean's divisor; an all-padding bag pools to 0."""
    rows = table[ids]                                        # (B, L, d)
    valid = ids != 0
    count = valid.sum(axis=1)
    if combiner == "max":
        val = np.where(valid[:, :, None], rows, -np.inf).max(axis=1)
        val = np.where(count[:, None] == 0, 0.0, val).astype(dt)
        return val, np.abs(val), np.ones(ids.shape[0])
    mask = valid[:, :, None].astype(dt)
    s = _rec_sum(rows * mask, 1, dt, order)
    A = (np.abs(rows) * mask).sum(axis=1)
    if combiner == "mean":
        den = np.maximum(count, 1).astype(dt)[:, None]
        return s / den, A / den, count + 1.0
    if combiner != "sum":
        raise ValueError(combiner)
    return s, A, np.maximum(count, 1).astype(np.float64)


def _rec_keys(name):
    return (f"second_order_embeddings.{name}.weight", f"first_order_embeddings.{name}.weight",
            f"second_order_embeddings.{name}.bias", f"first_order_embeddings.{name}.bias", f"projections.{name}.weight")


def record_forward_fp64(fields, params, batch, fm_dim, dt=np.float64, order="seq"):
    """FeatureEmbedding.forward + FMInteraction.  Returns a dict with first_order (B,), field_embeddings (B, F, fm_dim),
    flat_embeddings (B, sum d), fm (B,), fm_sum (B, fm_dim) and, under "A" and "n", dicts of the same keys and shapes
    (n broadcastable)."""
    c = lambda a: np.asarray(a, dtype=dt)
    F, D = len(fields), int(fm_dim)
    fo, fo_A, fo_n, e, e_A, e_n, raw_l, raw_A, raw_n = ([] for _ in range(9))
    for spec in fields:
        name, kind, d = spec["name"], spec["type"], spec["dim"]
        k2, k1, kb2, kb1, kp = _rec_keys(name)
        w2, w1, x = c(params[k2]), c(params[k1]), batch[name]
        if kind == "dense":
            xv = c(x)[:, None]
            t2, b2 = xv * w2[:, 0][None, :], c(params[kb2])[None, :]
            t1, b1 = xv[:, 0] * w1[0, 0], c(params[kb1])[0]
            r, rA, rn = t2 + b2, np.abs(t2) + np.abs(b2), np.full(len(x), 2.0)
            o, oA, on = t1 + b1, np.abs(t1) + np.abs(b1), np.full(len(x), 2.0)
        elif kind == "sparse":
            r, o = w2[x], w1[x, 0]
            rA, oA, rn, on = np.abs(r), np.abs(o), np.ones(len(x)), np.ones(len(x))
        elif kind == "sequence":
            r, rA, rn = _rec_pool(w2, x, spec["combiner"], dt, order)
            o, oA, on = _rec_pool(w1, x, spec["combiner"], dt, order)
            o, oA = o[:, 0], oA[:, 0]
        else:
            raise ValueError(kind)
        assert r.shape[1] == d
        raw_l.append(r); raw_A.append(rA); raw_n.append(np.broadcast_to(rn[:, None], r.shape))
        fo.append(o); fo_A.append(oA); fo_n.append(on)
        if kp in params:
            P = c(params[kp])                                 # (fm_dim, d): Linear(d, fm_dim, bias=False).weight
            e.append(_rec_sum(r[:, None, :] * P[None], 2, dt, order))
            e_A.append((rA[:, None, :] * np.abs(P)[None]).sum(axis=2))
            e_n.append(rn + d)
        else:
            assert d == D, f"field {name}: dim {d} != fm_dim {D} without a projection"
            e.append(r); e_A.append(rA); e_n.append(rn)
    fe, fe_A = np.stack(e, axis=1), np.stack(e_A, axis=1)
    fe_n = np.stack(e_n, axis=1)                              # (B, F)
    S, S_A, S_n = _rec_sum(fe, 1, dt, order), fe_A.sum(axis=1), F + fe_n.max(axis=1)
    sq = _rec_sum(fe * fe, 1, dt, order)
    half = np.asarray(0.5, dtype=dt)
    out = dict(first_order=_rec_sum(np.stack(fo, axis=1), 1, dt, order), field_embeddings=fe,
               flat_embeddings=np.concatenate(raw_l, axis=1), fm=half * _rec_sum(S * S - sq, 1, dt, order), fm_sum=S)
    out["A"] = dict(first_order=np.stack(fo_A, axis=1).sum(axis=1), field_embeddings=fe_A,
                    flat_embeddings=np.concatenate(raw_A, axis=1),
                    fm=0.5 * (S_A ** 2 + (fe_A ** 2).sum(axis=1)).sum(axis=1), fm_sum=S_A)
    out["n"] = dict(first_order=F + np.stack(fo_n, axis=1).max(axis=1), field_embeddings=fe_n[:, :, None],
                    flat_embeddings=np.concatenate(raw_n, axis=1), fm=S_n + D, fm_sum=S_n[:, None])
    return out


def record_backward_fp64(fields, params, batch, fm_dim, g_first, g_field, g_flat, g_fm=None, saved=None,
                         dt=np.float64, order="seq"):
    """The gradient of every parameter of FeatureEmbedding from the upstream gradients of first_order (B,),
    field_embeddings (B, F, fm_dim; None: 0) and flat_embeddings (B, sum d), plus g_fm (B,) of the FM value: d e =
    g_field + g_fm (S - e).  `saved`: the forward's field_embeddings, fm_sum and flat_embeddings as the caller holds them
    (default: this module's own forward).  Max bags send each column's gradient to the first position that holds the
    maximum.  Returns dict(grads, A, n) keyed like a state_dict; row 0 of a table gets no gradient."""
    c = lambda a: np.asarray(a, dtype=dt)
    F, D = len(fields), int(fm_dim)
    if saved is None:
        saved = record_forward_fp64(fields, params, batch, fm_dim, dt, order)
    fe, S, flat = c(saved["field_embeddings"]), c(saved["fm_sum"]), c(saved["flat_embeddings"])
    B = fe.shape[0]
    ge, ge_A, ge_n = np.zeros((B, F, D), dtype=dt), np.zeros((B, F, D)), 0
    if g_field is not None:
        ge, ge_A, ge_n = c(g_field).reshape(B, F, D), np.abs(c(g_field).reshape(B, F, D)).astype(np.float64), 1
    if g_fm is not None:
        gm = c(g_fm).reshape(B, 1, 1)
        ge = ge + gm * (S[:, None, :] - fe)
        ge_A = ge_A + np.abs(gm) * (np.abs(S)[:, None, :] + np.abs(fe))
        ge_n += 2
    g1 = c(g_first).reshape(B)
    gfl = c(g_flat)
    grads, A, n = {}, {}, {}

    def put(key, val, a, terms):
        grads[key], A[key], n[key] = val, np.asarray(a, dtype=np.float64), np.broadcast_to(np.asarray(terms, dtype=np.float64), val.shape)

    off = 0
    for f, spec in enumerate(fields):
        name, kind, d = spec["name"], spec["type"], spec["dim"]
        k2, k1, kb2, kb1, kp = _rec_keys(name)
        gr, gr_A = gfl[:, off:off + d], np.abs(gfl[:, off:off + d]).astype(np.float64)
        if kp in params:
            P, raw = c(params[kp]), flat[:, off:off + d]
            gr = gr + _rec_sum(ge[:, f, :, None] * P[None], 1, dt, order)
            gr_A = gr_A + (ge_A[:, f, :, None] * np.abs(P)[None]).sum(axis=1)
            gr_n = 1 + D + ge_n
            put(kp, _rec_sum(ge[:, f, :, None] * raw[:, None, :], 0, dt, order),
                (ge_A[:, f, :, None] * np.abs(raw)[:, None, :]).sum(axis=0), B + ge_n)
        else:
            gr, gr_A, gr_n = gr + ge[:, f, :], gr_A + ge_A[:, f, :], 1 + ge_n
        off += d
        x = batch[name]
        if kind == "dense":
            xv = c(x)[:, None]
            put(k2, _rec_sum(xv * gr, 0, dt, order)[:, None], (np.abs(xv) * gr_A).sum(axis=0)[:, None], B + gr_n)
            put(kb2, _rec_sum(gr, 0, dt, order), gr_A.sum(axis=0), B + gr_n)
            put(k1, _rec_sum(xv[:, 0] * g1, 0, dt, order).reshape(1, 1), np.abs(xv[:, 0] * g1).sum().reshape(1, 1), B + 1)
            put(kb1, _rec_sum(g1, 0, dt, order).reshape(1), np.abs(g1).sum().reshape(1), B)
            continue
        V = spec["vocab"]
        if kind == "sparse":
            keep = x != 0
            i2, v2, i1, v1, extra = (x[keep],), gr[keep], (x[keep],), g1[keep], 0
            a2, a1 = gr_A[keep], np.abs(v1)
        elif spec["combiner"] in ("mean", "sum"):
            valid = x != 0
            count = np.maximum(valid.sum(axis=1), 1).astype(dt)
            scale = 1.0 / count if spec["combiner"] == "mean" else np.ones_like(count)
            bsel, lsel = np.nonzero(valid)                    # (sample, position) order
            i2, v2, a2 = (x[bsel, lsel],), gr[bsel] * scale[bsel, None], gr_A[bsel] * scale[bsel, None]
            i1, v1 = i2, g1[bsel] * scale[bsel]
            a1, extra = np.abs(v1), int(spec["combiner"] == "mean")
        else:
            valid = x != 0
            live = valid.any(axis=1)
            w2, w1 = c(params[k2]), c(params[k1])
            arg2 = np.where(valid[:, :, None], w2[x], -np.inf).argmax(axis=1)          # (B, d): the first maximum
            arg1 = np.where(valid, w1[x, 0], -np.inf).argmax(axis=1)                   # (B,)
            bb, jj = np.nonzero(np.broadcast_to(live[:, None], arg2.shape))
            i2, v2, a2 = (x[bb, arg2[bb, jj]], jj), gr[bb, jj], gr_A[bb, jj]
            b1 = np.nonzero(live)[0]
            i1, v1 = (x[b1, arg1[b1]],), g1[b1]
            a1, extra = np.abs(v1), 0
        cnt2 = _rec_scatter((V, d) if len(i2) == 2 else (V,), i2, np.ones(len(v2)))
        cnt2 = cnt2 if cnt2.ndim == 2 else cnt2[:, None]
        cnt1 = _rec_scatter((V,), i1, np.ones(len(v1)))
        put(k2, _rec_scatter((V, d), i2, v2, dt, order), _rec_scatter((V, d), i2, a2),
            np.where(cnt2 > 0, cnt2 + gr_n + extra, 0))
        put(k1, _rec_scatter((V,), i1, v1, dt, order)[:, None], _rec_scatter((V,), i1, a1)[:, None],
            np.where(cnt1 > 0, cnt1 + 1 + extra, 0)[:, None])
    return dict(grads=grads, A=A, n=n)
