"""Multi-head self-attention over feature fields on MI355X
(reference ``deepfm/models/layers/attention.py:11-120``).

Same constructor (``ValueError`` when ``attention_dim % num_heads``), same ``forward((B,F,D)) -> (B,F,D)`` and the
same ``state_dict`` layout (``layers.<i>.{W_q,W_k,W_v,W_out}.{weight,bias}``, ``layers.<i>.layer_norm.*`` with
``use_residual``).  ``_AttentionBlock`` keeps ``nn.Linear`` / ``nn.LayerNorm`` parameter holders (PyTorch default
init, like the reference) whose forward is never called.

``block_route`` names the route of a block.  What each launches (LayerNorm only with ``use_residual``; every backward
of the first three ends in the streamed weight-gradient pass and one ``dfm_partials_finish``):

whole_block   ``dfm_attention_block_forward``: projection, core, W_out and residual LayerNorm in one launch.
              Backward: LayerNorm, ``dfm_attention_block_backward`` (d O, core and d x in one launch).
qkv_inside    ``dfm_attention_qkv_core_forward`` (Q|K|V never materialised), W_out GEMM, ``dfm_layernorm_forward``.
              Backward: LayerNorm, d O GEMM, ``dfm_attention_qkv_core_backward``, d x GEMM.
gemm_core     as qkv_inside with a Q|K|V GEMM and ``dfm_attention_core_forward`` / ``_backward`` (matrix-core or
              vector kernel: the library's choice).
per_sample    ``dfm_attention_forward`` / ``_backward``: one LDS kernel per sample (csrc/attention.hip), ``_AttnFn``.

The first three are ``block_forward`` / ``block_backward``: plain functions with their options as keyword arguments,
called directly by the fused training steps and the predictor, and wrapped by ``_AttnGemmFn`` for autograd.
"""

from __future__ import annotations

import dataclasses
import math

import torch
from typing import Optional
import torch.nn as nn

from deepfm_amd import _lib


class _AttentionBlock(nn.Module):
    def __init__(self, embed_dim: int, num_heads: int, attention_dim: int, use_residual: bool) -> None:
        super().__init__()
        self.embed_dim, self.attention_dim = embed_dim, attention_dim
        self.num_heads = num_heads
        self.head_dim = attention_dim // num_heads
        self.scale = math.sqrt(self.head_dim)
        self.use_residual = use_residual
        self.W_q = nn.Linear(embed_dim, attention_dim)
        self.W_k = nn.Linear(embed_dim, attention_dim)
        self.W_v = nn.Linear(embed_dim, attention_dim)
        self.W_out = nn.Linear(attention_dim, embed_dim)
        if use_residual:
            self.layer_norm = nn.LayerNorm(embed_dim)
        # projections as GEMMs over the B*F rows (dfm_gemm_f32) + per-(sample, head) core kernel;
        # False (or an unsupported shape) selects the single fused LDS kernel of csrc/attention.hip
        self.gemm_path = True
        # the forward as ONE kernel where its shape allows (4 heads of 16); False: core + GEMM + LayerNorm launches
        self.whole_block_kernel = True

    def adjacent_parameters(self):
        """Parameters an optimizer with ONE flat buffer should lay out back to back, in this order: the
        kernels take W_q | W_k | W_v as one stacked (3A, D) weight, and with this layout the stack is a
        view of the parameters (and of their gradients) instead of a torch.cat per step."""
        return [[self.W_q.weight, self.W_k.weight, self.W_v.weight], [self.W_q.bias, self.W_k.bias, self.W_v.bias]]

    def _param_list(self):
        ps = [self.W_q.weight, self.W_q.bias, self.W_k.weight, self.W_k.bias, self.W_v.weight,
              self.W_v.bias, self.W_out.weight, self.W_out.bias]
        if self.use_residual:
            ps += [self.layer_norm.weight, self.layer_norm.bias]
        return ps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        fn = _AttnFn if block_route(self, x.shape[1]) == "per_sample" else _AttnGemmFn
        return fn.apply(self, x, *self._param_list())


class MultiHeadSelfAttention(nn.Module):
    def __init__(self, embed_dim: int, num_heads: int = 4, attention_dim: int = 64, num_layers: int = 1,
                 use_residual: bool = True) -> None:
        super().__init__()
        self.embed_dim, self.num_heads, self.attention_dim = embed_dim, num_heads, attention_dim
        self.head_dim = attention_dim // num_heads
        self.use_residual = use_residual
        if attention_dim % num_heads != 0:
            raise ValueError(f"attention_dim ({attention_dim}) must be divisible by num_heads ({num_heads})")
        self.layers = nn.ModuleList(
            _AttentionBlock(embed_dim, num_heads, attention_dim, use_residual) for _ in range(num_layers))

    def forward(self, field_embeddings: torch.Tensor) -> torch.Tensor:
        if field_embeddings.dim() != 3 or field_embeddings.shape[2] != self.embed_dim:
            raise ValueError(f"expected (B, F, {self.embed_dim}), got {tuple(field_embeddings.shape)}")
        _lib.require_device(field_embeddings, "field_embeddings")
        x = field_embeddings.float()
        for block in self.layers:
            x = block(x)
        return x


def stacked_view(ts) -> "torch.Tensor | None":
    """(sum of rows, cols) view over tensors that lie back to back in one storage (RowSparseAdam lays
    W_q | W_k | W_v out that way, see ``_AttentionBlock.adjacent_parameters``), else None."""
    t0 = ts[0]
    cols = t0.shape[1] if t0.dim() == 2 else 1
    nxt, store = t0.data_ptr(), t0.untyped_storage().data_ptr()
    for t in ts:
        # same storage, not merely neighbouring allocations: the view must stay inside one storage
        if not t.is_contiguous() or t.data_ptr() != nxt or t.untyped_storage().data_ptr() != store \
                or t.dtype != t0.dtype or (t.shape[1] if t.dim() == 2 else 1) != cols:
            return None
        nxt += t.numel() * t.element_size()
    rows = sum(t.shape[0] for t in ts)
    return torch.as_strided(t0, (rows, cols) if t0.dim() == 2 else (rows,), (cols, 1) if t0.dim() == 2 else (1,))


def gemm_shape_fault(F: int, D: int, A: int, H: int) -> Optional[str]:
    """What keeps a block's shape off the GEMM routes: "dims" (embed_dim / attention_dim), "core" (the attention
    core kernel's shapes), or None."""
    if D % 4 or A % 4 or D > 64:
        return "dims"
    return None if _lib.load().dfm_attention_core_supported(F, A, H) else "core"


def block_route(block: _AttentionBlock, F: int, *, aligned: bool = True, w_out_aligned: bool = True) -> str:
    """The route of ``block`` over ``F`` fields (table in the module docstring).  ``aligned``: x, W_qkv and b_qkv
    lie on 16-byte boundaries; ``w_out_aligned``: W_out does."""
    D, A, H = block.embed_dim, block.attention_dim, block.num_heads
    if not block.gemm_path or gemm_shape_fault(F, D, A, H):
        return "per_sample"
    lib = _lib.load()
    if block.whole_block_kernel and aligned and w_out_aligned and lib.dfm_attention_block_supported(F, D, A, H):
        return "whole_block"
    if aligned and lib.dfm_attention_qkv_core_supported(F, D, A, H):
        return "qkv_inside"
    return "gemm_core"


def _weight_grad(g: torch.Tensor, x: torch.Tensor, rows: int, n1: int, n2: int, d_w: torch.Tensor,
                 d_b: torch.Tensor, finish: list) -> bool:
    """dW = g^T x and db = column sums of g in one streamed pass (csrc/gemm_skinny.hip) when the shape is one the
    kernel takes; False -> the caller uses the general GEMM (+ a ones-column GEMM).  The reduction of the pass's
    partial sums is appended to ``finish`` as a job for ``_finish_partials`` (one launch for all of a block's)."""
    lib = _lib.load()
    ws_bytes = lib.dfm_weight_grad_workspace_bytes(rows, n1, n2)
    if not ws_bytes:
        return False
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=g.device)
    _lib.check(lib.dfm_weight_grad_partials_f32(g.data_ptr(), n1, x.data_ptr(), n2, rows, n1, n2, ws.data_ptr(),
                                                _lib.stream_handle()))
    finish.append(dict(kind=0, blocks=lib.dfm_weight_grad_partial_blocks(rows), n1=n1, n2=n2, accumulate=0,
                       partial=ws, out_w=d_w.data_ptr(), out_b=d_b.data_ptr(), ldw=n2))
    return True


def _weight_grad_pair(ga, xa, n1a, n2a, dwa, dba, gb, xb, n1b, n2b, dwb, dbb, rows: int, finish: list) -> bool:
    """Two ``_weight_grad`` streamed passes over the same ``rows`` as one launch; False when the library has no joint
    kernel for the two shapes (nothing was enqueued)."""
    lib = _lib.load()
    wa, wb = lib.dfm_weight_grad_workspace_bytes(rows, n1a, n2a), lib.dfm_weight_grad_workspace_bytes(rows, n1b, n2b)
    if not wa or not wb:
        return False
    ws_a = torch.empty(wa // 4, dtype=torch.float32, device=ga.device)
    ws_b = torch.empty(wb // 4, dtype=torch.float32, device=ga.device)
    rc = lib.dfm_weight_grad_partials_pair_f32(ga.data_ptr(), n1a, xa.data_ptr(), n2a, n1a, n2a, ws_a.data_ptr(),
                                               gb.data_ptr(), n1b, xb.data_ptr(), n2b, n1b, n2b, ws_b.data_ptr(), rows,
                                               _lib.stream_handle())
    if rc == _lib.ERR_UNSUPPORTED:
        return False
    _lib.check(rc)
    blocks = lib.dfm_weight_grad_partial_blocks(rows)
    for n1, n2, ws, dw, db in ((n1a, n2a, ws_a, dwa, dba), (n1b, n2b, ws_b, dwb, dbb)):
        finish.append(dict(kind=0, blocks=blocks, n1=n1, n2=n2, accumulate=0, partial=ws, out_w=dw.data_ptr(),
                           out_b=db.data_ptr(), ldw=n2))
    return True


def _finish_partials(jobs: list) -> None:
    """The deferred reductions of a backward pass (weight-gradient partials, LayerNorm partials) in ONE launch."""
    if not jobs:
        return
    arr = (_lib.PartialJob * len(jobs))()
    for a, j in zip(arr, jobs):
        a.kind, a.blocks, a.n1, a.n2, a.accumulate = j["kind"], j["blocks"], j["n1"], j["n2"], j["accumulate"]
        a.partial, a.out_w, a.out_b, a.ldw = j["partial"].data_ptr(), j["out_w"], j["out_b"], j["ldw"]
    _lib.check(_lib.load().dfm_partials_finish(arr, len(jobs), _lib.stream_handle()))


@dataclasses.dataclass
class BlockSaved:
    """What ``block_forward`` leaves for ``block_backward``."""
    route: str
    whole_backward: bool       # the backward runs dfm_attention_block_backward
    dims: tuple                # (B, F, D, A, H)
    tensors: tuple             # (X, qkv or None, o, y, stats, w_qkv, b_qkv, wo, gamma)
    x_copied: bool = False     # x_copy_into was honoured (the whole-block kernel only)


@dataclasses.dataclass
class BlockGrads:
    d_x: torch.Tensor          # (B, F, D)
    params: Optional[tuple]    # in _param_list() order; None: written into the parameters' .grad
    tail_done: bool            # grad_tail was added in the kernel's one store of d x


def block_forward(block: _AttentionBlock, x: torch.Tensor, params=None, *, out_into=None, x_copy_into=None):
    """One _AttentionBlock on a GEMM route -> (out, BlockSaved).  ``out_into`` = (buffer, floats between samples): the
    output goes straight into a wider per-sample layout (the DNN's concatenated input) and ``out`` is that buffer, else
    ``out`` is (B, F, D); only the residual LayerNorm can write that way.  ``x_copy_into`` = (address, floats between
    samples) of a second home of the input rows: the whole-block kernel writes it on its way (``saved.x_copied``), on
    the other routes the caller copies."""
    from deepfm_amd.models.layers.dnn import _gemm
    if out_into is not None and not block.use_residual:
        raise ValueError("out_into needs a block with residual: only its LayerNorm writes a strided output")
    lib = _lib.load()
    params = block._param_list() if params is None else params
    x = x.contiguous()
    B, F, D = x.shape
    A, H, M = block.attention_dim, block.num_heads, B * F
    wq, bq, wk, bk, wv, bv, wo, bo = (p.contiguous() for p in params[:8])
    w_qkv = stacked_view([wq, wk, wv])                          # (3A, D): a view when the optimizer laid them out so
    b_qkv = stacked_view([bq, bk, bv])
    if w_qkv is None or b_qkv is None:
        w_qkv, b_qkv = torch.cat([wq, wk, wv], dim=0), torch.cat([bq, bk, bv], dim=0)
    X = x.view(M, D)
    aligned = X.data_ptr() % 16 == 0 and w_qkv.data_ptr() % 16 == 0 and b_qkv.data_ptr() % 16 == 0
    route = block_route(block, F, aligned=aligned, w_out_aligned=wo.data_ptr() % 16 == 0)
    if route == "per_sample":
        raise ValueError("block_forward takes the GEMM routes only (block_route says 'per_sample': _AttnFn)")
    # The backward takes the whole-block kernel whenever the projection ran inside and the block kernel takes the
    # shape: also after a qkv_inside forward that only a misaligned W_out forced.  Kept as it has always been.
    whole_backward = route == "whole_block" or (route == "qkv_inside" and block.whole_block_kernel
                                                and lib.dfm_attention_block_supported(F, D, A, H) == 1)
    f32 = dict(dtype=torch.float32, device=x.device)
    o, y = torch.empty(M, A, **f32), torch.empty(M, D, **f32)
    qkv = gamma = beta = stats = None
    out, ld, eps = y, 0, 0.0
    if block.use_residual:
        gamma, beta, eps = params[8].contiguous(), params[9].contiguous(), float(block.layer_norm.eps)
        stats = torch.empty(M, 2, **f32)
        out, ld = out_into if out_into is not None else (torch.empty(M, D, **f32), 0)
    if route == "whole_block":      # ONE launch: projection, softmax(QK^T)V, W_out, bias, residual LayerNorm
        xc = x_copy_into or (None, 0)
        _lib.check(lib.dfm_attention_block_forward(
            X.data_ptr(), w_qkv.data_ptr(), b_qkv.data_ptr(), wo.data_ptr(), bo.data_ptr(), _lib.ptr(gamma),
            _lib.ptr(beta), eps, B, F, D, A, H, o.data_ptr(), y.data_ptr(), out.data_ptr(), _lib.ptr(stats), ld,
            xc[0], xc[1], _lib.stream_handle()))
    else:
        if route == "qkv_inside":   # the (M, 3A) Q|K|V is never materialised
            _lib.check(lib.dfm_attention_qkv_core_forward(X.data_ptr(), w_qkv.data_ptr(), b_qkv.data_ptr(), B, F, D, A,
                                                          H, o.data_ptr(), _lib.stream_handle()))
        else:
            qkv = torch.empty(M, 3 * A, **f32)
            _gemm(X, D, True, w_qkv, D, True, qkv, M, 3 * A, D, bias=b_qkv)
            _lib.check(lib.dfm_attention_core_forward(qkv.data_ptr(), B, F, A, H, o.data_ptr(), _lib.stream_handle()))
        _gemm(o, A, True, wo, A, True, y, M, D, A, bias=bo)
        if block.use_residual:
            _lib.check(lib.dfm_layernorm_forward(
                y.data_ptr(), X.data_ptr(), M, D, gamma.data_ptr(), beta.data_ptr(), eps, out.data_ptr(),
                stats.data_ptr(), F if out_into is not None else 0, ld, _lib.stream_handle()))
    saved = BlockSaved(route, whole_backward, (B, F, D, A, H), (X, qkv, o, y, stats, w_qkv, b_qkv, wo, gamma),
                       x_copied=route == "whole_block" and x_copy_into is not None)
    return (out if out_into is not None else out.view(B, F, D)), saved


def block_backward(block: _AttentionBlock, saved: BlockSaved, g: torch.Tensor, *, direct: bool = False,
                   g_stride: int = 0, grad_tail: Optional[dict] = None) -> BlockGrads:
    """The backward of ``block_forward``.  ``direct``: parameter gradients are written straight into the (zeroed) .grad
    views of the optimizer's flat buffer — no temporaries, no adds — where that buffer is laid out for it (else they
    are returned, as without).  ``g_stride``: ``g`` lives in a wider per-sample layout, that many floats between
    samples; only the residual LayerNorm's backward can read it that way.  ``grad_tail`` = dict(out, g_flat, ld_flat,
    g_fm, fm_sum): the other gradients of the field embeddings, added in the whole-block kernel's one store of d x
    into ``out`` (``tail_done``); a backward on another route leaves them to the caller (``tail_done`` False)."""
    from deepfm_amd.models.layers.dnn import _gemm
    from deepfm_amd.models.layers.linear import ones_column
    if g_stride and not block.use_residual:
        raise ValueError("g_stride needs a block with residual: only its LayerNorm backward reads a strided gradient")
    lib = _lib.load()
    B, F, D, A, H = saved.dims
    M = B * F
    X, qkv, o, y, stats, w_qkv, b_qkv, wo, gamma = saved.tensors
    f32 = dict(dtype=torch.float32, device=X.device)
    gq = gb = None
    if direct:
        gq = stacked_view([block.W_q.weight.grad, block.W_k.weight.grad, block.W_v.weight.grad])
        gb = stacked_view([block.W_q.bias.grad, block.W_k.bias.grad, block.W_v.bias.grad])
        direct = gq is not None and gb is not None and block.W_out.weight.grad.is_contiguous()
    if not g_stride:
        g = g.contiguous().view(M, D)
    finish: list = []          # deferred reductions of this block's backward: ONE launch at its end
    g_y = g                    # d y: without residual the incoming gradient itself
    if block.use_residual:
        g_y = torch.empty(M, D, **f32)
        if direct:                           # accumulated into: zero at this point of the step
            d_gamma, d_beta = block.layer_norm.weight.grad, block.layer_norm.bias.grad
        else:
            d_gamma, d_beta = torch.zeros(D, **f32), torch.zeros(D, **f32)
        ws = torch.empty(max(lib.dfm_layernorm_workspace_bytes(M, D) // 4, 1), **f32)
        # d gamma / d beta: the partial planes stay in ws, added by the block's one finish launch below
        _lib.check(lib.dfm_layernorm_backward(g.data_ptr(), y.data_ptr(), X.data_ptr(), stats.data_ptr(), M, D,
                                              gamma.data_ptr(), g_y.data_ptr(), None, None, ws.data_ptr(),
                                              F if g_stride else 0, g_stride, _lib.stream_handle()))
        finish.append(dict(kind=1, blocks=lib.dfm_layernorm_partial_blocks(M), n1=D, n2=0, accumulate=1,
                           partial=ws, out_w=d_gamma.data_ptr(), out_b=d_beta.data_ptr(), ldw=0))
    d_wo = block.W_out.weight.grad if direct else torch.empty(D, A, **f32)
    d_bo = block.W_out.bias.grad.view(D, 1) if direct else torch.empty(D, 1, **f32)
    d_qkv = torch.empty(M, 3 * A, **f32)
    d_wqkv = gq if direct else torch.empty(3 * A, D, **f32)
    d_bqkv = gb.view(3 * A, 1) if direct else torch.empty(3 * A, 1, **f32)
    tail = grad_tail if saved.whole_backward else None
    if saved.whole_backward:                                                 # dO, the core and dX in one launch
        d_x = tail["out"].view(M, D) if tail else torch.empty(M, D, **f32)
        t = (tail["g_flat"], tail["ld_flat"], tail["g_fm"], tail["fm_sum"]) if tail else (None, 0, None, None)
        _lib.check(lib.dfm_attention_block_backward(
            X.data_ptr(), w_qkv.data_ptr(), b_qkv.data_ptr(), wo.data_ptr(), g_y.data_ptr(), int(block.use_residual),
            B, F, D, A, H, d_qkv.data_ptr(), d_x.data_ptr(), *t, _lib.stream_handle()))
    else:
        d_o = torch.empty(M, A, **f32)
        _gemm(g_y, D, True, wo, A, False, d_o, M, A, D)                      # dO = g_y Wo
        if qkv is None:                                                      # Q, K, V recomputed from X in-kernel
            _lib.check(lib.dfm_attention_qkv_core_backward(X.data_ptr(), w_qkv.data_ptr(), b_qkv.data_ptr(),
                                                           d_o.data_ptr(), B, F, D, A, H, d_qkv.data_ptr(),
                                                           _lib.stream_handle()))
        else:
            _lib.check(lib.dfm_attention_core_backward(qkv.data_ptr(), d_o.data_ptr(), B, F, A, H,
                                                       d_qkv.data_ptr(), _lib.stream_handle()))
    # dWqkv = dQKV^T X and dWo = g_y^T O (+ their bias gradients): both streamed passes in one launch when the pair
    # of shapes has a joint kernel, their reductions and the LayerNorm's in the block's one finish launch
    if not _weight_grad_pair(d_qkv, X, 3 * A, D, d_wqkv, d_bqkv, g_y, o, D, A, d_wo, d_bo, M, finish):
        if not _weight_grad(g_y, o, M, D, A, d_wo, d_bo, finish):
            _gemm(g_y, D, False, o, A, False, d_wo, D, A, M)
            _gemm(g_y, D, False, ones_column(M, X.device), 1, False, d_bo, D, 1, M)
        if not _weight_grad(d_qkv, X, M, 3 * A, D, d_wqkv, d_bqkv, finish):
            _gemm(d_qkv, 3 * A, False, X, D, False, d_wqkv, 3 * A, D, M)
            _gemm(d_qkv, 3 * A, False, ones_column(M, X.device), 1, False, d_bqkv, 3 * A, 1, M)
    _finish_partials(finish)
    if not saved.whole_backward:
        d_x = g_y if block.use_residual else torch.empty(M, D, **f32)       # residual branch, then +=
        _gemm(d_qkv, 3 * A, True, w_qkv, D, False, d_x, M, D, 3 * A, accumulate=block.use_residual)
    grads = None
    if not direct:
        d_bqkv = d_bqkv.view(-1)
        grads = (d_wqkv[:A], d_bqkv[:A], d_wqkv[A:2 * A], d_bqkv[A:2 * A], d_wqkv[2 * A:], d_bqkv[2 * A:],
                 d_wo, d_bo.view(-1)) + ((d_gamma, d_beta) if block.use_residual else ())
    return BlockGrads(d_x.view(B, F, D), grads, tail is not None)


class _AttnGemmFn(torch.autograd.Function):
    """``block_forward`` / ``block_backward`` under autograd (``save_for_backward`` keeps its in-place check)."""

    @staticmethod
    def forward(ctx, block: _AttentionBlock, x: torch.Tensor, *params):
        out, saved = block_forward(block, x, params)
        ctx.save_for_backward(*saved.tensors)
        ctx.block, ctx.saved = block, dataclasses.replace(saved, tensors=())
        return out

    @staticmethod
    def backward(ctx, g_out: torch.Tensor):
        r = block_backward(ctx.block, dataclasses.replace(ctx.saved, tensors=ctx.saved_tensors), g_out)
        return (None, r.d_x) + r.params


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, block: _AttentionBlock, x: torch.Tensor, *params):
        x = x.contiguous()
        B, F, D = x.shape
        params = [p.contiguous() for p in params]
        out = torch.empty_like(x)
        _lib.check(_lib.load().dfm_attention_forward(
            x.data_ptr(), B, F, D, block.attention_dim, block.num_heads, int(block.use_residual),
            _lib.ptrs(params), out.data_ptr(), _lib.stream_handle()))
        ctx.block = block
        ctx.save_for_backward(x, *params)
        return out

    @staticmethod
    def backward(ctx, g_out: torch.Tensor):
        lib = _lib.load()
        block = ctx.block
        x, *params = ctx.saved_tensors
        B, F, D = x.shape
        g_x = torch.empty_like(x)
        grads = [torch.zeros_like(p) for p in params]
        ws = torch.empty(max(lib.dfm_attention_backward_workspace_bytes(B, D, block.attention_dim) // 4, 1),
                         dtype=torch.float32, device=x.device)
        _lib.check(lib.dfm_attention_backward(
            x.data_ptr(), g_out.contiguous().data_ptr(), B, F, D, block.attention_dim, block.num_heads,
            int(block.use_residual), _lib.ptrs(params), g_x.data_ptr(), _lib.ptrs(grads), ws.data_ptr(),
            _lib.stream_handle()))
        return (None, g_x) + tuple(grads)
