"""``block_forward`` / ``block_backward`` (models/layers/attention.py) with every option against the same calls
without: ``out_into`` (a (B, 2 F D) buffer), ``x_copy_into``, ``g_stride``, ``grad_tail`` and ``direct``, on each GEMM
route and over two blocks, with and without residual.  ``out_into`` and ``g_stride`` need a block with residual:
without one they are left out, and asking for them is refused.  The bar is ``assert_close`` unchanged; ``W_k.bias``
(an identically zero gradient) keeps the absolute floor of tests/test_gpu_attention_matrix.py."""
import pytest
import torch

from tests.helpers import assert_close, attention_case_inputs, npy
from tests.test_gpu_attention_matrix import WKB_FLOOR, _case

B = 5
CASES = [       # the instantiation matrix's own shapes for these routes
    ("whole_block", _case(17, 32, 4, 64, B)),
    ("qkv_inside", _case(17, 48, 2, 32, B)),
    ("gemm_core", _case(32, 40, 2, 32, B)),
    ("whole_block", _case(17, 32, 4, 64, B, layers=2)),
]


def _blocks(c, params):
    """The blocks on the device, every ``.grad`` a view of one zeroed flat buffer laid out for direct writes
    (W_q | W_k | W_v back to back, weights then biases); -> (blocks, that buffer)."""
    from deepfm_amd.models.layers.attention import MultiHeadSelfAttention
    att = MultiHeadSelfAttention(c["D"], c["heads"], c["A"], c["layers"], c["residual"])
    att.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    blocks = list(att.cuda().layers)
    order = [p for blk in blocks for group in blk.adjacent_parameters() for p in group]
    order += [p for blk in blocks for p in blk._param_list()[6:]]
    flat = torch.zeros(sum(p.numel() for p in order), device="cuda")
    at = 0
    for p in order:
        assert at % 4 == 0                      # every view on a 16-byte boundary
        p.grad = flat[at:at + p.numel()].view_as(p)
        at += p.numel()
    return blocks, flat


@pytest.mark.gpu
@pytest.mark.parametrize("residual", [True, False], ids=["residual", "nores"])
@pytest.mark.parametrize("route,shape", CASES, ids=[f"{r}-{c['layers']}layer" for r, c in CASES])
def test_options_against_plain_calls(route, shape, residual):
    from deepfm_amd import _lib
    from deepfm_amd.models.layers.attention import block_backward, block_forward, block_route
    lib, st = _lib.load(), _lib.stream_handle()
    c = dict(shape, residual=residual)
    F, D = c["F"], c["D"]
    FD, ld = F * D, 2 * F * D
    params, x, up = attention_case_inputs(c)
    blocks, flat = _blocks(c, params)
    n, last = len(blocks), len(blocks) - 1
    for blk in blocks:
        assert block_route(blk, F) == route
    fe = torch.from_numpy(x).cuda()
    g_up = torch.from_numpy(up).cuda()

    # ---- plainly: contiguous everywhere, parameter gradients returned ----
    h, saved = fe, []
    for blk in blocks:
        h, s = block_forward(blk, h)
        assert s.route == route and not s.x_copied
        saved.append(s)
    out_plain = h
    assert out_plain.shape == fe.shape
    g, plain_grads = g_up, [None] * n
    for i in reversed(range(n)):
        r = block_backward(blocks[i], saved[i], g)
        assert not r.tail_done and len(r.params) == len(blocks[i]._param_list())
        g, plain_grads[i] = r.d_x, r.params
    d_x_plain = g
    # the returned temporaries added to the zeroed .grad views: what a direct backward has to leave there
    for blk, grads in zip(blocks, plain_grads):
        ps = blk._param_list()
        torch._foreach_add_([p.grad for p in ps], [t.view_as(p) for t, p in zip(grads, ps)])
    want_flat = flat.clone()
    flat.zero_()

    # ---- with the options ----
    nan = float("nan")
    xcat = torch.full((B, ld), nan, device="cuda")
    h, saved = fe, []
    for i, blk in enumerate(blocks):
        h, s = block_forward(blk, h, out_into=(xcat, ld) if i == last and residual else None,
                             x_copy_into=(xcat.data_ptr() + 4 * FD, ld) if i == 0 else None)
        saved.append(s)
    if residual:
        assert h is xcat
        assert_close(npy(xcat[:, :FD]).reshape(B, F, D), npy(out_plain), what="out")
    else:
        assert_close(npy(h), npy(out_plain), what="out")
        assert bool(torch.isnan(xcat[:, :FD]).all()), "out_into was not given, yet the buffer was written"
    assert saved[0].x_copied == (route == "whole_block") and not any(s.x_copied for s in saved[1:])
    if saved[0].x_copied:
        assert_close(npy(xcat[:, FD:]), npy(fe).reshape(B, FD), what="x copy")
    else:
        assert bool(torch.isnan(xcat[:, FD:]).all()), "x_copied is False, yet the copy was written"

    gen = torch.Generator(device="cuda").manual_seed(F * D)
    g_xcat = torch.full((B, ld), nan, device="cuda")      # d out in the first F D floats of each row
    g_xcat[:, :FD] = g_up.view(B, FD)
    g_dnn = torch.randn(B, ld, device="cuda", generator=gen)                  # d flat: its second half
    g_fm = torch.randn(B, device="cuda", generator=gen)
    fm_sum = torch.randn(B, D, device="cuda", generator=gen)
    g_fe = torch.full((B, F, D), nan, device="cuda")
    tail = dict(g_flat=g_dnn.data_ptr() + 4 * FD, ld_flat=ld, g_fm=g_fm.data_ptr(), fm_sum=fm_sum.data_ptr())
    g = g_xcat if residual else g_up
    for i in reversed(range(n)):
        r = block_backward(blocks[i], saved[i], g, direct=True, g_stride=ld if i == last and residual else 0,
                           grad_tail=dict(out=g_fe, **tail) if i == 0 else None)
        assert r.params is None, "the flat buffer is laid out for direct writes"
        assert r.tail_done == (i == 0 and saved[i].whole_backward)
        g = r.d_x
    assert saved[0].whole_backward == (route == "whole_block")
    if r.tail_done:                 # against the plain d x and the combine launch the caller would have made
        assert g.data_ptr() == g_fe.data_ptr()
        want = torch.empty_like(g_fe)
        _lib.check(lib.dfm_embedding_grad_combine(tail["g_flat"], ld, d_x_plain.data_ptr(), tail["g_fm"],
                                                  tail["fm_sum"], fe.data_ptr(), B, F, D, want.data_ptr(), st))
        assert_close(npy(g), npy(want), what="d_x with the tail")
    else:
        assert bool(torch.isnan(g_fe).all()), "tail_done is False, yet the tail's output was written"
        assert_close(npy(g), npy(d_x_plain), what="d_x")
    for i, blk in enumerate(blocks):
        for k, p in blk.named_parameters(prefix=f"layers.{i}"):
            at = p.grad.storage_offset()
            assert_close(npy(p.grad), npy(want_flat[at:at + p.numel()].view_as(p)), what="direct " + k,
                         floor=WKB_FLOOR if k.endswith("W_k.bias") else 0.0)


def test_options_a_route_cannot_honour_are_refused():
    """``out_into`` and a non-zero ``g_stride`` on a block without residual raise before any device work (so this
    test needs no GPU)."""
    from deepfm_amd.models.layers.attention import BlockSaved, _AttentionBlock, block_backward, block_forward
    blk = _AttentionBlock(32, 4, 64, use_residual=False)
    x = torch.zeros(B, 17, 32)
    with pytest.raises(ValueError, match="out_into"):
        block_forward(blk, x, out_into=(torch.zeros(B, 2 * 17 * 32), 2 * 17 * 32))
    saved = BlockSaved("whole_block", True, (B, 17, 32, 64, 4), (None,) * 9)
    with pytest.raises(ValueError, match="g_stride"):
        block_backward(blk, saved, x, g_stride=2 * 17 * 32)
