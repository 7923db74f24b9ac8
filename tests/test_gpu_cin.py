"""GPU parity: CIN kernels (through the C ABI) against reference golden vectors, the oracle and the fp64
reference of tests/helpers.py; tests/test_gpu_cin_matrix.py walks the instantiations and routes."""
import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests.helpers import assert_close, assert_close_mostly, cin_fp64, cin_full_params, group, load, npy
from tests.test_gpu_models_step import check_model_case

pytestmark = pytest.mark.gpu

CASES = ["cin_small_split", "cin_small_nosplit", "cin_single_layer", "cin_odd_split", "cin_criteo_full"]


def _module(g, params):
    from deepfm_amd.models.layers.cin import CIN
    F, D = g["x"].shape[1:]
    cin = CIN(F, D, [int(s) for s in g["layer_sizes"]], bool(g["split_half"]))
    assert cin.direct_sizes == list(g["direct_sizes"]) and cin.next_sizes == list(g["next_sizes"])
    assert cin.output_dim == int(g["output_dim"])
    cin.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return cin.cuda()


@pytest.mark.parametrize("case", CASES)
def test_cin_vs_golden(case):
    g = load(case)
    params = cin_full_params() if bool(g["hashed"]) else group(g, "param/")
    cin = _module(g, params)
    x = torch.from_numpy(g["x"]).cuda().requires_grad_()
    out = cin(x)
    assert out.shape == g["out"].shape
    assert_close(npy(out), g["out"], what="cin out")
    (out * torch.from_numpy(g["upstream"]).cuda()).sum().backward()
    assert_close(npy(x.grad), g["d_x"], what="cin d_x")
    for k, p in cin.named_parameters():
        assert p.grad is not None, k
        if bool(g["hashed"]):
            want = g["grad_sample/" + k]
            got = npy(p.grad).reshape(-1)
            got = got[::97] if k.endswith("weight") else got
        else:
            want, got = g["grad/" + k], npy(p.grad)
        assert_close(got, want, what=k)


def test_cin_reference_shape_tests():
    """tests/test_layers.py:143-168"""
    from deepfm_amd.models.layers.cin import CIN
    x = torch.randn(4, 3, 16, device="cuda")
    assert CIN(3, 16, [64, 64], split_half=False).cuda()(x).shape == (4, 128)
    split = CIN(3, 16, [64, 64], split_half=True).cuda()
    assert split.output_dim == 32 + 64 and split(x).shape == (4, 96)


def _cfg3_case(B, seed=7):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, 39, 16)) * 0.7).astype(np.float32)
    up = rng.standard_normal((B, 256)).astype(np.float32)
    return x, up


def test_cin_cfg3_batch_vs_oracle():
    """BASELINE.json config 3 layer sizes at a batch where ReLU-kink flips are still rare."""
    params = cin_full_params()
    cin = _module(load("cin_criteo_full"), params)
    x, up = _cfg3_case(192)
    t = torch.from_numpy(x).cuda().requires_grad_()
    out = cin(t)
    (out * torch.from_numpy(up).cuda()).sum().backward()
    assert_close(npy(out), O.cin_forward(x, params, [128, 128, 128], True), what="out")
    d_x, grads = O.cin_backward(x, params, [128, 128, 128], True, up)
    # gradients: an activation within rounding distance of the ReLU kink may flip in a (b, d)
    # column (39 elements of d_x each, one row-slice of dW): bounded outlier fraction allowed
    assert_close_mostly(npy(t.grad), d_x, 2e-3, what="d_x")
    for k, p in cin.named_parameters():
        assert_close_mostly(npy(p.grad), grads[k], 2e-2, rtol=2e-4, what=k)


def test_cin_cfg3_full_batch_vs_oracle():
    """BASELINE.json config 3 at its FULL batch: F = 39, D = 16, [128,128,128] split-half, B = 4096
    (cin.py:66-105) — forward and d x against the oracle on the golden case's weights.  The weight gradient at
    this batch is a sum over 65 536 (b, d) columns of terms with random signs, ~256 x one term: ONE activation
    that lands on the other side of the ReLU kink (split-bf16 products against the fp32 oracle, ~1e-5 relative)
    moves its whole dW row by ~0.4 %, and with 25 M pre-activations per layer about every second row holds such
    a column.  So on these weights dW is held to the bar on the rows without a flip (>= 40 % of the elements) and
    to 3 % of its scale everywhere; the
    kink-free full-batch test below holds every gradient element to the normal bar."""
    params = cin_full_params()
    cin = _module(load("cin_criteo_full"), params)
    x, up = _cfg3_case(4096)
    t = torch.from_numpy(x).cuda().requires_grad_()
    out = cin(t)
    (out * torch.from_numpy(up).cuda()).sum().backward()
    assert_close(npy(out), O.cin_forward(x, params, [128, 128, 128], True), what="out")
    d_x, grads = O.cin_backward(x, params, [128, 128, 128], True, up)
    assert_close_mostly(npy(t.grad), d_x, 2e-3, what="d_x")
    for k, p in cin.named_parameters():
        got, want = npy(p.grad).astype(np.float64), grads[k].astype(np.float64)
        scale = np.abs(want).max()
        err = np.abs(got - want)
        within = (err <= 2e-4 * np.abs(want) + 1e-5 * scale).mean()
        assert within >= 0.40, (k, float(within))          # rows without a flipped column: the normal bar
        assert err.max() < 0.03 * scale, (k, float(err.max() / scale))


def test_cin_cfg3_full_batch_kink_free_vs_oracle():
    """The same shape and batch with every pre-activation far from the ReLU kink (biases +6 / -6, see
    test_cin_mfma_backward_paths_vs_oracle): the gradient is continuous there, so all three MFMA kernels
    (forward, column-local dgrad, batch-sliced wgrad + slab reduce) must meet the bar on EVERY element."""
    from deepfm_amd.models.layers.cin import CIN
    torch.manual_seed(3)
    cin = CIN(39, 16, [128, 128, 128], True).cuda()
    with torch.no_grad():
        for conv in cin.conv_layers:
            c = torch.arange(conv.bias.numel(), device="cuda")
            conv.bias.copy_(torch.where(c % 3 == 2, -6.0, 6.0))
            conv.weight.mul_(0.25)
    params = {k: v.detach().cpu().numpy() for k, v in cin.state_dict().items()}
    x, up = _cfg3_case(4096, seed=8)
    t = torch.from_numpy(x).cuda().requires_grad_()
    out = cin(t)
    (out * torch.from_numpy(up).cuda()).sum().backward()
    want, cache = O.cin_forward(x, params, [128, 128, 128], True, return_cache=True)
    assert min(float(np.abs(y[y != 0]).min()) for _, y in cache) > 1e-2, "a pre-activation sits near the kink"
    assert_close(npy(out), want, what="out")
    d_x, grads = O.cin_backward(x, params, [128, 128, 128], True, up)
    assert_close_mostly(npy(t.grad), d_x, 0.0, rtol=2e-4, what="d_x")
    for k, p in cin.named_parameters():
        assert_close_mostly(npy(p.grad), grads[k], 0.0, rtol=2e-4, what=k)
    # and against the fp64 reference (samples are independent: batch chunks, parameter gradients added up)
    r_out, r_dx, r_grads = [], [], {}
    for b0 in range(0, 4096, 512):
        o, dx, g, pre = cin_fp64(x[b0:b0 + 512], params, [128, 128, 128], True, up[b0:b0 + 512])
        assert min(float(np.abs(a).min()) for a in pre) > 1e-2, "a pre-activation sits near the kink"
        r_out.append(o)
        r_dx.append(dx)
        for k in g:
            r_grads[k] = r_grads.get(k, 0.0) + g[k]
    assert_close(npy(out), np.concatenate(r_out), what="out vs fp64")
    assert_close(npy(t.grad), np.concatenate(r_dx), rtol=2e-4, what="d_x vs fp64")
    for k, p in cin.named_parameters():
        assert_close(npy(p.grad), r_grads[k], rtol=2e-4, what=k + " vs fp64")


@pytest.mark.parametrize("F,sizes,split,D,B", [
    (12, [48, 40, 24], True, 16, 96),    # MFMA backward, generic paths: < 128 channels (MB < 4, KS < 8); bias in a padding column
    (8, [32, 16], True, 16, 96),         # F a multiple of 8: no padding column -> separate bias-gradient kernels
    (16, [128, 128], False, 16, 96),     # 128-channel specialisation without split, bias fallback
    (39, [128, 64, 128], True, 16, 96),  # mixed: specialised and generic layers in one launch
    (12, [48, 40, 24], True, 8, 96),     # D = 8: a k-step of the weight gradient spans two samples
    (39, [128, 64, 128], True, 8, 50),   #        batch slices rounded to even sample counts
    (12, [48, 40, 24], True, 32, 96),    # D = 32: two k-steps per sample
    (39, [128, 64, 128], True, 32, 37),
    (8, [32, 16], True, 8, 33),          # D = 8 with an odd batch: the exact-fp32 VALU backward takes over
])
def test_cin_mfma_backward_paths_vs_oracle(F, sizes, split, D, B):
    """D in {8, 16, 32} takes the MFMA forward/backward kernels; shapes chosen to reach every code path of
    csrc/cin_mfma.hip / cin_mfma_bwd.hip (specialised vs generic inner loops, fused vs separate bias
    gradient).  The biases are set to +6 (live channel) / -6 (dead channel, every third) so that no
    pre-activation sits near the ReLU kink: the split-bf16 arithmetic (relative error ~1e-5) would
    otherwise flip a few dozen activations against the fp32 oracle, each flip moving a whole row of
    dW — with the kinks out of the way every gradient must meet the normal bar, no outliers."""
    from deepfm_amd.models.layers.cin import CIN
    rng = np.random.default_rng(100 + F)
    torch.manual_seed(F)
    cin = CIN(F, D, sizes, split).cuda()
    with torch.no_grad():
        for conv in cin.conv_layers:
            c = torch.arange(conv.bias.numel(), device="cuda")
            conv.bias.copy_(torch.where(c % 3 == 2, -6.0, 6.0))
            conv.weight.mul_(0.25)            # keeps |W Z| well inside the +-6 offsets in every layer
    params = {k: v.detach().cpu().numpy() for k, v in cin.state_dict().items()}
    x = (rng.standard_normal((B, F, D)) * 0.7).astype(np.float32)
    up = rng.standard_normal((B, cin.output_dim)).astype(np.float32)
    t = torch.from_numpy(x).cuda().requires_grad_()
    out = cin(t)
    (out * torch.from_numpy(up).cuda()).sum().backward()
    want, cache = O.cin_forward(x, params, sizes, split, return_cache=True)
    assert min(float(np.abs(y[y != 0]).min()) for _, y in cache) > 1e-2, "a pre-activation sits near the kink"
    assert_close(npy(out), want, what="out")
    d_x, grads = O.cin_backward(x, params, sizes, split, up)
    assert_close_mostly(npy(t.grad), d_x, 0.0, rtol=2e-4, what="d_x")
    for k, p in cin.named_parameters():
        assert_close_mostly(npy(p.grad), grads[k], 0.0, rtol=2e-4, what=k)
    r_out, r_dx, r_grads, pre = cin_fp64(x, params, sizes, split, up)
    assert min(float(np.abs(a).min()) for a in pre) > 1e-2, "a pre-activation sits near the kink"
    assert_close(npy(out), r_out, what="out vs fp64")
    assert_close(npy(t.grad), r_dx, rtol=2e-4, what="d_x vs fp64")
    for k, p in cin.named_parameters():
        assert_close(npy(p.grad), r_grads[k], rtol=2e-4, what=k + " vs fp64")


def test_xdeepfm_vs_golden():
    check_model_case("model_xdeepfm")
