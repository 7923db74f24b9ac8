"""CIN test matrix: every instantiation of the matrix-core kernels (D x field groups x SPLIT), both arithmetic
modes, the edges of the branch-free specialisations, ragged batches, the depth limit, and the general kernels at
real sizes, against the fp64 reference of tests/helpers.py (`cin_fp64`, no code shared with oracle/).

A case is (F, D, layer_sizes, split_half, B).  `expected_route` restates the library's route rules; the library
answers `dfm_cin_route` for the same shape, and every test asserts the two agree before it trusts a number.
The coverage assertions over these lists are in tests/test_cpu_cin_reference.py (they need no GPU)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.helpers import (assert_close, cin_bf16_emulation, cin_case_inputs, cin_fp64, cin_split_layout, npy)

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4          # the bar of test_cin_mfma_backward_paths_vs_oracle for d_x / dW / db, no outliers

# ---- the matrix ---------------------------------------------------------------------------------------------
MFMA_CASES = [
    (17, 16, (40, 24), True, 5),            # FG 3; odd B: a half-filled wave
    (24, 16, (64, 32), True, 19),           # FG 3, F % 8 == 0: separate bias kernels
    (25, 16, (33, 31, 9), True, 3),         # FG 4; odd C, odd split halves, odd H
    (32, 16, (48,), False, 1),              # FG 4 without a padding column; B = 1, L = 1
    (33, 16, (100, 120, 128), True, 21),    # FG 5; MB == 4 with padded rows (100); KS == 8 with padded rows (120)
    (40, 16, (113, 97), False, 18),         # F = 40; C = 97 / 113 on the edges of both specialisations; H = 113 next
                                            # to five field groups does not fit the forward's LDS: general kernels
    (40, 16, (113, 97), True, 18),          # the same edges on the matrix cores (H = 57)
    (1, 16, (8, 8), True, 7),               # F = 1
    (39, 16, (16,) * 8, True, 17),          # L = 8: one reduce launch with 8 jobs
    (8, 16, (128, 128), False, 257),        # H = 128; one sample past 16 full workgroups
    (12, 16, (24, 16), True, 3),            # D 16 / FG 2
    (20, 8, (40, 24), True, 6),             # D 8 / FG 3; B not a multiple of the 4 samples of a wave
    (28, 8, (64,), True, 2),                # D 8 / FG 4
    (40, 8, (100, 50), True, 34),           # D 8 / FG 5, MB == 4 padded
    (7, 8, (24, 16), True, 4),              # D 8 / FG 1
    (12, 8, (24, 16), True, 10),            # D 8 / FG 2
    (5, 32, (24, 16), True, 3),             # D 32 / FG 1
    (9, 32, (24, 16), True, 3),             # D 32 / FG 2
    (18, 32, (40, 24), True, 5),            # D 32 / FG 3
    (30, 32, (64, 32), False, 2),           # D 32 / FG 4
    (36, 32, (40, 24), True, 3),            # D 32 / FG 5
]
# (case, mode)
GENERAL_CASES = [
    ((39, 16, (200, 200, 200), True, 9), 0),    # the xDeepFM paper's layers: C > 128
    ((41, 16, (32, 16), True, 9), 0),           # F > 40
    ((12, 16, (16,) * 9, True, 9), 0),          # L = 9
    ((10, 10, (20, 12), True, 9), 0),           # D outside {8, 16, 32}
    ((39, 64, (64, 32), True, 5), 0),           # D = 64
    ((4, 64, (300, 40), True, 5), 0),           # (F + H + C) D 4 and C D 4 above 64 KB: forward, backward, bias partials
    ((4, 64, (256,), True, 5), 0),              # C D 4 = 64 KB exactly: the bias partials' default LDS limit
    ((4, 64, (257,), True, 5), 0),              #         one channel past it
    ((39, 16, (128, 64, 128), True, 9), 2),     # general kernels at a matrix-core shape
    ((39, 8, (128, 64, 128), True, 9), 0),      # matrix-core forward + general backward at real sizes
    ((12, 16, (24, 16), True, 3), 2),           # B below the 8 weight-gradient slices
    ((12, 16, (24, 16), True, 1), 2),
]
ALL_RUNS = [(c, 0) for c in MFMA_CASES] + GENERAL_CASES
ROUTES = ("mfma", "mfma_fwd+general_bwd", "general")


def case_id(c):
    F, D, sizes, split, B = c
    return f"F{F}-D{D}-{'x'.join(map(str, sizes))}-{'split' if split else 'whole'}-B{B}"


def run_id(run):
    return f"{case_id(run[0])}-mode{run[1]}"


def general_reasons(c, mode):
    """Why a run cannot take the matrix-core forward (empty: it can)."""
    F, D, sizes, split, B = c
    H = cin_split_layout(F, sizes, split)[0]
    FG = (F + 7) // 8
    why = set()
    if mode == 2:
        why.add("mode 2")
    if D not in (8, 16, 32):
        why.add("D")
    if F > 40:
        why.add("F > 40")
    if len(sizes) > 8:
        why.add("L > 8")
    if max(sizes) > 128 or max(H) > 128:
        why.add("C or H > 128")
    # the forward's LDS: 16 KB of weight slabs per field group + 1 KB per row of the padded hidden image
    if not why and 16 * FG + max(8 * FG, max(2 * ((h + 1) // 2) for h in H)) > 160:
        why.add("LDS")
    return why


def expected_route(c, mode):
    if general_reasons(c, mode):
        return "general"
    return "mfma_fwd+general_bwd" if (c[1] == 8 and c[4] % 2) else "mfma"


def library_route(lib, c):
    F, D, sizes, split, B = c
    return ROUTES[lib.dfm_cin_route((C.c_int32 * len(sizes))(*sizes), len(sizes), int(split), B, F, D)]


# ---- shared, read-only references -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(c, kink_free):
    """(params, x, up, (out, d_x, grads, pre)) of a case in fp64: computed once, shared by every test."""
    F, D, sizes, split, B = c
    params, x, up = cin_case_inputs(c, kink_free)
    return params, x, up, cin_fp64(x, params, list(sizes), split, up if kink_free else None)


@functools.lru_cache(maxsize=None)
def emulation(c):
    F, D, sizes, split, B = c
    params, x, up, _ = reference(c, True)
    return cin_bf16_emulation(x, params, list(sizes), split, up)


@pytest.fixture
def cin_mode():
    """Set the CIN arithmetic mode for one test; the previous mode is restored afterwards."""
    from deepfm_amd import _lib
    lib = _lib.load()
    before = lib.dfm_cin_get_mode()

    def set_mode(mode):
        assert lib.dfm_cin_set_mode(mode) == 0
        return lib
    try:
        yield set_mode
    finally:
        lib.dfm_cin_set_mode(before)


def _module(c, params):
    from deepfm_amd.models.layers.cin import CIN
    F, D, sizes, split, B = c
    cin = CIN(F, D, list(sizes), split)
    cin.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return cin.cuda()


def _run_module(c, params, x, up=None):
    cin = _module(c, params)
    t = torch.from_numpy(x).cuda().requires_grad_(up is not None)
    out = cin(t)
    if up is None:
        return npy(out), None, None
    (out * torch.from_numpy(up).cuda()).sum().backward()
    return npy(out), npy(t.grad), {k: npy(p.grad) for k, p in cin.named_parameters()}


def _check_grads(got_dx, got, want_dx, want, what=""):
    assert_close(got_dx, want_dx, rtol=GRAD_RTOL, what=what + "d_x")
    assert sorted(got) == sorted(want)
    for k in want:
        assert_close(got[k], want[k], rtol=GRAD_RTOL, what=what + k)


# ---- through the C ABI, every buffer inside a larger allocation --------------------------------------------------
GUARD = 64                      # floats on each side: keeps every buffer 256-byte aligned
SENTINEL = -1234.5


class Boxed:
    def __init__(self, nfloats, fill):
        self.whole = torch.full((nfloats + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.whole[GUARD:GUARD + nfloats]
        self.t.fill_(fill)

    def guards_intact(self):
        g = torch.cat([self.whole[:GUARD], self.whole[GUARD + self.t.numel():]]).view(torch.int32)
        want = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item()
        return bool((g == want).all())


def _run_abi(lib, c, params, x, up, prefill=0.0, with_saved=True, backward=True):
    """dfm_cin_forward / dfm_cin_backward on buffers with guard floats around them; workspaces and the saved
    buffer start as NaN.  Returns (rc_forward, dict of results and the boxes)."""
    from deepfm_amd import _lib
    F, D, sizes, split, B = c
    L = len(sizes)
    sz = (C.c_int32 * L)(*sizes)
    sp = int(split)
    out_dim = lib.dfm_cin_output_dim(sz, L, sp)
    nan = float("nan")
    box = dict(
        x0=Boxed(B * F * D, 0.0), out=Boxed(B * out_dim, nan), g_x0=Boxed(B * F * D, nan),
        saved=Boxed(max(lib.dfm_cin_saved_bytes(sz, L, sp, B, F, D) // 4, 4), nan),
        fws=Boxed((lib.dfm_cin_forward_workspace_bytes(sz, L, sp, F, D) + 3) // 4 + 4, nan),
        bws=Boxed((lib.dfm_cin_backward_workspace_bytes(sz, L, sp, B, F, D) + 3) // 4 + 4, nan))
    box["x0"].t.copy_(torch.from_numpy(x).reshape(-1))
    w = [torch.from_numpy(params[f"conv_layers.{i}.weight"]).cuda().contiguous() for i in range(L)]
    b = [torch.from_numpy(params[f"conv_layers.{i}.bias"]).cuda().contiguous() for i in range(L)]
    st = _lib.stream_handle()
    rc = lib.dfm_cin_forward(box["x0"].t.data_ptr(), B, F, D, _lib.ptrs(w), _lib.ptrs(b), sz, L, sp,
                             box["out"].t.data_ptr(), box["saved"].t.data_ptr() if with_saved else None,
                             box["fws"].t.data_ptr(), st)
    r = dict(box=box, out=None)
    if rc != 0:
        return rc, r
    torch.cuda.synchronize()
    r["out"] = npy(box["out"].t).reshape(B, out_dim)
    r["saved"] = box["saved"].t
    if not backward:
        return rc, r
    g_out = torch.from_numpy(up).cuda().contiguous()
    g_w = [torch.full_like(t, prefill) for t in w]
    g_b = [torch.full_like(t, prefill) for t in b]
    _lib.check(lib.dfm_cin_backward(box["x0"].t.data_ptr(), B, F, D, _lib.ptrs(w), sz, L, sp, box["saved"].t.data_ptr(),
                                    g_out.data_ptr(), box["g_x0"].t.data_ptr(), _lib.ptrs(g_w), _lib.ptrs(g_b),
                                    box["bws"].t.data_ptr(), st))
    torch.cuda.synchronize()
    r["d_x"] = npy(box["g_x0"].t).reshape(B, F, D)
    r["grads"] = {}
    for i in range(L):
        r["grads"][f"conv_layers.{i}.weight"] = npy(g_w[i])
        r["grads"][f"conv_layers.{i}.bias"] = npy(g_b[i])
    return rc, r


# ---- the tests -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ALL_RUNS + [(c, 1) for c in MFMA_CASES], ids=run_id)
def test_route(run, cin_mode):
    c, mode = run
    lib = cin_mode(mode)
    assert library_route(lib, c) == expected_route(c, mode)


@pytest.mark.parametrize("run", ALL_RUNS, ids=run_id)
def test_forward_ordinary_parameters(run, cin_mode):
    """Default-init weights and biases: pre-activations on both sides of the ReLU.  The forward is continuous, so
    every element meets the normal bar."""
    c, mode = run
    lib = cin_mode(mode)
    assert library_route(lib, c) == expected_route(c, mode)
    params, x, _, (want, _, _, _) = reference(c, False)
    out, _, _ = _run_module(c, params, x)
    assert np.isfinite(out).all()
    assert_close(out, want, what="out")


@pytest.mark.parametrize("run", ALL_RUNS, ids=run_id)
def test_forward_backward_kink_free(run, cin_mode):
    """Every pre-activation far from the kink (tests/test_cpu_cin_reference.py checks the margin on the reference):
    out, d_x and every parameter gradient meet the bar on every element; a second pass is bitwise the same."""
    c, mode = run
    lib = cin_mode(mode)
    assert library_route(lib, c) == expected_route(c, mode)
    params, x, up, (w_out, w_dx, w_grads, _) = reference(c, True)
    out, d_x, grads = _run_module(c, params, x, up)
    assert_close(out, w_out, what="out")
    _check_grads(d_x, grads, w_dx, w_grads)
    out2, d_x2, grads2 = _run_module(c, params, x, up)
    assert np.array_equal(out, out2) and np.array_equal(d_x, d_x2), "a second pass differs"
    for k in grads:
        assert np.array_equal(grads[k], grads2[k]), f"{k}: a second pass differs"


def _max_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max())


def _within_twice(got, emu, want, what):
    """|got - fp64| <= 2 max|emulation - fp64| + the normal bar.  The emulation adds in fp64 where the kernels add
    in fp32, so where it is exact (a bias gradient that is a plain sum of fp32 dY) the kernel still gets the bar
    every fp32 kernel gets."""
    want = np.asarray(want, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    e_emu = _max_err(np.asarray(emu).reshape(want.shape), want)
    bound = 2.0 * e_emu + GRAD_RTOL * np.abs(want) + 1e-5 * np.abs(want).max()
    err = np.abs(got - want)
    scale = np.abs(want).max()
    print(f"mode 1 {what}: emulation {e_emu / scale:.3e}, kernel {err.max() / scale:.3e} (of the tensor's scale)")
    assert (err <= bound).all(), f"{what}: kernel error {err.max():.3e}, emulation's own error {e_emu:.3e}"


@pytest.mark.parametrize("c", [c for c in MFMA_CASES if expected_route(c, 1) == "mfma"], ids=case_id)
def test_plain_bf16_mode(c, cin_mode):
    """dfm_cin_set_mode(1), SPLIT = false in all three kernels, against a CPU emulation of plain-bf16 products
    (tests/helpers.py::cin_bf16_emulation).  (a) Layer 0 — and the whole of a one-layer stack, gradients too —
    sees the same inputs as the emulation and must match IT to the normal bar: a wrong fragment or a padded lane
    shows here.  (b) On the full stack the kernel's error against fp64 is at most twice the emulation's (deeper
    hidden values differ in the last fp32 bit, which flips some bf16 roundings)."""
    lib = cin_mode(1)
    assert library_route(lib, c) == "mfma"
    F, D, sizes, split, B = c
    params, x, up, (w_out, w_dx, w_grads, _) = reference(c, True)
    emu = emulation(c)
    rc, r = _run_abi(lib, c, params, x, up)
    assert rc == 0
    H, direct, next_off, out_col, out_dim = cin_split_layout(F, sizes, split)
    # (a) layer 0: its pooled direct channels, and the next half the forward saves for the backward
    assert_close(r["out"][:, :direct[0]], emu["out"][:, :direct[0]], what="layer 0 pooled vs emulation")
    if len(sizes) > 1:
        y0 = npy(r["saved"][:B * sizes[0] * D]).reshape(B, sizes[0], D)[:, next_off[0]:]
        assert_close(y0, emu["y"][0][:, next_off[0]:], what="layer 0 next half vs emulation")
    else:
        assert_close(r["out"], emu["out"], what="out vs emulation")
        _check_grads(r["d_x"], r["grads"], emu["d_x"], emu["grads"], what="vs emulation: ")
    # (b) the full stack
    _within_twice(r["out"], emu["out"], w_out, "out")
    _within_twice(r["d_x"], emu["d_x"], w_dx, "d_x")
    for k in w_grads:
        _within_twice(r["grads"][k], emu["grads"][k], w_grads[k], k)


ACCUMULATE_RUNS = [
    ((17, 16, (40, 24), True, 5), 0),            # matrix cores, bias gradient in a padding column, one reduce launch
    ((24, 16, (64, 32), True, 19), 0),           # matrix cores, separate bias kernels, a reduce launch per layer
    ((39, 8, (128, 64, 128), True, 9), 0),       # general backward behind the matrix-core forward
    ((10, 10, (20, 12), True, 9), 0),            # general
]


@pytest.mark.parametrize("run", ACCUMULATE_RUNS, ids=run_id)
def test_parameter_gradients_are_added(run, cin_mode):
    """g_weights / g_biases pre-filled with 1.0 come back as 1.0 + gradient: the fused training step hands live
    gradient buffers to dfm_cin_backward."""
    c, mode = run
    lib = cin_mode(mode)
    assert library_route(lib, c) == expected_route(c, mode)
    params, x, up, (_, w_dx, w_grads, _) = reference(c, True)
    rc, r = _run_abi(lib, c, params, x, up, prefill=1.0)
    assert rc == 0
    got = {k: v.astype(np.float64).reshape(w_grads[k].shape) - 1.0 for k, v in r["grads"].items()}
    for k in w_grads:
        # the 1.0 costs the sum one fp32 rounding at its own magnitude
        assert_close(got[k], w_grads[k], rtol=GRAD_RTOL, floor=2.0 ** -23 * (1.0 + np.abs(w_grads[k]).max()), what=k)
    assert_close(r["d_x"], w_dx, rtol=GRAD_RTOL, what="d_x")


RAGGED_RUNS = [
    ((32, 16, (48,), False, 1), 0),
    ((25, 16, (33, 31, 9), True, 3), 0),
    ((17, 16, (40, 24), True, 5), 0),
    ((39, 16, (16,) * 8, True, 17), 0),
    ((8, 16, (128, 128), False, 257), 0),
    ((20, 8, (40, 24), True, 6), 0),
    ((5, 32, (24, 16), True, 3), 1),
    ((39, 8, (128, 64, 128), True, 9), 0),
    ((12, 16, (24, 16), True, 1), 2),
]


@pytest.mark.parametrize("run", RAGGED_RUNS, ids=run_id)
def test_nothing_outside_the_tensors_is_written_or_trusted(run, cin_mode):
    """x0, out, g_x0, the saved buffer and both workspaces sit inside larger allocations whose surrounding floats
    hold a sentinel; the workspaces, the saved buffer and the outputs start as NaN.  After a forward and a backward
    the guards are bit-identical and every output is finite and (mode 0 / 2) within the bar."""
    c, mode = run
    lib = cin_mode(mode)
    assert library_route(lib, c) == expected_route(c, mode)
    params, x, up, (w_out, w_dx, w_grads, _) = reference(c, True)
    rc, r = _run_abi(lib, c, params, x, up)
    assert rc == 0
    for name, b in r["box"].items():
        assert b.guards_intact(), f"{name}: a guard float changed"
    assert np.array_equal(npy(r["box"]["x0"].t).reshape(x.shape), x), "x0 was written"
    assert np.isfinite(r["out"]).all() and np.isfinite(r["d_x"]).all()
    assert all(np.isfinite(v).all() for v in r["grads"].values())
    if mode != 1:
        assert_close(r["out"], w_out, what="out")
        _check_grads(r["d_x"], {k: v.reshape(w_grads[k].shape) for k, v in r["grads"].items()}, w_dx, w_grads)


def test_null_saved_buffer(cin_mode):
    """Inference on the matrix cores may pass d_saved = NULL and gets bitwise the same output; the general kernels
    need the buffer and say so without launching anything."""
    lib = cin_mode(0)
    c = (17, 16, (40, 24), True, 5)
    assert library_route(lib, c) == "mfma"
    params, x, up, _ = reference(c, True)
    rc, with_saved = _run_abi(lib, c, params, x, up, backward=False)
    assert rc == 0
    rc, without = _run_abi(lib, c, params, x, up, with_saved=False, backward=False)
    assert rc == 0
    assert np.array_equal(with_saved["out"], without["out"])
    assert without["box"]["saved"].t.isnan().all(), "the saved buffer was not passed, yet it was written"
    c = (10, 10, (20, 12), True, 9)
    assert library_route(lib, c) == "general"
    params, x, up, _ = reference(c, True)
    rc, r = _run_abi(lib, c, params, x, up, with_saved=False, backward=False)
    assert rc != 0
    assert "need the d_saved buffer" in lib.dfm_last_error().decode()
    torch.cuda.synchronize()
    assert r["box"]["out"].t.isnan().all(), "a kernel ran"


def test_mode_api(cin_mode):
    lib = cin_mode(0)
    for mode in (0, 1, 2, 1, 0):
        assert lib.dfm_cin_set_mode(mode) == 0 and lib.dfm_cin_get_mode() == mode
    lib.dfm_cin_set_mode(1)
    for bad in (3, -1):
        assert lib.dfm_cin_set_mode(bad) != 0
        assert lib.dfm_cin_get_mode() == 1
