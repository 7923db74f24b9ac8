"""The layer matrix on the GPU: every case of tests/layer_cases.py through the C ABI on guarded buffers, against the
fp64 references of that module.  Every input and output lives in a GuardedBuffer, outputs NaN-filled; after each call
the guards are intact, the inputs hold their bits, every element the contract says is written holds no NaN and every
element it says is not written still holds its fill.  The integer family is compared with np.array_equal, the float
family with the measured bars.  Each test prints its worst |got - fp64| / bar."""
import numpy as np
import pytest
import torch

from deepfm_amd import _lib
from tests import layer_cases as L
from tests.helpers import GuardedBuffer as G

pytestmark = pytest.mark.gpu

NAN = float("nan")
FAMILIES = ("int", "float")
SENT64 = -0x123456789ABCDEF


def host(buf: G, *shape):
    a = buf.t.cpu().numpy()
    return a.reshape(shape) if shape else a


def call(fn, *args):
    _lib.check(fn(*args, _lib.stream_handle()))
    torch.cuda.synchronize()


def intact(*bufs):
    for b in bufs:
        if b is not None:
            assert b.guards_intact(), "a float outside a buffer was written"


def unchanged(pairs):
    for buf, arr in pairs:
        assert np.array_equal(host(buf).view(np.uint32), np.ascontiguousarray(arr, dtype=np.float32).reshape(-1).view(np.uint32)), \
            "an input was written"


def held(what, got, want, b, exact=False):
    """Integer family: the value of the (exact) fp64 reference.  Float family: the bar."""
    assert not np.isnan(got).any(), f"{what}: an element that must be written holds NaN"
    if exact:
        assert np.array_equal(got.astype(np.float64), want), f"{what}: {(got != want).sum()} of {got.size} elements differ"
        return 0.0
    r = L.worst(got, want, b)
    print(f"{what}: worst |got - fp64| / bar = {r:.3f}")
    assert r <= 1.0, f"{what}: {r:.3f} x the bar"
    return r


class Int64Cell:
    """One int64 on the device between two sentinels."""

    def __init__(self, value):
        self.t = torch.tensor([SENT64, value, SENT64], dtype=torch.int64, device="cuda")

    def ptr(self):
        return self.t[1:].data_ptr()

    def value(self):
        v = self.t.cpu().tolist()
        assert v[0] == SENT64 and v[2] == SENT64, "an int64 beside the cell was written"
        return v[1]


# =====================================================================================================================
# FMInteraction
# =====================================================================================================================
@pytest.mark.parametrize("name", list(L.FM_CASES))
def test_fm_forward(name):
    """fm_fwd_kernel<4> / <1>: every lanes-per-sample count, idle lanes inside a sample, the field loop's unroll
    remainders, the last sample of a workgroup and the first of the next; bases one float off 16 bytes run the scalar
    kernel."""
    c, lib = L.FM_CASES[name], _lib.load()
    for fam in FAMILIES:
        i = L.fm_inputs(c, fam)
        e, out = G.of(i["e"], c.shift), G(c.B, NAN)
        assert (e.ptr() % 16 == 0) == (c.shift == 0)
        call(lib.dfm_fm_forward, e.ptr(), c.B, c.F, c.D, out.ptr())
        ref, A = L.fm_fwd_ref(i["e"])
        held(f"fm_forward {name} {fam}", host(out), ref, L.bar(A, L.fm_fwd_chain(c), L.C["fm_fwd"]), fam == "int")
        intact(e, out)
        unchanged([(e, i["e"])])


@pytest.mark.parametrize("name", list(L.FM_CASES))
def test_fm_backward(name):
    c, lib = L.FM_CASES[name], _lib.load()
    for fam in FAMILIES:
        i = L.fm_inputs(c, fam)
        e, g, ge = G.of(i["e"], c.shift), G.of(i["g"]), G(c.B * c.F * c.D, NAN, c.shift)
        call(lib.dfm_fm_backward, e.ptr(), g.ptr(), c.B, c.F, c.D, ge.ptr())
        ref, A = L.fm_bwd_ref(i["e"], i["g"])
        got = host(ge, c.B, c.F, c.D)
        held(f"fm_backward {name} {fam}", got, ref, L.bar(A, L.fm_bwd_chain(c), L.C["fm_bwd"]), fam == "int")
        if fam == "int" and c.F == 1:
            assert not got.any()                          # S - e is exactly 0
        intact(e, g, ge)
        unchanged([(e, i["e"]), (g, i["g"])])


def test_fm_empty_batch_writes_nothing():
    lib = _lib.load()
    e, g, out, ge = G(64, 1.0), G(4, 1.0), G(4, NAN), G(64, NAN)
    call(lib.dfm_fm_forward, e.ptr(), 0, 4, 16, out.ptr())
    call(lib.dfm_fm_backward, e.ptr(), g.ptr(), 0, 4, 16, ge.ptr())
    assert np.isnan(host(out)).all() and np.isnan(host(ge)).all()
    intact(e, g, out, ge)


@pytest.mark.parametrize("name", list(L.COMBINE_CASES))
def test_embedding_grad_combine(name):
    """embedding_grad_combine_kernel: widths where c % dim is and is not a mask, padded row strides of g_flat, lane
    counts around a workgroup's 256, each of g_extra and the FM trio NULL or given."""
    c, lib = L.COMBINE_CASES[name], _lib.load()
    for fam in FAMILIES:
        i = L.combine_inputs(c, fam)
        b = {k: G.of(v) for k, v in i.items()}
        out = G(c.rows * c.width, NAN)
        call(lib.dfm_embedding_grad_combine, b["g_flat"].ptr(), c.ld, b["g_extra"].ptr() if c.extra else None,
             b["g_fm"].ptr() if c.fm else None, b["fm_sum"].ptr() if c.fm else None, b["e"].ptr() if c.fm else None,
             c.rows, c.F, c.D, out.ptr())
        ref, A = L.combine_ref(c, i)
        held(f"grad_combine {name} {fam}", host(out, c.rows, c.width), ref, L.bar(A, L.COMBINE_CHAIN, L.C["combine"]), fam == "int")
        intact(out, *b.values())
        unchanged([(b[k], i[k]) for k in i])


@pytest.mark.parametrize("rows", L.COPY_ROWS)
@pytest.mark.parametrize("width", L.COPY_WIDTH)
def test_copy_2d(width, rows):
    """copy_2d_kernel over every pair of row strides: a bit-equal copy, the columns of dst behind width keep their fill."""
    lib = _lib.load()
    rng = np.random.default_rng([width, rows])
    for ld_src in L.copy_lds(width):
        for ld_dst in L.copy_lds(width):
            a = rng.standard_normal((max(rows, 1), ld_src)).astype(np.float32)
            src, dst = G.of(a), G(max(rows, 1) * ld_dst, NAN)
            call(lib.dfm_copy_2d, src.ptr(), ld_src, dst.ptr(), ld_dst, rows, width)
            got = host(dst, max(rows, 1), ld_dst)
            assert np.array_equal(got[:rows, :width].view(np.uint32), a[:rows, :width].view(np.uint32))
            assert np.isnan(got[:rows, width:]).all() and np.isnan(got[rows:]).all(), "a float outside the block was written"
            intact(src, dst)
            unchanged([(src, a)])


# =====================================================================================================================
# BatchNorm -> ReLU -> dropout
# =====================================================================================================================
def _bn_forward(c: L.Bn, i):
    lib = _lib.load()
    M, N = c.M, c.N
    b = {k: G.of(i[k]) for k in ("z", "gamma", "beta", "running_mean", "running_var")}
    nb, seed = Int64Cell(i["num_batches"]), Int64Cell(c.seed if c.seed is not None else 0)
    out, ms = G(M * N, NAN), G(2 * N, NAN)
    ws_floats = lib.dfm_bn_workspace_bytes(M, N) // 4
    assert ws_floats == (2 * L.bn_slices(M) + 2) * N
    ws = G(ws_floats, NAN)
    run = c.running
    call(lib.dfm_bn_relu_dropout_forward, b["z"].ptr(), M, N, b["gamma"].ptr(), b["beta"].ptr(),
         b["running_mean"].ptr() if run else None, b["running_var"].ptr() if run else None, nb.ptr() if run else None,
         float(L.BN_MOMENTUM), float(L.BN_EPS), c.p, seed.ptr() if c.seed is not None else None, c.salt, out.ptr(), ms.ptr(),
         ws.ptr())
    intact(out, ms, ws, *b.values())
    unchanged([(b[k], i[k]) for k in ("z", "gamma", "beta")])
    assert seed.value() == (c.seed if c.seed is not None else 0)
    w = host(ws)
    assert not np.isnan(w[:2 * L.bn_slices(M) * N]).any() and np.isnan(w[2 * L.bn_slices(M) * N:]).all()
    return b, nb, out, ms


@pytest.mark.parametrize("name", list(L.BN_CASES))
def test_bn_relu_dropout_forward(name):
    """bn_fwd_partials / bn_fwd_finalize / bn_relu_dropout_fwd: 1 to 258 slices (each finalize lane folds 0, 1, 2 and
    17 of them), columns around the finalize's 16 and the partials' 256, every dropout threshold, and the statistics
    families, row 0 far from the column mean among them."""
    c, i, r = L.BN_CASES[name], L.bn_fwd_inputs(name), L.bn_fwd_ref(name)
    b, nb, out, ms = _bn_forward(c, i)
    stats = host(ms, 2, c.N)
    held(f"bn_forward {name} mean", stats[0], r["mean"], r["bar_mean"])
    held(f"bn_forward {name} rstd", stats[1], r["rstd"], r["bar_rstd"])
    got = host(out, c.M, c.N)
    held(f"bn_forward {name} out", got, r["out"], r["bar_out"])
    assert not got[~r["kept"]].any(), "an element the restated mask drops was kept"
    live = r["kept"] & (r["y"] > r["bar_out"])
    assert (got[live] > 0).all(), "an element the restated mask keeps was dropped"
    if c.running:
        held(f"bn_forward {name} running_mean", host(b["running_mean"]), r["running_mean"], r["bar_running_mean"])
        held(f"bn_forward {name} running_var", host(b["running_var"]), r["running_var"], r["bar_running_var"])
        assert nb.value() == i["num_batches"] + 1
    else:
        unchanged([(b[k], i[k]) for k in ("running_mean", "running_var")])
        assert nb.value() == i["num_batches"]
    _, _, out2, ms2 = _bn_forward(c, i)
    assert torch.equal(out.t.view(torch.int32), out2.t.view(torch.int32)) and torch.equal(ms.t.view(torch.int32), ms2.t.view(torch.int32))


@pytest.mark.parametrize("name", list(L.BN_BWD_CASES))
def test_bn_relu_dropout_backward(name):
    """bn_bwd_partials / bn_bwd_finalize / bn_relu_dropout_bwd on inputs moved off the ReLU kink: d gamma and d beta
    are added onto what the buffers hold (a second call adds the same again, bitwise), dz is written."""
    c, i, r = L.BN_BWD_CASES[name], L.bn_bwd_inputs(name), L.bn_bwd_ref(name)
    lib = _lib.load()
    M, N = c.M, c.N
    b = {k: G.of(i[k]) for k in ("g", "z", "stats", "gamma", "beta")}
    seed = Int64Cell(c.seed if c.seed is not None else 0)
    ws_floats = lib.dfm_bn_workspace_bytes(M, N) // 4

    def run(dg, db):
        dz, ws = G(M * N, NAN), G(ws_floats, NAN)
        call(lib.dfm_bn_relu_dropout_backward, b["g"].ptr(), b["z"].ptr(), b["stats"].ptr(), b["gamma"].ptr(), b["beta"].ptr(),
             M, N, c.p, seed.ptr() if c.seed is not None else None, c.salt, dz.ptr(), dg.ptr(), db.ptr(), ws.ptr())
        intact(dz, ws, dg, db, *b.values())
        assert not np.isnan(host(ws)).any()
        return dz

    zg, zb = G(N, 0.0), G(N, 0.0)
    dz = run(zg, zb)
    sg, sb = host(zg).copy(), host(zb).copy()              # 0 + s = s: the sums themselves
    n = L.bn_chain(M)
    held(f"bn_backward {name} d_gamma", sg, r["d_gamma"], L.bar(r["A_gamma"], n, L.C["bn_bwd"]))
    held(f"bn_backward {name} d_beta", sb, r["d_beta"], L.bar(r["A_beta"], n, L.C["bn_bwd"]))
    held(f"bn_backward {name} dz", host(dz, M, N), r["dz"], L.bar(r["A_dz"], L.bn_bwd_chain(M), L.C["bn_bwd"]))
    dg, db = G.of(i["d_gamma0"]), G.of(i["d_beta0"])
    want_g, want_b = i["d_gamma0"], i["d_beta0"]
    for _ in range(2):
        dz2 = run(dg, db)
        want_g, want_b = want_g + sg, want_b + sb           # float32 additions, as the kernel's
        assert np.array_equal(host(dg).view(np.uint32), want_g.view(np.uint32)), "d gamma: not the sum added on"
        assert np.array_equal(host(db).view(np.uint32), want_b.view(np.uint32)), "d beta: not the sum added on"
        assert torch.equal(dz.t.view(torch.int32), dz2.t.view(torch.int32))
    unchanged([(b[k], i[k]) for k in b])


# =====================================================================================================================
# BCE with logits
# =====================================================================================================================
@pytest.mark.parametrize("family,n", L.BCE_CASES)
def test_bce_with_logits(family, n):
    """bce_fwd_bwd / bce_finalize: sample counts around the 4 per thread and the 1024 per workgroup, 257 partials for
    the finalize's stride of 256; logits where expf underflows; soft labels."""
    lib = _lib.load()
    i, r = L.bce_inputs(family, n), L.bce_ref(family, n)
    P = L.bce_partials(n)
    assert lib.dfm_bce_workspace_bytes(n) == 4 * P
    z, y = G.of(i["z"]), G.of(i["y"])
    runs = []
    for _ in range(2):
        loss, dz, ws = G(1, NAN), G(n, NAN), G(P + 8, NAN)
        call(lib.dfm_bce_with_logits, z.ptr(), y.ptr(), n, loss.ptr(), dz.ptr(), ws.ptr())
        intact(z, y, loss, dz, ws)
        w = host(ws)
        assert np.isfinite(w[:P]).all() and np.isnan(w[P:]).all(), "the workspace does not hold exactly ceil(n / 1024) partials"
        runs.append((loss, dz, ws))
    (loss, dz, _), (loss2, dz2, _) = runs
    held(f"bce {family} {n} loss", host(loss), np.asarray([r["loss"]]), r["bar_loss"])
    held(f"bce {family} {n} dz", host(dz), r["dz"], r["bar_dz"])
    assert torch.equal(loss.t.view(torch.int32), loss2.t.view(torch.int32)) and torch.equal(dz.t.view(torch.int32), dz2.t.view(torch.int32))
    unchanged([(z, i["z"]), (y, i["y"])])


def test_bce_refuses_empty_batch():
    lib = _lib.load()
    z, loss, dz, ws = G(4, 0.0), G(1, NAN), G(4, NAN), G(8, NAN)
    assert lib.dfm_bce_with_logits(z.ptr(), z.ptr(), 0, loss.ptr(), dz.ptr(), ws.ptr(), _lib.stream_handle()) == 1
    torch.cuda.synchronize()
    assert np.isnan(host(loss)).all() and np.isnan(host(dz)).all() and np.isnan(host(ws)).all()


# =====================================================================================================================
# the predictor's tower
# =====================================================================================================================
@pytest.mark.parametrize("name", list(L.EVAL_CASES))
def test_linear_bn_eval(name):
    """linear_bn_eval_kernel<FAST> and its epilogue: tile edges in M and N, k tails around the 32-deep slice, the fast
    route (K % 4 == 0, ldx % 4 == 0, aligned bases) and the checked one forced by K, by ldx and by either base."""
    c, lib = L.EVAL_CASES[name], _lib.load()
    for fam in FAMILIES:
        i = L.eval_inputs(c, fam)
        xf = np.full((c.M, c.ldx), 7.0, dtype=np.float32)         # the padding holds a value: a fetch from it shows
        xf[:, :c.K] = i["x"]
        x, w = G.of(xf, c.x_shift), G.of(i["w"], c.w_shift)
        v = {k: G.of(i[k]) for k in ("b", "gamma", "beta", "running_mean", "running_var")}
        out = G(c.M * c.N, NAN)
        assert L.operand_fast(x.ptr() % 16 // 4, c.ldx, True, c.M, c.K) and L.operand_fast(w.ptr() % 16 // 4, c.K, True, c.N, c.K) \
            if c.fast else not (x.ptr() % 16 == 0 and w.ptr() % 16 == 0 and c.ldx % 4 == 0 and c.K % 4 == 0)
        call(lib.dfm_linear_bn_eval, x.ptr(), c.ldx, w.ptr(), v["b"].ptr() if c.bias else None, c.M, c.N, c.K, v["gamma"].ptr(),
             v["beta"].ptr(), v["running_mean"].ptr(), v["running_var"].ptr(), float(L.EVAL_EPS), out.ptr())
        r = L.eval_ref(c, i, fam)
        if fam == "int":
            assert np.abs(r["z"]).max() < 2 ** 24
        held(f"linear_bn_eval {name} {fam}", host(out, c.M, c.N), r["out"], r["bar_out"])
        intact(x, w, out, *v.values())
        unchanged([(x, xf), (w, i["w"])] + [(v[k], i[k]) for k in v])


@pytest.mark.parametrize("name", list(L.HEAD_CASES))
def test_predict_head(name):
    """predict_head_kernel on a plain stream: rows around the 32 per workgroup, widths around the 32 floats of a row's
    8 lanes, every `valid` edge, each optional operand NULL or given; rows at and beyond `valid` keep their fill."""
    c, lib = L.HEAD_CASES[name], _lib.load()
    for fam in FAMILIES:
        i = L.head_inputs(c, fam)
        b = {k: G.of(v) for k, v in i.items()}
        logits, probs = G(c.M, NAN), G(c.M, NAN)
        call(lib.dfm_predict_head, b["a"].ptr(), c.M, c.K, b["w"].ptr(), b["b"].ptr() if c.b else None,
             b["fo"].ptr() if c.fo else None, b["extra"].ptr() if c.extra else None, c.valid,
             logits.ptr() if c.logits else None, probs.ptr())
        r = L.head_ref(c, i, fam)
        zl, pr = host(logits), host(probs)
        v = c.valid
        assert np.isnan(zl[v:]).all() and np.isnan(pr[v:]).all(), "a row at or beyond valid was written"
        if c.logits:
            held(f"predict_head {name} {fam} logits", zl[:v], r["logits"][:v], r["bar_logits"][:v], fam == "int")
            if v:
                print(f"predict_head {name} {fam}: device sigmoid error {L.rel_error(pr[:v], L.sigmoid64(zl[:v])):.2f} EPS32 |ref|")
        else:
            assert np.isnan(zl).all()
        held(f"predict_head {name} {fam} probs", pr[:v], r["probs"][:v], r["bar_probs"][:v])
        assert ((pr[:v] >= 0) & (pr[:v] <= 1)).all()
        intact(logits, probs, *b.values())
        unchanged([(b[k], i[k]) for k in i])
