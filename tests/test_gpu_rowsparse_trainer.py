"""The Trainer over the uniform, row-sparse steps: the table term of the loss (``dfm_tables_sqnorm``,
``dfm_rows_sqnorm``, ``dfm_loss_accumulate_tables``), a main and a tail step over one row-sparse optimizer, and the
epoch loop on them.

Shapes: ``criteo_fields(300, 16, n_sparse=4, n_dense=2)`` (small vocabularies: rows repeat inside and across lists),
tower [64, 32], Adam with lr 1e-3, l2 1e-5, clip 1.0.  Batches of 512 / 4160 / 8200 rows are 1 / 2 / 3 row lists
(``DFM_ROWPLAN_CHUNK`` = 4096); tails of 7 / 257 / 4100 rows are 1 / 1 / 2."""

import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests.helpers import assert_close, npy
from deepfm_amd.data.synthetic import criteo_fields, random_fields_batch, schema_from_fields

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -52
NS, ND = 4, 2
FIELDS = criteo_fields(300, 16, n_sparse=NS, n_dense=ND)
HP = dict(lr=1e-3, l2=1e-5, max_grad_norm=1.0)
CH = 4096
KIND_CFG = {"deepfm": {}, "xdeepfm": dict(cin_layer_sizes=[32, 24, 16], cin_split_half=True),
            "attention_deepfm": dict(num_heads=4, num_layers=1, use_residual=True)}


# ----------------------------------------------------------------------------- 1. the kernels alone
def _table_struct(tables):
    from deepfm_amd import _lib
    S = len(tables) // 2
    arr = (_lib.Table * S)()
    for s in range(S):
        w2, w1 = tables[2 * s], tables[2 * s + 1]
        arr[s].w2, arr[s].w1 = w2.data_ptr(), w1.data_ptr()
        arr[s].stride2, arr[s].stride1 = w2.stride(0), w1.stride(0)
    return arr


def _tables_sqnorm(tables, dim):
    from deepfm_amd import _lib
    lib = _lib.load()
    S = len(tables) // 2
    vocab = (C.c_int32 * S)(*[t.shape[0] for t in tables[0::2]])
    partials = torch.full((lib.dfm_tables_sqnorm_num_partials(sum(vocab)),), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(lib.dfm_tables_sqnorm(_table_struct(tables), S, dim, vocab, partials.data_ptr(), out.data_ptr(),
                                     _lib.stream_handle()))
    return float(out), partials


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("dim", [4, 16, 64])
def test_tables_sqnorm_matches_float64_numpy(dim, packed):
    from deepfm_amd.models.layers.embedding import FeatureEmbedding
    for V in (1, 2, 63, 64, 65, 1023, 1025, 5000):
        fields = criteo_fields([V, 7], dim, n_sparse=2, n_dense=1)
        emb = FeatureEmbedding(schema_from_fields(fields), dim).cuda()
        if packed:
            emb.pack_tables_()
        tables = emb.table_parameters()
        g = torch.Generator(device=DEV).manual_seed(V * 131 + dim)
        with torch.no_grad():
            for t in tables:
                t.copy_(torch.randn(t.shape, device=DEV, generator=g))
        assert (tables[0].stride(0) != dim) == packed
        got, partials = _tables_sqnorm(tables, dim)
        again, partials2 = _tables_sqnorm(tables, dim)
        assert got == again and torch.equal(partials, partials2)            # bitwise reproducible
        want = sum(float(np.sum(npy(t).astype(np.float64) ** 2)) for t in tables)
        n_terms = sum(t.numel() for t in tables)
        assert abs(float(partials.sum()) - got) <= partials.numel() * U * got
        assert abs(got - want) <= n_terms * U * want, (V, dim, got, want)
    with torch.no_grad():                                                  # nothing to sum: exact
        for t in tables:
            t.zero_()
    assert _tables_sqnorm(tables, dim)[0] == 0.0


@pytest.mark.parametrize("L", [1, 2, 3])
def test_rows_sqnorm_sums_the_owned_entries_and_zeroes_the_rest(L):
    from deepfm_amd import _lib
    lib = _lib.load()
    S, D, V = 2, 16, 6000
    rng = np.random.default_rng(50 + L)
    g = torch.Generator(device=DEV).manual_seed(L)
    tables = []
    for s in range(S):
        tables += [torch.randn(V, D, device=DEV, generator=g), torch.randn(V, 1, device=DEV, generator=g)]
    host = [npy(t).astype(np.float64) for t in tables]
    own = lib.dfm_rowadam_num_partials(S, D, L)
    total = own + 5
    for counts in ([CH, 1, 0, CH, 1, CH], [0] * 6, [1] * 6):
        uniq = np.zeros((L, S, CH), np.int32)
        num = np.zeros((L, S), np.int32)
        owner = np.zeros((L, S, CH), np.int32)
        want, terms = 0.0, 0
        for s in range(S):
            seen = set()
            for l in range(L):
                n = counts[(l * S + s) % len(counts)]
                rows = np.sort(rng.choice(np.arange(1, V), size=n, replace=False)).astype(np.int32)
                uniq[l, s, :n], num[l, s] = rows, n
                uniq[l, s, n:] = 5                                  # behind num_uniq: never read as a row
                for j, r in enumerate(rows.tolist()):
                    if r not in seen:                               # a row that repeats in a later list: flag off
                        owner[l, s, j] = 1
                        want += float(np.sum(host[2 * s][r] ** 2) + host[2 * s + 1][r, 0] ** 2)
                        terms += D + 1
                    seen.add(r)
                owner[l, s, n:] = 1                                 # (and flags behind num_uniq do not count)
        partials = torch.full((total,), float("nan"), dtype=torch.float64, device=DEV)
        args = [torch.from_numpy(a).cuda() for a in (uniq, num, owner)]
        _lib.check(lib.dfm_rows_sqnorm(_table_struct(tables), S, D, L, *(a.data_ptr() for a in args),
                                       partials.data_ptr(), total, _lib.stream_handle()))
        p = npy(partials)
        assert not p[own:].any() and np.isfinite(p).all()
        got = float(p.sum())
        if L > 1 and counts[0] == CH:
            assert owner[1:, :, :].sum() < (L - 1) * S * CH          # some repeats were really switched off
        assert abs(got - want) <= terms * U * want, (L, counts, got, want)
        if terms == 0:
            assert got == 0.0
    with pytest.raises(RuntimeError, match="partials do not hold"):
        _lib.check(lib.dfm_rows_sqnorm(_table_struct(tables), S, D, L, *(a.data_ptr() for a in args),
                                       partials.data_ptr(), own - 1, _lib.stream_handle()))


# ----------------------------------------------------------------------------- the pieces
def _model(kind="deepfm", seed=0, dropout=0.0):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    cfg.dnn.hidden_units, cfg.dnn.dropout = [64, 32], dropout
    cfg.cin.layer_sizes, cfg.cin.split_half = [32, 24, 16], True
    cfg.attention.num_heads, cfg.attention.attention_dim, cfg.attention.num_layers = 4, 32, 1
    torch.manual_seed(seed)
    model = create_model(kind, schema_from_fields(FIELDS), cfg).cuda().train()
    model.embedding.set_grad_mode("rowsparse")
    return cfg, model


def _batch(B, rng):
    ids = np.stack([random_fields_batch([f], B, rng, 0.05)[f["name"]] for f in FIELDS[:NS]])
    dense = rng.random((ND, B)).astype(np.float32)
    labels = (rng.random(B) < 0.25).astype(np.float32)
    return ids, dense, labels


def _fresh(B, n, use_graph, kind="deepfm", dropout=0.0, track=True, steps_per_graph=1, capture=True, seed=4):
    from deepfm_amd.training.fused_step import fused_step_class
    from deepfm_amd.training.rowsparse import RowSparseAdam
    cfg, model = _model(kind, seed=seed, dropout=dropout)
    opt = RowSparseAdam(model, **HP)
    torch.manual_seed(17)                                   # the step draws its dropout seed from the device generator
    step = fused_step_class(model)(model, opt, B, use_graph=use_graph)
    if track:
        step.track_loss()
    tail = step.make_tail_step(n)
    if capture:
        step.capture(timed_variant=steps_per_graph > 1, steps_per_graph=steps_per_graph)
        tail.capture()
    return cfg, model, opt, step, tail


def _records(step, tail, pattern, seed):
    """[(step, record, (ids, dense, labels))] for a pattern of "B" / "n"."""
    rng = np.random.default_rng(seed)
    out = []
    for x in pattern:
        s = step if x == "B" else tail
        ids, dense, labels = _batch(s.B, rng)
        rec = s.pack_batches(torch.from_numpy(ids[None]).cuda(), torch.from_numpy(dense[None]).cuda(),
                             torch.from_numpy(labels[None]).cuda())[0]
        out.append((s, rec, (ids, dense, labels)))
    return out


def _state(opt, step):
    """Everything two runs must agree on bit for bit."""
    ts = list(opt._tables) + list(opt.exp_avg) + list(opt.exp_avg_sq)
    ts += [opt.flat_param, opt.flat_m, opt.flat_v, opt.flat_grad, opt.step_count, step.seed]
    if step._loss_acc is not None:
        ts += [step._loss_acc, step._table_sq[0]]
    return ts + list(step.model.buffers())


PATTERN = ["B", "B", "n", "B", "B", "n"]


# ----------------------------------------------------------------------------- 2. main + tail against the oracle
def _oracle_state(model):
    params = {k: npy(v).copy() for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")}
    state = {}
    for k, v in params.items():
        if "running_" not in k:
            state["m/" + k], state["v/" + k] = np.zeros_like(v), np.zeros_like(v)
    return params, state


def _zero_gradient_parameter(k: str) -> bool:
    """A Linear bias in front of a train-mode BatchNorm, the softmax-invariant W_k.bias, the attention stack's last
    LayerNorm bias (a per-feature constant into Linear -> BatchNorm): their reference gradient is rounding noise."""
    pre_bn = k.startswith("dnn.mlp.") and k.endswith(".bias") and int(k.split(".")[2]) % 4 == 0
    return pre_bn or k.endswith("W_k.bias") or k.endswith("layer_norm.bias")


# ReLU kinks.  A hidden pre-activation within rounding of 0 takes one side in the step and the other in the oracle (or in
# the oracle with another summation order): that sample's d embedding jumps by a few per cent, and Adam turns the jump
# into a parameter difference of a fraction of lr on the rows it feeds.  At 8200 rows x 96 hidden units x 6 steps such
# events are the rule: the oracle does not agree with ITSELF to this test's parameter tolerance there.  With its start
# perturbed by half a float32 ulp (relative 3e-8, random signs), or with the other order of its row sums, data seeds 3, 5,
# 6, 7, 9 and 10 leave 1 to 26 elements per table out of `rtol 1e-4, floor 1e-4` (worst |err| 1.1e-4 to 5.5e-4; seed 3:
# 3.0e-4), and the jump is visible in its row gradients (one step's max |d g| 2.7e-6 of 1.4e-3 against 1e-10 before).
# The step misses by the same amount (seed 3: 22 of 4800 elements of one table, worst 3.4e-4; seed 8, the one seed
# where the oracle's two gaps stay below 5e-5: worst 1.9e-4) while its losses agree to 2e-7.  So this case runs kink free,
# as tests/test_gpu_fullsize.py's "-kinkfree" cases do: BatchNorm biases of +6 / -6 keep every pre-activation away
# from 0 (a third of the units dead).  The oracle's own two gaps are then below 5e-5 on every parameter at seeds 3, 7
# and 10 alike.  (All of this measured on the CPU, on the oracle alone.)  Bound, reference, cases and pattern are
# unchanged.
KINK_FREE = {(8200, 4100)}


def _make_kink_free(model):
    with torch.no_grad():
        for m in model.dnn.mlp:
            if isinstance(m, torch.nn.BatchNorm1d):
                c = torch.arange(m.bias.numel(), device=m.bias.device)
                m.bias.copy_(torch.where(c % 3 == 2, -6.0, 6.0))


def _vs_oracle(kind, B, n):
    cfg, model, opt, step, tail = _fresh(B, n, use_graph=True, kind=kind, track=False)
    if (B, n) in KINK_FREE:
        _make_kink_free(model)
    params, state = _oracle_state(model)
    ocfg = dict(fm_dim=16, hidden_units=cfg.dnn.hidden_units, **KIND_CFG[kind])
    for i, (s, rec, (ids, dense, labels)) in enumerate(_records(step, tail, PATTERN, 3)):
        s.run_from(rec)
        batch = {f["name"]: ids[j] for j, f in enumerate(FIELDS[:NS])}
        batch.update({f["name"]: dense[j] for j, f in enumerate(FIELDS[NS:])})
        info = {}
        if kind == "deepfm":
            oloss = O.deepfm_train_step_rowsparse(FIELDS, params, state, batch, labels, ocfg, HP, i + 1,
                                                  exact_order=(s.B <= 512))
        else:
            oloss = O.train_step_rowsparse(kind, FIELDS, params, state, batch, labels, ocfg, HP, i + 1, info=info)
        got = float(s.loss)
        print(f"{kind} ({B}, {n}) step {i} rows {s.B}: loss {got!r} oracle {float(oloss)!r}")
        if kind == "deepfm":
            assert abs(got - float(oloss)) < 2e-5 + 1e-4 * abs(float(oloss)), (i, got, float(oloss))
            continue
        # the other models, as their step tests do (test_gpu_fused_tower.py): the losses of every step to 1e-4, and
        # after the first step the squared gradient norm and the Adam moments, which are linear in the gradients
        assert abs(got - float(oloss)) < 1e-4 * abs(float(oloss)), (i, got, float(oloss))
        if i == 0:
            assert abs(float(opt.sq_norm) - info["sq_norm"]) < 1e-4 * info["sq_norm"]
            for k, slots in opt.state_dict()["state"].items():
                if not _zero_gradient_parameter(k):
                    assert_close(npy(slots["exp_avg"]), state["m/" + k], rtol=1e-4, atol_scale=2e-5,
                                 what=f"{k} exp_avg after step 1")
    assert int(opt.step_count) == len(PATTERN)
    if kind != "deepfm":
        return
    got = {k: npy(v) for k, v in model.state_dict().items()}
    for k, want in params.items():
        if "running_" in k or _zero_gradient_parameter(k):
            continue
        if (B, n) in KINK_FREE and k == "dnn.mlp.1.bias":
            # kink free, the first block's ReLU is the identity on its live units, so this bias is a per-feature
            # constant into Linear -> BatchNorm like the Linear biases above: a zero-gradient parameter (the dead
            # units' gradient is exactly 0).  Measured: oracle 5.9979, step 6.00006 from 6.0, both rounding noise x lr
            continue
        assert_close(got[k], want, rtol=1e-4, atol_scale=0.0, floor=1e-4, what=k)


@pytest.mark.parametrize("B,n", [(512, 7), (4160, 257), (8200, 4100)])
def test_main_and_tail_steps_vs_oracle(B, n):
    _vs_oracle("deepfm", B, n)


@pytest.mark.parametrize("kind", ["xdeepfm", "attention_deepfm"])
def test_main_and_tail_steps_vs_oracle_other_models(kind):
    _vs_oracle(kind, 512, 7)


# ----------------------------------------------------------------------------- 3. bitwise
@pytest.mark.parametrize("n", [7, 2])
def test_graph_equals_eager_for_the_interleaved_sequence_and_capture_restores_shared_state(n):
    B = 512
    finals = []
    for mode in ("eager", "graph", "graph"):
        _, model, opt, step, tail = _fresh(B, n, use_graph=mode != "eager", dropout=0.1, capture=False)
        assert opt.seed_tick is step.seed and tail.seed is step.seed and tail._loss_acc is step._loss_acc
        assert tail._table_sq is step._table_sq and tail._rows is not step._rows
        seed0 = step.seed.clone()
        if mode != "eager":
            for s in (step, tail, step) if len(finals) == 1 else (tail, step, tail):
                before = [t.clone() for t in _state(opt, step)]    # either order of capture, and a re-capture
                s.capture()
                for a, b in zip(before, _state(opt, step)):
                    assert torch.equal(a, b), "capture() changed shared training state"
                assert opt.seed_tick is step.seed and int(opt.step_count) == 0
        step.reset_loss()
        for s, rec, _ in _records(step, tail, PATTERN, 21):
            s.run_from(rec)
        torch.cuda.synchronize()
        assert int(opt.step_count) == len(PATTERN) and int(step.seed) == int(seed0) + len(PATTERN)
        assert float(step._loss_acc[1]) == len(PATTERN)
        finals.append([t.clone() for t in _state(opt, step)] + [step.loss.clone(), tail.loss.clone()])
    for other in finals[1:]:
        for a, b in zip(finals[0], other):
            assert torch.equal(a, b)


def test_groups_singles_and_the_tail_interleaved_equal_eager():
    """B B B | B | n | B B B | B | n: three steps per graph launch with plan look-ahead (three sets of plan buffers),
    eager-gather singles and the tail step (other batch size, other row buffers, other optimizer workspaces when the
    list shapes differ) between them."""
    B, n = 4160, 7                                          # 2 row lists against 1: two workspace shapes
    pattern = ["B", "B", "B", "B", "n", "B", "B", "B", "B", "n"]
    finals = []
    for mode in ("eager", "groups"):
        _, model, opt, step, tail = _fresh(B, n, use_graph=mode != "eager", dropout=0.1,
                                           steps_per_graph=3 if mode == "groups" else 1)
        recs = _records(step, tail, pattern, 33)
        step.reset_loss()
        if mode == "eager":
            for s, rec, _ in recs:
                s.run_from(rec)
        else:
            assert step.cont_slots and step._plan_sets[0] is step._rows and len(opt._workspaces) == 2
            for base in (0, 5):
                step.run_group([recs[base + k][1] for k in range(3)])
                step.run_from(recs[base + 3][1], eager_gather=True)
                tail.run_from(recs[base + 4][1])
        torch.cuda.synchronize()
        assert int(opt.step_count) == len(pattern)
        finals.append([t.clone() for t in _state(opt, step)] + [step.loss.clone(), tail.loss.clone()])
    for a, b in zip(*finals):
        assert torch.equal(a, b)


def test_tracking_on_equals_tracking_off_bitwise():
    B, n = 512, 7
    finals = []
    for track in (False, True):
        _, model, opt, step, tail = _fresh(B, n, use_graph=True, dropout=0.1, track=track)
        assert (step._loss_acc is not None) == track and (step._table_sq is not None) == track
        for s, rec, _ in _records(step, tail, ["B", "B", "n", "B"], 23):
            s.run_from(rec)
        torch.cuda.synchronize()
        finals.append(list(opt._tables) + list(opt.exp_avg) + list(opt.exp_avg_sq) +
                      [opt.flat_param, opt.flat_m, opt.flat_v, step.loss, tail.loss])
    for a, b in zip(*finals):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- 4. the mean
def _table_sq_host(opt):
    return sum(float(np.sum(npy(t).astype(np.float64) ** 2)) for t in opt._tables)


def _touched_sq_host(opt, ids):
    """Sum of squares of the rows a batch updates: the distinct non-padding ids of every SPARSE field."""
    total = 0.0
    for s in range(NS):
        rows = np.unique(ids[s])
        rows = torch.from_numpy(rows[rows != 0]).cuda()
        for t in (opt._tables[2 * s], opt._tables[2 * s + 1]):
            total += float(np.sum(npy(t[rows]).astype(np.float64) ** 2))
    return total


@pytest.mark.parametrize("steps_per_graph", [1, 2])
def test_epoch_mean_is_the_float64_mean_over_an_eager_twins_steps(steps_per_graph):
    B, n = 512, 7
    pattern = ["B", "B", "n", "B", "B", "n"]
    _, model_e, opt_e, step_e, tail_e = _fresh(B, n, use_graph=False, track=False)
    n_tab = sum(t.numel() for t in opt_e._tables)
    l2 = np.float64(np.float32(opt_e.l2))
    terms, bces, S_host, A = [], [], [], _table_sq_host(opt_e)
    for s, rec, (ids, _, _) in _records(step_e, tail_e, pattern, 29):
        p = npy(opt_e.flat_param[:opt_e.n_l2]).astype(np.float64)               # the parameters before the step
        S_host.append(_table_sq_host(opt_e))
        old = _touched_sq_host(opt_e, ids)
        s.run_from(rec)
        A += old + _touched_sq_host(opt_e, ids)
        bce = np.float64(float(s.loss))
        bces.append(bce)
        terms.append(bce + l2 * (np.sum(p * p) + S_host[-1]))
    S_bound = n_tab * U * A                       # every magnitude ever added to or subtracted from S, any order

    _, model, opt, step, tail = _fresh(B, n, use_graph=True, steps_per_graph=steps_per_graph)
    recs = _records(step, tail, pattern, 29)

    def half(first):
        if steps_per_graph == 2:
            step.run_group([recs[first][1], recs[first + 1][1]])
        else:
            step.run_from(recs[first][1]); step.run_from(recs[first + 1][1])
        tail.run_from(recs[first + 2][1])

    step.reset_loss()
    got_S0 = float(step._table_sq[0])
    assert abs(got_S0 - S_host[0]) <= n_tab * U * S_host[0]
    half(0)
    half(3)
    got_loss, got_bce = step.mean_loss(), step.mean_bce()
    want_loss, want_bce = np.mean(terms), np.mean(bces)
    bound = l2 * S_bound + (opt.n_l2 + len(pattern) + 4) * U * want_loss
    print(f"spg {steps_per_graph}: mean_loss {got_loss!r} / {want_loss!r} |err| {abs(got_loss - want_loss):.3e} "
          f"bound {bound:.3e} (rel {abs(got_loss - want_loss) / want_loss:.3e}); l2 * S = {l2 * S_host[-1]:.6e}")
    assert abs(got_loss - want_loss) <= bound
    assert abs(got_bce - want_bce) <= (len(pattern) + 4) * U * want_bce
    assert got_loss - got_bce > 0.5 * l2 * S_host[0] > 0            # the table term is really in
    # S itself after the sequence: the value the last accumulate left is the tables' sum in front of the last step
    got_S = float(step._table_sq[0])
    print(f"  S {got_S!r} / {S_host[-1]!r} |err| {abs(got_S - S_host[-1]):.3e} bound {S_bound:.3e}")
    assert abs(got_S - S_host[-1]) <= S_bound
    # reset_loss() in the middle of a sequence re-derives S from the tables (the pending update is dropped with it)
    step.reset_loss()
    assert step._loss_acc.tolist() == [0.0, 0.0, 0.0]
    S_now = _table_sq_host(opt)
    assert abs(float(step._table_sq[0]) - S_now) <= n_tab * U * S_now
    assert not step._table_sq[1].any() and not step._table_sq[2].any()
    p = npy(opt.flat_param[:opt.n_l2]).astype(np.float64)
    tail.run_from(recs[2][1])
    want = np.float64(float(tail.loss)) + l2 * (np.sum(p * p) + S_now)
    assert abs(step.mean_loss() - want) <= l2 * n_tab * U * S_now + (opt.n_l2 + 4) * U * want


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_of_the_tail_step_and_of_tracking():
    _, model, opt, step, tail = _fresh(64, 5, use_graph=True, capture=False)
    with pytest.raises(ValueError, match="^Expected more than 1 value per channel when training"):
        step.make_tail_step(1)
    with pytest.raises(ValueError, match="no tail step of its own"):
        tail.make_tail_step(3)
    with pytest.raises(ValueError, match="main step"):
        tail.track_loss()
    with pytest.raises(ValueError, match="one step each"):
        tail.capture(steps_per_graph=2)
    assert opt.seed_tick is step.seed
    opt.split = True
    try:
        with pytest.raises(ValueError, match="data-parallel"):
            step.make_tail_step(5)
    finally:
        opt.split = False
    _, model2, opt2, step2, tail2 = _fresh(64, 5, use_graph=True, track=False)
    with pytest.raises(RuntimeError, match="before capture"):
        step2.track_loss()
    # a prepared launch of one step keeps the other from running
    recs = _records(step2, tail2, ["B", "n"], 5)
    step2.prepare_group([recs[0][1]])
    with pytest.raises(RuntimeError, match="prepared launch pending"):
        tail2.run_from(recs[1][1])
    step2.launch_prepared()
    tail2.run_from(recs[1][1])
    torch.cuda.synchronize()
    assert int(opt2.step_count) == 2


# ----------------------------------------------------------------------------- 6. the Trainer
ROWS = 7 * 256 + 37


def _trainer_config(tmp):
    from deepfm_amd.config import ExperimentConfig, TrainingConfig
    cfg = ExperimentConfig(output_dir=str(tmp), seed=3,
                           training=TrainingConfig(num_epochs=3, batch_size=256, lr=1e-3, early_stopping_patience=2,
                                                   metric="auc", scheduler="reduce_on_plateau", ranking_ks=[1, 5]))
    cfg.dnn.hidden_units, cfg.dnn.dropout = [64, 32], 0.1
    cfg.feature.embedding_l2_reg = 1e-5
    cfg.training.gradient_clip_norm = 1.0
    return cfg


def _split(n, seed):
    rng = np.random.default_rng(seed)
    ids, dense, _ = _batch(n, rng)
    feats = {f["name"]: ids[j] for j, f in enumerate(FIELDS[:NS])}
    feats.update({f["name"]: dense[j] for j, f in enumerate(FIELDS[NS:])})
    labels = ((ids[0] % 3 == 0) ^ (rng.random(n) < 0.2)).astype(np.float32)         # learnable from C1
    return types.SimpleNamespace(features=feats, labels=labels)


def _trainer_model(cfg):
    from deepfm_amd.models import create_model
    torch.manual_seed(11)
    model = create_model("deepfm", schema_from_fields(FIELDS), cfg)
    model.embedding.strict_indices = True
    return model


def _loader(ds, cfg, shuffle, depth=4):
    from deepfm_amd.data.device_epoch import DeviceColumns, DeviceEpochLoader
    from deepfm_amd.data.packed import PackedColumns
    cols = PackedColumns(schema_from_fields(FIELDS), ds.features, ds.labels)
    return DeviceEpochLoader(DeviceColumns(cols, DEV), cfg.training.batch_size, shuffle=shuffle, seed=cfg.seed, depth=depth)


@pytest.mark.parametrize("G", [1, 3])
def test_trainer_equals_a_hand_written_loop_over_the_same_pieces(tmp_path, G):
    import deepfm_amd.training as T
    from deepfm_amd.training.fused_step import FusedDeepFMStep
    from deepfm_amd.training.predict import FusedPredictor
    from deepfm_amd.training.rowsparse import RowSparseAdam, build_optimizer
    from deepfm_amd.training.trainer import LoopResult, run_training_loop
    from deepfm_amd.utils.io import load_checkpoint
    data = [_split(ROWS, 1), _split(600, 2), _split(600, 3)]
    # ---- the hand-written loop
    cfg = _trainer_config(tmp_path / "hand")
    B = cfg.training.batch_size
    train, val, test = _loader(data[0], cfg, True, depth=G + 2), _loader(data[1], cfg, False), _loader(data[2], cfg, False)
    assert (train.num_batches, train.tail_rows) == (7, 37)
    model = _trainer_model(cfg).cuda().train()
    model.embedding.set_grad_mode("rowsparse")
    opt = build_optimizer(model, cfg)
    assert isinstance(opt, RowSparseAdam)
    sched = T.build_scheduler(opt, cfg)
    step = FusedDeepFMStep(model, opt, B)
    seed0 = step.seed.clone()
    step.track_loss()
    tail = step.make_tail_step(37)
    step.capture(timed_variant=G > 1, steps_per_graph=G)
    tail.capture()
    pred = FusedPredictor(model, B)
    losses = []

    def train_epoch(epoch):
        train.set_epoch(epoch - 1)
        step.reset_loss()
        whole = 7 // G * G
        for first in range(0, whole, G):
            if G == 1:
                step.run_from(train.record(first))
            else:
                step.run_group([train.record(first + k) for k in range(G)])
        for k in range(whole, 7):
            step.run_from(train.record(k), eager_gather=True)
        tail.run_from(train.tail())
        losses.append(step.mean_loss())
        return losses[-1]

    best = {}
    result = run_training_loop(cfg.training, train_epoch,
                               lambda: pred.evaluate_loader(val, ranking_ks=cfg.training.ranking_ks),
                               lambda e, m: best.update(epoch=e, metric=m, state=opt.state_dict()), sched)
    assert isinstance(result, LoopResult)
    want_test = pred.evaluate_loader(test, ranking_ks=cfg.training.ranking_ks)
    want = [t.clone() for t in _state(opt, step)]
    assert int(opt.step_count) == result.total_epochs * 8 and all(np.isfinite(losses))
    # ---- the Trainer
    cfg2 = _trainer_config(tmp_path / "run")
    model2 = _trainer_model(cfg2)
    model2.embedding.set_grad_mode("rowsparse")
    seen = []
    trainer = T.Trainer(model2, schema_from_fields(FIELDS), cfg2, _loader(data[0], cfg2, True, depth=G + 2),
                        _loader(data[1], cfg2, False), _loader(data[2], cfg2, False), steps_per_graph=G)
    assert trainer.rowsparse and trainer.steps_per_graph == G and trainer.tail_step.B == 37
    assert type(trainer.step) is FusedDeepFMStep and type(trainer.predictor) is FusedPredictor
    trainer.step.seed.copy_(seed0)                            # the one thing drawn from the device generator
    inner = trainer._train_epoch
    trainer._train_epoch = lambda e: seen.append(inner(e)) or seen[-1]
    got = trainer.train()
    for a, b in zip(want, _state(trainer.optimizer, trainer.step)):
        assert torch.equal(a, b)
    assert seen == losses and got == result.best_metrics and {"auc", "logloss"} <= set(got)
    ck = load_checkpoint(tmp_path / "run" / "best_model.pt")
    assert sorted(ck) == ["best_metric", "epoch", "model_state_dict", "optimizer_state_dict"]
    assert ck["epoch"] == best["epoch"] == result.best_epoch and ck["best_metric"] == best["metric"]
    with open(tmp_path / "run" / "results.json") as f:
        res = json.load(f)
    assert res["training_info"] == {"best_epoch": result.best_epoch, "total_epochs": result.total_epochs}
    assert res["val_metrics"] == result.best_metrics and res["test_metrics"] == want_test
    # the checkpoint's optimizer state loads back into a fresh optimizer bit for bit
    cfg3, model3 = _trainer_config(tmp_path / "load"), None
    model3 = _trainer_model(cfg3).cuda().train()
    model3.embedding.set_grad_mode("rowsparse")
    opt3 = build_optimizer(model3, cfg3)
    opt3.load_state_dict(ck["optimizer_state_dict"])
    sd, sd3 = best["state"], opt3.state_dict()
    assert sd3["step"] == sd["step"] == ck["optimizer_state_dict"]["step"]
    for name, slots in sd["state"].items():
        for k, v in slots.items():
            assert torch.equal(sd3["state"][name][k], v), (name, k)
            assert torch.equal(ck["optimizer_state_dict"]["state"][name][k].to(v.device), v), (name, k)
    # a caller's loader whose ring does not hold a group is refused
    if G > 1:
        with pytest.raises(ValueError, match="its ring must hold a group"):
            T.Trainer(model3, schema_from_fields(FIELDS), cfg3, _loader(data[0], cfg3, True, depth=G + 1),
                      _loader(data[1], cfg3, False), _loader(data[2], cfg3, False), steps_per_graph=G)


def test_trainer_drop_in_form_and_the_dense_mode_refusal(tmp_path):
    """Objects with ``.features`` / ``.labels``; ``steps_per_graph`` is clipped to the epoch's whole batches."""
    import deepfm_amd.training as T
    cfg = _trainer_config(tmp_path / "drop_in")
    cfg.training.num_epochs = 2
    model = _trainer_model(cfg)
    with pytest.raises(ValueError, match=r"uniform schema: use the row-sparse step \(set_grad_mode\('rowsparse'\)"):
        T.Trainer(model, schema_from_fields(FIELDS), cfg, _split(600, 1), _split(300, 2), _split(300, 3))
    model.embedding.set_grad_mode("rowsparse")
    trainer = T.Trainer(model, schema_from_fields(FIELDS), cfg, _split(600, 1), _split(300, 2), _split(300, 3),
                        steps_per_graph=8)
    assert (len(trainer.train_ds), trainer.train_ds.tail_rows, trainer.tail_step.B) == (2, 88, 88)
    assert trainer.steps_per_graph == 2 and trainer.train_ds.depth >= 4
    before = {k: v.clone() for k, v in model.named_parameters()}
    metrics = trainer.train()
    assert "auc" in metrics and "logloss" in metrics and 0 <= metrics["auc"] <= 1 and metrics["logloss"] > 0
    assert int(trainer.optimizer.step_count) == 2 * 3
    assert any(not torch.equal(before[k], v) for k, v in model.named_parameters())
    assert (tmp_path / "drop_in" / "best_model.pt").exists() and (tmp_path / "drop_in" / "results.json").exists()
