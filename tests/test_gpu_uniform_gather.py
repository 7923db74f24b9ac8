"""GPU parity of the uniform embedding gather (csrc/embedding.hip) at every compiled width and at field
mixes other than Criteo's 26 + 13: the 8-wave kernel (shape 4) with one and several passes, plans with
no SPARSE or no DENSE field, the slot caps, the general path past them, the forced launch shapes, the
out-of-range flag, the dense-gradient backward and the training steps built on the gather.

Bars (BASELINE.json): SPARSE row gathers bit-exact; everything floating point within 1e-4 relative
(helpers.assert_close).  The schemas interleave SPARSE and DENSE fields, so a slot's field index differs
from its slot index, and every SPARSE field has its own (small) vocabulary.
"""
import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests.helpers import assert_close, npy, random_fields_batch, schema_from_fields, to_device_batch
from tests.test_gpu_models_step import _oracle_state

pytestmark = pytest.mark.gpu

WIDTHS = [4, 8, 16, 32, 64, 128, 256]
# (SPARSE, DENSE) field counts: small, one of each, SPARSE only, DENSE only, Criteo, the SPARSE slot cap at the
# 64-field limit, and past the SPARSE (48) and DENSE (32) slot caps, where the plan is not uniform
MIXES = [(3, 2), (1, 1), (9, 0), (0, 4), (26, 13), (48, 16), (49, 1), (5, 33)]
MAX_SPARSE_SLOTS, MAX_DENSE_SLOTS = 48, 32


def _fields(ns, nd, D, sparse_first=False):
    """ns SPARSE + nd DENSE fields of width D; interleaved (S D S D ... then the rest) unless ``sparse_first``."""
    kinds = ["sparse"] * ns + ["dense"] * nd
    if not sparse_first:
        kinds = []
        for k in range(max(ns, nd)):
            kinds += (["sparse"] if k < ns else []) + (["dense"] if k < nd else [])
    fields, si, di = [], 0, 0
    for kind in kinds:
        if kind == "sparse":
            fields.append(dict(name=f"s{si}", type="sparse", vocab=2 + (37 * si + 11) % 150, dim=D, max_len=1,
                               combiner="mean"))
            si += 1
        else:
            fields.append(dict(name=f"d{di}", type="dense", vocab=0, dim=D, max_len=1, combiner="mean"))
            di += 1
    return fields


def _module(fields, D, seed=0):
    from deepfm_amd.models.layers.embedding import FeatureEmbedding
    torch.manual_seed(seed)
    emb = FeatureEmbedding(schema_from_fields(fields), D)
    with torch.no_grad():       # non-zero DENSE biases (the initialisation leaves them 0)
        for f in fields:
            if f["type"] == "dense":
                for m in (emb.second_order_embeddings[f["name"]], emb.first_order_embeddings[f["name"]]):
                    m.bias.uniform_(-0.5, 0.5)
    emb.strict_indices = True
    return emb.cuda()


def _params(emb):
    return {k: npy(v).copy() for k, v in emb.state_dict().items()}


def _batch(fields, B, rng):
    batch = random_fields_batch(fields, B, rng, zero_frac=0.1)
    for j, f in enumerate(fields):          # a padding id in sample 0 of every other SPARSE field
        if f["type"] == "sparse" and j % 2 == 0:
            batch[f["name"]][0] = 0
    return batch


def _fm64(fe):
    e = np.asarray(fe, dtype=np.float64)
    s = e.sum(axis=1)
    return 0.5 * (s * s - (e * e).sum(axis=1)).sum(axis=1, keepdims=True)


def _sparse_cols(fields):
    return [j for j, f in enumerate(fields) if f["type"] == "sparse"]


def _check_forward(fields, params, D, batch, fo, fe, flat, fm=None, what=""):
    ofo, ofe, ofl = O.embedding_forward(fields, params, batch, D)
    sp = _sparse_cols(fields)
    assert fo.shape == ofo.shape and fe.shape == ofe.shape and flat.shape == ofl.shape, what
    assert np.array_equal(fe[:, sp], ofe[:, sp]), f"{what}: SPARSE rows not bit-exact"
    assert_close(fe, ofe, what=f"{what} fe")
    assert_close(fo, ofo, what=f"{what} fo")
    assert_close(flat, ofl, what=f"{what} flat")
    if fm is not None:
        # 0.5 * sum_d (S_d^2 - SQ_d) cancels: a sample whose exact value is 0 (one non-padding field) is held to fp32
        # rounding of the sums of squares it is the difference of
        floor = 1e-6 * float((ofe.astype(np.float64) ** 2).sum(axis=(1, 2)).max())
        assert_close(fm, _fm64(ofe), what=f"{what} fm", floor=floor)


def _batches(D):
    spw = 64 // (D // 4)
    return sorted({1, max(spw - 1, 1), spw + 1, 4099})


@pytest.mark.parametrize("mix", MIXES, ids=lambda m: f"{m[0]}s{m[1]}d")
@pytest.mark.parametrize("D", WIDTHS)
def test_forward_vs_oracle(D, mix):
    from deepfm_amd import _lib
    ns, nd = mix
    fields = _fields(ns, nd, D)
    emb = _module(fields, D, seed=D + 7 * ns + nd)
    params = _params(emb)
    uniform = ns <= MAX_SPARSE_SLOTS and nd <= MAX_DENSE_SLOTS
    rng = np.random.default_rng(D * 1000 + ns * 10 + nd)
    for B in _batches(D):
        batch = _batch(fields, B, rng)
        db = to_device_batch(batch)
        with torch.no_grad():
            fo, fe, flat = emb(db)
            inputs, _ = emb._gather_inputs(db)
            fo2, fe2, _, fm = emb._launch_forward(inputs, B, want_fm=True)
        assert _lib.load().dfm_embedding_plan_is_uniform(emb._plan) == int(uniform)
        what = f"D={D} {ns}+{nd} B={B}"
        _check_forward(fields, params, D, batch, npy(fo), npy(fe), npy(flat), npy(fm) if uniform else None, what)
        if uniform:
            assert flat.data_ptr() == fe.data_ptr(), what                  # the flat view aliases fe
            assert torch.equal(fe2, fe) and torch.equal(fo2, fo), what     # FM outputs change nothing else
        else:
            assert fm is None and flat.data_ptr() != fe.data_ptr(), what


def _forced_shapes(emb, inputs, B):
    """{shape: (fo, fe, fm)} of the gather launched in each forced shape 1-6."""
    from deepfm_amd import _lib
    lib = _lib.load()
    out = {}
    try:
        for shape in range(1, 7):
            _lib.check(lib.dfm_gather_set_shape(shape))
            with torch.no_grad():
                fo, fe, _, fm = emb._launch_forward(inputs, B, want_fm=True)
            out[shape] = (npy(fo), npy(fe), npy(fm))
    finally:
        _lib.check(lib.dfm_gather_set_shape(0))
    return out


@pytest.mark.parametrize("D", [4, 16, 32, 256])
def test_forced_shapes_on_the_criteo_schema(D):
    """Shapes 1-6 on 26 SPARSE + 13 DENSE (5 and 6: the two-wave kernel at D = 16 / 32, shape 4 elsewhere):
    the same field embeddings bit for bit, first order and FM within the bar."""
    fields = _fields(26, 13, D, sparse_first=True)
    emb = _module(fields, D, seed=3)
    params = _params(emb)
    rng = np.random.default_rng(D)
    for B in (64 // (D // 4) + 1, 4099):
        batch = _batch(fields, B, rng)
        inputs, _ = emb._gather_inputs(to_device_batch(batch))
        res = _forced_shapes(emb, inputs, B)
        for shape, (fo, fe, fm) in res.items():
            _check_forward(fields, params, D, batch, fo, fe, fe.reshape(B, -1), fm, f"D={D} B={B} shape {shape}")
            assert np.array_equal(fe, res[4][1]), f"D={D} B={B}: shape {shape} fe differs from shape 4"


@pytest.mark.parametrize("mix", [(27, 3), (16, 14), (9, 0), (0, 4), (3, 2)], ids=lambda m: f"{m[0]}s{m[1]}d")
@pytest.mark.parametrize("D", [8, 64])
def test_forced_shapes_on_other_schemas(D, mix):
    """Where a forced shape does not apply — shape 1 (one pass of 26 + 13 slots) on more fields of a kind,
    shapes 1-3 on a plan without SPARSE or DENSE fields, 5 / 6 off the Criteo counts — the launch must still
    compute every field."""
    ns, nd = mix
    fields = _fields(ns, nd, D)
    emb = _module(fields, D, seed=5)
    params = _params(emb)
    B = 4099
    batch = _batch(fields, B, np.random.default_rng(ns + nd))
    inputs, _ = emb._gather_inputs(to_device_batch(batch))
    res = _forced_shapes(emb, inputs, B)
    for shape, (fo, fe, fm) in res.items():
        _check_forward(fields, params, D, batch, fo, fe, fe.reshape(B, -1), fm, f"D={D} {ns}+{nd} shape {shape}")


@pytest.mark.parametrize("bad", [-1, "vocab"])
@pytest.mark.parametrize("D,mix", [(16, (26, 13)), (32, (26, 13)), (8, (48, 16)), (64, (9, 0)), (256, (3, 2))])
def test_out_of_range_ids_raise_index_error(D, mix, bad):
    """An id < 0 or >= vocabulary in the LAST SPARSE field at the LAST sample (the ragged tail workgroup; with
    48 SPARSE fields, the second pass of the 8-wave kernel) raises IndexError — through the two-wave kernel at
    26 + 13 and D = 16 / 32, through the 8-wave kernel elsewhere; the flag is cleared and a good batch passes."""
    ns, nd = mix
    fields = _fields(ns, nd, D, sparse_first=(mix == (26, 13)))
    emb = _module(fields, D)
    B = 64 // (D // 4) + 1
    batch = _batch(fields, B, np.random.default_rng(1))
    last = [f for f in fields if f["type"] == "sparse"][-1]
    good = to_device_batch(batch)
    batch[last["name"]][B - 1] = -1 if bad == -1 else last["vocab"]
    with torch.no_grad():
        with pytest.raises(IndexError):
            emb(to_device_batch(batch))
        emb(good)                                  # no stale flag


@pytest.mark.parametrize("mix", [(7, 3), (9, 0), (0, 4)], ids=lambda m: f"{m[0]}s{m[1]}d")
@pytest.mark.parametrize("D", [4, 64, 256])
def test_dense_grad_backward_vs_oracle(D, mix):
    """Dense-gradient mode on a uniform plan: the SPARSE scatter and emb_bwd_dense_fields_uniform (DENSE Linear
    gradients, 4 columns per block) against the oracle's autograd, duplicate ids included."""
    ns, nd = mix
    fields = _fields(ns, nd, D)
    emb = _module(fields, D, seed=11)
    params = _params(emb)
    B = 64 // (D // 4) * 20 + 3
    rng = np.random.default_rng(D + ns)
    batch = _batch(fields, B, rng)
    F = len(fields)
    g_fo = rng.standard_normal((B, 1)).astype(np.float32)
    g_fe = rng.standard_normal((B, F, D)).astype(np.float32)
    fo, fe, _ = emb(to_device_batch(batch))
    assert emb._plan_uniform
    ((fo * torch.from_numpy(g_fo).cuda()).sum() + (fe * torch.from_numpy(g_fe).cuda()).sum()).backward()
    want = O.embedding_backward(fields, params, batch, D, g_fo, g_fe, np.zeros((B, F * D), np.float32))
    names = [k for k, _ in emb.named_parameters()]
    assert sorted(names) == sorted(want)
    for k, p in emb.named_parameters():
        assert p.grad is not None, k
        assert_close(npy(p.grad), want[k], what=f"D={D} {ns}+{nd} {k}")
        if k.startswith(("second_order_embeddings.s", "first_order_embeddings.s")):
            assert not npy(p.grad)[0].any(), f"{k}: gradient in the padding row"


# ---------------------------------------------------------------------------------------------- training steps
STEP_KINDS = ["rowsparse-eager", "rowsparse-graph", "fused-eager", "fused-graph"]
# Adam moves an element by lr * g / (|g| + eps), eps = 1e-8: where the exact gradient is within 10x of eps (a
# random cancellation, 1 element in ~10^4 here), fp32 rounding of g changes the update by up to ~lr, so no
# bar on the parameter holds; above it, rounding moves the update by < 1e-6
ADAM_ILL_CONDITIONED = 1e-7


def _ill_conditioned(masks, info):
    """Mark (in place) the parameter elements whose clipped gradient of this oracle step is ill-conditioned."""
    for k, g in info["grads"].items():
        masks[k] |= np.abs(g * info["coef"]) < ADAM_ILL_CONDITIONED
    for name, (uniq, r2, r1) in info["rows"].items():
        masks[f"embedding.second_order_embeddings.{name}.weight"][uniq] |= np.abs(r2 * info["coef"]) < ADAM_ILL_CONDITIONED
        masks[f"embedding.first_order_embeddings.{name}.weight"][uniq, 0] |= np.abs(r1 * info["coef"]) < ADAM_ILL_CONDITIONED


@pytest.mark.parametrize("kind", STEP_KINDS)
@pytest.mark.parametrize("D,mix", [(8, (7, 3)), (64, (7, 3)), (16, (9, 0))], ids=["D8-7s3d", "D64-7s3d", "D16-9s0d"])
def test_train_steps_vs_oracle(D, mix, kind):
    """Two row-sparse training steps (RowSparseTrainStep / FusedDeepFMStep, eager with load_batch or captured
    graph with run_from on pack_batches records; packed row-record tables except in the first kind) against
    the oracle: the staged gather, row plan, row gradients, DENSE-field gradients and row-wise Adam at widths
    and field mixes other than Criteo's."""
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    from deepfm_amd.training.fused_step import FusedDeepFMStep
    from deepfm_amd.training.rowsparse import RowSparseAdam
    from deepfm_amd.training.step import RowSparseTrainStep
    ns, nd = mix
    fields = _fields(ns, nd, D)
    cfg = ExperimentConfig()
    cfg.dnn.hidden_units, cfg.dnn.dropout = [64, 32], 0.0
    cfg.feature.fm_embed_dim = D
    torch.manual_seed(D + ns)
    model = create_model("deepfm", schema_from_fields(fields), cfg).cuda().train()
    model.embedding.set_grad_mode("rowsparse")
    if kind != "rowsparse-eager":
        model.embedding.pack_tables_()
    hp = dict(lr=1e-3, l2=1e-5, max_grad_norm=1.0)
    params, state = _oracle_state(model)
    opt = RowSparseAdam(model, lr=hp["lr"], l2=hp["l2"], max_grad_norm=hp["max_grad_norm"])
    B, n = 516, 2          # B % 4 == 0: pack_batches records stay 16-byte aligned; ragged tail at D = 8, 16
    Step = FusedDeepFMStep if kind.startswith("fused") else RowSparseTrainStep
    graph = kind.endswith("graph")
    if Step is FusedDeepFMStep:
        assert Step.eligible(model)
    step = Step(model, opt, B, use_graph=graph)
    rng = np.random.default_rng(D)
    sp = [f for f in fields if f["type"] == "sparse"]
    de = [f for f in fields if f["type"] == "dense"]
    batches = [_batch(fields, B, rng) for _ in range(n)]
    ids = np.stack([np.stack([b[f["name"]] for f in sp]) if sp else np.zeros((0, B), np.int64) for b in batches])
    dense = np.stack([np.stack([b[f["name"]] for f in de]) if de else np.zeros((0, B), np.float32) for b in batches])
    labels = (rng.random((n, B)) < 0.25).astype(np.float32)
    t_ids, t_dense, t_labels = (torch.from_numpy(a).cuda() for a in (ids, dense, labels))
    if graph:
        recs = step.pack_batches(t_ids, t_dense, t_labels)
        step.capture()
    ocfg = dict(fm_dim=D, hidden_units=cfg.dnn.hidden_units)
    ill = {k: np.zeros(v.shape, bool) for k, v in params.items()}
    for i in range(n):
        if graph:
            step.run_from(recs[i])
        else:
            step.load_batch(t_ids[i], t_dense[i], t_labels[i])
            step.run()
        info = {}
        oloss = O.deepfm_train_step_rowsparse(fields, params, state, batches[i], labels[i], ocfg, hp, i + 1,
                                              exact_order=True, info=info)
        _ill_conditioned(ill, info)
        assert abs(float(step.loss) - float(oloss)) < 2e-5 + 1e-4 * abs(float(oloss)), (i, float(step.loss), float(oloss))
    torch.cuda.synchronize()
    got = {k: npy(v) for k, v in model.state_dict().items()}
    n_ill = n_all = 0
    for k, want in params.items():
        if "running_" in k:
            continue
        if k.startswith("dnn.mlp.") and k.endswith(".bias") and int(k.split(".")[2]) % 4 == 0:
            continue        # zero-gradient parameter (Linear bias in front of BatchNorm)
        keep = ~ill[k]
        n_ill, n_all = n_ill + int(ill[k].sum()), n_all + ill[k].size
        assert_close(got[k][keep], want[keep], rtol=1e-4, atol_scale=0.0, floor=1e-4, what=f"{kind} {k}")
    assert n_ill <= max(3, n_all // 1000), f"{n_ill} / {n_all} ill-conditioned elements"
