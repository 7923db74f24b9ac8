"""GPU: MixedSchemaPredictor (record gather -> interaction layer -> eval tower -> head) on the MovieLens schema:
the gather against the reference's embedding vectors, the predictor against the reference's eval logits,
``model.eval(); model.predict`` and the oracle, graph against eager, and ``evaluate`` against sklearn and
``compute_ranking_metrics``."""
import json

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests.helpers import (assert_close, cfg_of, fields_of, group, load, load_params, npy, random_fields_batch,
                           schema_from_fields, to_device_batch)
from tests.test_cpu_mixed_predict import movielens_cfg
from tools_shared import criteo_fields

pytestmark = pytest.mark.gpu


def _record(schema, batch, B, labels=None):
    """Device record in the mixed layout of the first n samples of a host batch dict (padded to B)."""
    from deepfm_amd.data.packed import PackedColumns, mixed_record_layout, write_mixed_record
    n = len(next(iter(batch.values())))
    labels = np.zeros(n, np.float32) if labels is None else labels
    cols = PackedColumns(schema, batch, labels)
    out = np.zeros(mixed_record_layout(schema, B)[-1], np.uint8)
    write_mixed_record(out, cols, B, 0, n)
    return torch.from_numpy(out).cuda()


@pytest.mark.parametrize("case", ["emb_movielens_mean", "emb_movielens_sum", "emb_movielens_max",
                                  "emb_layers_test_schema"])
def test_record_gather_vs_golden(case):
    from deepfm_amd.models.layers.embedding import FeatureEmbedding
    g = load(case)
    fields, D = fields_of(g), int(g["fm_dim"])
    schema = schema_from_fields(fields)
    emb = load_params(FeatureEmbedding(schema, fm_embed_dim=D), group(g, "param/"))
    emb.strict_indices = True
    batch = group(g, "batch/")
    B = g["out/first_order"].shape[0]
    labels = np.arange(B, dtype=np.float32)
    rec = _record(schema, batch, B, labels)
    F, T = len(fields), g["out/flat_embeddings"].shape[1]
    fo = torch.full((B, 1), np.nan, device="cuda")
    fe = torch.full((B, F, D), np.nan, device="cuda")
    fm = torch.full((B,), np.nan, device="cuda")
    lab = torch.full((B,), np.nan, device="cuda")
    ld = T + 12                                          # a wider row: only the flat columns are written
    flat = torch.full((B, ld), -7.0, device="cuda")
    emb.forward_record(rec.data_ptr(), B, fo, fe, flat.data_ptr() + 16, ld, fm, lab)
    emb.raise_on_bad_index()
    fl = npy(flat)
    assert (fl[:, :4] == -7.0).all() and (fl[:, 4 + T:] == -7.0).all()
    fl = fl[:, 4:4 + T]
    assert_close(npy(fo), g["out/first_order"], what="first_order")
    assert_close(npy(fe), g["out/field_embeddings"], what="field_embeddings")
    assert_close(fl, g["out/flat_embeddings"], what="flat_embeddings")
    assert_close(npy(fm), O.fm_forward(g["out/field_embeddings"]).reshape(-1), what="fm")
    assert np.array_equal(npy(lab), labels)
    off = 0
    for f in fields:                                     # pure gathers: bit-exact
        if f["type"] == "sparse":
            assert np.array_equal(fl[:, off:off + f["dim"]], g["out/flat_embeddings"][:, off:off + f["dim"]]), f["name"]
        off += f["dim"]
    with torch.no_grad():                                # the general path pools in the same order
        _, _, flat_general = emb(to_device_batch(batch))
    assert np.array_equal(fl, npy(flat_general))
    # without field embeddings or FM value: the same flat and first order
    fo2, flat2 = torch.empty_like(fo), torch.empty(B, T, device="cuda")
    emb.forward_record(rec.data_ptr(), B, fo2, None, flat2.data_ptr(), T)
    assert torch.equal(fo2, fo) and np.array_equal(npy(flat2), fl)


def _golden_model(case="model_deepfm_movielens"):
    from deepfm_amd.models import create_model
    from tests.test_gpu_models_step import _config
    g = load(case)
    c = cfg_of(g)
    model = create_model(c["kind"], schema_from_fields(fields_of(g)), _config(c))
    load_params(model, group(g, "param/"))
    model.embedding.strict_indices = True
    return g, model


@pytest.mark.parametrize("use_graph", [True, False])
def test_movielens_golden_logits(use_graph):
    from deepfm_amd.training import MixedSchemaPredictor
    g, model = _golden_model()
    batch = to_device_batch(group(g, "batch/"))
    n = g["logits_eval"].shape[0]
    pred = MixedSchemaPredictor(model, n, use_graph=use_graph)
    assert model.training
    p = pred.predict(batch)
    logits = pred.last_logits(n)
    assert p.shape == (n, 1)
    assert_close(npy(logits), g["logits_eval"], what="eval logits")
    assert torch.allclose(p, torch.sigmoid(logits), rtol=2e-7, atol=0)
    p5 = pred.predict({k: v[:5] for k, v in batch.items()})
    assert torch.equal(p5, p[:5])


def _movielens_model(kind, fields=None, seed=0):
    from deepfm_amd.models import create_model
    fields = fields or fields_of(load("model_deepfm_movielens"))
    torch.manual_seed(seed)
    with torch.device("cuda"):
        model = create_model(kind, schema_from_fields(fields), movielens_cfg(kind))
    with torch.no_grad():              # non-trivial running statistics
        for m in model.dnn.mlp:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
    model.embedding.strict_indices = True
    return fields, model


def _eval_predict(model, batch):
    was = model.training
    model.eval()
    with torch.no_grad():
        logits = model(batch)
        p = model.predict(batch)
    model.train(was)
    return logits, p


def _snapshot(model):
    return [t.clone() for t in model.state_dict().values()]


@pytest.mark.parametrize("kind", ["deepfm", "xdeepfm", "attention_deepfm"])
def test_models_on_the_movielens_schema(kind):
    from deepfm_amd.training import MixedSchemaPredictor
    fields, model = _movielens_model(kind)
    B = 1000
    rng = np.random.default_rng(7)
    hb = random_fields_batch(fields, B, rng, zero_frac=0.2)
    batch = to_device_batch(hb)
    before = _snapshot(model)
    graph = MixedSchemaPredictor(model, B, use_graph=True)
    eager = MixedSchemaPredictor(model, B, use_graph=False)
    rec = _record(model.schema, hb, B)
    pg, lg = graph.predict_from(rec), graph.last_logits()
    pe = eager.predict_from(rec)
    assert torch.equal(pg, pe) and torch.equal(lg, eager.last_logits())        # graph == eager, bit for bit
    for _ in range(3):
        assert torch.equal(graph.predict_from(rec), pg)
    assert torch.equal(graph.predict(batch), pg)                                 # dict API == record API
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(model)))      # parameters and statistics
    assert model.training
    want_l, want_p = _eval_predict(model, batch)
    assert_close(npy(lg), npy(want_l), what=f"{kind} logits vs model.eval()")
    assert_close(npy(pg), npy(want_p), what=f"{kind} probabilities vs model.predict")
    params = {k: npy(v) for k, v in model.state_dict().items()}
    cfg = movielens_cfg(kind)
    ocfg = dict(fm_dim=16, hidden_units=cfg.dnn.hidden_units)
    if kind == "xdeepfm":
        ocfg.update(cin_layer_sizes=cfg.cin.layer_sizes, cin_split_half=cfg.cin.split_half)
    if kind == "attention_deepfm":
        ocfg.update(num_heads=4, num_layers=1, use_residual=True)
    ref = O.model_logits(kind, fields, params, hb, ocfg, training=False)
    assert_close(npy(lg), ref, what=f"{kind} logits vs oracle")


@pytest.mark.parametrize("combiner", ["mean", "sum", "max"])
def test_bags_every_combiner(combiner):
    from deepfm_amd.training import MixedSchemaPredictor
    fields = json.loads(json.dumps(fields_of(load("model_deepfm_movielens"))))
    for f in fields:
        if f["type"] == "sequence":
            f["combiner"] = combiner
    fields, model = _movielens_model("deepfm", fields, seed=3)
    B = 300
    rng = np.random.default_rng(11)
    hb = random_fields_batch(fields, B, rng, zero_frac=0.1)
    bags = hb["genres"]
    bags[:20] = 0                                        # all-padding bags
    bags[20:40] = rng.integers(1, 20, size=(20, 1))      # one id repeated over the bag
    bags[40:60, :3] = bags[40:60, 3:]                    # repeated halves
    bags[60:80, 1:] = 0                                  # one id then padding
    batch = to_device_batch(hb)
    pred = MixedSchemaPredictor(model, B, use_graph=True)
    p = pred.predict(batch)
    _, want = _eval_predict(model, batch)
    assert_close(npy(p), npy(want), what=f"{combiner} probabilities")
    # an out-of-range id inside a bag
    hb["genres"][5, 2] = 20                              # vocab of genres is 20
    with pytest.raises(IndexError):
        pred.predict(to_device_batch(hb))
    hb["genres"][5, 2] = -1
    with pytest.raises(IndexError):
        pred.predict(to_device_batch(hb))
    hb["genres"][5, 2] = 1
    assert torch.equal(pred.predict(to_device_batch(hb))[6:], p[6:])


def test_evaluate_a_movielens_shaped_split():
    """943 users x (1 positive + 999 candidates), user-major as the reference's eval split, a ragged last batch."""
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.training import MixedSchemaPredictor, compute_ranking_metrics
    from tests.test_gpu_predict import _sk
    fields, model = _movielens_model("deepfm", seed=5)
    U, C, B = 943, 1000, 4096
    n = U * C
    rng = np.random.default_rng(13)
    feats = random_fields_batch(fields, n, rng, zero_frac=0.05)
    feats["user_id"] = np.repeat(np.arange(1, U + 1, dtype=np.int64), C)
    labels = np.zeros(n, np.float32)
    labels[np.arange(U) * C + rng.integers(0, C, U)] = 1.0
    cols = PackedColumns(model.schema, feats, labels)
    assert n % B
    pred = MixedSchemaPredictor(model, B)
    ks = [1, 5, 10, 20]
    m = pred.evaluate(cols, ranking_ks=ks)
    got = pred.last_scores
    assert got.numel() == n and torch.equal(pred.last_labels.cpu(), torch.from_numpy(labels))
    ref = []
    model.eval()
    with torch.no_grad():
        for s in range(0, n, B):
            ref.append(model.predict(to_device_batch({k: v[s:s + B] for k, v in feats.items()})).view(-1))
    model.train()
    ref = torch.cat(ref)
    assert_close(npy(got), npy(ref), what="scores vs model.predict")
    auc, ll = _sk(labels, npy(ref))
    assert abs(m["auc"] - auc) <= 1e-4 and abs(m["logloss"] - ll) <= 1e-5 * ll
    want = compute_ranking_metrics(feats["user_id"], labels, npy(ref), ks, num_users=944)
    own = compute_ranking_metrics(feats["user_id"], labels, npy(got), ks, num_users=944)
    for k in ks:
        for key in (f"HR@{k}", f"NDCG@{k}"):
            assert m[key] == own[key], key                           # the same pass on the same scores
            assert abs(m[key] - want[key]) <= 2.0 / U, key           # a near-tie may swap one user's rank


def test_uniform_schema_agrees_with_fused_predictor():
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    from deepfm_amd.training import FusedPredictor, MixedSchemaPredictor
    from deepfm_amd.data.packed import mixed_record_layout, record_layout
    fields = criteo_fields(1000, 16)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = create_model("deepfm", schema_from_fields(fields), ExperimentConfig())
    with torch.no_grad():
        for m in model.dnn.mlp:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
    B = 4096
    assert mixed_record_layout(model.schema, B)[-1] == record_layout(model.schema, B)[-1]
    hb = random_fields_batch(fields, B, np.random.default_rng(2), zero_frac=0.05)
    rec = _record(model.schema, hb, B)
    pf = FusedPredictor(model, B).predict_from(rec)
    mixed = MixedSchemaPredictor(model, B)
    pm = mixed.predict_from(rec)
    assert torch.allclose(pm, pf, rtol=1e-6, atol=0)
