"""GPU: FusedPredictor (eval-mode forward on dfm_linear_bn_eval / dfm_predict_head, one graph launch per batch) and
the on-device AUC / log loss, against the goldens, the model's own eval forward, the oracle and sklearn."""
import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from tests.helpers import (assert_close, cfg_of, fields_of, group, load, load_params, npy, schema_from_fields,
                           to_device_batch)
from tools_shared import criteo_fields

pytestmark = pytest.mark.gpu

V, B, S, ND = 1_000_000, 4096, 26, 13


@pytest.mark.parametrize("case", ["model_deepfm", "model_xdeepfm", "model_attention_deepfm"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_goldens(case, use_graph):
    from deepfm_amd.models import create_model
    from deepfm_amd.training import FusedPredictor
    from tests.test_gpu_models_step import _config
    g = load(case)
    c = cfg_of(g)
    model = create_model(c["kind"], schema_from_fields(fields_of(g)), _config(c))
    load_params(model, group(g, "param/"))
    model.embedding.strict_indices = True
    batch = to_device_batch(group(g, "batch/"))
    n = g["logits_eval"].shape[0]
    pred = FusedPredictor(model, n, use_graph=use_graph)
    assert model.training                                  # the predictor does not flip it
    p = pred.predict(batch)
    logits = pred.last_logits(n)
    assert p.shape == (n, 1)
    assert_close(npy(logits), g["logits_eval"], what="eval logits")
    assert torch.allclose(p, torch.sigmoid(logits), rtol=2e-7, atol=0)
    # a short batch: the first rows, padded inside the predictor
    p5 = pred.predict({k: v[:5] for k, v in batch.items()})
    assert torch.equal(p5, p[:5])


def _fullsize(kind, steps=20):
    """BASELINE.json configurations 2 / 3 / 4 (V = 10^6, B = 4096, tower [256, 128, 64], dropout 0.1) after
    ``steps`` fused graph steps: non-trivial running statistics and trained weights."""
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    from deepfm_amd.training.fused_step import fused_step_class
    from deepfm_amd.training.rowsparse import RowSparseAdam
    D = 32 if kind == "attention_deepfm" else 16
    cfg = ExperimentConfig()
    cfg.dnn.dropout = 0.1
    cfg.feature.fm_embed_dim = D
    if kind == "xdeepfm":
        cfg.cin.layer_sizes, cfg.cin.split_half = [128, 128, 128], True
    if kind == "attention_deepfm":
        cfg.attention.num_heads, cfg.attention.attention_dim = 4, 64
        cfg.attention.num_layers, cfg.attention.use_residual = 1, True
    fields = criteo_fields(V, D)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = create_model(kind, schema_from_fields(fields), cfg)
    model.train()
    model.embedding.pack_tables_()
    if kind != "deepfm":       # fresh V = 10^6 tables are ~2e-3: scale to trained-like values (test_gpu_fullsize.py)
        with torch.no_grad():
            for nm in model.embedding.packed:
                model.embedding.packed[nm]["buffer"][:, :D + 1].mul_(100.0)
    model.embedding.set_grad_mode("rowsparse")
    opt = RowSparseAdam(model, lr=1e-3, l2=1e-5, max_grad_norm=1.0)
    step = fused_step_class(model)(model, opt, B, use_graph=True)
    g = torch.Generator(device="cuda").manual_seed(5)
    n = 4
    ids = torch.randint(0, V, (n, S, B), generator=g, device="cuda", dtype=torch.int64)
    dense = torch.rand((n, ND, B), generator=g, device="cuda")
    labels = (torch.rand((n, B), generator=g, device="cuda") < 0.25).float()
    records = step.pack_batches(ids, dense, labels)
    step.load_packed(records[0])
    step.capture()
    for k in range(steps):
        step.run_from(records[k % n])
    torch.cuda.synchronize()
    return model, opt, step, fields, cfg, (ids, dense, labels)


def _batch_dict(model, ids, dense):
    out, si, di = {}, 0, 0
    from deepfm_amd.data.schema import FeatureType
    for name, spec in model.schema.fields.items():
        if spec.feature_type is FeatureType.SPARSE:
            out[name] = ids[si].contiguous(); si += 1
        else:
            out[name] = dense[di].contiguous(); di += 1
    return out


def _eval_logits(model, batch):
    was = model.training
    model.eval()
    with torch.no_grad():
        out = model(batch)
    model.train(was)
    return out


def _oracle_logits(kind, model, fields, cfg, batch):
    """Oracle eval logits on compact tables: only the rows the batch reads (ids renumbered per field)."""
    sd = {k: npy(v) for k, v in model.state_dict().items() if "embeddings.C" not in k}
    small_fields, small_batch = [], {}
    for f in fields:
        name = f["name"]
        x = npy(batch[name])
        if f["type"] != "sparse":
            small_fields.append(f); small_batch[name] = x
            continue
        u = np.unique(x)
        u = u[u != 0]                               # 0 stays the padding id, row 0 of the compact table
        rows = torch.from_numpy(u).cuda()
        for which in ("second", "first"):
            key = f"embedding.{which}_order_embeddings.{name}.weight"
            w = npy(getattr(model.embedding, f"{which}_order_embeddings")[name].weight[rows])
            sd[key] = np.concatenate([np.zeros((1, w.shape[1]), np.float32), w])
        small_batch[name] = np.where(x == 0, 0, np.searchsorted(u, x) + 1)
        small_fields.append(dict(f, vocab=len(u) + 1))
    ocfg = dict(fm_dim=cfg.feature.fm_embed_dim, hidden_units=cfg.dnn.hidden_units)
    if kind == "xdeepfm":
        ocfg.update(cin_layer_sizes=cfg.cin.layer_sizes, cin_split_half=cfg.cin.split_half)
    if kind == "attention_deepfm":
        ocfg.update(num_heads=4, num_layers=1, use_residual=True)
    return O.model_logits(kind, small_fields, sd, small_batch, ocfg, training=False)


def _state(model, opt, step):
    ts = [v.clone() for v in model.state_dict().values()]
    ts += [b["buffer"].clone() for b in model.embedding.packed.values()]
    ts += [opt.flat_param.clone(), opt.flat_m.clone(), opt.flat_v.clone(), opt.step_count.clone(), step.seed.clone()]
    return ts


@pytest.mark.parametrize("kind", ["deepfm", "xdeepfm", "attention_deepfm"])
def test_fullsize_after_training(kind):
    from deepfm_amd.training import FusedPredictor
    model, opt, step, fields, cfg, (ids, dense, labels) = _fullsize(kind)
    bn = model.dnn.mlp[1]
    assert int(bn.num_batches_tracked) >= 20 and float(bn.running_var.std()) > 0     # non-trivial statistics
    g = torch.Generator(device="cuda").manual_seed(99)
    t_ids = torch.randint(0, V, (1, S, B), generator=g, device="cuda", dtype=torch.int64)
    t_dense = torch.rand((1, ND, B), generator=g, device="cuda")
    rec = step.pack_batches(t_ids, t_dense, torch.zeros(1, B, device="cuda"))[0].contiguous()
    before = _state(model, opt, step)
    rowplan = model.embedding.rowsparse.sorted_pos.clone()
    graph = FusedPredictor(model, B, use_graph=True)
    eager = FusedPredictor(model, B, use_graph=False)
    pg = graph.predict_from(rec)
    lg = graph.last_logits()
    pe = eager.predict_from(rec)
    assert torch.equal(pg, pe) and torch.equal(lg, eager.last_logits())        # graph == eager, bit for bit
    for _ in range(10):
        assert torch.equal(graph.predict_from(rec), pg)                         # repeats are bit-identical
    after = _state(model, opt, step)
    assert all(torch.equal(a, b) for a, b in zip(before, after))                # no state changed
    assert torch.equal(model.embedding.rowsparse.sorted_pos, rowplan)           # no row plan built
    assert model.training
    batch = _batch_dict(model, t_ids[0], t_dense[0])
    want = _eval_logits(model, batch)
    assert_close(npy(lg), npy(want), what=f"{kind} logits vs model.eval()")
    assert_close(npy(pg), npy(torch.sigmoid(want)), what=f"{kind} probabilities vs model.eval()")
    ref = _oracle_logits(kind, model, fields, cfg, batch)
    assert_close(npy(lg), ref, what=f"{kind} logits vs oracle")
    # the dict API agrees with the record API
    assert torch.equal(graph.predict(batch), pg)


def test_interleaved_with_training():
    from deepfm_amd.training import FusedPredictor
    model, opt, step, fields, cfg, (ids, dense, labels) = _fullsize("deepfm", steps=2)
    records = step.pack_batches(ids, dense, labels)
    pred = FusedPredictor(model, B, use_graph=True)
    for k in range(6):
        step.run_from(records[k % 4])
        rec = records[(k + 1) % 4]
        p = pred.predict_from(rec)
        want = _eval_logits(model, _batch_dict(model, ids[(k + 1) % 4], dense[(k + 1) % 4]))
        assert_close(npy(pred.last_logits()), npy(want), what=f"step {k}")
        assert_close(npy(p), npy(torch.sigmoid(want)), what=f"step {k} probabilities")


def _small_deepfm(vocab=1000, seed=0):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.models import create_model
    cfg = ExperimentConfig()
    torch.manual_seed(seed)
    with torch.device("cuda"):
        model = create_model("deepfm", schema_from_fields(criteo_fields(vocab, 16)), cfg)
    with torch.no_grad():              # non-trivial running statistics
        for m in model.dnn.mlp:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
    return model


def _columns(model, n, seed, vocab=1000, rate=0.3):
    from deepfm_amd.data.packed import PackedColumns
    rng = np.random.default_rng(seed)
    feats = {}
    for name, spec in model.schema.fields.items():
        feats[name] = (rng.integers(0, vocab, n) if spec.feature_type.name == "SPARSE"
                       else rng.random(n).astype(np.float32))
    return PackedColumns(model.schema, feats, (rng.random(n) < rate).astype(np.float32))


def test_ragged_split_scores_every_sample_as_a_full_batch():
    from sklearn.metrics import log_loss, roc_auc_score

    from deepfm_amd.data.packed import record_layout
    from deepfm_amd.training import FusedPredictor
    model = _small_deepfm()
    n = 3 * B + 123
    cols = _columns(model, n, 1)
    pred = FusedPredictor(model, B)
    m = pred.evaluate(cols)
    got = pred.last_scores.clone()
    assert got.numel() == n
    # every sample scored as in a full batch: the last 123 samples padded with the first ones' columns
    ns, nd, o1, o2, nbytes = record_layout(model.schema, B)
    ref = []
    for k in range(4):
        idx = (np.arange(B) + k * B) % n
        rec = np.zeros(nbytes, np.uint8)
        rec[:o1].view(np.int64).reshape(ns, B)[:] = cols.ids[:, idx]
        rec[o1:o2].view(np.float32).reshape(nd, B)[:] = cols.dense[:, idx]
        ref.append(pred.predict_from(torch.from_numpy(rec).cuda()).view(-1))
    ref = torch.cat(ref)[:n]
    assert torch.equal(got, ref)
    y, s = cols.labels, npy(got)
    assert abs(m["auc"] - roc_auc_score(y, s)) <= 1e-12
    ll = log_loss(y, np.clip(s, 1e-7, 1 - 1e-7))
    assert abs(m["logloss"] - ll) <= 1e-9 * ll
    assert torch.equal(pred.last_labels.cpu(), torch.from_numpy(cols.labels))


def _sk(y, s):
    from sklearn.metrics import log_loss, roc_auc_score
    return roc_auc_score(y, s), log_loss(y, np.clip(s, 1e-7, 1 - 1e-7))


@pytest.mark.parametrize("case", ["ties", "constant", "clip"])
def test_metrics_match_sklearn(case):
    from deepfm_amd.training import compute_auc, compute_logloss
    rng = np.random.default_rng(3)
    if case == "ties":              # 5 M scores on 200 levels
        n = 5_000_000
        s = (np.floor(rng.random(n) * 200) / 200).astype(np.float32)
        y = (rng.random(n) < 0.2 + 0.5 * s).astype(np.float32)
    elif case == "constant":        # a constant model: every pair tied
        n = 100_000
        s = np.full(n, 0.37, np.float32)
        y = (rng.random(n) < 0.3).astype(np.float32)
    else:                           # at and beyond both clip limits
        base = np.array([0.0, 1.0, 1e-7, 1 - 1e-7, 1e-9, 1 - 1e-9, 0.5, 1.2e-7, 0.99999994], np.float32)
        s = np.tile(base, 1000)
        y = (rng.random(s.size) < 0.5).astype(np.float32)
    auc, ll = _sk(y, s)
    d_y, d_s = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
    assert abs(compute_auc(d_y, d_s) - auc) <= 1e-12
    assert abs(compute_logloss(d_y, d_s) - ll) <= 1e-9 * ll
    assert abs(compute_auc(y, s) - auc) <= 1e-12                 # numpy inputs are copied to the device


def test_metrics_single_class_and_nan():
    from deepfm_amd.training import FusedPredictor, compute_auc
    s = torch.rand(1000, device="cuda")
    with pytest.raises(ValueError):
        compute_auc(torch.zeros(1000, device="cuda"), s)
    bad = s.clone()
    bad[17] = float("nan")
    with pytest.raises(ValueError):
        compute_auc((s > 0.5).float(), bad)
    model = _small_deepfm()
    cols = _columns(model, 5000, 2, rate=0.0)
    m = FusedPredictor(model, 1024).evaluate(cols)
    assert m["auc"] == 0.0 and m["logloss"] > 0


def test_evaluate_agrees_with_model_predict_after_one_epoch():
    import tools_shared_auc as T
    from sklearn.metrics import roc_auc_score

    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.data.packed import PackedColumns
    from deepfm_amd.models import create_model
    from deepfm_amd.training import FusedPredictor
    from deepfm_amd.training.fused_step import FusedDeepFMStep
    from deepfm_amd.training.rowsparse import RowSparseAdam
    ids, dense, labels = T.make_task()
    fields = criteo_fields(T.VOCAB, T.DIM)
    cfg = ExperimentConfig()
    torch.manual_seed(0)
    model = create_model("deepfm", schema_from_fields(fields), cfg).cuda().train()
    model.embedding.pack_tables_()
    model.embedding.set_grad_mode("rowsparse")
    opt = RowSparseAdam(model, lr=cfg.training.lr, l2=cfg.feature.embedding_l2_reg,
                        max_grad_norm=cfg.training.gradient_clip_norm)
    step = FusedDeepFMStep(model, opt, T.BATCH, use_graph=True)
    d_ids = torch.from_numpy(ids).cuda().t().contiguous()
    d_dense = torch.from_numpy(dense).cuda().t().contiguous()
    d_labels = torch.from_numpy(labels).cuda()
    step.load_batch(d_ids[:, :T.BATCH], d_dense[:, :T.BATCH], d_labels[:T.BATCH])
    step.capture()
    order = torch.from_numpy(T.epoch_order(0)).cuda()
    for k in range(T.N_TRAIN // T.BATCH):
        idx = order[k * T.BATCH:(k + 1) * T.BATCH]
        step.load_batch(d_ids[:, idx], d_dense[:, idx], d_labels[idx])
        step.run()
    test = slice(T.N_TRAIN, T.N_TRAIN + T.N_TEST)
    feats = {f"C{j + 1}": ids[test, j] for j in range(T.N_SPARSE)}
    feats.update({f"I{j + 1}": dense[test, j] for j in range(T.N_DENSE)})
    cols = PackedColumns(model.schema, feats, labels[test])
    m = FusedPredictor(model, T.BATCH).evaluate(cols)
    model.eval()
    scores = []
    with torch.no_grad():
        for s in range(T.N_TRAIN, T.N_TRAIN + T.N_TEST, T.BATCH):
            batch = {f"C{j + 1}": d_ids[j, s:s + T.BATCH].contiguous() for j in range(T.N_SPARSE)}
            batch.update({f"I{j + 1}": d_dense[j, s:s + T.BATCH].contiguous() for j in range(T.N_DENSE)})
            scores.append(model.predict(batch).view(-1).cpu().numpy())
    model.train()
    auc = roc_auc_score(labels[test], np.concatenate(scores))
    assert abs(m["auc"] - auc) < 1e-6, (m, auc)
    assert m["auc"] > 0.6
