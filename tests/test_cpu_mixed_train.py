"""Host-side tests of the fused mixed-schema training step: eligibility and every refusal reason (no device work),
the reference train-step fixtures (``tools/make_mixed_train_golden.py``), the public names and the library's symbols."""
import numpy as np
import pytest
import torch

from tests.helpers import cfg_of, fields_of, group, load, schema_from_fields
from tests.test_gpu_models_step import _config

CASES = ["train_steps_deepfm_movielens", "train_steps_deepfm_movielens_l2clip"]


def _model(fields, kind="deepfm", hidden=(64, 32), **cfg_kw):
    from deepfm_amd.models import create_model
    c = dict(kind=kind, fm_dim=16, hidden_units=list(hidden))
    if kind == "xdeepfm":
        c.update(cin_sizes=[8, 8], cin_split=True)
    if kind == "attention_deepfm":
        c.update(heads=2, A=16, layers=1, residual=True)
    cfg = _config(c)
    for k, v in cfg_kw.items():
        setattr(cfg.dnn, k, v)
    return create_model(kind, schema_from_fields(fields), cfg).train()


def _movielens():
    return fields_of(load("model_deepfm_movielens"))


def test_movielens_deepfm_is_eligible_and_picked():
    from deepfm_amd.training import FusedMixedDeepFMStep, mixed_train_ineligible_reason
    model = _model(_movielens())
    assert mixed_train_ineligible_reason(model) is None
    assert mixed_train_ineligible_reason(model, 4096) is None
    assert FusedMixedDeepFMStep.eligible(model)


def test_every_refusal_names_its_reason():
    from deepfm_amd import _lib
    from deepfm_amd.training import FusedMixedDeepFMStep, mixed_train_ineligible_reason as why
    fields = _movielens()
    # other models: DeepFM only
    assert "DeepFM only" in why(_model(fields, "xdeepfm"))
    assert "DeepFM only" in why(_model(fields, "attention_deepfm"))
    # uniform schema -> the row-sparse step
    uniform = [dict(name=f"C{i}", type="sparse", vocab=50, dim=16, max_len=1, combiner="mean") for i in range(3)] + \
              [dict(name="I0", type="dense", vocab=0, dim=16, max_len=1, combiner="mean")]
    assert "use the row-sparse step" in why(_model(uniform))
    # max combiner
    mx = [dict(f, combiner="max") if f["type"] == "sequence" else f for f in fields]
    assert "pools with max" in why(_model(mx))
    # tower not fusable: no BatchNorm; a last width that is no multiple of 32; eval mode
    assert "tower is not fusable" in why(_model(fields, use_batch_norm=False))
    assert "tower is not fusable" in why(_model(fields, hidden=(64, 24)))
    assert "training mode" in why(_model(fields).eval())
    # over the record gather's LDS cap for projections: many projected fields
    many = [dict(name=f"P{i}", type="sparse", vocab=10, dim=32, max_len=1, combiner="mean") for i in range(20)]
    assert "bytes of LDS" in why(_model(many))
    # over the backward's own LDS cap: one very long bag
    long_bag = fields + [dict(name="hist", type="sequence", vocab=50, dim=8, max_len=64, combiner="mean")]
    assert "embedding backward stages" in why(_model(long_bag))
    # over the size cap: (sum of vocabulary sizes) * batch
    rows = sum(f["vocab"] for f in fields)
    big = _lib.BWD_RECORD_MAX_ROW_SAMPLES // rows + 1
    assert "row-owned scan's cap" in why(_model(fields), big)
    assert why(_model(fields), big - 1) is None
    # widths that are no multiple of 4
    odd = [dict(f, dim=6) if f["name"] == "gender" else f for f in fields]
    assert "multiple of 4" in why(_model(odd))
    # rowsparse still refuses the schema (existing behaviour), and the step refuses before any device work
    with pytest.raises(NotImplementedError):
        _model(fields).embedding.set_grad_mode("rowsparse")
    with pytest.raises(ValueError, match="DeepFM only"):
        FusedMixedDeepFMStep(_model(fields, "xdeepfm"), None, 64)


def test_backward_lds_bytes_mirror():
    from deepfm_amd.training.mixed_step import backward_lds_bytes
    # MovieLens: a d = 16 table (5 pieces): 16 * (256 * 5 + 64 + 1); genres: 16 * (256 * 3 + 384 + 1) + its projection;
    # a projection job of a d = 8 field: 256 samples of g_field (16) and flat (8)
    assert backward_lds_bytes(_model(_movielens())) == max(16 * (256 * 5 + 65), 16 * (256 * 3 + 385) + 4 * 16 * 8,
                                                           4 * 256 * (16 + 8)) == 24576


@pytest.mark.parametrize("case", CASES)
def test_golden_files_carry_untouched_rows_that_the_reference_moves(case):
    g = load(case)
    fields, lr, steps = fields_of(g), float(g["lr"]), int(g["steps"])
    assert cfg_of(g)["kind"] == "deepfm" and steps == 3 and g["step0/labels"].shape == (64,)
    names = [f["name"] for f in fields if f["type"] != "dense"]
    assert sorted(group(g, "untouched/")) == sorted(names)
    assert any(f["type"] == "sequence" for f in fields) and any(f["dim"] != 16 for f in fields)
    for f in fields:
        if f["type"] == "dense":
            continue
        free = g["untouched/" + f["name"]]
        assert free.any() and not free[0]
        for t in range(steps):                      # really untouched: no sample of any step names them
            ids = g[f"step{t}/batch/{f['name']}"]
            assert not free[ids.reshape(-1)].any()
        for order in ("second", "first"):
            k = f"embedding.{order}_order_embeddings.{f['name']}.weight"
            moved = np.abs(g[f"step{steps - 1}/param/{k}"] - g["init/" + k])[free]
            assert moved.min() > 1e-3 * lr          # a lazy implementation is outside the GPU test's bar
            assert (g[f"step0/grad/{k}"][free] != 0).any()
    bags = g["step0/batch/genres"]
    assert (bags == 0).all(axis=1).any() and ((bags == 0).sum(axis=1) > 0).any()      # empty and short bags


def test_public_names_and_library_symbols():
    import deepfm_amd.training as T
    from deepfm_amd import _lib
    for name in ("DenseTableOptimizer", "DenseTableAdam", "DenseTableAdamW", "DenseTableSGD", "build_dense_optimizer",
                 "FusedMixedDeepFMStep", "mixed_train_ineligible_reason"):
        assert hasattr(T, name), name
    assert issubclass(T.DenseTableAdam, T.RowSparseOptimizer) and T.DenseTableAdam.row_tables is False
    assert T.RowSparseAdam.row_tables is True
    lib = _lib.load()
    for sym in ("dfm_embedding_backward_record", "dfm_embedding_backward_record_parts", "dfm_embedding_backward_record_workspace_bytes",
                "dfm_step_dense_prepare", "dfm_step_dense_apply", "dfm_step_dense_num_partials"):
        assert hasattr(lib, sym) and sym in _lib.SIGNATURES
    assert lib.dfm_embedding_backward_record_parts(1) == 1 and lib.dfm_embedding_backward_record_parts(4096) == 16
    assert lib.dfm_embedding_backward_record_parts(1 << 20) == 16
    assert lib.dfm_embedding_backward_record_workspace_bytes(4096, 160) == 4 * 16 * 160


def test_build_dense_optimizer_rejects_unknown_and_maps_kinds(monkeypatch):
    from deepfm_amd.config import ExperimentConfig
    from deepfm_amd.training import dense_table
    cfg = ExperimentConfig()
    cfg.training.optimizer = "lion"
    with pytest.raises(ValueError, match="Unknown optimizer"):
        dense_table.build_dense_optimizer(None, cfg)
    assert set(dense_table.DENSE_OPTIMIZERS) == {"adam", "adamw", "sgd"}
    assert [dense_table.DENSE_OPTIMIZERS[k].kind for k in ("adam", "adamw", "sgd")] == ["adam", "adamw", "sgd"]


def test_loader_writes_mixed_records_with_bags():
    """PackedBatchLoader takes SEQUENCE schemas: its records are RecordLayout.of(schema, B) records."""
    from deepfm_amd.data.packed import PackedBatchLoader, PackedColumns, RecordLayout
    from deepfm_amd.data.synthetic import random_fields_batch
    fields = _movielens()
    rng = np.random.default_rng(0)
    feats = random_fields_batch(fields, 200, rng, zero_frac=0.1)
    labels = (rng.random(200) < 0.3).astype(np.float32)
    schema = schema_from_fields(fields)
    for shuffle in (False, True):
        loader = PackedBatchLoader(PackedColumns(schema, feats, labels), 64, shuffle=shuffle, seed=3)
        lay = RecordLayout.of(schema, 64)
        assert loader.record_bytes == lay.record_bytes and len(loader) == 3
        out = np.zeros(loader.record_bytes, np.uint8)
        loader.write(out, 1)
        batch, lab = lay.unpack(out)
        idx = loader.order[64:128] if shuffle else np.arange(64, 128)
        assert np.array_equal(lab, labels[idx])
        for f in fields:
            assert np.array_equal(batch[f["name"]], feats[f["name"]][idx]), f["name"]
