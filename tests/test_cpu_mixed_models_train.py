"""Host-side tests of the fused mixed-schema steps for xDeepFM and AttentionDeepFM: the public names and the
library's new symbols, which class ``mixed_step_class`` picks, every refusal of the family with its reason, and the
reference train-step fixtures (``tools/make_mixed_train_golden.py``)."""
import numpy as np
import pytest

from tests.helpers import cfg_of, fields_of, group, load, schema_from_fields
from tests.test_gpu_models_step import _config

CASES = {"train_steps_xdeepfm_movielens": "xdeepfm", "train_steps_xdeepfm_movielens_l2clip": "xdeepfm",
         "train_steps_attention_deepfm_movielens": "attention_deepfm",
         "train_steps_attention_deepfm_movielens_l2clip": "attention_deepfm"}


def load_case(case):
    """A train-step fixture; the AttentionDeepFM ones keep their ``step<t>/grad/`` keys in ``<case>_grads.npz``."""
    g = load(case)
    if not group(g, "step0/grad/"):
        g.update(load(case + "_grads"))
    return g


def _model(fields, kind, hidden=(64, 32), cin_sizes=(8, 8), heads=2, A=16, **cfg_kw):
    from deepfm_amd.models import create_model
    c = dict(kind=kind, fm_dim=16, hidden_units=list(hidden))
    if kind == "xdeepfm":
        c.update(cin_sizes=list(cin_sizes), cin_split=True)
    if kind == "attention_deepfm":
        c.update(heads=heads, A=A, layers=1, residual=True)
    cfg = _config(c)
    for k, v in cfg_kw.items():
        setattr(cfg.dnn, k, v)
    return create_model(kind, schema_from_fields(fields), cfg).train()


def _movielens():
    return fields_of(load("model_deepfm_movielens"))


def test_public_names_and_library_symbols():
    import deepfm_amd.training as T
    from deepfm_amd import _lib
    for name in ("FusedMixedDeepFMStep", "FusedMixedXDeepFMStep", "FusedMixedAttentionDeepFMStep", "mixed_step_class",
                 "mixed_step_ineligible_reason", "mixed_train_ineligible_reason"):
        assert hasattr(T, name), name
    lib = _lib.load()
    for sym in ("dfm_embedding_forward_record", "dfm_embedding_backward_record"):
        assert hasattr(lib, sym) and sym in _lib.SIGNATURES, sym
    # one entry each: d_fm_sum, the FM trio and fold_fm are operands, the last argument is the launch destination
    assert lib.dfm_abi_version() == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES["dfm_embedding_forward_record"][1]) == 12
    assert len(_lib.SIGNATURES["dfm_embedding_backward_record"][1]) == 18


def test_mixed_step_class_picks_each_class_on_movielens():
    import deepfm_amd.training as T
    from deepfm_amd.training.fused_step import fused_step_class
    fields = _movielens()
    want = {"deepfm": T.FusedMixedDeepFMStep, "xdeepfm": T.FusedMixedXDeepFMStep,
            "attention_deepfm": T.FusedMixedAttentionDeepFMStep}
    for kind, cls in want.items():
        model = _model(fields, kind)
        assert T.mixed_step_ineligible_reason(model) is None, kind
        assert T.mixed_step_ineligible_reason(model, 4096) is None, kind
        assert T.mixed_step_class(model) is cls and fused_step_class(model) is cls and cls.eligible(model)
        for other in want.values():
            assert other.eligible(model) == (other is cls)
    # the issue's shapes: CIN [16, 16, 8] and [24, 12]; 4 heads over attention dim 64
    assert T.mixed_step_class(_model(fields, "xdeepfm", hidden=(32, 32), cin_sizes=(16, 16, 8))) is T.FusedMixedXDeepFMStep
    assert T.mixed_step_class(_model(fields, "xdeepfm", hidden=(32, 32), cin_sizes=(24, 12))) is T.FusedMixedXDeepFMStep
    assert T.mixed_step_class(_model(fields, "attention_deepfm", hidden=(32, 32), heads=4, A=64)) \
        is T.FusedMixedAttentionDeepFMStep


def test_old_function_keeps_its_meaning():
    from deepfm_amd.training import mixed_train_ineligible_reason as why
    fields = _movielens()
    assert "DeepFM only" in why(_model(fields, "xdeepfm"))
    assert "DeepFM only" in why(_model(fields, "attention_deepfm"))
    assert why(_model(fields, "deepfm")) is None


@pytest.mark.parametrize("kind", ["xdeepfm", "attention_deepfm"])
def test_every_family_refusal_names_its_reason(kind):
    import deepfm_amd.training as T
    from deepfm_amd import _lib
    why = T.mixed_step_ineligible_reason
    cls = T.FusedMixedXDeepFMStep if kind == "xdeepfm" else T.FusedMixedAttentionDeepFMStep
    fields = _movielens()
    uniform = [dict(name=f"C{i}", type="sparse", vocab=50, dim=16, max_len=1, combiner="mean") for i in range(3)] + \
              [dict(name="I0", type="dense", vocab=0, dim=16, max_len=1, combiner="mean")]
    assert "use the row-sparse step" in why(_model(uniform, kind))
    assert T.mixed_step_class(_model(uniform, kind)) is None
    mx = [dict(f, combiner="max") if f["type"] == "sequence" else f for f in fields]
    assert "pools with max" in why(_model(mx, kind))
    assert "tower is not fusable" in why(_model(fields, kind, use_batch_norm=False))
    assert "tower is not fusable" in why(_model(fields, kind, hidden=(64, 24)))
    assert "training mode" in why(_model(fields, kind).eval())
    many = [dict(name=f"P{i}", type="sparse", vocab=10, dim=32, max_len=1, combiner="mean") for i in range(20)]
    assert "bytes of LDS" in why(_model(many, kind))
    long_bag = fields + [dict(name="hist", type="sequence", vocab=50, dim=8, max_len=64, combiner="mean")]
    assert "embedding backward stages" in why(_model(long_bag, kind))
    rows = sum(f["vocab"] for f in fields)
    big = _lib.BWD_RECORD_MAX_ROW_SAMPLES // rows + 1
    assert "row-owned scan's cap" in why(_model(fields, kind), big)
    assert why(_model(fields, kind), big - 1) is None
    odd = [dict(f, dim=6) if f["name"] == "gender" else f for f in fields]
    assert "multiple of 4" in why(_model(odd, kind))
    # the step refuses before any device work, and the wrong class of the family says which model it is for
    with pytest.raises(ValueError, match="pools with max"):
        cls(_model(mx, kind), None, 64)
    with pytest.raises(ValueError, match="does not take DeepFM"):
        cls(_model(fields, "deepfm"), None, 64)


def test_model_specific_refusals():
    import torch

    import deepfm_amd.training as T
    why = T.mixed_step_ineligible_reason
    fields = _movielens()
    # CIN: a layer of one feature map cannot be split in half (csrc/cin.hip: make_layout)
    assert "too small to split" in why(_model(fields, "xdeepfm", cin_sizes=(1, 8)))
    assert why(_model(fields, "xdeepfm", cin_sizes=(2, 8))) is None
    # attention: 3 heads do not divide attention dim 16 -> the module itself refuses; a head width the core kernel does
    # not take is refused by name; a block off the GEMM path too
    model = _model(fields, "attention_deepfm", heads=2, A=16)
    from deepfm_amd import _lib
    if not _lib.load().dfm_attention_core_supported(16, 520, 2):
        wide = _model(fields, "attention_deepfm", heads=2, A=520)
        assert "dfm_attention_core_supported" in why(wide)
    model.attention.layers[0].gemm_path = False
    assert "gemm_path" in why(model)
    # a model outside the family

    class Other(torch.nn.Module):
        pass
    assert "DeepFM, xDeepFM and AttentionDeepFM only" in why(Other())
    assert T.mixed_step_class(Other()) is None


@pytest.mark.parametrize("case", sorted(CASES))
def test_golden_files_carry_untouched_rows_that_the_reference_moves(case):
    g = load_case(case)
    fields, lr, steps = fields_of(g), float(g["lr"]), int(g["steps"])
    c = cfg_of(g)
    assert c["kind"] == CASES[case] and steps == 3 and g["step0/labels"].shape == (64,)
    assert c["hidden_units"] == [32, 32] and c["fm_dim"] == 16 and int(g["seed"]) >= 813
    if c["kind"] == "xdeepfm":
        assert c["cin_sizes"] == ([24, 12] if case.endswith("l2clip") else [16, 16, 8]) and c["cin_split"] is True
    else:
        assert (c["heads"], c["A"], c["residual"]) == (4, 64, True) and c["layers"] == (2 if case.endswith("l2clip") else 1)
    assert (float(g["lr"]), float(g["l2"]), float(g["clip"])) == \
        ((1e-2, 1e-2, 0.25) if case.endswith("l2clip") else (1e-3, 1e-5, 1.0))
    # the DeepFM pair's schema and key layout
    d = load("train_steps_deepfm_movielens")
    assert fields == fields_of(d)
    def meta(keys):           # everything that is not a parameter-shaped array
        return sorted(k for k in keys if k != "seed" and not any(p in k for p in ("/param/", "/grad/", "init/", "adam_")))
    assert meta(g) == meta(d)
    trained = sorted(k for k in group(g, "step0/param/") if "running_" not in k and "num_batches" not in k)
    assert sorted(group(g, "step0/grad/")) == trained == sorted(group(g, "adam_m/")) == sorted(group(g, "adam_v/"))
    assert sorted(group(g, "init/")) == sorted(group(g, "step2/param/"))
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
    assert any((g[f"step0/batch/{n}"] == 0).any() for n in names if n != "genres")    # id 0
