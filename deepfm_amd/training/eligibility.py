"""Which models the fused paths take: every shape limit of the kernels, stated once.

A rule is a function of the model that returns None (passes) or the reason it is refused; nothing here touches the
device.  The public predicates are short compositions of the rules, and the ORDER of a composition decides which reason
a model with several faults is given:

    ineligible_reason                  FusedPredictor         (training/predict.py)
    mixed_ineligible_reason            MixedSchemaPredictor
    mixed_train_ineligible_reason      FusedMixedDeepFMStep   (training/mixed_step.py)
    mixed_step_ineligible_reason       the three mixed-schema steps

The step classes compose their own ``ineligible_reason`` from the same rules (training/fused_step.py,
training/mixed_step.py); ``fused_step_class`` / ``mixed_step_class`` there pick the class that has none.
"""

from __future__ import annotations

from typing import Optional

from deepfm_amd import _lib
from deepfm_amd.data.schema import FeatureType

_BWD_STAGE = 256      # csrc/embedding.hip: kBwdStage (samples in LDS at a time)
_FAMILY = "DeepFM, xDeepFM and AttentionDeepFM"


# ---------------------------------------------------------------------- the rules
def model_kind(model, exact: bool = True) -> Optional[str]:
    """"deepfm" / "xdeepfm" / "attention" for the three models with fused paths, else None (``exact`` False: their
    subclasses count).  The one place that enumerates the family."""
    from deepfm_amd.models.attention_deepfm import AttentionDeepFM
    from deepfm_amd.models.deepfm import DeepFM
    from deepfm_amd.models.xdeepfm import xDeepFM
    family = {DeepFM: "deepfm", xDeepFM: "xdeepfm", AttentionDeepFM: "attention"}
    if exact:
        return family.get(type(model))
    return next((kind for cls, kind in family.items() if isinstance(model, cls)), None)


def family_reason(model, what: str, exact: bool = True) -> Optional[str]:
    if model_kind(model, exact) is None:
        return f"no {what} for {type(model).__name__}: {_FAMILY} only"
    return None


def _hidden_widths(dnn):
    return [dnn.mlp[4 * i].out_features for i in range(dnn._n_layers)]


def training_tower_reason(model) -> Optional[str]:
    """The tower the fused training kernels take (csrc/tower.hip), whatever the embedding's gradient mode."""
    if not model.training:
        return "the model must be in training mode"
    dnn = getattr(model, "dnn", None)
    ok = dnn is not None and getattr(dnn, "_fusable", False)
    if ok:
        widths, bn = _hidden_widths(dnn), dnn.mlp[1]
        ok = not (any(w % 4 for w in widths) or widths[-1] % 32 or widths[-1] > 256 or bn.momentum is None
                  or not bn.affine or dnn.mlp[0].in_features % 4)
    if not ok:
        return ("the DNN tower is not fusable: Linear -> BatchNorm1d (affine, momentum) -> ReLU, hidden widths "
                "multiples of 4, the last one a multiple of 32 and <= 256, input width a multiple of 4")
    return None


def eval_tower_reason(model) -> Optional[str]:
    """The tower ``dfm_linear_bn_eval`` takes: running statistics instead of a momentum, no rule for the last width."""
    dnn = model.dnn
    if not dnn._fusable:
        return "the DNN tower must be Linear -> BatchNorm1d -> ReLU (use_batch_norm=True, activation='relu')"
    widths = _hidden_widths(dnn)
    if any(w % 4 for w in widths):
        return f"hidden widths {widths} must be multiples of 4"
    for i in range(dnn._n_layers):
        bn = dnn.mlp[4 * i + 1]
        if not bn.affine or not bn.track_running_stats or bn.running_mean is None:
            return "every BatchNorm1d needs affine parameters and running statistics"
    return None


def attention_reason(model) -> Optional[str]:
    """The shapes the fused attention kernels take (csrc/attention*.hip), forward and backward."""
    from deepfm_amd.models.layers.attention import gemm_shape_fault
    att = model.attention
    F = model.schema.num_fields
    fault = gemm_shape_fault(F, att.embed_dim, att.attention_dim, att.num_heads)
    if fault == "dims":
        return (f"attention embed_dim {att.embed_dim} / attention_dim {att.attention_dim}: the fused attention kernels "
                "take multiples of 4 with embed_dim <= 64")
    if fault == "core":
        return (f"attention over {F} fields with attention_dim {att.attention_dim} and {att.num_heads} heads is outside "
                "the attention core kernel's shapes (dfm_attention_core_supported)")
    if not all(b.gemm_path for b in att.layers):
        return "an attention block does not run on the GEMM path (gemm_path is off)"
    return None


def cin_reason(model) -> Optional[str]:
    """The CIN stacks ``dfm_cin_forward`` lays out (csrc/cin.hip:make_layout); the matrix-core and the general fp32
    kernels take every such stack between them."""
    cin = model.cin
    sizes = list(cin.layer_sizes)
    if not 1 <= len(sizes) <= 16:
        return f"the CIN has {len(sizes)} layers: the CIN kernels take 1 to 16"
    for i, c in enumerate(sizes):
        if c < 1 or (cin.split_half and i < len(sizes) - 1 and c < 2):
            return f"CIN layer {i} has {c} feature maps: too small" + (" to split in half" if c == 1 else "")
    return None


def _released_table(model) -> Optional[str]:
    """Name of a SPARSE field whose embedding table is released (field-sharded model), or None."""
    for name, spec in model.schema.fields.items():
        if spec.feature_type is FeatureType.SPARSE and \
                model.embedding.second_order_embeddings[name].weight.shape[0] != spec.vocabulary_size:
            return name
    return None


def released_table_reason(model) -> Optional[str]:
    name = _released_table(model)
    if name is not None:
        return (f"the embedding table of field {name!r} is released (field-sharded model, "
                "TableShard.released): call restore_tables() first")
    return None


def uniform_schema_reason(model) -> Optional[str]:
    """The schemas the staged gather (``dfm_embedding_forward_staged``) and the row-sparse backward take."""
    D = model.embedding.fm_embed_dim
    for name, spec in model.schema.fields.items():
        if spec.feature_type is FeatureType.SEQUENCE:
            return f"field {name!r} is a SEQUENCE field: the staged gather needs a uniform SPARSE / DENSE schema"
        if spec.embedding_dim != D or D % 4:
            return (f"field {name!r}: embedding_dim {spec.embedding_dim} with fm_embed_dim {D}: the staged gather "
                    "needs embedding_dim == fm_embed_dim, a multiple of 4")
    return None


def mixed_param_bytes(model) -> int:
    """LDS bytes the record gather stages per workgroup: projections (fm_dim x d) and DENSE Linear(1, d) weights,
    biases and Linear(1, 1) (csrc/embedding.hip:plan_record_layout)."""
    D = model.embedding.fm_embed_dim
    floats = 0
    for spec in model.schema.fields.values():
        d = spec.embedding_dim
        if d != D:
            floats += D * d
        if spec.feature_type is FeatureType.DENSE:
            floats += 2 * d + 4
    return 4 * floats


def record_gather_reason(model) -> Optional[str]:
    """Why the record gather (``dfm_embedding_forward_record``) cannot take ``model``'s schema (None: it can)."""
    D = model.embedding.fm_embed_dim
    if D not in (4, 8, 16, 32, 64):
        return f"fm_embed_dim {D}: the record gather takes 4, 8, 16, 32 or 64"
    for name, spec in model.schema.fields.items():
        if spec.embedding_dim % 4:
            return f"field {name!r}: embedding_dim {spec.embedding_dim} is not a multiple of 4 (16-byte row pieces)"
    nbytes = mixed_param_bytes(model)
    if nbytes > _lib.RECORD_PARAM_LDS_BYTES:
        return (f"projection and DENSE parameters take {nbytes} bytes of LDS, over the record gather's cap of "
                f"{_lib.RECORD_PARAM_LDS_BYTES}")
    return None


def backward_lds_bytes(model) -> int:
    """LDS bytes per workgroup of ``dfm_embedding_backward_record`` for this schema (csrc/embedding.hip:
    describe_bwd_record): the widest field's staged vectors + ids + projection, or a projection job's operands."""
    D = model.embedding.fm_embed_dim
    need = 0
    for spec in model.schema.fields.values():
        d = spec.embedding_dim
        L = spec.max_length if spec.feature_type is FeatureType.SEQUENCE else 1
        proj = D * d if d != D else 0
        need = max(need, 16 * (_BWD_STAGE * (d // 4 + 1) + (_BWD_STAGE * L + 3) // 4 + 1) + 4 * proj)
        if proj:
            need = max(need, 4 * _BWD_STAGE * (D + d))
    return need


def record_backward_reason(model, batch_size: Optional[int] = None) -> Optional[str]:
    """Why the record backward (``dfm_embedding_backward_record``) cannot take ``model``'s schema (None: it can).
    ``batch_size``: also check the row-owned scan's size cap for that batch."""
    specs = model.schema.fields
    for name, spec in specs.items():
        if spec.feature_type is FeatureType.SEQUENCE and spec.combiner == "max":
            return (f"field {name!r} pools with max: the embedding backward's arg-max recompute is not built "
                    "(mean and sum bags only; train it in dense autograd mode)")
    nbytes = backward_lds_bytes(model)
    if nbytes > _lib.BWD_RECORD_LDS_BYTES:
        return (f"the embedding backward stages {nbytes} bytes of LDS for the widest field, over its cap of "
                f"{_lib.BWD_RECORD_LDS_BYTES}")
    rows = sum(s.vocabulary_size for s in specs.values() if s.feature_type is not FeatureType.DENSE)
    if batch_size is not None and rows * batch_size > _lib.BWD_RECORD_MAX_ROW_SAMPLES:
        return (f"{rows} table rows x {batch_size} samples is over the row-owned scan's cap of "
                f"{_lib.BWD_RECORD_MAX_ROW_SAMPLES} (tables this large belong to a row-sparse design)")
    return None


# ---------------------------------------------------------------------- the predictors
def _predictor_reason(model, gather_reason) -> Optional[str]:
    if family_reason(model, "fused predictor") is not None:          # (the predictors' own wording of it)
        return f"no fused predictor for {type(model).__name__} ({_FAMILY} only)"
    reason = gather_reason(model) or eval_tower_reason(model)
    if reason is None and model_kind(model) == "attention" and attention_reason(model) is not None:
        reason = "attention blocks outside the fused attention kernels' shapes"
    return reason or released_table_reason(model)


def ineligible_reason(model) -> Optional[str]:
    """Why ``FusedPredictor`` cannot take ``model`` (None: it can).  Checked on the host only."""
    return _predictor_reason(model, uniform_schema_reason)


def mixed_ineligible_reason(model) -> Optional[str]:
    """Why ``MixedSchemaPredictor`` cannot take ``model`` (None: it can).  Checked on the host only."""
    return _predictor_reason(model, record_gather_reason)


# ---------------------------------------------------------------------- the mixed-schema training steps
def _mixed_step_reason(model, batch_size: Optional[int]) -> Optional[str]:
    """What every mixed-schema step checks, whatever the model: schema, record gather and backward, grad mode,
    training tower, released tables."""
    if uniform_schema_reason(model) is None:
        return "uniform schema: use the row-sparse step (set_grad_mode('rowsparse') and fused_step_class(model))"
    reason = record_gather_reason(model) or record_backward_reason(model, batch_size)
    if reason is None and model.embedding.grad_mode != "dense":
        reason = "the embedding must be in 'dense' grad mode (its tables are dense parameters of the flat buffer)"
    return reason or training_tower_reason(model) or released_table_reason(model)


def mixed_train_ineligible_reason(model, batch_size: Optional[int] = None) -> Optional[str]:
    """Why ``FusedMixedDeepFMStep`` cannot take ``model`` (None: it can).  Checked on the host only, before any device
    work.  ``batch_size``: also check the row-owned scan's size cap for that batch."""
    if model_kind(model) != "deepfm":
        return (f"no fused mixed-schema step for {type(model).__name__}: DeepFM only (xDeepFM and AttentionDeepFM "
                "are the next step, DESIGN.md section 9)")
    return _mixed_step_reason(model, batch_size)


def mixed_step_ineligible_reason(model, batch_size: Optional[int] = None) -> Optional[str]:
    """Why no fused mixed-schema step (``FusedMixedDeepFMStep``, ``FusedMixedXDeepFMStep``,
    ``FusedMixedAttentionDeepFMStep``) can take ``model`` (None: ``mixed_step_class(model)`` can).  Host only."""
    reason = family_reason(model, "fused mixed-schema step") or _mixed_step_reason(model, batch_size)
    if reason is None:
        own = {"xdeepfm": cin_reason, "attention": attention_reason}.get(model_kind(model))
        reason = own(model) if own is not None else None
    return reason
