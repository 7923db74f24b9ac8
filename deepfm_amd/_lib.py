"""ctypes binding of the C ABI declared in ``include/deepfm_hip.h``.

The library is built in-tree by ``deepfm_amd/csrc/Makefile`` (``__graft_entry__.build()``)
into ``deepfm_amd/lib/libdeepfm_hip.so``.  There is no CPU fallback: if the library is
missing, or a tensor is not on a HIP device, the callers raise.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# DFM_LIB_PATH: load another build of the same library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("DFM_LIB_PATH") or os.path.join(_HERE, "lib", "libdeepfm_hip.so")

# == DFM_ABI_VERSION of include/deepfm_hip.h at the time SIGNATURES / the ctypes structs below were written:
# bumped together with the header whenever a struct layout or an argument list changes, so that a stale .so
# (the library is untracked and DFM_LIB_PATH can point anywhere) is refused instead of fed shifted arguments
ABI_VERSION = 11

MAX_FIELDS = 64
MAX_RANKS = 64
ROWPLAN_CHUNK = 4096
RECORD_PARAM_LDS_BYTES = 32768     # DFM_RECORD_PARAM_LDS_BYTES: the record gather's LDS cap for its parameters
BWD_RECORD_MAX_ROW_SAMPLES = 1 << 27   # DFM_BWD_RECORD_MAX_ROW_SAMPLES: (sum of vocabulary sizes) * batch of the record backward
BWD_RECORD_LDS_BYTES = 65536           # its LDS cap per workgroup (csrc/embedding.hip:kBwdMaxLds)
SPARSE, DENSE, SEQUENCE = 0, 1, 2
COMBINER = {"mean": 0, "sum": 1, "max": 2}

c_float_p = C.c_void_p  # device pointers travel as integers
c_int_p = C.c_void_p


class Field(C.Structure):
    """struct dfm_field"""
    _fields_ = [("kind", C.c_int32), ("dim", C.c_int32), ("vocab", C.c_int32), ("max_len", C.c_int32),
                ("combiner", C.c_int32), ("flat_offset", C.c_int32), ("stride2", C.c_int32),
                ("stride1", C.c_int32),
                ("w2", C.c_void_p), ("b2", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p),
                ("proj", C.c_void_p)]


class FieldGrad(C.Structure):
    """struct dfm_field_grad"""
    _fields_ = [("w2", C.c_void_p), ("b2", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p),
                ("proj", C.c_void_p)]


class Table(C.Structure):
    """struct dfm_table"""
    _fields_ = [("w2", C.c_void_p), ("m2", C.c_void_p), ("v2", C.c_void_p),
                ("w1", C.c_void_p), ("m1", C.c_void_p), ("v1", C.c_void_p),
                ("stride2", C.c_int32), ("stride1", C.c_int32)]


class Optim(C.Structure):
    """struct dfm_optim"""
    _fields_ = [("kind", C.c_int32), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("momentum", C.c_float), ("d_lr", C.c_void_p)]


OPT_ADAM, OPT_ADAMW, OPT_SGD = 0, 1, 2


class QuantField(C.Structure):
    """struct dfm_quant_field"""
    _fields_ = [("kind", C.c_int32), ("vocab", C.c_int32), ("rows", C.c_void_p),
                ("w2", C.c_void_p), ("b2", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p)]


QUANT_INT8_ROWWISE = 1                                 # enum dfm_quant_format
QUANT_UINT4_ROWWISE = 4
QUANT_DIMS = (16, 32, 64)                              # widths of the quantised tables and their gather
QUANT_MAX_SPARSE, QUANT_MAX_DENSE = 48, 32             # its slot caps (csrc/quant.hip)


class Launch(C.Structure):
    """struct dfm_launch: where a re-pointable launch goes (a stream, or a captured node of an instantiated graph).
    Passed as is for a ``const dfm_launch*`` argument (``LaunchArg``)."""
    _fields_ = [("stream", C.c_void_p), ("graph_exec", C.c_void_p), ("node", C.c_void_p)]


class LaunchArg:
    """argtype of a ``const dfm_launch*``: a ``Launch``, None (the null stream), or a bare stream handle, which means
    "enqueue there" as it does for every other entry."""

    @classmethod
    def from_param(cls, v):
        if v is None:
            return None
        return C.byref(v if isinstance(v, Launch) else Launch(v, None, None))


class BnBwd(C.Structure):
    """struct dfm_bn_bwd"""
    _fields_ = [("z", C.c_void_p), ("mean_rstd", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("dy", C.c_void_p), ("g_gamma", C.c_void_p), ("g_beta", C.c_void_p),
                ("seed", C.c_void_p), ("workspace", C.c_void_p), ("p_drop", C.c_float), ("salt", C.c_int32)]


class FmBwd(C.Structure):
    """struct dfm_fm_bwd"""
    _fields_ = [("g_fm", C.c_void_p), ("fm_sum", C.c_void_p), ("e", C.c_void_p), ("addend", C.c_void_p),
                ("dim", C.c_int32)]


class SlabRef(C.Structure):
    """struct dfm_slab_ref"""
    _fields_ = [("workspace", C.c_void_p), ("g_w", C.c_void_p), ("batch", C.c_int64), ("out_features", C.c_int32),
                ("in_features", C.c_int32), ("splits", C.c_int32), ("reserved", C.c_int32)]


class SplitJob(C.Structure):
    """struct dfm_split_job"""
    _fields_ = [("src", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int64), ("planes_f", C.c_void_p),
                ("planes_s", C.c_void_p)]


class PartialJob(C.Structure):
    """struct dfm_partial_job"""
    _fields_ = [("kind", C.c_int32), ("blocks", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32),
                ("accumulate", C.c_int32), ("reserved", C.c_int32), ("partial", C.c_void_p), ("out_w", C.c_void_p),
                ("out_b", C.c_void_p), ("ldw", C.c_int64)]


class HeadTail(C.Structure):
    """struct dfm_head_tail"""
    _fields_ = [("g_w", C.c_void_p), ("g_b", C.c_void_p), ("loss", C.c_void_p), ("g_b2", C.c_void_p)]


class AssembleColumn(C.Structure):
    """struct dfm_assemble_column"""
    _fields_ = [("kind", C.c_int32), ("role", C.c_int32), ("length", C.c_int32), ("num_edges", C.c_int32),
                ("record_offset", C.c_int64), ("pos", C.c_void_p), ("item", C.c_void_p), ("ctx", C.c_void_p),
                ("edges", C.c_void_p), ("bucket_ids", C.c_void_p)]


class CandidateList(C.Structure):
    """struct dfm_candidate_list: a ragged candidate list.  Passed as is for a ``const dfm_candidate_list*`` argument;
    None is the rectangular list."""
    _fields_ = [("d_counts", C.c_void_p), ("d_offsets", C.c_void_p), ("total", C.c_int64)]


ROLE_COPY, ROLE_ITEM, ROLE_BUCKET_DIFF = 0, 1, 2      # enum dfm_assemble_role
MAX_NEGATIVES = 16                                     # dfm_sample_negatives: 1 <= k <= 16
MAX_BUCKET_EDGES = 64
MAX_CANDIDATES = 1 << 20                               # DFM_MAX_CANDIDATES: an assemble plan's k, a selection's rows
WEIGHTED_MAX_ITEMS = 1 << 17                           # dfm_sample_weighted: 32 KiB of uint64 word prefixes in LDS
TOPK_MAX_K = 128                                       # dfm_catalogue_topk: 1 <= k <= 128
TOPK_LDS_ITEMS = 6144                                  # ... a score row up to this long is read from memory once
GEMM_TILED_SLOW, GEMM_TILED_FAST, GEMM_ROWS, GEMM_WGRAD = 0, 1, 2, 3     # DFM_GEMM_ROUTE_*: dfm_gemm_route
MAX_PARTIAL_JOBS = 8                                   # dfm_partials_finish: 1 <= count <= 8
CAL_PLATT, CAL_ISOTONIC = 0, 1                         # enum dfm_cal_kind
CAL_RUNNING, CAL_CONVERGED, CAL_SINGLE_CLASS, CAL_BAD_INPUT = 0, 1, 2, 3     # enum dfm_cal_status
CAL_FLAG_SLOPE_UNIDENTIFIED = 1
PLATT_STATE_DOUBLES = 32                               # DFM_PLATT_STATE_DOUBLES
ISOTONIC_MAX_BINS = 1024                               # DFM_ISOTONIC_MAX_BINS
ISOTONIC_KNOT_BYTES = 64 + 24 * ISOTONIC_MAX_BINS      # DFM_ISOTONIC_KNOT_BYTES


class _EncodeTable(C.Structure):
    _fields_ = [("slots", C.c_void_p), ("lengths", C.c_void_p)]


class _EncodeScale(C.Structure):
    _fields_ = [("lo", C.c_double), ("hi", C.c_double)]


class _EncodeUnion(C.Union):
    _fields_ = [("table", _EncodeTable), ("scale", _EncodeScale), ("num_buckets", C.c_uint64)]


class EncodeJob(C.Structure):
    """struct dfm_encode_job"""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("u", _EncodeUnion), ("kind", C.c_int32),
                ("in_stride", C.c_int32), ("out_stride", C.c_int32), ("width", C.c_int32), ("raw_width", C.c_int32),
                ("log2_capacity", C.c_int32)]


ENC_LOOKUP, ENC_BAG, ENC_HASHED, ENC_SCALE_F32, ENC_SCALE_F64, ENC_COPY_F32, ENC_ZERO_F32 = range(7)   # enum dfm_encode_kind
VOCAB_SLOT_BYTES = 16                                  # sizeof(dfm_vocab_slot)
VOCAB_MAX_KEYS = 1 << 30                               # dfm_vocab_capacity: n_keys in [0, 2^30]
COUNTS_LDS_ENTITIES = 8192                             # DFM_COUNTS_LDS_ENTITIES: dfm_entity_counts' LDS route up to here
BOOTSTRAP_CHUNK = 2048                                 # DFM_BOOTSTRAP_CHUNK: sorted samples per workgroup
BOOTSTRAP_REPLICATE_BLOCK = 16                         # DFM_BOOTSTRAP_REPLICATE_BLOCK: replicates per workgroup
BOOTSTRAP_MAX_N = 1 << 26                              # 2^DFM_BOOTSTRAP_MAX_LOG2_N samples
BOOTSTRAP_MAX_REPLICATES = 65536                       # DFM_BOOTSTRAP_MAX_REPLICATES
BOOTSTRAP_UNITS_CHUNK = 1024                           # DFM_BOOTSTRAP_UNITS_CHUNK: units per workgroup
BOOTSTRAP_UNITS_MAX_COLS = 24                          # DFM_BOOTSTRAP_UNITS_MAX_COLS
BOOTSTRAP_UNITS_MAX_UNITS = 1 << 30                    # dfm_bootstrap_units: 1 <= num_units <= 2^30
RANK_NOT_COUNTED, RANK_MISS = -1, -2                   # DFM_RANK_NOT_COUNTED, DFM_RANK_MISS


class RecordField(C.Structure):
    """struct dfm_record_field"""
    _fields_ = [("kind", C.c_int32), ("max_length", C.c_int32), ("offset", C.c_int64)]


HISTORY_MAX_LENGTH = 4096                              # DFM_HISTORY_MAX_LENGTH: dfm_record_assemble's bag cap
HISTORY_POSITION, HISTORY_EXCLUDE, HISTORY_LATEST = range(3)        # enum dfm_history_mode


class HistorySource(C.Structure):
    """struct dfm_history_source: the index of ``dfm_history_index_build`` as ``dfm_assemble_plan_bind_history`` takes
    it.  Passed as is for a ``const dfm_history_source*`` argument."""
    _fields_ = [("d_user_rows", C.c_void_p), ("d_item_rows", C.c_void_p), ("d_timestamps", C.c_void_p),
                ("d_item_ids", C.c_void_p), ("d_start", C.c_void_p), ("d_pos_of", C.c_void_p), ("d_rank", C.c_void_p),
                ("d_events", C.c_void_p), ("d_sorted_ts", C.c_void_p), ("d_event_count", C.c_void_p),
                ("n", C.c_int64), ("n_users", C.c_int64), ("n_items", C.c_int64), ("mode", C.c_int32)]


PERMUTATION_MAX_N = (1 << 31) - 1                      # dfm_permutation_keys / dfm_records_permute: 1 <= n < 2^31
PERMUTATION_MAX_REPEATS = 1 << 24                      # ... 0 <= repeat < 2^24

# name -> (restype, argtypes); must list every symbol of include/deepfm_hip.h
_P, _I, _L, _F, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t

_AT = LaunchArg
SIGNATURES = {
    "dfm_abi_version": (_I, []),
    "dfm_last_error": (C.c_char_p, []),
    "dfm_device_info": (_I, [_P, _P, C.c_char_p, _I]),
    "dfm_debug_empty_launch": (_I, [_P]),
    "dfm_embedding_plan_create": (_I, [C.POINTER(Field), _I, _I, C.POINTER(_P)]),
    "dfm_embedding_plan_destroy": (_I, [_P]),
    "dfm_embedding_plan_is_uniform": (_I, [_P]),
    "dfm_embedding_workspace_bytes": (_SZ, [_P, _L]),
    "dfm_embedding_forward": (_I, [_P, C.POINTER(_P), _L, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfm_embedding_forward_staged": (_I, [_P, C.POINTER(_P), C.POINTER(_P), _P, _P, _L, _P, _P, _P, _P, _P, _AT]),
    "dfm_embedding_forward_record": (_I, [_P, _P, _L, _P, _P, _P, _L, _P, _P, _P, _P, _AT]),
    "dfm_embedding_backward_record_parts": (_I, [_L]),
    "dfm_embedding_backward_record_workspace_bytes": (_SZ, [_L, _L]),
    "dfm_embedding_backward_record": (_I, [_P, _P, _L, _P, _P, _P, _L, _P, _L, _P, _P, _P, _I, C.POINTER(FieldGrad), _P,
                                           _L, _P, _AT]),
    "dfm_graph_last_node": (_I, [_P, C.POINTER(_P)]),
    "dfm_gather_timing_begin": (_I, [_I]),
    "dfm_gather_timing_end": (_I, [C.POINTER(C.c_float), _I, C.POINTER(_I)]),
    "dfm_gather_set_shape": (_I, [_I]),
    "dfm_cin_set_mode": (_I, [_I]),
    "dfm_cin_get_mode": (_I, []),
    "dfm_embedding_backward_dense": (_I, [_P, C.POINTER(_P), _L, _P, _P, _P, C.POINTER(FieldGrad), _P, _P]),
    "dfm_embedding_backward_dense_fields": (_I, [_P, C.POINTER(_P), _L, _P, _P, _P, C.POINTER(FieldGrad), _P]),
    "dfm_rowplan_build": (_I, [C.POINTER(_P), C.POINTER(C.c_int32), _I, _L, _P, _P, _P, _P, _P, _P, _I, _AT]),
    "dfm_rowgrad_build": (_I, [C.POINTER(C.c_int32), _I, _I, _I, _L, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dfm_rowadam_num_partials": (_L, [_I, _I, _I]),
    "dfm_grad_norm_finalize": (_I, [_P, _L, _F, _P, _P, _P, _P, _P]),
    "dfm_cin_output_dim": (_I, [C.POINTER(C.c_int32), _I, _I]),
    "dfm_cin_saved_bytes": (_SZ, [C.POINTER(C.c_int32), _I, _I, _L, _I, _I]),
    "dfm_cin_backward_workspace_bytes": (_SZ, [C.POINTER(C.c_int32), _I, _I, _L, _I, _I]),
    "dfm_cin_forward_workspace_bytes": (_SZ, [C.POINTER(C.c_int32), _I, _I, _I, _I]),
    "dfm_cin_route": (_I, [C.POINTER(C.c_int32), _I, _I, _L, _I, _I]),
    "dfm_cin_forward": (_I, [_P, _L, _I, _I, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32), _I, _I, _P, _P, _P, _P]),
    "dfm_cin_backward": (_I, [_P, _L, _I, _I, C.POINTER(_P), C.POINTER(C.c_int32), _I, _I, _P, _P, _P,
                              C.POINTER(_P), C.POINTER(_P), _P, _P]),
    "dfm_attention_forward": (_I, [_P, _L, _I, _I, _I, _I, _I, C.POINTER(_P), _P, _P]),
    "dfm_attention_backward_workspace_bytes": (_SZ, [_L, _I, _I]),
    "dfm_attention_backward": (_I, [_P, _P, _L, _I, _I, _I, _I, _I, C.POINTER(_P), _P, C.POINTER(_P), _P, _P]),
    "dfm_bn_workspace_bytes": (_SZ, [_L, _I]),
    "dfm_bn_relu_dropout_forward": (_I, [_P, _L, _I, _P, _P, _P, _P, _P, _F, _F, _F, _P, _I, _P, _P, _P, _P]),
    "dfm_bn_relu_dropout_backward": (_I, [_P, _P, _P, _P, _P, _L, _I, _F, _P, _I, _P, _P, _P, _P, _P]),
    "dfm_bce_workspace_bytes": (_SZ, [_L]),
    "dfm_bce_with_logits": (_I, [_P, _P, _L, _P, _P, _P, _P]),
    "dfm_gemm_workspace_bytes": (_SZ, [_I, _I, _I]),
    "dfm_gemm_f32": (_I, [_P, _L, _I, _P, _L, _I, _P, _L, _I, _I, _I, _P, _I, _P, _P]),
    "dfm_gemm_route": (_I, [_P, _L, _I, _P, _L, _I, _I, _I, _I, _I, _I]),
    "dfm_gemm_splits": (_I, [_I, _I, _I, _I]),
    "dfm_weight_grad_workspace_bytes": (_SZ, [_L, _I, _I]),
    "dfm_weight_grad_f32": (_I, [_P, _L, _P, _L, _L, _I, _I, _P, _L, _P, _I, _P, _P]),
    "dfm_attention_core_supported": (_I, [_I, _I, _I]),
    "dfm_attention_core_forward": (_I, [_P, _L, _I, _I, _I, _P, _P]),
    "dfm_attention_core_backward": (_I, [_P, _P, _L, _I, _I, _I, _P, _P]),
    "dfm_attention_qkv_core_supported": (_I, [_I, _I, _I, _I]),
    "dfm_attention_qkv_core_forward": (_I, [_P, _P, _P, _L, _I, _I, _I, _I, _P, _P]),
    "dfm_attention_qkv_core_backward": (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _I, _P, _P]),
    "dfm_attention_block_supported": (_I, [_I, _I, _I, _I]),
    "dfm_attention_block_forward": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _L, _I, _I, _I, _I, _P, _P, _P, _P, _L, _P, _L,
                                         _P]),
    "dfm_attention_block_backward": (_I, [_P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _I, _P, _P, _P, _L, _P, _P, _P]),
    "dfm_layernorm_workspace_bytes": (_SZ, [_L, _I]),
    "dfm_layernorm_forward": (_I, [_P, _P, _L, _I, _P, _P, _F, _P, _P, _L, _L, _P]),
    "dfm_layernorm_backward": (_I, [_P, _P, _P, _P, _L, _I, _P, _P, _P, _P, _P, _L, _L, _P]),
    "dfm_linear_bn_workspace_bytes": (_SZ, [_L, _I]),
    "dfm_linear_bn_forward": (_I, [_P, _L, _P, _P, _L, _I, _I, _P, _P, _P]),
    "dfm_bn_relu_dropout_apply": (_I, [_P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _F, _P, _I, _P, _P]),
    "dfm_bn_bwd_workspace_bytes": (_SZ, [_L, _I]),
    "dfm_bn_backward_apply": (_I, [C.POINTER(BnBwd), _L, _I, C.POINTER(HeadTail), _P, _P]),
    "dfm_linear1_supported": (_I, [_I]),
    "dfm_linear1_forward": (_I, [_P, _L, _I, _P, _P, _P, _P]),
    "dfm_linear1_backward_splits": (_I, [_L]),
    "dfm_linear1_backward": (_I, [_P, _P, _L, _I, _P, _P, _P, _P]),
    "dfm_head_bce": (_I, [_P, _L, _I, _P, _P, _P, _P, _P, _P, _P, C.POINTER(BnBwd), _P]),
    "dfm_head_bn_bce": (_I, [_P, _P, _P, _P, _P, _F, _F, _L, _I, _P, _P, _P, _P, _P, _P, _P, C.POINTER(BnBwd), _P]),
    "dfm_linear_backward_workspace_bytes": (_SZ, [_L, _I, _I]),
    "dfm_linear_backward": (_I, [_P, _L, _I, _P, _I, _P, _P, C.POINTER(BnBwd), C.POINTER(FmBwd), _I, _P, _P]),
    "dfm_linear_backward_finish": (_I, [C.POINTER(SlabRef), _I, _P]),
    "dfm_linear_backward_splits": (_I, [_L, _I, _I]),
    "dfm_step_embedding_backward": (_I, [_P, _I, C.POINTER(_P), C.POINTER(FieldGrad), C.POINTER(C.c_int32), _I, _I, _I,
                                         _L, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P]),
    "dfm_step_prepare_num_partials": (_L, [_I, _I, _I, _L]),
    "dfm_step_match_bytes": (_SZ, [_I, _I]),
    "dfm_step_prepare": (_I, [C.POINTER(Table), _I, _I, _I, _P, _P, _P, _P, _P, _F, _F, _P, _P, _L, _L,
                              C.POINTER(SlabRef), _I, _P, _I, _L, _P, _L, _P, _P]),
    "dfm_step_apply": (_I, [C.POINTER(Table), _I, _I, _I, _P, _P, _P, _P, _P, _P, C.POINTER(Optim), _P, _P, _P, _P,
                            _P, _L, _I, _P]),
    "dfm_step_apply_plan": (_I, [C.POINTER(Table), _I, _I, _I, _P, _P, _P, _P, _P, _P, C.POINTER(Optim), _P, _P, _P,
                                 _P, _P, _L, _I, _P, _L, _P, _I, _L, _P, _P, _P, _P, _P, _AT]),
    "dfm_step_dense_num_partials": (_L, [_L]),
    "dfm_step_dense_prepare": (_I, [_F, _P, _P, _L, _L, C.POINTER(SlabRef), _I, _P, _P]),
    "dfm_step_dense_apply": (_I, [_P, C.POINTER(Optim), _P, _P, _P, _P, _P, _L, _I, _P]),
    "dfm_loss_accumulate": (_I, [_P, _F, _P, _L, _P, _P]),
    "dfm_tables_sqnorm_num_partials": (_L, [_L]),
    "dfm_tables_sqnorm": (_I, [C.POINTER(Table), _I, _I, C.POINTER(C.c_int32), _P, _P, _P]),
    "dfm_rows_sqnorm": (_I, [C.POINTER(Table), _I, _I, _I, _P, _P, _P, _P, _L, _P]),
    "dfm_loss_accumulate_tables": (_I, [_P, _F, _P, _L, _P, _P, _P, _L, _P, _P]),
    "dfm_weight_grad_partial_blocks": (_I, [_L]),
    "dfm_weight_grad_partials_f32": (_I, [_P, _L, _P, _L, _L, _I, _I, _P, _P]),
    "dfm_weight_grad_partials_pair_f32": (_I, [_P, _L, _P, _L, _I, _I, _P, _P, _L, _P, _L, _I, _I, _P, _L, _P]),
    "dfm_layernorm_partial_blocks": (_I, [_L]),
    "dfm_partials_finish": (_I, [C.POINTER(PartialJob), _I, _P]),
    "dfm_tower_set_mode": (_I, [_I]),
    "dfm_tower_get_mode": (_I, []),
    "dfm_planes_bytes": (_SZ, [_L, _L]),
    "dfm_tower_x6_supported": (_I, [_L, _I, _I]),
    "dfm_split_planes": (_I, [C.POINTER(SplitJob), _I, _P]),
    "dfm_linear_bn_forward_x6": (_I, [_P, _L, _P, _P, _P, _L, _I, _I, _P, _P, _P]),
    "dfm_bn_relu_dropout_apply_planes": (_I, [_P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _F, _P, _I, _P, _P, _P,
                                              _P]),
    "dfm_bn_backward_apply_planes": (_I, [C.POINTER(BnBwd), _L, _I, C.POINTER(HeadTail), _P, _P, _P, _P]),
    "dfm_linear_backward_x6_splits": (_I, [_L, _I, _I]),
    "dfm_linear_backward_x6_workspace_bytes": (_SZ, [_L, _I, _I]),
    "dfm_linear_backward_x6": (_I, [_P, _P, _L, _I, _P, _P, _I, _P, _P, C.POINTER(BnBwd), C.POINTER(FmBwd), _P, _P]),
    "dfm_fm_forward": (_I, [_P, _L, _I, _I, _P, _P]),
    "dfm_fm_backward": (_I, [_P, _P, _L, _I, _I, _P, _P]),
    "dfm_copy_2d": (_I, [_P, _L, _P, _L, _L, _I, _P]),
    "dfm_stage_record": (_I, [_P, _P, _L, _AT]),
    "dfm_shard_gather": (_I, [C.POINTER(Table), C.POINTER(C.c_int32), _I, _I, _I, _L, _P, _P, _P, _P, _P]),
    "dfm_shard_pack_segment": (_L, [_L, _I, _I, _L]),
    "dfm_shard_pack": (_I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, C.POINTER(C.c_int32), _I, _I, _I, _L,
                            _P, _P, _P, _L, C.POINTER(SlabRef), _I, _P, _P]),
    "dfm_shard_rowgrad": (_I, [_I, _I, _I, _L, _P, _L, _P, _P, _P, _P, _P, _P]),
    "dfm_sum_floats": (_I, [_P, _L, _P, _P]),
    "dfm_embedding_grad_combine": (_I, [_P, _L, _P, _P, _P, _P, _L, _I, _I, _P, _P]),
    "dfm_linear_bn_eval": (_I, [_P, _L, _P, _P, _L, _I, _I, _P, _P, _P, _P, _F, _P, _P]),
    "dfm_predict_head": (_I, [_P, _L, _I, _P, _P, _P, _P, _L, _P, _P, _AT]),
    "dfm_metrics_workspace_bytes": (_SZ, [_L]),
    "dfm_metrics_prepare": (_I, [_P, _P, _L, _P, _P, _P]),
    "dfm_metrics_finish": (_I, [_P, _P, _L, _P, _P, _P, _P]),
    "dfm_ranking_workspace_bytes": (_SZ, [_L, _L]),
    "dfm_ranking_metrics": (_I, [_P, _P, _P, _L, _L, _P, _I, _I, _P, _P, _P]),
    "dfm_ranking_user_ranks": (_I, [_P, _P, _P, _L, _L, _I, _P, _P, _P, _P]),
    "dfm_grouped_auc_workspace_bytes": (_SZ, [_L, _L]),
    "dfm_grouped_auc_prepare": (_I, [_P, _P, _P, _L, _L, _P, _P, _P]),
    "dfm_grouped_auc_finish": (_I, [_P, _L, _L, _P, _P, _P, _P]),
    "dfm_grouped_auc_unit_columns": (_I, [_P, _L, _L, _P, _P, _P]),
    "dfm_calibration_workspace_bytes": (_SZ, [_I, _L]),
    "dfm_calibration_route": (_I, [_I, _L]),
    "dfm_calibration": (_I, [_P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _P]),
    "dfm_bootstrap_workspace_bytes": (_SZ, [_L, _I]),
    "dfm_bootstrap_prepare": (_I, [_P, _P, _P, _L, _P, _P, _P, _P]),
    "dfm_bootstrap_replicates": (_I, [_P, _P, _P, _L, _I, C.c_uint64, _P, _P, _P, _P, _P]),
    "dfm_bootstrap_units_workspace_bytes": (_SZ, [_L, _I, _I]),
    "dfm_bootstrap_units": (_I, [_P, _L, _I, _I, C.c_uint64, _P, _P, _P]),
    "dfm_bootstrap_rank_columns": (_I, [_P, _L, _P, _I, _P, _L, _P, _P]),
    "dfm_sample_negatives": (_I, [_P, _P, _P, _L, _I, _I, _I, C.c_uint64, C.c_uint64, C.POINTER(CandidateList), _P,
                                  _P]),
    "dfm_sample_weighted": (_I, [_P, _P, _P, _L, _I, _I, _I, C.c_uint64, C.c_uint64, C.POINTER(CandidateList), _P,
                                 _P]),
    "dfm_catalogue_topk": (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "dfm_assemble_plan_create": (_I, [C.POINTER(AssembleColumn), _I, _L, _I, _I, _L, _L, _L, _P, _L, _I, _I,
                                      C.POINTER(CandidateList), C.POINTER(_P)]),
    "dfm_assemble_plan_destroy": (_I, [_P]),
    "dfm_record_assemble": (_I, [_P, _P, _L, _L, _P, _P, _P]),
    "dfm_assemble_plan_bind_history": (_I, [_P, _I, C.POINTER(HistorySource)]),
    "dfm_quant_row_bytes": (_I, [_I, _I]),
    "dfm_quantize_rows": (_I, [_P, _L, _P, _L, _L, _I, _I, _P, _P, _P]),
    "dfm_dequantize_rows": (_I, [_P, _L, _I, _I, _P, _P, _P]),
    "dfm_embedding_forward_quant": (_I, [C.POINTER(QuantField), _I, _I, _I, C.POINTER(_P), _P, _P, _L, _P, _P, _P, _P,
                                         _P, _AT]),
    "dfm_embedding_forward_record_quant": (_I, [_P, C.POINTER(_P), _I, _P, _L, _P, _P, _P, _L, _P, _P, _P, _P, _AT]),
    "dfm_platt_workspace_bytes": (_SZ, [_L]),
    "dfm_platt_fit": (_I, [_P, _P, _L, _I, _I, _I, C.c_double, _P, _P, _P]),
    "dfm_isotonic_workspace_bytes": (_SZ, [_I]),
    "dfm_isotonic_fit": (_I, [_P, _P, _L, _I, _F, _F, _P, _P, _P]),
    "dfm_calibrate_apply": (_I, [_I, _P, _P, _L, _P, _AT]),
    "dfm_vocab_capacity": (_L, [_L]),
    "dfm_vocab_build": (_I, [_P, _L, _P, _L, _P, _P]),
    "dfm_encode_columns": (_I, [C.POINTER(EncodeJob), _I, _L, _L, _P]),
    "dfm_seen_sets_build": (_I, [_P, _P, _L, _L, _L, _P, _P, _P, _P]),
    "dfm_entity_counts": (_I, [_P, _P, _P, _L, _L, _L, _P, _P, _P]),
    "dfm_temporal_split_mark": (_I, [_P, _P, _P, _L, _L, _L, _L, _P, _P, _P, _P, _P]),
    "dfm_loo_split_mark": (_I, [_P, _P, _P, _L, _L, _L, _P, _P, _P]),
    "dfm_history_index_build": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _P, _P, _P, _P, _P, _P, _P]),
    "dfm_history_gather": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _P, _P, _P, _P, _P]),
    "dfm_permutation_keys": (_I, [C.c_uint64, _L, _L, _P, _P]),
    "dfm_records_permute": (_I, [_P, _L, C.POINTER(RecordField), _I, _L, _L, _L, _L, _P, C.c_uint64, _L, _L, _P, _P]),
}

_lib: Optional[C.CDLL] = None


class HipLibraryError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the library once; raise loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C deepfm_amd/csrc`). deepfm_amd has no CPU or eager-PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.dfm_abi_version() != ABI_VERSION:
        raise HipLibraryError(f"ABI version mismatch: library {lib.dfm_abi_version()} != binding {ABI_VERSION} "
                              f"(stale {LIB_PATH}? rebuild with make -C deepfm_amd/csrc)")
    _lib = lib
    return lib


ERR_UNSUPPORTED = 3        # enum dfm_status: DFM_ERR_UNSUPPORTED


def check(rc: int) -> None:
    if rc != 0:
        msg = load().dfm_last_error().decode("utf-8", "replace")
        raise HipLibraryError(f"deepfm_hip error {rc}: {msg}")


def ptr(t) -> int:
    """Device pointer of a torch tensor (0 for None)."""
    return 0 if t is None else t.data_ptr()


def ptrs(tensors):
    """C array of the tensors' device pointers (a ``const void* const*`` argument)."""
    return (C.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


def stream_handle() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


def last_node() -> C.c_void_p:
    """The node of the launch captured last on the current stream (call it right behind that launch; the stream must
    be capturing).  ``at_node`` / ``at_nodes`` turn it into a launch destination once the graph is instantiated."""
    node = C.c_void_p()
    check(load().dfm_graph_last_node(stream_handle(), C.byref(node)))
    return node


def at_node(graph_exec: int, node: int) -> Launch:
    """The destination that re-points a captured kernel node of an instantiated graph (nothing is enqueued).  Build it
    once, where the node is recorded, not per batch."""
    return Launch(None, graph_exec, node.value if isinstance(node, C.c_void_p) else node)


def at_nodes(graph_exec: int, nodes):
    """``at_node`` over the nodes a capture recorded, in the shape it recorded them: one node, None, a tuple or a
    dict of them."""
    if isinstance(nodes, dict):
        return {k: at_nodes(graph_exec, v) for k, v in nodes.items()}
    if isinstance(nodes, tuple):
        return tuple(at_nodes(graph_exec, v) for v in nodes)
    return None if nodes is None else at_node(graph_exec, nodes)


def require_device(t, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} is on {t.device}: deepfm_amd runs on an MI355X HIP device only "
            "(there is no CPU fallback; use the reference implementation on CPU).")
