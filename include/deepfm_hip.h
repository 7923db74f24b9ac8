/*
 * deepfm_hip.h — C ABI of the MI355X (gfx950) CTR feature-interaction library.
 *
 * The reference (CodexploreRepo/deepfm) has no FFI layer: its operator interface is
 * the forward() of four torch.nn modules plus autograd.  Each entry point below is
 * the native replacement of one of those Python call sites; the host-side mirror in
 * deepfm_amd/models/layers/ binds them with ctypes.
 *
 * Conventions
 *   - every pointer named d_* / in the "device" column is a DEVICE pointer (HBM);
 *     pointer tables passed as `const T* const*` are HOST arrays of device pointers;
 *   - all floating point is IEEE fp32, ids are int64 (reference dataset.py:28-38);
 *   - `stream` is a hipStream_t (NULL = the null stream); calls only enqueue work,
 *     they never synchronise and are safe under hipGraph stream capture;
 *   - return value: 0 = DFM_OK, otherwise an error code; dfm_last_error() gives text;
 *   - id range errors (id < 0 or id >= vocabulary) never fault: the id is treated as
 *     the padding id 0 and bit 0 of *d_error_flag is set (the reference raises
 *     IndexError from ATen; the Python mirror raises IndexError when it reads the flag).
 */
#ifndef DEEPFM_HIP_H
#define DEEPFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFM_ABI_VERSION 11  /* bump whenever a struct layout or a signature in this header changes */
#define DFM_MAX_FIELDS 64      /* per-call pointer tables travel as kernel arguments */
#define DFM_MAX_CANDIDATES (1 << 20)   /* candidates per positive of an assemble plan; rows of a catalogue selection */
#define DFM_MAX_RANKS 64       /* data-parallel ranks of one job (csrc/shard.hip) */
#define DFM_ROWPLAN_CHUNK 4096 /* ids per sorted list (one LDS-resident sort) */

enum dfm_status { DFM_OK = 0, DFM_ERR_INVALID = 1, DFM_ERR_HIP = 2, DFM_ERR_UNSUPPORTED = 3 };
enum dfm_field_kind { DFM_SPARSE = 0, DFM_DENSE = 1, DFM_SEQUENCE = 2 };
enum dfm_combiner { DFM_MEAN = 0, DFM_SUM = 1, DFM_MAX = 2 };

typedef void* dfm_stream_t;

/* Where a re-pointable launch goes.  Ten entries take one instead of a stream: dfm_embedding_forward_staged,
 * dfm_embedding_forward_record, dfm_embedding_backward_record, dfm_rowplan_build, dfm_step_apply_plan,
 * dfm_stage_record, dfm_predict_head, dfm_embedding_forward_quant, dfm_embedding_forward_record_quant and
 * dfm_calibrate_apply.  A NULL dfm_launch* is the null stream.
 *   node == NULL: the launch is enqueued on `stream`, like any other call of this header.
 *   node != NULL: the launch was captured into a graph earlier (e.g. by torch.cuda.graph; `node` is what
 *     dfm_graph_last_node returned right after that captured call, `graph_exec` the INSTANTIATED graph): the node of
 *     that exec is re-pointed at this call's arguments (another batch record, other buffers) instead.  Host-side
 *     only, nothing is enqueued, `stream` is ignored; takes effect at the next launch of the exec.  Never re-point an
 *     exec whose previous launch may still be pending (the training steps alternate two execs for that reason).
 * graph_exec and node are both NULL or both set, else DFM_ERR_INVALID: the first check of every such entry, before
 * any other argument is looked at and before any HIP call.  Both modes apply the same argument checks; where an
 * empty batch enqueues nothing and returns DFM_OK, re-pointing at one is DFM_ERR_INVALID. */
typedef struct dfm_launch {
  dfm_stream_t stream;   /* node == NULL: enqueue here */
  void* graph_exec;      /* hipGraphExec_t, with node: re-point that node instead; nothing is enqueued */
  void* node;            /* hipGraphNode_t from dfm_graph_last_node */
} dfm_launch;

int dfm_abi_version(void);
const char* dfm_last_error(void);
/* CU count, wavefront size and gcnArchName of the current device. */
int dfm_device_info(int* cu_count, int* wave_size, char* arch, int arch_len);
/* Launches an empty kernel (timing calibration of event brackets in bench.py). */
int dfm_debug_empty_launch(dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * FeatureEmbedding  (reference deepfm/models/layers/embedding.py:20-126)
 * ------------------------------------------------------------------------------- */

/* One schema field with its parameter tensors (reference embedding.py:32-62):
 *   SPARSE / SEQUENCE: w2 = second_order_embeddings.<f>.weight (vocab, dim),
 *                      w1 = first_order_embeddings.<f>.weight  (vocab, 1)
 *   DENSE:             w2 = Linear(1,dim).weight (dim,1), b2 = .bias (dim),
 *                      w1 = Linear(1,1).weight (1,1),     b1 = .bias (1)
 *   proj = projections.<f>.weight (fm_dim, dim) or NULL when dim == fm_dim. */
typedef struct dfm_field {
  int32_t kind;        /* dfm_field_kind */
  int32_t dim;         /* embedding_dim of the field */
  int32_t vocab;       /* rows of w2 / w1 (0 for DENSE) */
  int32_t max_len;     /* SEQUENCE: ids per bag (L) */
  int32_t combiner;    /* SEQUENCE: dfm_combiner */
  int32_t flat_offset; /* column of this field inside flat_embeddings */
  int32_t stride2;     /* floats between consecutive rows of w2 (0 = dim: contiguous) */
  int32_t stride1;     /* floats between consecutive rows of w1 (0 = 1: contiguous) */
  const float* w2;
  const float* b2;
  const float* w1;
  const float* b1;
  const float* proj;
} dfm_field;

/* Gradient buffers matching dfm_field (dense, same shapes as the parameters). */
typedef struct dfm_field_grad {
  float* w2;
  float* b2;
  float* w1;
  float* b1;
  float* proj;
} dfm_field_grad;

typedef struct dfm_embedding_plan dfm_embedding_plan;

/* Uploads the field table once.  `fields` is a host array in schema order. */
int dfm_embedding_plan_create(const dfm_field* fields, int num_fields, int fm_dim,
                              dfm_embedding_plan** out_plan);
int dfm_embedding_plan_destroy(dfm_embedding_plan* plan);
/* 1 when every field is SPARSE or DENSE with dim == fm_dim (dim % 4 == 0) and no
 * projection: flat_embeddings is then field_embeddings reshaped (same bytes) and the
 * fused gather kernel is used. */
int dfm_embedding_plan_is_uniform(const dfm_embedding_plan* plan);
/* Bytes of scratch the forward/backward calls need for a batch of `batch` samples. */
size_t dfm_embedding_workspace_bytes(const dfm_embedding_plan* plan, int64_t batch);

/* FeatureEmbedding.forward (embedding.py:76-126).
 *   inputs[f]: SPARSE int64 (B,), SEQUENCE int64 (B, L) row-major, DENSE float (B,)
 *   d_first_order (B,1)  d_field_emb (B,F,fm_dim)  d_flat_emb (B, sum dim)
 * For a uniform plan d_flat_emb may be NULL or equal to d_field_emb (aliased).
 * d_fm_out (B,1), optional (uniform plans only): the FMInteraction value
 * 0.5*sum_d[(sum_f e)^2 - sum_f e^2] (fm.py:18-23) computed from the rows while they
 * are in registers; d_fm_sum (B, fm_dim), optional: S = sum_f e, which the FM backward
 * g*(S - e) needs (dfm_linear_backward's dfm_fm_bwd epilogue). */
int dfm_embedding_forward(const dfm_embedding_plan* plan, const void* const* inputs, int64_t batch,
                          float* d_first_order, float* d_field_emb, float* d_flat_emb,
                          float* d_fm_out, float* d_fm_sum, void* d_workspace, int32_t* d_error_flag,
                          dfm_stream_t stream);

/* dfm_embedding_forward for a uniform plan whose inputs sit in a batch record that changes every
 * step: the kernel also copies every field's raw input to stage_out[f] (host array of device
 * pointers, schema order: int64 (B,) / float (B,)) and, optionally, one float per sample from
 * d_extra_src to d_extra_dst (the labels) — the "load the next batch into the step's static
 * buffers" copy (reference trainer.py:214-217) without a launch of its own.  Every stage_out[f] is a buffer
 * distinct from inputs[f]. */
int dfm_embedding_forward_staged(const dfm_embedding_plan* plan, const void* const* inputs,
                                 void* const* stage_out, const float* d_extra_src, float* d_extra_dst,
                                 int64_t batch, float* d_first_order, float* d_field_emb, float* d_fm_out,
                                 float* d_fm_sum, int32_t* d_error_flag, const dfm_launch* at);

/* Eval-mode gather of any schema (SPARSE, SEQUENCE and DENSE fields, projections, mixed widths) from ONE batch
 * record in the mixed layout (deepfm_amd/data/packed.py:mixed_record_layout):
 *   [ ids (S, B) int64 | dense (Dn, B) float32 | labels (B) float32 | per SEQUENCE field, each block starting
 *     16-byte aligned: (B, max_length) int64, 0-padded ]
 * S and Dn count at least one slot each (an empty kind keeps one unused slot).  Writes
 *   d_first_order (B,1); d_flat: row b at d_flat + b * ld_flat (ld_flat % 4 == 0, d_flat 16-byte aligned),
 *   total_dim columns; d_field_emb (B, F, fm_dim), optional; d_fm_out (B), optional: the FM value
 *   0.5 * sum_d[(sum_f e)^2 - sum_f e^2]; d_fm_sum (B, fm_dim), optional, 16-byte aligned: S = sum_f e, summed over
 *   the fields in the order f = 0 .. F-1 (what dfm_embedding_forward's d_fm_sum is for uniform plans; the FM backward
 *   needs it), the other outputs do not depend on it; d_labels_out (B), optional: a copy of the record's labels.
 * Semantics of dfm_embedding_forward's general path (bags skip id 0, mean divides by the non-padding count, an
 * all-padding bag gives zeros), sums over fields in a fixed order: bitwise reproducible.  The plan must satisfy
 * fm_dim in {4, 8, 16, 32, 64}, every embedding_dim % 4 == 0, 16-byte aligned table rows, and projection plus
 * DENSE Linear(1, d) parameters of at most DFM_RECORD_PARAM_LDS_BYTES (staged in LDS once per workgroup);
 * otherwise DFM_ERR_UNSUPPORTED with the reason.  batch >= 1. */
#define DFM_RECORD_PARAM_LDS_BYTES 32768
int dfm_embedding_forward_record(const dfm_embedding_plan* plan, const void* d_record, int64_t batch,
                                 float* d_first_order, float* d_field_emb, float* d_flat, int64_t ld_flat,
                                 float* d_fm_out, float* d_fm_sum, float* d_labels_out, int32_t* d_error_flag,
                                 const dfm_launch* at);

/* Backward of dfm_embedding_forward_record for a model whose tables are DENSE parameters of one flat gradient buffer
 * (training/mixed_step.py): reads the same batch record and the upstream gradients
 *   d_g_first (B), d_g_field (B, F, fm_dim), d_g_flat: row b at d_g_flat + b * ld_g_flat, total_dim columns,
 * and the forward's flat_embeddings (d_flat_saved, row stride ld_flat; projection gradients), and STORES, for each of
 * dfm_embedding_backward_record_parts(batch) batch slices p, the slice's whole gradient of every embedding parameter
 * at d_workspace[p * grad_elems + (address of the gradient element - d_grad_base)]:
 *   SPARSE / SEQUENCE: (V, d) and (V, 1) table gradients; a row's gradient is the sum, in sample order, over the
 *     samples that name it of g_flat[b, off:off+d] + P^T g_field[b, f] (no projection: + g_field[b, f]), times 1/count
 *     for a mean bag; id 0 and out-of-range ids contribute nothing; rows nobody names are stored as 0;
 *   projections: dP[k, j] = sum_b g_field[b, f, k] * flat[b, off + j];   DENSE: the four Linear gradients.
 * `grads` are views of [d_grad_base, d_grad_base + grad_elems) (each starting on a 64-byte boundary, grad_elems % 16
 * == 0): the flat gradient buffer's embedding prefix.  Whoever owns that buffer adds the slices in slice order (a
 * dfm_slab_ref {d_workspace, d_grad_base, 1, 1, grad_elems, parts}: dfm_step_dense_prepare / dfm_linear_backward_finish).
 * The kernel writes every parameter element of every slice on every call and never the padding between parameters:
 * zero the workspace once.  No atomics; every sum has a fixed order: bitwise reproducible.
 * fold_fm != 0: the FM backward (fm.py:18-23) rides along (the kernel's other instantiation): wherever
 * g_field[b, f, :] is read the kernel uses
 *   g_eff[b, f, :] = g_field[b, f, :] + g_fm[b] * (S[b, :] - e[b, f, :])
 * with d_g_field optional (NULL: 0) and the trio d_g_fm (B), d_fm_sum (B, fm_dim) = S, d_field_emb (B, F, fm_dim) = e
 * optional (all three or none; NULL: g_field alone, the bits of fold_fm == 0); fm_sum and field_emb 16-byte aligned.
 * The product is rounded before the add, so with d_g_field NULL the result has the bits of dfm_fm_backward into a
 * buffer followed by a fold_fm == 0 call on that buffer.  fold_fm == 0: d_g_field is required and the trio is NULL.
 * Same slices, order, caps and refusals either way.  (The flag and not the operands picks the instantiation because
 * the two differ in time even where they agree in bits: DESIGN.md, "One launch destination".)
 * DFM_ERR_UNSUPPORTED with the reason for: a plan the record gather refuses, a max-combiner bag, more than
 * DFM_BWD_RECORD_MAX_ROW_SAMPLES (sum of vocabulary sizes) * batch, a field too wide for 64 KB of LDS. */
#define DFM_BWD_RECORD_MAX_ROW_SAMPLES (1 << 27)
int dfm_embedding_backward_record_parts(int64_t batch);
size_t dfm_embedding_backward_record_workspace_bytes(int64_t batch, int64_t grad_elems);
int dfm_embedding_backward_record(const dfm_embedding_plan* plan, const void* d_record, int64_t batch,
                                  const float* d_g_first, const float* d_g_field, const float* d_g_flat,
                                  int64_t ld_g_flat, const float* d_flat_saved, int64_t ld_flat,
                                  const float* d_g_fm, const float* d_fm_sum, const float* d_field_emb, int fold_fm,
                                  const dfm_field_grad* grads, const float* d_grad_base, int64_t grad_elems,
                                  void* d_workspace, const dfm_launch* at);

/* Graph plumbing: the node of the operation captured last on `stream` (call right after the launch): the `node` of a
 * dfm_launch that re-points it. */
int dfm_graph_last_node(dfm_stream_t stream, void** node_out);

/* Kernel-accurate timing of the uniform gather (measurement aid, bench.py): after
 * dfm_gather_timing_begin(n) the next n dfm_embedding_forward launches of a uniform plan carry HIP
 * start/stop events recorded around the dispatch itself (hipExtLaunchKernelGGL), on the stream the
 * kernel is launched on; dfm_gather_timing_end synchronises them, writes up to `capacity` durations
 * in microseconds to the HOST array h_us, the number written to *h_count, and disarms. */
int dfm_gather_timing_begin(int launches);
int dfm_gather_timing_end(float* h_us, int capacity, int* h_count);

/* Launch shape of the uniform gather (tuning aid, tools/time_gather.py): 0 = automatic (default),
 * 1 = one wave owns its samples across all fields (26 sparse + 13 dense slots in flight, no LDS),
 * 2 = 2 waves x (13 + 7), 3 = 4 waves x (8 + 4), 4 = 8 waves x (4 + 2), 5 = the two-wave kernel with
 * compile-time slot indices (the automatic choice where it applies), 6 = shape 5 with streaming stores.
 * Every shape computes the
 * same values (bitwise for the gathered rows); only the work split inside a workgroup changes. */
int dfm_gather_set_shape(int shape);

/* Autograd of the forward w.r.t. every parameter as DENSE gradients — the reference
 * semantics (nn.Embedding(sparse=False), embedding.py:35-40).  Gradients are ADDED
 * into the buffers of `grads` (caller zero-fills them); row 0 receives none.
 * d_g_flat may be NULL for a uniform plan whose flat view aliases field_emb (the
 * caller has already summed both into d_g_field).  d_flat_saved: the forward's
 * flat_embeddings, needed only when the plan has projections (else NULL). */
int dfm_embedding_backward_dense(const dfm_embedding_plan* plan, const void* const* inputs,
                                 int64_t batch, const float* d_g_first, const float* d_g_field,
                                 const float* d_g_flat, const dfm_field_grad* grads,
                                 const void* d_flat_saved, dfm_stream_t stream);

/* Gradients of the DENSE fields' Linear parameters only (deterministic tree
 * reduction over the batch); used by the row-sparse mode together with
 * dfm_rowgrad_build for the SPARSE fields. */
int dfm_embedding_backward_dense_fields(const dfm_embedding_plan* plan, const void* const* inputs,
                                        int64_t batch, const float* d_g_first,
                                        const float* d_g_field, const float* d_g_flat,
                                        const dfm_field_grad* grads, dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Row plan + row-wise gradient: the backward scatter-add of the SPARSE fields without
 * atomics (reference: autograd of embedding.py:95-98, i.e. aten::embedding_dense_backward)
 * ------------------------------------------------------------------------------- */

/* For each of `num_sparse` id vectors (n ids each) and each chunk of DFM_ROWPLAN_CHUNK
 * ids: stable sort by id, drop id 0, find the distinct ids.  With C = ceil(n/chunk):
 *   d_sorted_pos (C, S, chunk) int32  sample position of every sorted entry
 *   d_uniq_rows  (C, S, chunk) int32  distinct ids, ascending
 *   d_seg_start  (C, S, chunk+1) int32  first sorted entry of every distinct id
 *   d_num_uniq   (C, S) int32
 * Entries of a list behind its num_uniq (+ 1 for d_seg_start) are working space of the library: the tail of
 * d_seg_start carries the list's runs of more than half a chunk and an arrival counter for
 * dfm_rowgrad_build, which sums such a run with several workgroups.
 * Depends on the ids only, so it can run ahead of the forward pass.
 * touch_tables (optional; dfm_table per SPARSE field, only w2 / stride2 are read; dim = row length for stride2 = 0):
 * extra workgroups of the same launch read the ids and TOUCH the first line of every row the batch will gather
 * (embedding.py:95-98 reads them next), pulling the ids and the 128-B row lines into the Infinity Cache while the
 * sort occupies 26 of the 256 CUs — launched in FRONT of dfm_embedding_forward_staged on the same batch record
 * (training/step.py), the gather then finds its operands on-die.  Results do not depend on it. */
typedef struct dfm_table dfm_table;
int dfm_rowplan_build(const int64_t* const* ids, const int32_t* vocab, int num_sparse, int64_t n,
                      int32_t* d_sorted_pos, int32_t* d_uniq_rows, int32_t* d_seg_start,
                      int32_t* d_num_uniq, int32_t* d_error_flag, const dfm_table* touch_tables, int dim,
                      const dfm_launch* at);

/* Row gradients of the distinct ids, contributions added in increasing sample order (runs of more than 64
 * contributions: by a fixed tree — reproducible run to run, equal to the sequential sum up to rounding):
 *   d_row_g2 (C, S, chunk, dim)   d_row_g1 (C, S, chunk)      rows behind num_uniq: working space
 * d_seg_start must come from dfm_rowplan_build (its tail is read, and its counter written).
 * `field_of_sparse[s]` is the schema position of sparse field s inside d_g_field
 * (B, F, dim); d_g_first is (B,1).  Uniform plans only (dim == fm_dim). */
int dfm_rowgrad_build(const int32_t* field_of_sparse, int num_sparse, int num_fields, int dim,
                      int64_t n, const float* d_g_first, const float* d_g_field,
                      const int32_t* d_sorted_pos, int32_t* d_seg_start,
                      const int32_t* d_num_uniq, float* d_row_g2, float* d_row_g1,
                      dfm_stream_t stream);

/* Row-wise optimizer over `num_lists` = ranks x chunks lists (all-gathered under data
 * parallelism).  A row present in several lists is owned by its first list; the owner
 * adds the other lists' gradients in list order (bit-identical on every replica),
 * then:  g = grad_scale * sum + 2*l2*w ;  g *= clip ;  update rule (w, m, v, g)
 * (reference trainer.py:224-237 restricted to the rows the batch touched — DESIGN.md).
 * dfm_step_prepare writes the merged gradients in place and one partial sum of |g|^2 per
 * workgroup into d_partials[0 .. dfm_rowadam_num_partials); dfm_step_apply reads
 * *d_clip_coef (NULL = 1). */
typedef struct dfm_table {
  float* w2; float* m2; float* v2;   /* (V, dim) weights and Adam moments, row stride `stride2` floats */
  float* w1; float* m1; float* v1;   /* (V, 1) first-order ones, row stride `stride1` floats */
  int32_t stride2;                   /* 0 = dim (contiguous tensors) */
  int32_t stride1;                   /* 0 = 1 */
} dfm_table;
/* Packed row records (FeatureEmbedding.pack_tables_): all six arrays are views of one (V, RS)
 * buffer — [w2 | w1 m1 v1 pad | m2 | v2 | pad], RS a multiple of 32 floats — so a row's forward
 * reads hit one 128-B line and its Adam update touches one contiguous record. */

/* Update rules of the apply launches (dfm_optim.kind), each as the reference's trainer builds it (trainer.py:67-78):
 *   DFM_OPT_ADAM  : torch.optim.Adam(betas, eps)
 *   DFM_OPT_ADAMW : torch.optim.AdamW(betas, eps, weight_decay): p *= 1 - lr*wd, then the Adam update
 *   DFM_OPT_SGD   : torch.optim.SGD(momentum, dampening 0, no Nesterov): buf = momentum*buf + g, p -= lr*buf;
 *                   buf lives where Adam's first moment does (m2 / m1 / d_m); v2 / v1 / d_v are not accessed
 * The learning rate is read from device memory (d_lr: one fp32 scalar) by every launch, so a captured graph uses
 * the value current when it runs.  Row-wise updates stay lazy: only the rows a batch touched decay or move. */
enum dfm_opt_kind { DFM_OPT_ADAM = 0, DFM_OPT_ADAMW = 1, DFM_OPT_SGD = 2 };
typedef struct dfm_optim {
  int32_t kind;
  float beta1, beta2, eps;      /* Adam / AdamW */
  float weight_decay;           /* AdamW */
  float momentum;               /* SGD */
  const float* d_lr;
} dfm_optim;

int64_t dfm_rowadam_num_partials(int num_sparse, int dim, int num_lists);

/* *d_sq_norm = sum(partials) in a fixed order; *d_clip_coef = min(1, max_norm/(sqrt+1e-6))
 * (clip_grad_norm_, trainer.py:232-235; max_norm <= 0 disables clipping: coef 1).
 * Optional "tick": *d_step_tick += 1 (Adam's step count, read by the update kernels enqueued after
 * this call) and *d_seed_tick += 1 (dropout seed of the next step) — saves two launches. */
int dfm_grad_norm_finalize(const float* d_partials, int64_t num_partials, float max_norm,
                           float* d_sq_norm, float* d_clip_coef, int32_t* d_step_tick,
                           int64_t* d_seed_tick, dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * FMInteraction  (reference deepfm/models/layers/fm.py:18-23)
 * dfm_fm_forward / dfm_fm_backward: dim <= 64, or a multiple of 4 up to 256 with the (B, F, dim) buffers 16-byte
 * aligned (the float4 kernels; a multiple of 4 on a buffer that is not runs one float per lane, dim <= 64).
 * dfm_embedding_grad_combine and dfm_copy_2d: 16-byte aligned buffers only.
 * ------------------------------------------------------------------------------- */
int dfm_fm_forward(const float* d_field_emb, int64_t batch, int num_fields, int dim, float* d_out,
                   dfm_stream_t stream);
/* d e[b,f,:] = g[b] * (S[b,:] - e[b,f,:]) */
int dfm_fm_backward(const float* d_field_emb, const float* d_g_out, int64_t batch, int num_fields,
                    int dim, float* d_g_field, dfm_stream_t stream);
/* d field_embeddings of a model with several consumers of the embeddings (attention_deepfm.py:48-66):
 * out[b, :] = g_flat[b, :width] (row stride ld_flat floats: a slice of the DNN's d input)
 *           + g_extra[b, :]                     (d from another layer, e.g. the attention stack; or NULL)
 *           + g_fm[b] * (S[b, d] - e[b, f, d])  (FMInteraction backward, fm.py:18-23; or NULL). */
int dfm_embedding_grad_combine(const float* d_g_flat, int64_t ld_flat, const float* d_g_extra, const float* d_g_fm,
                               const float* d_fm_sum, const float* d_field_emb, int64_t batch, int num_fields, int dim,
                               float* d_g_field, dfm_stream_t stream);
/* dst[r, :width] = src[r, :width] for r < rows, row strides ld_src / ld_dst floats (slices of the
 * concatenated DNN input of attention_deepfm.py:57-61 and of its gradient). */
int dfm_copy_2d(const float* d_src, int64_t ld_src, float* d_dst, int64_t ld_dst, int64_t rows, int width,
                dfm_stream_t stream);

/* Arithmetic of the matrix-core CIN path: 0 = bf16 x 3 split products (default; meets the 1e-4 bar
 * against cin.py:66-105), 1 = plain bf16 (throughput mode, its own looser tolerance), 2 = exact-fp32
 * VALU kernels only.  Process-wide; bench.py records it and refuses to report headline numbers in a
 * non-default mode. */
int dfm_cin_set_mode(int mode);
int dfm_cin_get_mode(void);

/* ---------------------------------------------------------------------------------
 * CIN  (reference deepfm/models/layers/cin.py:26-105)
 *   per layer i:  Z[b,h*F+f,d] = hidden_i[b,h,d] * x0[b,f,d]          (cin.py:84-87, never stored)
 *                 Y_i = relu(W_i Z + bias_i)  (B, C_i, D)              (cin.py:90-91)
 *                 split [direct | next] along channels, direct first   (cin.py:93-96)
 *                 out[:, col_i : col_i+direct_i] = sum_d Y_i[:, :direct_i, :]  (cin.py:102-105)
 *   weights[i] = conv_layers.<i>.weight (C_i, H_i*F[, 1]),  biases[i] = conv_layers.<i>.bias (C_i)
 *   layer_sizes / split_half as in CIN.__init__ (cin.py:41-64).
 * d_saved receives the post-ReLU Y_i of every layer (dfm_cin_saved_bytes) for the backward
 * (may be NULL for inference on the matrix-core path).  d_workspace
 * (dfm_cin_forward_workspace_bytes) holds the bf16 hi/lo weight fragments of the MFMA path
 * (F <= 40, D in {8,16,32}, at most 8 layers, layer sizes <= 128, and 16 KB per 8 fields + 1 KB per
 * hidden row of the tallest layer within the 160 KB of LDS); without it, or for other shapes, the general
 * fp32 kernels run.  Environment DFM_CIN_MODE = split (default, bf16 x 3: parity grade) |
 * bf16 (plain bf16 MFMA, throughput mode) | fp32 (general kernels only).
 * ------------------------------------------------------------------------------- */
int dfm_cin_output_dim(const int32_t* layer_sizes, int num_layers, int split_half);
size_t dfm_cin_saved_bytes(const int32_t* layer_sizes, int num_layers, int split_half, int64_t batch,
                           int num_fields, int dim);
size_t dfm_cin_forward_workspace_bytes(const int32_t* layer_sizes, int num_layers, int split_half,
                                       int num_fields, int dim);
size_t dfm_cin_backward_workspace_bytes(const int32_t* layer_sizes, int num_layers, int split_half,
                                        int64_t batch, int num_fields, int dim);
/* The kernels dfm_cin_forward (called with its workspace) and dfm_cin_backward take for this shape in the
 * current mode: 0 = matrix-core forward and backward, 1 = matrix-core forward, general backward (D = 8 with an
 * odd batch), 2 = general fp32 kernels; negative for an invalid layer list.  Host-side and read-only. */
int dfm_cin_route(const int32_t* layer_sizes, int num_layers, int split_half, int64_t batch,
                  int num_fields, int dim);
int dfm_cin_forward(const float* d_x0, int64_t batch, int num_fields, int dim,
                    const float* const* weights, const float* const* biases,
                    const int32_t* layer_sizes, int num_layers, int split_half, float* d_out,
                    float* d_saved, void* d_workspace, dfm_stream_t stream);
/* d_g_x0 (B,F,D) is overwritten; weight / bias gradients are ADDED into g_weights[i] / g_biases[i]. */
int dfm_cin_backward(const float* d_x0, int64_t batch, int num_fields, int dim,
                     const float* const* weights, const int32_t* layer_sizes, int num_layers,
                     int split_half, const float* d_saved, const float* d_g_out, float* d_g_x0,
                     float* const* g_weights, float* const* g_biases, void* d_workspace,
                     dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Field self-attention block  (reference deepfm/models/layers/attention.py:67-120)
 *   one _AttentionBlock per call; MultiHeadSelfAttention.forward (attention.py:52-64) calls it
 *   once per layer.  params[] (device pointers), PyTorch layouts:
 *     0 W_q.weight (A,D) 1 W_q.bias (A) 2 W_k.weight 3 W_k.bias 4 W_v.weight 5 W_v.bias
 *     6 W_out.weight (D,A) 7 W_out.bias (D) 8 layer_norm.weight (D) 9 layer_norm.bias (D)
 *   (8, 9 only when use_residual).  x, out, g_out, g_x are (B, F, D).
 * The backward recomputes the forward per sample; parameter gradients are ADDED into
 * g_params[] (same order/shapes as params[]); d_g_x is overwritten.
 * ------------------------------------------------------------------------------- */
int dfm_attention_forward(const float* d_x, int64_t batch, int num_fields, int embed_dim,
                          int attention_dim, int num_heads, int use_residual,
                          const float* const* params, float* d_out, dfm_stream_t stream);
size_t dfm_attention_backward_workspace_bytes(int64_t batch, int embed_dim, int attention_dim);
int dfm_attention_backward(const float* d_x, const float* d_g_out, int64_t batch, int num_fields,
                           int embed_dim, int attention_dim, int num_heads, int use_residual,
                           const float* const* params, float* d_g_x, float* const* g_params,
                           void* d_workspace, dfm_stream_t stream);

/* GEMM-structured attention path (attention.py:91-120): the projections run on dfm_gemm_f32 over
 * the B*F rows; these are the remaining per-sample pieces.
 *   core   : o[b,i,h*hd:(h+1)*hd] = softmax(q_h k_h^T / sqrt(hd)) v_h, qkv (B*F, 3A) rows [q|k|v]
 *            (F <= 64, head_dim in {4,8,16,32}); the backward recomputes the probabilities
 *   LN     : out = LayerNorm(y + res) * gamma + beta over the last dim; stats (rows, 2) = mean, rstd;
 *            backward gives d(y+res) and ADDS d gamma / d beta */
int dfm_attention_core_supported(int num_fields, int attention_dim, int num_heads);
int dfm_attention_core_forward(const float* d_qkv, int64_t batch, int num_fields, int attention_dim,
                               int num_heads, float* d_o, dfm_stream_t stream);
int dfm_attention_core_backward(const float* d_qkv, const float* d_g_o, int64_t batch, int num_fields,
                                int attention_dim, int num_heads, float* d_g_qkv, dfm_stream_t stream);
/* The same core with the Q | K | V projection (attention.py:95-97, three Linear(D, A)) inside the kernel:
 * d_x (batch * num_fields, embed_dim), d_w_qkv (3 * attention_dim, embed_dim) = [W_q; W_k; W_v] stacked,
 * d_b_qkv (3 * attention_dim).  The (batch * num_fields, 3 * attention_dim) projection is never written;
 * the backward recomputes it from d_x and returns its gradient d_g_qkv, which feeds the weight / input
 * gradient GEMMs.  _supported(): head_dim 16, <= 48 fields, embed_dim in {16, 32, 48, 64}; all buffers
 * 16-byte aligned. */
int dfm_attention_qkv_core_supported(int num_fields, int embed_dim, int attention_dim, int num_heads);
int dfm_attention_qkv_core_forward(const float* d_x, const float* d_w_qkv, const float* d_b_qkv, int64_t batch,
                                   int num_fields, int embed_dim, int attention_dim, int num_heads, float* d_o,
                                   dfm_stream_t stream);
int dfm_attention_qkv_core_backward(const float* d_x, const float* d_w_qkv, const float* d_b_qkv,
                                    const float* d_g_o, int64_t batch, int num_fields, int embed_dim,
                                    int attention_dim, int num_heads, float* d_g_qkv, dfm_stream_t stream);
/* The whole forward of one _AttentionBlock (attention.py:91-120) in ONE launch, num_heads == 4 (a workgroup's
 * four waves are the four heads of a sample): projection + softmax(QK^T / sqrt(hd)) V + W_out + b_out and, when
 * d_gamma / d_beta are given, LayerNorm(y + x).  Writes what the backward needs: d_o (batch * num_fields,
 * attention_dim) head outputs, d_y (batch * num_fields, embed_dim) = the block's output before the residual,
 * d_stats (rows, 2) mean / rstd; d_out as dfm_layernorm_forward (out_group_stride > 0: sample b's rows at
 * d_out + b * out_group_stride).  _supported(): dfm_attention_qkv_core_supported and num_heads == 4. */
int dfm_attention_block_supported(int num_fields, int embed_dim, int attention_dim, int num_heads);
int dfm_attention_block_forward(const float* d_x, const float* d_w_qkv, const float* d_b_qkv, const float* d_w_out,
                                const float* d_b_out, const float* d_gamma, const float* d_beta, float eps,
                                int64_t batch, int num_fields, int embed_dim, int attention_dim, int num_heads,
                                float* d_o, float* d_y, float* d_out, float* d_stats, int64_t out_group_stride,
                                float* d_x_copy, int64_t x_copy_group_stride, dfm_stream_t stream);
/* (d_x_copy, optional: the block's input rows once more, sample b at d_x_copy + b * x_copy_group_stride — the
 * second half of AttentionDeepFM's cat([attention(e), e]), attention_deepfm.py:57-61, without a copy pass.)
 * The backward of the same block from d_g_y (gradient of the output projection's result y; residual != 0: also
 * the gradient reaching x through the residual) to d_g_x (batch * num_fields, embed_dim), in ONE launch: the
 * head's d O = d y W_out[:, head], the core backward, and d x = d Q W_q + d K W_k + d V W_v (+ d y) all stay in
 * the kernel.  d_g_qkv (batch * num_fields, 3 * attention_dim) is written for the weight-gradient GEMM
 * d W_qkv = d_g_qkv^T x; d W_out = d_g_y^T o is a GEMM on the forward's d_o.  d_g_x must not alias an input.
 * Optional further terms of d_g_x for the block that reads the field embeddings themselves (what
 * dfm_embedding_grad_combine adds in a pass of its own): d_g_flat (rows of num_fields * embed_dim floats at
 * stride ld_flat: the flat half of the DNN's d input) and the FM backward d_g_fm[b] * (d_fm_sum[b, :] - x). */
int dfm_attention_block_backward(const float* d_x, const float* d_w_qkv, const float* d_b_qkv, const float* d_w_out,
                                 const float* d_g_y, int residual, int64_t batch, int num_fields, int embed_dim,
                                 int attention_dim, int num_heads, float* d_g_qkv, float* d_g_x,
                                 const float* d_g_flat, int64_t ld_flat, const float* d_g_fm, const float* d_fm_sum,
                                 dfm_stream_t stream);
size_t dfm_layernorm_workspace_bytes(int64_t rows, int dim);
/* out_group_rows > 0: output row r is written at d_out + (r / out_group_rows) * out_group_stride +
 * (r % out_group_rows) * dim (the attention output as the first half of the DNN's concatenated input,
 * attention_deepfm.py:57-61, without a copy); 0: contiguous (rows, dim). */
int dfm_layernorm_forward(const float* d_y, const float* d_res, int64_t rows, int dim, const float* d_gamma,
                          const float* d_beta, float eps, float* d_out, float* d_stats, int64_t out_group_rows,
                          int64_t out_group_stride, dfm_stream_t stream);
/* g_group_rows / g_group_stride: the same addressing for the incoming gradient d_g_out. */
int dfm_layernorm_backward(const float* d_g_out, const float* d_y, const float* d_res, const float* d_stats,
                           int64_t rows, int dim, const float* d_gamma, float* d_g_sum, float* d_g_gamma,
                           float* d_g_beta, void* d_workspace, int64_t g_group_rows, int64_t g_group_stride,
                           dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * DNN tower glue (reference deepfm/models/layers/dnn.py:45-55): BatchNorm1d (training
 * statistics) -> ReLU -> Dropout between the Linear GEMMs, two launches each way.
 *   forward : out = dropout_p(relu(gamma * (z - mean) * rstd + beta)), z (batch, features);
 *             saves mean / rstd (2, features); updates running_mean / running_var (unbiased,
 *             momentum) and num_batches_tracked like nn.BatchNorm1d when they are non-NULL
 *   backward: d z from d out (recomputes y and the dropout mask); ADDS d gamma / d beta
 * Dropout keeps element i iff hash(*d_seed, salt, i) >= p * 2^32 (scale 1/(1-p)); the seed is
 * read on the device, so forward and backward agree and a replayed graph gets fresh masks.
 * ------------------------------------------------------------------------------- */
size_t dfm_bn_workspace_bytes(int64_t batch, int features);
int dfm_bn_relu_dropout_forward(const float* d_z, int64_t batch, int features, const float* d_gamma,
                                const float* d_beta, float* d_running_mean, float* d_running_var,
                                int64_t* d_num_batches, float momentum, float eps, float p_drop,
                                const int64_t* d_seed, int salt, float* d_out, float* d_mean_rstd,
                                void* d_workspace, dfm_stream_t stream);
int dfm_bn_relu_dropout_backward(const float* d_g_out, const float* d_z, const float* d_mean_rstd,
                                 const float* d_gamma, const float* d_beta, int64_t batch, int features,
                                 float p_drop, const int64_t* d_seed, int salt, float* d_g_z,
                                 float* d_g_gamma, float* d_g_beta, void* d_workspace,
                                 dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * BCEWithLogitsLoss, mean reduction (reference deepfm/training/trainer.py:59, 221):
 * *d_loss = mean(max(z,0) - z*y + log1p(exp(-|z|)));  d_g_logits = (sigmoid(z) - y) / n.
 * ------------------------------------------------------------------------------- */
size_t dfm_bce_workspace_bytes(int64_t n);
int dfm_bce_with_logits(const float* d_logits, const float* d_labels, int64_t n, float* d_loss,
                        float* d_g_logits, void* d_workspace, dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Fused DNN tower + head of the training step (reference dnn.py:45-55 [Linear -> BatchNorm1d ->
 * ReLU -> Dropout] * n; deepfm.py:30-42 first_order + fm + output_linear(dnn); trainer.py:59,221
 * BCEWithLogitsLoss).  Few launches, none with a serial tail (csrc/tower.hip):
 *   forward, per layer : dfm_linear_bn_forward (GEMM + per-tile column statistics),
 *                        dfm_bn_relu_dropout_apply (merges the statistics, then normalises)
 *   head               : dfm_head_bce (logits, d logits, the last BN's mask, partial sums), or
 *                        dfm_head_bn_bce = the last block's dfm_bn_relu_dropout_apply + dfm_head_bce
 *   backward, per layer: dfm_bn_backward_apply (merges the partial sums, then dz),
 *                        dfm_linear_backward (dW and dx in one launch; the dx epilogue is the lower
 *                        layer's BatchNorm mask or the FM backward)
 * All reductions have a fixed order (no floating-point atomics, no arrival counters).
 * ------------------------------------------------------------------------------- */

/* One BatchNorm -> ReLU -> Dropout block as the backward sees it.  Producer (dfm_head_bce or
 * dfm_linear_backward's bn_below): dy = g * [y > 0] * dropout mask/(1-p), y = gamma*(z-mean)*rstd
 * + beta, plus partial column sums of dy and dy*xhat in `workspace`.  Consumer
 * (dfm_bn_backward_apply): merges them, adds the affine gradients, writes dz. */
typedef struct dfm_bn_bwd {
  const float* z;          /* (batch, features) pre-activations saved by the forward */
  const float* mean_rstd;  /* (2, features) batch mean, 1/sqrt(var+eps) from dfm_bn_relu_dropout_apply */
  const float* gamma;      /* (features) BatchNorm weight */
  const float* beta;       /* (features) BatchNorm bias */
  float* dy;               /* (batch, features) masked upstream gradient */
  float* g_gamma;          /* (features), ADDED: sum dy * xhat */
  float* g_beta;           /* (features), ADDED: sum dy */
  const int64_t* seed;     /* device dropout seed (NULL when p_drop == 0) */
  void* workspace;         /* dfm_bn_bwd_workspace_bytes(batch, features) */
  float p_drop;
  int32_t salt;            /* layer index, as passed to dfm_bn_relu_dropout_apply */
} dfm_bn_bwd;

/* What else flows back into the embeddings, folded into the first Linear's d input:
 * d e = d flat + g_fm * (S - e)  [FMInteraction backward, fm.py:18-23; g_fm NULL: no FM term]
 *              + addend          [gradient from another consumer of field_embeddings: CIN
 *                                 (xdeepfm.py:36-48) or the attention stack; NULL: none]. */
typedef struct dfm_fm_bwd {
  const float* g_fm;       /* (batch) d loss / d fm value, or NULL */
  const float* fm_sum;     /* (batch, dim) S = sum_f e (dfm_embedding_forward's d_fm_sum) */
  const float* e;          /* (batch, fields * dim) field embeddings */
  const float* addend;     /* (batch, fields * dim), or NULL */
  int32_t dim;
} dfm_fm_bwd;

/* What dfm_head_bce leaves for the dfm_bn_backward_apply that follows it to finish. */
typedef struct dfm_head_tail {
  float* g_w;              /* (features) head weight gradient, ADDED */
  float* g_b;              /* (1) head bias gradient, ADDED (may be NULL) */
  float* loss;             /* (1) mean BCE-with-logits, written */
  float* g_b2;             /* (1) ADDED the same sum as g_b: the bias of another 1-wide Linear that is added to the
                            * logit (xDeepFM's cin_linear, xdeepfm.py:41-47), or NULL */
} dfm_head_tail;

size_t dfm_linear_bn_workspace_bytes(int64_t batch, int features);
/* z (batch, out) = x W^T + b; per-column (mean, M2) of every 32-row tile go to d_workspace for
 * dfm_bn_relu_dropout_apply. */
int dfm_linear_bn_forward(const float* d_x, int64_t ldx, const float* d_w, const float* d_bias,
                          int64_t batch, int out_features, int in_features, float* d_z,
                          void* d_workspace, dfm_stream_t stream);
/* Batch statistics from dfm_linear_bn_forward's workspace -> d_mean_rstd (2, features) = mean and
 * 1/sqrt(biased var + eps); running_mean / running_var / num_batches_tracked updated like
 * nn.BatchNorm1d when non-NULL; out = dropout_p(relu(gamma * (z - mean) * rstd + beta)).
 * features % 4 == 0. */
int dfm_bn_relu_dropout_apply(const float* d_z, int64_t batch, int features, const void* d_workspace,
                              const float* d_gamma, const float* d_beta, float* d_mean_rstd,
                              float* d_running_mean, float* d_running_var, int64_t* d_num_batches,
                              float momentum, float eps, float p_drop, const int64_t* d_seed, int salt,
                              float* d_out, dfm_stream_t stream);
size_t dfm_bn_bwd_workspace_bytes(int64_t batch, int features);
/* logits = (first_order + fm) + (a w^T + b)   (NULL first_order / fm / b count as 0);
 * d_g_logits = (sigmoid - y) / batch; the gradient w.r.t. a goes through `bn` (the BatchNorm block
 * that produced a): bn->dy and partial sums in bn->workspace.  The loss and the head's own
 * gradients are finished by dfm_bn_backward_apply(bn, ..., head).  features % 32 == 0, <= 256. */
int dfm_head_bce(const float* d_a, int64_t batch, int features, const float* d_w, const float* d_b,
                 const float* d_first_order, const float* d_fm, const float* d_labels, float* d_logits,
                 float* d_g_logits, const dfm_bn_bwd* bn, dfm_stream_t stream);
/* dfm_bn_relu_dropout_apply of the tower's LAST block and dfm_head_bce in one launch: every workgroup merges
 * the column statistics in d_fwd_workspace (dfm_linear_bn_forward's) exactly as dfm_bn_relu_dropout_apply does,
 * workgroup 0 writes d_mean_rstd (= bn->mean_rstd) and the running statistics, and
 * a = dropout(relu(gamma * (bn->z - mean) * rstd + beta)) is formed in registers and never stored (the backward
 * needs z, the statistics and the mask).  Results are bit-identical to the two calls it replaces. */
int dfm_head_bn_bce(const void* d_fwd_workspace, float* d_mean_rstd, float* d_running_mean, float* d_running_var,
                    int64_t* d_num_batches, float momentum, float eps, int64_t batch, int features,
                    const float* d_w, const float* d_b, const float* d_first_order, const float* d_fm,
                    const float* d_labels, float* d_logits, float* d_g_logits, const dfm_bn_bwd* bn,
                    dfm_stream_t stream);
/* dz = gamma * rstd * (dy - mean(dy) - xhat * mean(dy * xhat)), d gamma / d beta ADDED; d_dz may be
 * bn->dy.  `head` non-NULL iff bn was filled by dfm_head_bce (it then also receives the loss and
 * the head gradients). */
int dfm_bn_backward_apply(const dfm_bn_bwd* bn, int64_t batch, int features, const dfm_head_tail* head,
                          float* d_dz, dfm_stream_t stream);
size_t dfm_linear_backward_workspace_bytes(int64_t batch, int out_features, int in_features);
/* Backward of z = x W^T + b given dz (batch, out): the d weight product dz^T x, split over the
 * batch into partial products left in d_workspace (dfm_linear_backward_finish adds them into the
 * gradient buffers of all layers in one launch), and the gradient
 * w.r.t. x (batch, in) either stored to d_g_x (plus the FM backward when `fm` is given), or pushed
 * through the BatchNorm block that produced x (`bn_below`; d_g_x unused).  The bias gradient is
 * not computed: in front of a training-mode BatchNorm it is identically zero.
 * parts: 1 = d weight only, 2 = d input only, 3 = both in one launch.  The two halves are
 * independent given dz, so a caller may put the d weight half on a side stream: only d input is on
 * the backward's critical path. */
int dfm_linear_backward(const float* d_dz, int64_t batch, int out_features, const float* d_x,
                        int in_features, const float* d_w, float* d_g_x,
                        const dfm_bn_bwd* bn_below, const dfm_fm_bwd* fm, int parts, void* d_workspace,
                        dfm_stream_t stream);
/* A Linear with ONE output that is added to the logit (xDeepFM's cin_linear, xdeepfm.py:41-47).
 * forward: d_out[b] = d_x[b, :] . d_w (+ d_b[0]).  backward: d_g_x[b, :] = d_g[b] * d_w, and the weight
 * gradient as dfm_linear1_backward_splits(batch) slabs of `features` floats in d_workspace — add them with a
 * dfm_slab_ref {workspace, g_w, batch 1, out 1, in features, splits}; the bias gradient is sum(d_g) =
 * dfm_head_tail.g_b2 when d_g is the head's d logits.  features % 4 == 0, <= 1024 (dfm_linear1_supported). */
int dfm_linear1_supported(int features);
int dfm_linear1_forward(const float* d_x, int64_t batch, int features, const float* d_w, const float* d_b,
                        float* d_out, dfm_stream_t stream);
int dfm_linear1_backward_splits(int64_t batch);
int dfm_linear1_backward(const float* d_g, const float* d_x, int64_t batch, int features, const float* d_w,
                         float* d_g_x, void* d_workspace, dfm_stream_t stream);
/* d_g_w (out, in) += sum of the batch-split partial products of one dfm_linear_backward call. */
typedef struct dfm_slab_ref {
  const void* workspace;   /* the d_workspace that call was given */
  float* g_w;              /* (out, in) gradient buffer, ADDED */
  int64_t batch;
  int32_t out_features;
  int32_t in_features;
  int32_t splits;          /* 0: the batch split dfm_linear_backward chose for (batch, out, in); > 0: that many
                            * slabs of out * in floats from any producer (dfm_step_embedding_backward's
                            * batch-split DENSE-field gradients) */
  int32_t reserved;
} dfm_slab_ref;
int dfm_linear_backward_finish(const dfm_slab_ref* refs, int count, dfm_stream_t stream);
/* Number of batch splits (slabs) dfm_linear_backward leaves in its workspace for this shape. */
/* Arithmetic of the DNN tower's GEMMs (dnn.py:45-59): 0 = exact fp32 matrix pipe; 1 = fp32 forward, bf16 x 3 split
 * (fp32 accumulate, 2^-16 per product) inside dfm_linear_backward — ReLU / dropout masks never change; 2 = bf16 x 6
 * (every fp32 operand split exactly into three bf16 values, the six largest partial products kept: 2^-23 per
 * product, i.e. fp32-faithful) forward and backward — the fused training steps then run the tower through the
 * *_x6 / *_planes entry points below; the library only records the choice.
 * Process-wide, explicit; applies to steps built / calls enqueued afterwards (a captured graph keeps what it
 * captured). */
int dfm_tower_set_mode(int mode);
int dfm_tower_get_mode(void);

/* ---- bf16 x 6 tower (csrc/gemm_x6.h, tower.hip): operands of the tower's GEMMs as "planes" ---------------------
 * A plane set holds an fp32 matrix split exactly into three bf16 matrices (x = h + m + l), laid out for one
 * contraction: bf16 [3][G][Rp][8], G = 8 ceil(contraction / 64), Rp = 64 ceil(rows / 64).  "Role F" of a
 * [rows][cols] matrix contracts over its columns (x in z = x W^T; d z in d x = d z W), "role S" over its rows
 * (d z and x in d W = d z^T x; W in d x = d z W).  Buffers are dfm_planes_bytes(rows, contraction) bytes and must be
 * ZERO-FILLED once by the caller (pads are never written and must read as zero). */
size_t dfm_planes_bytes(int64_t rows, int64_t contraction);
int dfm_tower_x6_supported(int64_t batch, int out_features, int in_features);   /* batch % 64, features % 8 */
typedef struct {
  const float* src;        /* [rows][cols] row-major, 16-byte aligned, cols % 4 == 0 */
  int64_t rows, cols;
  void* planes_f;          /* role F: dfm_planes_bytes(rows, cols); cols % 8 == 0; or NULL */
  void* planes_s;          /* role S: dfm_planes_bytes(cols, rows); rows % 8 == 0; or NULL */
} dfm_split_job;
/* Up to 8 matrices in one launch (the tower's weights, once per step after the optimizer). */
int dfm_split_planes(const dfm_split_job* jobs, int count, dfm_stream_t stream);
/* dfm_linear_bn_forward on planes: x either fp32 (d_x, split by the kernel: the first layer's input) or role-F planes
 * of (batch, in_features); W as role-F planes of (out_features, in_features).  Same workspace and statistics. */
int dfm_linear_bn_forward_x6(const float* d_x, int64_t ldx, const void* d_x_planes_f, const void* d_w_planes_f,
                             const float* d_bias, int64_t batch, int out_features, int in_features, float* d_z,
                             void* d_workspace, dfm_stream_t stream);
/* dfm_bn_relu_dropout_apply / dfm_bn_backward_apply that also (d_out / d_dz may be NULL: only) write their result as
 * planes: role F of (batch, features) and role S = planes of (features, batch).  batch % 32 == 0, features % 8 == 0. */
int dfm_bn_relu_dropout_apply_planes(const float* d_z, int64_t batch, int features, const void* d_workspace,
                                     const float* d_gamma, const float* d_beta, float* d_mean_rstd,
                                     float* d_running_mean, float* d_running_var, int64_t* d_num_batches,
                                     float momentum, float eps, float p_drop, const int64_t* d_seed, int salt,
                                     float* d_out, void* d_planes_f, void* d_planes_s, dfm_stream_t stream);
int dfm_bn_backward_apply_planes(const dfm_bn_bwd* bn, int64_t batch, int features, const dfm_head_tail* head,
                                 float* d_dz, void* d_planes_f, void* d_planes_s, dfm_stream_t stream);
/* dfm_linear_backward (both parts) on planes: d z in both roles, x as role-S planes of (in_features, batch) or fp32
 * (d_x, the first layer), W as role-S planes of (in_features, out_features).  Its own batch split:
 * dfm_linear_backward_x6_splits slabs in a workspace of dfm_linear_backward_x6_workspace_bytes (pass the split count
 * in dfm_slab_ref.splits). */
int dfm_linear_backward_x6_splits(int64_t batch, int out_features, int in_features);
size_t dfm_linear_backward_x6_workspace_bytes(int64_t batch, int out_features, int in_features);
int dfm_linear_backward_x6(const void* d_dz_planes_f, const void* d_dz_planes_s, int64_t batch, int out_features,
                           const float* d_x, const void* d_x_planes_s, int in_features, const void* d_w_planes_s,
                           float* d_g_x, const dfm_bn_bwd* bn_below, const dfm_fm_bwd* fm, void* d_workspace,
                           dfm_stream_t stream);

int dfm_linear_backward_splits(int64_t batch, int out_features, int in_features);

/* ---------------------------------------------------------------------------------
 * Grouped launches for the tail of the training step (csrc/step_tail.hip): kernels of the step that
 * do not depend on each other share one dispatch.  dfm_step_embedding_backward has the same arithmetic
 * and reduction order as the stand-alone entry points it combines (bit-identical results).
 * ------------------------------------------------------------------------------- */
/* dfm_embedding_backward_dense_fields + dfm_rowgrad_build for a uniform plan in one launch.
 * d_dense_list: device array with the schema positions of the num_dense DENSE fields; dense_x and
 * dense_grads: host arrays indexed by schema position (as dfm_embedding_forward's inputs and
 * dfm_field_grad[]); the remaining arguments as in dfm_rowgrad_build. */
int dfm_step_embedding_backward(const int32_t* d_dense_list, int num_dense, const void* const* dense_x,
                                const dfm_field_grad* dense_grads, const int32_t* field_of_sparse,
                                int num_sparse, int num_fields, int dim, int64_t batch,
                                const float* d_g_first, const float* d_g_field,
                                const int32_t* d_sorted_pos, int32_t* d_seg_start,
                                const int32_t* d_num_uniq, float* d_row_g2, float* d_row_g1,
                                float* d_dense_partials, int dense_parts, const float* d_dense_grad_base,
                                int64_t dense_grad_elems, dfm_stream_t stream);
/* d_dense_partials (optional): instead of adding into the dense_grads buffers, the DENSE-field gradients are
 * computed over dense_parts batch slices (dense_parts x as many workgroups: the single-slice form is a
 * latency chain over the whole batch on 65 workgroups) and slice p's values are STORED at
 * d_dense_partials[p * dense_grad_elems + (address of the element - d_dense_grad_base)]; every dense_grads
 * buffer must lie inside [d_dense_grad_base, + dense_grad_elems).  The slices are added by whoever consumes
 * the dfm_slab_ref {d_dense_partials, d_dense_grad_base, 1, 1, dense_grad_elems, dense_parts}. */
/* The first launch of the optimizer tail (dfm_step_prepare -> dfm_grad_norm_finalize -> dfm_step_apply):
 * the ownership merge of the row lists (the dfm_table comment above) and, on the dense buffer,
 * g[i] += 2*l2*p[i] for i < n_l2 (the embedding parameters come first in the buffer), both with
 * one partial sum of |g|^2 per workgroup, in one launch; `slabs` (optional) are dfm_linear_backward
 * workspaces whose batch-split products are added into their d_g views first (replaces
 * dfm_linear_backward_finish).  d_partials: dfm_step_prepare_num_partials floats, to be summed by
 * dfm_grad_norm_finalize.  d_match (optional, dfm_step_match_bytes): with three or more lists the
 * memberships of every row in the other lists are resolved first by one extra launch through LDS
 * (the merge then does byte reads instead of num_lists - 1 global binary searches per row).
 * d_dense_gathered (optional, data parallel): (world, n) — every rank's dense gradient buffer from
 * the step's exchange, rank r's at d_dense_gathered + r * gathered_stride floats (0 = n: contiguous);
 * d_g is then REPLACED by grad_scale * their sum in rank order (an all-reduce with a fixed summation
 * order and no launch of its own).  dense_partial_offset: where in d_partials the dense buffer's partials
 * start (0 = right behind the dfm_rowadam_num_partials row partials; field-sharded tables pad the row part
 * to the same length on every rank so that it can be all-gathered). */
int64_t dfm_step_prepare_num_partials(int num_sparse, int dim, int num_lists, int64_t n);
size_t dfm_step_match_bytes(int num_sparse, int num_lists);
int dfm_step_prepare(const dfm_table* tables, int num_sparse, int dim, int num_lists,
                     const int32_t* d_uniq_rows, const int32_t* d_num_uniq, float* d_row_g2,
                     float* d_row_g1, int32_t* d_owner_flag, float grad_scale, float l2, float* d_g,
                     const float* d_p, int64_t n, int64_t n_l2, const dfm_slab_ref* slabs, int num_slabs,
                     const float* d_dense_gathered, int world, int64_t gathered_stride, float* d_partials,
                     int64_t dense_partial_offset, void* d_match, dfm_stream_t stream);
/* The optimizer of a model WITHOUT row-wise tables (every parameter, embedding tables included, lives in the flat
 * buffer): the dense halves of dfm_step_prepare and dfm_step_apply as launches of their own, same bodies, same
 * arithmetic.  prepare: g += slabs (in slab order), g[i] += 2 * l2 * p[i] for i < n_l2, one |g|^2 partial per
 * workgroup (dfm_step_dense_num_partials(n) floats, summed by dfm_grad_norm_finalize); apply: the update rule on
 * all n elements, zero_grad != 0 also clears g. */
int64_t dfm_step_dense_num_partials(int64_t n);
int dfm_step_dense_prepare(float l2, float* d_g, const float* d_p, int64_t n, int64_t n_l2, const dfm_slab_ref* slabs,
                           int num_slabs, float* d_partials, dfm_stream_t stream);
int dfm_step_dense_apply(const float* d_clip_coef, const dfm_optim* opt, const int32_t* d_step, float* d_p, float* d_m,
                         float* d_v, float* d_g, int64_t n, int zero_grad, dfm_stream_t stream);

/* trainer.py:221-239 without a host read per step (csrc/loss.hip):
 *   d_acc[0] += (double)*d_loss + (double)l2 * sum_{i < n_l2} (double)d_p[i]^2      (loss + get_l2_reg_loss, base.py:78-83)
 *   d_acc[1] += 1                                                                    (batches)
 *   d_acc[2] += (double)*d_loss                                                      (BCE alone)
 * n_l2 == 0 or l2 == 0: no parameter is read.  One launch of one workgroup at every n_l2, double arithmetic
 * throughout, a fixed order of additions (no atomics, no arrival counter): bitwise reproducible.  d_p 16-byte aligned
 * is read with 16-byte loads; any other alignment works, element by element.  Enqueue it between the launch that
 * writes *d_loss and the optimizer's update, so that d_p holds the parameters the forward saw. */
int dfm_loss_accumulate(const float* d_loss, float l2, const float* d_p, int64_t n_l2, double* d_acc, dfm_stream_t stream);

/* The same loss when the SPARSE tables are row tables (dfm_table), which get_l2_reg_loss covers in full (base.py:78-83)
 * and no step can re-sum: S = sum over every element of every w2 / w1 of w^2 is carried in one double on the device.
 *
 * dfm_tables_sqnorm: *d_out = S, one streaming pass (once per epoch).  vocab (HOST, num_sparse): rows per table; row
 * strides as in dfm_table (packed tables work).  The tables are laid end to end and workgroup b sums the rows
 * [b * R, (b + 1) * R), R = ceil(rows / dfm_tables_sqnorm_num_partials(rows)), in double, into d_partials[b]; a second
 * launch of one workgroup adds the partials in index order.  Bitwise reproducible.
 *
 * dfm_rows_sqnorm: the sum of w^2 over the entries of a step's row lists that d_owner_flag marks (one entry per
 * distinct row over all lists: the rows dfm_step_apply updates), dim / 4 lanes per row as there; one double per
 * workgroup in d_partials[0 .. n_partials_total), 0 from the workgroups behind the step's own
 * dfm_rowadam_num_partials(num_sparse, dim, num_lists) (which n_partials_total must cover).  The grid depends on
 * (num_sparse, dim, num_lists, n_partials_total) only; d_num_uniq is read on the device.  Enqueue it behind
 * dfm_step_prepare (which writes the flags) and in front of the apply launch into the "old" partials, and behind the
 * apply launch into the "new" ones.
 *
 * dfm_loss_accumulate_tables: dfm_loss_accumulate's one workgroup, which first folds the PREVIOUS step's update,
 *   *d_S = (*d_S + sum_i d_new_partials[i]) - sum_i d_old_partials[i]        (each sum in a fixed order; partials cleared)
 * and then adds
 *   d_acc[0] += (double)*d_loss + (double)l2 * (sum_{i < n_l2} (double)d_p[i]^2 + *d_S),   d_acc[1] += 1,
 *   d_acc[2] += (double)*d_loss.
 * Enqueue it where dfm_loss_accumulate goes: in front of this step's dfm_step_prepare.  No atomics, no arrival counter;
 * every rounding as written (no contraction). */
int64_t dfm_tables_sqnorm_num_partials(int64_t total_rows);
int dfm_tables_sqnorm(const dfm_table* tables, int num_sparse, int dim, const int32_t* vocab, double* d_partials,
                      double* d_out, dfm_stream_t stream);
int dfm_rows_sqnorm(const dfm_table* tables, int num_sparse, int dim, int num_lists, const int32_t* d_uniq_rows,
                    const int32_t* d_num_uniq, const int32_t* d_owner_flag, double* d_partials,
                    int64_t n_partials_total, dfm_stream_t stream);
int dfm_loss_accumulate_tables(const float* d_loss, float l2, const float* d_p, int64_t n_l2, double* d_S,
                               double* d_old_partials, double* d_new_partials, int64_t n_partials, double* d_acc,
                               dfm_stream_t stream);

/* The update rule and device learning rate of a dfm_optim descriptor on the rows the lists own and on the
 * flat dense buffer d_p / d_m / d_v, in one launch; gradients are scaled by *d_clip_coef (NULL = 1).
 * zero_grad != 0 also clears d_g (optimizer.zero_grad() of the next step, trainer.py:219).  For DFM_OPT_SGD,
 * d_v and the tables' v2 / v1 may be NULL. */
int dfm_step_apply(const dfm_table* tables, int num_sparse, int dim, int num_lists,
                   const int32_t* d_uniq_rows, const int32_t* d_num_uniq, const float* d_row_g2,
                   const float* d_row_g1, const int32_t* d_owner_flag, const float* d_clip_coef,
                   const dfm_optim* opt, const int32_t* d_step, float* d_p, float* d_m, float* d_v, float* d_g,
                   int64_t n, int zero_grad, dfm_stream_t stream);
/* dfm_step_apply of step t + dfm_rowplan_build (with its row touch) of step t + 1 in ONE launch: the plan depends on
 * the next batch's ids only (trainer.py:212-217 hands batches over one by one; a graph of several steps knows them
 * all), and sorts on the first workgroups of the optimizer's last launch instead of costing a ~13 us launch of its
 * own at the head of the next step.  d_next_ids: (num_sparse, batch) int64, column s at d_next_ids + s * ids_stride
 * (a batch record); d_vocab (num_sparse) int32 on the device, max_vocab their maximum; d_next_*: the plan buffers of
 * the NEXT step (not the ones this step's lists live in).  Re-pointing (dfm_launch) reads the node's kernel
 * (hipGraphKernelNodeGetParams) and refuses (DFM_ERR_INVALID) a node whose kernel is not the instantiation it would
 * set (a node captured for another rule). */
int dfm_step_apply_plan(const dfm_table* tables, int num_sparse, int dim, int num_lists,
                        const int32_t* d_uniq_rows, const int32_t* d_num_uniq, const float* d_row_g2,
                        const float* d_row_g1, const int32_t* d_owner_flag, const float* d_clip_coef,
                        const dfm_optim* opt, const int32_t* d_step, float* d_p, float* d_m, float* d_v,
                        float* d_g, int64_t n, int zero_grad, const int64_t* d_next_ids, int64_t ids_stride,
                        const int32_t* d_vocab, int max_vocab, int64_t batch, int32_t* d_next_sorted_pos,
                        int32_t* d_next_uniq_rows, int32_t* d_next_seg_start, int32_t* d_next_num_uniq,
                        int32_t* d_error_flag, const dfm_launch* at);

/* ---------------------------------------------------------------------------------
 * Exact-fp32 GEMM on the matrix cores (v_mfma_f32_32x32x2_f32) for the DNN tower's Linear
 * layers (reference dnn.py:45-47):  C[m,n] (+)= sum_k A(m,k) * B(n,k) (+ bias[n]).
 * `*_k_contiguous` = 1: element (r,k) at base[r*ld + k];  0: at base[k*ld + r].  Forward
 * (x W^T + b), d input (dz W) and d weight (dz^T x, accumulate = 1) of nn.Linear are this one
 * entry point without transposed copies.  d_workspace (dfm_gemm_workspace_bytes) enables a
 * split reduction with fixed-order slab summation for small outputs with a long k (d weight).
 * ------------------------------------------------------------------------------- */
size_t dfm_gemm_workspace_bytes(int m, int n, int k);
int dfm_gemm_f32(const float* d_a, int64_t lda, int a_k_contiguous, const float* d_b, int64_t ldb,
                 int b_k_contiguous, float* d_c, int64_t ldc, int m, int n, int k,
                 const float* d_bias, int accumulate, void* d_workspace, dfm_stream_t stream);
/* Which kernel dfm_gemm_f32 runs such a product on, and how many k splits it launches: host arithmetic only, the
 * same functions dfm_gemm_f32 decides with.  The pointers are inspected for their alignment and never read;
 * has_bias / has_workspace say whether d_bias / d_workspace would be non-NULL.  Routes: the 64 x 64 tiled kernel with
 * guarded element-wise loads (SLOW) or 16-byte loads (FAST: both operands 16-byte aligned with ld % 4 == 0 and a
 * vectorised extent that is a multiple of 4), the rows kernel (A K-contiguous, m >= 8192, (n, k) one of its
 * instantiations, 16-byte aligned rows) and the streamed weight gradient (both operands K-strided, no bias, a
 * workspace, dfm_weight_grad_workspace_bytes(k, m, n) != 0).  dfm_gemm_route returns -1 and dfm_gemm_splits 0 for a
 * shape that is not positive; the split count of the tiled routes is 1 without a workspace. */
#define DFM_GEMM_ROUTE_TILED_SLOW 0
#define DFM_GEMM_ROUTE_TILED_FAST 1
#define DFM_GEMM_ROUTE_ROWS 2
#define DFM_GEMM_ROUTE_WGRAD 3
int dfm_gemm_route(const float* a, int64_t lda, int a_k_contiguous, const float* b, int64_t ldb, int b_k_contiguous,
                   int m, int n, int k, int has_bias, int has_workspace);
int dfm_gemm_splits(int m, int n, int k, int has_workspace);

/* Weight and bias gradient of an nn.Linear over many rows (the attention projections W_q|W_k|W_v and
 * W_out, attention.py:95-97, :115; rows = B*F):  dW[n1,n2] (+)= sum_r g[r,n1] * x[r,n2],
 * db[n1] (+)= sum_r g[r,n1] (d_db may be NULL).  Both operands are streamed once, per-workgroup
 * partials are summed in a fixed order (bitwise reproducible).  Shapes: n1, n2 multiples of 32 with
 * (n1/32, n2/32) in {(6,1),(3,1),(2,1),(1,1),(1,2),(2,2),(1,3)} and rows >= 8192 — otherwise
 * dfm_weight_grad_workspace_bytes returns 0 and the call DFM_ERR_UNSUPPORTED (use dfm_gemm_f32).
 * dfm_gemm_f32 itself routes these shapes (and the many-rows x tiny-weight products
 * C = A W^T with n*k <= 6144) to the same kernels (csrc/gemm_skinny.hip). */
size_t dfm_weight_grad_workspace_bytes(int64_t rows, int n1, int n2);
int dfm_weight_grad_f32(const float* d_g, int64_t ldg, const float* d_x, int64_t ldx, int64_t rows, int n1,
                        int n2, float* d_dw, int64_t lddw, float* d_db, int accumulate, void* d_workspace,
                        dfm_stream_t stream);
/* Deferred finish: dfm_weight_grad_partials_f32 runs the streamed pass only and leaves
 * dfm_weight_grad_partial_blocks(rows) partial rows of n1 * n2 + n1 floats in the workspace; dfm_layernorm_backward
 * with d_g_gamma == d_g_beta == NULL leaves dfm_layernorm_partial_blocks(rows) partial planes [2][dim] in its
 * workspace.  dfm_partials_finish then adds up to 8 such sets in ONE launch (same fixed order as the stand-alone
 * finishes: bit-identical) — an attention block's backward (attention.py:91-120 under autograd) ends in one
 * reduction launch instead of three. */
int dfm_weight_grad_partial_blocks(int64_t rows);
int dfm_weight_grad_partials_f32(const float* d_g, int64_t ldg, const float* d_x, int64_t ldx, int64_t rows, int n1,
                                 int n2, void* d_workspace, dfm_stream_t stream);
/* Two such passes over the same rows in one launch (an attention block's dW_qkv and dW_out); DFM_ERR_UNSUPPORTED when
 * the pair of shapes has no joint kernel ((192, 32) + (32, 64) has one) — make the two calls then. */
int dfm_weight_grad_partials_pair_f32(const float* d_g_a, int64_t ldg_a, const float* d_x_a, int64_t ldx_a, int n1_a,
                                      int n2_a, void* d_workspace_a, const float* d_g_b, int64_t ldg_b,
                                      const float* d_x_b, int64_t ldx_b, int n1_b, int n2_b, void* d_workspace_b,
                                      int64_t rows, dfm_stream_t stream);
int dfm_layernorm_partial_blocks(int64_t rows);
typedef struct {
  int32_t kind;            /* 0: weight gradient partials -> out_w = dW (row stride ldw), out_b = db or NULL;
                            * 1: LayerNorm partials -> out_w = d gamma, out_b = d beta (always accumulated into) */
  int32_t blocks;          /* partial rows */
  int32_t n1, n2;          /* kind 0: dW is n1 x n2; kind 1: n1 = dim */
  int32_t accumulate;      /* kind 0: 0 store, 1 add */
  int32_t reserved;
  const float* partial;
  float* out_w;
  float* out_b;
  int64_t ldw;
} dfm_partial_job;
int dfm_partials_finish(const dfm_partial_job* jobs, int count, dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Field-sharded embedding tables under data parallelism (csrc/shard.hip).  The reference trains on one
 * device (deepfm/training/trainer.py:47-56), so nothing of it is replaced here: these are the device
 * halves of this build's N-GPU step — rank r owns the tables of a contiguous block of
 * SPARSE fields, serves their rows to every rank's batch and receives the gradients back; three
 * all-to-alls per step (ids, rows, gradients) carry plain contiguous buffers:
 *   ids   segment for owner q : the batch's ids of q's fields               (nf_q, batch) int64
 *   rows  segment for rank p  : [e (batch, nf_r, dim) | first-order w (batch, nf_r)]
 *   grads segment for owner q : [d e (batch, nf_q, dim) | d first (batch) | dense gradients (n_dense)]
 * ------------------------------------------------------------------------------- */
/* Copy of a batch record into the step's static inputs as a kernel of its own (the first node of a
 * captured step, re-pointed at another record before each replay). */
int dfm_stage_record(const void* d_src, void* d_dst, int64_t nbytes, const dfm_launch* at);
/* Owner side, forward: d_ids (world, num_owned, batch) as received -> d_send (world segments of
 * batch * num_owned * (dim + 1) floats, layout above) and d_gids (num_owned, world * batch): the same
 * ids field-major, the input of dfm_rowplan_build over the global batch.  tables[j] / vocab[j]: the
 * owned tables in field order (Adam state pointers unused).  Out-of-range ids: row 0 + *d_error_flag |= 1. */
int dfm_shard_gather(const dfm_table* tables, const int32_t* vocab, int num_owned, int dim, int world,
                     int64_t batch, const int64_t* d_ids, float* d_send, int64_t* d_gids,
                     int32_t* d_error_flag, dfm_stream_t stream);
/* Batch side, backward: length in floats of one gradient segment, and the kernel that fills all of
 * them: first_field[q] / field_count[q] = rank q's block of SPARSE fields (indices into
 * field_of_sparse, which maps a SPARSE field to its schema position in d_g_field (batch, num_fields, dim)).
 * `slabs` (optional, as in dfm_step_prepare): dfm_linear_backward workspaces whose batch-split products are
 * added to their weights' part of the dense segment on the way (d_dense itself is not modified). */
int64_t dfm_shard_pack_segment(int64_t batch, int num_owned, int dim, int64_t n_dense);
int dfm_shard_pack(const int32_t* first_field, const int32_t* field_count, int world,
                   const int32_t* field_of_sparse, int num_sparse, int num_fields, int dim, int64_t batch,
                   const float* d_g_field, const float* d_g_first, const float* d_dense, int64_t n_dense,
                   const dfm_slab_ref* slabs, int num_slabs, float* d_send, dfm_stream_t stream);
/* Owner side, backward: dfm_rowgrad_build over the received gradient segments (d_recv: world segments
 * of `segment` floats each, source-rank major; sample p * batch + b of the row plan is sample b of
 * segment p). */
int dfm_shard_rowgrad(int num_owned, int dim, int world, int64_t batch, const float* d_recv, int64_t segment,
                      const int32_t* d_sorted_pos, int32_t* d_seg_start, const int32_t* d_num_uniq,
                      float* d_row_g2, float* d_row_g1, dfm_stream_t stream);
/* *d_out = x[0] + ... + x[n-1] in a fixed order (one workgroup): a rank's share of |g|^2. */
int dfm_sum_floats(const float* d_x, int64_t n, float* d_out, dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Eval-mode forward and evaluation metrics (csrc/predict.hip): reference trainer.py:244-294
 * (model.eval(); model.predict(batch) per batch; compute_auc / compute_logloss of metrics.py:9-18).
 * In eval mode BatchNorm uses its running statistics and dropout is the identity (dnn.py:45-55).
 * ------------------------------------------------------------------------------- */
/* One tower layer, eval mode: out (batch, out_features) =
 *   relu(gamma * ((x W^T + b - running_mean) * rsqrt(running_var + eps)) + beta)
 * on the exact-fp32 MFMA GEMM of dfm_linear_bn_forward.  x rows at stride ldx; d_bias may be NULL.  Nothing
 * but `out` is written (no z, no statistics, running statistics untouched). */
int dfm_linear_bn_eval(const float* d_x, int64_t ldx, const float* d_w, const float* d_bias, int64_t batch,
                       int out_features, int in_features, const float* d_gamma, const float* d_beta,
                       const float* d_running_mean, const float* d_running_var, float eps, float* d_out,
                       dfm_stream_t stream);
/* Eval head (deepfm.py:30-42, xdeepfm.py:36-48): logit = (first_order + extra) + (a . w + b), prob = sigmoid(logit)
 * for the rows b < valid only (a padded batch writes nothing past them).  a (batch, features), features % 4 == 0,
 * a and w 16-byte aligned; d_first_order / d_extra / d_b / d_logits may be NULL.  Re-pointed per batch for its
 * outputs and valid count. */
int dfm_predict_head(const float* d_a, int64_t batch, int features, const float* d_w, const float* d_b,
                     const float* d_first_order, const float* d_extra, int64_t valid, float* d_logits, float* d_probs,
                     const dfm_launch* at);
/* AUC and log loss of n (label, score) pairs, deterministic.  dfm_metrics_prepare zeroes the counters in the
 * workspace (dfm_metrics_workspace_bytes(n), 16-byte aligned), sums per-sample log loss in fp64 (scores clipped to
 * [1e-7, 1 - 1e-7] in fp32, then sklearn's log_loss of float32 input) and writes the sort keys d_keys (n): the score
 * of a negative (label <= 0.5), +inf for a positive.  The caller sorts the keys ascending; dfm_metrics_finish counts
 * 2 #(neg < s) + #(neg == s) over the positives in int64 (Mann-Whitney, ties 1/2) and writes
 * d_out[5] = {auc (NaN if a class is empty), logloss, npos, nneg, number of NaN scores}. */
size_t dfm_metrics_workspace_bytes(int64_t n);
int dfm_metrics_prepare(const float* d_labels, const float* d_scores, int64_t n, float* d_keys, void* d_workspace,
                        dfm_stream_t stream);
int dfm_metrics_finish(const float* d_labels, const float* d_scores, int64_t n, const float* d_sorted_keys,
                       void* d_workspace, double* d_out, dfm_stream_t stream);
/* Leave-one-out ranking metrics (csrc/ranking.hip; reference trainer.py:296-332 and RankingEvaluator.evaluate,
 * metrics.py:62-111) of n samples grouped by d_user_ids (int64, each in [0, num_users)), deterministic.  Per user,
 * rank = the 0-based position of its first positive (label 1) in the stable descending order of its scores (ties
 * in dataset order; -0 == +0); a user counts when it has both classes (require_both_classes != 0: the trainer's
 * filter) or any sample (0: RankingEvaluator, a user without a positive is a miss).  For the h_ks[num_ks] cut-offs
 * (host array, 1 <= num_ks <= 8, every k >= 1) it writes the fp64
 *   d_out[1 + 2 num_ks + 3] = {users, HR@k..., NDCG@k..., bad ids, NaN scores, labels other than 0 / 1}
 * with HR@k = hits / users and NDCG@k = sum(1 / log2(rank + 2) : rank < k) / users (both 0 without users); results
 * are meaningless unless the three counts are 0.  1 <= n < 2^32.  d_workspace: dfm_ranking_workspace_bytes(n,
 * num_users) bytes, 16-byte aligned, cleared by the call itself. */
size_t dfm_ranking_workspace_bytes(int64_t n, int64_t num_users);
int dfm_ranking_metrics(const int64_t* d_user_ids, const float* d_labels, const float* d_scores, int64_t n,
                        int64_t num_users, const int32_t* h_ks, int num_ks, int require_both_classes,
                        void* d_workspace, double* d_out, dfm_stream_t stream);
/* dfm_ranking_user_ranks: the per-user integers behind dfm_ranking_metrics, from the same two per-sample passes and the same workspace
 * (dfm_ranking_workspace_bytes): d_rank[num_users] (int64) = the user's rank (>= 0) when it counts and has a positive,
 * DFM_RANK_NOT_COUNTED for a user that does not count (no sample, or one class only with require_both_classes != 0),
 * DFM_RANK_MISS for a user that counts without a positive (possible only with require_both_classes == 0).  The ranks and
 * the counted users are exactly those dfm_ranking_metrics uses: HR@k = #{rank in [0, k)} / #{counted}.  It writes the
 * fp64 d_out[4] = {users counted, bad ids, NaN scores, labels other than 0 / 1}. */
#define DFM_RANK_NOT_COUNTED (-1)
#define DFM_RANK_MISS (-2)
int dfm_ranking_user_ranks(const int64_t* d_user_ids, const float* d_labels, const float* d_scores, int64_t n,
                           int64_t num_users, int require_both_classes, void* d_workspace, int64_t* d_rank,
                           double* d_out, dfm_stream_t stream);
/* Grouped AUC (csrc/grouped_auc.hip) of n samples grouped by d_group_ids (int64, each in [0, num_groups)),
 * deterministic and independent of the order of the samples.  For a group g with P_g labels 1 and N_g labels 0 (it
 * qualifies when both are > 0), W_g / T_g its (positive, negative) pairs with s_pos > s_neg / s_pos == s_neg (float32
 * order, -0 == +0):
 *   auc_g = double(2 W_g + T_g) / double(2 P_g N_g)             (unsigned 64-bit integers)
 *   gauc  = sum (P_g + N_g) auc_g / sum (P_g + N_g),  uauc = mean auc_g       over the qualifying groups, fp64 sums
 *           in a fixed tree over the group ids (grouped_auc.hip)
 * dfm_grouped_auc_prepare clears the three counts in the workspace and writes d_keys_out (n) =
 * group << 33 | label << 32 | order bits of the score, INT64_MAX for a sample with an id outside [0, num_groups), a NaN
 * score or a label other than 0 / 1 (each counted, none used).  The caller sorts the keys ascending (values only);
 * dfm_grouped_auc_finish takes the sorted keys and writes the fp64
 *   d_out[7] = {qualifying groups, gauc, uauc, samples in qualifying groups, bad ids, NaN scores, bad labels}
 * (gauc and uauc NaN when no group qualifies) and, when d_group_auc is not NULL, d_group_auc[num_groups] = auc_g, NaN
 * for a group that does not qualify.  1 <= n < 2^31, 1 <= num_groups <= 2^30.  d_workspace:
 * dfm_grouped_auc_workspace_bytes(n, num_groups) bytes (0 for arguments that are not positive), 16-byte aligned, the
 * same buffer for both calls. */
size_t dfm_grouped_auc_workspace_bytes(int64_t n, int64_t num_groups);
int dfm_grouped_auc_prepare(const int64_t* d_group_ids, const float* d_labels, const float* d_scores, int64_t n,
                            int64_t num_groups, int64_t* d_keys_out, void* d_workspace, dfm_stream_t stream);
int dfm_grouped_auc_finish(const int64_t* d_sorted_keys, int64_t n, int64_t num_groups, void* d_workspace,
                           double* d_group_auc, double* d_out, dfm_stream_t stream);
/* dfm_grouped_auc_unit_columns: the per-group integers behind gauc / uauc as columns for dfm_bootstrap_units
 * (csrc/bootstrap_units.hip).  It takes the sorted keys as
 * dfm_grouped_auc_finish does (after dfm_grouped_auc_prepare and the sort, the same workspace; it forms the groups'
 * runs and numerators itself, so it may run before, after or without dfm_grouped_auc_finish) and writes
 *   d_cols[4][num_groups] = {qual, qual * q_g, qual * size_g, qual * size_g * q_g}              (uint64, column-major)
 * with qual = 1 for a qualifying group and 0 otherwise, size_g = P_g + N_g and q_g = llrint(auc_g * 2^30), auc_g the
 * double dfm_grouped_auc_finish forms.  For n <= 2^26 every weighted sum of a column stays below 12 * 2^26 * 2^30. */
int dfm_grouped_auc_unit_columns(const int64_t* d_sorted_keys, int64_t n, int64_t num_groups, void* d_workspace,
                                 uint64_t* d_cols, dfm_stream_t stream);
/* Calibration (csrc/calibration.hip) of n samples: float32 labels, float32 probabilities and, with num_slices > 0,
 * int64 slice ids in [0, num_slices); deterministic and independent of the order of the samples.  A sample is used
 * unless its slice id is outside [0, num_slices), its score is NaN, its score is outside [0, 1] (-0 is inside) or its
 * label is other than exactly 0 or 1; each of the four is counted, and a sample with any of them enters nothing else.
 * For a used sample with score p and label y (K = num_bins):
 *   bin = min(K - 1, (int)(p * (float)K))   (float32 product; p == 1 is in the last bin)
 *   P = llrint((double)p * 2^32),  Q = llrint(((double)p - y)^2 * 2^32),  L = llrint(l * 2^27), l the per-sample
 *   log loss of dfm_metrics_prepare (score clipped to [1e-7, 1 - 1e-7] in fp32, fp64 logarithm)
 * All sums are 64-bit integer sums (none can overflow for n < 2^31): N, positives, sum P, sum Q, sum L over all used
 * samples; count, positives, sum P per bin; count, positives, sum P, sum L per slice.  The finish forms, in fp64:
 *   d_bins[num_bins][3]     = {count, positives, sum P_b * 2^-32}
 *   d_slices[num_slices][4] = {count, positives, sum P_s * 2^-32, sum L_s * 2^-27}
 *   gap_b = fabs(sum P_b * 2^-32 - positives_b);  ece = (gap_0 + gap_1 + ..., ascending b, one by one) / N;
 *   mce = max over the non-empty bins of gap_b / count_b
 *   d_out[12] = {N, positives, sum P * 2^-32 / N (mean prediction), sum Q * 2^-32 / N (Brier score),
 *                sum L * 2^-27 / N (log loss), ece, mce, bad slice ids, NaN scores, scores outside [0, 1],
 *                labels other than 0 / 1, 0}                    (the five ratios NaN when N == 0)
 * 1 <= n < 2^31, 1 <= num_bins <= 1024, 0 <= num_slices <= 2^24; d_slice_ids and d_slices are NULL exactly when
 * num_slices == 0.  d_workspace: dfm_calibration_workspace_bytes(num_bins, num_slices) bytes (0 for sizes outside
 * these limits), 16-byte aligned, cleared by the call itself.  dfm_calibration_route is 0 when the bin and slice tables
 * of a workgroup are both kept in LDS ((3 num_bins + 4 num_slices) * 8 bytes within 48 KiB), 1 when the slice sums go
 * to global memory with integer atomics per sample (the bins stay in LDS), -1 for sizes outside the limits. */
size_t dfm_calibration_workspace_bytes(int num_bins, int64_t num_slices);
int dfm_calibration_route(int num_bins, int64_t num_slices);
int dfm_calibration(const float* d_labels, const float* d_scores, const int64_t* d_slice_ids, int64_t n, int num_bins,
                    int64_t num_slices, void* d_workspace, double* d_bins, double* d_slices, double* d_out,
                    dfm_stream_t stream);
/* Poisson bootstrap (csrc/bootstrap.hip) of the pooled AUC and log loss of n samples (float32 labels and scores):
 * `replicates` integer re-weightings of the samples, or of whole units when d_unit_ids (int64) is not NULL (without
 * it the unit of sample i is i); exact in integers, deterministic, and with unit ids independent of the order of the
 * samples.  A sample is used when its score is not NaN, its label is exactly 0 or 1 and its unit id lies in [0, 2^40);
 * each of the three failures is counted on its own and a sample with any of them enters nothing else.
 * Weight of unit u in replicate r (wrapping uint64 arithmetic; mix32 is the counter hash of csrc/dropout.h):
 *   h = mix32(seed * 0x9E3779B97F4A7C15 + 0x426F6F7453747261 + (r << 40) + u)
 *   w = number of k in 0..11 with h >= T[k],  T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!) =
 *       {1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291,
 *        4294609777, 4294923276, 4294962463, 4294966817, 4294967252, 4294967292}
 * i.e. Poisson(1) truncated at 12, a function of (seed, r, unit) only: two calls with one seed resample identically.
 * Per replicate, over the used samples, a sample weighing its unit's w (float32 score order, -0 == +0):
 *   P = sum of w over y = 1,  N = sum of w over y = 0,  S = P + N
 *   U = sum over (y_i = 1, y_j = 0) of w_i w_j (2 [s_i > s_j] + [s_i == s_j])
 *   L = sum of w_i * llrint(l_i * 2^27),  l_i the per-sample log loss of dfm_metrics_prepare (dfm_calibration's L)
 *   d_counts[replicates][5] = {U, P, N, L, S}                     (unsigned 64-bit integers; none can overflow)
 *   d_out[replicates][2]    = {double(U) / double(2 P N)          (NaN when P N == 0),
 *                              double(L) * 2^-27 / double(S)}     (NaN when S == 0)
 *   d_faults[3]             = {NaN scores, labels other than 0 / 1, unit ids outside [0, 2^40)}
 * dfm_bootstrap_prepare clears and fills the three counts and the log-loss terms in the workspace and writes two key
 * vectors (n each): ord(score) << 27 | tiebit << 26 | i, with tiebit the label in d_keys_neg_first (tied scores: the
 * negatives in front) and its complement in d_keys_pos_first, INT64_MAX for a sample that is not used.  The caller
 * sorts both ascending (values only); dfm_bootstrap_replicates takes the sorted vectors and the same unit ids.  With
 * A = sum over the positives of w_i * (weight of the negatives in front of i) in one order, U = A_neg_first +
 * A_pos_first.  A workgroup takes DFM_BOOTSTRAP_CHUNK consecutive sorted samples for DFM_BOOTSTRAP_REPLICATE_BLOCK
 * replicates; the launches (six) do not depend on n, and on the replicates only through the grid.
 * 1 <= n <= 2^DFM_BOOTSTRAP_MAX_LOG2_N, 1 <= replicates <= DFM_BOOTSTRAP_MAX_REPLICATES.  d_workspace:
 * dfm_bootstrap_workspace_bytes(n, replicates) bytes (0 outside these limits; a multiple of 16, monotone in both),
 * 16-byte aligned, the same buffer for both calls (prepare needs no more than the bytes of replicates = 1). */
#define DFM_BOOTSTRAP_CHUNK 2048
#define DFM_BOOTSTRAP_REPLICATE_BLOCK 16
#define DFM_BOOTSTRAP_MAX_LOG2_N 26
#define DFM_BOOTSTRAP_MAX_REPLICATES 65536
size_t dfm_bootstrap_workspace_bytes(int64_t n, int replicates);
int dfm_bootstrap_prepare(const float* d_labels, const float* d_scores, const int64_t* d_unit_ids, int64_t n,
                          int64_t* d_keys_neg_first, int64_t* d_keys_pos_first, void* d_workspace,
                          dfm_stream_t stream);
int dfm_bootstrap_replicates(const int64_t* d_sorted_neg_first, const int64_t* d_sorted_pos_first,
                             const int64_t* d_unit_ids, int64_t n, int replicates, uint64_t seed, void* d_workspace,
                             uint64_t* d_counts, double* d_out, uint64_t* d_faults, dfm_stream_t stream);
/* The same bootstrap for metrics that are means over units (users): HR@k, NDCG@k, gauc, uauc (csrc/bootstrap_units.hip).
 * Each is a quotient of two sums of per-unit integers, so a replicate is a quotient of two weighted column sums.
 * dfm_bootstrap_units takes d_cols (num_cols, num_units) uint64, every column contiguous, and writes
 *   d_sums[replicates][num_cols] = sum over the units u of w(seed, r, u) * d_cols[m][u]
 * in wrapping unsigned 64-bit arithmetic (exact mod 2^64), w the weight above with the unit's index as u: with user ids
 * as units it weighs user u as dfm_bootstrap_replicates does under the same seed.  A workgroup takes
 * DFM_BOOTSTRAP_UNITS_CHUNK consecutive units for DFM_BOOTSTRAP_REPLICATE_BLOCK replicates, reads the chunk's columns
 * once (16-byte loads where a column is 16-byte aligned; d_cols itself need only be 8-byte aligned) and adds one
 * 64-bit integer atomic per (workgroup, replicate, column) into one of at most 16 copies of the sums in the workspace;
 * a second launch adds the copies up.  Three launches whatever num_units is; integer sums, so the results do not depend
 * on the launch geometry or the order of the atomics.  1 <= num_units <= 2^30, 1 <= num_cols <=
 * DFM_BOOTSTRAP_UNITS_MAX_COLS, 1 <= replicates <= DFM_BOOTSTRAP_MAX_REPLICATES.  d_workspace:
 * dfm_bootstrap_units_workspace_bytes(num_units, num_cols, replicates) bytes (0 outside these limits; a multiple of 16,
 * monotone in all three), 16-byte aligned, cleared by the call itself.
 *
 * dfm_bootstrap_rank_columns writes the columns of HR@k / NDCG@k from the ranks of dfm_ranking_user_ranks:
 *   d_cols[1 + 2 num_ks][num_users] = {counted, [rank < k_j] (num_ks), rank < k_j ? d_gain[rank] : 0 (num_ks)}
 * (counted: rank >= 0 or DFM_RANK_MISS; a hit needs rank >= 0) for the h_ks[num_ks] cut-offs (host array, 1 <= num_ks
 * <= 8, 1 <= k <= gain_len).  d_gain[gain_len] (uint64) is the caller's fixed-point gain table, d_gain[i] =
 * llrint(2^30 / log2(i + 2)): the device never evaluates a logarithm.  1 <= num_users <= 2^30.
 * The replicates' values are formed by the caller in fp64 (NaN for a zero denominator):
 *   HR@k_r = sum w hit / sum w counted,   NDCG@k_r = (sum w gain) 2^-30 / sum w counted,
 *   uauc_r = (sum w qual q) 2^-30 / sum w qual,   gauc_r = (sum w qual size q) 2^-30 / sum w qual size */
#define DFM_BOOTSTRAP_UNITS_CHUNK 1024
#define DFM_BOOTSTRAP_UNITS_MAX_COLS 24
size_t dfm_bootstrap_units_workspace_bytes(int64_t num_units, int num_cols, int replicates);
int dfm_bootstrap_units(const uint64_t* d_cols, int64_t num_units, int num_cols, int replicates, uint64_t seed,
                        void* d_workspace, uint64_t* d_sums, dfm_stream_t stream);
int dfm_bootstrap_rank_columns(const int64_t* d_rank, int64_t num_users, const int32_t* h_ks, int num_ks,
                               const uint64_t* d_gain, int64_t gain_len, uint64_t* d_cols, dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * An epoch's input side on the device (csrc/sampler.hip): the reference re-draws its training negatives every
 * epoch on the host (movielens.py:532-565, random.sample over the user's unseen movies per positive) and forms
 * batches in a DataLoader.  Here the positives, an item table and the per-user seen-sets stay on the device.
 * ------------------------------------------------------------------------------- */
/* The candidate list of `num` queries (positives), taken by both draws and by the assemble plan.  NULL is the
 * rectangular list: k entries per query, entry t of query q at [q * k + t] of a (num, k) output.  A struct is the
 * ragged list: the reference draws min(num_neg, unseen) candidates for a user with fewer unseen items than num_neg
 * (movielens.py:575-580 for evaluation, _sample_negatives_for_user for training), so query q owns d_counts[q] <= k
 * entries of one flat (total) int32 output, entry t < d_counts[q] at [d_offsets[q] + t].
 * Draw t of query q uses the counters (seed, epoch, q, t) in either shape, so a query with d_counts[q] == k receives,
 * bit for bit, the k items of the rectangular draw, and a shorter one its first d_counts[q].  The draws check only
 * 0 <= total <= num * k (data/device_epoch.py checks the two arrays on the host); their kernels cut every query to
 * min(d_counts[q], k) entries inside [0, total), so a wrong array cannot make them write outside the list.
 * total == 0 launches nothing, and the output may then be NULL.  The struct is read during the call and need not
 * outlive it; the arrays it names must stay alive until the launch has run (and see dfm_assemble_plan_create). */
typedef struct dfm_candidate_list {
  const int32_t* d_counts;   /* (num) int32, 0 <= d_counts[q] <= k */
  const int64_t* d_offsets;  /* (num + 1) int64, the exclusive scan of d_counts */
  int64_t total;             /* == d_offsets[num]: entries of the flat list */
} dfm_candidate_list;

/* For each of num_pos positives, k distinct item rows its user has not seen, uniform without replacement.
 *   d_seen   (n_users, W) uint32, W = ceil(n_items / 32): bit i of user u set = u has seen item row i; the bits at
 *            and above n_items are set;
 *   d_prefix (n_users, W + 1) uint32: prefix[u][w] = zero bits in words < w, so prefix[u][W] = the unseen count U;
 *   d_user_of (num_pos) int32; d_neg_items (num_pos, k) int32, or the flat output of `list`; 1 <= k <= 16.
 * Draw t of positive p: h = mix32(seed * 0x9E3779B97F4A7C15 + (epoch << 40) + 16 p + t) (wrapping uint64; the
 * hash of csrc/dropout.h), r = (h * (U - t)) >> 32; for every rank q already drawn for p, ascending: r += (r >= q);
 * the item is the r-th zero bit of the user's row (binary search of the prefix, then a select inside the word).
 * Bounded work per draw, no rejection.  Every user named needs U >= its count of draws (the caller checks; a draw
 * that cannot be made, or a user outside [0, n_users), is written as -1 and nothing outside the tables is read);
 * with d_counts[p] = min(k, U) the rank-select over a short user's U rows returns each of them once. */
int dfm_sample_negatives(const uint32_t* d_seen, const uint32_t* d_prefix, const int32_t* d_user_of,
                         int64_t num_pos, int n_users, int n_items, int k, uint64_t seed, uint64_t epoch,
                         const dfm_candidate_list* list, int32_t* d_neg_items, dfm_stream_t stream);

/* The reference's popularity-weighted evaluation negatives (movielens.py:567-604, _add_eval_negatives: random.choices
 * with weights count^alpha over the user's unseen movies, drawn once per split).  For each of num_queries queries,
 * c item rows drawn WITH replacement from the rows its user has not seen, row i with probability
 * w[i] / T, T = the sum of w over the user's unseen rows.
 *   d_seen    as dfm_sample_negatives (no prefix table is needed);
 *   d_weight  (n_items) uint32, every value in [1, 2^24] (data/candidates.py:item_weights): integers make the draw
 *             exact and independent of any summation order;
 *   d_user_of (num_queries) int32; d_items (num_queries, c) int32, or the flat output of `list` (a short user gets
 *             fewer draws; a workgroup whose query has no entry returns at once); 1 <= c <= DFM_MAX_CANDIDATES;
 *             num_queries <= 2^19.
 * Draw t of query p, all wrapping uint64:
 *   x = seed * 0x9E3779B97F4A7C15 + (epoch << 40) + 0xD1B54A32D192ED03 + (p << 21) + 2 t
 *   h = mix32(x) << 32 | mix32(x + 1);   r = (h * T) >> 64   (the high half of the 128-bit product)
 * and the item is the smallest unseen row whose inclusive prefix sum of unseen weights exceeds r.  The constant
 * 0xD1B54A32D192ED03 keeps the stream apart from dfm_sample_negatives' for the same (seed, epoch).  One workgroup per
 * query: per-word (32 rows) sums scanned in LDS as uint64, then per draw a binary search and a walk inside one word;
 * integers only, no atomics, no rejection.  n_items above 2^17 (_lib.WEIGHTED_MAX_ITEMS: 32 KiB of prefixes) is
 * DFM_ERR_UNSUPPORTED.  A user outside [0, n_users) or without an unseen row gets -1 entries; nothing outside the
 * tables is read. */
int dfm_sample_weighted(const uint32_t* d_seen, const int32_t* d_user_of, const uint32_t* d_weight,
                        int64_t num_queries, int n_users, int n_items, int c, uint64_t seed, uint64_t epoch,
                        const dfm_candidate_list* list, int32_t* d_items, dfm_stream_t stream);

/* Batch records from device-resident columns.  An epoch has num_pos * (1 + k) virtual rows: row j < num_pos is
 * positive j (every column from `pos`, label d_labels[j]); row j >= num_pos is negative t = (j - num_pos) % k of
 * positive p = (j - num_pos) / k with item = neg_items[p][t] and label 0, each column filled by its role.
 * 0 <= k <= DFM_MAX_CANDIDATES: a candidate list of any length (only dfm_sample_negatives is held to 16), an item
 * may repeat inside it; num_pos * (1 + k) must fit the int64 row index.
 * With a ragged `list` (dfm_candidate_list; 1 <= k = the largest count, num_pos <= 2^36) the epoch has
 * num_pos + total virtual rows: row j >= num_pos is candidate c = j - num_pos of the flat neg_items (total) and
 * belongs to the query p with d_offsets[p] <= c < d_offsets[p + 1], found by a binary search of one probe per bit of
 * num_pos - 1 (20 for 2^20 queries), the same count for every lane.  Roles, bags, padding and the guards are those
 * of the rectangular plan. */
enum dfm_assemble_role {
  DFM_ROLE_COPY = 0,         /* the value of positive p (user and context fields) */
  DFM_ROLE_ITEM = 1,         /* row `item` of the item table's column */
  DFM_ROLE_BUCKET_DIFF = 2   /* SPARSE only: d = ctx[p] - item_val[item] in float32; b = 0 if either operand is NaN
                                or d < 0, else 1 + #{e in edges : e <= d}; the id is bucket_ids[b] */
};
typedef struct dfm_assemble_column {
  int32_t kind;              /* dfm_field_kind */
  int32_t role;              /* dfm_assemble_role */
  int32_t length;            /* SEQUENCE: max_length */
  int32_t num_edges;         /* BUCKET_DIFF: at most 64 */
  int64_t record_offset;     /* bytes: the field's column in the record (RecordLayout.field_offsets) */
  const void* pos;           /* SPARSE int64 (num_pos), DENSE float (num_pos), SEQUENCE int64 (num_pos, length) */
  const void* item;          /* ITEM: the same types over (n_items[, length]); BUCKET_DIFF: item_val float (n_items) */
  const float* ctx;          /* BUCKET_DIFF: (num_pos) */
  const float* edges;        /* BUCKET_DIFF: (num_edges) */
  const int64_t* bucket_ids; /* BUCKET_DIFF: (num_edges + 2) */
} dfm_assemble_column;
typedef struct dfm_assemble_plan dfm_assemble_plan;
/* Uploads the column descriptors (host array, schema order; device pointers inside) and the launch map of a
 * record of `batch` slots whose block offsets are RecordLayout.of's (checked against id_rows / dense_rows).
 * The arrays of a ragged `list` are read back once here and refused unless 0 <= d_counts[p] <= k and d_offsets is the
 * exclusive scan of d_counts ending in total, so that no launch of the plan can leave neg_items; the plan keeps
 * d_offsets, which must stay alive and unchanged as long as the plan. */
int dfm_assemble_plan_create(const dfm_assemble_column* columns, int num_columns, int64_t batch, int id_rows,
                             int dense_rows, int64_t dense_offset, int64_t labels_offset, int64_t record_bytes,
                             const float* d_labels, int64_t num_pos, int n_items, int k,
                             const dfm_candidate_list* list, dfm_assemble_plan** out_plan);
int dfm_assemble_plan_destroy(dfm_assemble_plan* plan);
/* One launch writes the record's `batch` slots from the virtual rows d_order[first .. first + count) (int64, at
 * least first + count entries; NULL: the identity), count <= batch.  Slots >= count, the padding row of an ids /
 * dense block without a field, and a row d_order names outside the epoch are zeros: what RecordLayout.write
 * leaves.  d_neg_items (num_pos, k) may be NULL when k == 0: the device form of RecordLayout.write_indexed.
 * d_record: 16-byte aligned. */
int dfm_record_assemble(const dfm_assemble_plan* plan, const int64_t* d_order, int64_t first, int64_t count,
                        const int32_t* d_neg_items, void* d_record, dfm_stream_t stream);

/* Full-catalogue selection (csrc/catalogue.hip): the unsampled form of the reference's leave-one-out ranking
 * (trainer.py:296-332 ranks 1 + 999 sampled candidates; the held-out positive is in the seen-set by construction,
 * movielens.py:262-265).  One workgroup per query over d_scores (num_queries, n_items) float32, row-major.
 *   eligible rows of query q: the rows whose bit in d_seen[d_user_of[q]] is clear (every row when exclude_seen == 0;
 *   d_seen may then be NULL), and the target d_target[q] when it is >= 0, seen or not (d_target NULL: no targets);
 *   order: dfm_ranking_metrics' key ord_bits(score) << 32 | (0xFFFFFFFF - row): descending score, ties by ascending
 *   row, -0 == +0.
 * d_out_items / d_out_scores (num_queries, k), 1 <= k <= 128: the first k eligible rows in that order and their scores
 * as stored, padded with -1 / -inf; d_out_rank (num_queries): the eligible rows other than the target that precede
 * it, -1 without a target; d_status[3] uint64, cleared by the call: NaN scores among eligible rows, users outside
 * [0, n_users) (padding and rank -1), targets outside [-1, n_items) (taken as no target).  Results are meaningless
 * unless all three are 0.  A row of up to 6144 scores is read once (keys in LDS); a longer one is re-read by each of
 * the ten passes; n_items above DFM_MAX_CANDIDATES is DFM_ERR_UNSUPPORTED.  Integer comparisons only: bitwise
 * reproducible. */
int dfm_catalogue_topk(const float* d_scores, const uint32_t* d_seen, const int32_t* d_user_of,
                       const int32_t* d_target, int64_t num_queries, int n_users, int n_items, int k,
                       int exclude_seen, int32_t* d_out_items, float* d_out_scores, int32_t* d_out_rank,
                       uint64_t* d_status, dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Quantised embedding tables for serving (csrc/quant.hip)
 * ------------------------------------------------------------------------------- */
/* DFM_QUANT_INT8_ROWWISE, widths D in {16, 32, 64}: one record of row_bytes = 16 + D per table row, records
 * contiguous, the base 16-byte aligned:
 *   bytes  0-3   scale (fp32)
 *   bytes  4-7   lo    (fp32)
 *   bytes  8-11  w1: the first-order weight of the same id, copied unchanged
 *   bytes 12-15  zero
 *   bytes 16 .. 16+D   q[0..D), uint8
 * Arithmetic, every step one IEEE fp32 operation (a numpy float32 restatement gives the same bits):
 *   lo, hi = min, max of the row's D values;  scale = (hi - lo) / 255.0f  (one subtract, one correctly rounded divide)
 *   q[j] = min(255, rint((x[j] - lo) / scale))  (subtract, divide, round half to even; rint can see a value a hair
 *          above 255, hence the clamp);  q[j] = 0 when scale == 0
 *   x'[j] = fadd(fmul((float)q[j], scale), lo): two roundings, never contracted into an fma.
 * A constant row dequantises exactly (the all-zero padding row 0 gives exactly 0); for every other row
 *   |x' - x| <= scale / 2 + 2^-21 * max(|lo|, |hi|)   (the second term covers the four fp32 roundings).
 * A table with a non-finite element, or a row whose hi - lo overflows, is refused: the quantise pass sets bit 0 of
 * *d_flag (its records are then meaningless) and the Python mirror raises ValueError naming the field. */
/* DFM_QUANT_UINT4_ROWWISE, the same widths: one record of row_bytes = 8 + D / 2 per table row (16 / 24 / 40 bytes),
 * records contiguous, the base 16-byte aligned, so every record is 8-byte aligned (and at D = 16 one aligned 16 bytes):
 *   bytes 0-1   scale (IEEE binary16)
 *   bytes 2-3   lo    (IEEE binary16)
 *   bytes 4-7   w1 (fp32): the first-order weight of the same id, copied unchanged
 *   bytes 8 ..  q[0..D), 4 bits each: element j in byte 8 + j / 2, the low nibble for even j
 * Arithmetic, every step one IEEE operation, never contracted (a numpy restatement gives the same bits):
 *   lo32, hi32 = min, max of the row's D values in fp32
 *   lo_h    = the largest binary16 <= lo32 (round to nearest even; where that is above lo32, one binary16 value
 *             towards -inf: -0 steps to -2^-24);  lo = (float)lo_h
 *   scale_h = the smallest binary16 >= (hi32 - lo) / 15.0f (round to nearest even; where that is below, one value
 *             towards +inf: 0 steps to 2^-24); then, where lo + 15 scale_h < hi32 still (the fp32 subtract and
 *             divide both rounded down; compared in fp64, where both sides are exact), one more value towards
 *             +inf;  scale = (float)scale_h
 *   q[j]  = min(15, rint((x[j] - lo) / scale))  (round half to even);  q[j] = 0 when scale == 0
 *   x'[j] = fadd(fmul((float)q[j], scale), lo).
 * So lo <= min and lo + 15 scale >= max hold exactly: x - lo >= 0, and the clamp is a safety net.
 * The all-zero padding row dequantises to exactly 0 (a constant row only if binary16 holds its value); every row has
 *   |x' - x| <= scale / 2 + 2^-21 * max(|lo|, |lo + 15 scale|).
 * Refused (bit 0 of *d_flag, as above): a non-finite element, an infinite lo_h (lo32 < -65504), an infinite scale_h. */
enum dfm_quant_format { DFM_QUANT_NONE = 0, DFM_QUANT_INT8_ROWWISE = 1, DFM_QUANT_UINT4_ROWWISE = 4 };
/* Record size in bytes; 0 for an unsupported width or format. */
int dfm_quant_row_bytes(int dim, int format);
/* One streaming pass over `rows` table rows: row r is the dim floats at d_w2 + r * stride2 (16-byte aligned,
 * stride2 % 4 == 0) with its first-order weight at d_w1 + r * stride1, strides in floats as in dfm_field, so packed
 * row records work as well as contiguous tables.  Writes rows * row_bytes bytes at d_out (16-byte aligned); d_flag as
 * above (never cleared by the call). */
int dfm_quantize_rows(const float* d_w2, int64_t stride2, const float* d_w1, int64_t stride1, int64_t rows, int dim,
                      int format, void* d_out, int32_t* d_flag, dfm_stream_t stream);
/* The inverse, into contiguous fp32: d_w2 (rows, dim), 16-byte aligned, and d_w1 (rows), either may be NULL. */
int dfm_dequantize_rows(const void* d_records, int64_t rows, int dim, int format, float* d_w2, float* d_w1,
                        dfm_stream_t stream);

/* One field of the quantised gather: a SPARSE field reads `rows` (vocab records), a DENSE field the four fp32
 * pointers of its Linear(1, dim) / Linear(1, 1) as dfm_field names them. */
typedef struct dfm_quant_field {
  int32_t kind;        /* DFM_SPARSE or DFM_DENSE */
  int32_t vocab;       /* records behind rows (0 for DENSE) */
  const void* rows;
  const float* w2;
  const float* b2;
  const float* w1;
  const float* b1;
} dfm_quant_field;

/* dfm_embedding_forward_staged for a uniform schema (every field SPARSE or DENSE of width dim) whose SPARSE tables
 * are quantised records: the same outputs (d_first_order (B,1), d_field_emb (B, F, dim), optional d_fm_out (B) and
 * d_fm_sum (B, dim)) from the dequantised rows, and the optional per-sample copy d_extra_src -> d_extra_dst (the
 * labels); no stage outputs.  `fields` is a HOST array in schema order, inputs[f] the field's int64 (B,) ids or float
 * (B,) values.  SPARSE columns of d_field_emb are x' above bit for bit, DENSE columns fmaf(x, w, b) as in
 * dfm_embedding_forward bit for bit; the sums over fields run in a fixed order (no float atomics).  An out-of-range id
 * sets bit 0 of *d_error_flag and reads record 0.  Needs no dfm_embedding_plan.  Enqueues, or with `at` naming a
 * captured node re-points it (dfm_launch above).  At most 48 SPARSE and 32 DENSE fields and dim in {16, 32, 64}, else
 * DFM_ERR_UNSUPPORTED with the reason.  batch >= 1. */
int dfm_embedding_forward_quant(const dfm_quant_field* fields, int num_fields, int dim, int format,
                                const void* const* inputs, const float* d_extra_src, float* d_extra_dst,
                                int64_t batch, float* d_first_order, float* d_field_emb, float* d_fm_out,
                                float* d_fm_sum, int32_t* d_error_flag, const dfm_launch* at);

/* dfm_embedding_forward_record (any schema: SPARSE, SEQUENCE and DENSE fields, projections, mixed widths; the same
 * record, outputs, error flag and launch geometry) with some SPARSE and SEQUENCE fields served from quantised records.
 *   quant_rows   a HOST array of plan->num_fields entries, carried to the kernel as arguments.  quant_rows[f] is the
 *                16-byte aligned base of field f's `vocab` records in `format`, of the field's OWN width (its
 *                embedding_dim, 16, 32 or 64, whatever fm_dim is); NULL: the field is read in fp32 through the plan,
 *                exactly as dfm_embedding_forward_record reads it.  With every entry NULL the two calls agree bit for
 *                bit on every output.
 *   format       DFM_QUANT_INT8_ROWWISE or DFM_QUANT_UINT4_ROWWISE, one for the whole call.
 * A quantised SPARSE field reads one record per sample: its row is x' = fadd(fmul(q, scale), lo) and its first-order
 * value the header's w1.  A quantised SEQUENCE field pools x' and w1 of its bag in ONE walk per 16-byte piece of the
 * row, in the order l = 0 .. L-1 with several record loads in flight; id 0 is skipped wherever it stands, an
 * out-of-range id sets bit 0 of *d_error_flag and counts as id 0, mean divides by the count of non-padding ids, max
 * works per column and on the first-order weight, an all-padding bag gives zeros.  Projected fields (dim != fm_dim)
 * accumulate with fmaf in the order j = 0 .. dim-1 and the raw x' go to d_flat, as in the fp32 gather.  So
 * first_order, field_emb, flat and fm_sum equal dfm_embedding_forward_record over the dequantised tables bit for bit
 * (fm too: the two kernels share their epilogue).  The plan's fp32 tables of the quantised fields are never read.
 * DFM_ERR_UNSUPPORTED with the reason: a quantised field whose dim is not 16, 32 or 64, a quantised DENSE field, a bad
 * format, a plan that dfm_embedding_forward_record refuses; DFM_ERR_INVALID: a misaligned base.  Enqueues, or with `at`
 * naming a captured node re-points it (dfm_launch above).  batch >= 1. */
int dfm_embedding_forward_record_quant(const dfm_embedding_plan* plan, const void* const* quant_rows, int format,
                                       const void* d_record, int64_t batch, float* d_first_order, float* d_field_emb,
                                       float* d_flat, int64_t ld_flat, float* d_fm_out, float* d_fm_sum,
                                       float* d_labels_out, int32_t* d_error_flag, const dfm_launch* at);

/* ---- score calibrators (csrc/calibrator.hip): fitted on the device from (label, logit) buffers, applied per launch ----
 * Both fits read n float32 labels (exactly 0 or 1) and n float32 LOGITS z, 1 <= n < 2^31, pointers of any 4-byte
 * alignment, use no float atomic, never synchronise and enqueue a fixed number of launches on `stream` (so a fit can be
 * captured into a graph).  A non-finite logit and a label other than 0 / 1 are faults: counted, and used for nothing.
 *
 * Platt scaling: q = sigmoid(a z + b), minimising
 *   F(a, b) = (1/n) sum_i [ log1p(exp(-|s_i|)) + max(s_i, 0) - t_i s_i ],   s_i = a z_i + b,
 * with t_i = y_i, or with smooth = 1 Platt's targets t = (N+ + 1) / (N+ + 2) for a positive and 1 / (N- + 2) for a
 * negative.  dfm_platt_fit enqueues 2 + 2 * max_rounds launches: a count pass and an init, then max_rounds pairs of
 *   sums    every workgroup walks its samples in a fixed order and leaves one vector of fp64 partial sums (per sample
 *           in fp64: the loss term, (q - t) z, (q - t), w z^2, w z, w with w = q (1 - q)) at the trial point read from
 *           the state block; no partial is combined by an atomic, so the result is the same bit for bit from run to
 *           run for the same input and the same n;
 *   update  one workgroup adds the partials in workgroup order (one thread per sum) and one thread advances the state:
 *           the first trial is the identity (1, 0); a trial with F <= the accepted F is accepted (so is one whose F
 *           equals the accepted F to within 64 units of fp64 rounding while its max |g| is smaller: close to the
 *           optimum the decrease of F falls below the rounding of its sum, the gradient's does not), and its Newton
 *           step d = -H^-1 g becomes the direction, with step length 1; a worse trial halves the step from the
 *           accepted point.  When the accepted point's mean gradient has max |g| <= gtol the status is converged.
 * Once the status is not DFM_CAL_RUNNING every later sums launch returns at once and every later update is a no-op.
 * fit_slope = 0 keeps a = 1 and fits b only (max |g| is then |g_b|).  A Hessian with det <= 1e-12 H_zz H_11 (all
 * logits equal) takes the bias-only step d = (0, -g_b / H_11) and sets DFM_CAL_FLAG_SLOPE_UNIDENTIFIED.
 *
 * The state block: 32 doubles (integers are stored as doubles; all are exact)
 *   [0] a  [1] b   the accepted point ((1, 0) until a trial is accepted, and for ever with single_class / bad_input)
 *   [2] F at the accepted point        [3] F at the identity (1, 0)        [4] max |g| at the accepted point
 *   [5] rounds used (sums evaluated)   [6] status (enum dfm_cal_status)    [7] flags (DFM_CAL_FLAG_*)
 *   [8] N+   [9] N-   [10] non-finite logits   [11] labels other than 0 / 1
 *   [12] [13] the trial point   [14] [15] the direction   [16] the step length   [17] [18] the targets t+, t-
 *   [19] n   [20] gtol   [21] fit_slope   [22 .. 31] reserved (0)
 * DFM_CAL_RUNNING after the call's last launch means max_rounds did not suffice; [0] [1] are then the best point seen.
 * d_workspace: dfm_platt_workspace_bytes(n) bytes (0 for n outside [1, 2^31)), 16-byte aligned; d_state 8-byte aligned. */
enum dfm_cal_kind { DFM_CAL_PLATT = 0, DFM_CAL_ISOTONIC = 1 };
enum dfm_cal_status { DFM_CAL_RUNNING = 0, DFM_CAL_CONVERGED = 1, DFM_CAL_SINGLE_CLASS = 2, DFM_CAL_BAD_INPUT = 3 };
#define DFM_CAL_FLAG_SLOPE_UNIDENTIFIED 1
#define DFM_PLATT_STATE_DOUBLES 32
size_t dfm_platt_workspace_bytes(int64_t n);
int dfm_platt_fit(const float* d_labels, const float* d_logits, int64_t n, int fit_slope, int smooth, int max_rounds,
                  double gtol, void* d_workspace, double* d_state, dfm_stream_t stream);

/* Isotonic regression over K = num_bins logit bins, 1 <= K <= 1024, equal-width over [z_lo, z_hi], -64 <= z_lo < z_hi
 * <= 64.  Three launches besides clearing the workspace.  For a sample without a fault, all in float32:
 *   z_c = fminf(fmaxf(z, z_lo), z_hi);   scale = (float)((double)K / ((double)z_hi - (double)z_lo))   (on the host)
 *   bin = min(K - 1, (int)fmul(fsub(z_c, z_lo), scale))                      two roundings, never contracted
 * and per bin three 64-bit integer sums: count, positives, sum of llrint((double)z_c * 2^24) (|.| <= 2^30 each, so
 * below 2^61 in all).  Integer sums: the table does not depend on the order of the samples or the launch geometry.
 * d_workspace (dfm_isotonic_workspace_bytes(K) bytes, 0 for K outside [1, 1024]; 16-byte aligned) holds, after the
 * call, 8 + 3 K int64 cells:  [0] used samples  [1] positives  [2] non-finite logits  [3] labels other than 0 / 1
 * [4 .. 7] 0, then {count, positives, sum z_fixed} per bin.
 * One workgroup then runs pool-adjacent-violators over the non-empty bins: blocks carry (positives, count), two
 * neighbours i < j are pooled only when pos_i cnt_j > pos_j cnt_i (a strict decrease, in 64-bit integers), a block's
 * value is the one fp64 division pos / cnt.  The knot table d_knots (DFM_ISOTONIC_KNOT_BYTES bytes, 16-byte aligned):
 *   int64 [0] m, the non-empty bins   [1] K   [2] non-finite logits   [3] labels other than 0 / 1   [4] used samples
 *         [5] positives   [6] blocks after pooling   [7] 0                                            (64 bytes)
 *   float  x32[1024], float v32[1024]    the knots as the apply reads them (float32 roundings of the fp64 values)
 *   double x[1024],   double v[1024]     x_j = ((double)sum z_fixed_j * 2^-24) / (double)cnt_j,  v_j = pos / cnt of
 *                                        the block that holds bin j
 * with one knot per non-empty bin, in bin order (interior knots of a constant run are kept); entries from m on are 0.
 * Every value is a ratio of integer sums, so the knots do not depend on the pooling order. */
#define DFM_ISOTONIC_MAX_BINS 1024
#define DFM_ISOTONIC_KNOT_BYTES (64 + 24 * DFM_ISOTONIC_MAX_BINS)
size_t dfm_isotonic_workspace_bytes(int num_bins);
int dfm_isotonic_fit(const float* d_labels, const float* d_logits, int64_t n, int num_bins, float z_lo, float z_hi,
                     void* d_workspace, void* d_knots, dfm_stream_t stream);

/* d_probs[i] = calibrated probability of the logit d_logits[i], i < n, 1 <= n < 2^31; one launch, enqueued or, with
 * `at` naming a captured node, re-pointed (dfm_launch above).  d_params (a Platt state block or a knot table, 16-byte
 * aligned) is read on the device when the launch runs: a refit changes what live graphs compute.  d_probs may alias
 * nothing else; the pointers may have any 4-byte alignment (16-byte loads and stores where both reach 16-byte
 * alignment after the same number of elements, one by one in front, behind and otherwise).  All in float32, every
 * operation its own rounding (nothing is contracted into an fma):
 *   DFM_CAL_PLATT     s = fadd(fmul((float)a, z), (float)b);  q = 1.f / (1.f + expf(-s))     (dfm_predict_head's form)
 *   DFM_CAL_ISOTONIC  NaN for a NaN z;  m == 0 (nothing fitted): q = 1.f / (1.f + expf(-z));  v32[0] for z <= x32[0];
 *                     v32[m-1] for z >= x32[m-1];  else with lo the last knot with x32[lo] <= z and hi = lo + 1:
 *                     t = fdiv(fsub(z, x_lo), fsub(x_hi, x_lo));  q = fminf(fadd(v_lo, fmul(t, fsub(v_hi, v_lo))), v_hi)
 *                     (the fminf keeps q inside [v_lo, v_hi] whatever the roundings, hence non-decreasing in z). */
int dfm_calibrate_apply(int kind, const void* d_params, const float* d_logits, int64_t n, float* d_probs,
                        const dfm_launch* at);

/* ---------------------------------------------------------------------------------
 * Feature encoders (csrc/encode.hip): raw int64 keys and raw values to the ids and scaled
 * values every other entry of this header takes (reference deepfm/data/transforms.py)
 * ------------------------------------------------------------------------------- */
/* The vocabulary of one field (reference transforms.py:14-18 and :59-63: a Python dict from value to index, index 0
 * for anything unseen): an open-addressing hash table of `capacity` 16-byte slots, 16-byte aligned, capacity a power
 * of two.  index == 0 marks an empty slot, so EVERY int64 is a legal key (0, -1, INT64_MIN and INT64_MAX included).
 * The home slot of a key is mix64((uint64_t)key) & (capacity - 1), probing is linear (+1, wrapping), and the one
 * mixer of this section is, in wrapping uint64 arithmetic,
 *   mix64(x):  x ^= x >> 33;  x *= 0xFF51AFD7ED558CCD;  x ^= x >> 33;  x *= 0xC4CEB9FE1A85EC53;  x ^= x >> 33. */
typedef struct dfm_vocab_slot {
  int64_t key;
  int32_t index;   /* 0: empty; else the 1-based rank of key among the kept keys */
  int32_t pad;     /* 0 */
} dfm_vocab_slot;
/* The capacity dfm_vocab_build wants for n_keys keys: the smallest power of two that is >= 2 * n_keys and >= 16, so
 * the load factor is at most 0.5; 0 for n_keys outside [0, 2^30]. */
int64_t dfm_vocab_capacity(int64_t n_keys);
/* Fills d_slots (dfm_vocab_capacity(n_keys) slots) from d_keys (n_keys) int64, STRICTLY increasing: key i receives
 * index i + 1 (the reference's sorted(set(values)) numbering, transforms.py:15-17).  The call clears the slots and
 * d_status first, then one thread per key claims the first slot of its probe sequence whose index is 0 with an integer
 * compare-and-swap on the index and writes the key with a plain store; nothing waits on another thread, and a probe
 * sequence ends after `capacity` slots.  Lookups run in later launches.  d_status[2] uint64:
 *   [0] keys that found no slot (cannot happen at this load factor; counted, not looped on)
 *   [1] keys that are not greater than their predecessor
 * The table is meaningless unless both are 0 (data/encoders.py reads them back once per fit and raises).  Which slot
 * of a probe run a key lands in depends on arrival order, what a lookup returns does not.  n_keys == 0 is an empty
 * table. */
int dfm_vocab_build(const int64_t* d_keys, int64_t n_keys, dfm_vocab_slot* d_slots, int64_t capacity,
                    uint64_t* d_status, dfm_stream_t stream);

enum dfm_encode_kind {
  DFM_ENC_LOOKUP = 0,     /* int64 in -> int64 out: the key's index, 0 if absent (transforms.py:20-23) */
  DFM_ENC_BAG = 1,        /* int64 (n, raw_width) in, optional lengths -> int64 (n, width) out (transforms.py:65-71) */
  DFM_ENC_HASHED = 2,     /* int64 in -> int64 out: 1 + mix64(raw) % num_buckets (unsigned); no table */
  DFM_ENC_SCALE_F32 = 3,  /* float  in -> float out: (float)(((double)v - lo) / (hi - lo)), 0 when hi == lo */
  DFM_ENC_SCALE_F64 = 4,  /* double in -> float out: the same (transforms.py:44-49, then PackedColumns' cast) */
  DFM_ENC_COPY_F32 = 5,   /* float in -> float out, unchanged: the labels */
  DFM_ENC_ZERO_F32 = 6    /* nothing in -> `width` float zeros per sample: absent labels, a block's padding row */
};
/* One column of a dfm_encode_columns launch.  Sample s reads in[s * in_stride .. + raw_width) and writes
 * out[s * out_stride .. + width), strides in ELEMENTS of the job's types, so one kernel writes the (S, n) id matrix of
 * DeviceColumns (stride 1) and the blocks of a batch record (RecordLayout: stride 1, a bag block stride max_length).
 * width = raw_width = 1 except for BAG (width = max_length, raw_width = tokens per input row) and ZERO (any width). */
typedef struct dfm_encode_job {
  const void* in;
  void* out;
  union {
    struct {
      const dfm_vocab_slot* slots;  /* LOOKUP, BAG */
      const int32_t* lengths;       /* BAG: (n) valid tokens per row, cut to [0, raw_width]; NULL: raw_width */
    } table;
    struct {
      double lo, hi;                /* SCALE: the fitted min and max */
    } scale;
    uint64_t num_buckets;           /* HASHED: >= 1 */
  } u;
  int32_t kind;           /* dfm_encode_kind */
  int32_t in_stride;
  int32_t out_stride;
  int32_t width;
  int32_t raw_width;
  int32_t log2_capacity;  /* LOOKUP, BAG: the table has 1 << log2_capacity slots */
} dfm_encode_job;
/* One launch over num_jobs <= DFM_MAX_FIELDS jobs (a HOST array, carried to the kernel as arguments; a larger schema
 * takes several calls): one thread per (job, sample, output position), consecutive lanes consecutive samples.  Samples
 * [0, n) are encoded; samples [n, n_out) are written as zeros (the padding tail RecordLayout.write leaves), and
 * nothing is read for them; 0 <= n <= n_out, n_out >= 1.
 *   BAG: position j < min(length, width) is the lookup of token j, an absent token is 0 IN PLACE (not compacted),
 *        every other position 0;
 *   SCALE: double arithmetic, one subtract and one divide, then one rounding to float; no clipping, a value outside
 *        [lo, hi] lands outside [0, 1] as in the reference.
 * Only plain C++ loads and stores; a thread touches its own sample's elements only.  in / out / slots / lengths must be
 * aligned to their element size (slots to 16 bytes).  Enqueues on `stream`, never synchronises. */
int dfm_encode_columns(const dfm_encode_job* jobs, int num_jobs, int64_t n, int64_t n_out, dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * Interaction log (csrc/interactions.hip, DESIGN.md section 7b "Interaction log on the device"): the integer work of
 * the reference's adapter between reading the ratings and fitting the encoders (deepfm/data/movielens.py:235-304,
 * 334-344, 467-480) over (user row, item row, timestamp, label) columns that are on the device already.
 * Integer atomics (or / add / 64-bit min) and plain stores only, so every output is bitwise independent of execution
 * order.  Every entry enqueues on `stream` and never synchronises.  d_status counts the rows an entry refused; no entry
 * clears it (the caller zeroes it once and reads it once), a refused row contributes nothing and is never used as an
 * index.
 * ------------------------------------------------------------------------------- */
/* The per-user seen-sets dfm_sample_negatives and its kin read (data/device_epoch.py:SeenSets), W = ceil(n_items / 32):
 * d_bitmap (n_users, W) uint32, bit i & 31 of word i >> 5 of user u set for every interaction (u, i), the bits at and
 * above n_items of the last word set; d_prefix (n_users, W + 1) uint32, prefix[u][w] = zero bits of the user's words
 * < w.  Three launches: every word initialised, one atomic or per interaction (duplicates are legal), one wavefront per
 * user for the prefix.  n == 0 gives the all-unseen sets.  d_status[1] uint64:
 *   [0] interactions with user < 0, user >= n_users, item < 0 or item >= n_items
 * n < 2^31, n_users and n_items >= 1, 4 * n_users * (2 W + 1) <= 2^30 bytes. */
int dfm_seen_sets_build(const int64_t* d_user_rows, const int64_t* d_item_rows, int64_t n, int64_t n_users,
                        int64_t n_items, uint32_t* d_bitmap, uint32_t* d_prefix, uint64_t* d_status,
                        dfm_stream_t stream);
/* Up to this many entities dfm_entity_counts keeps a workgroup's histogram in LDS (32 KiB of uint32) and adds its
 * non-zero counters to d_counts when the workgroup is done; above, every selected row is one global atomic add. */
#define DFM_COUNTS_LDS_ENTITIES 8192
/* d_counts[e] (int64, n_entities) = selected log rows r with d_entity_rows[r] == e and, when d_labels is given,
 * d_labels[r] == 1.0f exactly.  Selected: the rows d_index[0 .. m) (int64, any order, repeats count again), or, with
 * d_index NULL, all n_log rows (m is ignored).  The call zeroes d_counts itself.  d_status[2] uint64:
 *   [0] selected rows whose entity row is outside [0, n_entities)
 *   [1] entries of d_index outside [0, n_log)
 * 0 <= m, n_log < 2^31; 1 <= n_entities < 2^31. */
int dfm_entity_counts(const int64_t* d_entity_rows, const float* d_labels, const int64_t* d_index, int64_t m,
                      int64_t n_log, int64_t n_entities, int64_t* d_counts, uint64_t* d_status, dfm_stream_t stream);
/* The per-user marks of the global temporal split (movielens.py:269-304).  d_order (n) is the permutation of a
 * stable sort of the log by timestamp; positions [0, n_train) are the train rows, [n_train, n_trainval) the validation
 * window, [n_trainval, n) the test window (0 <= n_train <= n_trainval <= n).  Leaves
 *   d_in_train[u]   (uint8, n_users)  1 if user u has a row among the train positions, else 0
 *   d_first_val[u]  (int64, n_users)  the smallest position p of the validation window with d_labels[d_order[p]] == 1.0f
 *                                     and d_user_rows[d_order[p]] == u, for a user with d_in_train[u]; n if there is none
 *   d_first_test[u]                   the same over the test window
 * Three launches: the three outputs initialised, one plain store per train position, one 64-bit atomic min per
 * positive of a marked user in the windows.  d_status[1] uint64:
 *   [0] positions whose d_order entry is outside [0, n) or whose user row is outside [0, n_users)
 * n < 2^31. */
int dfm_temporal_split_mark(const int64_t* d_user_rows, const float* d_labels, const int64_t* d_order, int64_t n,
                            int64_t n_users, int64_t n_train, int64_t n_trainval, uint8_t* d_in_train,
                            int64_t* d_first_val, int64_t* d_first_test, uint64_t* d_status, dfm_stream_t stream);
/* The role of every row of the leave-one-out split (movielens.py:235-267).  d_order (n) is the permutation of a
 * stable sort of the log by (user row, timestamp), so a user's rows are one run of positions; d_user_counts (int64,
 * n_users) its rows in the whole log.  d_roles[p] (uint8, n): for a user with d_user_counts[u] >= min_interactions the
 * last position of its run is 2 (test), the one before it 1 (validation), every other 0 (train); for any other user
 * every position is 0.  One launch, one plain store per position; a position reads its two successors.
 * d_status[1] uint64 as for dfm_temporal_split_mark (such a position is role 0 and ends its neighbours' runs).
 * min_interactions >= 2; n < 2^31. */
int dfm_loo_split_mark(const int64_t* d_user_rows, const int64_t* d_order, const int64_t* d_user_counts, int64_t n,
                       int64_t n_users, int64_t min_interactions, uint8_t* d_roles, uint64_t* d_status,
                       dfm_stream_t stream);

/* ---------------------------------------------------------------------------------
 * User histories (csrc/history.hip, DESIGN.md section 7b "User histories on the device"): per query row of the log,
 * the items its user interacted with before it, latest first.  The log's order is (user row, timestamp, log position).
 * An event is a log row with d_source_mask[r] != 0 (every row when the mask is NULL) and d_labels[r] == 1.0f (every
 * row when d_labels is NULL).  Plain loads and stores only (the status counters are the one atomic), no LDS, and no
 * workgroup waits on another: every output is a pure function of the inputs.  Both entries enqueue on `stream` and
 * never synchronise; neither clears d_status.
 * ------------------------------------------------------------------------------- */
#define DFM_HISTORY_MAX_LENGTH 4096      /* dfm_record_assemble's bag cap */
enum dfm_history_mode { DFM_HISTORY_POSITION = 0, DFM_HISTORY_EXCLUDE = 1, DFM_HISTORY_LATEST = 2 };
/* The index of a log.  d_order (n) is the permutation of a stable sort of the log by (user row, timestamp), d_start
 * (n_users + 1, int64) the exclusive scan of the per-user row counts, so the positions [d_start[u], d_start[u + 1]) of
 * d_order are user u's rows in order.  One wavefront per user walks its segment 64 positions per trip.  Per position p
 * with log row r = d_order[p]:
 *   d_pos_of[r]    (int32, n)  p
 *   d_rank[p]      (int32, n)  the events of this user at positions before p
 *   d_sorted_ts[p] (int64, n)  d_timestamps[r]
 *   d_events[d_start[u] + d_rank[p]] (int32, n) = r for an event: the user's events, in order, compacted into the front
 *                  of its own segment (the entries behind them are not written)
 * and d_event_count[u] (int32, n_users) the user's events.  d_status[1] uint64:
 *   [0] positions whose d_order entry is outside [0, n), whose row names another user than the segment's (a user row
 *       outside [0, n_users) among them) or an item row outside [0, n_items), and segments that are not inside [0, n);
 *       such a position is no event, and its d_pos_of is not written
 * Reads 8 (order) + 8 (user) + 8 (item) + 8 (timestamp) + 4 (label) + 1 (mask) bytes per row and writes 4 + 4 + 8 and
 * 4 per event.  0 <= n < 2^31; 1 <= n_users, n_items < 2^31. */
int dfm_history_index_build(const int64_t* d_user_rows, const int64_t* d_item_rows, const int64_t* d_timestamps,
                            const float* d_labels, const uint8_t* d_source_mask, const int64_t* d_order,
                            const int64_t* d_start, int64_t n, int64_t n_users, int64_t n_items, int32_t* d_pos_of,
                            int32_t* d_rank, int32_t* d_events, int64_t* d_sorted_ts, int32_t* d_event_count,
                            uint64_t* d_status, dfm_stream_t stream);
/* The bags of m queries from that index.  d_queries[i] is a log row q (DFM_HISTORY_POSITION, DFM_HISTORY_EXCLUDE) or a
 * user row (DFM_HISTORY_LATEST).  With u the query's user and c its prior count
 *   POSITION  c = d_rank[d_pos_of[q]]: the user's events e with (ts[e], e) < (ts[q], q)
 *   EXCLUDE   c = d_rank at the first position of u's segment whose timestamp is not below ts[q] (a binary search over
 *             d_sorted_ts[d_start[u] .. d_pos_of[q]]): the user's events with ts[e] < ts[q]
 *   LATEST    c = d_event_count[u]
 * the outputs are, with e_j = d_events[d_start[u] + c - 1 - j],
 *   d_bag[i][j]  (int64, (m, length))  d_item_ids[d_item_rows[e_j]] for j < min(length, c), 0 behind; d_item_ids NULL:
 *                d_item_rows[e_j] + 1
 *   d_count[i]   (int64, m)  c
 *   d_gap[i]     (int64, m)  ts[q] - ts[e_0]; -1 when c == 0, and always for LATEST
 * A wavefront takes 64 queries: each lane forms one query's (user, start, c) once, then the lanes write the 64 bags as
 * one contiguous run of int64 (the per-query values come over by __shfl).  Every index is checked before it is used,
 * so no read leaves its buffer whatever the index holds.  d_status[2] uint64:
 *   [0] queries outside [0, n) (LATEST: [0, n_users)), or whose user row or position is outside the index: count 0,
 *       gap -1, an all-zero bag
 *   [1] bag slots whose event row or item row is outside its table: the slot is 0
 * 1 <= length <= DFM_HISTORY_MAX_LENGTH; 0 <= m, n < 2^31; m * length * 8 <= 2^32 bytes; m == 0 launches nothing. */
int dfm_history_gather(const int64_t* d_queries, int64_t m, int mode, int length, const int64_t* d_user_rows,
                       const int64_t* d_item_rows, const int64_t* d_timestamps, const int64_t* d_item_ids,
                       const int64_t* d_start, const int32_t* d_pos_of, const int32_t* d_rank, const int32_t* d_events,
                       const int64_t* d_sorted_ts, const int32_t* d_event_count, int64_t n, int64_t n_users,
                       int64_t n_items, int64_t* d_bag, int64_t* d_count, int64_t* d_gap, uint64_t* d_status,
                       dfm_stream_t stream);

/* The index as the record assembly takes it: the arrays dfm_history_gather takes (their shapes and types are stated
 * there and at dfm_history_index_build), the sizes and the mode.  The struct is read during the call that takes it and
 * need not outlive it; the arrays it names must stay alive and unchanged as long as the plan they were bound to. */
typedef struct dfm_history_source {
  const int64_t* d_user_rows;
  const int64_t* d_item_rows;
  const int64_t* d_timestamps;
  const int64_t* d_item_ids;      /* NULL: item row + 1 */
  const int64_t* d_start;
  const int32_t* d_pos_of;
  const int32_t* d_rank;
  const int32_t* d_events;
  const int64_t* d_sorted_ts;
  const int32_t* d_event_count;
  int64_t n;
  int64_t n_users;
  int64_t n_items;
  int32_t mode;                   /* dfm_history_mode */
} dfm_history_source;
/* Binds column `column` (an index into the `columns` array given to dfm_assemble_plan_create) of `plan` to the index:
 * from then on dfm_record_assemble forms that column's bags itself, in its one launch, and the column's `pos` is read
 * as (num_pos) int64 queries, one per positive: a log row (DFM_HISTORY_POSITION, DFM_HISTORY_EXCLUDE) or a user row
 * (DFM_HISTORY_LATEST).  Slot s of the record then holds, for the virtual row j = d_order[first + s] of positive p,
 * the `length` words dfm_history_gather writes for the query pos[p]: a negative or candidate row takes its positive's
 * bag (DFM_ROLE_COPY), and a padding slot (s >= count), a row d_order names outside the epoch and a query outside the
 * log (the user table) are all-zero bags.  The column must be a DFM_SEQUENCE column with DFM_ROLE_COPY.
 * A bound column is served by one wavefront per 64 slots (256 slots per workgroup, so the plan's launch map is rebuilt
 * here): a lane resolves its slot's positive and forms (segment start, prior count) once, then the 64 lanes write the
 * 64 bags as one contiguous run of int64, the per-slot values coming over by __shfl.  No atomics and no status word:
 * the caller validates the queries once (data/interactions.py:HistoryBag); every index is still checked before use, so
 * no read leaves its buffer.  Binding again re-points the column; no launch of the plan may be in flight then.
 * 0 <= n < 2^31; 1 <= n_users, n_items < 2^31; pointers aligned to their element size. */
int dfm_assemble_plan_bind_history(dfm_assemble_plan* plan, int column, const dfm_history_source* source);

/* ---------------------------------------------------------------------------------
 * Permutation field importance (csrc/importance.hip, DESIGN.md section 7d "Field importance"): the device side that
 * forms the batch records of an evaluation set with some fields shuffled across the samples.  Both entries enqueue on
 * `stream`, never synchronise, and use plain loads and stores only (no atomics, no LDS).
 * ------------------------------------------------------------------------------- */
/* The sort keys of the permutation of (seed, repeat) over n samples (wrapping uint64 arithmetic; mix32 is the counter
 * hash of csrc/dropout.h, the counter is formed as dfm_bootstrap_replicates forms its own, with another salt):
 *   counter(seed, repeat, i) = seed * 0x9E3779B97F4A7C15 + 0x5065726D4B657973 + (repeat << 40) + i
 *   d_keys[i] = (int64)(mix32(counter(seed, repeat, i)) >> 1) << 32 | i
 * Dropping one hash bit keeps every key non-negative (signed and unsigned order agree); the low word makes the keys
 * distinct, so their ascending sort has no ties and perm[j] = low 32 bits of sorted_keys[j] is a bijection of [0, n)
 * that depends on (seed, repeat, n) only.  1 <= n < 2^31, 0 <= repeat < 2^24. */
int dfm_permutation_keys(uint64_t seed, int64_t repeat, int64_t n, int64_t* d_keys, dfm_stream_t stream);
/* One field of a batch record (data/packed.py:RecordLayout): kind DFM_SPARSE (a row of B int64 ids), DFM_DENSE (a row
 * of B floats) or DFM_SEQUENCE (a block of B bags of max_length int64 ids); max_length is read for SEQUENCE only. */
typedef struct dfm_record_field {
  int32_t kind;
  int32_t max_length;
  int64_t offset;          /* byte offset of the field's column in the record */
} dfm_record_field;
/* The batch record of samples [first, first + count) of an evaluation set with the fields of `mask` permuted.
 *   d_set     the set as whole batch records of batch_size samples in RecordLayout's layout, ceil(n / batch_size)
 *             records set_stride bytes apart: sample g is slot g % batch_size of record g / batch_size;
 *   fields    num_fields <= DFM_MAX_FIELDS entries, schema order (a HOST array, carried to the kernel as arguments);
 *             offsets, labels_offset and record_bytes must be exactly those RecordLayout gives these kinds and lengths
 *             at this batch size, anything else is refused: every address the launch forms is checked here;
 *   d_sorted_keys  the n keys of dfm_permutation_keys, sorted ascending: perm[j] = low 32 bits of d_sorted_keys[j]
 *             (an entry whose low word is not below n is taken as j: whatever the keys hold, no read leaves the set);
 *   mask      bit f set: field f of slot i is that of sample perm[first + i]; clear: that of sample first + i, as the
 *             label always is.  A SEQUENCE field moves as its whole bag.  Bits at and above num_fields must be clear.
 * Slots at and beyond count are padding: id 0, value 0, label 0, all-padding bags.  Every byte of the id, dense, label
 * and bag blocks of d_out is written (the empty row that a schema without SPARSE or without DENSE fields keeps is
 * zeroed); the alignment gaps in front of the bag blocks and everything beyond record_bytes are not touched.
 * One launch: grid.y is the field (then the labels and the empty rows), a thread per 8-byte word of the field's block
 * (4-byte words for DENSE fields and the labels) in a grid-stride loop; stores are coalesced, a permuted word is one
 * gathered load.  d_set and d_out 16-byte aligned, set_stride a multiple of 16 and >= record_bytes;
 * 1 <= n < 2^31, 0 <= first, 1 <= count <= batch_size, first + count <= n. */
int dfm_records_permute(const void* d_set, int64_t set_stride, const dfm_record_field* fields, int num_fields,
                        int64_t batch_size, int64_t labels_offset, int64_t record_bytes, int64_t n,
                        const int64_t* d_sorted_keys, uint64_t mask, int64_t first, int64_t count, void* d_out,
                        dfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPFM_HIP_H */
