// FeatureEmbedding forward / dense-gradient backward for gfx950.
//
// Reference semantics: deepfm/models/layers/embedding.py:76-126 (forward) and its
// autograd (dense V x d gradients, nn.Embedding(sparse=False), embedding.py:35-40).
//
// Two forward paths:
//   * emb_fwd_uniform<D,W,US,UD>  — every field SPARSE or DENSE with dim == fm_dim == D and no
//     projection (the Criteo shape).  ONE launch gathers all tables: a workgroup of W waves owns
//     64/(D/4) consecutive samples, a wave US sparse + UD dense fields of them per pass, so ids are
//     read as one coalesced line and rows as 16-byte pieces, ALL loads of a pass in flight at once
//     (the kernel is one dependent chain kernarg -> ids -> rows -> stores; round-2 stamps:
//     profiles/r02_gather_microbench.txt).
//     first_order and the FM value are reduced across the block's waves through LDS in a fixed
//     order (W == 1: no LDS, no barrier).
//   * emb_fwd_general — any schema (mixed dims, projections, SEQUENCE bags): one thread
//     per (sample, field).  Correctness path for MovieLens-shaped schemas.
// and, for evaluation, emb_fwd_record<D>: the same semantics as emb_fwd_general + first_order_sum + the
// FM kernel, read from one batch record, with a lane group per (sample, field) (below).
#include "quant_records.h"
#include "tail_bodies.h"

#include <hip/hip_ext.h>

#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

using namespace dfm;

// One piece of parameters the record gather copies into LDS at workgroup start: n floats from src to LDS float dst.
struct RecordStage {
  const float* src;
  int32_t dst;
  int32_t n;
};

struct dfm_embedding_plan {
  int num_fields = 0;
  int fm_dim = 0;
  int total_dim = 0;
  int uniform = 0;
  int max_dim = 0;
  std::vector<dfm_field> h_fields;
  std::vector<int32_t> h_sparse, h_dense, h_proj;
  dfm_field* d_fields = nullptr;
  int32_t* d_sparse = nullptr;
  int32_t* d_dense = nullptr;
  int32_t* d_proj = nullptr;
  // record gather (emb_fwd_record): "" when the plan qualifies, else why not
  std::string record_why;
  int record_param_floats = 0;      // LDS floats of projections + DENSE Linear(1, d) parameters
  std::vector<RecordStage> h_stage;
  std::vector<int32_t> h_lds_off;   // per field: [LDS offset of its projection, of its DENSE parameters] (-1: none)
  RecordStage* d_stage = nullptr;
  int32_t* d_lds_off = nullptr;
};

static void plan_record_layout(dfm_embedding_plan* plan);

// ======================================================================================
// uniform fused gather
// ======================================================================================
// Per-call slot tables travel BY VALUE in the kernel-argument segment: a wave's slot index
// depends only on its wave id, so the slot (pointers + vocab) is one scalar load issued at
// kernel entry — the dependent chain is kernarg -> ids -> rows, nothing else.
struct SparseSlot {
  const int64_t* ids;
  const float* w2;
  const float* w1;
  int32_t vocab;
  int32_t field;
  int32_t stride2;  // floats between rows of w2 / w1 (packed row records: the record size)
  int32_t stride1;
  int64_t* ids_out;  // optional: the ids are also copied here (staging of the step's static inputs)
};
struct DenseSlot {
  const float* x;
  const float* w2;
  const float* b2;
  const float* w1;
  const float* b1;
  int32_t field;
  int32_t pad;
  float* x_out;      // optional: copy of x (staging)
};
constexpr int kMaxSparseSlots = 48, kMaxDenseSlots = 32;   // 48*48 + 32*56 B of kernel arguments
struct UniformArgs {
  SparseSlot sp[kMaxSparseSlots];
  DenseSlot de[kMaxDenseSlots];
};

typedef float v4f __attribute__((ext_vector_type(4)));
// Streaming (nt) stores of field_embeddings: -0.8 us for the isolated kernel (tools/microbench_gather2), but
// inside the training step they cost 0.4-1.2 us and 3.7 MB of extra write requests (the consumer is the next
// kernel of the graph) — the product kernel stores plainly; shape 6 keeps the nt variant for the tools.
__device__ __forceinline__ void st4_stream(float* p, const float4& v) {
  v4f t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(p));
}

template <int D, int W, int US, int UD>
__device__ __forceinline__ void emb_fwd_uniform_body(
    const UniformArgs& args, int ns, int nd, int64_t B, int F, float* __restrict__ first_order,
    float* __restrict__ fe, float* __restrict__ fm_out, float* __restrict__ fm_sum, int32_t* error_flag,
    const float* __restrict__ extra_src = nullptr, float* __restrict__ extra_dst = nullptr) {
  constexpr int LPR = D / 4;        // lanes per row (16 B each)
  constexpr int SPW = kWave / LPR;  // samples per wave == samples per block
  const int lane = lane_id();
  const int wave = W == 1 ? 0 : wave_id_uniform();
  const int s = lane / LPR, q = lane % LPR;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * SPW + s;
  const bool live = b < B;
  const int64_t bc = live ? b : B - 1;  // clamped: dead lanes load valid addresses

  float4 S = make_float4(0.f, 0.f, 0.f, 0.f);   // sum_f e
  float4 SQ = make_float4(0.f, 0.f, 0.f, 0.f);  // sum_f e^2
  float fo = 0.f;
  bool bad = false;

  // One straight-line block per pass: every slot, then every id / dense value, then every row, then
  // the arithmetic, and only then the (predicated) stores — so no branch sits between a load and
  // its first use and the waits stay counted, not vmcnt(0).  Slots past the end are clamped to
  // slot 0 (a duplicate, cache-hitting load) and masked — so a kind with no fields must be launched
  // with US == 0 / UD == 0 (describe_uniform), never with an unset slot 0.
  const int sp_iters = US ? (ns + W * US - 1) / (W * US) : 0;
  const int de_iters = UD ? (nd + W * UD - 1) / (W * UD) : 0;
  // W == 1 (the host launches it only when one pass covers the plan): slot indices are compile-time
  // constants, so every slot field is an immediate-offset scalar load from the kernel arguments
  const int iters = W == 1 ? 1 : (sp_iters > de_iters ? sp_iters : de_iters);
  for (int it = 0; it < iters; ++it) {
    bool oks[US + 1], okd[UD + 1];
    SparseSlot sl[US + 1];
    DenseSlot dl[UD + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) {
      const int i = W == 1 ? u : wave + (it * US + u) * W;
      oks[u] = i < ns;
      sl[u] = args.sp[oks[u] ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      const int i = W == 1 ? u : wave + (it * UD + u) * W;
      okd[u] = i < nd;
      dl[u] = args.de[okd[u] ? i : 0];
    }
    int64_t id[US + 1];
    float x[UD + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) id[u] = sl[u].ids[bc];
#pragma unroll
    for (int u = 0; u < UD; ++u) x[u] = dl[u].x[bc];
    // staging: the raw inputs also go to the step's static buffers (row plan, embedding backward)
#pragma unroll
    for (int u = 0; u < US; ++u)
      if (sl[u].ids_out && live && q == 0 && oks[u]) sl[u].ids_out[b] = id[u];
#pragma unroll
    for (int u = 0; u < UD; ++u)
      if (dl[u].x_out && live && q == 0 && okd[u]) dl[u].x_out[b] = x[u];
    float4 row[US + 1];
    float w1v[US + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) {
      const bool oob = static_cast<uint64_t>(id[u]) >= static_cast<uint64_t>(sl[u].vocab);
      bad |= oob && oks[u];
      id[u] = oob ? 0 : id[u];
      row[u] = ld4(sl[u].w2 + id[u] * sl[u].stride2 + q * 4);
      w1v[u] = sl[u].w1[id[u] * sl[u].stride1];   // same address on the row's lanes: one request
    }
    float4 dw[UD + 1], db[UD + 1];
    float dw1[UD + 1], db1[UD + 1];
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      dw[u] = ld4(dl[u].w2 + q * 4);
      db[u] = ld4(dl[u].b2 + q * 4);
      dw1[u] = dl[u].w1[0];
      db1[u] = dl[u].b1[0];
    }
    float* out = fe + b * F * D + q * 4;
#pragma unroll
    for (int u = 0; u < US; ++u) {
      const float m = oks[u] ? 1.f : 0.f;
      const float4 e = row[u];
      S.x = fmaf(m, e.x, S.x); S.y = fmaf(m, e.y, S.y); S.z = fmaf(m, e.z, S.z); S.w = fmaf(m, e.w, S.w);
      SQ.x = fmaf(m * e.x, e.x, SQ.x); SQ.y = fmaf(m * e.y, e.y, SQ.y);
      SQ.z = fmaf(m * e.z, e.z, SQ.z); SQ.w = fmaf(m * e.w, e.w, SQ.w);
      fo = fmaf(m, w1v[u], fo);
      if (live && oks[u]) st4(out + sl[u].field * D, e);
    }
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      const float m = okd[u] ? 1.f : 0.f;
      float4 e;
      e.x = fmaf(x[u], dw[u].x, db[u].x); e.y = fmaf(x[u], dw[u].y, db[u].y);
      e.z = fmaf(x[u], dw[u].z, db[u].z); e.w = fmaf(x[u], dw[u].w, db[u].w);
      S.x = fmaf(m, e.x, S.x); S.y = fmaf(m, e.y, S.y); S.z = fmaf(m, e.z, S.z); S.w = fmaf(m, e.w, S.w);
      SQ.x = fmaf(m * e.x, e.x, SQ.x); SQ.y = fmaf(m * e.y, e.y, SQ.y);
      SQ.z = fmaf(m * e.z, e.z, SQ.z); SQ.w = fmaf(m * e.w, e.w, SQ.w);
      fo = fmaf(m, fmaf(x[u], dw1[u], db1[u]), fo);
      if (live && okd[u]) st4(out + dl[u].field * D, e);
    }
  }
  if (bad && error_flag) atomicOr(error_flag, 1);
  if (q != 0) fo = 0.f;  // every lane of a row loaded the same first-order value: count it once
  float acc[9] = {S.x, S.y, S.z, S.w, SQ.x, SQ.y, SQ.z, SQ.w, fo};
  if (W > 1) {
    // ---- fixed-order reduction over the block's waves ------------------------------------
    __shared__ float red[W][9][kWave];
#pragma unroll
    for (int c = 0; c < 9; ++c) red[wave][c][lane] = acc[c];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int c = 0; c < 9; ++c) acc[c] = red[0][c][lane];
    for (int w = 1; w < W; ++w) {
#pragma unroll
      for (int c = 0; c < 9; ++c) acc[c] += red[w][c][lane];
    }
  }
  // 0.5 * sum_d (S_d^2 - SQ_d)   (fm.py:20-22)
  float t = (acc[0] * acc[0] - acc[4]) + (acc[1] * acc[1] - acc[5]) +
            (acc[2] * acc[2] - acc[6]) + (acc[3] * acc[3] - acc[7]);
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) t += __shfl_xor(t, m, kWave);
  if (live && q == 0) {
    first_order[b] = acc[8];
    if (fm_out) fm_out[b] = 0.5f * t;
  }
  // S[b, :] = sum_f e[b, f, :] for the FM backward g * (S - e)
  if (live && fm_sum) st4(fm_sum + b * D + q * 4, make_float4(acc[0], acc[1], acc[2], acc[3]));
  if (live && q == 0 && extra_dst) extra_dst[b] = extra_src[b];      // per-sample payload (labels)
}

// --------------------------------------------------------------------------------------------------
// emb_fwd_pair<D, NS, ND, STAGE>: the same gather compiled for an EXACT field count (the Criteo shape:
// NS = 26 SPARSE + ND = 13 DENSE).  A workgroup of TWO waves owns 64/(D/4) samples; wave w takes the
// slots 2u + w.  Every slot index and both counts are compile-time constants: slot fields are
// immediate-offset scalar loads, there is no run-time selection, masking or branch between a load and
// its use (staging is a template flag), and all of a wave's loads are in flight in three rounds:
// ids + dense values -> rows + first-order scalars + dense weights -> math + streaming stores.
// Measured against the 8-wave shape on the same tables: profiles/r02_gather_shapes.csv.
template <int D, int NS, int ND, bool STAGE, int WAVE, bool NT>
__device__ __forceinline__ void emb_fwd_pair_wave(
    const UniformArgs& args, int64_t B, int F, float* __restrict__ fe, int32_t* error_flag, float (&acc)[9]) {
  constexpr int LPR = D / 4;
  constexpr int SPW = kWave / LPR;
  constexpr int HS = (NS - WAVE + 1) / 2, HD = (ND - WAVE + 1) / 2;   // this wave's slots: 2u + WAVE
  const int lane = lane_id();
  const int s = lane / LPR, q = lane % LPR;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * SPW + s;
  const bool live = b < B;
  const int64_t bc = live ? b : B - 1;
  int64_t id[HS + 1];
  float x[HD + 1];
#pragma unroll
  for (int u = 0; u < HS; ++u) id[u] = args.sp[2 * u + WAVE].ids[bc];
#pragma unroll
  for (int u = 0; u < HD; ++u) x[u] = args.de[2 * u + WAVE].x[bc];
  float4 row[HS + 1];
  float w1v[HS + 1];
  bool bad = false;
#pragma unroll
  for (int u = 0; u < HS; ++u) {
    const SparseSlot& sl = args.sp[2 * u + WAVE];
    const bool oob = static_cast<uint64_t>(id[u]) >= static_cast<uint64_t>(sl.vocab);
    bad |= oob;
    const int64_t i = oob ? 0 : id[u];
    row[u] = ld4(sl.w2 + i * sl.stride2 + q * 4);
    w1v[u] = sl.w1[i * sl.stride1];
  }
  float4 dw[HD + 1], db[HD + 1];
  float dw1[HD + 1], db1[HD + 1];
#pragma unroll
  for (int u = 0; u < HD; ++u) {
    const DenseSlot& dl = args.de[2 * u + WAVE];
    dw[u] = ld4(dl.w2 + q * 4);
    db[u] = ld4(dl.b2 + q * 4);
    dw1[u] = dl.w1[0];
    db1[u] = dl.b1[0];
  }
  if (STAGE && live && q == 0) {
#pragma unroll
    for (int u = 0; u < HS; ++u) args.sp[2 * u + WAVE].ids_out[b] = id[u];
#pragma unroll
    for (int u = 0; u < HD; ++u) args.de[2 * u + WAVE].x_out[b] = x[u];
  }
  float4 S = make_float4(0.f, 0.f, 0.f, 0.f), SQ = make_float4(0.f, 0.f, 0.f, 0.f);
  float fo = 0.f;
  float* out = fe + b * F * D + q * 4;
#pragma unroll
  for (int u = 0; u < HS; ++u) {
    const float4 e = row[u];
    S.x += e.x; S.y += e.y; S.z += e.z; S.w += e.w;
    SQ.x = fmaf(e.x, e.x, SQ.x); SQ.y = fmaf(e.y, e.y, SQ.y);
    SQ.z = fmaf(e.z, e.z, SQ.z); SQ.w = fmaf(e.w, e.w, SQ.w);
    fo += w1v[u];
    if (live) { if (NT) st4_stream(out + args.sp[2 * u + WAVE].field * D, e); else st4(out + args.sp[2 * u + WAVE].field * D, e); }
  }
#pragma unroll
  for (int u = 0; u < HD; ++u) {
    float4 e;
    e.x = fmaf(x[u], dw[u].x, db[u].x); e.y = fmaf(x[u], dw[u].y, db[u].y);
    e.z = fmaf(x[u], dw[u].z, db[u].z); e.w = fmaf(x[u], dw[u].w, db[u].w);
    S.x += e.x; S.y += e.y; S.z += e.z; S.w += e.w;
    SQ.x = fmaf(e.x, e.x, SQ.x); SQ.y = fmaf(e.y, e.y, SQ.y);
    SQ.z = fmaf(e.z, e.z, SQ.z); SQ.w = fmaf(e.w, e.w, SQ.w);
    fo += fmaf(x[u], dw1[u], db1[u]);
    if (live) { if (NT) st4_stream(out + args.de[2 * u + WAVE].field * D, e); else st4(out + args.de[2 * u + WAVE].field * D, e); }
  }
  if (bad && error_flag) atomicOr(error_flag, 1);
  if (q != 0) fo = 0.f;
  acc[0] = S.x; acc[1] = S.y; acc[2] = S.z; acc[3] = S.w;
  acc[4] = SQ.x; acc[5] = SQ.y; acc[6] = SQ.z; acc[7] = SQ.w; acc[8] = fo;
}

template <int D, int NS, int ND, bool STAGE, bool NT = false>
__global__ __launch_bounds__(128) void emb_fwd_pair(
    UniformArgs args, int64_t B, int F, float* __restrict__ first_order, float* __restrict__ fe,
    float* __restrict__ fm_out, float* __restrict__ fm_sum, int32_t* error_flag,
    const float* __restrict__ extra_src, float* __restrict__ extra_dst) {
  constexpr int LPR = D / 4;
  constexpr int SPW = kWave / LPR;
  __shared__ float red[9][kWave];
  const int lane = lane_id();
  float acc[9];
  if (wave_id_uniform() == 1) {
    emb_fwd_pair_wave<D, NS, ND, STAGE, 1, NT>(args, B, F, fe, error_flag, acc);
#pragma unroll
    for (int c = 0; c < 9; ++c) red[c][lane] = acc[c];
    __syncthreads();
    return;
  }
  emb_fwd_pair_wave<D, NS, ND, STAGE, 0, NT>(args, B, F, fe, error_flag, acc);
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 9; ++c) acc[c] += red[c][lane];      // fixed order: wave 0 + wave 1
  const int s = lane / LPR, q = lane % LPR;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * SPW + s;
  const bool live = b < B;
  float t = (acc[0] * acc[0] - acc[4]) + (acc[1] * acc[1] - acc[5]) +
            (acc[2] * acc[2] - acc[6]) + (acc[3] * acc[3] - acc[7]);
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) t += __shfl_xor(t, m, kWave);
  if (live && q == 0) {
    first_order[b] = acc[8];
    if (fm_out) fm_out[b] = 0.5f * t;
    if (STAGE && extra_dst) extra_dst[b] = extra_src[b];
  }
  if (live && fm_sum) st4(fm_sum + b * D + q * 4, make_float4(acc[0], acc[1], acc[2], acc[3]));
}

// slot tables in the kernel-argument segment (first touch measured at 0-40 ns: the segment is hot
// when the waves start)
template <int D, int W, int US, int UD>
__global__ __launch_bounds__(W * 64) void emb_fwd_uniform(
    UniformArgs args, int ns, int nd, int64_t B, int F, float* __restrict__ first_order,
    float* __restrict__ fe, float* __restrict__ fm_out, float* __restrict__ fm_sum, int32_t* error_flag,
    const float* __restrict__ extra_src, float* __restrict__ extra_dst) {
  emb_fwd_uniform_body<D, W, US, UD>(args, ns, nd, B, F, first_order, fe, fm_out, fm_sum, error_flag, extra_src, extra_dst);
}

// ======================================================================================
// general path
// ======================================================================================
__device__ __forceinline__ float bag_pool(const float* __restrict__ table, int stride, int j,
                                          const int64_t* __restrict__ ids, int L, int vocab,
                                          int combiner, int32_t* error_flag) {
  float acc = 0.f;
  int count = 0;
  bool first = true;
  for (int l = 0; l < L; ++l) {
    const int64_t id = checked_id(ids[l], vocab, error_flag);
    if (id == 0) continue;
    const float v = table[id * stride + j];
    if (combiner == DFM_MAX) {
      if (first || v > acc) acc = v;
      first = false;
    } else {
      acc += v;
    }
    ++count;
  }
  if (combiner == DFM_MEAN && count > 0) acc = acc / static_cast<float>(count);
  return acc;
}

__global__ void emb_fwd_general(const dfm_field* __restrict__ fields, PtrTable in, int64_t B, int F,
                                int fm_dim, int total_dim, float* __restrict__ fo_parts,
                                float* __restrict__ fe, float* __restrict__ flat,
                                int32_t* error_flag) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= B * F) return;
  const int f = static_cast<int>(t % F);
  const int64_t b = t / F;
  const dfm_field fd = fields[f];
  const int d = fd.dim;
  float* flat_row = flat + b * total_dim + fd.flat_offset;
  float* fe_row = fe + (b * F + f) * fm_dim;
  float fo;
  if (fd.kind == DFM_SPARSE) {
    const int64_t id = checked_id(static_cast<const int64_t*>(in.p[f])[b], fd.vocab, error_flag);
    const float* row = fd.w2 + id * fd.stride2;
    for (int j = 0; j < d; ++j) flat_row[j] = row[j];
    fo = fd.w1[id * fd.stride1];
  } else if (fd.kind == DFM_DENSE) {
    const float x = static_cast<const float*>(in.p[f])[b];
    for (int j = 0; j < d; ++j) flat_row[j] = fmaf(x, fd.w2[j], fd.b2[j]);
    fo = fmaf(x, fd.w1[0], fd.b1[0]);
  } else {
    const int64_t* ids = static_cast<const int64_t*>(in.p[f]) + b * fd.max_len;
    for (int j = 0; j < d; ++j)
      flat_row[j] = bag_pool(fd.w2, fd.stride2, j, ids, fd.max_len, fd.vocab, fd.combiner, error_flag);
    fo = bag_pool(fd.w1, fd.stride1, 0, ids, fd.max_len, fd.vocab, fd.combiner, error_flag);
  }
  fo_parts[b * F + f] = fo;
  if (fd.proj) {
    for (int k = 0; k < fm_dim; ++k) {
      float acc = 0.f;
      for (int j = 0; j < d; ++j) acc = fmaf(flat_row[j], fd.proj[k * d + j], acc);
      fe_row[k] = acc;
    }
  } else {
    for (int j = 0; j < d; ++j) fe_row[j] = flat_row[j];
  }
}

__global__ void first_order_sum(const float* __restrict__ fo_parts, int64_t B, int F,
                                float* __restrict__ first_order) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float acc = 0.f;
  for (int f = 0; f < F; ++f) acc += fo_parts[b * F + f];
  first_order[b] = acc;
}

// ======================================================================================
// dense-gradient backward
// ======================================================================================
// gradient w.r.t. the raw (pre-projection) embedding element j of (b, f)
__device__ __forceinline__ float raw_grad(const dfm_field& fd, int f, int64_t b, int j, int F,
                                          int fm_dim, int total_dim,
                                          const float* __restrict__ g_field,
                                          const float* __restrict__ g_flat) {
  float g = g_flat ? g_flat[b * total_dim + fd.flat_offset + j] : 0.f;
  const float* gf = g_field + (b * F + f) * fm_dim;
  if (fd.proj) {
    for (int k = 0; k < fm_dim; ++k) g = fmaf(gf[k], fd.proj[k * fd.dim + j], g);
  } else {
    g += gf[j];
  }
  return g;
}

// SPARSE + SEQUENCE rows: float atomics into the dense (V, d) gradients.
__global__ void emb_bwd_scatter(const dfm_field* __restrict__ fields, PtrTable in, GradTable gt,
                                int64_t B, int F, int fm_dim, int total_dim,
                                const float* __restrict__ g_first,
                                const float* __restrict__ g_field,
                                const float* __restrict__ g_flat) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= B * F) return;
  const int f = static_cast<int>(t % F);
  const int64_t b = t / F;
  const dfm_field fd = fields[f];
  if (fd.kind == DFM_DENSE) return;
  const int d = fd.dim;
  const dfm_field_grad g = gt.g[f];
  const float gfo = g_first[b];
  if (fd.kind == DFM_SPARSE) {
    int64_t id = static_cast<const int64_t*>(in.p[f])[b];
    if (id <= 0 || id >= fd.vocab) return;  // padding row: no gradient
    for (int j = 0; j < d; ++j)
      atomicAdd(g.w2 + id * d + j, raw_grad(fd, f, b, j, F, fm_dim, total_dim, g_field, g_flat));
    atomicAdd(g.w1 + id, gfo);
    return;
  }
  // SEQUENCE
  const int64_t* ids = static_cast<const int64_t*>(in.p[f]) + b * fd.max_len;
  const int L = fd.max_len;
  int count = 0;
  for (int l = 0; l < L; ++l) count += (ids[l] > 0 && ids[l] < fd.vocab) ? 1 : 0;
  if (count == 0) return;
  if (fd.combiner == DFM_MAX) {
    for (int j = 0; j <= d; ++j) {  // j == d: the (V,1) first-order table
      const float* table = j < d ? fd.w2 : fd.w1;
      const int stride = j < d ? fd.stride2 : fd.stride1, col = j < d ? j : 0;
      int64_t best = 0;
      float bestv = 0.f;
      for (int l = 0; l < L; ++l) {
        const int64_t id = ids[l];
        if (id <= 0 || id >= fd.vocab) continue;
        const float v = table[id * stride + col];
        if (best == 0 || v > bestv) { best = id; bestv = v; }
      }
      if (j < d)
        atomicAdd(g.w2 + best * d + j, raw_grad(fd, f, b, j, F, fm_dim, total_dim, g_field, g_flat));
      else
        atomicAdd(g.w1 + best, gfo);
    }
    return;
  }
  const float scale = fd.combiner == DFM_MEAN ? 1.f / static_cast<float>(count) : 1.f;
  for (int j = 0; j < d; ++j) {
    const float gj = raw_grad(fd, f, b, j, F, fm_dim, total_dim, g_field, g_flat) * scale;
    for (int l = 0; l < L; ++l) {
      const int64_t id = ids[l];
      if (id > 0 && id < fd.vocab) atomicAdd(g.w2 + id * d + j, gj);
    }
  }
  for (int l = 0; l < L; ++l) {
    const int64_t id = ids[l];
    if (id > 0 && id < fd.vocab) atomicAdd(g.w1 + id, gfo * scale);
  }
}

// Block-wide fixed-order sum of two values (256 threads).
using tail::block_sum2;

// DENSE fields: dW2[j] = sum_b x_b * g_raw[b,j], db2[j] = sum_b g_raw[b,j]; block (i, j);
// j == dim handles the first-order Linear(1,1).
__global__ __launch_bounds__(256) void emb_bwd_dense_fields(
    const dfm_field* __restrict__ fields, const int32_t* __restrict__ dense_list, PtrTable in,
    GradTable gt, int64_t B, int F, int fm_dim, int total_dim, const float* __restrict__ g_first,
    const float* __restrict__ g_field, const float* __restrict__ g_flat) {
  const int f = dense_list[blockIdx.x];
  const dfm_field fd = fields[f];
  const int j = blockIdx.y;
  if (j > fd.dim) return;
  const float* x = static_cast<const float*>(in.p[f]);
  float sw = 0.f, sb = 0.f;
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    const float g = j < fd.dim ? raw_grad(fd, f, b, j, F, fm_dim, total_dim, g_field, g_flat)
                               : g_first[b];
    sw = fmaf(x[b], g, sw);
    sb += g;
  }
  block_sum2(sw, sb);
  if (threadIdx.x == 0) {
    const dfm_field_grad g = gt.g[f];
    if (j < fd.dim) { g.w2[j] += sw; g.b2[j] += sb; }
    else            { g.w1[0] += sw; g.b1[0] += sb; }
  }
}

// Uniform plans (dim == fm_dim, no projection, g_flat folded into g_field): block (i, jq) sums 4
// columns of field i's gradient with 16-byte loads — the 4 column groups of a field walk the same
// 64-byte segments, so the second to fourth hit L2 — instead of one 4-byte load per line and column.
// jq == dim/4 handles the first-order Linear(1,1).
__global__ __launch_bounds__(256) void emb_bwd_dense_fields_uniform(
    const int32_t* __restrict__ dense_list, PtrTable in, GradTable gt, int64_t B, int F, int D,
    const float* __restrict__ g_first, const float* __restrict__ g_field) {
  tail::dense_fields_uniform_body(blockIdx.x, dense_list, in, gt, B, F, D, g_first, g_field);
}

// Projection gradient dP[k,j] = sum_b g_field[b,f,k] * raw[b,j]; block (i, k*max_dim + j).
__global__ __launch_bounds__(256) void emb_bwd_proj(
    const dfm_field* __restrict__ fields, const int32_t* __restrict__ proj_list, GradTable gt,
    int64_t B, int F, int fm_dim, int total_dim, int max_dim, const float* __restrict__ g_field,
    const float* __restrict__ flat_saved) {
  const int f = proj_list[blockIdx.x];
  const dfm_field fd = fields[f];
  const int k = blockIdx.y / max_dim, j = blockIdx.y % max_dim;
  if (j >= fd.dim) return;
  float acc = 0.f, unused = 0.f;
  for (int64_t b = threadIdx.x; b < B; b += 256)
    acc = fmaf(g_field[(b * F + f) * fm_dim + k], flat_saved[b * total_dim + fd.flat_offset + j], acc);
  block_sum2(acc, unused);
  if (threadIdx.x == 0) gt.g[f].proj[k * fd.dim + j] += acc;
}

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" int dfm_embedding_plan_create(const dfm_field* fields, int num_fields, int fm_dim,
                              dfm_embedding_plan** out_plan) {
  DFM_REQUIRE(fields && out_plan, "null argument");
  DFM_REQUIRE(num_fields > 0 && num_fields <= DFM_MAX_FIELDS,
              "num_fields %d outside [1, %d]", num_fields, DFM_MAX_FIELDS);
  DFM_REQUIRE(fm_dim > 0, "fm_dim must be positive");
  auto* plan = new dfm_embedding_plan();
  plan->num_fields = num_fields;
  plan->fm_dim = fm_dim;
  plan->h_fields.assign(fields, fields + num_fields);
  bool uniform = (fm_dim % 4 == 0) && (kWave % (fm_dim / 4) == 0) && fm_dim <= 256;
  int off = 0;
  for (int f = 0; f < num_fields; ++f) {
    dfm_field& fd = plan->h_fields[f];
    if (fd.dim <= 0 || !fd.w2 || !fd.w1 || (fd.kind == DFM_DENSE && (!fd.b2 || !fd.b1)) ||
        (fd.kind != DFM_DENSE && fd.vocab <= 0) || (fd.kind == DFM_SEQUENCE && fd.max_len <= 0) ||
        fd.kind < 0 || fd.kind > 2 || fd.combiner < 0 || fd.combiner > 2 ||
        ((fd.dim != fm_dim) != (fd.proj != nullptr))) {
      delete plan;
      return fail(DFM_ERR_INVALID, "field %d: inconsistent descriptor", f);
    }
    if (fd.stride2 == 0) fd.stride2 = fd.dim;
    if (fd.stride1 == 0) fd.stride1 = 1;
    if (fd.kind != DFM_DENSE && (fd.stride2 < fd.dim || fd.stride1 < 1)) {
      delete plan;
      return fail(DFM_ERR_INVALID, "field %d: bad row strides", f);
    }
    fd.flat_offset = off;
    off += fd.dim;
    plan->max_dim = fd.dim > plan->max_dim ? fd.dim : plan->max_dim;
    if (fd.kind == DFM_SPARSE) plan->h_sparse.push_back(f);
    if (fd.kind == DFM_DENSE) plan->h_dense.push_back(f);
    if (fd.proj) plan->h_proj.push_back(f);
    if (fd.kind == DFM_SEQUENCE || fd.proj || fd.dim != fm_dim) uniform = false;
  }
  plan->total_dim = off;
  // the uniform gather reads rows as 16-byte pieces; decided here, once every field has had its say on `uniform`
  // (inside the loop a width like 6 behind a field of width fm_dim was refused for its stride, in a plan that is not
  // uniform at all)
  for (int f = 0; uniform && f < num_fields; ++f) {
    if (plan->h_fields[f].kind != DFM_DENSE && plan->h_fields[f].stride2 % 4 != 0) {
      delete plan;
      return fail(DFM_ERR_INVALID, "field %d: bad row strides", f);
    }
  }
  if (plan->h_sparse.size() > (size_t)kMaxSparseSlots || plan->h_dense.size() > (size_t)kMaxDenseSlots) uniform = false;
  plan->uniform = uniform ? 1 : 0;
  plan_record_layout(plan);
  auto upload = [](const void* src, size_t bytes, void** dst) -> hipError_t {
    if (bytes == 0) { *dst = nullptr; return hipSuccess; }
    hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  };
  hipError_t e = upload(plan->h_fields.data(), sizeof(dfm_field) * num_fields, (void**)&plan->d_fields);
  if (e == hipSuccess) e = upload(plan->h_sparse.data(), 4 * plan->h_sparse.size(), (void**)&plan->d_sparse);
  if (e == hipSuccess) e = upload(plan->h_dense.data(), 4 * plan->h_dense.size(), (void**)&plan->d_dense);
  if (e == hipSuccess) e = upload(plan->h_proj.data(), 4 * plan->h_proj.size(), (void**)&plan->d_proj);
  if (e == hipSuccess && plan->record_why.empty()) {
    e = upload(plan->h_stage.data(), sizeof(RecordStage) * plan->h_stage.size(), (void**)&plan->d_stage);
    if (e == hipSuccess) e = upload(plan->h_lds_off.data(), 4 * plan->h_lds_off.size(), (void**)&plan->d_lds_off);
  }
  if (e != hipSuccess) {
    dfm_embedding_plan_destroy(plan);
    return fail(DFM_ERR_HIP, "plan upload failed: %s", hipGetErrorString(e));
  }
  *out_plan = plan;
  return DFM_OK;
}

extern "C" int dfm_embedding_plan_destroy(dfm_embedding_plan* plan) {
  if (!plan) return DFM_OK;
  (void)hipFree(plan->d_fields);
  (void)hipFree(plan->d_sparse);
  (void)hipFree(plan->d_dense);
  (void)hipFree(plan->d_proj);
  (void)hipFree(plan->d_stage);
  (void)hipFree(plan->d_lds_off);
  delete plan;
  return DFM_OK;
}

extern "C" int dfm_embedding_plan_is_uniform(const dfm_embedding_plan* plan) { return plan ? plan->uniform : 0; }

extern "C" size_t dfm_embedding_workspace_bytes(const dfm_embedding_plan* plan, int64_t batch) {
  if (!plan || plan->uniform || batch <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(batch) * plan->num_fields;  // fo_parts
}

static int fill_ptrs(const dfm_embedding_plan* plan, const void* const* inputs, PtrTable* t) {
  memset(t, 0, sizeof(*t));
  for (int f = 0; f < plan->num_fields; ++f) {
    DFM_REQUIRE(inputs[f] != nullptr, "input %d is null", f);
    t->p[f] = inputs[f];
  }
  return DFM_OK;
}

// Per-launch kernel timing for bench.py: when armed, the uniform gather is launched with
// hipExtLaunchKernelGGL, whose start/stop events are recorded by the command processor exactly
// around the dispatch (the same interval rocprofv3's kernel trace reports) instead of around the
// host-visible launch call.
namespace {
struct GatherTimer {
  std::vector<hipEvent_t> start, stop;
  int used = 0;
} g_gather_timer;
int g_gather_shape = 0;   // 0 = automatic; tools only (dfm_gather_set_shape)
}  // namespace

// Launch shapes (W waves per workgroup, US sparse + UD dense slots in flight per wave and pass):
//   1: W = 1, 26 + 13 — a lane group owns its sample across all fields: no LDS, no barrier
//   2: W = 2, 13 + 7
//   3: W = 4,  8 + 4
//   4: W = 8,  4 + 2  (round 1's shape; more slots than a pass holds simply take more passes)
//   5: emb_fwd_pair — two waves, compile-time field counts (26 SPARSE + 13 DENSE, D = 16 / 32)
//   6: shape 5 with streaming stores
// Automatic choice: 5 where it applies, else 4.  Shapes 1-3 exist for tools/time_gather.py; where they do not
// apply (a plan without SPARSE or DENSE fields, shape 1 past 26 + 13) the launch takes shape 4.
extern "C" int dfm_gather_set_shape(int shape) {
  DFM_REQUIRE(shape >= 0 && shape <= 6, "gather shape %d outside [0, 6]", shape);
  g_gather_shape = shape;
  return DFM_OK;
}

// One gather launch, fully described: the kernel, its geometry and its argument values.  The same
// description either goes to the stream (optionally with start/stop events attached to the dispatch) or
// rewrites the kernel node of an instantiated graph (dfm_launch).
struct GatherLaunch {
  const void* func = nullptr;
  dim3 grid, block;
  UniformArgs args;
  int ns = 0, nd = 0, F = 0;
  int64_t B = 0;
  float *fo = nullptr, *fe = nullptr, *fm_out = nullptr, *fm_sum = nullptr;
  int32_t* err = nullptr;
  const float* extra_src = nullptr;
  float* extra_dst = nullptr;
  bool pair = false;
  void* params[12];
  void bind() {
    int n = 0;
    params[n++] = &args;
    if (!pair) { params[n++] = &ns; params[n++] = &nd; }
    params[n++] = &B; params[n++] = &F; params[n++] = &fo; params[n++] = &fe; params[n++] = &fm_out;
    params[n++] = &fm_sum; params[n++] = &err; params[n++] = &extra_src; params[n++] = &extra_dst;
  }
};

template <int D>
static int describe_uniform(const dfm_embedding_plan* plan, const PtrTable& in, int64_t B,
                            float* fo, float* fe, float* fm_out, float* fm_sum, int32_t* err,
                            void* const* stage_out, const float* extra_src, float* extra_dst, GatherLaunch* g) {
  constexpr int SPW = kWave / (D / 4);
  memset(&g->args, 0, sizeof(g->args));
  const int ns = static_cast<int>(plan->h_sparse.size()), nd = static_cast<int>(plan->h_dense.size());
  for (int i = 0; i < ns; ++i) {
    const int f = plan->h_sparse[i];
    const dfm_field& fd = plan->h_fields[f];
    g->args.sp[i] = SparseSlot{static_cast<const int64_t*>(in.p[f]), fd.w2, fd.w1, fd.vocab, f, fd.stride2, fd.stride1,
                               stage_out ? static_cast<int64_t*>(stage_out[f]) : nullptr};
  }
  for (int i = 0; i < nd; ++i) {
    const int f = plan->h_dense[i];
    const dfm_field& fd = plan->h_fields[f];
    g->args.de[i] = DenseSlot{static_cast<const float*>(in.p[f]), fd.w2, fd.b2, fd.w1, fd.b1, f, 0,
                              stage_out ? static_cast<float*>(stage_out[f]) : nullptr};
  }
  g->ns = ns; g->nd = nd; g->B = B; g->F = plan->num_fields;
  g->fo = fo; g->fe = fe; g->fm_out = fm_out; g->fm_sum = fm_sum; g->err = err;
  g->extra_src = extra_src; g->extra_dst = extra_dst;
  g->grid = dim3(static_cast<unsigned>((B + SPW - 1) / SPW));
  int shape = g_gather_shape;
  // automatic: the exact-count two-wave kernel for the Criteo field counts (D = 16 / 32), else 8 waves
  const bool pair_ok = (D == 16 || D == 32) && ns == 26 && nd == 13;
  if (shape == 0) shape = pair_ok ? 5 : 4;
  if (shape == 5 && !pair_ok) shape = 4;
  if (shape == 6 && !pair_ok) shape = 4;
  // Shapes 1-3 (tools only) have no variant without SPARSE or without DENSE slots, and shape 1 takes exactly
  // one pass (W == 1): anything it does not cover in that pass goes to shape 4 instead of being dropped.
  if (shape >= 1 && shape <= 3 && (ns == 0 || nd == 0 || (shape == 1 && (ns > 26 || nd > 13)))) shape = 4;
  g->pair = shape == 5 || shape == 6;
#define DFM_UNIFORM_KERNEL(WV, US_, UD_)                                               \
  do {                                                                                 \
    g->func = reinterpret_cast<const void*>(&emb_fwd_uniform<D, WV, US_, UD_>);        \
    g->block = dim3(WV * 64);                                                          \
  } while (0)
  switch (shape) {
    case 1: DFM_UNIFORM_KERNEL(1, 26, 13); break;
    case 2: DFM_UNIFORM_KERNEL(2, 13, 7); break;
    case 3: DFM_UNIFORM_KERNEL(4, 8, 4); break;
    case 5:
      if constexpr (D == 16 || D == 32) {
        g->func = stage_out ? reinterpret_cast<const void*>(&emb_fwd_pair<D, 26, 13, true>)
                            : reinterpret_cast<const void*>(&emb_fwd_pair<D, 26, 13, false>);
        g->block = dim3(128);
      }
      break;
    case 6:     // shape 5 with streaming (nt) stores of field_embeddings
      if constexpr (D == 16 || D == 32) {
        g->func = stage_out ? reinterpret_cast<const void*>(&emb_fwd_pair<D, 26, 13, true, true>)
                            : reinterpret_cast<const void*>(&emb_fwd_pair<D, 26, 13, false, true>);
        g->block = dim3(128);
      }
      break;
    default:
      // a kind with no fields gets no slots: a slot past the end is clamped to slot 0, which would be unset
      if (ns == 0)      DFM_UNIFORM_KERNEL(8, 0, 2);
      else if (nd == 0) DFM_UNIFORM_KERNEL(8, 4, 0);
      else              DFM_UNIFORM_KERNEL(8, 4, 2);
  }
#undef DFM_UNIFORM_KERNEL
  g->bind();
  return DFM_OK;
}

static int describe_gather(const dfm_embedding_plan* plan, const PtrTable& in, int64_t B, float* fo, float* fe,
                           float* fm_out, float* fm_sum, int32_t* err, void* const* stage_out,
                           const float* extra_src, float* extra_dst, GatherLaunch* g) {
#define DFM_DESCRIBE(DD) \
  case DD: return describe_uniform<DD>(plan, in, B, fo, fe, fm_out, fm_sum, err, stage_out, extra_src, extra_dst, g)
  switch (plan->fm_dim) {
    DFM_DESCRIBE(4); DFM_DESCRIBE(8); DFM_DESCRIBE(16); DFM_DESCRIBE(32); DFM_DESCRIBE(64); DFM_DESCRIBE(128); DFM_DESCRIBE(256);
    default: break;
  }
#undef DFM_DESCRIBE
  return fail(DFM_ERR_UNSUPPORTED, "no uniform gather for fm_dim %d", plan->fm_dim);
}

static int launch_gather(GatherLaunch* g, hipStream_t st) {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (g_gather_timer.used < static_cast<int>(g_gather_timer.start.size())) {
    ev0 = g_gather_timer.start[g_gather_timer.used];
    ev1 = g_gather_timer.stop[g_gather_timer.used];
    ++g_gather_timer.used;
  }
  if (ev0) DFM_HIP_TRY(hipExtLaunchKernel(g->func, g->grid, g->block, g->params, 0, st, ev0, ev1, 0));
  else     DFM_HIP_TRY(hipLaunchKernel(g->func, g->grid, g->block, g->params, 0, st));
  return DFM_OK;
}

extern "C" int dfm_embedding_forward(const dfm_embedding_plan* plan, const void* const* inputs, int64_t batch,
                          float* d_first_order, float* d_field_emb, float* d_flat_emb,
                          float* d_fm_out, float* d_fm_sum, void* d_workspace, int32_t* d_error_flag,
                          dfm_stream_t stream) {
  DFM_REQUIRE(plan && inputs && d_first_order && d_field_emb, "null argument");
  DFM_REQUIRE(batch >= 0 && batch < (int64_t(1) << 31), "batch %lld out of range", (long long)batch);
  if (batch == 0) return DFM_OK;
  PtrTable in;
  if (int rc = fill_ptrs(plan, inputs, &in)) return rc;
  hipStream_t st = as_stream(stream);
  if (plan->uniform && (d_flat_emb == nullptr || d_flat_emb == d_field_emb)) {
    GatherLaunch g;
    if (int rc = describe_gather(plan, in, batch, d_first_order, d_field_emb, d_fm_out, d_fm_sum, d_error_flag,
                                 nullptr, nullptr, nullptr, &g)) return rc;
    return launch_gather(&g, st);
  }
  DFM_REQUIRE(d_fm_out == nullptr && d_fm_sum == nullptr, "fused FM outputs need a uniform plan");
  DFM_REQUIRE(d_flat_emb && d_flat_emb != d_field_emb, "general plan needs a separate flat_embeddings buffer");
  DFM_REQUIRE(d_workspace, "general plan needs workspace (dfm_embedding_workspace_bytes)");
  float* fo_parts = static_cast<float*>(d_workspace);
  const int64_t total = batch * plan->num_fields;
  hipLaunchKernelGGL(emb_fwd_general, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st,
                     plan->d_fields, in, batch, plan->num_fields, plan->fm_dim, plan->total_dim,
                     fo_parts, d_field_emb, d_flat_emb, d_error_flag);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(first_order_sum, dim3(static_cast<unsigned>((batch + 255) / 256)), dim3(256), 0, st,
                     fo_parts, batch, plan->num_fields, d_first_order);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

static int fill_grads(const dfm_embedding_plan* plan, const dfm_field_grad* grads, GradTable* gt,
                      bool dense_only) {
  memset(gt, 0, sizeof(*gt));
  for (int f = 0; f < plan->num_fields; ++f) {
    const dfm_field& fd = plan->h_fields[f];
    const dfm_field_grad& g = grads[f];
    if (fd.kind == DFM_DENSE) {
      DFM_REQUIRE(g.w2 && g.b2 && g.w1 && g.b1, "field %d: missing DENSE gradient buffer", f);
    } else if (!dense_only) {
      DFM_REQUIRE(g.w2 && g.w1, "field %d: missing table gradient buffer", f);
    }
    if (fd.proj && !dense_only) DFM_REQUIRE(g.proj, "field %d: missing projection gradient buffer", f);
    gt->g[f] = g;
  }
  return DFM_OK;
}

static int launch_dense_fields(const dfm_embedding_plan* plan, const PtrTable& in, const GradTable& gt,
                               int64_t batch, const float* g_first, const float* g_field,
                               const float* g_flat, hipStream_t st) {
  const int nd = static_cast<int>(plan->h_dense.size());
  if (nd == 0) return DFM_OK;
  if (plan->uniform && g_flat == nullptr && (reinterpret_cast<uintptr_t>(g_field) & 15) == 0) {
    hipLaunchKernelGGL(emb_bwd_dense_fields_uniform, dim3(nd * (plan->fm_dim / 4 + 1)), dim3(256), 0, st, plan->d_dense,
                       in, gt, batch, plan->num_fields, plan->fm_dim, g_first, g_field);
    DFM_LAUNCH_CHECK();
    return DFM_OK;
  }
  hipLaunchKernelGGL(emb_bwd_dense_fields, dim3(nd, plan->max_dim + 1), dim3(256), 0, st,
                     plan->d_fields, plan->d_dense, in, gt, batch, plan->num_fields, plan->fm_dim,
                     plan->total_dim, g_first, g_field, g_flat);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_embedding_backward_dense(const dfm_embedding_plan* plan, const void* const* inputs,
                                 int64_t batch, const float* d_g_first, const float* d_g_field,
                                 const float* d_g_flat, const dfm_field_grad* grads,
                                 const void* d_workspace, dfm_stream_t stream) {
  DFM_REQUIRE(plan && inputs && d_g_first && d_g_field && grads, "null argument");
  DFM_REQUIRE(plan->uniform || d_g_flat, "general plan needs d_g_flat");
  if (batch == 0) return DFM_OK;
  PtrTable in;
  GradTable gt;
  if (int rc = fill_ptrs(plan, inputs, &in)) return rc;
  if (int rc = fill_grads(plan, grads, &gt, false)) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t total = batch * plan->num_fields;
  hipLaunchKernelGGL(emb_bwd_scatter, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st,
                     plan->d_fields, in, gt, batch, plan->num_fields, plan->fm_dim, plan->total_dim,
                     d_g_first, d_g_field, d_g_flat);
  DFM_LAUNCH_CHECK();
  if (int rc = launch_dense_fields(plan, in, gt, batch, d_g_first, d_g_field, d_g_flat, st)) return rc;
  const int np = static_cast<int>(plan->h_proj.size());
  if (np > 0) {
    // projections need the forward's flat_embeddings (raw rows): passed through d_workspace
    DFM_REQUIRE(d_workspace, "projection gradients need the saved flat_embeddings in d_workspace");
    hipLaunchKernelGGL(emb_bwd_proj, dim3(np, plan->fm_dim * plan->max_dim), dim3(256), 0, st,
                       plan->d_fields, plan->d_proj, gt, batch, plan->num_fields, plan->fm_dim,
                       plan->total_dim, plan->max_dim, d_g_field, static_cast<const float*>(d_workspace));
    DFM_LAUNCH_CHECK();
  }
  return DFM_OK;
}

extern "C" int dfm_embedding_backward_dense_fields(const dfm_embedding_plan* plan, const void* const* inputs,
                                        int64_t batch, const float* d_g_first,
                                        const float* d_g_field, const float* d_g_flat,
                                        const dfm_field_grad* grads, dfm_stream_t stream) {
  DFM_REQUIRE(plan && inputs && d_g_first && d_g_field && grads, "null argument");
  if (batch == 0) return DFM_OK;
  PtrTable in;
  GradTable gt;
  if (int rc = fill_ptrs(plan, inputs, &in)) return rc;
  if (int rc = fill_grads(plan, grads, &gt, true)) return rc;
  return launch_dense_fields(plan, in, gt, batch, d_g_first, d_g_field, d_g_flat, as_stream(stream));
}


extern "C" int dfm_embedding_forward_staged(const dfm_embedding_plan* plan, const void* const* inputs,
                                           void* const* stage_out, const float* d_extra_src, float* d_extra_dst,
                                           int64_t batch, float* d_first_order, float* d_field_emb, float* d_fm_out,
                                           float* d_fm_sum, int32_t* d_error_flag, const dfm_launch* at) {
  DFM_CHECK_LAUNCH(at);
  DFM_REQUIRE(plan && inputs && stage_out && d_first_order && d_field_emb, "null argument");
  DFM_REQUIRE(plan->uniform, "staged gather needs a uniform plan");
  DFM_REQUIRE((d_extra_src == nullptr) == (d_extra_dst == nullptr), "extra source and destination go together");
  DFM_REQUIRE(batch >= (repoints(at) ? 1 : 0) && batch < (int64_t(1) << 31), "batch %lld out of range", (long long)batch);
  if (batch == 0) return DFM_OK;
  PtrTable in;
  if (int rc = fill_ptrs(plan, inputs, &in)) return rc;
  for (int f = 0; f < plan->num_fields; ++f)
    DFM_REQUIRE(stage_out[f] != nullptr && stage_out[f] != inputs[f], "stage_out[%d] must be a distinct buffer", f);
  GatherLaunch g;
  if (int rc = describe_gather(plan, in, batch, d_first_order, d_field_emb, d_fm_out, d_fm_sum, d_error_flag,
                               stage_out, d_extra_src, d_extra_dst, &g)) return rc;
  if (repoints(at)) return launch_at(at, g.func, g.grid, g.block, 0, g.params, false);
  return launch_gather(&g, launch_stream(at));   // the timed dispatch exists on the stream path only
}

extern "C" int dfm_gather_timing_begin(int launches) {
  DFM_REQUIRE(launches > 0 && launches <= (1 << 20), "bad launch count");
  DFM_REQUIRE(g_gather_timer.start.empty(), "gather timing already armed");
  g_gather_timer.start.resize(launches);
  g_gather_timer.stop.resize(launches);
  for (int i = 0; i < launches; ++i) {
    DFM_HIP_TRY(hipEventCreate(&g_gather_timer.start[i]));
    DFM_HIP_TRY(hipEventCreate(&g_gather_timer.stop[i]));
  }
  g_gather_timer.used = 0;
  return DFM_OK;
}

extern "C" int dfm_gather_timing_end(float* h_us, int capacity, int* h_count) {
  DFM_REQUIRE(h_count, "null argument");
  const int n = g_gather_timer.used < capacity ? g_gather_timer.used : capacity;
  for (int i = 0; i < g_gather_timer.used; ++i) {
    DFM_HIP_TRY(hipEventSynchronize(g_gather_timer.stop[i]));
    float ms = 0.f;
    DFM_HIP_TRY(hipEventElapsedTime(&ms, g_gather_timer.start[i], g_gather_timer.stop[i]));
    if (i < n && h_us) h_us[i] = ms * 1e3f;
  }
  *h_count = n;
  for (size_t i = 0; i < g_gather_timer.start.size(); ++i) {
    (void)hipEventDestroy(g_gather_timer.start[i]);
    (void)hipEventDestroy(g_gather_timer.stop[i]);
  }
  g_gather_timer.start.clear();
  g_gather_timer.stop.clear();
  g_gather_timer.used = 0;
  return DFM_OK;
}

// ======================================================================================
// record gather (evaluation): any schema, one launch per batch record
// ======================================================================================
// emb_fwd_record<D>: a lane group of LPR = D/4 lanes per (sample, field); lane q owns output dims 4q..4q+3 of the
// field's projected embedding.  A workgroup holds SB whole samples (SB * F * LPR lanes, about 512).
//   1. the projections and the DENSE Linear(1, d) weights and biases are copied into LDS (RecordStage table);
//   2. each lane group reads its field from the record: an id and a 16-byte row piece, a bag pooled piece by
//      piece, or x * w + b from LDS.  Without a projection (d == D) lane q reads piece q, which is its output;
//      with one, every lane of the group walks the row's d/4 pieces (same addresses: one request per piece) and
//      accumulates proj[4q..4q+3, :] . raw from LDS in the order j = 0..d-1 of emb_fwd_general.  Piece p of the
//      raw row goes to flat by lane p % LPR (16-byte stores);
//   3. each lane leaves its 4 output dims and the group its first-order value in LDS; after one barrier the
//      field-0 group of every sample sums them over f = 0..F-1 (fixed order: bitwise reproducible), forms the FM
//      value and finishes with a butterfly over its LPR lanes.
// A wave holds several fields of a sample, so kinds diverge inside a wave; the kernel is latency-bound (tables
// of MovieLens size sit in cache), not issue-bound.
constexpr int kRecordThreads = 512;

// A reason the plan cannot take the record gather, or "" (also fills the LDS staging tables).
static void plan_record_layout(dfm_embedding_plan* plan) {
  const int D = plan->fm_dim, F = plan->num_fields;
  char buf[192];
  plan->record_why.clear();
  plan->h_stage.clear();
  plan->h_lds_off.assign(2 * F, -1);
  if (D != 4 && D != 8 && D != 16 && D != 32 && D != 64) {
    snprintf(buf, sizeof(buf), "fm_embed_dim %d: the record gather takes 4, 8, 16, 32 or 64", D);
    plan->record_why = buf;
    return;
  }
  int off = 0;
  for (int f = 0; f < F; ++f) {
    const dfm_field& fd = plan->h_fields[f];
    const int d = fd.dim;
    if (d % 4) {
      snprintf(buf, sizeof(buf), "field %d: embedding_dim %d is not a multiple of 4", f, d);
      plan->record_why = buf;
      return;
    }
    if (fd.kind != DFM_DENSE && (fd.stride2 % 4 || reinterpret_cast<uintptr_t>(fd.w2) % 16)) {
      snprintf(buf, sizeof(buf), "field %d: table rows are not 16-byte aligned", f);
      plan->record_why = buf;
      return;
    }
    if (fd.proj) {
      plan->h_lds_off[2 * f] = off;
      plan->h_stage.push_back(RecordStage{fd.proj, off, D * d});
      off += D * d;
    }
    if (fd.kind == DFM_DENSE) {   // [w2 (d) | b2 (d) | w1 | b1 | pad to 4]
      plan->h_lds_off[2 * f + 1] = off;
      plan->h_stage.push_back(RecordStage{fd.w2, off, d});
      plan->h_stage.push_back(RecordStage{fd.b2, off + d, d});
      plan->h_stage.push_back(RecordStage{fd.w1, off + 2 * d, 1});
      plan->h_stage.push_back(RecordStage{fd.b1, off + 2 * d + 1, 1});
      off += 2 * d + 4;
    }
  }
  plan->record_param_floats = off;
  if (4 * off > DFM_RECORD_PARAM_LDS_BYTES) {
    snprintf(buf, sizeof(buf), "projection and DENSE parameters take %d bytes of LDS, over the cap of %d",
             4 * off, DFM_RECORD_PARAM_LDS_BYTES);
    plan->record_why = buf;
  }
}

// Quantised fields (dfm_embedding_forward_record_quant; Rec is a record format of quant_records.h, void: there are
// none and the code below is that of the fp32 gather alone).  A field f with qrows[f] set reads records of its own
// width d in {16, 32, 64} instead of its fp32 row and first-order weight:
//   SPARSE    one record: the header (scale, lo, w1) and the payload dword or half dword of piece p;
//   SEQUENCE  ONE walk of the bag per piece: the record brings w1 with the codes, so the first-order walk is gone.
//             The ids of a bag are known before any row arrives and only the additions are ordered, so the walk goes
//             kBagAhead ids at a time: their record loads are issued together, the next kBagAhead ids are requested
//             behind them, and then the values are added in the order l = 0 .. L-1 (id 0 skipped, as above).
// x' = q * scale + lo is a multiply and an add of one rounding each (dequant4: mul_rn, add_rn), also under this file's
// contraction, so every output but fm equals the fp32 gather over the dequantised tables bit for bit.
constexpr int kBagAhead = 8;

// The quantised field fd of sample bc, pieces p0 .. p1 - 1 handed to consume(p, x') in order; returns the field's
// first-order value.  error_flag is NULL on a dead lane.
template <class Rec, class Consume>
__device__ __forceinline__ float record_quant_field(const dfm_field& fd, const uint8_t* qbase, const void* input,
                                                    int64_t bc, int32_t* error_flag, int p0, int p1,
                                                    Consume&& consume) {
  const int d = fd.dim;
  float fo = 0.f;
  if (fd.kind == DFM_SPARSE) {
    const int64_t id = checked_id(static_cast<const int64_t*>(input)[bc], fd.vocab, error_flag);
    const uint8_t* rec = qbase + id * Rec::row_bytes(d);
    for (int p = p0; p < p1; ++p) {
      const auto raw = Rec::load_piece(rec, d, p);
      const float4 h = Rec::widen(raw.head);       // scale, lo, w1, 0
      fo = h.z;
      consume(p, qrec::dequant4<Rec::kBits>(raw.pay, 0, h.x, h.y));
    }
  } else {
    const int L = fd.max_len;
    const int64_t* ids = static_cast<const int64_t*>(input) + bc * L;
    const int64_t rb = Rec::row_bytes(d);
    bool bad = false;
    for (int p = p0; p < p1; ++p) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      float w = 0.f;
      int count = 0;
      bool first = true;
      int64_t next[kBagAhead];
#pragma unroll
      for (int u = 0; u < kBagAhead; ++u) next[u] = L > 0 ? ids[u < L ? u : L - 1] : 0;
      for (int l0 = 0; l0 < L; l0 += kBagAhead) {
        int64_t id[kBagAhead];
        qrec::RawRec<typename Rec::Head> raw[kBagAhead];
#pragma unroll
        for (int u = 0; u < kBagAhead; ++u) {
          const bool oob = next[u] < 0 || next[u] >= fd.vocab;
          bad |= oob && l0 + u < L;
          id[u] = (oob || l0 + u >= L) ? 0 : next[u];
          raw[u] = Rec::load_piece(qbase + id[u] * rb, d, p);      // id 0: record 0, loaded and left alone
        }
#pragma unroll
        for (int u = 0; u < kBagAhead; ++u) {
          const int l = l0 + kBagAhead + u;
          next[u] = ids[l < L ? l : L - 1];
        }
#pragma unroll
        for (int u = 0; u < kBagAhead; ++u) {
          if (id[u] != 0) {
            const float4 h = Rec::widen(raw[u].head);
            const float4 v = qrec::dequant4<Rec::kBits>(raw[u].pay, 0, h.x, h.y);
            if (fd.combiner == DFM_MAX) {
              if (first || v.x > a.x) a.x = v.x;
              if (first || v.y > a.y) a.y = v.y;
              if (first || v.z > a.z) a.z = v.z;
              if (first || v.w > a.w) a.w = v.w;
              if (first || h.z > w) w = h.z;
              first = false;
            } else {
              a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
              w += h.z;
            }
            ++count;
          }
        }
      }
      if (fd.combiner == DFM_MEAN && count > 0) {
        const float c = static_cast<float>(count);
        a.x = a.x / c; a.y = a.y / c; a.z = a.z / c; a.w = a.w / c;
        w = w / c;
      }
      if (p == p0) fo = w;                         // every walk pools the same first-order weights
      consume(p, a);
    }
    if (bad && error_flag) atomicOr(error_flag, 1);
  }
  return fo;
}

template <int D, class Rec>
__device__ __forceinline__ void emb_fwd_record_body(
    const dfm_field* __restrict__ fields, const int32_t* __restrict__ lds_off, const RecordStage* __restrict__ stage,
    int n_stage, int param_floats, const PtrTable& in, const void* const* qrows, int64_t B, int F, int SB,
    float* __restrict__ first_order, float* __restrict__ fe, float* __restrict__ flat, int64_t ld_flat,
    float* __restrict__ fm_out, int32_t* error_flag, const float* __restrict__ labels_src,
    float* __restrict__ labels_dst, float* __restrict__ fm_sum) {
  constexpr int LPR = D / 4;
  constexpr bool kQuant = !std::is_void<Rec>::value;
  extern __shared__ float4 lds4[];
  float* params = reinterpret_cast<float*>(lds4);
  float4* part = lds4 + param_floats / 4;                          // [SB][F][LPR]: each lane's 4 output dims
  float* fo_part = reinterpret_cast<float*>(part + SB * F * LPR);  // [SB][F]
  const int t = threadIdx.x;
  for (int e = 0; e < n_stage; ++e) {
    const RecordStage st = stage[e];
    for (int j = t; j < st.n; j += blockDim.x) params[st.dst + j] = st.src[j];
  }
  __syncthreads();

  const int per = F * LPR;
  const int s = t / per, r = t - s * per, f = r / LPR, q = r - f * LPR;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * SB + s;
  const bool live = b < B;
  const int64_t bc = live ? b : B - 1;   // dead lanes read valid addresses
  const dfm_field fd = fields[f];
  const int d = fd.dim, np = d / 4;
  const float* P = fd.proj ? params + lds_off[2 * f] : nullptr;
  // projection: every piece, all lanes; none: this lane's piece only (d == D)
  const int p0 = P ? 0 : q, p1 = P ? np : q + 1;
  float* flat_row = flat + bc * ld_flat + fd.flat_offset;
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
  float fo = 0.f;

  auto consume = [&](int p, const float4& v) {
    if (live && p % LPR == q) st4(flat_row + 4 * p, v);
    if (!P) { out = v; return; }
    const float* w = P + (4 * q) * d + 4 * p;
    const float4 w0 = *reinterpret_cast<const float4*>(w), w1 = *reinterpret_cast<const float4*>(w + d);
    const float4 w2 = *reinterpret_cast<const float4*>(w + 2 * d), w3 = *reinterpret_cast<const float4*>(w + 3 * d);
    out.x = fmaf(v.w, w0.w, fmaf(v.z, w0.z, fmaf(v.y, w0.y, fmaf(v.x, w0.x, out.x))));
    out.y = fmaf(v.w, w1.w, fmaf(v.z, w1.z, fmaf(v.y, w1.y, fmaf(v.x, w1.x, out.y))));
    out.z = fmaf(v.w, w2.w, fmaf(v.z, w2.z, fmaf(v.y, w2.y, fmaf(v.x, w2.x, out.z))));
    out.w = fmaf(v.w, w3.w, fmaf(v.z, w3.z, fmaf(v.y, w3.y, fmaf(v.x, w3.x, out.w))));
  };

  const uint8_t* qbase = nullptr;
  if constexpr (kQuant) qbase = static_cast<const uint8_t*>(qrows[f]);
  if (kQuant && qbase) {
    if constexpr (kQuant) fo = record_quant_field<Rec>(fd, qbase, in.p[f], bc, live ? error_flag : nullptr, p0, p1, consume);
  } else if (fd.kind == DFM_SPARSE) {
    const int64_t id = checked_id(static_cast<const int64_t*>(in.p[f])[bc], fd.vocab, live ? error_flag : nullptr);
    const float* row = fd.w2 + id * fd.stride2;
    fo = fd.w1[id * fd.stride1];
    for (int p = p0; p < p1; ++p) consume(p, ld4(row + 4 * p));
  } else if (fd.kind == DFM_DENSE) {
    const float x = static_cast<const float*>(in.p[f])[bc];
    const float* dw = params + lds_off[2 * f + 1];
    fo = fmaf(x, dw[2 * d], dw[2 * d + 1]);
    for (int p = p0; p < p1; ++p) {
      const float4 w = *reinterpret_cast<const float4*>(dw + 4 * p);
      const float4 c = *reinterpret_cast<const float4*>(dw + d + 4 * p);
      consume(p, make_float4(fmaf(x, w.x, c.x), fmaf(x, w.y, c.y), fmaf(x, w.z, c.z), fmaf(x, w.w, c.w)));
    }
  } else {
    // bag_pool of emb_fwd_general, 4 columns at a time: id 0 skipped, mean over the non-padding ids, max per
    // column, an all-padding bag gives zeros
    const int L = fd.max_len;
    const int64_t* ids = static_cast<const int64_t*>(in.p[f]) + bc * L;
    int count = 0;
    bool first = true;
    for (int l = 0; l < L; ++l) {
      const int64_t id = checked_id(ids[l], fd.vocab, live ? error_flag : nullptr);
      if (id == 0) continue;
      const float v = fd.w1[id * fd.stride1];
      if (fd.combiner == DFM_MAX) { if (first || v > fo) fo = v; first = false; }
      else fo += v;
      ++count;
    }
    if (fd.combiner == DFM_MEAN && count > 0) fo = fo / static_cast<float>(count);
    for (int p = p0; p < p1; ++p) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      first = true;
      for (int l = 0; l < L; ++l) {
        int64_t id = ids[l];
        id = (id < 0 || id >= fd.vocab) ? 0 : id;      // flagged above
        if (id == 0) continue;
        const float4 v = ld4(fd.w2 + id * fd.stride2 + 4 * p);
        if (fd.combiner == DFM_MAX) {
          if (first || v.x > a.x) a.x = v.x;
          if (first || v.y > a.y) a.y = v.y;
          if (first || v.z > a.z) a.z = v.z;
          if (first || v.w > a.w) a.w = v.w;
          first = false;
        } else {
          a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
      }
      if (fd.combiner == DFM_MEAN && count > 0) {
        const float c = static_cast<float>(count);
        a.x = a.x / c; a.y = a.y / c; a.z = a.z / c; a.w = a.w / c;
      }
      consume(p, a);
    }
  }
  if (live && fe) st4(fe + (b * F + f) * D + 4 * q, out);
  part[t] = out;
  if (q == 0) fo_part[s * F + f] = fo;
  __syncthreads();
  if (f != 0) return;
  // the field-0 lane group of sample s: sums over the fields in order f = 0..F-1
  float4 S = make_float4(0.f, 0.f, 0.f, 0.f), SQ = make_float4(0.f, 0.f, 0.f, 0.f);
  float fsum = 0.f;
  for (int g = 0; g < F; ++g) {
    const float4 e = part[(s * F + g) * LPR + q];
    S.x += e.x; S.y += e.y; S.z += e.z; S.w += e.w;
    SQ.x = fmaf(e.x, e.x, SQ.x); SQ.y = fmaf(e.y, e.y, SQ.y);
    SQ.z = fmaf(e.z, e.z, SQ.z); SQ.w = fmaf(e.w, e.w, SQ.w);
    fsum += fo_part[s * F + g];
  }
  // S = sum_f e for a training step's FM backward (the uniform gather's fm_sum): lane q's 4 dims, one 16-byte store
  if (live && fm_sum) st4(fm_sum + b * D + 4 * q, S);
  float v = (S.x * S.x - SQ.x) + (S.y * S.y - SQ.y) + (S.z * S.z - SQ.z) + (S.w * S.w - SQ.w);
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) v += __shfl_xor(v, m, kWave);
  if (live && q == 0) {
    first_order[b] = fsum;
    if (fm_out) fm_out[b] = 0.5f * v;
    if (labels_dst) labels_dst[b] = labels_src[b];
  }
}

template <int D>
__global__ __launch_bounds__(1024) void emb_fwd_record(
    const dfm_field* __restrict__ fields, const int32_t* __restrict__ lds_off, const RecordStage* __restrict__ stage,
    int n_stage, int param_floats, PtrTable in, int64_t B, int F, int SB, float* __restrict__ first_order,
    float* __restrict__ fe, float* __restrict__ flat, int64_t ld_flat, float* __restrict__ fm_out,
    int32_t* error_flag, const float* __restrict__ labels_src, float* __restrict__ labels_dst,
    float* __restrict__ fm_sum) {
  emb_fwd_record_body<D, void>(fields, lds_off, stage, n_stage, param_floats, in, nullptr, B, F, SB, first_order, fe,
                               flat, ld_flat, fm_out, error_flag, labels_src, labels_dst, fm_sum);
}

// The same launch with a table of record bases behind the arguments (qrows.p[f] NULL: field f is read in fp32).
template <int D, class Rec>
__global__ __launch_bounds__(1024) void emb_fwd_record_quant(
    const dfm_field* __restrict__ fields, const int32_t* __restrict__ lds_off, const RecordStage* __restrict__ stage,
    int n_stage, int param_floats, PtrTable in, int64_t B, int F, int SB, float* __restrict__ first_order,
    float* __restrict__ fe, float* __restrict__ flat, int64_t ld_flat, float* __restrict__ fm_out,
    int32_t* error_flag, const float* __restrict__ labels_src, float* __restrict__ labels_dst,
    float* __restrict__ fm_sum, PtrTable qrows) {
  emb_fwd_record_body<D, Rec>(fields, lds_off, stage, n_stage, param_floats, in, qrows.p, B, F, SB, first_order, fe,
                              flat, ld_flat, fm_out, error_flag, labels_src, labels_dst, fm_sum);
}

// One record-gather launch, fully described.
struct RecordLaunch {
  const void* func = nullptr;
  dim3 grid, block;
  unsigned lds = 0;
  const dfm_field* fields = nullptr;
  const int32_t* lds_off = nullptr;
  const RecordStage* stage = nullptr;
  int n_stage = 0, param_floats = 0;
  PtrTable in;
  int64_t B = 0;
  int F = 0, SB = 0;
  float *fo = nullptr, *fe = nullptr, *flat = nullptr;
  int64_t ld_flat = 0;
  float* fm = nullptr;
  int32_t* err = nullptr;
  const float* labels_src = nullptr;
  float* labels_dst = nullptr;
  float* fm_sum = nullptr;
  PtrTable qrows;                   // emb_fwd_record_quant's last argument; emb_fwd_record has none there
  void* params[19];
  void bind() {
    void* p[] = {&fields, &lds_off, &stage, &n_stage, &param_floats, &in, &B, &F, &SB, &fo, &fe, &flat, &ld_flat,
                 &fm, &err, &labels_src, &labels_dst, &fm_sum, &qrows};
    static_assert(sizeof(p) / sizeof(p[0]) <= sizeof(params) / sizeof(params[0]), "params");
    for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i) params[i] = p[i];
  }
};

// Every field's input inside one batch record in the mixed layout (data/packed.py:RecordLayout) -> in; returns the
// record's labels.
static const float* record_inputs(const dfm_embedding_plan* plan, const void* d_record, int64_t batch, PtrTable* in) {
  int ns = 0, nd = 0;
  for (const dfm_field& fd : plan->h_fields) { ns += fd.kind == DFM_SPARSE; nd += fd.kind == DFM_DENSE; }
  const int64_t o1 = static_cast<int64_t>(ns > 0 ? ns : 1) * batch * 8;
  const int64_t o2 = o1 + static_cast<int64_t>(nd > 0 ? nd : 1) * batch * 4;
  int64_t oq = (o2 + batch * 4 + 15) / 16 * 16;
  const char* rec = static_cast<const char*>(d_record);
  memset(in, 0, sizeof(*in));
  int si = 0, di = 0;
  for (int f = 0; f < plan->num_fields; ++f) {
    const dfm_field& fd = plan->h_fields[f];
    if (fd.kind == DFM_SPARSE) {
      in->p[f] = rec + static_cast<int64_t>(si++) * batch * 8;
    } else if (fd.kind == DFM_DENSE) {
      in->p[f] = rec + o1 + static_cast<int64_t>(di++) * batch * 4;
    } else {
      in->p[f] = rec + oq;
      oq = (oq + batch * fd.max_len * 8 + 15) / 16 * 16;
    }
  }
  return reinterpret_cast<const float*>(rec + o2);
}

static int describe_record(const dfm_embedding_plan* plan, const void* d_record, int64_t batch, float* fo, float* fe,
                           float* flat, int64_t ld_flat, float* fm, float* fm_sum, float* labels_out, int32_t* err,
                           RecordLaunch* g) {
  DFM_REQUIRE(plan && d_record && fo && flat, "null argument");
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(fm_sum) % 16 == 0, "fm_sum must be 16-byte aligned");
  if (!plan->record_why.empty()) return fail(DFM_ERR_UNSUPPORTED, "record gather: %s", plan->record_why.c_str());
  DFM_REQUIRE(batch > 0 && batch < (int64_t(1) << 31), "batch %lld out of range", (long long)batch);
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(d_record) % 16 == 0, "batch records must be 16-byte aligned");
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(flat) % 16 == 0 && ld_flat % 4 == 0 && ld_flat >= plan->total_dim,
              "flat rows must be 16-byte aligned with ld_flat %% 4 == 0 and ld_flat >= %d", plan->total_dim);
  DFM_REQUIRE(!fe || reinterpret_cast<uintptr_t>(fe) % 16 == 0, "field embeddings must be 16-byte aligned");
  const int F = plan->num_fields, D = plan->fm_dim, LPR = D / 4;
  const float* labels = record_inputs(plan, d_record, batch, &g->in);
  const int per = F * LPR;
  const int SB = per >= kRecordThreads ? 1 : kRecordThreads / per;
  g->fields = plan->d_fields; g->lds_off = plan->d_lds_off; g->stage = plan->d_stage;
  g->n_stage = static_cast<int>(plan->h_stage.size());
  g->param_floats = plan->record_param_floats;
  g->B = batch; g->F = F; g->SB = SB;
  g->fo = fo; g->fe = fe; g->flat = flat; g->ld_flat = ld_flat; g->fm = fm; g->err = err;
  g->labels_src = labels_out ? labels : nullptr;
  g->labels_dst = labels_out;
  g->fm_sum = fm_sum;
  g->grid = dim3(static_cast<unsigned>((batch + SB - 1) / SB));
  g->block = dim3(static_cast<unsigned>(SB * per));
  g->lds = static_cast<unsigned>(4 * (g->param_floats + SB * F * D + SB * F));
  switch (D) {
    case 4: g->func = reinterpret_cast<const void*>(&emb_fwd_record<4>); break;
    case 8: g->func = reinterpret_cast<const void*>(&emb_fwd_record<8>); break;
    case 16: g->func = reinterpret_cast<const void*>(&emb_fwd_record<16>); break;
    case 32: g->func = reinterpret_cast<const void*>(&emb_fwd_record<32>); break;
    default: g->func = reinterpret_cast<const void*>(&emb_fwd_record<64>); break;
  }
  g->bind();
  return DFM_OK;
}

extern "C" int dfm_embedding_forward_record(const dfm_embedding_plan* plan, const void* d_record, int64_t batch,
                                            float* d_first_order, float* d_field_emb, float* d_flat, int64_t ld_flat,
                                            float* d_fm_out, float* d_fm_sum, float* d_labels_out,
                                            int32_t* d_error_flag, const dfm_launch* at) {
  DFM_CHECK_LAUNCH(at);
  RecordLaunch g;
  if (int rc = describe_record(plan, d_record, batch, d_first_order, d_field_emb, d_flat, ld_flat, d_fm_out, d_fm_sum,
                               d_labels_out, d_error_flag, &g)) return rc;
  return launch_at(at, g.func, g.grid, g.block, g.lds, g.params, false);
}

template <class Rec>
static const void* record_quant_kernel(int D) {
  switch (D) {
    case 4: return reinterpret_cast<const void*>(&emb_fwd_record_quant<4, Rec>);
    case 8: return reinterpret_cast<const void*>(&emb_fwd_record_quant<8, Rec>);
    case 16: return reinterpret_cast<const void*>(&emb_fwd_record_quant<16, Rec>);
    case 32: return reinterpret_cast<const void*>(&emb_fwd_record_quant<32, Rec>);
    default: return reinterpret_cast<const void*>(&emb_fwd_record_quant<64, Rec>);
  }
}

extern "C" int dfm_embedding_forward_record_quant(const dfm_embedding_plan* plan, const void* const* quant_rows,
                                                  int format, const void* d_record, int64_t batch,
                                                  float* d_first_order, float* d_field_emb, float* d_flat,
                                                  int64_t ld_flat, float* d_fm_out, float* d_fm_sum,
                                                  float* d_labels_out, int32_t* d_error_flag, const dfm_launch* at) {
  DFM_CHECK_LAUNCH(at);
  DFM_REQUIRE(plan && quant_rows, "null argument");
  if (format != DFM_QUANT_INT8_ROWWISE && format != DFM_QUANT_UINT4_ROWWISE)
    return fail(DFM_ERR_UNSUPPORTED, "quantised format %d: DFM_QUANT_INT8_ROWWISE and DFM_QUANT_UINT4_ROWWISE only", format);
  RecordLaunch g;
  if (int rc = describe_record(plan, d_record, batch, d_first_order, d_field_emb, d_flat, ld_flat, d_fm_out, d_fm_sum,
                               d_labels_out, d_error_flag, &g)) return rc;
  memset(&g.qrows, 0, sizeof(g.qrows));
  for (int f = 0; f < plan->num_fields; ++f) {
    if (!quant_rows[f]) continue;
    const dfm_field& fd = plan->h_fields[f];
    if (fd.kind == DFM_DENSE)
      return fail(DFM_ERR_UNSUPPORTED, "field %d: a DENSE field has no table to quantise (quant_rows[%d] must be NULL)", f, f);
    if (fd.dim != 16 && fd.dim != 32 && fd.dim != 64)
      return fail(DFM_ERR_UNSUPPORTED, "field %d: quantised tables of width %d: widths 16, 32 and 64 only", f, fd.dim);
    DFM_REQUIRE(reinterpret_cast<uintptr_t>(quant_rows[f]) % 16 == 0, "field %d: records must be 16-byte aligned", f);
    g.qrows.p[f] = quant_rows[f];
  }
  // the formats' loads and headers do not depend on the trait's width: the record gather passes each field's own
  g.func = format == DFM_QUANT_UINT4_ROWWISE ? record_quant_kernel<qrec::Uint4Rec<16>>(plan->fm_dim)
                                             : record_quant_kernel<qrec::Int8Rec<16>>(plan->fm_dim);
  return launch_at(at, g.func, g.grid, g.block, g.lds, g.params, false);
}

// ======================================================================================
// record backward (training with the tables as dense parameters): any schema, one launch, no atomics
// ======================================================================================
// emb_bwd_record<D>: the gradient of every embedding parameter from the upstream gradients of dfm_embedding_forward_record's
// outputs, as `parts` batch slices that the owner of the flat gradient buffer adds in slice order (a dfm_slab_ref).
// Row-owned scan: the tables this path is for are small (MovieLens: 3 112 rows in all), so a thread owns kBwdRows
// table rows (one 16-byte piece of them, or the first-order scalar) and walks the slice's ids; no sort, no atomics,
// and a row nobody names is stored as 0 — the kernel owns the whole gradient, there is no memset.
// A workgroup is one of
//   table job (field, row tile, slice):  per stage of kBwdStage samples, (1) the ids go to LDS as int32, padding and
//     out-of-range ids as -1; (2) the per-(sample, field) vector g_flat slice + P^T g_field (P staged in LDS once; no
//     projection: + g_field), times 1 / count for a mean bag, is formed by one thread per 16-byte piece and left in
//     LDS with g_first behind it; (3) every thread walks the ids in (sample, position) order — four LDS reads of the
//     vectors in flight per 16-byte read of ids, the id made wave-uniform so that a tile none of whose rows is named
//     skips the adds on a scalar branch — and adds the vector of a sample that names its row (select, not multiply);
//   DENSE job (field, slice): the same staging, then thread j sums x * g[:, j] and g[:, j] over the samples in order
//     (j == d: the first-order Linear);
//   projection job (field, 256 outputs, slice): g_field and the saved flat rows staged in LDS, thread (k, j) sums
//     g_field[b, f, k] * flat[b, off + j] over the samples in order.
// Sums inside a slice run in sample order and slices are added in slice order: bitwise reproducible.
namespace {
constexpr int kBwdThreads = 256;
constexpr int kBwdStage = 256;      // samples in LDS at a time
constexpr int kBwdMaxParts = 16;    // batch slices: one slab reference of the optimizer's prepare launch
constexpr int kBwdRows = 2;         // table rows per thread
constexpr unsigned kBwdMaxLds = 65536;

struct BwdJobs {
  int32_t first[DFM_MAX_FIELDS + 1];    // field f: workgroups [first[f], first[f + 1]) = tiles[f] * parts, slice-major
  int32_t tiles[DFM_MAX_FIELDS];
  int32_t pfirst[DFM_MAX_FIELDS + 1];   // projection i (plan->h_proj order), behind first[F]: chunks[i] * parts
  int32_t chunks[DFM_MAX_FIELDS];
};
// where each gradient starts inside a slice (floats from d_grad_base)
struct BwdOffsets {
  int32_t w2[DFM_MAX_FIELDS], b2[DFM_MAX_FIELDS], w1[DFM_MAX_FIELDS], b1[DFM_MAX_FIELDS], proj[DFM_MAX_FIELDS];
};
__device__ __forceinline__ void add_if(float4& acc, bool m, const float4& v) {
  acc.x += m ? v.x : 0.f; acc.y += m ? v.y : 0.f; acc.z += m ? v.z : 0.f; acc.w += m ? v.w : 0.f;
}
}  // namespace

// FM: the variant with the FM backward folded in (emb_bwd_record_fm): wherever the field gradient is read it is
//   g_eff[b, f, :] = g_field[b, f, :] + g_fm[b] * (S[b, :] - e[b, f, :])        (fm.py:18-23; S = sum_f e)
// with g_field optional (absent: 0) and the trio (g_fm, fm_sum, field_emb) optional (absent: g_field alone).  The
// product is rounded before the add (no contraction): the bits of dfm_fm_backward's d e added to g_field.
template <int D, bool FM>
__device__ __forceinline__ void emb_bwd_record_body(
    const dfm_field* __restrict__ fields, const int32_t* __restrict__ proj_list, const PtrTable& in,
    const BwdJobs& jobs, const BwdOffsets& go, int64_t B, int F, int parts, int64_t rows_per_part, int64_t elems,
    const float* __restrict__ g_first, const float* __restrict__ g_field, const float* __restrict__ g_flat,
    int64_t ld_g, const float* __restrict__ flat_saved, int64_t ld_flat, float* __restrict__ partial,
    const float* __restrict__ g_fm, const float* __restrict__ fm_sum, const float* __restrict__ field_emb) {
  extern __shared__ float4 lds4[];
  const int t = threadIdx.x;
  const int blk = blockIdx.x;
  // 16 bytes (dims 4 k4 .. 4 k4 + 3) of the effective gradient of field ff of sample b
  auto field_grad = [&](int64_t b, int ff, int k4) -> float4 {
    if constexpr (!FM) {
      return ld4(g_field + (b * F + ff) * D + 4 * k4);
    } else {
#pragma clang fp contract(off)
      float4 e = g_field ? ld4(g_field + (b * F + ff) * D + 4 * k4) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (g_fm) {
        const float gm = g_fm[b];
        const float4 s4 = ld4(fm_sum + b * D + 4 * k4), e4 = ld4(field_emb + (b * F + ff) * D + 4 * k4);
        const float4 m = make_float4(gm * (s4.x - e4.x), gm * (s4.y - e4.y), gm * (s4.z - e4.z), gm * (s4.w - e4.w));
        if (g_field) { e.x += m.x; e.y += m.y; e.z += m.z; e.w += m.w; }
        else e = m;
      }
      return e;
    }
  };
  if (blk >= jobs.first[F]) {
    // ---- projection job ----
    int local = blk - jobs.first[F], pi = 0;
    while (local >= jobs.pfirst[pi + 1]) ++pi;
    local -= jobs.pfirst[pi];
    const int chunks = jobs.chunks[pi], part = local / chunks, oc = local - part * chunks;
    const int f = proj_list[pi];
    const dfm_field fd = fields[f];
    const int d = fd.dim, np = d / 4;
    const int o = oc * kBwdThreads + t;
    const bool valid = o < D * d;
    const int k = valid ? o / d : 0, j = valid ? o - k * d : 0;
    const float* gf = reinterpret_cast<const float*>(lds4);          // [kBwdStage][D]
    const float* fl = gf + kBwdStage * D;                            // [kBwdStage][d]
    const int64_t b_lo = part * rows_per_part, b_hi = b_lo + rows_per_part < B ? b_lo + rows_per_part : B;
    float acc = 0.f;
    for (int64_t s0 = b_lo; s0 < b_hi; s0 += kBwdStage) {
      const int n = static_cast<int>(b_hi - s0 < kBwdStage ? b_hi - s0 : kBwdStage);
      __syncthreads();
      for (int i = t; i < n * (D / 4); i += kBwdThreads) {
        const int s = i / (D / 4), p = i - s * (D / 4);
        lds4[i] = field_grad(s0 + s, f, p);
      }
      for (int i = t; i < n * np; i += kBwdThreads) {
        const int s = i / np, p = i - s * np;
        lds4[kBwdStage * (D / 4) + i] = ld4(flat_saved + (s0 + s) * ld_flat + fd.flat_offset + 4 * p);
      }
      __syncthreads();
      if (valid)
        for (int s = 0; s < n; ++s) acc = fmaf(gf[s * D + k], fl[s * d + j], acc);
    }
    if (valid) partial[part * elems + go.proj[f] + o] = acc;
    return;
  }
  int f = 0;
  while (blk >= jobs.first[f + 1]) ++f;
  const int local = blk - jobs.first[f];
  const int ntiles = jobs.tiles[f], part = local / ntiles, tile = local - part * ntiles;
  const dfm_field fd = fields[f];
  const int d = fd.dim, np = d / 4, pieces = np + 1;
  const bool bag = fd.kind == DFM_SEQUENCE, dense = fd.kind == DFM_DENSE;
  const int L = bag ? fd.max_len : 1;
  const int V = fd.vocab;
  float* gv = reinterpret_cast<float*>(lds4);                                   // [kBwdStage][d + 4]: vector | g_first
  int32_t* lids = reinterpret_cast<int32_t*>(lds4 + kBwdStage * pieces);        // [kBwdStage * L] (+ pad); DENSE: x
  float* xs = reinterpret_cast<float*>(lids);
  float* P = reinterpret_cast<float*>(lds4 + kBwdStage * pieces + (kBwdStage * L + 3) / 4 + 1);   // [D][d]
  if (fd.proj)
    for (int i = t; i < D * d; i += kBwdThreads) P[i] = fd.proj[i];
  const int64_t b_lo = part * rows_per_part, b_hi = b_lo + rows_per_part < B ? b_lo + rows_per_part : B;
  float* out = partial + part * elems;

  // table job: row slots
  const int rpp = kBwdThreads / pieces;
  const int slot = t / pieces, q = t - slot * pieces;
  const bool active = slot < rpp;
  const int tile_lo = tile * rpp * kBwdRows;
  const int tile_hi = tile_lo + rpp * kBwdRows < V ? tile_lo + rpp * kBwdRows : V;
  const int row0 = active ? tile_lo + slot : -2, row1 = active ? tile_lo + rpp + slot : -2;
  float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = acc0;
  float sw = 0.f, sb = 0.f;        // DENSE job, thread j = t <= d

  for (int64_t s0 = b_lo; s0 < b_hi; s0 += kBwdStage) {
    const int n = static_cast<int>(b_hi - s0 < kBwdStage ? b_hi - s0 : kBwdStage);
    const int total = n * L, total4 = (total + 3) & ~3;
    __syncthreads();               // the previous stage has been consumed (first stage: P is in LDS)
    if (dense) {
      const float* x = static_cast<const float*>(in.p[f]);
      for (int i = t; i < n; i += kBwdThreads) xs[i] = x[s0 + i];
    } else {
      const int64_t* ids = static_cast<const int64_t*>(in.p[f]) + s0 * L;
      for (int i = t; i < total4; i += kBwdThreads) {
        int32_t v = -1;
        if (i < total) {
          const int64_t id = ids[i];
          if (id > 0 && id < V) v = static_cast<int32_t>(id);
        }
        lids[i] = v;
      }
    }
    __syncthreads();
    for (int i = t; i < n * pieces; i += kBwdThreads) {
      const int s = i / pieces, p = i - s * pieces;
      const int64_t b = s0 + s;
      float scale = 1.f;
      if (bag && fd.combiner == DFM_MEAN) {
        int count = 0;
        for (int l = 0; l < L; ++l) count += lids[s * L + l] >= 0 ? 1 : 0;
        scale = count > 0 ? 1.f / static_cast<float>(count) : 0.f;
      }
      float4 g;
      if (p == np) {
        g = make_float4(g_first[b], 0.f, 0.f, 0.f);
      } else {
        g = ld4(g_flat + b * ld_g + fd.flat_offset + 4 * p);
        if (fd.proj) {
          // raw_grad's order: g = fmaf(g_field[k], P[k, j], g), k = 0 .. D-1
#pragma unroll
          for (int k4 = 0; k4 < D / 4; ++k4) {
            const float4 e = field_grad(b, f, k4);
            const float ek[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const float4 w = *reinterpret_cast<const float4*>(P + (4 * k4 + u) * d + 4 * p);
              g.x = fmaf(ek[u], w.x, g.x); g.y = fmaf(ek[u], w.y, g.y);
              g.z = fmaf(ek[u], w.z, g.z); g.w = fmaf(ek[u], w.w, g.w);
            }
          }
        } else {
          const float4 e = field_grad(b, f, p);
          g.x += e.x; g.y += e.y; g.z += e.z; g.w += e.w;
        }
      }
      if (bag) { g.x *= scale; g.y *= scale; g.z *= scale; g.w *= scale; }
      lds4[i] = g;                 // == gv[s * (d + 4) + 4 * p]
    }
    __syncthreads();
    if (dense) {
      if (t <= d)
        for (int s = 0; s < n; ++s) {
          const float g = gv[s * (d + 4) + t];
          sw = fmaf(xs[s], g, sw);
          sb += g;
        }
      continue;
    }
    const int4* ids4 = reinterpret_cast<const int4*>(lids);
    const float4* gvq = lds4 + q;
    int s = 0, l = 0;
    for (int i = 0; i < total; i += 4) {
      const int4 w = ids4[i >> 2];
      const int wid[4] = {w.x, w.y, w.z, w.w};
      float4 v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        v[c] = gvq[(s < n ? s : n - 1) * pieces];
        if (++l == L) { l = 0; ++s; }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int id = __builtin_amdgcn_readfirstlane(wid[c]);
        if (id >= tile_lo && id < tile_hi) {
          add_if(acc0, id == row0, v[c]);
          add_if(acc1, id == row1, v[c]);
        }
      }
    }
  }
  if (dense) {
    if (t < d) { out[go.w2[f] + t] = sw; out[go.b2[f] + t] = sb; }
    else if (t == d) { out[go.w1[f]] = sw; out[go.b1[f]] = sb; }
    return;
  }
  if (row0 >= 0 && row0 < V) {
    if (q < np) st4(out + go.w2[f] + static_cast<int64_t>(row0) * d + 4 * q, acc0);
    else out[go.w1[f] + row0] = acc0.x;
  }
  if (row1 >= 0 && row1 < V) {
    if (q < np) st4(out + go.w2[f] + static_cast<int64_t>(row1) * d + 4 * q, acc1);
    else out[go.w1[f] + row1] = acc1.x;
  }
}

template <int D>
__global__ __launch_bounds__(kBwdThreads) void emb_bwd_record(
    const dfm_field* __restrict__ fields, const int32_t* __restrict__ proj_list, PtrTable in, BwdJobs jobs,
    BwdOffsets go, int64_t B, int F, int parts, int64_t rows_per_part, int64_t elems,
    const float* __restrict__ g_first, const float* __restrict__ g_field, const float* __restrict__ g_flat,
    int64_t ld_g, const float* __restrict__ flat_saved, int64_t ld_flat, float* __restrict__ partial) {
  emb_bwd_record_body<D, false>(fields, proj_list, in, jobs, go, B, F, parts, rows_per_part, elems, g_first, g_field,
                                g_flat, ld_g, flat_saved, ld_flat, partial, nullptr, nullptr, nullptr);
}

template <int D>
__global__ __launch_bounds__(kBwdThreads) void emb_bwd_record_fm(
    const dfm_field* __restrict__ fields, const int32_t* __restrict__ proj_list, PtrTable in, BwdJobs jobs,
    BwdOffsets go, int64_t B, int F, int parts, int64_t rows_per_part, int64_t elems,
    const float* __restrict__ g_first, const float* __restrict__ g_field, const float* __restrict__ g_flat,
    int64_t ld_g, const float* __restrict__ flat_saved, int64_t ld_flat, float* __restrict__ partial,
    const float* __restrict__ g_fm, const float* __restrict__ fm_sum, const float* __restrict__ field_emb) {
  emb_bwd_record_body<D, true>(fields, proj_list, in, jobs, go, B, F, parts, rows_per_part, elems, g_first, g_field,
                               g_flat, ld_g, flat_saved, ld_flat, partial, g_fm, fm_sum, field_emb);
}

namespace {
struct BwdRecordLaunch {
  const void* func = nullptr;
  dim3 grid, block;
  unsigned lds = 0;
  const dfm_field* fields = nullptr;
  const int32_t* proj_list = nullptr;
  PtrTable in;
  BwdJobs jobs;
  BwdOffsets go;
  int64_t B = 0, rows_per_part = 0, elems = 0, ld_g = 0, ld_flat = 0;
  int F = 0, parts = 0;
  const float *g_first = nullptr, *g_field = nullptr, *g_flat = nullptr, *flat_saved = nullptr;
  float* partial = nullptr;
  const float *g_fm = nullptr, *fm_sum = nullptr, *field_emb = nullptr;    // emb_bwd_record_fm only
  void* params[20];
  void bind() {
    void* p[] = {&fields, &proj_list, &in, &jobs, &go, &B, &F, &parts, &rows_per_part, &elems, &g_first, &g_field,
                 &g_flat, &ld_g, &flat_saved, &ld_flat, &partial, &g_fm, &fm_sum, &field_emb};
    static_assert(sizeof(p) / sizeof(p[0]) == sizeof(params) / sizeof(params[0]), "params");
    for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i) params[i] = p[i];
  }
};

inline int bwd_parts(int64_t batch) {
  const int64_t stages = (batch + kBwdStage - 1) / kBwdStage;
  return static_cast<int>(stages < 1 ? 1 : (stages > kBwdMaxParts ? kBwdMaxParts : stages));
}

int describe_bwd_record(const dfm_embedding_plan* plan, const void* d_record, int64_t batch, const float* g_first,
                        const float* g_field, const float* g_flat, int64_t ld_g, const float* flat_saved,
                        int64_t ld_flat, const float* g_fm, const float* fm_sum, const float* field_emb, bool fm,
                        const dfm_field_grad* grads, const float* base, int64_t elems, void* ws, BwdRecordLaunch* g) {
  DFM_REQUIRE(plan && d_record && g_first && (g_field || fm) && g_flat && grads && base && ws, "null argument");
  DFM_REQUIRE(fm || !(g_fm || fm_sum || field_emb), "the FM term needs fold_fm != 0");
  DFM_REQUIRE((!g_fm && !fm_sum && !field_emb) || (g_fm && fm_sum && field_emb),
              "the FM term needs g_fm, fm_sum and field_embeddings together");
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(fm_sum) % 16 == 0 && reinterpret_cast<uintptr_t>(field_emb) % 16 == 0,
              "fm_sum and field_embeddings must be 16-byte aligned");
  if (!plan->record_why.empty()) return fail(DFM_ERR_UNSUPPORTED, "record backward: %s", plan->record_why.c_str());
  DFM_REQUIRE(batch > 0 && batch < (int64_t(1) << 31), "batch %lld out of range", (long long)batch);
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(d_record) % 16 == 0, "batch records must be 16-byte aligned");
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(g_flat) % 16 == 0 && ld_g % 4 == 0 && ld_g >= plan->total_dim &&
                  reinterpret_cast<uintptr_t>(g_field) % 16 == 0,
              "upstream gradients must be 16-byte aligned, ld_g_flat %% 4 == 0 and >= %d", plan->total_dim);
  DFM_REQUIRE(plan->h_proj.empty() || (flat_saved && reinterpret_cast<uintptr_t>(flat_saved) % 16 == 0 &&
                                       ld_flat % 4 == 0 && ld_flat >= plan->total_dim),
              "projection gradients need the forward's flat_embeddings, 16-byte aligned rows");
  DFM_REQUIRE(elems > 0 && elems % 16 == 0 && elems < (int64_t(1) << 31) &&
                  reinterpret_cast<uintptr_t>(base) % 64 == 0 && reinterpret_cast<uintptr_t>(ws) % 16 == 0,
              "the gradient range must be 64-byte aligned with a multiple of 16 elements");
  const int F = plan->num_fields, D = plan->fm_dim;
  const int parts = bwd_parts(batch);
  auto inside = [&](const float* p, int64_t n, int32_t* off) {
    if (!p || p < base || p + n > base + elems || (p - base) % 4) return false;
    *off = static_cast<int32_t>(p - base);
    return true;
  };
  memset(&g->jobs, 0, sizeof(g->jobs));
  memset(&g->go, 0, sizeof(g->go));
  int64_t blocks = 0, row_sum = 0;
  unsigned lds = 0;
  for (int f = 0; f < F; ++f) {
    const dfm_field& fd = plan->h_fields[f];
    const dfm_field_grad& gr = grads[f];
    const int d = fd.dim, pieces = d / 4 + 1;
    const int L = fd.kind == DFM_SEQUENCE ? fd.max_len : 1;
    bool ok;
    if (fd.kind == DFM_DENSE) {
      ok = inside(gr.w2, d, &g->go.w2[f]) && inside(gr.b2, d, &g->go.b2[f]) && inside(gr.w1, 1, &g->go.w1[f]) &&
           inside(gr.b1, 1, &g->go.b1[f]);
      DFM_REQUIRE(d + 1 <= kBwdThreads, "field %d: embedding_dim %d too wide", f, d);
      g->jobs.tiles[f] = 1;
    } else {
      if (fd.kind == DFM_SEQUENCE && fd.combiner == DFM_MAX)
        return fail(DFM_ERR_UNSUPPORTED, "record backward: field %d pools with max (the arg-max recompute is not built)", f);
      ok = inside(gr.w2, static_cast<int64_t>(fd.vocab) * d, &g->go.w2[f]) && inside(gr.w1, fd.vocab, &g->go.w1[f]);
      DFM_REQUIRE(pieces <= kBwdThreads, "field %d: embedding_dim %d too wide", f, d);
      const int rows = kBwdThreads / pieces * kBwdRows;
      g->jobs.tiles[f] = (fd.vocab + rows - 1) / rows;
      row_sum += fd.vocab;
    }
    if (fd.proj) ok = ok && inside(gr.proj, static_cast<int64_t>(D) * d, &g->go.proj[f]);
    DFM_REQUIRE(ok, "field %d: a gradient buffer is missing or lies outside [d_grad_base, d_grad_base + grad_elems)", f);
    g->jobs.first[f] = static_cast<int32_t>(blocks);
    blocks += static_cast<int64_t>(g->jobs.tiles[f]) * parts;
    const unsigned need = 16u * (kBwdStage * pieces + (kBwdStage * L + 3) / 4 + 1) + 4u * (fd.proj ? D * d : 0);
    lds = need > lds ? need : lds;
  }
  g->jobs.first[F] = static_cast<int32_t>(blocks);
  if (row_sum * batch > static_cast<int64_t>(DFM_BWD_RECORD_MAX_ROW_SAMPLES))
    return fail(DFM_ERR_UNSUPPORTED, "record backward: %lld table rows x %lld samples, over the row-owned scan's cap of %d",
                (long long)row_sum, (long long)batch, DFM_BWD_RECORD_MAX_ROW_SAMPLES);
  int64_t pblocks = 0;
  for (size_t i = 0; i < plan->h_proj.size(); ++i) {
    const dfm_field& fd = plan->h_fields[plan->h_proj[i]];
    g->jobs.chunks[i] = (D * fd.dim + kBwdThreads - 1) / kBwdThreads;
    g->jobs.pfirst[i] = static_cast<int32_t>(pblocks);
    pblocks += static_cast<int64_t>(g->jobs.chunks[i]) * parts;
    const unsigned need = 4u * kBwdStage * (D + fd.dim);
    lds = need > lds ? need : lds;
  }
  for (size_t i = plan->h_proj.size(); i <= static_cast<size_t>(DFM_MAX_FIELDS); ++i)
    g->jobs.pfirst[i] = static_cast<int32_t>(pblocks);
  blocks += pblocks;
  DFM_REQUIRE(blocks < (int64_t(1) << 24), "too many workgroups");
  if (lds > kBwdMaxLds)
    return fail(DFM_ERR_UNSUPPORTED, "record backward: a field needs %u bytes of LDS, over the cap of %u", lds, kBwdMaxLds);
  record_inputs(plan, d_record, batch, &g->in);
  g->fields = plan->d_fields; g->proj_list = plan->d_proj;
  g->B = batch; g->F = F; g->parts = parts; g->rows_per_part = (batch + parts - 1) / parts; g->elems = elems;
  g->g_first = g_first; g->g_field = g_field; g->g_flat = g_flat; g->ld_g = ld_g;
  g->flat_saved = flat_saved; g->ld_flat = ld_flat; g->partial = static_cast<float*>(ws);
  g->grid = dim3(static_cast<unsigned>(blocks)); g->block = dim3(kBwdThreads); g->lds = lds;
  g->g_fm = g_fm; g->fm_sum = fm_sum; g->field_emb = field_emb;
  switch (D) {
    case 4: g->func = fm ? reinterpret_cast<const void*>(&emb_bwd_record_fm<4>)
                         : reinterpret_cast<const void*>(&emb_bwd_record<4>); break;
    case 8: g->func = fm ? reinterpret_cast<const void*>(&emb_bwd_record_fm<8>)
                         : reinterpret_cast<const void*>(&emb_bwd_record<8>); break;
    case 16: g->func = fm ? reinterpret_cast<const void*>(&emb_bwd_record_fm<16>)
                         : reinterpret_cast<const void*>(&emb_bwd_record<16>); break;
    case 32: g->func = fm ? reinterpret_cast<const void*>(&emb_bwd_record_fm<32>)
                         : reinterpret_cast<const void*>(&emb_bwd_record<32>); break;
    default: g->func = fm ? reinterpret_cast<const void*>(&emb_bwd_record_fm<64>)
                         : reinterpret_cast<const void*>(&emb_bwd_record<64>); break;
  }
  g->bind();
  return DFM_OK;
}
}  // namespace

extern "C" int dfm_embedding_backward_record_parts(int64_t batch) { return batch > 0 ? bwd_parts(batch) : 0; }

extern "C" size_t dfm_embedding_backward_record_workspace_bytes(int64_t batch, int64_t grad_elems) {
  if (batch <= 0 || grad_elems <= 0) return 0;
  return sizeof(float) * static_cast<size_t>(bwd_parts(batch)) * static_cast<size_t>(grad_elems);
}

// fold_fm picks the instantiation: emb_bwd_record_fm<D> (d_g_field and the trio optional) or the plain emb_bwd_record<D>.
// With a NULL trio both have the same bits but not the same time: DESIGN.md has the measurement that kept the flag.
extern "C" int dfm_embedding_backward_record(const dfm_embedding_plan* plan, const void* d_record, int64_t batch,
                                             const float* d_g_first, const float* d_g_field, const float* d_g_flat,
                                             int64_t ld_g_flat, const float* d_flat_saved, int64_t ld_flat,
                                             const float* d_g_fm, const float* d_fm_sum, const float* d_field_emb,
                                             int fold_fm, const dfm_field_grad* grads, const float* d_grad_base,
                                             int64_t grad_elems, void* d_workspace, const dfm_launch* at) {
  DFM_CHECK_LAUNCH(at);
  BwdRecordLaunch g;
  if (int rc = describe_bwd_record(plan, d_record, batch, d_g_first, d_g_field, d_g_flat, ld_g_flat, d_flat_saved,
                                   ld_flat, d_g_fm, d_fm_sum, d_field_emb, fold_fm != 0, grads, d_grad_base, grad_elems,
                                   d_workspace, &g)) return rc;
  return launch_at(at, g.func, g.grid, g.block, g.lds, g.params, false);
}
