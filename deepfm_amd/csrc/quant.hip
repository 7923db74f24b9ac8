// Row-wise quantised embedding tables for serving (include/deepfm_hip.h: DFM_QUANT_INT8_ROWWISE and
// DFM_QUANT_UINT4_ROWWISE).  A record is [header | D codes of kBits bits each]; what depends on the
// format stands in one trait per format, Int8Rec<D> and Uint4Rec<D> (quant_records.h, which the record gather of
// embedding.hip reads quantised fields through as well).  Three kernels are written once over the trait:
//
//   quant_rows<Rec>           one streaming pass over a table: kRowLanes lanes per row, each with the 32 / kBits
//                             floats that fill one payload dword; min, max and the refusal by lane shuffles; one
//                             header store per row and one dword of payload per lane.
//   dequant_rows<Rec>         the inverse into contiguous fp32 (QuantizedTables.dequantized(), and the tests' second
//                             route), in the same lane split.
//   emb_fwd_quant<Rec,US,UD>  the uniform gather of embedding.hip (emb_fwd_uniform_body: a sample over D / kCols
//                             lanes, a workgroup of 8 waves owns 64 / (D / kCols) samples, a wave US SPARSE + UD DENSE
//                             fields of them per pass; ids and dense values first, then every record, then the
//                             arithmetic, then predicated stores) reading ONE aligned record per (sample, SPARSE
//                             field): scale, lo and the first-order weight from its header, the lane's kCols codes.
//
// Every step of the quantisers' arithmetic is one IEEE fp32 operation, so that a numpy float32 restatement gives the
// same bits: contraction is off for the whole file (x' = q * scale + lo must stay a multiply and an add), the DENSE
// fields and the accumulators say fmaf where embedding.hip's gather does.
#include "common.h"

#pragma STDC FP_CONTRACT OFF

#include "quant_records.h"     // the record formats: Int8Rec<D>, Uint4Rec<D>, mul_rn / add_rn / sub_rn, dequant4, quant4

using namespace dfm;
using namespace dfm::qrec;

namespace {

constexpr int kQuantThreads = 256;

bool quant_dim_ok(int dim) { return dim == 16 || dim == 32 || dim == 64; }
bool quant_format_ok(int format) { return format == DFM_QUANT_INT8_ROWWISE || format == DFM_QUANT_UINT4_ROWWISE; }

__device__ __forceinline__ bool finite4(const float4& x) {
  return isfinite(x.x) && isfinite(x.y) && isfinite(x.z) && isfinite(x.w);
}
__device__ __forceinline__ float min4(const float4& x) { return fminf(fminf(x.x, x.y), fminf(x.z, x.w)); }
__device__ __forceinline__ float max4(const float4& x) { return fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w)); }

// ---- the quantiser and its inverse --------------------------------------------------------------------------------
template <class Rec>
__global__ __launch_bounds__(kQuantThreads) void quant_rows(
    const float* __restrict__ w2, int64_t stride2, const float* __restrict__ w1, int64_t stride1, int64_t rows,
    uint8_t* __restrict__ out, int32_t* flag) {
  constexpr int LPR = Rec::kRowLanes;
  constexpr int NV = Rec::kDim / LPR / 4;      // float4 groups of a lane: its 32 / kBits columns
  static_assert(NV * 4 * Rec::kBits == 32, "a lane of a row has the columns of one payload dword");
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kQuantThreads + threadIdx.x;
  const int64_t r = t / LPR;
  const int q = static_cast<int>(t % LPR);
  const bool live = r < rows;
  const int64_t rc = live ? r : rows - 1;      // dead lanes repeat the last row: whole lane groups stay in the shuffles
  float4 x[NV];
#pragma unroll
  for (int h = 0; h < NV; ++h) x[h] = ld4(w2 + rc * stride2 + q * (4 * NV) + h * 4);
  const float w = w1[rc * stride1];            // same address on the row's lanes: one request
  float lo32 = min4(x[0]), hi32 = max4(x[0]);
#pragma unroll
  for (int h = 1; h < NV; ++h) {
    lo32 = fminf(lo32, min4(x[h]));
    hi32 = fmaxf(hi32, max4(x[h]));
  }
  bool fin = true;                             // fminf / fmaxf drop a NaN: look at the elements themselves
#pragma unroll
  for (int h = 0; h < NV; ++h) fin = fin && finite4(x[h]);
  int bad = fin ? 0 : 1;
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) {
    lo32 = fminf(lo32, __shfl_xor(lo32, m, kWave));
    hi32 = fmaxf(hi32, __shfl_xor(hi32, m, kWave));
    bad |= __shfl_xor(bad, m, kWave);
  }
  const typename Rec::Head hd = Rec::header(lo32, hi32, w, bad);
  const float scale = Rec::widen(hd).x, lo = Rec::widen(hd).y;
  const bool ok = !bad && scale != 0.f;
  uint32_t p = 0;
#pragma unroll
  for (int h = 0; h < NV; ++h) p |= quant4<Rec::kBits>(x[h], h, lo, scale, ok);
  if (!live) return;
  uint8_t* rec = out + r * Rec::kRowBytes;     // aligned as the header: kRowBytes is a multiple of kHeaderBytes
  if (q == 0) *reinterpret_cast<typename Rec::Head*>(rec) = hd;
  *reinterpret_cast<uint32_t*>(rec + Rec::kHeaderBytes + q * 4) = p;
  if (bad && q == 0) atomicOr(flag, 1);
}

template <class Rec>
__global__ __launch_bounds__(kQuantThreads) void dequant_rows(
    const uint8_t* __restrict__ recs, int64_t rows, float* __restrict__ w2, float* __restrict__ w1) {
  constexpr int LPR = Rec::kRowLanes, D = Rec::kDim;
  constexpr int NV = D / LPR / 4;
  static_assert(NV * 4 * Rec::kBits == 32, "a lane of a row has the columns of one payload dword");
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kQuantThreads + threadIdx.x;
  const int64_t r = t / LPR;
  const int q = static_cast<int>(t % LPR);
  if (r >= rows) return;
  const auto raw = load_lane<Rec>(recs + r * Rec::kRowBytes, q);
  const float4 v = Rec::widen(raw.head);        // scale, lo, w1, 0
  if (w2) {
#pragma unroll
    for (int h = 0; h < NV; ++h) st4(w2 + r * D + q * (4 * NV) + h * 4, dequant4<Rec::kBits>(raw.pay, h, v.x, v.y));
  }
  if (w1 && q == 0) w1[r] = v.z;
}

// ---- the gather ----------------------------------------------------------------------------------------------------
// Slot tables by value in the kernel arguments, as embedding.hip's UniformArgs: 48 * 24 + 32 * 48 bytes.
struct QSparseSlot {
  const int64_t* ids;
  const uint8_t* rows;
  int32_t vocab;
  int32_t field;
};
struct QDenseSlot {
  const float* x;
  const float* w2;
  const float* b2;
  const float* w1;
  const float* b1;
  int32_t field;
  int32_t pad;
};
constexpr int kMaxSparseSlots = 48, kMaxDenseSlots = 32;
struct QuantArgs {
  QSparseSlot sp[kMaxSparseSlots];
  QDenseSlot de[kMaxDenseSlots];
};

constexpr int kGatherWaves = 8;

// S += m e and SQ += m e^2 over 4 columns
__device__ __forceinline__ void fm_accumulate(float* S, float* SQ, float m, const float4& e) {
  S[0] = fmaf(m, e.x, S[0]); S[1] = fmaf(m, e.y, S[1]); S[2] = fmaf(m, e.z, S[2]); S[3] = fmaf(m, e.w, S[3]);
  SQ[0] = fmaf(m * e.x, e.x, SQ[0]); SQ[1] = fmaf(m * e.y, e.y, SQ[1]);
  SQ[2] = fmaf(m * e.z, e.z, SQ[2]); SQ[3] = fmaf(m * e.w, e.w, SQ[3]);
}
__device__ __forceinline__ float4 dense_row4(float x, const float4& w, const float4& b) {
  return make_float4(fmaf(x, w.x, b.x), fmaf(x, w.y, b.y), fmaf(x, w.z, b.z), fmaf(x, w.w, b.w));
}

// A kind with no fields is launched with US == 0 / UD == 0: a slot past the end is clamped to slot 0 (a duplicate,
// cache-hitting load, masked in the arithmetic), which must therefore be set.
template <class Rec, int US, int UD>
__global__ __launch_bounds__(kGatherWaves * 64) void emb_fwd_quant(
    QuantArgs args, int ns, int nd, int64_t B, int F, float* __restrict__ first_order, float* __restrict__ fe,
    float* __restrict__ fm_out, float* __restrict__ fm_sum, int32_t* error_flag, const float* __restrict__ extra_src,
    float* __restrict__ extra_dst) {
  constexpr int W = kGatherWaves, D = Rec::kDim;
  constexpr int CPL = Rec::kCols;   // columns of a lane
  constexpr int NV = CPL / 4;       // its float4 groups
  constexpr int LPR = D / CPL;      // lanes per row
  constexpr int SPW = kWave / LPR;  // samples per wave == samples per block
  constexpr int NC = 2 * CPL + 1;
  static_assert(NV * 4 == CPL && CPL * Rec::kBits <= 32, "a lane's codes come out of one payload dword");
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int s = lane / LPR, q = lane % LPR;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * SPW + s;
  const bool live = b < B;
  const int64_t bc = live ? b : B - 1;  // clamped: dead lanes load valid addresses

  float acc[NC] = {};               // of columns CPL * q ..: sum_f e (CPL), sum_f e^2 (CPL); the first-order sum
  float *const S = acc, *const SQ = acc + CPL, &fo = acc[2 * CPL];
  bool bad = false;

  const int sp_iters = US ? (ns + W * US - 1) / (W * US) : 0;
  const int de_iters = UD ? (nd + W * UD - 1) / (W * UD) : 0;
  const int iters = sp_iters > de_iters ? sp_iters : de_iters;
  for (int it = 0; it < iters; ++it) {
    bool oks[US + 1], okd[UD + 1];
    QSparseSlot sl[US + 1];
    QDenseSlot dl[UD + 1];
    const auto slot = [&](int u, int U, int n, bool& ok) {      // the wave's u-th of U slots of this pass, of n
      const int i = wave + (it * U + u) * W;
      ok = i < n;
      return ok ? i : 0;
    };
#pragma unroll
    for (int u = 0; u < US; ++u) sl[u] = args.sp[slot(u, US, ns, oks[u])];
#pragma unroll
    for (int u = 0; u < UD; ++u) dl[u] = args.de[slot(u, UD, nd, okd[u])];
    int64_t id[US + 1];
    float x[UD + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) id[u] = sl[u].ids[bc];
#pragma unroll
    for (int u = 0; u < UD; ++u) x[u] = dl[u].x[bc];
    RawRec<typename Rec::Head> raw[US + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) {
      const bool oob = static_cast<uint64_t>(id[u]) >= static_cast<uint64_t>(sl[u].vocab);
      bad |= oob && oks[u];
      id[u] = oob ? 0 : id[u];
      raw[u] = Rec::load(sl[u].rows + id[u] * Rec::kRowBytes, q);
    }
    float4 dw[UD + 1][NV], db[UD + 1][NV];
    float dw1[UD + 1], db1[UD + 1];
#pragma unroll
    for (int u = 0; u < UD; ++u) {
#pragma unroll
      for (int h = 0; h < NV; ++h) {
        dw[u][h] = ld4(dl[u].w2 + q * CPL + h * 4);
        db[u][h] = ld4(dl[u].b2 + q * CPL + h * 4);
      }
      dw1[u] = dl[u].w1[0];
      db1[u] = dl[u].b1[0];
    }
    float* out = fe + b * F * D + q * CPL;
#pragma unroll
    for (int u = 0; u < US; ++u) {
      const float m = oks[u] ? 1.f : 0.f;
      const float4 v = Rec::widen(raw[u].head);  // scale, lo, w1, 0
#pragma unroll
      for (int h = 0; h < NV; ++h) {
        const float4 e = dequant4<Rec::kBits>(raw[u].pay, h, v.x, v.y);
        fm_accumulate(S + 4 * h, SQ + 4 * h, m, e);
        if (live && oks[u]) st4(out + sl[u].field * D + h * 4, e);
      }
      fo = fmaf(m, v.z, fo);
    }
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      const float m = okd[u] ? 1.f : 0.f;
#pragma unroll
      for (int h = 0; h < NV; ++h) {
        const float4 e = dense_row4(x[u], dw[u][h], db[u][h]);
        fm_accumulate(S + 4 * h, SQ + 4 * h, m, e);
        if (live && okd[u]) st4(out + dl[u].field * D + h * 4, e);
      }
      fo = fmaf(m, fmaf(x[u], dw1[u], db1[u]), fo);
    }
  }
  if (bad && error_flag) atomicOr(error_flag, 1);
  if (q != 0) fo = 0.f;  // every lane of a row read the same first-order value: count it once
  // ---- fixed-order reduction over the block's waves ------------------------------------
  __shared__ float red[W][NC][kWave];
#pragma unroll
  for (int c = 0; c < NC; ++c) red[wave][c][lane] = acc[c];
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = red[0][c][lane];
  for (int w = 1; w < W; ++w) {
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] += red[w][c][lane];
  }
  // 0.5 * sum_d (S_d^2 - SQ_d), the lane's columns in order
  float t = S[0] * S[0] - SQ[0];
#pragma unroll
  for (int c = 1; c < CPL; ++c) t += S[c] * S[c] - SQ[c];
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) t += __shfl_xor(t, m, kWave);
  if (live && q == 0) {
    first_order[b] = fo;
    if (fm_out) fm_out[b] = 0.5f * t;
    if (extra_dst) extra_dst[b] = extra_src[b];      // per-sample payload (labels)
  }
  if (live && fm_sum) {
#pragma unroll
    for (int h = 0; h < NV; ++h)
      st4(fm_sum + b * D + q * CPL + h * 4, make_float4(S[4 * h], S[4 * h + 1], S[4 * h + 2], S[4 * h + 3]));
  }
}

// fn(Rec{}) with the trait of a width and a format that quant_dim_ok and quant_format_ok let through
template <class Fn>
auto with_record(int dim, int format, Fn&& fn) {
  const bool u4 = format == DFM_QUANT_UINT4_ROWWISE;
  switch (dim) {
    case 16: return u4 ? fn(Uint4Rec<16>{}) : fn(Int8Rec<16>{});
    case 32: return u4 ? fn(Uint4Rec<32>{}) : fn(Int8Rec<32>{});
    default: return u4 ? fn(Uint4Rec<64>{}) : fn(Int8Rec<64>{});
  }
}

unsigned quant_grid(int64_t rows, int lanes_per_row) {
  return static_cast<unsigned>((rows * lanes_per_row + kQuantThreads - 1) / kQuantThreads);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_shape(int dim, int format) {
  if (!quant_format_ok(format))
    return fail(DFM_ERR_UNSUPPORTED, "quantised format %d: DFM_QUANT_INT8_ROWWISE and DFM_QUANT_UINT4_ROWWISE only", format);
  if (!quant_dim_ok(dim)) return fail(DFM_ERR_UNSUPPORTED, "quantised tables of width %d: widths 16, 32 and 64 only", dim);
  return DFM_OK;
}

}  // namespace

extern "C" int dfm_quant_row_bytes(int dim, int format) {
  if (!quant_dim_ok(dim) || !quant_format_ok(format)) return 0;
  return with_record(dim, format, [](auto rec) { return decltype(rec)::kRowBytes; });
}

extern "C" int dfm_quantize_rows(const float* d_w2, int64_t stride2, const float* d_w1, int64_t stride1, int64_t rows,
                                 int dim, int format, void* d_out, int32_t* d_flag, dfm_stream_t stream) {
  if (const int rc = check_shape(dim, format)) return rc;
  DFM_REQUIRE(d_w2 && d_w1 && d_out && d_flag, "null argument");
  DFM_REQUIRE(rows >= 0 && rows < (int64_t(1) << 31), "rows %lld out of range", (long long)rows);
  DFM_REQUIRE(aligned16(d_w2) && stride2 % 4 == 0 && stride2 >= dim, "table rows must be 16-byte aligned, stride >= dim");
  DFM_REQUIRE(stride1 >= 1, "first-order stride must be positive");
  DFM_REQUIRE(aligned16(d_out), "records must be 16-byte aligned");
  if (rows == 0) return DFM_OK;
  with_record(dim, format, [&](auto rec) {
    using Rec = decltype(rec);
    hipLaunchKernelGGL(quant_rows<Rec>, dim3(quant_grid(rows, Rec::kRowLanes)), dim3(kQuantThreads), 0,
                       as_stream(stream), d_w2, stride2, d_w1, stride1, rows, static_cast<uint8_t*>(d_out), d_flag);
  });
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_dequantize_rows(const void* d_records, int64_t rows, int dim, int format, float* d_w2, float* d_w1,
                                   dfm_stream_t stream) {
  if (const int rc = check_shape(dim, format)) return rc;
  DFM_REQUIRE(d_records, "null argument");
  DFM_REQUIRE(rows >= 0 && rows < (int64_t(1) << 31), "rows %lld out of range", (long long)rows);
  DFM_REQUIRE(aligned16(d_records) && aligned16(d_w2), "records and d_w2 must be 16-byte aligned");
  if (rows == 0 || (!d_w2 && !d_w1)) return DFM_OK;
  with_record(dim, format, [&](auto rec) {
    using Rec = decltype(rec);
    hipLaunchKernelGGL(dequant_rows<Rec>, dim3(quant_grid(rows, Rec::kRowLanes)), dim3(kQuantThreads), 0,
                       as_stream(stream), static_cast<const uint8_t*>(d_records), rows, d_w2, d_w1);
  });
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_embedding_forward_quant(const dfm_quant_field* fields, int num_fields, int dim, int format,
                                           const void* const* inputs, const float* d_extra_src, float* d_extra_dst,
                                           int64_t batch, float* d_first_order, float* d_field_emb, float* d_fm_out,
                                           float* d_fm_sum, int32_t* d_error_flag, const dfm_launch* at) {
  DFM_CHECK_LAUNCH(at);
  if (const int rc = check_shape(dim, format)) return rc;
  DFM_REQUIRE(fields && inputs && d_first_order && d_field_emb, "null argument");
  DFM_REQUIRE(num_fields >= 1 && num_fields <= DFM_MAX_FIELDS, "num_fields %d outside [1, %d]", num_fields, DFM_MAX_FIELDS);
  DFM_REQUIRE((d_extra_src == nullptr) == (d_extra_dst == nullptr), "extra source and destination go together");
  DFM_REQUIRE(batch >= (repoints(at) ? 1 : 0) && batch < (int64_t(1) << 31), "batch %lld out of range", (long long)batch);
  DFM_REQUIRE(aligned16(d_field_emb) && aligned16(d_fm_sum), "field_embeddings and fm_sum must be 16-byte aligned");
  int ns = 0, nd = 0;
  for (int f = 0; f < num_fields; ++f) {
    DFM_REQUIRE(fields[f].kind == DFM_SPARSE || fields[f].kind == DFM_DENSE,
                "field %d: the quantised gather takes SPARSE and DENSE fields", f);
    (fields[f].kind == DFM_SPARSE ? ns : nd) += 1;
  }
  if (ns > kMaxSparseSlots || nd > kMaxDenseSlots)
    return fail(DFM_ERR_UNSUPPORTED, "%d SPARSE + %d DENSE fields: the quantised gather takes at most %d SPARSE and "
                "%d DENSE fields", ns, nd, kMaxSparseSlots, kMaxDenseSlots);
  if (batch == 0) return DFM_OK;
  QuantArgs args;
  memset(&args, 0, sizeof(args));
  ns = nd = 0;
  for (int f = 0; f < num_fields; ++f) {
    const dfm_quant_field& fd = fields[f];
    DFM_REQUIRE(inputs[f] != nullptr, "inputs[%d] is null", f);
    if (fd.kind == DFM_SPARSE) {
      DFM_REQUIRE(fd.rows && aligned16(fd.rows) && fd.vocab >= 1, "field %d: records must be 16-byte aligned, vocab >= 1", f);
      DFM_REQUIRE((reinterpret_cast<uintptr_t>(inputs[f]) & 7) == 0, "inputs[%d]: ids must be 8-byte aligned", f);
      args.sp[ns++] = QSparseSlot{static_cast<const int64_t*>(inputs[f]), static_cast<const uint8_t*>(fd.rows), fd.vocab, f};
    } else {
      DFM_REQUIRE(fd.w2 && fd.b2 && fd.w1 && fd.b1, "field %d: missing DENSE parameter", f);
      args.de[nd++] = QDenseSlot{static_cast<const float*>(inputs[f]), fd.w2, fd.b2, fd.w1, fd.b1, f, 0};
    }
  }
  int F = num_fields;
  void* params[] = {&args, &ns, &nd, &batch, &F, &d_first_order, &d_field_emb, &d_fm_out, &d_fm_sum, &d_error_flag,
                    &d_extra_src, &d_extra_dst};
  return with_record(dim, format, [&](auto rec) {
    using Rec = decltype(rec);
    const void* func = ns == 0   ? reinterpret_cast<const void*>(&emb_fwd_quant<Rec, 0, 2>)
                       : nd == 0 ? reinterpret_cast<const void*>(&emb_fwd_quant<Rec, 4, 0>)
                                 : reinterpret_cast<const void*>(&emb_fwd_quant<Rec, 4, 2>);
    constexpr int spw = kWave / (Rec::kDim / Rec::kCols);        // samples per workgroup
    return launch_at(at, func, dim3(static_cast<unsigned>((batch + spw - 1) / spw)), dim3(kGatherWaves * 64), 0, params,
                     false);
  });
}
