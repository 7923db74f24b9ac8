// Row-wise int8 and 4-bit embedding tables for serving (include/deepfm_hip.h: DFM_QUANT_INT8_ROWWISE and
// DFM_QUANT_UINT4_ROWWISE).  The int8 kernels first; the 4-bit ones (quant_rows_uint4, dequant_rows_uint4,
// emb_fwd_quant4) keep their shapes and are described where they stand.
//
//   quant_rows_int8<D>    one streaming pass over a table: D/4 lanes per row, each with 16 bytes of it; min and max
//                         by lane shuffles; one 16-byte header store per row and one dword of payload per lane.
//   dequant_rows_int8<D>  the inverse into contiguous fp32 (QuantizedTables.dequantized(), and the tests' second route).
//   emb_fwd_quant<D,...>  the uniform gather of embedding.hip (emb_fwd_uniform_body: samples over D/4 lanes, a
//                         workgroup of 8 waves owns 64/(D/4) samples, a wave US SPARSE + UD DENSE fields of them per
//                         pass; ids and dense values first, then every record, then the arithmetic, then predicated
//                         stores) reading ONE 16-byte-aligned record per (sample, SPARSE field): the header (same
//                         address on the row's lanes: one request) carries scale, lo and the first-order weight, and
//                         lane q converts dword q of the payload into its float4 of field_embeddings.
//
// Every step of the quantiser's arithmetic is one IEEE fp32 operation, so that a numpy float32 restatement gives the
// same bits: contraction is off for the whole file (x' = q * scale + lo must stay a multiply and an add), the DENSE
// fields and the accumulators say fmaf where embedding.hip's gather does.
#include "common.h"

#pragma STDC FP_CONTRACT OFF

using namespace dfm;

namespace {

constexpr int kHeaderBytes = 16;
constexpr int kQuantThreads = 256;

bool quant_dim_ok(int dim) { return dim == 16 || dim == 32 || dim == 64; }

__device__ __forceinline__ bool finite4(const float4& x) {
  return isfinite(x.x) && isfinite(x.y) && isfinite(x.z) && isfinite(x.w);
}

// One rounding each.  The header's __fmul_rn / __fadd_rn are plain operators compiled where contraction is allowed,
// so a product and a sum of theirs still fuse into an fma after inlining; these, compiled under the pragma above
// (and the one inside), do not.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// x' of the four bytes of one payload dword (q[4k] is the low byte)
__device__ __forceinline__ float4 dequant4(uint32_t p, float scale, float lo) {
  float4 e;
  e.x = add_rn(mul_rn(static_cast<float>(p & 0xffu), scale), lo);
  e.y = add_rn(mul_rn(static_cast<float>((p >> 8) & 0xffu), scale), lo);
  e.z = add_rn(mul_rn(static_cast<float>((p >> 16) & 0xffu), scale), lo);
  e.w = add_rn(mul_rn(static_cast<float>(p >> 24), scale), lo);
  return e;
}

__device__ __forceinline__ uint32_t quant1(float x, float lo, float scale, bool ok) {
  const float v = fminf(rintf(sub_rn(x, lo) / scale), 255.f);
  return static_cast<uint32_t>(ok ? v : 0.f);
}

template <int D>
__global__ __launch_bounds__(kQuantThreads) void quant_rows_int8(
    const float* __restrict__ w2, int64_t stride2, const float* __restrict__ w1, int64_t stride1, int64_t rows,
    uint8_t* __restrict__ out, int32_t* flag) {
  constexpr int LPR = D / 4;
  constexpr int RB = kHeaderBytes + D;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kQuantThreads + threadIdx.x;
  const int64_t r = t / LPR;
  const int q = static_cast<int>(t % LPR);
  const bool live = r < rows;
  const int64_t rc = live ? r : rows - 1;      // dead lanes repeat the last row: whole lane groups stay in the shuffles
  const float4 x = ld4(w2 + rc * stride2 + q * 4);
  const float w = w1[rc * stride1];            // same address on the row's lanes: one request
  float lo = fminf(fminf(x.x, x.y), fminf(x.z, x.w));
  float hi = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
  int bad = finite4(x) ? 0 : 1;                // fminf / fmaxf drop a NaN: look at the elements themselves
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) {
    lo = fminf(lo, __shfl_xor(lo, m, kWave));
    hi = fmaxf(hi, __shfl_xor(hi, m, kWave));
    bad |= __shfl_xor(bad, m, kWave);
  }
  const float range = sub_rn(hi, lo);
  if (!isfinite(range)) bad = 1;               // hi - lo overflows
  const float scale = range / 255.0f;
  const bool ok = !bad && scale != 0.f;
  const uint32_t p = quant1(x.x, lo, scale, ok) | (quant1(x.y, lo, scale, ok) << 8) |
                     (quant1(x.z, lo, scale, ok) << 16) | (quant1(x.w, lo, scale, ok) << 24);
  if (!live) return;
  uint8_t* rec = out + r * RB;
  if (q == 0) st4(reinterpret_cast<float*>(rec), make_float4(scale, lo, w, 0.f));
  *reinterpret_cast<uint32_t*>(rec + kHeaderBytes + q * 4) = p;
  if (bad && q == 0) atomicOr(flag, 1);
}

template <int D>
__global__ __launch_bounds__(kQuantThreads) void dequant_rows_int8(
    const uint8_t* __restrict__ recs, int64_t rows, float* __restrict__ w2, float* __restrict__ w1) {
  constexpr int LPR = D / 4;
  constexpr int RB = kHeaderBytes + D;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kQuantThreads + threadIdx.x;
  const int64_t r = t / LPR;
  const int q = static_cast<int>(t % LPR);
  if (r >= rows) return;
  const uint8_t* rec = recs + r * RB;
  const float4 h = ld4(reinterpret_cast<const float*>(rec));
  const uint32_t p = *reinterpret_cast<const uint32_t*>(rec + kHeaderBytes + q * 4);
  if (w2) st4(w2 + r * D + q * 4, dequant4(p, h.x, h.y));
  if (w1 && q == 0) w1[r] = h.z;
}

// ---- DFM_QUANT_UINT4_ROWWISE ---------------------------------------------------------------------------------------
// Records of 8 + D / 2 bytes: [scale binary16 | lo binary16 | w1 fp32 | q, 4 bits each].  D / 8 lanes per row: a lane
// has 8 floats of it (two 16-byte loads or stores) and one payload dword, element 8 * lane + k in bits 4k .. 4k + 3.
constexpr int kHeaderBytes4 = 8;

__device__ __forceinline__ uint32_t half_bits(_Float16 h) { return __builtin_bit_cast(unsigned short, h); }
__device__ __forceinline__ float half_value(uint32_t bits) {
  return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<unsigned short>(bits)));
}
__device__ __forceinline__ bool half_is_inf(uint32_t bits) { return (bits & 0x7fffu) == 0x7c00u; }

// The largest binary16 <= v: round to nearest even, then one step towards -inf where that went above v (for a
// negative value, -0 included, the next bit pattern; for a positive one the previous).
__device__ __forceinline__ uint32_t half_floor(float v) {
  const uint32_t b = half_bits(static_cast<_Float16>(v));
  if (!(half_value(b) > v)) return b;
  return (b & 0x8000u) ? b + 1 : b - 1;
}
// The smallest binary16 >= v, for v >= 0: the next bit pattern where round to nearest even went below v.
__device__ __forceinline__ uint32_t half_ceil(float v) {
  const uint32_t b = half_bits(static_cast<_Float16>(v));
  return half_value(b) < v ? b + 1 : b;
}

__device__ __forceinline__ uint32_t quant1_u4(float x, float lo, float scale, bool ok) {
  const float v = fminf(rintf(sub_rn(x, lo) / scale), 15.f);
  return static_cast<uint32_t>(ok ? v : 0.f);
}

// x' of nibbles 4h .. 4h + 3 of one payload dword
__device__ __forceinline__ float4 dequant4_u4(uint32_t p, int h, float scale, float lo) {
  p >>= 16 * h;
  float4 e;
  e.x = add_rn(mul_rn(static_cast<float>(p & 15u), scale), lo);
  e.y = add_rn(mul_rn(static_cast<float>((p >> 4) & 15u), scale), lo);
  e.z = add_rn(mul_rn(static_cast<float>((p >> 8) & 15u), scale), lo);
  e.w = add_rn(mul_rn(static_cast<float>((p >> 12) & 15u), scale), lo);
  return e;
}

template <int D>
__global__ __launch_bounds__(kQuantThreads) void quant_rows_uint4(
    const float* __restrict__ w2, int64_t stride2, const float* __restrict__ w1, int64_t stride1, int64_t rows,
    uint8_t* __restrict__ out, int32_t* flag) {
  constexpr int LPR = D / 8;
  constexpr int RB = kHeaderBytes4 + D / 2;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kQuantThreads + threadIdx.x;
  const int64_t r = t / LPR;
  const int q = static_cast<int>(t % LPR);
  const bool live = r < rows;
  const int64_t rc = live ? r : rows - 1;      // dead lanes repeat the last row: whole lane groups stay in the shuffles
  const float4 x0 = ld4(w2 + rc * stride2 + q * 8);
  const float4 x1 = ld4(w2 + rc * stride2 + q * 8 + 4);
  const float w = w1[rc * stride1];            // same address on the row's lanes: one request
  float lo32 = fminf(fminf(fminf(x0.x, x0.y), fminf(x0.z, x0.w)), fminf(fminf(x1.x, x1.y), fminf(x1.z, x1.w)));
  float hi32 = fmaxf(fmaxf(fmaxf(x0.x, x0.y), fmaxf(x0.z, x0.w)), fmaxf(fmaxf(x1.x, x1.y), fmaxf(x1.z, x1.w)));
  int bad = finite4(x0) && finite4(x1) ? 0 : 1;
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) {
    lo32 = fminf(lo32, __shfl_xor(lo32, m, kWave));
    hi32 = fmaxf(hi32, __shfl_xor(hi32, m, kWave));
    bad |= __shfl_xor(bad, m, kWave);
  }
  const uint32_t lo_h = half_floor(lo32);
  const float lo = half_value(lo_h);
  uint32_t scale_h = half_ceil(sub_rn(hi32, lo) / 15.0f);
  // The subtract and the divide can both round down, onto a binary16 value that the ceiling then keeps: where
  // lo + 15 scale is still below hi (exact in fp64: the terms span under 53 bits), one more binary16 value up.
  if (static_cast<double>(lo) + 15.0 * static_cast<double>(half_value(scale_h)) < static_cast<double>(hi32)) scale_h += 1;
  const float scale = half_value(scale_h);
  if (half_is_inf(lo_h) || half_is_inf(scale_h)) bad = 1;    // lo below -65504, or a range past 15 * 65504
  const bool ok = !bad && scale != 0.f;
  const uint32_t p = quant1_u4(x0.x, lo, scale, ok) | (quant1_u4(x0.y, lo, scale, ok) << 4) |
                     (quant1_u4(x0.z, lo, scale, ok) << 8) | (quant1_u4(x0.w, lo, scale, ok) << 12) |
                     (quant1_u4(x1.x, lo, scale, ok) << 16) | (quant1_u4(x1.y, lo, scale, ok) << 20) |
                     (quant1_u4(x1.z, lo, scale, ok) << 24) | (quant1_u4(x1.w, lo, scale, ok) << 28);
  if (!live) return;
  uint8_t* rec = out + r * RB;                 // 8-byte aligned: RB % 8 == 0
  if (q == 0) *reinterpret_cast<uint2*>(rec) = make_uint2(scale_h | (lo_h << 16), __float_as_uint(w));
  *reinterpret_cast<uint32_t*>(rec + kHeaderBytes4 + q * 4) = p;
  if (bad && q == 0) atomicOr(flag, 1);
}

template <int D>
__global__ __launch_bounds__(kQuantThreads) void dequant_rows_uint4(
    const uint8_t* __restrict__ recs, int64_t rows, float* __restrict__ w2, float* __restrict__ w1) {
  constexpr int LPR = D / 8;
  constexpr int RB = kHeaderBytes4 + D / 2;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kQuantThreads + threadIdx.x;
  const int64_t r = t / LPR;
  const int q = static_cast<int>(t % LPR);
  if (r >= rows) return;
  const uint8_t* rec = recs + r * RB;
  const uint2 h = *reinterpret_cast<const uint2*>(rec);
  const uint32_t p = *reinterpret_cast<const uint32_t*>(rec + kHeaderBytes4 + q * 4);
  const float scale = half_value(h.x & 0xffffu), lo = half_value(h.x >> 16);
  if (w2) {
    st4(w2 + r * D + q * 8, dequant4_u4(p, 0, scale, lo));
    st4(w2 + r * D + q * 8 + 4, dequant4_u4(p, 1, scale, lo));
  }
  if (w1 && q == 0) w1[r] = __uint_as_float(h.y);
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

// A kind with no fields is launched with US == 0 / UD == 0: a slot past the end is clamped to slot 0 (a duplicate,
// cache-hitting load, masked in the arithmetic), which must therefore be set.
template <int D, int US, int UD>
__global__ __launch_bounds__(kGatherWaves * 64) void emb_fwd_quant(
    QuantArgs args, int ns, int nd, int64_t B, int F, float* __restrict__ first_order, float* __restrict__ fe,
    float* __restrict__ fm_out, float* __restrict__ fm_sum, int32_t* error_flag, const float* __restrict__ extra_src,
    float* __restrict__ extra_dst) {
  constexpr int W = kGatherWaves;
  constexpr int LPR = D / 4;        // lanes per row: 16 bytes of fp32 output, one payload dword each
  constexpr int SPW = kWave / LPR;  // samples per wave == samples per block
  constexpr int RB = kHeaderBytes + D;
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int s = lane / LPR, q = lane % LPR;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * SPW + s;
  const bool live = b < B;
  const int64_t bc = live ? b : B - 1;  // clamped: dead lanes load valid addresses

  float4 S = make_float4(0.f, 0.f, 0.f, 0.f);   // sum_f e
  float4 SQ = make_float4(0.f, 0.f, 0.f, 0.f);  // sum_f e^2
  float fo = 0.f;
  bool bad = false;

  const int sp_iters = US ? (ns + W * US - 1) / (W * US) : 0;
  const int de_iters = UD ? (nd + W * UD - 1) / (W * UD) : 0;
  const int iters = sp_iters > de_iters ? sp_iters : de_iters;
  for (int it = 0; it < iters; ++it) {
    bool oks[US + 1], okd[UD + 1];
    QSparseSlot sl[US + 1];
    QDenseSlot dl[UD + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) {
      const int i = wave + (it * US + u) * W;
      oks[u] = i < ns;
      sl[u] = args.sp[oks[u] ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      const int i = wave + (it * UD + u) * W;
      okd[u] = i < nd;
      dl[u] = args.de[okd[u] ? i : 0];
    }
    int64_t id[US + 1];
    float x[UD + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) id[u] = sl[u].ids[bc];
#pragma unroll
    for (int u = 0; u < UD; ++u) x[u] = dl[u].x[bc];
    float4 head[US + 1];      // scale, lo, w1, 0
    uint32_t pay[US + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) {
      const bool oob = static_cast<uint64_t>(id[u]) >= static_cast<uint64_t>(sl[u].vocab);
      bad |= oob && oks[u];
      id[u] = oob ? 0 : id[u];
      const uint8_t* rec = sl[u].rows + id[u] * RB;
      head[u] = ld4(reinterpret_cast<const float*>(rec));      // same address on the row's lanes: one request
      pay[u] = *reinterpret_cast<const uint32_t*>(rec + kHeaderBytes + q * 4);
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
      const float4 e = dequant4(pay[u], head[u].x, head[u].y);
      S.x = fmaf(m, e.x, S.x); S.y = fmaf(m, e.y, S.y); S.z = fmaf(m, e.z, S.z); S.w = fmaf(m, e.w, S.w);
      SQ.x = fmaf(m * e.x, e.x, SQ.x); SQ.y = fmaf(m * e.y, e.y, SQ.y);
      SQ.z = fmaf(m * e.z, e.z, SQ.z); SQ.w = fmaf(m * e.w, e.w, SQ.w);
      fo = fmaf(m, head[u].z, fo);
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
  if (q != 0) fo = 0.f;  // every lane of a row read the same first-order value: count it once
  float acc[9] = {S.x, S.y, S.z, S.w, SQ.x, SQ.y, SQ.z, SQ.w, fo};
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
  // 0.5 * sum_d (S_d^2 - SQ_d)
  float t = (acc[0] * acc[0] - acc[4]) + (acc[1] * acc[1] - acc[5]) +
            (acc[2] * acc[2] - acc[6]) + (acc[3] * acc[3] - acc[7]);
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) t += __shfl_xor(t, m, kWave);
  if (live && q == 0) {
    first_order[b] = acc[8];
    if (fm_out) fm_out[b] = 0.5f * t;
    if (extra_dst) extra_dst[b] = extra_src[b];      // per-sample payload (labels)
  }
  if (live && fm_sum) st4(fm_sum + b * D + q * 4, make_float4(acc[0], acc[1], acc[2], acc[3]));
}

__device__ __forceinline__ void fm_accumulate(float4& S, float4& SQ, float m, const float4& e) {
  S.x = fmaf(m, e.x, S.x); S.y = fmaf(m, e.y, S.y); S.z = fmaf(m, e.z, S.z); S.w = fmaf(m, e.w, S.w);
  SQ.x = fmaf(m * e.x, e.x, SQ.x); SQ.y = fmaf(m * e.y, e.y, SQ.y);
  SQ.z = fmaf(m * e.z, e.z, SQ.z); SQ.w = fmaf(m * e.w, e.w, SQ.w);
}
__device__ __forceinline__ float4 dense_row4(float x, const float4& w, const float4& b) {
  return make_float4(fmaf(x, w.x, b.x), fmaf(x, w.y, b.y), fmaf(x, w.z, b.z), fmaf(x, w.w, b.w));
}

// The same skeleton over DFM_QUANT_UINT4_ROWWISE records.  At D = 32 and 64 a lane has 8 columns (D / 8 lanes per row,
// 16 / 8 samples per workgroup): its payload dword, two 16-byte stores per field, and 17 partial sums (8 of S, 8 of
// SQ, the first-order sum) in the reduction, 8 * 17 * 64 floats of LDS.  At D = 16 that would leave 128 workgroups for
// a batch of 4096, half as many as there are CUs, so a lane has 4 columns there as in the int8 gather (4 lanes per row,
// 16 samples per workgroup); the record is 16 bytes and 16-byte aligned: one load, the same address on the row's
// lanes, of which lane q keeps 16 bits.
constexpr int quant4_cols_per_lane(int D) { return D == 16 ? 4 : 8; }

template <int D, int US, int UD>
__global__ __launch_bounds__(kGatherWaves * 64) void emb_fwd_quant4(
    QuantArgs args, int ns, int nd, int64_t B, int F, float* __restrict__ first_order, float* __restrict__ fe,
    float* __restrict__ fm_out, float* __restrict__ fm_sum, int32_t* error_flag, const float* __restrict__ extra_src,
    float* __restrict__ extra_dst) {
  constexpr int W = kGatherWaves;
  constexpr int CPL = quant4_cols_per_lane(D);
  constexpr int NV = CPL / 4;       // float4 groups of a lane
  constexpr int LPR = D / CPL;      // lanes per row
  constexpr int SPW = kWave / LPR;  // samples per wave == samples per block
  constexpr int RB = kHeaderBytes4 + D / 2;
  constexpr int NC = 2 * CPL + 1;
  const int lane = lane_id();
  const int wave = wave_id_uniform();
  const int s = lane / LPR, q = lane % LPR;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * SPW + s;
  const bool live = b < B;
  const int64_t bc = live ? b : B - 1;  // clamped: dead lanes load valid addresses

  float4 S[NV], SQ[NV];             // sum_f e and sum_f e^2 of columns CPL * q + 4h .. + 3
#pragma unroll
  for (int h = 0; h < NV; ++h) S[h] = SQ[h] = make_float4(0.f, 0.f, 0.f, 0.f);
  float fo = 0.f;
  bool bad = false;

  const int sp_iters = US ? (ns + W * US - 1) / (W * US) : 0;
  const int de_iters = UD ? (nd + W * UD - 1) / (W * UD) : 0;
  const int iters = sp_iters > de_iters ? sp_iters : de_iters;
  for (int it = 0; it < iters; ++it) {
    bool oks[US + 1], okd[UD + 1];
    QSparseSlot sl[US + 1];
    QDenseSlot dl[UD + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) {
      const int i = wave + (it * US + u) * W;
      oks[u] = i < ns;
      sl[u] = args.sp[oks[u] ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      const int i = wave + (it * UD + u) * W;
      okd[u] = i < nd;
      dl[u] = args.de[okd[u] ? i : 0];
    }
    int64_t id[US + 1];
    float x[UD + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) id[u] = sl[u].ids[bc];
#pragma unroll
    for (int u = 0; u < UD; ++u) x[u] = dl[u].x[bc];
    uint2 head[US + 1];       // scale | lo << 16, w1
    uint32_t pay[US + 1];
#pragma unroll
    for (int u = 0; u < US; ++u) {
      const bool oob = static_cast<uint64_t>(id[u]) >= static_cast<uint64_t>(sl[u].vocab);
      bad |= oob && oks[u];
      id[u] = oob ? 0 : id[u];
      const uint8_t* rec = sl[u].rows + id[u] * RB;
      if constexpr (D == 16) {
        const uint4 r = *reinterpret_cast<const uint4*>(rec);
        head[u] = make_uint2(r.x, r.y);
        pay[u] = ((q & 2) ? r.w : r.z) >> (16 * (q & 1));        // dequant4_u4 looks at the low 16 bits only
      } else {
        head[u] = *reinterpret_cast<const uint2*>(rec);          // same address on the row's lanes: one request
        pay[u] = *reinterpret_cast<const uint32_t*>(rec + kHeaderBytes4 + q * 4);
      }
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
      const float scale = half_value(head[u].x & 0xffffu), lo = half_value(head[u].x >> 16);
#pragma unroll
      for (int h = 0; h < NV; ++h) {
        const float4 e = dequant4_u4(pay[u], h, scale, lo);
        fm_accumulate(S[h], SQ[h], m, e);
        if (live && oks[u]) st4(out + sl[u].field * D + h * 4, e);
      }
      fo = fmaf(m, __uint_as_float(head[u].y), fo);
    }
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      const float m = okd[u] ? 1.f : 0.f;
#pragma unroll
      for (int h = 0; h < NV; ++h) {
        const float4 e = dense_row4(x[u], dw[u][h], db[u][h]);
        fm_accumulate(S[h], SQ[h], m, e);
        if (live && okd[u]) st4(out + dl[u].field * D + h * 4, e);
      }
      fo = fmaf(m, fmaf(x[u], dw1[u], db1[u]), fo);
    }
  }
  if (bad && error_flag) atomicOr(error_flag, 1);
  if (q != 0) fo = 0.f;  // every lane of a row read the same first-order value: count it once
  float acc[NC];                    // S (CPL), SQ (CPL), fo
#pragma unroll
  for (int h = 0; h < NV; ++h) {
    acc[4 * h] = S[h].x; acc[4 * h + 1] = S[h].y; acc[4 * h + 2] = S[h].z; acc[4 * h + 3] = S[h].w;
    acc[CPL + 4 * h] = SQ[h].x; acc[CPL + 4 * h + 1] = SQ[h].y;
    acc[CPL + 4 * h + 2] = SQ[h].z; acc[CPL + 4 * h + 3] = SQ[h].w;
  }
  acc[2 * CPL] = fo;
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
  // 0.5 * sum_d (S_d^2 - SQ_d)
  float t = 0.f;
#pragma unroll
  for (int c = 0; c < CPL; ++c) t += acc[c] * acc[c] - acc[CPL + c];
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) t += __shfl_xor(t, m, kWave);
  if (live && q == 0) {
    first_order[b] = acc[2 * CPL];
    if (fm_out) fm_out[b] = 0.5f * t;
    if (extra_dst) extra_dst[b] = extra_src[b];      // per-sample payload (labels)
  }
  if (live && fm_sum) {
#pragma unroll
    for (int h = 0; h < NV; ++h)
      st4(fm_sum + b * D + q * CPL + h * 4, make_float4(acc[4 * h], acc[4 * h + 1], acc[4 * h + 2], acc[4 * h + 3]));
  }
}

template <int D>
const void* gather_kernel(bool u4, int ns, int nd) {
  if (u4) {
    if (ns == 0) return reinterpret_cast<const void*>(&emb_fwd_quant4<D, 0, 2>);
    if (nd == 0) return reinterpret_cast<const void*>(&emb_fwd_quant4<D, 4, 0>);
    return reinterpret_cast<const void*>(&emb_fwd_quant4<D, 4, 2>);
  }
  if (ns == 0) return reinterpret_cast<const void*>(&emb_fwd_quant<D, 0, 2>);
  if (nd == 0) return reinterpret_cast<const void*>(&emb_fwd_quant<D, 4, 0>);
  return reinterpret_cast<const void*>(&emb_fwd_quant<D, 4, 2>);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int dfm_quant_row_bytes(int dim, int format) {
  if (!quant_dim_ok(dim)) return 0;
  if (format == DFM_QUANT_INT8_ROWWISE) return kHeaderBytes + dim;
  if (format == DFM_QUANT_UINT4_ROWWISE) return kHeaderBytes4 + dim / 2;
  return 0;
}

#define DFM_QUANT_CHECK_SHAPE(dim, format)                                                                          \
  do {                                                                                                              \
    if ((format) != DFM_QUANT_INT8_ROWWISE && (format) != DFM_QUANT_UINT4_ROWWISE)                                  \
      return fail(DFM_ERR_UNSUPPORTED, "quantised format %d: DFM_QUANT_INT8_ROWWISE and DFM_QUANT_UINT4_ROWWISE only", \
                  (format));                                                                                        \
    if (!quant_dim_ok(dim))                                                                                         \
      return fail(DFM_ERR_UNSUPPORTED, "quantised tables of width %d: widths 16, 32 and 64 only", (dim));           \
  } while (0)

extern "C" int dfm_quantize_rows(const float* d_w2, int64_t stride2, const float* d_w1, int64_t stride1, int64_t rows,
                                 int dim, int format, void* d_out, int32_t* d_flag, dfm_stream_t stream) {
  DFM_QUANT_CHECK_SHAPE(dim, format);
  DFM_REQUIRE(d_w2 && d_w1 && d_out && d_flag, "null argument");
  DFM_REQUIRE(rows >= 0 && rows < (int64_t(1) << 31), "rows %lld out of range", (long long)rows);
  DFM_REQUIRE(aligned16(d_w2) && stride2 % 4 == 0 && stride2 >= dim, "table rows must be 16-byte aligned, stride >= dim");
  DFM_REQUIRE(stride1 >= 1, "first-order stride must be positive");
  DFM_REQUIRE(aligned16(d_out), "records must be 16-byte aligned");
  if (rows == 0) return DFM_OK;
  const bool u4 = format == DFM_QUANT_UINT4_ROWWISE;
  const int64_t threads = rows * (dim / (u4 ? 8 : 4));
  const dim3 grid(static_cast<unsigned>((threads + kQuantThreads - 1) / kQuantThreads)), block(kQuantThreads);
  uint8_t* out = static_cast<uint8_t*>(d_out);
  hipStream_t st = as_stream(stream);
  const auto launch = [&](auto int8_kernel, auto uint4_kernel) {
    hipLaunchKernelGGL(u4 ? uint4_kernel : int8_kernel, grid, block, 0, st, d_w2, stride2, d_w1, stride1, rows, out, d_flag);
  };
  switch (dim) {
    case 16: launch(quant_rows_int8<16>, quant_rows_uint4<16>); break;
    case 32: launch(quant_rows_int8<32>, quant_rows_uint4<32>); break;
    default: launch(quant_rows_int8<64>, quant_rows_uint4<64>); break;
  }
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_dequantize_rows(const void* d_records, int64_t rows, int dim, int format, float* d_w2, float* d_w1,
                                   dfm_stream_t stream) {
  DFM_QUANT_CHECK_SHAPE(dim, format);
  DFM_REQUIRE(d_records, "null argument");
  DFM_REQUIRE(rows >= 0 && rows < (int64_t(1) << 31), "rows %lld out of range", (long long)rows);
  DFM_REQUIRE(aligned16(d_records) && aligned16(d_w2), "records and d_w2 must be 16-byte aligned");
  if (rows == 0 || (!d_w2 && !d_w1)) return DFM_OK;
  const bool u4 = format == DFM_QUANT_UINT4_ROWWISE;
  const int64_t threads = rows * (dim / (u4 ? 8 : 4));
  const dim3 grid(static_cast<unsigned>((threads + kQuantThreads - 1) / kQuantThreads)), block(kQuantThreads);
  const uint8_t* recs = static_cast<const uint8_t*>(d_records);
  hipStream_t st = as_stream(stream);
  const auto launch = [&](auto int8_kernel, auto uint4_kernel) {
    hipLaunchKernelGGL(u4 ? uint4_kernel : int8_kernel, grid, block, 0, st, recs, rows, d_w2, d_w1);
  };
  switch (dim) {
    case 16: launch(dequant_rows_int8<16>, dequant_rows_uint4<16>); break;
    case 32: launch(dequant_rows_int8<32>, dequant_rows_uint4<32>); break;
    default: launch(dequant_rows_int8<64>, dequant_rows_uint4<64>); break;
  }
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_embedding_forward_quant(const dfm_quant_field* fields, int num_fields, int dim, int format,
                                           const void* const* inputs, const float* d_extra_src, float* d_extra_dst,
                                           int64_t batch, float* d_first_order, float* d_field_emb, float* d_fm_out,
                                           float* d_fm_sum, int32_t* d_error_flag, const dfm_launch* at) {
  DFM_CHECK_LAUNCH(at);
  DFM_QUANT_CHECK_SHAPE(dim, format);
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
  const bool u4 = format == DFM_QUANT_UINT4_ROWWISE;
  const void* func = dim == 16 ? gather_kernel<16>(u4, ns, nd) : dim == 32 ? gather_kernel<32>(u4, ns, nd)
                                                                            : gather_kernel<64>(u4, ns, nd);
  const int spw = kWave / (dim / (u4 ? quant4_cols_per_lane(dim) : 4));
  int F = num_fields;
  void* params[] = {&args, &ns, &nd, &batch, &F, &d_first_order, &d_field_emb, &d_fm_out, &d_fm_sum, &d_error_flag,
                    &d_extra_src, &d_extra_dst};
  return launch_at(at, func, dim3(static_cast<unsigned>((batch + spw - 1) / spw)), dim3(kGatherWaves * 64), 0, params,
                   false);
}
