// The row-wise quantised record formats (include/deepfm_hip.h: DFM_QUANT_INT8_ROWWISE and DFM_QUANT_UINT4_ROWWISE) as
// one trait per format, Int8Rec<D> and Uint4Rec<D>, with the one-rounding arithmetic they are specified in.  Shared by
// quant.hip (the quantiser, its inverse, the uniform gather) and embedding.hip (the record gather over quantised
// fields): the header is compiled under either file's contraction setting, so everything that must stay two roundings
// goes through mul_rn / add_rn / sub_rn.
#pragma once

#include "common.h"

namespace dfm {
namespace qrec {

// One rounding each.  The header's __fmul_rn / __fadd_rn are plain operators compiled where contraction is allowed,
// so a product and a sum of theirs still fuse into an fma after inlining; these, compiled under the pragma inside,
// carry no permission to contract: neither with each other nor with an addition of the caller that takes their result.
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

// Codes of BITS bits, 32 / BITS to a payload dword, the first in the lowest bits.
// x' of codes 4h .. 4h + 3 of one payload dword
template <int BITS>
__device__ __forceinline__ float4 dequant4(uint32_t p, int h, float scale, float lo) {
  const auto value = [&](int k) {
    return add_rn(mul_rn(static_cast<float>((p >> BITS * (4 * h + k)) & ((1u << BITS) - 1)), scale), lo);
  };
  return make_float4(value(0), value(1), value(2), value(3));
}
// the codes of columns 4h .. 4h + 3 of a lane in their place in its payload dword; all 0 where ok is not set
template <int BITS>
__device__ __forceinline__ uint32_t quant4(const float4& x, int h, float lo, float scale, bool ok) {
  const auto code = [&](float v, int k) {
    const float c = fminf(rintf(sub_rn(v, lo) / scale), static_cast<float>((1 << BITS) - 1));
    return static_cast<uint32_t>(ok ? c : 0.f) << BITS * (4 * h + k);
  };
  return code(x.x, 0) | code(x.y, 1) | code(x.z, 2) | code(x.w, 3);
}

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

// ---- the record formats ---------------------------------------------------------------------------------------------
// A trait says, for records of width D:
//   kBits, kHeaderBytes, kRowBytes, kRowLanes   lanes per row in the quantiser and the inverse, one payload dword each
//   kCols                                       columns per lane in the gather (D / kCols lanes per sample)
//   Head, header(lo32, hi32, w1, bad)           the header as it is stored; the quantiser's, from a row's minimum and
//                                               maximum, with its refusals
//   widen(head)                                 the header's values in fp32: scale, lo, w1, 0
//   load(rec, q)                                the loads alone of lane q of the gather
//   row_bytes(d), load_piece(rec, d, p)         the same for a width known at run time (the record gather, where a
//                                               lane owns 4 columns whatever the format): the record size, and the
//                                               loads alone of piece p, columns 4p .. 4p + 3

// What a lane loads of a record: the header and, from bit 0 on, the lane's codes.
template <class Head>
struct RawRec {
  Head head;
  uint32_t pay;
};
// lane q of kRowLanes: the header (same address on the row's lanes: one request) and payload dword q
template <class Rec>
__device__ __forceinline__ RawRec<typename Rec::Head> load_lane(const uint8_t* rec, int q) {
  return {*reinterpret_cast<const typename Rec::Head*>(rec),
          *reinterpret_cast<const uint32_t*>(rec + Rec::kHeaderBytes + q * 4)};
}

// DFM_QUANT_INT8_ROWWISE: 16 + D bytes, [scale fp32 | lo fp32 | w1 fp32 | 0 | q, a byte each], 16-byte aligned.
template <int D>
struct Int8Rec {
  static constexpr int kDim = D, kBits = 8, kHeaderBytes = 16, kRowBytes = kHeaderBytes + D;
  static constexpr int kRowLanes = D / 4, kCols = 4;

  using Head = float4;        // scale, lo, w1, 0
  static __device__ __forceinline__ Head header(float lo32, float hi32, float w1, int& bad) {
    const float range = sub_rn(hi32, lo32);
    if (!isfinite(range)) bad = 1;               // hi - lo overflows
    return make_float4(range / 255.0f, lo32, w1, 0.f);
  }
  static __device__ __forceinline__ float4 widen(const Head& h) { return h; }
  static __device__ __forceinline__ RawRec<Head> load(const uint8_t* rec, int q) { return load_lane<Int8Rec>(rec, q); }
  static __device__ __forceinline__ int64_t row_bytes(int d) { return kHeaderBytes + d; }
  static __device__ __forceinline__ RawRec<Head> load_piece(const uint8_t* rec, int, int p) {
    return load_lane<Int8Rec>(rec, p);           // dword p of the payload is piece p
  }
};

// DFM_QUANT_UINT4_ROWWISE: 8 + D / 2 bytes, [scale binary16 | lo binary16 | w1 fp32 | q, 4 bits each], 8-byte aligned.
// In the gather a lane has 8 columns at D = 32 and 64 (16 / 8 samples per workgroup, 17 partial sums per lane in the
// reduction).  At D = 16 that would leave 128 workgroups for a batch of 4096, half as many as there are CUs, so a
// lane has 4 columns there as in the int8 gather; the record is 16 bytes and 16-byte aligned: one load, the same
// address on the row's lanes, of which lane q keeps 16 bits.
template <int D>
struct Uint4Rec {
  static constexpr int kDim = D, kBits = 4, kHeaderBytes = 8, kRowBytes = kHeaderBytes + D / 2;
  static constexpr int kRowLanes = D / 8, kCols = D == 16 ? 4 : 8;

  using Head = uint2;         // scale | lo << 16, w1
  static __device__ __forceinline__ Head header(float lo32, float hi32, float w1, int& bad) {
    const uint32_t lo_h = half_floor(lo32);
    const float lo = half_value(lo_h);
    uint32_t scale_h = half_ceil(sub_rn(hi32, lo) / 15.0f);
    // The subtract and the divide can both round down, onto a binary16 value that the ceiling then keeps: where
    // lo + 15 scale is still below hi (exact in fp64: the terms span under 53 bits), one more binary16 value up.
    if (static_cast<double>(lo) + 15.0 * static_cast<double>(half_value(scale_h)) < static_cast<double>(hi32)) scale_h += 1;
    if (half_is_inf(lo_h) || half_is_inf(scale_h)) bad = 1;    // lo below -65504, or a range past 15 * 65504
    return make_uint2(scale_h | (lo_h << 16), __float_as_uint(w1));
  }
  static __device__ __forceinline__ float4 widen(const Head& h) {
    return make_float4(half_value(h.x & 0xffffu), half_value(h.x >> 16), __uint_as_float(h.y), 0.f);
  }
  // all four payload halves of a 16-byte record in one load; half q from bit 0 on (dequant4 looks at 16 bits only)
  static __device__ __forceinline__ RawRec<Head> load16(const uint8_t* rec, int q) {
    const uint4 r = *reinterpret_cast<const uint4*>(rec);
    return {make_uint2(r.x, r.y), ((q & 2) ? r.w : r.z) >> (16 * (q & 1))};
  }
  static __device__ __forceinline__ RawRec<Head> load(const uint8_t* rec, int q) {
    if constexpr (D == 16) {
      return load16(rec, q);
    } else {
      return load_lane<Uint4Rec>(rec, q);
    }
  }
  static __device__ __forceinline__ int64_t row_bytes(int d) { return kHeaderBytes + d / 2; }
  static __device__ __forceinline__ RawRec<Head> load_piece(const uint8_t* rec, int d, int p) {
    if (d == 16) return load16(rec, p);
    RawRec<Head> r = load_lane<Uint4Rec>(rec, p >> 1);           // 16 bits of dword p / 2
    r.pay >>= 16 * (p & 1);
    return r;
  }
};

}  // namespace qrec
}  // namespace dfm
