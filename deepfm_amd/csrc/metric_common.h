// What the evaluation kernels share (ranking, catalogue, grouped_auc, bootstrap, bootstrap_units, calibration,
// calibrator and the metrics of predict.hip): one copy of every piece that two of them must agree on.  The
// training-side reductions (loss.hip, step_tail.hip, shard.hip, tail_bodies.h) add in another order and are not served
// from here.
#pragma once

#include "common.h"
#include "dropout.h"   // mix32: the one counter hash of the library

namespace dfm {

// ---- host: grids and workspaces ---------------------------------------------------------------------------------
// workgroups for n items at per_block items each, at most max_blocks (0 for n == 0)
inline int blocks_for(int64_t n, int per_block, int max_blocks) {
  const int64_t b = (n + per_block - 1) / per_block;
  return static_cast<int>(b < max_blocks ? b : max_blocks);
}

inline size_t round16(size_t bytes) { return (bytes + 15) & ~size_t(15); }

// A cursor over a workspace: the arrays of a layout one after another.  Over a null base only `off` means anything
// (the *_workspace_bytes entry points).
struct Carver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off += sizeof(T) * count;
    return p;
  }
  void align16() { off = round16(off); }
};

constexpr int64_t kInvalidKey = INT64_MAX;   // the sort key of a sample that enters nothing: behind every real key

// ---- device -------------------------------------------------------------------------------------------------------
// the quiet NaN every "undefined" fp64 output holds (the bits of (double)NAN)
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// Order-preserving bits of a float: a < b  <=>  ord_bits(a) < ord_bits(b) for non-NaN a, b.  Every key format
// (ranking and catalogue: ord << 32 | ~row; grouped AUC: group << 33 | label << 32 | ord; bootstrap: ord << 27 | ...)
// relies on three facts: -0 maps as +0 (ties compare equal); ord_bits(-inf) = 0x007FFFFF is the smallest value, so
// every real key is > 0 and 0 can mean "none"; and the map is the same everywhere, so the orders agree.
__device__ __forceinline__ unsigned int ord_bits(float s) {
  const unsigned int b = __float_as_uint(s == 0.f ? 0.f : s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The label rule: exactly 1 is a positive, exactly 0 a negative, anything else (NaN included) is bad.
__device__ __forceinline__ void label_class(float y, bool& pos, bool& bad) {
  pos = y == 1.f;
  bad = !pos && y != 0.f;
}

// Sum over the wave in every lane: the xor butterfly o = 1, 2, ... 32.  For double this order is part of the result.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned long long w = __shfl_xor(v, o, kWave);
    v = w > v ? w : v;
  }
  return v;
}

// the first lane of a ballot mask (-1 for an empty one)
__device__ __forceinline__ int lane_of(unsigned long long mask) {
  return __ffsll(static_cast<long long>(mask)) - 1;
}

// v[0, M) summed over a workgroup of THREADS in one halving tree, x[t] += x[t + s] for s = THREADS / 2 .. 1: a fixed
// order, one barrier per level for all M values.  Thread 0 gets the sums in v; every thread may read sum q as
// red[q][0]: the last barrier is behind the last add, so a caller that hands `red` to another call puts a barrier
// between the two.
template <int M, int THREADS, typename T>
__device__ __forceinline__ void block_sums(T (&v)[M], T (*red)[THREADS]) {
  for (int q = 0; q < M; ++q) red[q][threadIdx.x] = v[q];
  __syncthreads();
#pragma unroll
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s)
      for (int q = 0; q < M; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    for (int q = 0; q < M; ++q) v[q] = red[q][0];
}

// Three fault flags of a wave's samples into their 64-bit counters: three ballots, then lane 0 adds each non-zero
// popcount with one atomic.  Every lane of the wave calls it (a lane without a sample passes false).
__device__ __forceinline__ void count_faults(bool flag0, bool flag1, bool flag2, unsigned long long* cell0,
                                             unsigned long long* cell1, unsigned long long* cell2) {
  const unsigned long long m0 = __ballot(flag0), m1 = __ballot(flag1), m2 = __ballot(flag2);
  if ((m0 | m1 | m2) && lane_id() == 0) {
    if (m0) atomicAdd(cell0, static_cast<unsigned long long>(__popcll(m0)));
    if (m1) atomicAdd(cell1, static_cast<unsigned long long>(__popcll(m1)));
    if (m2) atomicAdd(cell2, static_cast<unsigned long long>(__popcll(m2)));
  }
}

// ---- the Poisson bootstrap's weights (bootstrap.hip over samples, bootstrap_units.hip over per-unit columns) ------
// The counter of unit u in replicate r is bs_seed_base(seed) + (r << 40) + u, in wrapping uint64 arithmetic.
inline unsigned long long bs_seed_base(uint64_t seed) {
  return static_cast<unsigned long long>(seed) * 0x9E3779B97F4A7C15ull + 0x426F6F7453747261ull;
}

// The weight of a counter: Poisson(1) truncated at 12, T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!)
__device__ __forceinline__ uint32_t bs_weight(unsigned long long x) {
  const uint32_t h = mix32(x);
  return (h >= 1580030168u) + (h >= 3160060337u) + (h >= 3950075421u) + (h >= 4213413783u) + (h >= 4279248373u) +
         (h >= 4292415291u) + (h >= 4294609777u) + (h >= 4294923276u) + (h >= 4294962463u) + (h >= 4294966817u) +
         (h >= 4294967252u) + (h >= 4294967292u);
}

// ---- the walk over n (label, score[, id]) samples ---------------------------------------------------------------
// samples in front of the body at which both pointers are 16-byte aligned; -1 when there is no such count below 4
inline int pair_head(const float* a, const float* b) {
  for (int h = 0; h < 4; ++h)
    if ((reinterpret_cast<uintptr_t>(a + h) & 15) == 0 && (reinterpret_cast<uintptr_t>(b + h) & 15) == 0) return h;
  return -1;
}

// fn(label, score, id) for every sample: the aligned body four at a time (16-byte loads of the two float columns and,
// with kIds, two of the int64 column), the samples in front of and behind it (and everything when head < 0) one by
// one.  Without kIds `ids` is not read and fn gets 0.  The order in which a thread sees its samples depends on n,
// head and the launch geometry only.
template <int THREADS, bool kIds, typename Fn>
__device__ __forceinline__ void walk_pairs(const float* __restrict__ labels, const float* __restrict__ scores,
                                           const int64_t* __restrict__ ids, int64_t n, int head, Fn fn) {
  const int64_t first = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * THREADS;
  const int64_t nv = head < 0 ? 0 : (n - head) / 4;
  const int64_t h = head < 0 ? 0 : head;
  for (int64_t v = first; v < nv; v += stride) {
    const int64_t i = h + 4 * v;
    const float4 y4 = ld4(labels + i), z4 = ld4(scores + i);
    longlong2 a = {0, 0}, b = {0, 0};
    if (kIds) {
      a = *reinterpret_cast<const longlong2*>(ids + i);
      b = *reinterpret_cast<const longlong2*>(ids + i + 2);
    }
    fn(y4.x, z4.x, a.x);
    fn(y4.y, z4.y, a.y);
    fn(y4.z, z4.z, b.x);
    fn(y4.w, z4.w, b.y);
  }
  const int64_t rest = n - 4 * nv;
  for (int64_t r = first; r < rest; r += stride) {
    const int64_t i = r < h ? r : r + 4 * nv;
    fn(labels[i], scores[i], kIds ? ids[i] : 0);
  }
}

}  // namespace dfm
