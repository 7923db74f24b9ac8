// Full-catalogue selection: per query, the first K eligible item rows in the project's ranking
// order and the rank of a target row, from a (Q, n_items) score matrix.  The reference has no such call: its
// evaluation ranks 1 + 999 sampled candidates (trainer.py:296-332); this is the unsampled form of the same metric.
//
// The order is csrc/ranking.hip's: key(i) = ord_bits(score_i) << 32 | (0xFFFFFFFF - i), larger first, so descending
// score, ties by ascending row, -0 == +0 (metric_common.h).  Keys are distinct (the row is in the low word) and every
// real key is above 0, so an ineligible row is key 0 and "the K largest" is one exact set.
//
//   catalogue_topk_kernel   one workgroup per query.
//     pass 0   keys from the score row and the user's seen bits (kept in LDS when the row fits kLdsKeys, else
//              recomputed from memory by every later pass); counts of eligible rows, of NaN scores among them and
//              of the eligible rows ahead of the target
//     select   more than K eligible rows: radix select of the K-th largest key, 8 bits a pass from the top: a
//              256-bin LDS histogram of the keys that match the digits fixed so far, a suffix scan, one bin chosen
//     collect  the keys >= the K-th (exactly min(K, eligible) of them) into LDS, each placed by the number of
//              survivors above it; the K scores are read again by row so that a -0.0 leaves as it came
//
// Integer comparisons and integer LDS atomics only: every output is bitwise reproducible.
#include "metric_common.h"

using namespace dfm;

namespace {

constexpr int kThreads = 256;
constexpr int kLdsKeys = 6144;               // 48 KiB of keys: a row up to this long is read from memory once
constexpr int kMaxK = 128;

struct Row {
  const float* scores;                       // the query's n_items scores
  const uint32_t* bits;                      // the user's seen words, or null: every row is eligible
  int n_items, target;
};

__device__ __forceinline__ unsigned long long make_key(const Row& r, int i, float s) {
  const bool eligible = !r.bits || i == r.target || !((r.bits[i >> 5] >> (i & 31)) & 1u);
  return eligible ? (static_cast<unsigned long long>(ord_bits(s)) << 32) | (0xFFFFFFFFu - static_cast<unsigned int>(i))
                  : 0ull;
}

template <bool kInLds>
__device__ __forceinline__ unsigned long long key_at(const Row& r, const unsigned long long* keys, int i) {
  return kInLds ? keys[i] : make_key(r, i, r.scores[i]);
}

template <bool kInLds>
__global__ __launch_bounds__(kThreads) void catalogue_topk_kernel(
    const float* __restrict__ scores, const uint32_t* __restrict__ seen, const int32_t* __restrict__ user_of,
    const int32_t* __restrict__ target_of, int n_users, int n_items, int words, int K, int exclude_seen,
    int32_t* __restrict__ out_items, float* __restrict__ out_scores, int32_t* __restrict__ out_rank,
    unsigned long long* __restrict__ status) {
  extern __shared__ unsigned long long keys[];       // n_items keys when kInLds
  __shared__ unsigned long long surv[kMaxK];
  __shared__ unsigned int hist[kThreads];
  __shared__ unsigned int counts[4];                 // eligible, NaN, ahead of the target, survivors
  __shared__ unsigned long long sel_prefix;
  __shared__ unsigned int sel_k;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  int32_t* o_items = out_items + q * K;
  float* o_scores = out_scores + q * K;
  const int u = user_of[q];
  int target = target_of ? target_of[q] : -1;
  const bool bad_target = target < -1 || target >= n_items;
  if (bad_target) target = -1;
  if (u < 0 || u >= n_users) {                       // never read outside the tables
    for (int j = tid; j < K; j += kThreads) { o_items[j] = -1; o_scores[j] = -INFINITY; }
    if (tid == 0) {
      out_rank[q] = -1;
      atomicAdd(&status[1], 1ull);
      if (bad_target) atomicAdd(&status[2], 1ull);
    }
    return;
  }
  Row r;
  r.scores = scores + q * n_items;
  r.bits = exclude_seen ? seen + static_cast<int64_t>(u) * words : nullptr;
  r.n_items = n_items; r.target = target;
  if (tid < 4) counts[tid] = 0;
  __syncthreads();
  // ---- pass 0
  unsigned long long tkey = 0;
  if (target >= 0) tkey = make_key(r, target, r.scores[target]);
  unsigned int n_el = 0, n_nan = 0, n_ahead = 0;
  for (int i = tid; i < n_items; i += kThreads) {
    const float s = r.scores[i];
    const unsigned long long k = make_key(r, i, s);
    if (kInLds) keys[i] = k;
    n_el += k != 0;
    n_nan += (k != 0 && s != s);
    n_ahead += k > tkey;                             // tkey == 0 without a target: the count is not used
  }
  if (n_el) atomicAdd(&counts[0], n_el);
  if (n_nan) atomicAdd(&counts[1], n_nan);
  if (n_ahead) atomicAdd(&counts[2], n_ahead);
  __syncthreads();
  const unsigned int eligible = counts[0];
  if (tid == 0) {
    out_rank[q] = target >= 0 ? static_cast<int32_t>(counts[2]) : -1;
    if (counts[1]) atomicAdd(&status[0], static_cast<unsigned long long>(counts[1]));
    if (bad_target) atomicAdd(&status[2], 1ull);
  }
  // ---- select: thr = the K-th largest key, or 1 (every real key) when at most K rows are eligible
  unsigned long long thr = 1;
  if (eligible > static_cast<unsigned int>(K)) {
    if (tid == 0) { sel_prefix = 0; sel_k = static_cast<unsigned int>(K); }
    for (int shift = 56; shift >= 0; shift -= 8) {
      hist[tid] = 0;
      __syncthreads();
      const unsigned long long prefix = sel_prefix;
      const unsigned int want = sel_k;
      const unsigned long long mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
      for (int i = tid; i < n_items; i += kThreads) {
        const unsigned long long k = key_at<kInLds>(r, keys, i);
        if (k != 0 && (k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
      }
      __syncthreads();
      // suffix sums: hist[b] = the matching keys whose digit is >= b
      for (int o = 1; o < kThreads; o <<= 1) {
        const unsigned int add = tid + o < kThreads ? hist[tid + o] : 0;
        __syncthreads();
        hist[tid] += add;
        __syncthreads();
      }
      const unsigned int above = tid + 1 < kThreads ? hist[tid + 1] : 0;
      if (hist[tid] >= want && above < want) {       // exactly one digit holds the want-th largest
        sel_prefix = prefix | (static_cast<unsigned long long>(tid) << shift);
        sel_k = want - above;
      }
      __syncthreads();
    }
    thr = sel_prefix;
  }
  // ---- collect
  for (int i = tid; i < n_items; i += kThreads) {
    const unsigned long long k = key_at<kInLds>(r, keys, i);
    if (k >= thr) {                                  // thr >= 1: never an ineligible row
      const unsigned int slot = atomicAdd(&counts[3], 1u);
      if (slot < kMaxK) surv[slot] = k;
    }
  }
  __syncthreads();
  const int ns = min(static_cast<int>(counts[3]), K);
  for (int j = tid; j < K; j += kThreads) {
    if (j < ns) {
      const unsigned long long k = surv[j];
      int pos = 0;
      for (int m = 0; m < ns; ++m) pos += surv[m] > k;
      const int row = static_cast<int>(0xFFFFFFFFu - static_cast<unsigned int>(k));
      o_items[pos] = row;
      o_scores[pos] = r.scores[row];
    } else {
      o_items[j] = -1;                               // positions ns .. K-1: no survivor is placed there
      o_scores[j] = -INFINITY;
    }
  }
}

}  // namespace

extern "C" int dfm_catalogue_topk(const float* d_scores, const uint32_t* d_seen, const int32_t* d_user_of,
                                  const int32_t* d_target, int64_t num_queries, int n_users, int n_items, int k,
                                  int exclude_seen, int32_t* d_out_items, float* d_out_scores, int32_t* d_out_rank,
                                  uint64_t* d_status, dfm_stream_t stream) {
  DFM_REQUIRE(d_scores && d_user_of && d_out_items && d_out_scores && d_out_rank && d_status, "null argument");
  DFM_REQUIRE(d_seen || !exclude_seen, "exclude_seen needs the seen-sets");
  DFM_REQUIRE(num_queries >= 1 && num_queries <= 0x7fffffff, "num_queries %lld outside [1, 2^31)",
              (long long)num_queries);
  DFM_REQUIRE(n_users >= 1 && n_items >= 1, "n_users and n_items must be positive");
  DFM_REQUIRE(k >= 1 && k <= kMaxK, "k = %d outside [1, %d]", k, kMaxK);
  if (n_items > DFM_MAX_CANDIDATES)
    return fail(DFM_ERR_UNSUPPORTED, "n_items = %d above the %d rows a selection takes", n_items, DFM_MAX_CANDIDATES);
  const hipStream_t st = as_stream(stream);
  DFM_HIP_TRY(hipMemsetAsync(d_status, 0, 3 * sizeof(uint64_t), st));
  const int words = (n_items + 31) / 32;
  auto* status = reinterpret_cast<unsigned long long*>(d_status);
  const dim3 grid(static_cast<unsigned>(num_queries)), block(kThreads);
  if (n_items <= kLdsKeys) {
    hipLaunchKernelGGL(catalogue_topk_kernel<true>, grid, block, sizeof(unsigned long long) * n_items, st, d_scores,
                       d_seen, d_user_of, d_target, n_users, n_items, words, k, exclude_seen ? 1 : 0, d_out_items,
                       d_out_scores, d_out_rank, status);
  } else {
    hipLaunchKernelGGL(catalogue_topk_kernel<false>, grid, block, 0, st, d_scores, d_seen, d_user_of, d_target,
                       n_users, n_items, words, k, exclude_seen ? 1 : 0, d_out_items, d_out_scores, d_out_rank,
                       status);
  }
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
