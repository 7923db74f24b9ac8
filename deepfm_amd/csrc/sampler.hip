// The input side of an epoch on the device: per-epoch training negatives drawn from the per-user
// seen-sets, and batch records formed from device-resident columns in RecordLayout's byte format
// (data/packed.py), which dfm_embedding_forward_record and the fused steps read unchanged.
//
//   sample_negatives_kernel   one thread per positive: K exact rank-selects, uniform without replacement over the
//                             user's unseen item rows.  Work is bounded by K, log2(W) and 5 popcount probes: no
//                             rejection loop, a user who has seen nearly everything costs what any other does.
//   sample_weighted_kernel    one workgroup per query: C draws with replacement over the user's unseen rows, row i with
//                             probability w[i] / (sum of w over the unseen rows), integer arithmetic throughout
//                             (the reference's evaluation negatives, movielens.py:567-604).
//   record_assemble_kernel    one thread per (column, sample) element of one record ((sample, position) for a
//                             bag); a workgroup serves one column, consecutive lanes consecutive samples.  A column
//                             bound to a history index (dfm_assemble_plan_bind_history) is served by one wavefront per
//                             64 samples instead: its bags are formed from the index, never read from memory.
// Each of the three is instantiated for both shapes of a candidate list (dfm_candidate_list: K candidates per query,
// or counts[q] <= K of them at offsets[q] of a flat list, the reference's min(num_neg, unseen), movielens.py:575-580).
#include <vector>

#include "common.h"
#include "dropout.h"   // mix32: the one counter hash of the library
#include "history_body.h"

namespace dfm {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxNeg = 16;       // negatives per positive: the draw counter is 16 p + t
constexpr int kMaxEdges = 64;     // BUCKET_DIFF edges (a linear count per element)
constexpr int kMaxWeightedItems = 1 << 17;                       // _lib.WEIGHTED_MAX_ITEMS
constexpr int kMaxWeightedWords = kMaxWeightedItems / 32;        // the uint64 word prefixes live in LDS: 32 KiB + 8
constexpr uint64_t kWeightedSalt = 0xD1B54A32D192ED03ull;        // keeps the stream apart from the training sampler's

// The last w in [0, words) with pre[w] <= r; the caller has pre[0] <= r < pre[words].
template <typename T>
__device__ __forceinline__ int last_le(const T* pre, int words, T r) {
  int lo = 0, hi = words;                            // invariant: pre[lo] <= r < pre[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pre[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------------
// The first n <= kMaxNeg draws of positive p into out[0 .. n): draw t depends on (base, p, t) and on the draws before
// it only, so a query cut short at n receives the first n items of the longer draw.
__device__ __forceinline__ void draw_negatives(const uint32_t* __restrict__ seen, const uint32_t* __restrict__ prefix,
                                               int u, int n_users, int words, int64_t p, int n, uint64_t base,
                                               int32_t* __restrict__ out) {
  if (u < 0 || u >= n_users) {                       // never read outside the tables
    for (int t = 0; t < n; ++t) out[t] = -1;
    return;
  }
  const uint32_t* pre = prefix + static_cast<int64_t>(u) * (words + 1);
  const uint32_t* bits = seen + static_cast<int64_t>(u) * words;
  const uint32_t unseen = pre[words];
  uint32_t q[kMaxNeg];                               // ranks drawn so far, ascending (compile-time indices only)
#pragma unroll
  for (int i = 0; i < kMaxNeg; ++i) q[i] = 0xffffffffu;
  for (int t = 0; t < n; ++t) {
    if (unseen <= static_cast<uint32_t>(t)) {        // more draws than unseen rows: the caller refuses or truncates
      out[t] = -1;
      continue;
    }
    const uint32_t h = mix32(base + 16ull * static_cast<uint64_t>(p) + static_cast<uint64_t>(t));
    uint32_t r = static_cast<uint32_t>((static_cast<uint64_t>(h) * (unseen - t)) >> 32);
    // rank among the rows not drawn yet -> rank among all unseen rows
#pragma unroll
    for (int i = 0; i < kMaxNeg; ++i)
      if (i < t && r >= q[i]) ++r;
    // insert: carry the larger value up the sorted list
    uint32_t carry = r;
#pragma unroll
    for (int i = 0; i < kMaxNeg; ++i) {
      if (i < t) {
        if (q[i] > carry) { const uint32_t x = q[i]; q[i] = carry; carry = x; }
      } else if (i == t) {
        q[i] = carry;
      }
    }
    // select: the word with pre[w] <= r < pre[w + 1] (r < pre[words], so it exists), then the zero bit inside it
    const int lo = last_le(pre, words, r);
    const uint32_t z = ~bits[lo];
    uint32_t m = r - pre[lo];
    int pos = 0;
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) {
      const uint32_t c = __popc((z >> pos) & ((1u << s) - 1u));
      if (m >= c) { m -= c; pos += s; }
    }
    out[t] = lo * 32 + pos;
  }
}

// The slots of query p in the flat list: counts[p] of them from offsets[p] on, cut to `cap` and to the list, so that
// nothing past entry `total` is ever written whatever the two arrays hold.
__device__ __forceinline__ int ragged_slots(const dfm_candidate_list& list, int64_t p, int cap, int64_t* first) {
  const int64_t off = list.d_offsets[p];
  *first = off;
  if (off < 0 || off > list.total) return 0;
  const int64_t n = min(static_cast<int64_t>(min(list.d_counts[p], cap)), list.total - off);
  return n > 0 ? static_cast<int>(n) : 0;
}

// `list` is read by the ragged instantiation only: the rectangular one is handed an empty one.
template <bool kRagged>
__global__ __launch_bounds__(kBlock) void sample_negatives_kernel(
    const uint32_t* __restrict__ seen, const uint32_t* __restrict__ prefix, const int32_t* __restrict__ user_of,
    int64_t num_pos, int n_users, int words, int k, uint64_t base, int32_t* __restrict__ neg_items,
    dfm_candidate_list list) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (p >= num_pos) return;
  int64_t first = p * k;
  int n = k;
  if constexpr (kRagged) {
    n = ragged_slots(list, p, k, &first);
    if (n == 0) return;
  }
  draw_negatives(seen, prefix, user_of[p], n_users, words, p, n, base, neg_items + first);
}

// ---------------------------------------------------------------------------------------------------------------
// Weighted draws with replacement.  pre[w] = the summed weights of the unseen rows in words < w (uint64; at most
// 2^17 rows of at most 2^24 each: below 2^41), pre[words] = T.  Draw t: h = the 64-bit uniform of two mix32 values,
// r = mulhi(h, T) in [0, T), the item is the smallest unseen row whose inclusive prefix exceeds r.
// One workgroup draws the c candidates of query p into out[0 .. c); every thread of it makes the same call.
__device__ __forceinline__ void draw_weighted(const uint32_t* __restrict__ seen, const uint32_t* __restrict__ weight,
                                              int u, int n_users, int n_items, int words, int64_t p, int c,
                                              uint64_t base, int32_t* __restrict__ out) {
  extern __shared__ uint64_t pre[];                  // words + 1 prefixes, then kBlock chunk totals
  uint64_t* chunk = pre + words + 1;
  const int tid = threadIdx.x;
  if (u < 0 || u >= n_users) {                       // never read outside the tables
    for (int t = tid; t < c; t += kBlock) out[t] = -1;
    return;
  }
  const uint32_t* bits = seen + static_cast<int64_t>(u) * words;
  // per word: the summed weights of its unseen rows (32 weights of at most 2^24: below 2^30), coalesced over rows
  for (int i = tid; i < words * 32; i += kBlock) {
    uint32_t v = 0;
    if (i < n_items && !((bits[i >> 5] >> (i & 31)) & 1u)) v = weight[i];
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o, kWave);
    if ((i & 31) == 0) pre[i >> 5] = v;
  }
  __syncthreads();
  // exclusive scan: a contiguous chunk of words per thread, then the chunk totals
  const int per = (words + kBlock - 1) / kBlock;
  const int w0 = min(tid * per, words), w1 = min(w0 + per, words);
  uint64_t sum = 0;
  for (int w = w0; w < w1; ++w) sum += pre[w];
  chunk[tid] = sum;
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {
    const uint64_t add = tid >= o ? chunk[tid - o] : 0;
    __syncthreads();
    chunk[tid] += add;
    __syncthreads();
  }
  uint64_t run = chunk[tid] - sum;                   // the words before this thread's chunk
  for (int w = w0; w < w1; ++w) {
    const uint64_t x = pre[w];
    pre[w] = run;
    run += x;
  }
  if (tid == kBlock - 1) pre[words] = chunk[kBlock - 1];
  __syncthreads();
  const uint64_t total = pre[words];
  for (int t = tid; t < c; t += kBlock) {
    int32_t item = -1;
    if (total > 0) {
      const uint64_t ctr = base + (static_cast<uint64_t>(p) << 21) + 2ull * static_cast<uint64_t>(t);
      const uint64_t h = (static_cast<uint64_t>(mix32(ctr)) << 32) | mix32(ctr + 1);
      const uint64_t r = __umul64hi(h, total);
      const int lo = last_le<uint64_t>(pre, words, r);
      uint32_t z = ~bits[lo];
      if (lo == words - 1 && (n_items & 31)) z &= (1u << (n_items & 31)) - 1u;
      uint64_t rem = r - pre[lo];
      while (z) {                                    // at most 32 rows
        const int b = __ffs(static_cast<int>(z)) - 1;
        const uint32_t w = weight[lo * 32 + b];
        if (rem < w) { item = lo * 32 + b; break; }
        rem -= w;
        z &= z - 1;
      }
    }
    out[t] = item;
  }
}

// `list` stays ahead of the scalars: behind out_items the ragged instantiation fetches its arguments in one more load
// and measured 0.5 us of 35 slower (943 queries x 999 draws); the rectangular one never reads it.
template <bool kRagged>
__global__ __launch_bounds__(kBlock) void sample_weighted_kernel(
    const uint32_t* __restrict__ seen, const int32_t* __restrict__ user_of, const uint32_t* __restrict__ weight,
    dfm_candidate_list list, int n_users, int n_items, int words, int c, uint64_t base,
    int32_t* __restrict__ out_items) {
  const int64_t p = blockIdx.x;
  int64_t first = p * c;
  int n = c;
  if constexpr (kRagged) {
    n = ragged_slots(list, p, c, &first);              // the same for the whole workgroup
    if (n == 0) return;
  }
  draw_weighted(seen, weight, user_of[p], n_users, n_items, words, p, n, base, out_items + first);
}

// ---------------------------------------------------------------------------------------------------------------
enum { kOutId = 0, kOutFloat = 1, kOutBag = 2, kOutLabel = 3 };
enum { kZero = -1 };                                  // internal role: a padding row of the ids / dense block

struct HistorySource {                                // what a bound column forms its bags from
  HistoryIndex ix;
  int32_t mode;                                       // dfm_history_mode
};

struct Col {                                          // one output block of the record
  int32_t out, role, length, num_edges;
  int64_t offset;                                     // bytes from the record's start
  const void* pos;                                    // positive rows: int64 (P[, L]) or float (P); bound: queries (P)
  const void* item;                                   // ITEM: the item table's column; BUCKET_DIFF: item_val
  const float* ctx;
  const float* edges;
  const int64_t* bucket_ids;
  const HistorySource* hist;                          // a bag bound to a history index (device memory), or null
};

struct AssembleArgs {
  const Col* cols;
  const int2* block_col;                              // per workgroup: (column, its workgroup index inside it)
  const int64_t* order;                               // virtual row of every epoch slot, or null: the identity
  const int32_t* neg_items;                           // (P, K), or the flat list of a ragged plan
  const int64_t* offsets;                             // ragged: (P + 1), query p's candidates are [offsets[p], offsets[p+1])
  int64_t first, count, batch, num_pos;
  int64_t rows;                                       // virtual rows of the epoch: num_pos + the candidates
  int64_t top;                                        // ragged: the largest power of two below num_pos (0: one query)
  int32_t k, n_items;
  unsigned char* record;
};

// The query of candidate cand of a ragged plan: the last p with offsets[p] <= cand (offsets[0] = 0 <= cand, and the
// empty queries before a candidate share its offset, so the last one is its owner).  One probe per bit of
// num_pos - 1, the same count for every lane: at most 20 for 2^20 queries.
__device__ __forceinline__ int64_t query_of(const AssembleArgs& a, int64_t cand) {
  int64_t p = 0;
  for (int64_t step = a.top; step > 0; step >>= 1) {
    const int64_t mid = p + step;
    if (mid < a.num_pos && a.offsets[mid] <= cand) p = mid;
  }
  return p;
}

// Element e = (slot, l) of column c from the virtual row j (-1: padding): a positive, or the candidate `item` of
// query p.  The one statement of the roles for both plan shapes.
__device__ __forceinline__ void write_element(const AssembleArgs& a, const Col& c, int64_t e, int64_t l, int64_t j,
                                              int64_t p, int item) {
  const int64_t L = c.length;
  const bool neg = j >= a.num_pos;
  if (c.out == kOutLabel) {
    reinterpret_cast<float*>(a.record + c.offset)[e] = (j < 0 || neg) ? 0.f : static_cast<const float*>(c.pos)[j];
    return;
  }
  if (c.out == kOutFloat) {
    float v = 0.f;
    if (j >= 0) {
      if (!neg) v = static_cast<const float*>(c.pos)[j];
      else if (c.role == DFM_ROLE_ITEM) v = static_cast<const float*>(c.item)[item];
      else v = static_cast<const float*>(c.pos)[p];
    }
    reinterpret_cast<float*>(a.record + c.offset)[e] = v;
    return;
  }
  int64_t v = 0;                                      // SPARSE id or one position of a bag
  if (j >= 0) {
    if (!neg) {
      v = static_cast<const int64_t*>(c.pos)[j * L + l];
    } else if (c.role == DFM_ROLE_ITEM) {
      v = static_cast<const int64_t*>(c.item)[static_cast<int64_t>(item) * L + l];
    } else if (c.role == DFM_ROLE_BUCKET_DIFF) {
      const float x = c.ctx[p], y = static_cast<const float*>(c.item)[item];
      const float d = x - y;
      int b = 0;
      if (!(x != x) && !(y != y) && !(d < 0.f)) {
        b = 1;
        for (int i = 0; i < c.num_edges; ++i) b += c.edges[i] <= d ? 1 : 0;
      }
      v = c.bucket_ids[b];
    } else {
      v = static_cast<const int64_t*>(c.pos)[p * L + l];
    }
  }
  reinterpret_cast<int64_t*>(a.record + c.offset)[e] = v;
}

// Workgroup `block` of a column bound to a history index: a wavefront takes 64 slots, the structure of
// history_gather_kernel.  A lane resolves its slot's virtual row and owning positive, reads that positive's query and
// forms (segment start, prior count) once; then the 64 lanes write the 64 bags as one contiguous run of int64 words,
// the per-slot pair coming over by __shfl.  Every lane of a wavefront that stays makes every trip: nothing between here
// and the last __shfl returns or loops per lane.  A padding slot, a bad order entry and a query outside the index keep
// (0, 0): an all-zero bag.
template <bool kRagged>
__device__ __forceinline__ void assemble_history(const AssembleArgs& a, const Col& c, int block) {
  const int64_t first = (static_cast<int64_t>(block) * (kBlock / kWave) + wave_id_uniform()) * kWave;
  if (first >= a.batch) return;                                             // the whole wavefront leaves together
  const int lane = lane_id();
  const int slots_here = static_cast<int>(a.batch - first < kWave ? a.batch - first : kWave);
  const HistorySource& h = *c.hist;
  int32_t seg = 0, cnt = 0;
  const int64_t s = first + lane;
  if (lane < slots_here && s < a.count) {
    const int64_t j = a.order ? a.order[a.first + s] : a.first + s;
    if (j >= 0 && j < a.rows) {
      int64_t p = j;                                                        // a candidate takes its positive's bag
      if (j >= a.num_pos) p = kRagged ? query_of(a, j - a.num_pos) : (j - a.num_pos) / a.k;
      history_prior(h.ix, h.mode, static_cast<const int64_t*>(c.pos)[p], &seg, &cnt);
    }
  }
  const int length = c.length;
  const int total = slots_here * length;                                    // at most 64 * 4096 words
  const int step_q = kWave / length, step_j = kWave % length;
  int qi = lane / length, l = lane % length;
  int64_t* __restrict__ out = reinterpret_cast<int64_t*>(a.record + c.offset) + first * length;
  for (int base = 0; base < total; base += kWave) {                         // the trip count is the same for every lane
    const int src = qi < kWave ? qi : kWave - 1;
    const int32_t s_q = __shfl(seg, src, kWave), c_q = __shfl(cnt, src, kWave);
    const int w = base + lane;
    if (w < total) {
      bool bad;
      out[w] = history_slot(h.ix, s_q, c_q, l, &bad);
    }
    qi += step_q;
    l += step_j;
    if (l >= length) {
      l -= length;
      ++qi;
    }
  }
}

template <bool kRagged>
__global__ __launch_bounds__(kBlock) void record_assemble_kernel(AssembleArgs a) {
  const int2 bc = a.block_col[blockIdx.x];
  const Col c = a.cols[bc.x];
  if (c.hist) {                                                             // the same for the whole workgroup
    assemble_history<kRagged>(a, c, bc.y);
    return;
  }
  const int64_t e = static_cast<int64_t>(bc.y) * kBlock + threadIdx.x;
  const int64_t L = c.length;
  if (e >= a.batch * L) return;
  const int64_t s = e / L, l = e - s * L;
  // the virtual row: j < P a positive, else a candidate of positive p (rectangular: negative t of p = cand / k)
  int64_t j = -1, p = 0;
  int item = -1;
  if (s < a.count && c.role != kZero) {
    j = a.order ? a.order[a.first + s] : a.first + s;
    if (j < 0 || j >= a.rows) j = -1;                                       // a bad order entry is written as padding
    if (j >= a.num_pos) {
      p = kRagged ? query_of(a, j - a.num_pos) : (j - a.num_pos) / a.k;
      const int it = a.neg_items[j - a.num_pos];                            // == neg_items[p][t]
      item = (it >= 0 && it < a.n_items) ? it : -1;
      if (item < 0 && c.role != DFM_ROLE_COPY) j = -1;
    }
  }
  write_element(a, c, e, l, j, p, item);
}

}  // namespace
}  // namespace dfm

using namespace dfm;

struct dfm_assemble_plan {
  Col* d_cols = nullptr;
  int2* d_block_col = nullptr;
  int num_blocks = 0;
  std::vector<Col> cols;                              // the host copy of d_cols: binding a column changes both
  int user_cols = 0;                                  // the caller's columns lead `cols`; the extras follow
  std::vector<HistorySource*> d_hist;                 // per caller's column: its bound source (device), or null
  int64_t batch = 0, num_pos = 0, record_bytes = 0;
  int k = 0, n_items = 0;
  bool ragged = false;                                // then the candidates of query p are [offsets[p], offsets[p+1])
  const int64_t* d_offsets = nullptr;                 // the caller's (num_pos + 1), alive as long as the plan
  int64_t total = 0, top = 0;
};

constexpr int64_t kMaxLogRows = (int64_t{1} << 31) - 1;         // history.hip:kMaxRows

static bool aligned_to(const void* p, size_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

// plan->cols into d_cols (allocated by the caller, the count never changes) and the launch map they need, rebuilt:
// 256 elements per workgroup of a plain column, 256 slots per workgroup of a column bound to a history index.
static hipError_t upload_columns(dfm_assemble_plan* plan) {
  std::vector<int2> block_col;
  for (size_t ci = 0; ci < plan->cols.size(); ++ci) {
    const Col& c = plan->cols[ci];
    const int64_t blocks = (plan->batch * (c.hist ? 1 : c.length) + kBlock - 1) / kBlock;
    for (int64_t b = 0; b < blocks; ++b) block_col.push_back(make_int2(static_cast<int>(ci), static_cast<int>(b)));
  }
  hipError_t e = hipMemcpy(plan->d_cols, plan->cols.data(), sizeof(Col) * plan->cols.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) return e;
  (void)hipFree(plan->d_block_col);
  plan->d_block_col = nullptr;
  plan->num_blocks = 0;
  e = hipMalloc(reinterpret_cast<void**>(&plan->d_block_col), sizeof(int2) * block_col.size());
  if (e == hipSuccess)
    e = hipMemcpy(plan->d_block_col, block_col.data(), sizeof(int2) * block_col.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) plan->num_blocks = static_cast<int>(block_col.size());
  return e;
}

// The start of the counter stream of one (seed, epoch), wrapping uint64.
static uint64_t stream_base(uint64_t seed, uint64_t epoch) { return seed * 0x9E3779B97F4A7C15ull + (epoch << 40); }

// What the two draws share: the table sizes, then what they require of a ragged list on the host.  The arrays
// themselves are the caller's to get right (data/device_epoch.py checks them); the kernels cut every query to the list
// whatever they hold.  *total: the entries to draw, 0 when there is nothing to launch (no user has an unseen row).
static int check_draw(int n_users, int n_items, const dfm_candidate_list* list, int64_t n, int cap, int64_t* total) {
  DFM_REQUIRE(n_users >= 1 && n_items >= 1, "n_users and n_items must be positive");
  *total = list ? list->total : n * cap;
  if (!list) return DFM_OK;
  DFM_REQUIRE(list->d_counts && list->d_offsets, "null argument");
  DFM_REQUIRE(*total >= 0 && *total <= n * cap, "total_candidates %lld outside [0, %lld]", (long long)*total,
              (long long)(n * cap));
  return DFM_OK;
}

extern "C" int dfm_sample_negatives(const uint32_t* d_seen, const uint32_t* d_prefix, const int32_t* d_user_of,
                                    int64_t num_pos, int n_users, int n_items, int k, uint64_t seed, uint64_t epoch,
                                    const dfm_candidate_list* list, int32_t* d_neg_items, dfm_stream_t stream) {
  DFM_REQUIRE(d_seen && d_prefix && d_user_of, "null argument");
  DFM_REQUIRE(num_pos >= 1 && num_pos <= (int64_t{1} << 36), "num_pos %lld outside [1, 2^36]", (long long)num_pos);
  DFM_REQUIRE(k >= 1 && k <= kMaxNeg, "k = %d outside [1, %d]", k, kMaxNeg);
  int64_t total;
  if (int rc = check_draw(n_users, n_items, list, num_pos, k, &total)) return rc;
  if (total == 0) return DFM_OK;
  DFM_REQUIRE(d_neg_items, "null argument");
  const int words = (n_items + 31) / 32;
  const int64_t blocks = (num_pos + kBlock - 1) / kBlock;
  DFM_REQUIRE(blocks <= 0x7fffffff, "too many positives for one launch");
  hipLaunchKernelGGL(list ? sample_negatives_kernel<true> : sample_negatives_kernel<false>,
                     dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, as_stream(stream), d_seen, d_prefix,
                     d_user_of, num_pos, n_users, words, k, stream_base(seed, epoch), d_neg_items,
                     list ? *list : dfm_candidate_list{});
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_sample_weighted(const uint32_t* d_seen, const int32_t* d_user_of, const uint32_t* d_weight,
                                   int64_t num_queries, int n_users, int n_items, int c, uint64_t seed, uint64_t epoch,
                                   const dfm_candidate_list* list, int32_t* d_items, dfm_stream_t stream) {
  DFM_REQUIRE(d_seen && d_user_of && d_weight, "null argument");
  DFM_REQUIRE(num_queries >= 1 && num_queries <= (int64_t{1} << 19), "num_queries %lld outside [1, 2^19]",
              (long long)num_queries);
  DFM_REQUIRE(c >= 1 && c <= DFM_MAX_CANDIDATES, "c = %d outside [1, %d]", c, DFM_MAX_CANDIDATES);
  int64_t total;
  if (int rc = check_draw(n_users, n_items, list, num_queries, c, &total)) return rc;
  if (n_items > kMaxWeightedItems)
    return fail(DFM_ERR_UNSUPPORTED, "n_items = %d: the word prefixes of more than %d items do not fit the LDS", n_items,
                kMaxWeightedItems);
  if (total == 0) return DFM_OK;
  DFM_REQUIRE(d_items, "null argument");
  const int words = (n_items + 31) / 32;
  static_assert(kMaxWeightedWords * 8 + 8 + kBlock * 8 <= 65536, "the prefixes must fit 64 KiB of LDS");
  const size_t lds = sizeof(uint64_t) * (static_cast<size_t>(words) + 1 + kBlock);
  hipLaunchKernelGGL(list ? sample_weighted_kernel<true> : sample_weighted_kernel<false>,
                     dim3(static_cast<unsigned>(num_queries)), dim3(kBlock), lds, as_stream(stream), d_seen, d_user_of,
                     d_weight, list ? *list : dfm_candidate_list{}, n_users, n_items, words, c,
                     stream_base(seed, epoch) + kWeightedSalt, d_items);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

// What a plan requires of a ragged list: it is read back once and checked here, so that no launch of the plan can
// leave neg_items.
static int check_plan_list(const dfm_candidate_list& list, int64_t num_pos, int k) {
  DFM_REQUIRE(list.d_counts && list.d_offsets, "null argument");
  DFM_REQUIRE(num_pos >= 1 && num_pos <= (int64_t{1} << 36), "num_pos %lld outside [1, 2^36]", (long long)num_pos);
  DFM_REQUIRE(k >= 1 && k <= DFM_MAX_CANDIDATES, "a ragged plan needs k in [1, %d]", DFM_MAX_CANDIDATES);
  std::vector<int32_t> counts(static_cast<size_t>(num_pos));
  std::vector<int64_t> offsets(static_cast<size_t>(num_pos) + 1);
  hipError_t e = hipMemcpy(counts.data(), list.d_counts, sizeof(int32_t) * counts.size(), hipMemcpyDeviceToHost);
  if (e == hipSuccess)
    e = hipMemcpy(offsets.data(), list.d_offsets, sizeof(int64_t) * offsets.size(), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(DFM_ERR_HIP, "reading the ragged list failed: %s", hipGetErrorString(e));
  int64_t run = 0;
  for (int64_t p = 0; p < num_pos; ++p) {
    DFM_REQUIRE(counts[p] >= 0 && counts[p] <= k, "counts[%lld] = %d outside [0, k = %d]", (long long)p, counts[p], k);
    DFM_REQUIRE(offsets[p] == run, "offsets[%lld] = %lld is not the sum %lld of the counts before it", (long long)p,
                (long long)offsets[p], (long long)run);
    run += counts[p];
  }
  DFM_REQUIRE(offsets[num_pos] == run && list.total == run,
              "offsets[num_pos] = %lld and total_candidates = %lld must both be the sum %lld of the counts",
              (long long)offsets[num_pos], (long long)list.total, (long long)run);
  return DFM_OK;
}

extern "C" int dfm_assemble_plan_create(const dfm_assemble_column* columns, int num_columns, int64_t batch,
                                        int id_rows, int dense_rows, int64_t dense_offset, int64_t labels_offset,
                                        int64_t record_bytes, const float* d_labels, int64_t num_pos, int n_items,
                                        int k, const dfm_candidate_list* list, dfm_assemble_plan** out_plan) {
  if (list)
    if (int rc = check_plan_list(*list, num_pos, k)) return rc;
  DFM_REQUIRE(columns && out_plan && d_labels, "null argument");
  DFM_REQUIRE(num_columns > 0 && num_columns <= DFM_MAX_FIELDS, "num_columns %d outside [1, %d]", num_columns,
              DFM_MAX_FIELDS);
  DFM_REQUIRE(batch >= 1 && batch <= (1 << 24), "batch %lld outside [1, 2^24]", (long long)batch);
  DFM_REQUIRE(num_pos >= 1 && k >= 0 && k <= DFM_MAX_CANDIDATES, "num_pos must be positive and k in [0, %d]",
              DFM_MAX_CANDIDATES);
  DFM_REQUIRE(num_pos <= INT64_MAX / (1 + static_cast<int64_t>(k)), "num_pos * (1 + k) overflows the row index");
  DFM_REQUIRE(k == 0 || n_items >= 1, "negatives need an item table");
  DFM_REQUIRE(id_rows >= 1 && dense_rows >= 1, "a record holds at least one ids row and one dense row");
  DFM_REQUIRE(dense_offset == 8 * batch * id_rows && labels_offset == dense_offset + 4 * batch * dense_rows &&
                  record_bytes >= labels_offset + 4 * batch,
              "the block offsets are not those of a record of %d ids rows and %d dense rows", id_rows, dense_rows);
  std::vector<Col> cols;
  int ns = 0, nd = 0;
  for (int f = 0; f < num_columns; ++f) {
    const dfm_assemble_column& s = columns[f];
    Col c{};
    DFM_REQUIRE(s.kind >= DFM_SPARSE && s.kind <= DFM_SEQUENCE, "column %d: bad kind %d", f, s.kind);
    DFM_REQUIRE(s.role >= DFM_ROLE_COPY && s.role <= DFM_ROLE_BUCKET_DIFF, "column %d: bad role %d", f, s.role);
    DFM_REQUIRE(s.pos != nullptr, "column %d: no positive rows", f);
    c.out = s.kind == DFM_SPARSE ? kOutId : s.kind == DFM_DENSE ? kOutFloat : kOutBag;
    c.role = s.role;
    c.length = s.kind == DFM_SEQUENCE ? s.length : 1;
    DFM_REQUIRE(c.length >= 1 && c.length <= 4096, "column %d: bag length %d outside [1, 4096]", f, c.length);
    const int64_t bytes = batch * c.length * (s.kind == DFM_DENSE ? 4 : 8);
    DFM_REQUIRE(s.record_offset >= 0 && s.record_offset % (s.kind == DFM_DENSE ? 4 : 8) == 0 &&
                    s.record_offset + bytes <= record_bytes,
                "column %d: its block leaves the record", f);
    if (s.kind == DFM_SPARSE) {
      DFM_REQUIRE(s.record_offset == 8 * batch * ns && ns < id_rows, "column %d: not row %d of the ids block", f, ns);
      ++ns;
    } else if (s.kind == DFM_DENSE) {
      DFM_REQUIRE(s.record_offset == dense_offset + 4 * batch * nd && nd < dense_rows,
                  "column %d: not row %d of the dense block", f, nd);
      ++nd;
    } else {
      DFM_REQUIRE(s.record_offset >= labels_offset + 4 * batch, "column %d: the bag overlaps the labels", f);
    }
    if (k > 0 && s.role == DFM_ROLE_ITEM) DFM_REQUIRE(s.item != nullptr, "column %d: ITEM without a table column", f);
    if (s.role == DFM_ROLE_BUCKET_DIFF) {
      DFM_REQUIRE(s.kind == DFM_SPARSE, "column %d: BUCKET_DIFF is for SPARSE fields", f);
      DFM_REQUIRE(s.num_edges >= 0 && s.num_edges <= kMaxEdges, "column %d: %d edges outside [0, %d]", f,
                  s.num_edges, kMaxEdges);
      DFM_REQUIRE(k == 0 || (s.item && s.ctx && s.bucket_ids && (s.edges || s.num_edges == 0)),
                  "column %d: BUCKET_DIFF needs ctx, item values, edges and bucket ids", f);
    }
    c.num_edges = s.num_edges;
    c.offset = s.record_offset;
    c.pos = s.pos; c.item = s.item; c.ctx = s.ctx; c.edges = s.edges; c.bucket_ids = s.bucket_ids;
    cols.push_back(c);
  }
  DFM_REQUIRE(ns == id_rows || (ns == 0 && id_rows == 1), "%d SPARSE columns for %d ids rows", ns, id_rows);
  DFM_REQUIRE(nd == dense_rows || (nd == 0 && dense_rows == 1), "%d DENSE columns for %d dense rows", nd, dense_rows);
  auto extra = [&](int out, int role, int64_t offset, const void* pos) {
    Col c{};
    c.out = out; c.role = role; c.length = 1; c.offset = offset; c.pos = pos;
    cols.push_back(c);
  };
  if (ns == 0) extra(kOutId, kZero, 0, nullptr);                   // the padding row of an empty block
  if (nd == 0) extra(kOutFloat, kZero, dense_offset, nullptr);
  extra(kOutLabel, DFM_ROLE_COPY, labels_offset, d_labels);
  auto* plan = new dfm_assemble_plan();
  plan->user_cols = num_columns;
  plan->cols = cols;
  plan->d_hist.assign(static_cast<size_t>(num_columns), nullptr);
  plan->batch = batch; plan->num_pos = num_pos; plan->record_bytes = record_bytes;
  plan->k = k; plan->n_items = n_items;
  if (list) { plan->ragged = true; plan->d_offsets = list->d_offsets; plan->total = list->total; }
  for (int64_t t = 1; plan->ragged && t < num_pos; t *= 2) plan->top = t;      // the largest power of two below num_pos
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&plan->d_cols), sizeof(Col) * cols.size());
  if (e == hipSuccess) e = upload_columns(plan);
  if (e != hipSuccess) {
    dfm_assemble_plan_destroy(plan);
    return fail(DFM_ERR_HIP, "plan upload failed: %s", hipGetErrorString(e));
  }
  *out_plan = plan;
  return DFM_OK;
}
extern "C" int dfm_assemble_plan_destroy(dfm_assemble_plan* plan) {
  if (!plan) return DFM_OK;
  (void)hipFree(plan->d_cols);
  (void)hipFree(plan->d_block_col);
  for (HistorySource* h : plan->d_hist) (void)hipFree(h);
  delete plan;
  return DFM_OK;
}

extern "C" int dfm_assemble_plan_bind_history(dfm_assemble_plan* plan, int column, const dfm_history_source* source) {
  DFM_REQUIRE(plan && source, "null argument");
  DFM_REQUIRE(column >= 0 && column < plan->user_cols, "column %d outside [0, %d)", column, plan->user_cols);
  const dfm_history_source& s = *source;
  Col& c = plan->cols[static_cast<size_t>(column)];
  DFM_REQUIRE(c.out == kOutBag, "column %d: only a SEQUENCE column is bound to a history index", column);
  DFM_REQUIRE(c.role == DFM_ROLE_COPY, "column %d: role %d: a history is its positive's (DFM_ROLE_COPY)", column,
              c.role);
  DFM_REQUIRE(s.mode == DFM_HISTORY_POSITION || s.mode == DFM_HISTORY_EXCLUDE || s.mode == DFM_HISTORY_LATEST,
              "mode = %d: expected DFM_HISTORY_POSITION, DFM_HISTORY_EXCLUDE or DFM_HISTORY_LATEST", s.mode);
  DFM_REQUIRE(s.n >= 0 && s.n <= kMaxLogRows, "n = %lld outside [0, 2^31)", (long long)s.n);
  DFM_REQUIRE(s.n_users >= 1 && s.n_users <= kMaxLogRows, "n_users = %lld outside [1, 2^31)", (long long)s.n_users);
  DFM_REQUIRE(s.n_items >= 1 && s.n_items <= kMaxLogRows, "n_items = %lld outside [1, 2^31)", (long long)s.n_items);
  DFM_REQUIRE(s.d_start && s.d_event_count, "null argument");
  DFM_REQUIRE((s.d_user_rows && s.d_item_rows && s.d_timestamps && s.d_pos_of && s.d_rank && s.d_events &&
               s.d_sorted_ts) || s.n == 0,
              "null argument");
  DFM_REQUIRE(aligned_to(c.pos, 8) && aligned_to(s.d_user_rows, 8) && aligned_to(s.d_item_rows, 8) &&
                  aligned_to(s.d_timestamps, 8) && aligned_to(s.d_item_ids, 8) && aligned_to(s.d_start, 8) &&
                  aligned_to(s.d_pos_of, 4) && aligned_to(s.d_rank, 4) && aligned_to(s.d_events, 4) &&
                  aligned_to(s.d_sorted_ts, 8) && aligned_to(s.d_event_count, 4),
              "misaligned argument");
  HistorySource h{};
  h.ix = HistoryIndex{s.d_user_rows, s.d_item_rows, s.d_timestamps, s.d_item_ids, s.d_start,  s.d_pos_of, s.d_rank,
                      s.d_events,    s.d_sorted_ts, s.d_event_count, s.n,        s.n_users,  s.n_items};
  h.mode = s.mode;
  HistorySource*& d_h = plan->d_hist[static_cast<size_t>(column)];
  hipError_t e = d_h ? hipSuccess : hipMalloc(reinterpret_cast<void**>(&d_h), sizeof(HistorySource));
  if (e == hipSuccess) e = hipMemcpy(d_h, &h, sizeof(HistorySource), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    c.hist = d_h;
    e = upload_columns(plan);                         // a bound column has its own workgroup count
  }
  if (e != hipSuccess) return fail(DFM_ERR_HIP, "binding the history failed: %s", hipGetErrorString(e));
  return DFM_OK;
}

extern "C" int dfm_record_assemble(const dfm_assemble_plan* plan, const int64_t* d_order, int64_t first,
                                   int64_t count, const int32_t* d_neg_items, void* d_record, dfm_stream_t stream) {
  DFM_REQUIRE(plan && d_record, "null argument");
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(d_record) % 16 == 0, "batch records must be 16-byte aligned");
  DFM_REQUIRE(count >= 0 && count <= plan->batch, "count %lld outside [0, %lld]", (long long)count,
              (long long)plan->batch);
  const int64_t rows = plan->ragged ? plan->num_pos + plan->total : plan->num_pos * (1 + plan->k);
  DFM_REQUIRE(first >= 0 && first + count <= rows, "rows [%lld, %lld) outside the epoch's %lld", (long long)first,
              (long long)(first + count), (long long)rows);
  DFM_REQUIRE(plan->k == 0 || d_neg_items || (plan->ragged && plan->total == 0), "a plan with negatives needs neg_items");
  AssembleArgs a;
  a.cols = plan->d_cols; a.block_col = plan->d_block_col; a.order = d_order; a.neg_items = d_neg_items;
  a.first = first; a.count = count; a.batch = plan->batch; a.num_pos = plan->num_pos;
  a.k = plan->k; a.n_items = plan->n_items;
  a.offsets = plan->d_offsets; a.rows = rows; a.top = plan->top;
  a.record = static_cast<unsigned char*>(d_record);
  if (plan->ragged)
    hipLaunchKernelGGL(record_assemble_kernel<true>, dim3(plan->num_blocks), dim3(kBlock), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(record_assemble_kernel<false>, dim3(plan->num_blocks), dim3(kBlock), 0, as_stream(stream), a);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
