// User histories on the device (DESIGN.md §7b "User histories on the device"): per query row of the interaction log,
// the items its user interacted with before it, latest first, from an index that is built once per log.
//
//   history_index_kernel    one wavefront per user over its segment of the (user, timestamp, position) order: 64
//                           positions per trip, a uniform trip count, wave scan of the event flags, running carry;
//                           the user's events are compacted into the front of its own segment
//   history_gather_kernel   one wavefront per 64 queries: a lane forms one query's (start, prior count, gap) once, then
//                           the lanes write the 64 bags as one contiguous run of int64
//
// Plain loads and stores only (the status counters are the one atomic), no LDS, no workgroup waits on another.  Every
// index that comes out of memory is checked before it is used as one.
#include "common.h"
#include "history_body.h"
#include "wave_scan.h"

namespace dfm {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int64_t kMaxRows = (int64_t{1} << 31) - 1;
constexpr int64_t kHistoryMaxBytes = int64_t{1} << 32;   // data/interactions.py:HISTORY_MAX_BYTES

using u64 = unsigned long long;

__device__ __forceinline__ bool inside(int64_t v, int64_t n) { return v >= 0 && v < n; }

// ---------------------------------------------------------------------------------------------- the index
__global__ __launch_bounds__(kBlock) void history_index_kernel(
    const int64_t* __restrict__ users, const int64_t* __restrict__ items, const int64_t* __restrict__ ts,
    const float* __restrict__ labels, const uint8_t* __restrict__ mask, const int64_t* __restrict__ order,
    const int64_t* __restrict__ start, int64_t n, int64_t n_users, int64_t n_items, int32_t* __restrict__ pos_of,
    int32_t* __restrict__ rank, int32_t* __restrict__ events, int64_t* __restrict__ sorted_ts,
    int32_t* __restrict__ event_count, u64* __restrict__ status) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (u >= n_users) return;                              // the whole wavefront leaves together
  const int lane = lane_id();
  const int64_t s = start[u], e = start[u + 1];
  if (s < 0 || e < s || e > n) {                         // not a segment of the log: nothing of it is touched
    if (lane == 0) {
      event_count[u] = 0;
      atomicAdd(&status[0], 1ull);
    }
    return;
  }
  uint32_t carry = 0;
  for (int64_t base = s; base < e; base += kWave) {      // the trip count is the same for every lane
    const int64_t p = base + lane;
    const bool valid = p < e;
    int64_t r = -1, t = 0;
    bool event = false;
    if (valid) {
      r = order[p];
      bool ok = inside(r, n);
      if (ok) ok = users[r] == u && inside(items[r], n_items);
      if (ok) {
        t = ts[r];
        event = (!labels || labels[r] == 1.0f) && (!mask || mask[r] != 0);
      } else {
        atomicAdd(&status[0], 1ull);
        r = -1;
      }
    }
    const uint32_t incl = wave_inclusive_sum(event ? 1u : 0u);
    const uint32_t before = carry + incl - (event ? 1u : 0u);
    if (valid) {
      rank[p] = static_cast<int32_t>(before);
      sorted_ts[p] = t;
      if (r >= 0) pos_of[r] = static_cast<int32_t>(p);
      if (event) events[s + before] = static_cast<int32_t>(r);      // before < p - s + 1: inside the segment
    }
    carry += __shfl(incl, kWave - 1, kWave);
  }
  if (lane == 0) event_count[u] = static_cast<int32_t>(carry);
}

// ---------------------------------------------------------------------------------------------- the bags
// The prior-set rule itself (history_prior, history_slot) is csrc/history_body.h's: the record assembly forms the bags
// of a bound column by the same two functions.
template <int MODE>
__global__ __launch_bounds__(kBlock) void history_gather_kernel(const int64_t* __restrict__ queries, int64_t m,
                                                                int length, HistoryIndex ix, int64_t* __restrict__ bag,
                                                                int64_t* __restrict__ count, int64_t* __restrict__ gap,
                                                                u64* __restrict__ status) {
  const int64_t first = (static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform()) * kWave;
  if (first >= m) return;                                // the whole wavefront leaves together
  const int lane = lane_id();
  const int queries_here = static_cast<int>(m - first < kWave ? m - first : kWave);

  // one query per lane: the first position of its user's segment, its prior count, its gap
  int32_t seg = 0, c = 0;
  int64_t g = -1;
  if (lane < queries_here) {
    const int64_t q = queries[first + lane];
    if (!history_prior(ix, MODE, q, &seg, &c)) {
      atomicAdd(&status[0], 1ull);
    } else if (MODE != DFM_HISTORY_LATEST && c > 0) {
      const int64_t e0 = ix.events[static_cast<int64_t>(seg) + c - 1];
      if (inside(e0, ix.n)) g = ix.ts[q] - ix.ts[e0];
    }
    count[first + lane] = c;
    gap[first + lane] = g;
  }

  // the 64 bags are one contiguous run of queries_here * length words: consecutive lanes, consecutive words
  const int total = queries_here * length;
  const int step_q = kWave / length, step_j = kWave % length;
  int qi = lane / length, j = lane % length;
  int64_t* __restrict__ out = bag + first * length;
  for (int base = 0; base < total; base += kWave) {      // the trip count is the same for every lane
    const int src = qi < kWave ? qi : kWave - 1;
    const int32_t s_q = __shfl(seg, src, kWave), c_q = __shfl(c, src, kWave);
    const int w = base + lane;
    if (w < total) {
      bool bad;
      const int64_t id = history_slot(ix, s_q, c_q, j, &bad);
      if (bad) atomicAdd(&status[1], 1ull);
      out[w] = id;
    }
    qi += step_q;
    j += step_j;
    if (j >= length) {
      j -= length;
      ++qi;
    }
  }
}

bool aligned(const void* p, size_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

}  // namespace
}  // namespace dfm

using namespace dfm;

extern "C" int dfm_history_index_build(const int64_t* d_user_rows, const int64_t* d_item_rows,
                                       const int64_t* d_timestamps, const float* d_labels, const uint8_t* d_source_mask,
                                       const int64_t* d_order, const int64_t* d_start, int64_t n, int64_t n_users,
                                       int64_t n_items, int32_t* d_pos_of, int32_t* d_rank, int32_t* d_events,
                                       int64_t* d_sorted_ts, int32_t* d_event_count, uint64_t* d_status,
                                       dfm_stream_t stream) {
  DFM_REQUIRE(n >= 0 && n <= kMaxRows, "n = %lld outside [0, 2^31)", (long long)n);
  DFM_REQUIRE(n_users >= 1 && n_users <= kMaxRows, "n_users = %lld outside [1, 2^31)", (long long)n_users);
  DFM_REQUIRE(n_items >= 1 && n_items <= kMaxRows, "n_items = %lld outside [1, 2^31)", (long long)n_items);
  DFM_REQUIRE(d_start && d_event_count && d_status, "null argument");
  DFM_REQUIRE((d_user_rows && d_item_rows && d_timestamps && d_order && d_pos_of && d_rank && d_events &&
               d_sorted_ts) || n == 0,
              "null argument");
  DFM_REQUIRE(aligned(d_user_rows, 8) && aligned(d_item_rows, 8) && aligned(d_timestamps, 8) && aligned(d_labels, 4) &&
                  aligned(d_order, 8) && aligned(d_start, 8) && aligned(d_pos_of, 4) && aligned(d_rank, 4) &&
                  aligned(d_events, 4) && aligned(d_sorted_ts, 8) && aligned(d_event_count, 4) && aligned(d_status, 8),
              "misaligned argument");
  const int64_t blocks = (n_users + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(history_index_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, as_stream(stream),
                     d_user_rows, d_item_rows, d_timestamps, d_labels, d_source_mask, d_order, d_start, n, n_users,
                     n_items, d_pos_of, d_rank, d_events, d_sorted_ts, d_event_count, reinterpret_cast<u64*>(d_status));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_history_gather(const int64_t* d_queries, int64_t m, int mode, int length, const int64_t* d_user_rows,
                                  const int64_t* d_item_rows, const int64_t* d_timestamps, const int64_t* d_item_ids,
                                  const int64_t* d_start, const int32_t* d_pos_of, const int32_t* d_rank,
                                  const int32_t* d_events, const int64_t* d_sorted_ts, const int32_t* d_event_count,
                                  int64_t n, int64_t n_users, int64_t n_items, int64_t* d_bag, int64_t* d_count,
                                  int64_t* d_gap, uint64_t* d_status, dfm_stream_t stream) {
  DFM_REQUIRE(mode == DFM_HISTORY_POSITION || mode == DFM_HISTORY_EXCLUDE || mode == DFM_HISTORY_LATEST,
              "mode = %d: expected DFM_HISTORY_POSITION, DFM_HISTORY_EXCLUDE or DFM_HISTORY_LATEST", mode);
  DFM_REQUIRE(length >= 1 && length <= DFM_HISTORY_MAX_LENGTH, "length = %d outside [1, %d]", length,
              DFM_HISTORY_MAX_LENGTH);
  DFM_REQUIRE(n >= 0 && n <= kMaxRows, "n = %lld outside [0, 2^31)", (long long)n);
  DFM_REQUIRE(m >= 0 && m <= kMaxRows, "m = %lld outside [0, 2^31)", (long long)m);
  DFM_REQUIRE(m * length * 8 <= kHistoryMaxBytes, "%lld bags of %d ids take more than %lld bytes", (long long)m, length,
              (long long)kHistoryMaxBytes);
  DFM_REQUIRE(n_users >= 1 && n_users <= kMaxRows, "n_users = %lld outside [1, 2^31)", (long long)n_users);
  DFM_REQUIRE(n_items >= 1 && n_items <= kMaxRows, "n_items = %lld outside [1, 2^31)", (long long)n_items);
  if (m == 0) return DFM_OK;
  DFM_REQUIRE(d_queries && d_start && d_event_count && d_bag && d_count && d_gap && d_status, "null argument");
  DFM_REQUIRE((d_user_rows && d_item_rows && d_timestamps && d_pos_of && d_rank && d_events && d_sorted_ts) || n == 0,
              "null argument");
  DFM_REQUIRE(aligned(d_queries, 8) && aligned(d_user_rows, 8) && aligned(d_item_rows, 8) && aligned(d_timestamps, 8) &&
                  aligned(d_item_ids, 8) && aligned(d_start, 8) && aligned(d_pos_of, 4) && aligned(d_rank, 4) &&
                  aligned(d_events, 4) && aligned(d_sorted_ts, 8) && aligned(d_event_count, 4) && aligned(d_bag, 8) &&
                  aligned(d_count, 8) && aligned(d_gap, 8) && aligned(d_status, 8),
              "misaligned argument");
  const HistoryIndex ix{d_user_rows, d_item_rows, d_timestamps, d_item_ids, d_start,     d_pos_of, d_rank,
                        d_events,    d_sorted_ts, d_event_count, n,         n_users,     n_items};
  const dim3 grid(static_cast<unsigned>((m + kBlock - 1) / kBlock)), block(kBlock);
  u64* status = reinterpret_cast<u64*>(d_status);
  if (mode == DFM_HISTORY_POSITION)
    hipLaunchKernelGGL(history_gather_kernel<DFM_HISTORY_POSITION>, grid, block, 0, as_stream(stream), d_queries, m,
                       length, ix, d_bag, d_count, d_gap, status);
  else if (mode == DFM_HISTORY_EXCLUDE)
    hipLaunchKernelGGL(history_gather_kernel<DFM_HISTORY_EXCLUDE>, grid, block, 0, as_stream(stream), d_queries, m,
                       length, ix, d_bag, d_count, d_gap, status);
  else
    hipLaunchKernelGGL(history_gather_kernel<DFM_HISTORY_LATEST>, grid, block, 0, as_stream(stream), d_queries, m,
                       length, ix, d_bag, d_count, d_gap, status);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
