// The interaction log on the device: the integer work of the reference's adapter between reading the
// ratings and fitting the encoders (deepfm/data/movielens.py:235-304, 334-344, 467-480).  Integer atomics (or / add /
// 64-bit min) and plain stores only, so every output is the same bits whatever order the threads run in.
//
//   seen_init_kernel        every bitmap word: 0, or the bits at and above n_items in a user's last word
//   seen_scatter_kernel     one thread per interaction: one atomic or
//   seen_prefix_kernel      one wavefront per user: 64 words per trip, popcount, wave scan, running carry
//   counts_lds_kernel       the histogram of a workgroup's rows in LDS (uint32), its non-zero counters added to memory
//   counts_global_kernel    one 64-bit atomic add per selected row
//   temporal_*_kernel       init; mark the users of the train positions; 64-bit atomic min of the window positions
//   loo_roles_kernel        one thread per sorted position, which looks at the users of its two successors
//
// A row that names something outside its table is counted in d_status and used for nothing.
#include "common.h"
#include "wave_scan.h"

namespace dfm {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;                         // grid-stride beyond: 256 CUs x 8 workgroups
constexpr int64_t kMaxRows = (int64_t{1} << 31) - 1;
constexpr int64_t kSeenMaxBytes = int64_t{1} << 30;      // data/device_epoch.py:SEEN_SETS_MAX_BYTES
constexpr int kCountsRowsPerLdsBlock = 16 * kBlock;      // an LDS histogram is worth its flush from this many rows on

using u64 = unsigned long long;

__device__ __forceinline__ bool inside(int64_t v, int64_t n) { return v >= 0 && v < n; }

unsigned grid_for(int64_t work, int64_t per_block = kBlock) {
  const int64_t blocks = (work + per_block - 1) / per_block;
  return static_cast<unsigned>(blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks));
}

// ---------------------------------------------------------------------------------------------- seen-sets
__global__ __launch_bounds__(kBlock) void seen_init_kernel(uint32_t* __restrict__ bitmap, int64_t n_users, int64_t W,
                                                           uint32_t tail_mask) {
  const int64_t total = n_users * W, stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += stride)
    bitmap[e] = (e % W == W - 1) ? tail_mask : 0u;
}

__global__ __launch_bounds__(kBlock) void seen_scatter_kernel(const int64_t* __restrict__ users,
                                                              const int64_t* __restrict__ items, int64_t n,
                                                              int64_t n_users, int64_t n_items, int64_t W,
                                                              uint32_t* __restrict__ bitmap, u64* __restrict__ status) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; r < n; r += stride) {
    const int64_t u = users[r], i = items[r];
    if (inside(u, n_users) && inside(i, n_items))
      atomicOr(&bitmap[u * W + (i >> 5)], 1u << (i & 31));
    else
      atomicAdd(&status[0], 1ull);
  }
}

__global__ __launch_bounds__(kBlock) void seen_prefix_kernel(const uint32_t* __restrict__ bitmap, int64_t n_users,
                                                             int64_t W, uint32_t* __restrict__ prefix) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + wave_id_uniform();
  if (u >= n_users) return;                              // the whole wavefront leaves together
  const int lane = lane_id();
  const uint32_t* __restrict__ words = bitmap + u * W;
  uint32_t* __restrict__ out = prefix + u * (W + 1);
  uint32_t carry = 0;
  if (lane == 0) out[0] = 0;
  for (int64_t base = 0; base < W; base += kWave) {      // the trip count is the same for every lane
    const int64_t w = base + lane;
    const uint32_t zeros = w < W ? 32u - static_cast<uint32_t>(__popc(words[w])) : 0u;
    const uint32_t incl = wave_inclusive_sum(zeros);
    if (w < W) out[w + 1] = carry + incl;
    carry += __shfl(incl, kWave - 1, kWave);
  }
}

// ---------------------------------------------------------------------------------------------- counts
// The entity row selected row s counts for, or -1: not selected by its label, or refused and counted in status.
__device__ __forceinline__ int64_t counted_entity(const int64_t* __restrict__ entity, const float* __restrict__ labels,
                                                  const int64_t* __restrict__ index, int64_t s, int64_t n_log,
                                                  int64_t n_entities, u64* __restrict__ status) {
  int64_t r = s;
  if (index) {
    r = index[s];
    if (!inside(r, n_log)) {
      atomicAdd(&status[1], 1ull);
      return -1;
    }
  }
  const int64_t e = entity[r];
  if (!inside(e, n_entities)) {
    atomicAdd(&status[0], 1ull);
    return -1;
  }
  return (labels && labels[r] != 1.0f) ? -1 : e;
}

__global__ __launch_bounds__(kBlock) void counts_lds_kernel(const int64_t* __restrict__ entity,
                                                            const float* __restrict__ labels,
                                                            const int64_t* __restrict__ index, int64_t m, int64_t n_log,
                                                            int n_entities, u64* __restrict__ counts,
                                                            u64* __restrict__ status) {
  __shared__ uint32_t hist[DFM_COUNTS_LDS_ENTITIES];     // a workgroup sees fewer than 2^31 rows
  for (int e = threadIdx.x; e < n_entities; e += kBlock) hist[e] = 0;
  __syncthreads();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; s < m; s += stride) {
    const int64_t e = counted_entity(entity, labels, index, s, n_log, n_entities, status);
    if (e >= 0) atomicAdd(&hist[e], 1u);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n_entities; e += kBlock) {
    const uint32_t c = hist[e];
    if (c) atomicAdd(&counts[e], static_cast<u64>(c));
  }
}

__global__ __launch_bounds__(kBlock) void counts_global_kernel(const int64_t* __restrict__ entity,
                                                               const float* __restrict__ labels,
                                                               const int64_t* __restrict__ index, int64_t m,
                                                               int64_t n_log, int64_t n_entities,
                                                               u64* __restrict__ counts, u64* __restrict__ status) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; s < m; s += stride) {
    const int64_t e = counted_entity(entity, labels, index, s, n_log, n_entities, status);
    if (e >= 0) atomicAdd(&counts[e], 1ull);
  }
}

// ---------------------------------------------------------------------------------------------- temporal split
__global__ __launch_bounds__(kBlock) void temporal_init_kernel(int64_t n, int64_t n_users, uint8_t* __restrict__ in_train,
                                                               u64* __restrict__ first_val, u64* __restrict__ first_test) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; u < n_users; u += stride) {
    in_train[u] = 0;
    first_val[u] = static_cast<u64>(n);
    first_test[u] = static_cast<u64>(n);
  }
}

// The user row of sorted position p, or -1 (counted, when `count`: each position is counted by one kernel only).
__device__ __forceinline__ int64_t user_at(const int64_t* __restrict__ users, const int64_t* __restrict__ order,
                                           int64_t p, int64_t n, int64_t n_users, int64_t* row,
                                           u64* __restrict__ status, bool count) {
  const int64_t r = order[p];
  if (inside(r, n)) {
    const int64_t u = users[r];
    if (inside(u, n_users)) {
      *row = r;
      return u;
    }
  }
  if (count) atomicAdd(&status[0], 1ull);
  return -1;
}

__global__ __launch_bounds__(kBlock) void temporal_train_users_kernel(const int64_t* __restrict__ users,
                                                                      const int64_t* __restrict__ order, int64_t n,
                                                                      int64_t n_users, int64_t n_train,
                                                                      uint8_t* __restrict__ in_train,
                                                                      u64* __restrict__ status) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; p < n_train; p += stride) {
    int64_t r;
    const int64_t u = user_at(users, order, p, n, n_users, &r, status, true);
    if (u >= 0) in_train[u] = 1;                         // every writer stores the same byte
  }
}

__global__ __launch_bounds__(kBlock) void temporal_first_kernel(const int64_t* __restrict__ users,
                                                                const float* __restrict__ labels,
                                                                const int64_t* __restrict__ order, int64_t n,
                                                                int64_t n_users, int64_t n_train, int64_t n_trainval,
                                                                const uint8_t* __restrict__ in_train,
                                                                u64* __restrict__ first_val, u64* __restrict__ first_test,
                                                                u64* __restrict__ status) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t p = n_train + static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; p < n; p += stride) {
    int64_t r;
    const int64_t u = user_at(users, order, p, n, n_users, &r, status, true);
    if (u < 0 || labels[r] != 1.0f || !in_train[u]) continue;
    atomicMin(p < n_trainval ? &first_val[u] : &first_test[u], static_cast<u64>(p));
  }
}

// ---------------------------------------------------------------------------------------------- leave one out
__global__ __launch_bounds__(kBlock) void loo_roles_kernel(const int64_t* __restrict__ users,
                                                           const int64_t* __restrict__ order,
                                                           const int64_t* __restrict__ user_counts, int64_t n,
                                                           int64_t n_users, int64_t min_interactions,
                                                           uint8_t* __restrict__ roles, u64* __restrict__ status) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; p < n; p += stride) {
    int64_t r;
    const int64_t u = user_at(users, order, p, n, n_users, &r, status, true);
    uint8_t role = 0;
    if (u >= 0 && user_counts[u] >= min_interactions) {
      const int64_t u1 = p + 1 < n ? user_at(users, order, p + 1, n, n_users, &r, status, false) : -1;
      if (u1 != u) {
        role = 2;
      } else {
        const int64_t u2 = p + 2 < n ? user_at(users, order, p + 2, n, n_users, &r, status, false) : -1;
        if (u2 != u) role = 1;
      }
    }
    roles[p] = role;
  }
}

bool aligned(const void* p, size_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

}  // namespace
}  // namespace dfm

using namespace dfm;

extern "C" int dfm_seen_sets_build(const int64_t* d_user_rows, const int64_t* d_item_rows, int64_t n, int64_t n_users,
                                   int64_t n_items, uint32_t* d_bitmap, uint32_t* d_prefix, uint64_t* d_status,
                                   dfm_stream_t stream) {
  DFM_REQUIRE(n >= 0 && n <= kMaxRows, "n = %lld outside [0, 2^31)", (long long)n);
  DFM_REQUIRE(n_users >= 1 && n_items >= 1 && n_users <= kSeenMaxBytes && n_items <= 32 * kSeenMaxBytes,
              "n_users = %lld, n_items = %lld: both must be positive", (long long)n_users, (long long)n_items);
  const int64_t W = (n_items + 31) / 32;
  DFM_REQUIRE(2 * W + 1 <= kSeenMaxBytes / 4 / n_users,
              "the seen-sets of %lld users x %lld items take more than %lld bytes", (long long)n_users,
              (long long)n_items, (long long)kSeenMaxBytes);
  DFM_REQUIRE(d_bitmap && d_prefix && d_status && ((d_user_rows && d_item_rows) || n == 0), "null argument");
  DFM_REQUIRE(aligned(d_bitmap, 4) && aligned(d_prefix, 4) && aligned(d_status, 8) && aligned(d_user_rows, 8) &&
                  aligned(d_item_rows, 8),
              "misaligned argument");
  const uint32_t tail_mask = (n_items % 32) ? 0xFFFFFFFFu << (n_items % 32) : 0u;
  hipLaunchKernelGGL(seen_init_kernel, dim3(grid_for(n_users * W)), dim3(kBlock), 0, as_stream(stream), d_bitmap,
                     n_users, W, tail_mask);
  DFM_LAUNCH_CHECK();
  if (n > 0) {
    hipLaunchKernelGGL(seen_scatter_kernel, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), d_user_rows,
                       d_item_rows, n, n_users, n_items, W, d_bitmap, reinterpret_cast<u64*>(d_status));
    DFM_LAUNCH_CHECK();
  }
  const int64_t blocks = (n_users + kBlock / kWave - 1) / (kBlock / kWave);
  hipLaunchKernelGGL(seen_prefix_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, as_stream(stream),
                     d_bitmap, n_users, W, d_prefix);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_entity_counts(const int64_t* d_entity_rows, const float* d_labels, const int64_t* d_index, int64_t m,
                                 int64_t n_log, int64_t n_entities, int64_t* d_counts, uint64_t* d_status,
                                 dfm_stream_t stream) {
  DFM_REQUIRE(n_log >= 0 && n_log <= kMaxRows, "n_log = %lld outside [0, 2^31)", (long long)n_log);
  if (!d_index) m = n_log;
  DFM_REQUIRE(m >= 0 && m <= kMaxRows, "m = %lld outside [0, 2^31)", (long long)m);
  DFM_REQUIRE(n_entities >= 1 && n_entities <= kMaxRows, "n_entities = %lld outside [1, 2^31)", (long long)n_entities);
  DFM_REQUIRE(d_counts && d_status && (d_entity_rows || m == 0), "null argument");
  DFM_REQUIRE(aligned(d_counts, 8) && aligned(d_status, 8) && aligned(d_entity_rows, 8) && aligned(d_index, 8) &&
                  aligned(d_labels, 4),
              "misaligned argument");
  DFM_HIP_TRY(hipMemsetAsync(d_counts, 0, static_cast<size_t>(n_entities) * sizeof(int64_t), as_stream(stream)));
  if (m == 0) return DFM_OK;
  u64* counts = reinterpret_cast<u64*>(d_counts);
  u64* status = reinterpret_cast<u64*>(d_status);
  if (n_entities <= DFM_COUNTS_LDS_ENTITIES) {
    hipLaunchKernelGGL(counts_lds_kernel, dim3(grid_for(m, kCountsRowsPerLdsBlock)), dim3(kBlock), 0, as_stream(stream),
                       d_entity_rows, d_labels, d_index, m, n_log, static_cast<int>(n_entities), counts, status);
  } else {
    hipLaunchKernelGGL(counts_global_kernel, dim3(grid_for(m)), dim3(kBlock), 0, as_stream(stream), d_entity_rows,
                       d_labels, d_index, m, n_log, n_entities, counts, status);
  }
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_temporal_split_mark(const int64_t* d_user_rows, const float* d_labels, const int64_t* d_order,
                                       int64_t n, int64_t n_users, int64_t n_train, int64_t n_trainval,
                                       uint8_t* d_in_train, int64_t* d_first_val, int64_t* d_first_test,
                                       uint64_t* d_status, dfm_stream_t stream) {
  DFM_REQUIRE(n >= 0 && n <= kMaxRows, "n = %lld outside [0, 2^31)", (long long)n);
  DFM_REQUIRE(n_users >= 1 && n_users <= kMaxRows, "n_users = %lld outside [1, 2^31)", (long long)n_users);
  DFM_REQUIRE(0 <= n_train && n_train <= n_trainval && n_trainval <= n,
              "need 0 <= n_train = %lld <= n_trainval = %lld <= n = %lld", (long long)n_train, (long long)n_trainval,
              (long long)n);
  DFM_REQUIRE(d_in_train && d_first_val && d_first_test && d_status && ((d_user_rows && d_labels && d_order) || n == 0),
              "null argument");
  DFM_REQUIRE(aligned(d_first_val, 8) && aligned(d_first_test, 8) && aligned(d_status, 8) && aligned(d_user_rows, 8) &&
                  aligned(d_order, 8) && aligned(d_labels, 4),
              "misaligned argument");
  u64* first_val = reinterpret_cast<u64*>(d_first_val);
  u64* first_test = reinterpret_cast<u64*>(d_first_test);
  u64* status = reinterpret_cast<u64*>(d_status);
  hipLaunchKernelGGL(temporal_init_kernel, dim3(grid_for(n_users)), dim3(kBlock), 0, as_stream(stream), n, n_users,
                     d_in_train, first_val, first_test);
  DFM_LAUNCH_CHECK();
  if (n_train > 0) {
    hipLaunchKernelGGL(temporal_train_users_kernel, dim3(grid_for(n_train)), dim3(kBlock), 0, as_stream(stream),
                       d_user_rows, d_order, n, n_users, n_train, d_in_train, status);
    DFM_LAUNCH_CHECK();
  }
  if (n > n_train) {
    hipLaunchKernelGGL(temporal_first_kernel, dim3(grid_for(n - n_train)), dim3(kBlock), 0, as_stream(stream),
                       d_user_rows, d_labels, d_order, n, n_users, n_train, n_trainval, d_in_train, first_val,
                       first_test, status);
    DFM_LAUNCH_CHECK();
  }
  return DFM_OK;
}

extern "C" int dfm_loo_split_mark(const int64_t* d_user_rows, const int64_t* d_order, const int64_t* d_user_counts,
                                  int64_t n, int64_t n_users, int64_t min_interactions, uint8_t* d_roles,
                                  uint64_t* d_status, dfm_stream_t stream) {
  DFM_REQUIRE(n >= 0 && n <= kMaxRows, "n = %lld outside [0, 2^31)", (long long)n);
  DFM_REQUIRE(n_users >= 1 && n_users <= kMaxRows, "n_users = %lld outside [1, 2^31)", (long long)n_users);
  DFM_REQUIRE(min_interactions >= 2, "min_interactions = %lld: a user gives two rows away, so at least 2",
              (long long)min_interactions);
  if (n == 0) return DFM_OK;
  DFM_REQUIRE(d_user_rows && d_order && d_user_counts && d_roles && d_status, "null argument");
  DFM_REQUIRE(aligned(d_user_rows, 8) && aligned(d_order, 8) && aligned(d_user_counts, 8) && aligned(d_status, 8),
              "misaligned argument");
  hipLaunchKernelGGL(loo_roles_kernel, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), d_user_rows, d_order,
                     d_user_counts, n, n_users, min_interactions, d_roles, reinterpret_cast<u64*>(d_status));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
