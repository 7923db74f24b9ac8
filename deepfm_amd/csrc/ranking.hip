// Leave-one-out ranking metrics over a device score buffer (reference trainer.py:296-332 and
// RankingEvaluator.evaluate, metrics.py:62-111): HR@k and NDCG@k per user, averaged over the users.
//
// Per user everything reduces to one integer, the 0-based position of the user's first positive in the stable
// descending order of its scores (np.argsort(-s, kind="stable"): ties keep dataset order):
//
//   rank = #{j in u : s_j > s*} + #{j in u : s_j == s*, j < p*}     s* the best positive score, p* its lowest index
//
// With key(i) = ord(s_i) << 32 | (0xFFFFFFFF - i) (ord: the float's order-preserving unsigned bits, -0 == +0) the
// best positive is the positive of the largest key, and sample j precedes it exactly when key(j) > key(best).
//
//   rank_best      per sample: cnt | npos << 32 (one 64-bit add), atomicMax(best[u], key) for a positive;
//                  counts of bad ids, NaN scores and labels other than 0 / 1
//   rank_count     per sample: ahead[u] += key(i) > best[u]
//   rank_finalize  per user, in user-id order: qualify, HR / NDCG per k -> per-workgroup partials
//   rank_reduce    one workgroup: partials in a fixed order -> out
//
// dfm_ranking_user_ranks stops at the integers (the columns of the bootstrap over users, bootstrap_units.hip): the same
// two per-sample passes, then
//
//   rank_ranks     per user: its rank, or that it does not count / counts without a positive, by rank_finalize's rules
//   rank_counts    the users counted and the three fault counts -> out
//
// Integer atomics only and fixed-order fp64 sums: the results are bitwise reproducible.  The per-sample passes
// aggregate inside the wave first (Guideline 12): the lanes of the first user still pending are combined by
// ballot into one atomic per wave, up to kPeel users per wave (a wave of a contiguous layout holds one or two
// users); lanes left after that (interleaved users) fall back to one atomic each.
#include "metric_common.h"

using namespace dfm;

namespace {

constexpr int kRkThreads = 256;
constexpr int kRkMaxBlocks = 2048;
constexpr int kRkFinBlocks = 1024;
constexpr int kMaxKs = 8;
constexpr int kPeel = 2;
constexpr int kPartial = 1 + 2 * kMaxKs;     // users, hits[8], ndcg[8] (doubles)

struct RankHeader {                           // the first 64 bytes of the workspace
  unsigned long long bad_id, nan_score, bad_label;
  unsigned long long counted;                 // rank_ranks only: the users that count
  unsigned long long pad[4];
};

struct RankKs {
  int k[kMaxKs];
};

int sample_blocks(int64_t n) { return blocks_for(n, kRkThreads, kRkMaxBlocks); }
int user_blocks(int64_t users) { return blocks_for(users, kRkThreads, kRkFinBlocks); }

// workspace: header | best[U] u64 | cn[U] u64 (cnt | npos << 32) | ahead[U] u32 | partials[blocks][kPartial] f64
struct RankWs {
  RankHeader* hdr;
  unsigned long long* best;
  unsigned long long* cn;
  unsigned int* ahead;
  double* partial;
  size_t zero_bytes;                          // header .. ahead: cleared before every run
};

RankWs carve(void* ws, int64_t users) {
  Carver c{static_cast<char*>(ws)};
  const size_t nu = static_cast<size_t>(users);
  RankWs w;
  w.hdr = c.take<RankHeader>(1);
  w.best = c.take<unsigned long long>(nu);
  w.cn = c.take<unsigned long long>(nu);
  w.ahead = c.take<unsigned int>(nu);
  c.align16();
  w.zero_bytes = c.off;
  w.partial = c.take<double>(0);
  return w;
}

size_t ws_bytes(int64_t users) {
  return carve(nullptr, users).zero_bytes + sizeof(double) * kPartial * static_cast<size_t>(user_blocks(users));
}

__device__ __forceinline__ unsigned long long sample_key(float s, int64_t i) {
  return (static_cast<unsigned long long>(ord_bits(s)) << 32) | (0xFFFFFFFFu - static_cast<unsigned int>(i));
}

// Lanes walk the samples wave by wave (a wave's lanes hold consecutive samples, every lane runs every iteration,
// so ballots see the whole wave).
__global__ __launch_bounds__(kRkThreads) void rank_best_kernel(const int64_t* __restrict__ uids,
                                                               const float* __restrict__ labels,
                                                               const float* __restrict__ scores, int64_t n,
                                                               int64_t users, RankHeader* __restrict__ hdr,
                                                               unsigned long long* __restrict__ best,
                                                               unsigned long long* __restrict__ cn) {
  const int lane = lane_id();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kRkThreads;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kRkThreads + (threadIdx.x & ~(kWave - 1)); base < n;
       base += stride) {
    const int64_t i = base + lane;
    const bool valid = i < n;
    const int64_t u = valid ? uids[i] : 0;
    const float y = valid ? labels[i] : 0.f;
    const float s = valid ? scores[i] : 0.f;
    const bool ok = valid && u >= 0 && u < users;
    bool pos, y_bad;
    label_class(y, pos, y_bad);
    count_faults(valid && !ok, valid && isnan(s), valid && y_bad, &hdr->bad_id, &hdr->nan_score, &hdr->bad_label);
    const unsigned long long key = (ok && pos) ? sample_key(s, i) : 0ull;
    bool todo = ok;
#pragma unroll
    for (int r = 0; r < kPeel; ++r) {
      const unsigned long long m = __ballot(todo);
      if (!m) break;
      const int lead = lane_of(m);
      const int64_t u0 = __shfl(u, lead, kWave);
      const bool mine = todo && u == u0;
      const unsigned long long mm = __ballot(mine);
      const unsigned long long mp = __ballot(mine && pos);
      unsigned long long kmax = 0;
      if (mp) kmax = wave_max(mine ? key : 0ull);
      if (lane == lead) {
        atomicAdd(&cn[u0], static_cast<unsigned long long>(__popcll(mm)) |
                               (static_cast<unsigned long long>(__popcll(mp)) << 32));
        if (mp) atomicMax(&best[u0], kmax);
      }
      todo = todo && !mine;
    }
    if (todo) {
      atomicAdd(&cn[u], 1ull | (static_cast<unsigned long long>(pos) << 32));
      if (pos) atomicMax(&best[u], key);
    }
  }
}

__global__ __launch_bounds__(kRkThreads) void rank_count_kernel(const int64_t* __restrict__ uids,
                                                                const float* __restrict__ scores, int64_t n,
                                                                int64_t users,
                                                                const unsigned long long* __restrict__ best,
                                                                unsigned int* __restrict__ ahead) {
  const int lane = lane_id();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kRkThreads;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kRkThreads + (threadIdx.x & ~(kWave - 1)); base < n;
       base += stride) {
    const int64_t i = base + lane;
    const bool valid = i < n;
    const int64_t u = valid ? uids[i] : -1;
    const bool ok = valid && u >= 0 && u < users;
    const unsigned long long b = ok ? best[u] : 0ull;
    // b == 0: the user has no positive (every real key is > 0: ord_bits(-inf) = 0x007FFFFF)
    bool todo = ok && b != 0 && sample_key(scores[i], i) > b;
#pragma unroll
    for (int r = 0; r < kPeel; ++r) {
      const unsigned long long m = __ballot(todo);
      if (!m) break;
      const int lead = lane_of(m);
      const int64_t u0 = __shfl(u, lead, kWave);
      const bool mine = todo && u == u0;
      const unsigned long long mm = __ballot(mine);
      if (lane == lead) atomicAdd(&ahead[u0], static_cast<unsigned int>(__popcll(mm)));
      todo = todo && !mine;
    }
    if (todo) atomicAdd(&ahead[u], 1u);
  }
}

// per workgroup: partial[blockIdx.x] = {users, hits[k] (as doubles, exact), ndcg sums[k]}
__global__ __launch_bounds__(kRkThreads) void rank_finalize_kernel(const unsigned long long* __restrict__ best,
                                                                   const unsigned long long* __restrict__ cn,
                                                                   const unsigned int* __restrict__ ahead,
                                                                   int64_t users, RankKs ks, int num_ks,
                                                                   int require_both, double* __restrict__ partial) {
  __shared__ double red[kPartial][kRkThreads];
  unsigned long long nu = 0;
  unsigned long long hits[kMaxKs] = {};
  double ndcg[kMaxKs] = {};
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kRkThreads;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kRkThreads + threadIdx.x; u < users; u += stride) {
    const unsigned long long c = cn[u];
    const unsigned int cnt = static_cast<unsigned int>(c), np = static_cast<unsigned int>(c >> 32);
    const bool keep = require_both ? (np > 0 && np < cnt) : cnt > 0;
    if (!keep) continue;
    ++nu;
    if (np == 0 || best[u] == 0) continue;    // no positive: a miss at every k
    const unsigned int rank = ahead[u];
    const double gain = 1.0 / log2(static_cast<double>(rank) + 2.0);
#pragma unroll
    for (int j = 0; j < kMaxKs; ++j) {
      if (j < num_ks && static_cast<long long>(rank) < ks.k[j]) {
        ++hits[j];
        ndcg[j] += gain;
      }
    }
  }
  double v[kPartial];
  v[0] = static_cast<double>(nu);
#pragma unroll
  for (int j = 0; j < kMaxKs; ++j) {
    v[1 + j] = static_cast<double>(hits[j]);  // integers below 2^53: exact in fp64
    v[1 + kMaxKs + j] = ndcg[j];
  }
  block_sums(v, red);                         // everything is loaded before its first barrier
  if (threadIdx.x == 0) {
    double* dst = partial + static_cast<size_t>(blockIdx.x) * kPartial;
#pragma unroll
    for (int q = 0; q < kPartial; ++q) dst[q] = v[q];
  }
}

// out: [users, HR@k (num_ks), NDCG@k (num_ks), bad ids, NaN scores, non-binary labels]
__global__ __launch_bounds__(kRkThreads) void rank_reduce_kernel(const double* __restrict__ partial, int blocks,
                                                                 int num_ks, const RankHeader* __restrict__ hdr,
                                                                 double* __restrict__ out) {
  __shared__ double red[kPartial][kRkThreads];
  double v[kPartial] = {};
  for (int b = threadIdx.x; b < blocks; b += kRkThreads) {
#pragma unroll
    for (int q = 0; q < kPartial; ++q) v[q] += partial[static_cast<size_t>(b) * kPartial + q];
  }
  block_sums(v, red);
  if (threadIdx.x == 0) {
    const double nu = v[0];
    for (int j = 0; j < num_ks; ++j) {
      out[1 + j] = nu > 0 ? v[1 + j] / nu : 0.0;
      out[1 + num_ks + j] = nu > 0 ? v[1 + kMaxKs + j] / nu : 0.0;
    }
    out[0] = nu;
    out[1 + 2 * num_ks] = static_cast<double>(hdr->bad_id);
    out[2 + 2 * num_ks] = static_cast<double>(hdr->nan_score);
    out[3 + 2 * num_ks] = static_cast<double>(hdr->bad_label);
  }
}

// rank[u]: the user's rank, DFM_RANK_NOT_COUNTED or DFM_RANK_MISS, by rank_finalize's rules; the users that count are
// added up per wave (every lane runs every iteration, so ballots see the whole wave)
__global__ __launch_bounds__(kRkThreads) void rank_ranks_kernel(const unsigned long long* __restrict__ best,
                                                                const unsigned long long* __restrict__ cn,
                                                                const unsigned int* __restrict__ ahead, int64_t users,
                                                                int require_both, int64_t* __restrict__ rank,
                                                                unsigned long long* __restrict__ counted) {
  const int lane = lane_id();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kRkThreads;
  unsigned long long nu = 0;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kRkThreads + (threadIdx.x & ~(kWave - 1)); base < users;
       base += stride) {
    const int64_t u = base + lane;
    const bool valid = u < users;
    const unsigned long long c = valid ? cn[u] : 0ull;
    const unsigned int cnt = static_cast<unsigned int>(c), np = static_cast<unsigned int>(c >> 32);
    const bool keep = valid && (require_both ? (np > 0 && np < cnt) : cnt > 0);
    nu += static_cast<unsigned long long>(__popcll(__ballot(keep)));
    if (valid) {
      int64_t r = DFM_RANK_NOT_COUNTED;
      if (keep) r = (np == 0 || best[u] == 0) ? DFM_RANK_MISS : static_cast<int64_t>(ahead[u]);
      rank[u] = r;
    }
  }
  if (lane == 0 && nu) atomicAdd(counted, nu);
}

// out: [users counted, bad ids, NaN scores, non-binary labels]
__global__ void rank_counts_kernel(const RankHeader* __restrict__ hdr, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    out[0] = static_cast<double>(hdr->counted);
    out[1] = static_cast<double>(hdr->bad_id);
    out[2] = static_cast<double>(hdr->nan_score);
    out[3] = static_cast<double>(hdr->bad_label);
  }
}

int rank_check_sizes(int64_t n, int64_t num_users) {
  DFM_REQUIRE(n >= 1 && n < (int64_t(1) << 32), "sample count %lld outside [1, 2^32)", (long long)n);
  DFM_REQUIRE(num_users >= 1 && num_users < (int64_t(1) << 40), "bad num_users %lld", (long long)num_users);
  return DFM_OK;
}

// the two per-sample passes of both entry points: the workspace cleared, then best / cn, then ahead
int rank_sample_passes(const int64_t* d_user_ids, const float* d_labels, const float* d_scores, int64_t n,
                       int64_t num_users, void* d_workspace, const RankWs& w, hipStream_t st) {
  DFM_HIP_TRY(hipMemsetAsync(d_workspace, 0, w.zero_bytes, st));
  const int sb = sample_blocks(n);
  hipLaunchKernelGGL(rank_best_kernel, dim3(sb), dim3(kRkThreads), 0, st, d_user_ids, d_labels, d_scores, n,
                     num_users, w.hdr, w.best, w.cn);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_count_kernel, dim3(sb), dim3(kRkThreads), 0, st, d_user_ids, d_scores, n, num_users,
                     w.best, w.ahead);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

}  // namespace

extern "C" size_t dfm_ranking_workspace_bytes(int64_t n, int64_t num_users) {
  if (n < 1 || num_users < 1) return 0;
  return ws_bytes(num_users);
}

extern "C" int dfm_ranking_metrics(const int64_t* d_user_ids, const float* d_labels, const float* d_scores, int64_t n,
                                   int64_t num_users, const int32_t* h_ks, int num_ks, int require_both_classes,
                                   void* d_workspace, double* d_out, dfm_stream_t stream) {
  DFM_REQUIRE(d_user_ids && d_labels && d_scores && h_ks && d_workspace && d_out, "null argument");
  if (int rc = rank_check_sizes(n, num_users)) return rc;
  DFM_REQUIRE(num_ks >= 1 && num_ks <= kMaxKs, "num_ks %d outside [1, %d]", num_ks, kMaxKs);
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  RankKs ks;
  for (int j = 0; j < kMaxKs; ++j) ks.k[j] = 0;
  for (int j = 0; j < num_ks; ++j) {
    DFM_REQUIRE(h_ks[j] >= 1, "k = %d: every k must be >= 1", h_ks[j]);
    ks.k[j] = h_ks[j];
  }
  const RankWs w = carve(d_workspace, num_users);
  const hipStream_t st = as_stream(stream);
  if (int rc = rank_sample_passes(d_user_ids, d_labels, d_scores, n, num_users, d_workspace, w, st)) return rc;
  const int ub = user_blocks(num_users);
  hipLaunchKernelGGL(rank_finalize_kernel, dim3(ub), dim3(kRkThreads), 0, st, w.best, w.cn, w.ahead, num_users, ks,
                     num_ks, require_both_classes ? 1 : 0, w.partial);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_reduce_kernel, dim3(1), dim3(kRkThreads), 0, st, w.partial, ub, num_ks, w.hdr, d_out);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_ranking_user_ranks(const int64_t* d_user_ids, const float* d_labels, const float* d_scores, int64_t n,
                                      int64_t num_users, int require_both_classes, void* d_workspace, int64_t* d_rank,
                                      double* d_out, dfm_stream_t stream) {
  DFM_REQUIRE(d_user_ids && d_labels && d_scores && d_workspace && d_rank && d_out, "null argument");
  if (int rc = rank_check_sizes(n, num_users)) return rc;
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const RankWs w = carve(d_workspace, num_users);
  const hipStream_t st = as_stream(stream);
  if (int rc = rank_sample_passes(d_user_ids, d_labels, d_scores, n, num_users, d_workspace, w, st)) return rc;
  hipLaunchKernelGGL(rank_ranks_kernel, dim3(user_blocks(num_users)), dim3(kRkThreads), 0, st, w.best, w.cn, w.ahead,
                     num_users, require_both_classes ? 1 : 0, d_rank, &w.hdr->counted);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(rank_counts_kernel, dim3(1), dim3(kWave), 0, st, w.hdr, d_out);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
