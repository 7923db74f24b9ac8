// Grouped AUC over a device score buffer: the Mann-Whitney AUC of every group (a user, or the id of any SPARSE field),
// averaged over the groups with both classes, weighted by the group's samples (gauc) or plainly (uauc).
//
//   P_g, N_g   the group's labels equal to 1 / 0; it qualifies when both are > 0
//   W_g, T_g   its (positive, negative) pairs with s_pos > s_neg / s_pos == s_neg (float32, -0 == +0: ord_bits)
//   auc_g      double(2 W_g + T_g) / double(2 P_g N_g)                   (unsigned 64-bit integers)
//   gauc       sum (P_g + N_g) auc_g / sum (P_g + N_g),   uauc = mean auc_g    over the qualifying groups
//
// Two entry points around one ascending sort of int64 keys (the pooled AUC's shape, predict.hip):
//
//   prepare    per sample: key = group << 33 | label << 32 | ord_bits(score); INT64_MAX for a sample with an id outside
//              [0, num_groups), a NaN score or a label other than 0 / 1 (counted in the header, one atomic per wave)
//   (sort)     each group's negatives in front of its positives, each class ascending by score; invalid samples last
//   finish     gauc_bounds   per sorted key: a lane that opens / closes a (group, label) run stores the run's bounds
//              gauc_pairs    per positive: two binary searches inside its group's negatives -> 2 W + T of that
//                            positive; summed over the lanes of one group by ballot + shuffle, one u64 atomic per run
//                            of a wave (sorted keys: a wave holds few groups)
//              gauc_groups   per group, in group-id order: auc_g (optionally stored), per-workgroup partial sums
//              gauc_reduce   one workgroup: partials in a fixed order -> out
//   unit_columns   (the columns of the bootstrap over users, bootstrap_units.hip) gauc_bounds and gauc_pairs as above, then
//              gauc_columns  per group: qual, q_g = llrint(auc_g 2^30), size_g and size_g q_g as integers
//
// Every search is bounded by the group's negatives, so the work is O(n log n) whatever the group sizes.  The
// per-group numerators are integers summed with integer atomics, and the fp64 sums run over the groups in a tree that
// is fixed (below): the results are bitwise independent of the order of the samples.
//
// The tree has 1024 * 256 leaves whatever num_groups is: leaf l adds the terms of the groups l, l + 2^18, l + 2 * 2^18,
// ... in that order (0 for a group that does not qualify); workgroup b folds its leaves 256 b .. 256 b + 255 by
// halving (x[t] += x[t + s], s = 128 .. 1: block_sums, metric_common.h); the reduce pass does the same over the 1024
// workgroups' sums (thread t adds those of the workgroups t, t + 256, t + 512, t + 768, then the halving).  Products
// and sums are separate roundings (no fma).  Absent groups add zeros, so the results do not depend on num_groups either.
#include "metric_common.h"

using namespace dfm;

namespace {

constexpr int kGaThreads = 256;
constexpr int kGaMaxBlocks = 2048;
constexpr int kGaGroupBlocks = 1024;          // always: the tree of the fp64 sums is the grid
constexpr int kGaPeel = 2;
constexpr int kGaPartial = 4;                 // qualifying groups, sum (P+N) auc, sum auc, sum (P+N) (doubles)

struct GaucHeader {                           // the first 64 bytes of the workspace
  unsigned long long bad_id, nan_score, bad_label;
  unsigned long long pad[5];
};

// a group's runs in the sorted keys: negatives [neg_lo, neg_hi), positives [pos_lo, pos_hi); all 0 when absent
struct GaucRuns {
  unsigned int neg_lo, neg_hi, pos_lo, pos_hi;
};

int ga_sample_blocks(int64_t n) { return blocks_for(n, kGaThreads, kGaMaxBlocks); }

// workspace: header | runs[G] (16 B) | num[G] u64 (2W + T) | partials[blocks][kGaPartial] f64
struct GaucWs {
  GaucHeader* hdr;
  GaucRuns* runs;
  unsigned long long* num;
  double* partial;
  size_t group_bytes;                         // runs .. num: cleared by every finish
};

GaucWs ga_carve(void* ws, int64_t groups) {
  Carver c{static_cast<char*>(ws)};
  GaucWs w;
  w.hdr = c.take<GaucHeader>(1);
  w.runs = c.take<GaucRuns>(static_cast<size_t>(groups));
  w.num = c.take<unsigned long long>(static_cast<size_t>(groups));
  w.group_bytes = c.off - sizeof(GaucHeader);
  w.partial = c.take<double>(0);
  return w;
}

size_t ga_ws_bytes(int64_t groups) {
  return sizeof(GaucHeader) + ga_carve(nullptr, groups).group_bytes +
         sizeof(double) * kGaPartial * static_cast<size_t>(kGaGroupBlocks);
}

// Lanes walk the samples wave by wave (every lane runs every iteration, so ballots see the whole wave).
__global__ __launch_bounds__(kGaThreads) void gauc_prepare_kernel(const int64_t* __restrict__ gids,
                                                                  const float* __restrict__ labels,
                                                                  const float* __restrict__ scores, int64_t n,
                                                                  int64_t groups, GaucHeader* __restrict__ hdr,
                                                                  int64_t* __restrict__ keys) {
  const int lane = lane_id();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kGaThreads;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kGaThreads + (threadIdx.x & ~(kWave - 1)); base < n;
       base += stride) {
    const int64_t i = base + lane;
    const bool valid = i < n;
    const int64_t g = valid ? gids[i] : 0;
    const float y = valid ? labels[i] : 0.f;
    const float s = valid ? scores[i] : 0.f;
    const bool id_bad = g < 0 || g >= groups;
    const bool s_bad = isnan(s);
    bool pos, y_bad;
    label_class(y, pos, y_bad);
    count_faults(valid && id_bad, valid && s_bad, valid && y_bad, &hdr->bad_id, &hdr->nan_score, &hdr->bad_label);
    if (valid) {
      // shifted as unsigned: a bad id may not fit, and its key is discarded
      const int64_t key = static_cast<int64_t>((static_cast<unsigned long long>(g) << 33) |
                                               (static_cast<unsigned long long>(pos) << 32) | ord_bits(s));
      keys[i] = (id_bad || s_bad || y_bad) ? kInvalidKey : key;
    }
  }
}

// run of a key: group << 1 | label, -1 for the invalid key
__device__ __forceinline__ int64_t ga_run(int64_t key) { return key == kInvalidKey ? -1 : key >> 32; }

__global__ __launch_bounds__(kGaThreads) void gauc_bounds_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                                 int64_t groups, GaucRuns* __restrict__ runs) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kGaThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kGaThreads + threadIdx.x; i < n; i += stride) {
    const int64_t r = ga_run(keys[i]);
    const int64_t g = r >> 1;
    if (g < 0 || g >= groups) continue;       // invalid, or not prepare's keys for this num_groups: never index
    const bool opens = i == 0 || ga_run(keys[i - 1]) != r;
    const bool closes = i == n - 1 || ga_run(keys[i + 1]) != r;
    unsigned int* dst = reinterpret_cast<unsigned int*>(runs) + 4 * g + 2 * (r & 1);
    if (opens) dst[0] = static_cast<unsigned int>(i);
    if (closes) dst[1] = static_cast<unsigned int>(i + 1);
  }
}

// first index in [lo, hi) whose key is >= want (hi when none)
__device__ __forceinline__ unsigned int ga_lower_bound(const int64_t* __restrict__ keys, unsigned int lo,
                                                       unsigned int hi, int64_t want) {
  while (lo < hi) {
    const unsigned int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kGaThreads) void gauc_pairs_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                                int64_t groups, const GaucRuns* __restrict__ runs,
                                                                unsigned long long* __restrict__ num) {
  const int lane = lane_id();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kGaThreads;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kGaThreads + (threadIdx.x & ~(kWave - 1)); base < n;
       base += stride) {
    const int64_t i = base + lane;
    const int64_t key = i < n ? keys[i] : kInvalidKey;
    const int64_t g = key >> 33;
    bool todo = key != kInvalidKey && ((key >> 32) & 1) && g >= 0 && g < groups;
    unsigned long long c = 0;
    if (todo) {
      const GaucRuns r = runs[g];
      // clamped: whatever the keys hold, no search leaves [0, n)
      const unsigned int hi = r.neg_hi < n ? r.neg_hi : static_cast<unsigned int>(n);
      const unsigned int lo = r.neg_lo < hi ? r.neg_lo : hi;
      const int64_t same = key & ~(int64_t(1) << 32);              // this score among the group's negatives
      const unsigned int ge = ga_lower_bound(keys, lo, hi, same);
      const unsigned int gt = ga_lower_bound(keys, ge, hi, same + 1);
      c = 2ull * (ge - lo) + (gt - ge);
      todo = c != 0;
    }
#pragma unroll
    for (int p = 0; p < kGaPeel; ++p) {
      const unsigned long long m = __ballot(todo);
      if (!m) break;
      const int lead = lane_of(m);
      const int64_t g0 = __shfl(g, lead, kWave);
      const bool mine = todo && g == g0;
      const unsigned long long sum = wave_sum(mine ? c : 0ull);
      if (lane == lead) atomicAdd(&num[g0], sum);
      todo = todo && !mine;
    }
    if (todo) atomicAdd(&num[g], c);
  }
}

// per workgroup: partial[blockIdx.x] = {qualifying groups, sum (P+N) auc_g, sum auc_g, sum (P+N)}
__global__ __launch_bounds__(kGaThreads) void gauc_groups_kernel(const GaucRuns* __restrict__ runs,
                                                                 const unsigned long long* __restrict__ num,
                                                                 int64_t groups, double* __restrict__ group_auc,
                                                                 double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double red[kGaPartial][kGaThreads];
  unsigned long long ng = 0, ns = 0;
  double wsum = 0.0, asum = 0.0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kGaThreads;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * kGaThreads + threadIdx.x; g < groups; g += stride) {
    const GaucRuns r = runs[g];
    const unsigned long long nn = r.neg_hi - r.neg_lo, np = r.pos_hi - r.pos_lo;
    const bool keep = nn > 0 && np > 0;
    double auc = quiet_nan();
    if (keep) {
      auc = static_cast<double>(num[g]) / static_cast<double>(2ull * np * nn);
      const double term = static_cast<double>(np + nn) * auc;
      ++ng;
      ns += np + nn;
      wsum = wsum + term;
      asum = asum + auc;
    }
    if (group_auc) group_auc[g] = auc;
  }
  // the two counts are integers below 2^53: exact in fp64
  double v[kGaPartial] = {static_cast<double>(ng), wsum, asum, static_cast<double>(ns)};
  block_sums(v, red);
  if (threadIdx.x == 0) {
    double* dst = partial + static_cast<size_t>(blockIdx.x) * kGaPartial;
#pragma unroll
    for (int q = 0; q < kGaPartial; ++q) dst[q] = v[q];
  }
}

// out: [qualifying groups, gauc, uauc, samples in qualifying groups, bad ids, NaN scores, labels other than 0 / 1]
__global__ __launch_bounds__(kGaThreads) void gauc_reduce_kernel(const double* __restrict__ partial, int blocks,
                                                                 const GaucHeader* __restrict__ hdr,
                                                                 double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red[kGaPartial][kGaThreads];
  double v[kGaPartial] = {};
  for (int b = threadIdx.x; b < blocks; b += kGaThreads) {
#pragma unroll
    for (int q = 0; q < kGaPartial; ++q) v[q] = v[q] + partial[static_cast<size_t>(b) * kGaPartial + q];
  }
  block_sums(v, red);
  if (threadIdx.x == 0) {
    const double nan = quiet_nan();
    out[0] = v[0];
    out[1] = v[0] > 0 ? v[1] / v[3] : nan;
    out[2] = v[0] > 0 ? v[2] / v[0] : nan;
    out[3] = v[3];
    out[4] = static_cast<double>(hdr->bad_id);
    out[5] = static_cast<double>(hdr->nan_score);
    out[6] = static_cast<double>(hdr->bad_label);
  }
}

// cols (4, groups): qual | qual q | qual size | qual size q, size = P + N, q = llrint(auc_g 2^30) of gauc_groups' auc_g
__global__ __launch_bounds__(kGaThreads) void gauc_columns_kernel(const GaucRuns* __restrict__ runs,
                                                                  const unsigned long long* __restrict__ num,
                                                                  int64_t groups,
                                                                  unsigned long long* __restrict__ cols) {
#pragma clang fp contract(off)
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kGaThreads;
  const size_t ng = static_cast<size_t>(groups);
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * kGaThreads + threadIdx.x; g < groups; g += stride) {
    const GaucRuns r = runs[g];
    const unsigned long long nn = r.neg_hi - r.neg_lo, np = r.pos_hi - r.pos_lo;
    const bool keep = nn > 0 && np > 0;
    unsigned long long q = 0, size = 0;
    if (keep) {
      const double auc = static_cast<double>(num[g]) / static_cast<double>(2ull * np * nn);
      q = static_cast<unsigned long long>(llrint(auc * 1073741824.0));        // auc in [0, 1]: q <= 2^30
      size = np + nn;
    }
    cols[g] = keep ? 1ull : 0ull;
    cols[ng + g] = q;
    cols[2 * ng + g] = size;
    cols[3 * ng + g] = size * q;
  }
}

int ga_check_sizes(int64_t n, int64_t num_groups) {
  DFM_REQUIRE(n >= 1 && n < (int64_t(1) << 31), "sample count %lld outside [1, 2^31)", (long long)n);
  DFM_REQUIRE(num_groups >= 1 && num_groups <= (int64_t(1) << 30), "num_groups %lld outside [1, 2^30]",
              (long long)num_groups);
  return DFM_OK;
}

// the per-group integers of both entry points behind the sort: runs and numerators cleared, then filled
int ga_group_integers(const int64_t* d_sorted_keys, int64_t n, int64_t num_groups, const GaucWs& w, hipStream_t st) {
  DFM_HIP_TRY(hipMemsetAsync(w.runs, 0, w.group_bytes, st));
  const int sb = ga_sample_blocks(n);
  hipLaunchKernelGGL(gauc_bounds_kernel, dim3(sb), dim3(kGaThreads), 0, st, d_sorted_keys, n, num_groups, w.runs);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(gauc_pairs_kernel, dim3(sb), dim3(kGaThreads), 0, st, d_sorted_keys, n, num_groups, w.runs,
                     w.num);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

}  // namespace

extern "C" size_t dfm_grouped_auc_workspace_bytes(int64_t n, int64_t num_groups) {
  if (n < 1 || num_groups < 1) return 0;
  return ga_ws_bytes(num_groups);
}

extern "C" int dfm_grouped_auc_prepare(const int64_t* d_group_ids, const float* d_labels, const float* d_scores,
                                       int64_t n, int64_t num_groups, int64_t* d_keys_out, void* d_workspace,
                                       dfm_stream_t stream) {
  DFM_REQUIRE(d_group_ids && d_labels && d_scores && d_keys_out && d_workspace, "null argument");
  if (int rc = ga_check_sizes(n, num_groups)) return rc;
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const GaucWs w = ga_carve(d_workspace, num_groups);
  const hipStream_t st = as_stream(stream);
  DFM_HIP_TRY(hipMemsetAsync(w.hdr, 0, sizeof(GaucHeader), st));
  hipLaunchKernelGGL(gauc_prepare_kernel, dim3(ga_sample_blocks(n)), dim3(kGaThreads), 0, st, d_group_ids, d_labels,
                     d_scores, n, num_groups, w.hdr, d_keys_out);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_grouped_auc_finish(const int64_t* d_sorted_keys, int64_t n, int64_t num_groups, void* d_workspace,
                                      double* d_group_auc, double* d_out, dfm_stream_t stream) {
  DFM_REQUIRE(d_sorted_keys && d_workspace && d_out, "null argument");
  if (int rc = ga_check_sizes(n, num_groups)) return rc;
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const GaucWs w = ga_carve(d_workspace, num_groups);
  const hipStream_t st = as_stream(stream);
  if (int rc = ga_group_integers(d_sorted_keys, n, num_groups, w, st)) return rc;
  const int gb = kGaGroupBlocks;
  hipLaunchKernelGGL(gauc_groups_kernel, dim3(gb), dim3(kGaThreads), 0, st, w.runs, w.num, num_groups, d_group_auc,
                     w.partial);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(gauc_reduce_kernel, dim3(1), dim3(kGaThreads), 0, st, w.partial, gb, w.hdr, d_out);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_grouped_auc_unit_columns(const int64_t* d_sorted_keys, int64_t n, int64_t num_groups,
                                            void* d_workspace, uint64_t* d_cols, dfm_stream_t stream) {
  DFM_REQUIRE(d_sorted_keys && d_workspace && d_cols, "null argument");
  if (int rc = ga_check_sizes(n, num_groups)) return rc;
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const GaucWs w = ga_carve(d_workspace, num_groups);
  const hipStream_t st = as_stream(stream);
  if (int rc = ga_group_integers(d_sorted_keys, n, num_groups, w, st)) return rc;
  hipLaunchKernelGGL(gauc_columns_kernel, dim3(blocks_for(num_groups, kGaThreads, kGaMaxBlocks)), dim3(kGaThreads), 0, st,
                     w.runs, w.num, num_groups, reinterpret_cast<unsigned long long*>(d_cols));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
