// Poisson bootstrap of the pooled AUC and log loss over a device score buffer: R replicates, each an integer
// re-weighting of the samples (or of whole units: users), exact in 64-bit integers (include/deepfm_hip.h has the
// contract).
//
//   weight     w(seed, r, unit) = #{k : mix32(seed * G + B + (r << 40) + unit) >= T[k]}, Poisson(1) truncated at 12
//   per r      P, N, S = sum of w over the positives / negatives / all used samples
//              U       = sum over (positive i, negative j) of w_i w_j (2 [s_i > s_j] + [s_i == s_j])
//              L       = sum of w_i * llrint(sample_logloss * 2^27)
//   auc_r = double(U) / double(2 P N),  logloss_r = double(L) * 2^-27 / double(S)
//
// The pair count is two prefix sums.  The caller sorts two key vectors, ord(score) << 27 | tiebit << 26 | position with
// tiebit the label (tied scores: negatives in front) and its complement (positives in front).  For one order let
// A = sum over the positives of w_i * (weight of the negatives in front of i); then U = A_negfirst + A_posfirst: a
// negative with a smaller score is in front in both orders (2), one with the same score in exactly one (1).
//
//   prepare      per sample: the three fault counts, the fixed-point log-loss term, both keys (INT64_MAX when unused)
//   (two sorts)
//   replicates   bs_gather   per sorted key of either order: unit | label << 40 | used << 41 (and the log-loss term in
//                            sorted order 0), so that the passes below read coalesced and never index by position
//                bs_totals   workgroup = (chunk of kBsChunk sorted samples, block of kBsBlock replicates, order): the
//                            chunk stays in registers, the hash is the only per-replicate input; writes the weight of
//                            the chunk's negatives per replicate
//                bs_scan     workgroup = (order, replicate): exclusive prefix of its row of chunk totals, in place
//                bs_pairs    the same grid as bs_totals: the prefix of the negatives' weights inside the chunk (thread,
//                            wave, workgroup) on top of the chunk's offset -> A; order 0 also sums P, N and L; one u64
//                            atomic per workgroup, replicate and quantity
//                bs_finish   per replicate: S, the two quotients; the fault counts
//
// No workgroup waits for another: the dependencies between chunks are the launch boundaries.  Every sum is an integer
// sum, so the results do not depend on the launch geometry, the order of the atomics or the order of the samples.
#include "metric_common.h"

using namespace dfm;

namespace {

using u64 = unsigned long long;

constexpr int kBsThreads = 256;
constexpr int kBsWaves = kBsThreads / kWave;
constexpr int kBsItems = 8;                                   // consecutive sorted samples per thread
constexpr int kBsChunk = DFM_BOOTSTRAP_CHUNK;
constexpr int kBsBlock = DFM_BOOTSTRAP_REPLICATE_BLOCK;
static_assert(kBsChunk == kBsThreads * kBsItems, "a chunk is one workgroup's registers");
static_assert(kBsBlock <= kBsThreads, "one thread per replicate of a block writes its sums");
constexpr int kBsMaxBlocks = 2048;
constexpr int64_t kBsMaxN = int64_t(1) << DFM_BOOTSTRAP_MAX_LOG2_N;
constexpr int kBsPosBits = DFM_BOOTSTRAP_MAX_LOG2_N;          // key = ord << 27 | tiebit << 26 | position
constexpr u64 kBsPosMask = (u64(1) << kBsPosBits) - 1;
constexpr int64_t kBsUnitLimit = int64_t(1) << 40;
constexpr u64 kBsLabelBit = u64(1) << 40, kBsUsedBit = u64(1) << 41, kBsUnitMask = kBsLabelBit - 1;

struct BsHeader {                                             // the first 64 bytes of the workspace
  u64 nan_score, bad_label, bad_unit;
  u64 pad[5];
};

int64_t bs_chunks(int64_t n) { return (n + kBsChunk - 1) / kBsChunk; }

// workspace: header | lterm[n] u32 (by position) | packed[2][n] u64 | lsorted[n] u32 | totals[2][R][chunks] u32
struct BsWs {
  BsHeader* hdr;
  uint32_t* lterm;
  u64* packed;
  uint32_t* lsorted;
  uint32_t* totals;
  size_t bytes;
};

BsWs bs_carve(void* ws, int64_t n, int replicates) {
  Carver c{static_cast<char*>(ws)};
  const size_t sn = static_cast<size_t>(n);
  BsWs w;
  w.hdr = c.take<BsHeader>(1);                                // every array starts 16-byte aligned
  w.lterm = c.take<uint32_t>(sn); c.align16();
  w.packed = c.take<u64>(2 * sn); c.align16();
  w.lsorted = c.take<uint32_t>(sn); c.align16();
  w.totals = c.take<uint32_t>(2 * static_cast<size_t>(replicates) * static_cast<size_t>(bs_chunks(n))); c.align16();
  w.bytes = c.off;
  return w;
}

int bs_sample_blocks(int64_t n) { return blocks_for(n, kBsThreads, kBsMaxBlocks); }

__device__ __forceinline__ uint32_t bs_wave_inclusive(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}

// Lanes walk the samples wave by wave (every lane runs every iteration, so ballots see the whole wave).
__global__ __launch_bounds__(kBsThreads) void bs_prepare_kernel(const float* __restrict__ labels,
                                                                const float* __restrict__ scores,
                                                                const int64_t* __restrict__ units, int64_t n,
                                                                BsHeader* __restrict__ hdr,
                                                                uint32_t* __restrict__ lterm,
                                                                int64_t* __restrict__ keys_neg_first,
                                                                int64_t* __restrict__ keys_pos_first) {
  const int lane = lane_id();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBsThreads;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBsThreads + (threadIdx.x & ~(kWave - 1)); base < n;
       base += stride) {
    const int64_t i = base + lane;
    const bool valid = i < n;
    const float y = valid ? labels[i] : 0.f;
    const float s = valid ? scores[i] : 0.f;
    const int64_t u = (valid && units) ? units[i] : 0;
    const bool s_bad = isnan(s);
    bool pos, y_bad;
    label_class(y, pos, y_bad);
    const bool u_bad = u < 0 || u >= kBsUnitLimit;
    count_faults(valid && s_bad, valid && y_bad, valid && u_bad, &hdr->nan_score, &hdr->bad_label, &hdr->bad_unit);
    if (valid) {
      const bool used = !(s_bad || y_bad || u_bad);
      // at most -log(2^-23) * 2^27 < 2^32
      lterm[i] = used ? static_cast<uint32_t>(llrint(sample_logloss(s, pos) * 134217728.0)) : 0u;
      const u64 key = (static_cast<u64>(ord_bits(s)) << (kBsPosBits + 1)) | static_cast<u64>(i);
      keys_neg_first[i] = used ? static_cast<int64_t>(key | (static_cast<u64>(pos) << kBsPosBits)) : kInvalidKey;
      keys_pos_first[i] = used ? static_cast<int64_t>(key | (static_cast<u64>(!pos) << kBsPosBits)) : kInvalidKey;
    }
  }
}

// blockIdx.y: the order (0: tied negatives in front, 1: tied positives in front)
__global__ __launch_bounds__(kBsThreads) void bs_gather_kernel(const int64_t* __restrict__ sorted_neg_first,
                                                               const int64_t* __restrict__ sorted_pos_first,
                                                               const int64_t* __restrict__ units,
                                                               const uint32_t* __restrict__ lterm, int64_t n,
                                                               u64* __restrict__ packed,
                                                               uint32_t* __restrict__ lsorted) {
  const int order = blockIdx.y;
  const int64_t* keys = order ? sorted_pos_first : sorted_neg_first;
  u64* dst = packed + static_cast<size_t>(order) * static_cast<size_t>(n);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBsThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBsThreads + threadIdx.x; i < n; i += stride) {
    const int64_t key = keys[i];
    const int64_t p = static_cast<int64_t>(static_cast<u64>(key) & kBsPosMask);
    // whatever the keys hold, no read leaves [0, n)
    const bool used = key != kInvalidKey && key >= 0 && p < n;
    u64 v = 0;
    uint32_t lt = 0;
    if (used) {
      const u64 tie = (static_cast<u64>(key) >> kBsPosBits) & 1;
      const u64 unit = units ? static_cast<u64>(units[p]) : static_cast<u64>(p);
      v = (unit & kBsUnitMask) | ((order ? tie ^ 1 : tie) ? kBsLabelBit : 0) | kBsUsedBit;
      if (order == 0) lt = lterm[p];
    }
    dst[i] = v;
    if (order == 0) lsorted[i] = lt;
  }
}

// a workgroup's kBsItems consecutive sorted samples per thread; past n: unused
__device__ __forceinline__ void bs_load_chunk(const u64* __restrict__ packed, int64_t n, int64_t first,
                                              u64 (&item)[kBsItems]) {
#pragma unroll
  for (int j = 0; j < kBsItems; ++j) item[j] = first + j < n ? packed[first + j] : 0;
}

// grid (chunks, replicate blocks, 2 orders): totals[(order * R + r) * chunks + chunk] = weight of the chunk's negatives
__global__ __launch_bounds__(kBsThreads) void bs_totals_kernel(const u64* __restrict__ packed, int64_t n,
                                                               int replicates, int64_t chunks, u64 seed_base,
                                                               uint32_t* __restrict__ totals) {
  __shared__ uint32_t part[kBsBlock][kBsWaves];
  const int order = blockIdx.z, lane = lane_id(), wave = wave_id_uniform();
  const int r0 = blockIdx.y * kBsBlock;
  u64 item[kBsItems];
  bs_load_chunk(packed + static_cast<size_t>(order) * static_cast<size_t>(n), n,
                static_cast<int64_t>(blockIdx.x) * kBsChunk + static_cast<int64_t>(threadIdx.x) * kBsItems, item);
  for (int k = 0; k < kBsBlock && r0 + k < replicates; ++k) {
    const u64 base = seed_base + (static_cast<u64>(r0 + k) << 40);
    uint32_t neg = 0;
#pragma unroll
    for (int j = 0; j < kBsItems; ++j) {
      const bool counts = (item[j] & (kBsUsedBit | kBsLabelBit)) == kBsUsedBit;
      neg += counts ? bs_weight(base + (item[j] & kBsUnitMask)) : 0u;
    }
    neg = wave_sum(neg);
    if (lane == 0) part[k][wave] = neg;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < kBsBlock && r0 + k < replicates) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < kBsWaves; ++w) t += part[k][w];
    totals[(static_cast<size_t>(order) * replicates + (r0 + k)) * static_cast<size_t>(chunks) + blockIdx.x] = t;
  }
}

// one workgroup per row (order, replicate): exclusive prefix of the row's chunk totals, in place (below 2^32)
__global__ __launch_bounds__(kBsThreads) void bs_scan_kernel(uint32_t* __restrict__ totals, int64_t chunks) {
  __shared__ uint32_t wtot[2][kBsWaves];
  const int lane = lane_id(), wave = wave_id_uniform();
  uint32_t* row = totals + static_cast<size_t>(blockIdx.x) * static_cast<size_t>(chunks);
  uint32_t carry = 0;
  int flip = 0;
  for (int64_t c0 = 0; c0 < chunks; c0 += kBsThreads, flip ^= 1) {
    const int64_t c = c0 + threadIdx.x;
    const uint32_t v = c < chunks ? row[c] : 0u;
    const uint32_t incl = bs_wave_inclusive(v, lane);
    if (lane == kWave - 1) wtot[flip][wave] = incl;
    __syncthreads();                          // the other buffer is written next: one barrier per tile
    uint32_t before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < kBsWaves; ++w) {
      const uint32_t t = wtot[flip][w];
      if (w < wave) before += t;
      all += t;
    }
    if (c < chunks) row[c] = before + incl - v;
    carry += all;
  }
}

// counts[r][5] = {U, P, N, L, S}: U from both orders, P, N, L from order 0, S by bs_finish
__global__ __launch_bounds__(kBsThreads) void bs_pairs_kernel(const u64* __restrict__ packed,
                                                              const uint32_t* __restrict__ lsorted, int64_t n,
                                                              int replicates, int64_t chunks, u64 seed_base,
                                                              const uint32_t* __restrict__ offsets,
                                                              u64* __restrict__ counts) {
  __shared__ uint32_t wtot[2][kBsWaves];
  __shared__ u64 part_u[kBsBlock][kBsWaves], part_l[kBsBlock][kBsWaves];
  __shared__ uint32_t part_p[kBsBlock][kBsWaves], part_n[kBsBlock][kBsWaves];
  const int order = blockIdx.z, lane = lane_id(), wave = wave_id_uniform();
  const int r0 = blockIdx.y * kBsBlock;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kBsChunk + static_cast<int64_t>(threadIdx.x) * kBsItems;
  u64 item[kBsItems];
  uint32_t lt[kBsItems];
  bs_load_chunk(packed + static_cast<size_t>(order) * static_cast<size_t>(n), n, first, item);
#pragma unroll
  for (int j = 0; j < kBsItems; ++j) lt[j] = (order == 0 && first + j < n) ? lsorted[first + j] : 0u;
  for (int k = 0; k < kBsBlock && r0 + k < replicates; ++k) {
    const int r = r0 + k;
    const u64 base = seed_base + (static_cast<u64>(r) << 40);
    // in sorted order: the negatives' weight so far, and the positives' weight times it
    uint32_t neg = 0, pos = 0;
    u64 a = 0, l = 0;
#pragma unroll
    for (int j = 0; j < kBsItems; ++j) {
      const bool used = item[j] & kBsUsedBit;
      const uint32_t w = used ? bs_weight(base + (item[j] & kBsUnitMask)) : 0u;
      if (item[j] & kBsLabelBit) {
        a += static_cast<u64>(w) * neg;
        pos += w;
      } else {
        neg += w;
      }
      l += static_cast<u64>(w) * lt[j];
    }
    const uint32_t incl = bs_wave_inclusive(neg, lane);
    if (lane == kWave - 1) wtot[k & 1][wave] = incl;
    __syncthreads();                          // the other buffer is written next: one barrier per replicate
    uint32_t before = offsets[(static_cast<size_t>(order) * replicates + r) * static_cast<size_t>(chunks) + blockIdx.x] +
                      incl - neg;
#pragma unroll
    for (int w = 0; w < kBsWaves; ++w)
      if (w < wave) before += wtot[k & 1][w];
    const u64 u = wave_sum(a + static_cast<u64>(pos) * before);
    if (lane == 0) part_u[k][wave] = u;
    if (order == 0) {
      // a wave's positives and negatives weigh at most 64 * 8 * 12 each: both in one word
      const uint32_t pn = wave_sum(pos | (neg << 16));
      l = wave_sum(l);
      if (lane == 0) {
        part_p[k][wave] = pn & 0xFFFFu;
        part_n[k][wave] = pn >> 16;
        part_l[k][wave] = l;
      }
    }
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < kBsBlock && r0 + k < replicates) {
    u64 u = 0, l = 0, p = 0, m = 0;
#pragma unroll
    for (int w = 0; w < kBsWaves; ++w) {
      u += part_u[k][w];
      if (order == 0) {
        l += part_l[k][w];
        p += part_p[k][w];
        m += part_n[k][w];
      }
    }
    u64* dst = counts + 5 * static_cast<size_t>(r0 + k);
    if (u) atomicAdd(dst + 0, u);
    if (order == 0) {
      if (p) atomicAdd(dst + 1, p);
      if (m) atomicAdd(dst + 2, m);
      if (l) atomicAdd(dst + 3, l);
    }
  }
}

__global__ __launch_bounds__(kBsThreads) void bs_finish_kernel(u64* __restrict__ counts, int replicates,
                                                               const BsHeader* __restrict__ hdr,
                                                               double* __restrict__ out, u64* __restrict__ faults) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * kBsThreads + threadIdx.x;
  if (r == 0) {
    faults[0] = hdr->nan_score;
    faults[1] = hdr->bad_label;
    faults[2] = hdr->bad_unit;
  }
  if (r >= replicates) return;
  u64* c = counts + 5 * static_cast<size_t>(r);
  const u64 U = c[0], P = c[1], N = c[2], L = c[3], S = P + N;
  c[4] = S;
  const double nan = quiet_nan();
  out[2 * r + 0] = (P && N) ? static_cast<double>(U) / static_cast<double>(2ull * P * N) : nan;
  out[2 * r + 1] = S ? static_cast<double>(L) * (1.0 / 134217728.0) / static_cast<double>(S) : nan;
}

int bs_check_sizes(int64_t n) {
  DFM_REQUIRE(n >= 1 && n <= kBsMaxN, "sample count %lld outside [1, 2^%d]", (long long)n, DFM_BOOTSTRAP_MAX_LOG2_N);
  return DFM_OK;
}

}  // namespace

extern "C" size_t dfm_bootstrap_workspace_bytes(int64_t n, int replicates) {
  if (n < 1 || n > kBsMaxN || replicates < 1 || replicates > DFM_BOOTSTRAP_MAX_REPLICATES) return 0;
  return bs_carve(nullptr, n, replicates).bytes;
}

extern "C" int dfm_bootstrap_prepare(const float* d_labels, const float* d_scores, const int64_t* d_unit_ids, int64_t n,
                                     int64_t* d_keys_neg_first, int64_t* d_keys_pos_first, void* d_workspace,
                                     dfm_stream_t stream) {
  DFM_REQUIRE(d_labels && d_scores && d_keys_neg_first && d_keys_pos_first && d_workspace, "null argument");
  if (int rc = bs_check_sizes(n)) return rc;
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const BsWs w = bs_carve(d_workspace, n, 1);                 // the part in front does not depend on the replicates
  const hipStream_t st = as_stream(stream);
  DFM_HIP_TRY(hipMemsetAsync(w.hdr, 0, sizeof(BsHeader), st));
  hipLaunchKernelGGL(bs_prepare_kernel, dim3(bs_sample_blocks(n)), dim3(kBsThreads), 0, st, d_labels, d_scores,
                     d_unit_ids, n, w.hdr, w.lterm, d_keys_neg_first, d_keys_pos_first);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_bootstrap_replicates(const int64_t* d_sorted_neg_first, const int64_t* d_sorted_pos_first,
                                        const int64_t* d_unit_ids, int64_t n, int replicates, uint64_t seed,
                                        void* d_workspace, uint64_t* d_counts, double* d_out, uint64_t* d_faults,
                                        dfm_stream_t stream) {
  DFM_REQUIRE(d_sorted_neg_first && d_sorted_pos_first && d_workspace && d_counts && d_out && d_faults,
              "null argument");
  if (int rc = bs_check_sizes(n)) return rc;
  DFM_REQUIRE(replicates >= 1 && replicates <= DFM_BOOTSTRAP_MAX_REPLICATES, "replicates %d outside [1, %d]",
              replicates, DFM_BOOTSTRAP_MAX_REPLICATES);
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const BsWs w = bs_carve(d_workspace, n, replicates);
  const hipStream_t st = as_stream(stream);
  const int64_t chunks = bs_chunks(n);
  const int rblocks = (replicates + kBsBlock - 1) / kBsBlock;
  const u64 seed_base = bs_seed_base(seed);
  u64* counts = reinterpret_cast<u64*>(d_counts);
  DFM_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(u64) * 5 * static_cast<size_t>(replicates), st));
  hipLaunchKernelGGL(bs_gather_kernel, dim3(bs_sample_blocks(n), 2), dim3(kBsThreads), 0, st, d_sorted_neg_first,
                     d_sorted_pos_first, d_unit_ids, w.lterm, n, w.packed, w.lsorted);
  DFM_LAUNCH_CHECK();
  const dim3 grid(static_cast<unsigned>(chunks), static_cast<unsigned>(rblocks), 2);
  hipLaunchKernelGGL(bs_totals_kernel, grid, dim3(kBsThreads), 0, st, w.packed, n, replicates, chunks, seed_base,
                     w.totals);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(bs_scan_kernel, dim3(2u * static_cast<unsigned>(replicates)), dim3(kBsThreads), 0, st, w.totals,
                     chunks);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(bs_pairs_kernel, grid, dim3(kBsThreads), 0, st, w.packed, w.lsorted, n, replicates, chunks,
                     seed_base, w.totals, counts);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(bs_finish_kernel, dim3((replicates + kBsThreads - 1) / kBsThreads), dim3(kBsThreads), 0, st,
                     counts, replicates, w.hdr, d_out, reinterpret_cast<u64*>(d_faults));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
