// Poisson bootstrap of metrics that are means over units (users): HR@k, NDCG@k, gauc, uauc.  Each is a quotient of two
// sums of per-unit integers, so a replicate is a quotient of two weighted column sums (include/deepfm_hip.h has the
// contract):
//
//   sums[r][m] = sum over the units u of w(seed, r, u) * cols[m][u]          (wrapping unsigned 64-bit arithmetic)
//
// with w the weight of bootstrap.hip (bs_weight, metric_common.h): one seed resamples the users alike in both files.
//
//   bu_sums     workgroup = (chunk of kBuChunk consecutive units, block of kBuBlock replicates): every column of the
//               chunk is read once into registers (16-byte loads where the column is aligned), the hash is the only
//               per-replicate input; per replicate the columns' products are summed over the wave by shuffles and over
//               the waves through LDS, then one u64 atomic per (workgroup, replicate, column) into slab chunk % slabs
//   bu_finish   sums = the slabs added up
//
// The slabs (at most kBuSlabs copies of the sums, in the workspace) spread the atomics of the chunks over several
// addresses.  Every sum is an integer sum mod 2^64, so the results do not depend on the launch geometry, the number of
// slabs or the order of the atomics.  Three launches (the clear of the slabs is one) whatever num_units is.
//
// dfm_bootstrap_rank_columns turns the per-user ranks of dfm_ranking_user_ranks into the columns of HR@k / NDCG@k.
#include "metric_common.h"

using namespace dfm;

namespace {

using u64 = unsigned long long;

constexpr int kBuThreads = 256;
constexpr int kBuWaves = kBuThreads / kWave;
constexpr int kBuItems = 4;                                   // units per thread: two pairs, kBuChunk / 2 apart
constexpr int kBuChunk = DFM_BOOTSTRAP_UNITS_CHUNK;
constexpr int kBuBlock = DFM_BOOTSTRAP_REPLICATE_BLOCK;
constexpr int kBuMaxCols = DFM_BOOTSTRAP_UNITS_MAX_COLS;
constexpr int kBuSlabs = 16;
constexpr int kBuMaxBlocks = 2048;
constexpr int64_t kBuMaxUnits = int64_t(1) << 30;
constexpr int kBuMaxKs = 8;
static_assert(kBuChunk == kBuThreads * kBuItems, "a chunk is one workgroup's registers");

struct BuKs {
  int k[kBuMaxKs];
};

int64_t bu_chunks(int64_t units) { return (units + kBuChunk - 1) / kBuChunk; }
int bu_slabs(int64_t units) { return static_cast<int>(bu_chunks(units) < kBuSlabs ? bu_chunks(units) : kBuSlabs); }

bool bu_sizes_ok(int64_t units, int cols, int replicates) {
  return units >= 1 && units <= kBuMaxUnits && cols >= 1 && cols <= kBuMaxCols && replicates >= 1 &&
         replicates <= DFM_BOOTSTRAP_MAX_REPLICATES;
}

size_t bu_ws_bytes(int64_t units, int cols, int replicates) {
  return round16(sizeof(u64) * static_cast<size_t>(bu_slabs(units)) * static_cast<size_t>(replicates) *
                 static_cast<size_t>(cols));
}

// w * c mod 2^64 for w < 2^32: one 32 x 32 -> 64 multiply and one 32-bit multiply
__device__ __forceinline__ u64 bu_mul(uint32_t w, u64 c) {
  const u64 lo = static_cast<u64>(w) * static_cast<uint32_t>(c);
  return lo + (static_cast<u64>(w * static_cast<uint32_t>(c >> 32)) << 32);
}

// grid (chunks, replicate blocks); MC: the columns a thread has registers for (num_cols <= MC)
template <int MC>
__global__ __launch_bounds__(kBuThreads) void bu_sums_kernel(const u64* __restrict__ cols, int64_t units, int num_cols,
                                                             int replicates, u64 seed_base, int num_slabs,
                                                             u64* __restrict__ slabs) {
  __shared__ u64 part[kBuBlock][kBuWaves][MC];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int r0 = blockIdx.y * kBuBlock;
  // item 2 h + e of a thread is unit first + h * kBuChunk / 2 + e: every load instruction of the workgroup covers
  // kBuChunk / 2 consecutive units, 16 bytes per lane
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kBuChunk + 2 * static_cast<int64_t>(threadIdx.x);
  u64 c[MC][kBuItems];
#pragma unroll
  for (int q = 0; q < MC; ++q) {
#pragma unroll
    for (int j = 0; j < kBuItems; ++j) c[q][j] = 0;
    if (q < num_cols) {
      const u64* col = cols + static_cast<size_t>(q) * static_cast<size_t>(units);
      const bool aligned = (reinterpret_cast<uintptr_t>(col) & 15) == 0;      // `first` is even
#pragma unroll
      for (int h = 0; h < kBuItems / 2; ++h) {
        const int64_t i = first + h * (kBuChunk / 2);
        if (aligned && i + 1 < units) {
          const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(col + i);
          c[q][2 * h] = v.x;
          c[q][2 * h + 1] = v.y;
        } else {
          if (i < units) c[q][2 * h] = col[i];
          if (i + 1 < units) c[q][2 * h + 1] = col[i + 1];
        }
      }
    }
  }
  for (int k = 0; k < kBuBlock && r0 + k < replicates; ++k) {
    const u64 base = seed_base + (static_cast<u64>(r0 + k) << 40) + static_cast<u64>(first);
    uint32_t w[kBuItems];                     // a unit past the end has zero columns: its weight is not looked at
#pragma unroll
    for (int j = 0; j < kBuItems; ++j) w[j] = bs_weight(base + static_cast<u64>((j >> 1) * (kBuChunk / 2) + (j & 1)));
#pragma unroll
    for (int q = 0; q < MC; ++q) {
      if (q < num_cols) {
        u64 a = 0;
#pragma unroll
        for (int j = 0; j < kBuItems; ++j) a += bu_mul(w[j], c[q][j]);
        a = wave_sum(a);
        if (lane == 0) part[k][wave][q] = a;
      }
    }
  }
  __syncthreads();
  u64* slab = slabs + static_cast<size_t>(blockIdx.x % num_slabs) * static_cast<size_t>(replicates) *
                          static_cast<size_t>(num_cols);
  for (int t = threadIdx.x; t < kBuBlock * MC; t += kBuThreads) {
    const int k = t / MC, q = t % MC;
    if (r0 + k < replicates && q < num_cols) {
      u64 s = 0;
#pragma unroll
      for (int v = 0; v < kBuWaves; ++v) s += part[k][v][q];
      if (s) atomicAdd(slab + static_cast<size_t>(r0 + k) * num_cols + q, s);
    }
  }
}

__global__ __launch_bounds__(kBuThreads) void bu_finish_kernel(const u64* __restrict__ slabs, int num_slabs,
                                                               int64_t cells, u64* __restrict__ sums) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBuThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBuThreads + threadIdx.x; i < cells; i += stride) {
    u64 s = 0;
    for (int v = 0; v < num_slabs; ++v) s += slabs[static_cast<size_t>(v) * static_cast<size_t>(cells) + i];
    sums[i] = s;
  }
}

// cols (1 + 2 num_ks, users): counted | [rank < k_j] | rank < k_j ? gain[rank] : 0
__global__ __launch_bounds__(kBuThreads) void bu_rank_columns_kernel(const int64_t* __restrict__ rank, int64_t users,
                                                                     BuKs ks, int num_ks,
                                                                     const u64* __restrict__ gain, int64_t gain_len,
                                                                     u64* __restrict__ cols) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBuThreads;
  const size_t nu = static_cast<size_t>(users);
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kBuThreads + threadIdx.x; u < users; u += stride) {
    const int64_t r = rank[u];
    cols[u] = (r >= 0 || r == DFM_RANK_MISS) ? 1ull : 0ull;
    const u64 g = (r >= 0 && r < gain_len) ? gain[r] : 0ull;   // whatever the ranks hold, no read leaves the table
#pragma unroll
    for (int j = 0; j < kBuMaxKs; ++j) {
      if (j < num_ks) {
        const bool hit = r >= 0 && r < ks.k[j];
        cols[static_cast<size_t>(1 + j) * nu + u] = hit ? 1ull : 0ull;
        cols[static_cast<size_t>(1 + num_ks + j) * nu + u] = hit ? g : 0ull;
      }
    }
  }
}

template <int MC>
void bu_launch(dim3 grid, hipStream_t st, const u64* cols, int64_t units, int num_cols, int replicates, u64 seed_base,
               int num_slabs, u64* slabs) {
  hipLaunchKernelGGL(bu_sums_kernel<MC>, grid, dim3(kBuThreads), 0, st, cols, units, num_cols, replicates, seed_base,
                     num_slabs, slabs);
}

}  // namespace

extern "C" size_t dfm_bootstrap_units_workspace_bytes(int64_t num_units, int num_cols, int replicates) {
  if (!bu_sizes_ok(num_units, num_cols, replicates)) return 0;
  return bu_ws_bytes(num_units, num_cols, replicates);
}

extern "C" int dfm_bootstrap_units(const uint64_t* d_cols, int64_t num_units, int num_cols, int replicates,
                                   uint64_t seed, void* d_workspace, uint64_t* d_sums, dfm_stream_t stream) {
  DFM_REQUIRE(d_cols && d_workspace && d_sums, "null argument");
  DFM_REQUIRE(num_units >= 1 && num_units <= kBuMaxUnits, "num_units %lld outside [1, 2^30]", (long long)num_units);
  DFM_REQUIRE(num_cols >= 1 && num_cols <= kBuMaxCols, "num_cols %d outside [1, %d]", num_cols, kBuMaxCols);
  DFM_REQUIRE(replicates >= 1 && replicates <= DFM_BOOTSTRAP_MAX_REPLICATES, "replicates %d outside [1, %d]",
              replicates, DFM_BOOTSTRAP_MAX_REPLICATES);
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_cols) & 7) == 0, "columns must be 8-byte aligned");
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const hipStream_t st = as_stream(stream);
  const int num_slabs = bu_slabs(num_units);
  const int64_t cells = static_cast<int64_t>(replicates) * num_cols;
  u64* slabs = static_cast<u64*>(d_workspace);
  const u64* cols = reinterpret_cast<const u64*>(d_cols);
  DFM_HIP_TRY(hipMemsetAsync(slabs, 0, bu_ws_bytes(num_units, num_cols, replicates), st));
  const dim3 grid(static_cast<unsigned>(bu_chunks(num_units)),
                  static_cast<unsigned>((replicates + kBuBlock - 1) / kBuBlock));
  const u64 seed_base = bs_seed_base(seed);
  if (num_cols <= 4) bu_launch<4>(grid, st, cols, num_units, num_cols, replicates, seed_base, num_slabs, slabs);
  else if (num_cols <= 8) bu_launch<8>(grid, st, cols, num_units, num_cols, replicates, seed_base, num_slabs, slabs);
  else if (num_cols <= 16) bu_launch<16>(grid, st, cols, num_units, num_cols, replicates, seed_base, num_slabs, slabs);
  else bu_launch<kBuMaxCols>(grid, st, cols, num_units, num_cols, replicates, seed_base, num_slabs, slabs);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(bu_finish_kernel, dim3(blocks_for(cells, kBuThreads, kBuMaxBlocks)), dim3(kBuThreads), 0, st, slabs,
                     num_slabs, cells, reinterpret_cast<u64*>(d_sums));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_bootstrap_rank_columns(const int64_t* d_rank, int64_t num_users, const int32_t* h_ks, int num_ks,
                                          const uint64_t* d_gain, int64_t gain_len, uint64_t* d_cols,
                                          dfm_stream_t stream) {
  DFM_REQUIRE(d_rank && h_ks && d_gain && d_cols, "null argument");
  DFM_REQUIRE(num_users >= 1 && num_users <= kBuMaxUnits, "num_users %lld outside [1, 2^30]", (long long)num_users);
  DFM_REQUIRE(num_ks >= 1 && num_ks <= kBuMaxKs, "num_ks %d outside [1, %d]", num_ks, kBuMaxKs);
  BuKs ks;
  for (int j = 0; j < kBuMaxKs; ++j) ks.k[j] = 0;
  for (int j = 0; j < num_ks; ++j) {
    DFM_REQUIRE(h_ks[j] >= 1, "k = %d: every k must be >= 1", h_ks[j]);
    DFM_REQUIRE(h_ks[j] <= gain_len, "k = %d beyond the gain table (%lld entries)", h_ks[j], (long long)gain_len);
    ks.k[j] = h_ks[j];
  }
  hipLaunchKernelGGL(bu_rank_columns_kernel, dim3(blocks_for(num_users, kBuThreads, kBuMaxBlocks)), dim3(kBuThreads), 0,
                     as_stream(stream), d_rank, num_users, ks, num_ks, reinterpret_cast<const u64*>(d_gain), gain_len,
                     reinterpret_cast<u64*>(d_cols));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
