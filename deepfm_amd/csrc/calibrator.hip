// Score calibrators fitted on the device from (label, logit) buffers and applied per launch (include/deepfm_hip.h
// states every formula, the state block and the knot table).
//
//   Platt      count pass (N+, N-, faults: integer atomics) and init, then max_rounds pairs of
//              sums    256 threads walk chunks of 1024 samples (four per thread, 16-byte loads when both pointers reach
//                      16-byte alignment after the same number of samples); six fp64 sums per thread in a fixed order,
//                      a wave butterfly, four waves added in order, one partial vector per workgroup, no atomic;
//              update  one workgroup: the partials go to LDS, thread q adds column q in workgroup order, thread 0
//                      advances the damped Newton iteration in the state block.  Both return at once when the status
//                      says so.
//   isotonic   histogram: calibration.hip's pass (a private table per workgroup in LDS, 64-bit LDS adds, up to 16
//              copies of a small table picked by the lane, non-zero cells to the global table with integer atomics),
//              then pool-adjacent-violators in one workgroup: the non-empty bins compacted by ballot, the pooling on
//              one thread over LDS in 64-bit integers, the knots written by one thread each.
//   apply      four logits per thread with 16-byte loads and stores; the isotonic knots in LDS, a binary search per
//              element.  Its parameters are read from device memory, so a refit re-aims live graphs.
#include <cmath>

#include "metric_common.h"

// every float operation that the header states as its own rounding stays one (plain operators; the functions that
// matter repeat the pragma, which is what survives inlining)
#pragma STDC FP_CONTRACT OFF

using namespace dfm;

namespace {

typedef unsigned long long u64;
typedef long long i64;

// The fits walk their (label, logit) samples with walk_pairs (metric_common.h), without an id column.
// ---- Platt ----------------------------------------------------------------------------------------------------
constexpr int kPlThreads = 256;
constexpr int kPlChunk = kPlThreads * 4;
constexpr int kPlMaxBlocks = 512;             // two per CU; the update adds this many partials per sum, one by one
constexpr int kPlHeader = 8;                  // u64 cells in front of the partials: N+, N-, non-finite, bad labels
constexpr int kPlSums = 6;
constexpr int kPlStride = 8;                  // doubles per partial vector
constexpr int kPlMaxRounds = 1024;

enum { sA = 0, sB, sF, sF0, sG, sRounds, sStatus, sFlags, sPos, sNeg, sNonFinite, sBadLabel, sTa, sTb, sDa, sDb, sStep,
       sTpos, sTneg, sN, sGtol, sFitSlope };

__global__ __launch_bounds__(kPlThreads) void platt_count_kernel(const float* __restrict__ labels,
                                                                 const float* __restrict__ logits, int64_t n, int head,
                                                                 u64* __restrict__ hdr) {
  __shared__ u64 red[4][kPlThreads / kWave];
  u64 c[4] = {0, 0, 0, 0};
  walk_pairs<kPlThreads, false>(labels, logits, nullptr, n, head, [&](float y, float z, int64_t) {
    bool pos, y_bad;
    label_class(y, pos, y_bad);
    const bool z_bad = !(fabsf(z) <= 3.4028234663852886e38f);      // NaN, +inf, -inf
    c[2] += z_bad;
    c[3] += y_bad;
    if (z_bad || y_bad) return;
    c[0] += pos;
    c[1] += !pos;
  });
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u64 s = wave_sum(c[q]);
    if (lane_id() == 0) red[q][threadIdx.x / kWave] = s;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < kPlThreads / kWave; ++w) s += red[threadIdx.x][w];
    if (s) atomicAdd(hdr + threadIdx.x, s);
  }
}

__global__ void platt_init_kernel(const u64* __restrict__ hdr, int64_t n, int fit_slope, int smooth, double gtol,
                                  double* __restrict__ st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double np = static_cast<double>(hdr[0]), nn = static_cast<double>(hdr[1]);
  const bool faults = hdr[2] != 0 || hdr[3] != 0;
  const bool one_class = hdr[0] == 0 || hdr[1] == 0;
  for (int i = 0; i < DFM_PLATT_STATE_DOUBLES; ++i) st[i] = 0.0;
  st[sA] = 1.0;
  st[sStatus] = faults ? DFM_CAL_BAD_INPUT : (one_class && !smooth ? DFM_CAL_SINGLE_CLASS : DFM_CAL_RUNNING);
  st[sPos] = np;
  st[sNeg] = nn;
  st[sNonFinite] = static_cast<double>(hdr[2]);
  st[sBadLabel] = static_cast<double>(hdr[3]);
  st[sTa] = 1.0;
  st[sStep] = 1.0;
  st[sTpos] = smooth ? (np + 1.0) / (np + 2.0) : 1.0;
  st[sTneg] = smooth ? 1.0 / (nn + 2.0) : 0.0;
  st[sN] = static_cast<double>(n);
  st[sGtol] = gtol;
  st[sFitSlope] = fit_slope ? 1.0 : 0.0;
}

__global__ __launch_bounds__(kPlThreads) void platt_sums_kernel(const float* __restrict__ labels,
                                                                const float* __restrict__ logits, int64_t n, int head,
                                                                const double* __restrict__ st,
                                                                double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double red[kPlSums][kPlThreads / kWave];
  if (st[sStatus] != static_cast<double>(DFM_CAL_RUNNING)) return;
  const double a = st[sTa], b = st[sTb], t_pos = st[sTpos], t_neg = st[sTneg];
  double acc[kPlSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  walk_pairs<kPlThreads, false>(labels, logits, nullptr, n, head, [&](float y, float zf, int64_t) {
#pragma clang fp contract(off)
    const double z = static_cast<double>(zf);
    const double t = y == 1.f ? t_pos : t_neg;
    const double s = a * z + b;
    const double e = exp(-fabs(s));
    const double d = 1.0 + e;
    const double q = (s >= 0.0 ? 1.0 : e) / d;
    const double w = e / (d * d);
    const double r = q - t;
    acc[0] += (log1p(e) + fmax(s, 0.0)) - t * s;
    acc[1] += r * z;
    acc[2] += r;
    acc[3] += (w * z) * z;
    acc[4] += w * z;
    acc[5] += w;
  });
#pragma unroll
  for (int q = 0; q < kPlSums; ++q) {
    const double s = wave_sum(acc[q]);
    if (lane_id() == 0) red[q][threadIdx.x / kWave] = s;
  }
  __syncthreads();
  if (threadIdx.x < kPlStride) {              // the two cells behind the six sums are written as zeros
    double s = 0.0;
    if (threadIdx.x < kPlSums) {
      s = red[threadIdx.x][0];
#pragma unroll
      for (int w = 1; w < kPlThreads / kWave; ++w) s += red[threadIdx.x][w];
    }
    partial[static_cast<size_t>(blockIdx.x) * kPlStride + threadIdx.x] = s;
  }
}

// The partials travel to LDS with every thread's loads in flight together; the six sums are then added from there in
// workgroup order, one by one (a thread that adds 512 values straight from memory waits for 512 loads in turn, which
// made a round at 1 M samples take 85 us).
__global__ __launch_bounds__(kPlThreads) void platt_update_kernel(const double* __restrict__ partial, int blocks,
                                                                  double* __restrict__ st) {
#pragma clang fp contract(off)
  __shared__ double stage[kPlMaxBlocks * kPlStride];
  __shared__ double sums[kPlSums];
  if (st[sStatus] != static_cast<double>(DFM_CAL_RUNNING)) return;
  for (int c = threadIdx.x; c < blocks * kPlStride; c += kPlThreads) stage[c] = partial[c];
  __syncthreads();
  if (threadIdx.x < kPlSums) {
    const int q = threadIdx.x;
    double s = 0.0;
    int w = 0;
    for (; w + 8 <= blocks; w += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = stage[(w + u) * kPlStride + q];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; w < blocks; ++w) s += stage[w * kPlStride + q];
    sums[q] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n = st[sN], gtol = st[sGtol];
  const bool fit_slope = st[sFitSlope] != 0.0;
  const double F = sums[0] / n, ga = sums[1] / n, gb = sums[2] / n;
  const double haa = sums[3] / n, hab = sums[4] / n, hbb = sums[5] / n;
  const double gmax = fit_slope ? fmax(fabs(ga), fabs(gb)) : fabs(gb);
  const bool first = st[sRounds] == 0.0;
  st[sRounds] += 1.0;
  if (first) st[sF0] = F;
  const double F_acc = st[sF];
  // within the rounding of the sum, the smaller gradient decides (see the header)
  const bool tie = fabs(F - F_acc) <= 64.0 * 1.1102230246251565e-16 * fabs(F_acc) && gmax < st[sG];
  if (first || F <= F_acc || tie) {
    st[sA] = st[sTa];
    st[sB] = st[sTb];
    st[sF] = F;
    st[sG] = gmax;
    if (gmax <= gtol) {
      st[sStatus] = static_cast<double>(DFM_CAL_CONVERGED);
      return;
    }
    double da = 0.0, db = 0.0;
    const double det = haa * hbb - hab * hab;
    if (fit_slope && haa > 0.0 && hbb > 0.0 && det > 1e-12 * (haa * hbb)) {
      da = -(hbb * ga - hab * gb) / det;
      db = -(haa * gb - hab * ga) / det;
    } else {
      if (fit_slope) st[sFlags] = static_cast<double>(DFM_CAL_FLAG_SLOPE_UNIDENTIFIED);
      db = hbb > 0.0 ? -gb / hbb : 0.0;
    }
    st[sDa] = da;
    st[sDb] = db;
    st[sStep] = 1.0;
  } else {
    st[sStep] = 0.5 * st[sStep];
  }
  st[sTa] = st[sA] + st[sStep] * st[sDa];
  st[sTb] = st[sB] + st[sStep] * st[sDb];
}

// ---- isotonic ---------------------------------------------------------------------------------------------------
constexpr int kIsoThreads = 1024;
constexpr int kIsoChunk = kIsoThreads * 4;
constexpr int kIsoMaxBlocks = 512;
constexpr int kIsoHeader = 8;                 // i64 cells in front of the bin table
constexpr size_t kIsoCopyLds = 12 * 1024;     // the further copies of a small bin table, on top of the first
constexpr int kIsoMaxCopies = 16;
constexpr int kMaxBins = DFM_ISOTONIC_MAX_BINS;

int iso_copies(int num_bins) {
  int r = kIsoMaxCopies;
  while (r > 1 && 24 * static_cast<size_t>(num_bins) * (r - 1) > kIsoCopyLds) r >>= 1;
  return r;
}

// ws: header[kIsoHeader] | bins[K][3], all 64-bit, zero on entry
__global__ __launch_bounds__(kIsoThreads) void iso_hist_kernel(const float* __restrict__ labels,
                                                               const float* __restrict__ logits, int64_t n, int head,
                                                               int num_bins, float z_lo, float z_hi, float scale,
                                                               int copies, u64* __restrict__ ws) {
  extern __shared__ u64 iso_lds[];            // bins[K][copies][3]
  __shared__ u64 red[4][kIsoThreads / kWave];
  const int cells = 3 * num_bins * copies;
  for (int c = threadIdx.x; c < cells; c += kIsoThreads) iso_lds[c] = 0;
  __syncthreads();
  const int copy = threadIdx.x & (copies - 1);
  u64 acc[4] = {0, 0, 0, 0};                  // used, positives, non-finite logits, bad labels
  walk_pairs<kIsoThreads, false>(labels, logits, nullptr, n, head, [&](float y, float z, int64_t) {
#pragma clang fp contract(off)
    bool pos, y_bad;
    label_class(y, pos, y_bad);
    const bool z_bad = !(fabsf(z) <= 3.4028234663852886e38f);
    acc[2] += z_bad;
    acc[3] += y_bad;
    if (z_bad || y_bad) return;
    acc[0] += 1;
    acc[1] += pos;
    const float zc = fminf(fmaxf(z, z_lo), z_hi);
    const float off = zc - z_lo;
    int bin = static_cast<int>(off * scale);
    bin = bin < num_bins - 1 ? bin : num_bins - 1;
    bin = bin > 0 ? bin : 0;
    const u64 zfix = static_cast<u64>(llrint(static_cast<double>(zc) * 16777216.0));
    u64* b = iso_lds + 3 * (static_cast<size_t>(bin) * copies + copy);
    atomicAdd(b, 1ull);
    if (pos) atomicAdd(b + 1, 1ull);
    atomicAdd(b + 2, zfix);
  });
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u64 s = wave_sum(acc[q]);
    if (lane_id() == 0) red[q][threadIdx.x / kWave] = s;
  }
  __syncthreads();                            // also: every LDS add of the workgroup has landed
  if (threadIdx.x < 4) {
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < kIsoThreads / kWave; ++w) s += red[threadIdx.x][w];
    if (s) atomicAdd(ws + threadIdx.x, s);
  }
  u64* g_bins = ws + kIsoHeader;
  for (int c = threadIdx.x; c < 3 * num_bins; c += kIsoThreads) {
    const u64* src = iso_lds + 3 * static_cast<size_t>(c / 3) * copies + c % 3;
    u64 s = 0;
    for (int r = 0; r < copies; ++r) s += src[3 * r];
    if (s) atomicAdd(g_bins + c, s);
  }
}

struct KnotTable {                            // DFM_ISOTONIC_KNOT_BYTES
  i64 hdr[8];
  float x32[kMaxBins];
  float v32[kMaxBins];
  double x[kMaxBins];
  double v[kMaxBins];
};
static_assert(sizeof(KnotTable) == DFM_ISOTONIC_KNOT_BYTES, "knot table layout");

__global__ __launch_bounds__(kMaxBins) void iso_pav_kernel(const i64* __restrict__ ws, int num_bins,
                                                           KnotTable* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ i64 k_pos[kMaxBins], k_cnt[kMaxBins];      // the non-empty bins, compacted
  __shared__ i64 b_pos[kMaxBins], b_cnt[kMaxBins];      // the stack of blocks
  __shared__ int k_bin[kMaxBins], b_start[kMaxBins], k_block[kMaxBins];
  __shared__ int wave_count[kMaxBins / kWave];
  __shared__ int s_blocks;
  const int t = threadIdx.x, wave = t / kWave, lane = t & (kWave - 1);
  const i64* bins = ws + kIsoHeader;
  const i64 cnt = t < num_bins ? bins[3 * t] : 0;
  const i64 pos = t < num_bins ? bins[3 * t + 1] : 0;
  const u64 mask = __ballot(cnt > 0);
  if (lane == 0) wave_count[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, m = 0;
  for (int w = 0; w < kMaxBins / kWave; ++w) {
    if (w < wave) before += wave_count[w];
    m += wave_count[w];
  }
  if (cnt > 0) {
    const int j = before + __popcll(mask & ((1ull << lane) - 1ull));
    k_bin[j] = t;
    k_pos[j] = pos;
    k_cnt[j] = cnt;
  }
  __syncthreads();
  if (t == 0) {
    int top = 0;
    for (int j = 0; j < m; ++j) {
      i64 bp = k_pos[j], bc = k_cnt[j];
      int bs = j;
      while (top > 0 && b_pos[top - 1] * bc > bp * b_cnt[top - 1]) {     // a strict decrease: pool
        --top;
        bp += b_pos[top];
        bc += b_cnt[top];
        bs = b_start[top];
      }
      b_pos[top] = bp;
      b_cnt[top] = bc;
      b_start[top] = bs;
      ++top;
    }
    s_blocks = top;
  }
  __syncthreads();
  const int blocks = s_blocks;
  if (t < blocks) {
    const int end = t + 1 < blocks ? b_start[t + 1] : m;
    for (int j = b_start[t]; j < end; ++j) k_block[j] = t;
  }
  __syncthreads();
  double x = 0.0, v = 0.0;
  if (t < m) {
    const int k = k_block[t];
    v = static_cast<double>(b_pos[k]) / static_cast<double>(b_cnt[k]);
    x = (static_cast<double>(bins[3 * k_bin[t] + 2]) * (1.0 / 16777216.0)) / static_cast<double>(k_cnt[t]);
  }
  out->x[t] = x;
  out->v[t] = v;
  out->x32[t] = static_cast<float>(x);
  out->v32[t] = static_cast<float>(v);
  if (t == 0) {
    out->hdr[0] = m;
    out->hdr[1] = num_bins;
    out->hdr[2] = ws[2];
    out->hdr[3] = ws[3];
    out->hdr[4] = ws[0];
    out->hdr[5] = ws[1];
    out->hdr[6] = blocks;
    out->hdr[7] = 0;
  }
}

// ---- apply ------------------------------------------------------------------------------------------------------
constexpr int kApThreads = 256;
constexpr int kApChunk = kApThreads * 4;
constexpr int kApMaxBlocks = 1024;

struct PlattMap {
  float a, b;
  __device__ __forceinline__ void load(const void* params) {
    const double* st = static_cast<const double*>(params);
    a = static_cast<float>(st[sA]);
    b = static_cast<float>(st[sB]);
  }
  __device__ __forceinline__ float operator()(float z) const {
#pragma clang fp contract(off)
    const float az = a * z;                   // plain operators under the pragma: the header's __fmul_rn / __fadd_rn
    const float s = az + b;                   // are compiled where contraction is allowed and would fuse into an fma
    return 1.f / (1.f + expf(-s));
  }
};

struct IsotonicMap {
  const float* x;
  const float* v;
  int m;
  __device__ __forceinline__ void load(const void* params) {
    __shared__ float knots[2 * kMaxBins];
    const KnotTable* tab = static_cast<const KnotTable*>(params);
    const i64 mm = tab->hdr[0];
    m = mm < 0 ? 0 : (mm > kMaxBins ? kMaxBins : static_cast<int>(mm));
    for (int j = threadIdx.x; j < m; j += kApThreads) {
      knots[j] = tab->x32[j];
      knots[kMaxBins + j] = tab->v32[j];
    }
    __syncthreads();
    x = knots;
    v = knots + kMaxBins;
  }
  __device__ __forceinline__ float operator()(float z) const {
#pragma clang fp contract(off)
    if (isnan(z)) return z;
    if (m == 0) return 1.f / (1.f + expf(-z));
    if (z <= x[0]) return v[0];
    if (z >= x[m - 1]) return v[m - 1];
    int lo = 0, hi = m - 1;                   // x[lo] <= z < x[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (x[mid] <= z) lo = mid; else hi = mid;
    }
    const float t = (z - x[lo]) / (x[hi] - x[lo]);
    const float rise = t * (v[hi] - v[lo]);
    return fminf(v[lo] + rise, v[hi]);
  }
};

template <typename Map>
__global__ __launch_bounds__(kApThreads) void cal_apply_kernel(const void* __restrict__ params,
                                                               const float* __restrict__ logits, int64_t n, int head,
                                                               float* __restrict__ probs) {
  Map map;
  map.load(params);
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kApThreads + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kApThreads;
  const int64_t nv = head < 0 ? 0 : (n - head) / 4;
  const int64_t h = head < 0 ? 0 : head;
  for (int64_t k = first; k < nv; k += stride) {
    const int64_t i = h + 4 * k;
    const float4 z4 = ld4(logits + i);
    st4(probs + i, make_float4(map(z4.x), map(z4.y), map(z4.z), map(z4.w)));
  }
  const int64_t rest = n - 4 * nv;
  for (int64_t r = first; r < rest; r += stride) {
    const int64_t i = r < h ? r : r + 4 * nv;
    probs[i] = map(logits[i]);
  }
}

bool sample_count_ok(int64_t n) { return n >= 1 && n < (int64_t(1) << 31); }

int fit_args(const float* d_labels, const float* d_logits, int64_t n, const void* d_workspace) {
  DFM_REQUIRE(d_labels && d_logits && d_workspace, "null argument");
  DFM_REQUIRE(sample_count_ok(n), "sample count %lld outside [1, 2^31)", (long long)n);
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_labels) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_logits) & 3) == 0,
              "labels and logits must be 4-byte aligned");
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  return DFM_OK;
}

}  // namespace

extern "C" size_t dfm_platt_workspace_bytes(int64_t n) {
  if (!sample_count_ok(n)) return 0;
  return 8 * (kPlHeader + static_cast<size_t>(kPlStride) * blocks_for(n, kPlChunk, kPlMaxBlocks));
}

extern "C" int dfm_platt_fit(const float* d_labels, const float* d_logits, int64_t n, int fit_slope, int smooth,
                             int max_rounds, double gtol, void* d_workspace, double* d_state, dfm_stream_t stream) {
  if (int rc = fit_args(d_labels, d_logits, n, d_workspace)) return rc;
  DFM_REQUIRE(d_state && (reinterpret_cast<uintptr_t>(d_state) & 7) == 0, "the state block must be 8-byte aligned");
  DFM_REQUIRE(max_rounds >= 1 && max_rounds <= kPlMaxRounds, "max_rounds %d outside [1, %d]", max_rounds,
              kPlMaxRounds);
  DFM_REQUIRE(gtol >= 0.0, "gtol must be a number >= 0");
  const hipStream_t st = as_stream(stream);
  u64* hdr = static_cast<u64*>(d_workspace);
  double* partial = reinterpret_cast<double*>(hdr + kPlHeader);
  const int head = pair_head(d_labels, d_logits);
  const int blocks = blocks_for(n, kPlChunk, kPlMaxBlocks);
  DFM_HIP_TRY(hipMemsetAsync(hdr, 0, 8 * kPlHeader, st));
  hipLaunchKernelGGL(platt_count_kernel, dim3(blocks), dim3(kPlThreads), 0, st, d_labels, d_logits, n, head, hdr);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(platt_init_kernel, dim3(1), dim3(kWave), 0, st, hdr, n, fit_slope, smooth, gtol, d_state);
  DFM_LAUNCH_CHECK();
  for (int r = 0; r < max_rounds; ++r) {
    hipLaunchKernelGGL(platt_sums_kernel, dim3(blocks), dim3(kPlThreads), 0, st, d_labels, d_logits, n, head, d_state,
                       partial);
    DFM_LAUNCH_CHECK();
    hipLaunchKernelGGL(platt_update_kernel, dim3(1), dim3(kPlThreads), 0, st, partial, blocks, d_state);
    DFM_LAUNCH_CHECK();
  }
  return DFM_OK;
}

extern "C" size_t dfm_isotonic_workspace_bytes(int num_bins) {
  if (num_bins < 1 || num_bins > kMaxBins) return 0;
  return 8 * (kIsoHeader + 3 * static_cast<size_t>(num_bins));
}

extern "C" int dfm_isotonic_fit(const float* d_labels, const float* d_logits, int64_t n, int num_bins, float z_lo,
                                float z_hi, void* d_workspace, void* d_knots, dfm_stream_t stream) {
  if (int rc = fit_args(d_labels, d_logits, n, d_workspace)) return rc;
  DFM_REQUIRE(num_bins >= 1 && num_bins <= kMaxBins, "num_bins %d outside [1, %d]", num_bins, kMaxBins);
  DFM_REQUIRE(z_lo >= -64.f && z_hi <= 64.f && z_lo < z_hi, "the logit range must satisfy -64 <= z_lo < z_hi <= 64");
  DFM_REQUIRE(d_knots && (reinterpret_cast<uintptr_t>(d_knots) & 15) == 0, "the knot table must be 16-byte aligned");
  const hipStream_t st = as_stream(stream);
  u64* ws = static_cast<u64*>(d_workspace);
  DFM_HIP_TRY(hipMemsetAsync(ws, 0, dfm_isotonic_workspace_bytes(num_bins), st));
  const float scale = static_cast<float>(static_cast<double>(num_bins) /
                                         (static_cast<double>(z_hi) - static_cast<double>(z_lo)));
  const int copies = iso_copies(num_bins);
  const size_t lds = 24 * static_cast<size_t>(num_bins) * copies;
  hipLaunchKernelGGL(iso_hist_kernel, dim3(blocks_for(n, kIsoChunk, kIsoMaxBlocks)), dim3(kIsoThreads), lds, st,
                     d_labels, d_logits, n, pair_head(d_labels, d_logits), num_bins, z_lo, z_hi, scale, copies, ws);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(iso_pav_kernel, dim3(1), dim3(kMaxBins), 0, st, reinterpret_cast<const i64*>(ws), num_bins,
                     static_cast<KnotTable*>(d_knots));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_calibrate_apply(int kind, const void* d_params, const float* d_logits, int64_t n, float* d_probs,
                                   const dfm_launch* at) {
  DFM_CHECK_LAUNCH(at);
  DFM_REQUIRE(kind == DFM_CAL_PLATT || kind == DFM_CAL_ISOTONIC, "calibrator kind %d: 0 (Platt) or 1 (isotonic)", kind);
  DFM_REQUIRE(d_params && d_logits && d_probs, "null argument");
  DFM_REQUIRE(sample_count_ok(n), "sample count %lld outside [1, 2^31)", (long long)n);
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_params) & 15) == 0, "the parameters must be 16-byte aligned");
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_logits) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_probs) & 3) == 0,
              "logits and probabilities must be 4-byte aligned");
  int head = pair_head(d_logits, d_probs);
  void* params[5] = {&d_params, &d_logits, &n, &head, &d_probs};
  const void* func = kind == DFM_CAL_PLATT ? reinterpret_cast<const void*>(&cal_apply_kernel<PlattMap>)
                                           : reinterpret_cast<const void*>(&cal_apply_kernel<IsotonicMap>);
  return launch_at(at, func, dim3(blocks_for(n, kApChunk, kApMaxBlocks)), dim3(kApThreads), 0, params, false);
}
