// Calibration of a device score buffer: one streaming pass over n (label, probability[, slice id]) samples into 64-bit
// integer sums, then a finish that turns the integers into the fp64 reliability table, the per-slice table and
//   out[12] = {N, positives, mean prediction, Brier score, log loss, ECE, MCE,
//              bad slice ids, NaN scores, scores outside [0, 1], labels other than 0 / 1, 0}.
//
// A sample is used only when its slice id lies in [0, num_slices) (with slices), its score is a number in [0, 1]
// (-0 included) and its label is exactly 0 or 1; every other sample is counted in the counter of each of its faults
// and enters nothing else.  For a used sample with float32 score p and label y (K = num_bins):
//
//   bin = min(K - 1, (int)(p * (float)K))            float32 product; p == 1 lands in the last bin
//   P   = llrint((double)p * 2^32)
//   Q   = llrint(((double)p - y)^2 * 2^32)
//   L   = llrint(l * 2^27)                           l = sample_logloss(p, y == 1) (common.h: the pooled metric's term)
//
// and the sums are  N, positives, sum P, sum Q, sum L  globally;  count, positives, sum P  per bin;  count, positives,
// sum P, sum L  per slice.  With n < 2^31 none can overflow (l <= -log(FLT_EPSILON) < 16, so L < 2^31).  Every sum is
// an integer sum, so the results do not depend on the order of the samples or on the launch geometry, bit for bit.
//
//   finish     bins[b]   = {count, positives, sum P_b * 2^-32}
//              slices[s] = {count, positives, sum P_s * 2^-32, sum L_s * 2^-27}
//              gap_b = fabs(sum P_b * 2^-32 - positives_b);  ece = (gap_0 + gap_1 + ..., ascending, one by one) / N;
//              mce = max over the non-empty bins of gap_b / count_b;  the five ratios of out are NaN when N == 0
//
// The pass: a workgroup of 1024 threads walks chunks of 4096 samples (four per thread: 16-byte loads of the labels and
// the scores, two of the ids, when the three pointers reach 16-byte alignment after the same number of samples; the
// samples in front of and behind the aligned body, at most six, and the whole input otherwise, go one by one).  The
// global sums stay in registers until the workgroup's end (wave shuffles, LDS, one atomic per non-zero value; the four
// fault counts only when a wave has any).  The bin table, and on route 0 the slice table, are private to the workgroup
// in LDS (64-bit LDS adds); a small bin table is held in up to 16 copies picked by the lane, because a model's scores
// crowd into a few bins and the lanes of a wave that add to one LDS address take turns (256 threads adding their sums
// to one LDS cell each doubled the time of the pass at 1 M samples).  At its end the workgroup adds its non-zero cells
// to the global tables with 64-bit integer atomics.  On route 1 ((3 K + 4 S) * 8 bytes above kCalTableLds) the slice
// sums go to the global table with integer atomics per sample.  No float atomic anywhere.
#include "metric_common.h"

using namespace dfm;

namespace {

typedef unsigned long long u64;

constexpr int kCalThreads = 1024;
constexpr int kCalFinishThreads = 256;
constexpr int kCalPerThread = 4;
constexpr int kCalChunk = kCalThreads * kCalPerThread;
constexpr int kCalMaxBlocks = 512;            // two per CU
constexpr int kCalMaxBins = 1024;
constexpr int64_t kCalMaxSlices = int64_t(1) << 24;
constexpr size_t kCalTableLds = 48 * 1024;    // route 0: one copy of the bin table and the slice table fit in here
constexpr size_t kCalCopyLds = 12 * 1024;     // on top: the further copies of a small bin table
constexpr int kCalMaxCopies = 16;
constexpr int kCalHeader = 16;                // u64 cells in front of the tables (128 bytes)
constexpr int kCalFinishBlocks = 1024;

enum { kN = 0, kPos, kSumP, kSumQ, kSumL, kBadId, kNan, kRange, kBadLabel, kCalSums };

int cal_route(int num_bins, int64_t num_slices) {
  return (3 * static_cast<size_t>(num_bins) + 4 * static_cast<size_t>(num_slices)) * 8 <= kCalTableLds ? 0 : 1;
}

// copies of the bin table in LDS: the largest power of two up to 16 whose extra copies fit kCalCopyLds
int cal_copies(int num_bins) {
  int r = kCalMaxCopies;
  while (r > 1 && 24 * static_cast<size_t>(num_bins) * (r - 1) > kCalCopyLds) r >>= 1;
  return r;
}

bool cal_sizes_ok(int num_bins, int64_t num_slices) {
  return num_bins >= 1 && num_bins <= kCalMaxBins && num_slices >= 0 && num_slices <= kCalMaxSlices;
}

size_t cal_ws_cells(int num_bins, int64_t num_slices) {
  return kCalHeader + 3 * static_cast<size_t>(num_bins) + 4 * static_cast<size_t>(num_slices);
}

// Few, large workgroups: every workgroup ends with atomics on the same few dozen hot cells (the global sums, the
// filled bins), which the memory side takes one after another; at 1 M samples twice as many workgroups of a quarter
// of the size took 6 us longer.
int cal_blocks(int64_t n) { return blocks_for(n, kCalChunk, kCalMaxBlocks); }

// One sample into the thread's sums, the workgroup's bin table and the slice table (LDS on route 0, global on route 1).
template <bool kSlices>
__device__ __forceinline__ void cal_sample(float y, float p, int64_t sid, int num_bins, int64_t num_slices, int copy,
                                           int copies, u64* __restrict__ l_bins, u64* __restrict__ slice_table,
                                           u64 (&acc)[kCalSums]) {
#pragma clang fp contract(off)
  const bool id_bad = kSlices && (sid < 0 || sid >= num_slices);
  const bool s_nan = isnan(p);
  const bool s_range = !s_nan && !(p >= 0.f && p <= 1.f);
  bool pos, y_bad;
  label_class(y, pos, y_bad);
  acc[kBadId] += id_bad;
  acc[kNan] += s_nan;
  acc[kRange] += s_range;
  acc[kBadLabel] += y_bad;
  if (id_bad || s_nan || s_range || y_bad) return;
  const double pd = static_cast<double>(p);
  const double d = pd - (pos ? 1.0 : 0.0);
  const u64 P = static_cast<u64>(llrint(pd * 4294967296.0));
  const u64 Q = static_cast<u64>(llrint(d * d * 4294967296.0));
  const u64 L = static_cast<u64>(llrint(sample_logloss(p, pos) * 134217728.0));
  acc[kN] += 1;
  acc[kPos] += pos;
  acc[kSumP] += P;
  acc[kSumQ] += Q;
  acc[kSumL] += L;
  int bin = static_cast<int>(__fmul_rn(p, static_cast<float>(num_bins)));
  bin = bin < num_bins - 1 ? bin : num_bins - 1;
  u64* b = l_bins + 3 * (static_cast<size_t>(bin) * copies + copy);
  atomicAdd(b, 1ull);
  if (pos) atomicAdd(b + 1, 1ull);
  atomicAdd(b + 2, P);
  if (kSlices) {
    u64* s = slice_table + 4 * static_cast<size_t>(sid);      // LDS or global: atomicAdd takes either
    atomicAdd(s, 1ull);
    if (pos) atomicAdd(s + 1, 1ull);
    atomicAdd(s + 2, P);
    atomicAdd(s + 3, L);
  }
}

// ws: header[kCalHeader] | bins[K][3] | slices[S][4], all u64, zero on entry.  head: samples in front of the aligned
// body, or -1 when the pointers never line up (everything goes one by one).
template <bool kSlices, bool kSliceLds>
__global__ __launch_bounds__(kCalThreads) void calibration_kernel(const float* __restrict__ labels,
                                                                  const float* __restrict__ scores,
                                                                  const int64_t* __restrict__ ids, int64_t n, int head,
                                                                  int num_bins, int64_t num_slices, int copies,
                                                                  u64* __restrict__ ws) {
  extern __shared__ u64 cal_lds[];            // bins[K][copies][3] | slices[S][4] (route 0)
  __shared__ u64 red[kCalSums][kCalThreads / kWave];
  u64* l_bins = cal_lds;
  const int bin_cells = 3 * num_bins * copies;
  u64* l_slices = cal_lds + bin_cells;
  const int lds_cells = bin_cells + (kSlices && kSliceLds ? 4 * static_cast<int>(num_slices) : 0);
  for (int c = threadIdx.x; c < lds_cells; c += kCalThreads) cal_lds[c] = 0;
  __syncthreads();

  u64* g_bins = ws + kCalHeader;
  u64* g_slices = g_bins + 3 * static_cast<size_t>(num_bins);
  u64* slice_table = kSliceLds ? l_slices : g_slices;
  const int copy = threadIdx.x & (copies - 1);
  u64 acc[kCalSums] = {};
  static_assert(kCalPerThread == 4, "walk_pairs' aligned body: four consecutive samples per thread");
  walk_pairs<kCalThreads, kSlices>(labels, scores, ids, n, head, [&](float y, float p, int64_t sid) {
    cal_sample<kSlices>(y, p, sid, num_bins, num_slices, copy, copies, l_bins, slice_table, acc);
  });

  // the global sums: per wave, per workgroup, then one atomic per non-zero value
  const int wave = threadIdx.x / kWave;
  const bool faults = __ballot((acc[kBadId] | acc[kNan] | acc[kRange] | acc[kBadLabel]) != 0) != 0;
#pragma unroll
  for (int q = 0; q < kCalSums; ++q) {
    u64 s = 0;
    if (q < kBadId || faults) s = wave_sum(acc[q]);
    if (lane_id() == 0) red[q][wave] = s;
  }
  __syncthreads();                            // also: every LDS add of the workgroup has landed
  if (threadIdx.x < kCalSums) {
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < kCalThreads / kWave; ++w) s += red[threadIdx.x][w];
    if (s) atomicAdd(ws + threadIdx.x, s);
  }
  // the tables: the copies of a bin cell summed, non-zero cells only
  for (int c = threadIdx.x; c < 3 * num_bins; c += kCalThreads) {
    const u64* src = l_bins + 3 * static_cast<size_t>(c / 3) * copies + c % 3;
    u64 s = 0;
    for (int r = 0; r < copies; ++r) s += src[3 * r];
    if (s) atomicAdd(g_bins + c, s);
  }
  if (kSlices && kSliceLds) {
    for (int c = threadIdx.x; c < 4 * static_cast<int>(num_slices); c += kCalThreads) {
      const u64 s = l_slices[c];
      if (s) atomicAdd(g_slices + c, s);
    }
  }
}

__device__ __forceinline__ double cal_f64(u64 v) { return static_cast<double>(static_cast<long long>(v)); }

// Every workgroup converts its share of the slice table; workgroup 0 also writes the bin table and out.
__global__ __launch_bounds__(kCalFinishThreads) void calibration_finish_kernel(const u64* __restrict__ ws,
                                                                               int num_bins, int64_t num_slices,
                                                                               double* __restrict__ bins,
                                                                               double* __restrict__ slices,
                                                                               double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double gap[kCalMaxBins];
  __shared__ double ratio[kCalMaxBins];        // gap_b / count_b, -1 for an empty bin
  const double p_unit = 1.0 / 4294967296.0, l_unit = 1.0 / 134217728.0;
  const u64* g_bins = ws + kCalHeader;
  const u64* g_slices = g_bins + 3 * static_cast<size_t>(num_bins);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kCalFinishThreads;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kCalFinishThreads + threadIdx.x; s < num_slices; s += stride) {
    const u64* src = g_slices + 4 * s;
    double* dst = slices + 4 * s;
    dst[0] = cal_f64(src[0]);
    dst[1] = cal_f64(src[1]);
    dst[2] = cal_f64(src[2]) * p_unit;
    dst[3] = cal_f64(src[3]) * l_unit;
  }
  if (blockIdx.x != 0) return;
  for (int b = threadIdx.x; b < num_bins; b += kCalFinishThreads) {
    const double cnt = cal_f64(g_bins[3 * b]), pos = cal_f64(g_bins[3 * b + 1]);
    const double sum_p = cal_f64(g_bins[3 * b + 2]) * p_unit;
    bins[3 * b] = cnt;
    bins[3 * b + 1] = pos;
    bins[3 * b + 2] = sum_p;
    const double g = fabs(sum_p - pos);
    gap[b] = g;
    ratio[b] = cnt > 0 ? g / cnt : -1.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double nan = quiet_nan();
    double total = 0.0, worst = -1.0;
    for (int b = 0; b < num_bins; ++b) {
      total = total + gap[b];
      worst = ratio[b] > worst ? ratio[b] : worst;
    }
    const u64 N = ws[kN];
    const double dn = cal_f64(N);
    out[0] = dn;
    out[1] = cal_f64(ws[kPos]);
    out[2] = N ? cal_f64(ws[kSumP]) * p_unit / dn : nan;
    out[3] = N ? cal_f64(ws[kSumQ]) * p_unit / dn : nan;
    out[4] = N ? cal_f64(ws[kSumL]) * l_unit / dn : nan;
    out[5] = N ? total / dn : nan;
    out[6] = N ? worst : nan;
    out[7] = cal_f64(ws[kBadId]);
    out[8] = cal_f64(ws[kNan]);
    out[9] = cal_f64(ws[kRange]);
    out[10] = cal_f64(ws[kBadLabel]);
    out[11] = 0.0;
  }
}

// samples in front of the body at which labels, scores and (when given) ids are all 16-byte aligned; -1 when there is
// no such count below 4
int cal_head(const float* labels, const float* scores, const int64_t* ids) {
  for (int h = 0; h < kCalPerThread; ++h) {
    const bool ok = (reinterpret_cast<uintptr_t>(labels + h) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(scores + h) & 15) == 0 &&
                    (!ids || (reinterpret_cast<uintptr_t>(ids + h) & 15) == 0);
    if (ok) return h;
  }
  return -1;
}

template <bool kSlices, bool kSliceLds>
int cal_launch(const float* labels, const float* scores, const int64_t* ids, int64_t n, int head, int num_bins,
               int64_t num_slices, u64* ws, hipStream_t st) {
  const int copies = cal_copies(num_bins);
  const size_t lds =
      8 * (3 * static_cast<size_t>(num_bins) * copies + (kSliceLds ? 4 * static_cast<size_t>(num_slices) : 0));
  hipLaunchKernelGGL((calibration_kernel<kSlices, kSliceLds>), dim3(cal_blocks(n)), dim3(kCalThreads), lds, st, labels,
                     scores, ids, n, head, num_bins, num_slices, copies, ws);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

}  // namespace

extern "C" size_t dfm_calibration_workspace_bytes(int num_bins, int64_t num_slices) {
  if (!cal_sizes_ok(num_bins, num_slices)) return 0;
  return 8 * cal_ws_cells(num_bins, num_slices);
}

extern "C" int dfm_calibration_route(int num_bins, int64_t num_slices) {
  if (!cal_sizes_ok(num_bins, num_slices)) return -1;
  return cal_route(num_bins, num_slices);
}

extern "C" int dfm_calibration(const float* d_labels, const float* d_scores, const int64_t* d_slice_ids, int64_t n,
                               int num_bins, int64_t num_slices, void* d_workspace, double* d_bins, double* d_slices,
                               double* d_out, dfm_stream_t stream) {
  DFM_REQUIRE(d_labels && d_scores && d_workspace && d_bins && d_out, "null argument");
  DFM_REQUIRE(n >= 1 && n < (int64_t(1) << 31), "sample count %lld outside [1, 2^31)", (long long)n);
  DFM_REQUIRE(num_bins >= 1 && num_bins <= kCalMaxBins, "num_bins %d outside [1, %d]", num_bins, kCalMaxBins);
  DFM_REQUIRE(num_slices >= 0 && num_slices <= kCalMaxSlices, "num_slices %lld outside [0, 2^24]",
              (long long)num_slices);
  DFM_REQUIRE((num_slices > 0) == (d_slice_ids != nullptr) && (num_slices > 0) == (d_slices != nullptr),
              "slice ids and the slice table go with num_slices > 0, and only with it");
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_labels) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_scores) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(d_slice_ids) & 7) == 0,
              "labels and scores must be 4-byte aligned, slice ids 8-byte aligned");
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  const hipStream_t st = as_stream(stream);
  u64* ws = static_cast<u64*>(d_workspace);
  DFM_HIP_TRY(hipMemsetAsync(ws, 0, 8 * cal_ws_cells(num_bins, num_slices), st));
  const int head = cal_head(d_labels, d_scores, d_slice_ids);
  int rc;
  if (num_slices == 0)
    rc = cal_launch<false, false>(d_labels, d_scores, nullptr, n, head, num_bins, 0, ws, st);
  else if (cal_route(num_bins, num_slices) == 0)
    rc = cal_launch<true, true>(d_labels, d_scores, d_slice_ids, n, head, num_bins, num_slices, ws, st);
  else
    rc = cal_launch<true, false>(d_labels, d_scores, d_slice_ids, n, head, num_bins, num_slices, ws, st);
  if (rc) return rc;
  const int64_t fb = (num_slices + kCalFinishThreads - 1) / kCalFinishThreads;
  const int finish_blocks = static_cast<int>(fb < 1 ? 1 : (fb < kCalFinishBlocks ? fb : kCalFinishBlocks));
  hipLaunchKernelGGL(calibration_finish_kernel, dim3(finish_blocks), dim3(kCalFinishThreads), 0, st, ws, num_bins,
                     num_slices, d_bins, d_slices, d_out);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
