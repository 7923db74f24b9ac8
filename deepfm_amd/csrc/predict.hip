// Forward-only (eval-mode) tower, head and the evaluation metrics (reference deepfm/training/trainer.py:244-294:
// model.eval(); probs = model.predict(batch); compute_auc / compute_logloss over the whole split).
//
// Eval mode differs from the training forward in the DNN tower only: BatchNorm normalises with its running
// statistics and dropout is the identity (reference dnn.py:45-55).  So one launch per layer suffices:
//
//   linear_bn_eval     a = relu(gamma * (x W^T + b - running_mean) * rsqrt(running_var + eps) + beta)
//                      on the exact-fp32 MFMA tile loop of gemm_core.h; z, statistics and running
//                      statistics are neither written nor read back
//   predict_head       logit = (first_order + extra) + (a . w + b), prob = sigmoid(logit), rows < valid only
//
// Metrics over a device score buffer, deterministic (integer atomics only, fp64 sums in a fixed order):
//   metrics_prepare    per-sample log loss (fp64) -> per-workgroup partials; npos / nneg; NaN flag; sort keys
//                      (the score of a negative, +inf for a positive: one ascending sort puts the negatives first)
//   auc_count          every positive binary-searches the sorted negatives: 2 #(neg < s) + #(neg == s), int64
//   metrics_finalize   one workgroup: log loss partials in order, AUC = count / (2 npos nneg) in fp64
#include <cmath>

#include "gemm_core.h"
#include "metric_common.h"

using namespace dfm;
using namespace dfm::gemm;

namespace {

// BatchNorm's normalisation as bn_relu_dropout_apply forms it (gamma * ((z - mean) * rstd) + beta), with the running
// statistics in place of the batch statistics.
__device__ __forceinline__ void eval_tile_epilogue(const f32x16& acc, const TilePos& pos, int m0, int n0, int M,
                                                   int N, const float* __restrict__ bias,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   const float* __restrict__ running_mean,
                                                   const float* __restrict__ running_var, float eps,
                                                   float* __restrict__ out) {
  const int n = n0 + pos.col();
  if (n >= N) return;
  const float bv = bias ? bias[n] : 0.f;
  const float mu = running_mean[n], rs = rsqrtf(running_var[n] + eps), ga = gamma[n], be = beta[n];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int m = m0 + pos.row(reg);
    if (m < M) {
      const float z = acc[reg] + bv;
      out[static_cast<int64_t>(m) * N + n] = fmaxf(fmaf(ga, (z - mu) * rs, be), 0.f);
    }
  }
}

template <bool FAST>
__global__ __launch_bounds__(kThreads) void linear_bn_eval_kernel(
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ running_mean,
    const float* __restrict__ running_var, float eps, float* __restrict__ out, int M, int N, int K, int tiles_n) {
  __shared__ Smem sm;
  const TilePos pos;
  const int lt = xcd_logical_index(blockIdx.x, gridDim.x);
  const int m0 = (lt / tiles_n) * BM, n0 = (lt % tiles_n) * BN;
  f32x16 acc = {};
  mainloop<true, true, FAST, FAST>(x, ldx, w, K, M, N, m0, n0, 0, K, sm, pos, acc);
  if (pos.khalf == 1) return;
  eval_tile_epilogue(acc, pos, m0, n0, M, N, bias, gamma, beta, running_mean, running_var, eps, out);
}

// ---- head: 8 lanes per sample, one float4 per lane and 32 features ----------------------------------------
constexpr int kPhThreads = 256, kPhLanes = 8, kPhRows = kPhThreads / kPhLanes;

__global__ __launch_bounds__(kPhThreads) void predict_head_kernel(
    const float* __restrict__ a, int M, int K, const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ fo, const float* __restrict__ extra, int valid, float* __restrict__ logits,
    float* __restrict__ probs) {
  const int l8 = threadIdx.x & (kPhLanes - 1);
  const int m = blockIdx.x * kPhRows + threadIdx.x / kPhLanes;
  const int mc = m < M ? m : M - 1;                // every lane takes part in the butterfly
  const float* row = a + static_cast<int64_t>(mc) * K;
  float dot = 0.f;
  for (int j = l8 * 4; j < K; j += kPhLanes * 4) {
    const float4 av = ld4(row + j), wv = ld4(w + j);
    dot = fmaf(av.x, wv.x, dot); dot = fmaf(av.y, wv.y, dot);
    dot = fmaf(av.z, wv.z, dot); dot = fmaf(av.w, wv.w, dot);
  }
  dot += __shfl_xor(dot, 1, kWave);
  dot += __shfl_xor(dot, 2, kWave);
  dot += __shfl_xor(dot, 4, kWave);
  if (l8 != 0 || m >= valid) return;
  // (first_order + extra) + (dnn . w + b): the association of deepfm.py / xdeepfm.py / attention_deepfm.py
  const float zl = ((fo ? fo[m] : 0.f) + (extra ? extra[m] : 0.f)) + (dot + (b ? b[0] : 0.f));
  if (logits) logits[m] = zl;
  probs[m] = 1.f / (1.f + expf(-zl));
}

struct HeadArgs {
  const float* a; int M, K; const float* w; const float* b; const float* fo; const float* extra; int valid;
  float* logits; float* probs;
  void* params[10];
  void bind() {
    params[0] = &a; params[1] = &M; params[2] = &K; params[3] = &w; params[4] = &b;
    params[5] = &fo; params[6] = &extra; params[7] = &valid; params[8] = &logits; params[9] = &probs;
  }
};

int head_args(const float* d_a, int64_t batch, int features, const float* d_w, const float* d_b,
              const float* d_first_order, const float* d_extra, int64_t valid, float* d_logits, float* d_probs,
              HeadArgs* h) {
  DFM_REQUIRE(d_a && d_w && d_probs, "null argument");
  DFM_REQUIRE(batch > 0 && batch < (1 << 30), "bad batch");
  DFM_REQUIRE(valid >= 0 && valid <= batch, "valid %lld outside [0, batch]", (long long)valid);
  DFM_REQUIRE(features > 0 && features % 4 == 0, "head features must be a positive multiple of 4");
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_a) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_w) & 15) == 0,
              "pointers must be 16-byte aligned");
  *h = HeadArgs{d_a, static_cast<int>(batch), features, d_w, d_b, d_first_order, d_extra, static_cast<int>(valid),
                d_logits, d_probs, {}};
  h->bind();
  return DFM_OK;
}

dim3 head_grid(int64_t batch) { return dim3(static_cast<unsigned>((batch + kPhRows - 1) / kPhRows)); }

// ---- metrics -------------------------------------------------------------------------------------------
constexpr int kMtThreads = 256;
constexpr int kMtMaxBlocks = 1024;

struct MetricsHeader {                 // the first 64 bytes of the workspace
  unsigned long long npos, nneg, count, nan;
  unsigned long long pad[4];
};

int metrics_blocks(int64_t n) {
  const int b = blocks_for(n, kMtThreads, kMtMaxBlocks);
  return b > 0 ? b : 1;
}

// one value through block_sums (metric_common.h): the sum in every thread; a barrier goes between two calls on one red
template <typename T>
__device__ __forceinline__ T block_sum(T v, T (*red)[kMtThreads]) {
  T one[1] = {v};
  block_sums(one, red);
  return red[0][0];
}

__global__ __launch_bounds__(kMtThreads) void metrics_prepare_kernel(const float* __restrict__ labels,
                                                                     const float* __restrict__ scores, int64_t n,
                                                                     float* __restrict__ keys,
                                                                     MetricsHeader* __restrict__ hdr,
                                                                     double* __restrict__ partial) {
  __shared__ double redd[1][kMtThreads];
  __shared__ unsigned long long redu[1][kMtThreads];
  double ll = 0.0;
  unsigned long long np = 0, nn = 0, bad = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMtThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kMtThreads + threadIdx.x; i < n; i += stride) {
    const float s = scores[i];
    const bool pos = labels[i] > 0.5f;
    if (isnan(s)) ++bad;
    np += pos; nn += !pos;
    keys[i] = pos ? INFINITY : s;
    ll += sample_logloss(s, pos);
  }
  ll = block_sum(ll, redd);
  const unsigned long long tp = block_sum(np, redu);
  __syncthreads();
  const unsigned long long tn = block_sum(nn, redu);
  __syncthreads();
  const unsigned long long tb = block_sum(bad, redu);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = ll;
    atomicAdd(&hdr->npos, tp);
    atomicAdd(&hdr->nneg, tn);
    atomicAdd(&hdr->nan, tb);
  }
}

// #(sorted[0, n) < s) and #(sorted[0, n) <= s)
__device__ __forceinline__ int64_t lower_bound(const float* __restrict__ v, int64_t n, float s) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (v[mid] < s) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int64_t upper_bound(const float* __restrict__ v, int64_t n, float s) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (v[mid] <= s) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kMtThreads) void auc_count_kernel(const float* __restrict__ labels,
                                                               const float* __restrict__ scores, int64_t n,
                                                               const float* __restrict__ sorted,
                                                               MetricsHeader* __restrict__ hdr) {
  __shared__ unsigned long long red[1][kMtThreads];
  const int64_t nneg = static_cast<int64_t>(hdr->nneg);
  unsigned long long c = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kMtThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kMtThreads + threadIdx.x; i < n; i += stride) {
    if (!(labels[i] > 0.5f)) continue;
    const float s = scores[i];
    const int64_t lt = lower_bound(sorted, nneg, s);
    const int64_t le = upper_bound(sorted, nneg, s);
    c += static_cast<unsigned long long>(lt + le);      // 2 #(neg < s) + #(neg == s)
  }
  c = block_sum(c, red);
  if (threadIdx.x == 0) atomicAdd(&hdr->count, c);
}

// out: [auc (NaN when a class is missing), logloss, npos, nneg, NaN scores]
__global__ __launch_bounds__(kMtThreads) void metrics_finalize_kernel(const MetricsHeader* __restrict__ hdr,
                                                                      const double* __restrict__ partial, int blocks,
                                                                      int64_t n, double* __restrict__ out) {
  __shared__ double red[1][kMtThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < blocks; i += kMtThreads) s += partial[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const double np = static_cast<double>(hdr->npos), nn = static_cast<double>(hdr->nneg);
    out[0] = (hdr->npos && hdr->nneg) ? static_cast<double>(hdr->count) / (2.0 * np * nn) : quiet_nan();
    out[1] = s / static_cast<double>(n);
    out[2] = np;
    out[3] = nn;
    out[4] = static_cast<double>(hdr->nan);
  }
}

}  // namespace

extern "C" int dfm_linear_bn_eval(const float* d_x, int64_t ldx, const float* d_w, const float* d_bias,
                                  int64_t batch, int out_features, int in_features, const float* d_gamma,
                                  const float* d_beta, const float* d_running_mean, const float* d_running_var,
                                  float eps, float* d_out, dfm_stream_t stream) {
  DFM_REQUIRE(d_x && d_w && d_gamma && d_beta && d_running_mean && d_running_var && d_out, "null argument");
  DFM_REQUIRE(batch > 0 && batch < (1 << 30) && out_features > 0 && in_features > 0 && ldx >= in_features,
              "bad shape");
  const int M = static_cast<int>(batch), N = out_features, K = in_features;
  const int tn = (N + BN - 1) / BN;
  const dim3 grid(static_cast<unsigned>(tn) * static_cast<unsigned>((M + BM - 1) / BM));
  const bool fast = operand_fast(d_x, ldx, true, M, K) && operand_fast(d_w, K, true, N, K);
  if (fast)
    hipLaunchKernelGGL(linear_bn_eval_kernel<true>, grid, dim3(kThreads), 0, as_stream(stream), d_x, ldx, d_w,
                       d_bias, d_gamma, d_beta, d_running_mean, d_running_var, eps, d_out, M, N, K, tn);
  else
    hipLaunchKernelGGL(linear_bn_eval_kernel<false>, grid, dim3(kThreads), 0, as_stream(stream), d_x, ldx, d_w,
                       d_bias, d_gamma, d_beta, d_running_mean, d_running_var, eps, d_out, M, N, K, tn);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_predict_head(const float* d_a, int64_t batch, int features, const float* d_w, const float* d_b,
                                const float* d_first_order, const float* d_extra, int64_t valid, float* d_logits,
                                float* d_probs, const dfm_launch* at) {
  DFM_CHECK_LAUNCH(at);
  HeadArgs h;
  if (int rc = head_args(d_a, batch, features, d_w, d_b, d_first_order, d_extra, valid, d_logits, d_probs, &h))
    return rc;
  return launch_at(at, reinterpret_cast<const void*>(&predict_head_kernel), head_grid(batch), dim3(kPhThreads), 0,
                   h.params, false);
}

extern "C" size_t dfm_metrics_workspace_bytes(int64_t n) {
  return sizeof(MetricsHeader) + sizeof(double) * static_cast<size_t>(metrics_blocks(n));
}

extern "C" int dfm_metrics_prepare(const float* d_labels, const float* d_scores, int64_t n, float* d_keys,
                                   void* d_workspace, dfm_stream_t stream) {
  DFM_REQUIRE(d_labels && d_scores && d_keys && d_workspace, "null argument");
  DFM_REQUIRE(n > 0 && n < (int64_t(1) << 40), "bad sample count");
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "workspace must be 16-byte aligned");
  MetricsHeader* hdr = static_cast<MetricsHeader*>(d_workspace);
  DFM_HIP_TRY(hipMemsetAsync(hdr, 0, sizeof(MetricsHeader), as_stream(stream)));
  hipLaunchKernelGGL(metrics_prepare_kernel, dim3(metrics_blocks(n)), dim3(kMtThreads), 0, as_stream(stream),
                     d_labels, d_scores, n, d_keys, hdr, reinterpret_cast<double*>(hdr + 1));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_metrics_finish(const float* d_labels, const float* d_scores, int64_t n, const float* d_sorted_keys,
                                  void* d_workspace, double* d_out, dfm_stream_t stream) {
  DFM_REQUIRE(d_labels && d_scores && d_sorted_keys && d_workspace && d_out, "null argument");
  DFM_REQUIRE(n > 0 && n < (int64_t(1) << 40), "bad sample count");
  MetricsHeader* hdr = static_cast<MetricsHeader*>(d_workspace);
  const int blocks = metrics_blocks(n);
  hipLaunchKernelGGL(auc_count_kernel, dim3(blocks), dim3(kMtThreads), 0, as_stream(stream), d_labels, d_scores, n,
                     d_sorted_keys, hdr);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(metrics_finalize_kernel, dim3(1), dim3(kMtThreads), 0, as_stream(stream), hdr,
                     reinterpret_cast<const double*>(hdr + 1), blocks, n, d_out);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
