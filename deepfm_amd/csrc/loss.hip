// BCEWithLogitsLoss (mean reduction) forward + gradient in one pass
// (reference deepfm/training/trainer.py:59, 221: nn.BCEWithLogitsLoss()):
//   loss = mean( max(z,0) - z*y + log1p(exp(-|z|)) ),   d loss / d z = (sigmoid(z) - y) / B
// Stage 1 writes d z and one partial sum per workgroup; stage 2 adds the partials in a fixed
// order (bitwise reproducible) and divides by B.
#include "common.h"

using namespace dfm;

namespace {
constexpr int kThreads = 256;
constexpr int kPerThread = 4;
inline int64_t bce_blocks(int64_t n) { return (n + kThreads * kPerThread - 1) / (kThreads * kPerThread); }
}

__global__ __launch_bounds__(kThreads) void bce_fwd_bwd(const float* __restrict__ z, const float* __restrict__ y,
                                                        int64_t n, float inv_n, float* __restrict__ dz,
                                                        float* __restrict__ partial) {
  const int64_t base = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * kPerThread;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t i = base + j;
    if (i < n) {
      const float zi = z[i], yi = y[i];
      const float e = expf(-fabsf(zi));
      acc += fmaxf(zi, 0.f) - zi * yi + log1pf(e);
      const float sig = zi >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      dz[i] = (sig - yi) * inv_n;
    }
  }
  __shared__ float wsum[kThreads / kWave];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, kWave);
  if (lane_id() == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(kThreads) void bce_finalize(const float* __restrict__ partial, int n_partials,
                                                         float inv_n, float* __restrict__ loss) {
  __shared__ float wsum[kThreads / kWave];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_partials; i += kThreads) acc += partial[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, kWave);
  if (lane_id() == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])) * inv_n;
}

extern "C" size_t dfm_bce_workspace_bytes(int64_t n) { return sizeof(float) * static_cast<size_t>(bce_blocks(n > 0 ? n : 1)); }

extern "C" int dfm_bce_with_logits(const float* d_logits, const float* d_labels, int64_t n, float* d_loss,
                                   float* d_g_logits, void* d_workspace, dfm_stream_t stream) {
  DFM_REQUIRE(d_logits && d_labels && d_loss && d_g_logits && d_workspace, "null argument");
  DFM_REQUIRE(n > 0, "empty batch");
  hipStream_t st = as_stream(stream);
  const int64_t blocks = bce_blocks(n);
  float* partial = static_cast<float*>(d_workspace);
  const float inv_n = 1.f / static_cast<float>(n);
  hipLaunchKernelGGL(bce_fwd_bwd, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, d_logits, d_labels, n,
                     inv_n, d_g_logits, partial);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(bce_finalize, dim3(1), dim3(kThreads), 0, st, partial, static_cast<int>(blocks), inv_n, d_loss);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The epoch's training loss on the device (reference trainer.py:221-239: total_loss += loss.item() per batch,
// loss = BCE + get_l2_reg_loss(), base.py:78-83) without a host read per step: dfm_loss_accumulate.
//
// One workgroup of 1024 threads, one launch at every size: thread t sums, in double, the squares of the float4s
// t, t + 1024, ... of d_p (then of the scalar elements behind the last whole float4), the 64 lanes of a wave are added
// by a shift-down tree, the 16 wave sums by thread 0 in wave order.  No atomics, no arrival counter, no second
// launch: the order of every addition is a function of (n_l2, alignment of d_p) alone, so the sum is bitwise
// reproducible.  At the MovieLens size (n_l2 ~ 5e4: 12 float4 loads per thread) the launch is latency, not
// bandwidth; 1e6 floats are ~250 loads per thread, still one launch.
namespace {

constexpr int kLossThreads = 1024;

__device__ __forceinline__ double sq4(float4 v) {
  const double x = v.x, y = v.y, z = v.z, w = v.w;
  return ((x * x + y * y) + z * z) + w * w;
}

__global__ __launch_bounds__(kLossThreads) void loss_accumulate_kernel(const float* __restrict__ loss, float l2,
                                                                       const float* __restrict__ p, int64_t n,
                                                                       int vec, double* __restrict__ acc) {
  __shared__ double wave_sum[kLossThreads / kWave];
  const int t = threadIdx.x;
  double s = 0.0;
  const int64_t n4 = vec ? n / 4 : 0;
#pragma unroll 4
  for (int64_t i = t; i < n4; i += kLossThreads) s += sq4(ld4(p + 4 * i));
  for (int64_t i = 4 * n4 + t; i < n; i += kLossThreads) {
    const double x = p[i];
    s += x * x;
  }
  for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
  if (lane_id() == 0) wave_sum[t / kWave] = s;
  __syncthreads();
  if (t == 0) {
    // the header's formula as written, a product and a sum with a rounding each: no contraction into an fma, so that
    // a host restatement in double gives the same bits for the same order
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int w = 0; w < kLossThreads / kWave; ++w) sum += wave_sum[w];
    const double bce = static_cast<double>(*loss);
    acc[0] += bce + static_cast<double>(l2) * sum;
    acc[1] += 1.0;
    acc[2] += bce;
  }
}

}  // namespace

extern "C" int dfm_loss_accumulate(const float* d_loss, float l2, const float* d_p, int64_t n_l2, double* d_acc,
                                   dfm_stream_t stream) {
  DFM_REQUIRE(d_loss && d_acc, "null argument");
  DFM_REQUIRE(n_l2 >= 0, "n_l2 must be non-negative");
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(d_acc) % 8 == 0, "d_acc must be 8-byte aligned");
  const bool reads = n_l2 > 0 && l2 != 0.0f;       // otherwise no parameter is read (d_p may be NULL)
  DFM_REQUIRE(!reads || d_p, "d_p is NULL with n_l2 > 0 and l2 != 0");
  const int vec = reads && reinterpret_cast<uintptr_t>(d_p) % 16 == 0;
  hipLaunchKernelGGL(loss_accumulate_kernel, dim3(1), dim3(kLossThreads), 0, as_stream(stream), d_loss, l2, d_p,
                     reads ? n_l2 : int64_t(0), vec, d_acc);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
