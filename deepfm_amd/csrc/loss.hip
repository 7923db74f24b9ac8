// BCEWithLogitsLoss (mean reduction) forward + gradient in one pass
// (reference deepfm/training/trainer.py:59, 221: nn.BCEWithLogitsLoss()):
//   loss = mean( max(z,0) - z*y + log1p(exp(-|z|)) ),   d loss / d z = (sigmoid(z) - y) / B
// Stage 1 writes d z and one partial sum per workgroup; stage 2 adds the partials in a fixed
// order (bitwise reproducible) and divides by B.
#include "common.h"
#include "tail_bodies.h"

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

// ---------------------------------------------------------------------------------------------------------------
// The same loss with ROW tables (training/rowsparse.py): get_l2_reg_loss covers every element of every SPARSE table,
// up to 442 M floats at the Criteo shape, which no step can re-sum.  The sum S of their squares changes only on the
// rows a step updates, so it is carried: dfm_tables_sqnorm forms it once per epoch, dfm_rows_sqnorm sums the rows a
// step owns before and after its update, and dfm_loss_accumulate_tables folds the difference into S in front of the
// next step's loss.  Doubles throughout, one partial per workgroup, partials added in index order by one workgroup:
// no atomics, no arrival counters, no workgroup reads what another of the same launch wrote.
namespace {

constexpr int kSqThreads = 256;
constexpr int64_t kSqMinRows = 64;        // rows per workgroup of dfm_tables_sqnorm, at least
constexpr int64_t kSqMaxBlocks = 4096;

struct SqTables {
  const float* w2[DFM_MAX_FIELDS];
  const float* w1[DFM_MAX_FIELDS];
  int32_t stride2[DFM_MAX_FIELDS];
  int32_t stride1[DFM_MAX_FIELDS];
  int64_t first[DFM_MAX_FIELDS + 1];      // first[s]: rows of the tables in front of table s; first[S]: all rows
};

inline int64_t sq_blocks(int64_t total_rows) {
  const int64_t b = (total_rows + kSqMinRows - 1) / kSqMinRows;
  return b < 1 ? 1 : (b > kSqMaxBlocks ? kSqMaxBlocks : b);
}

// sum of s over the workgroup: a shift-down tree inside each wave, the wave sums in wave order by thread 0 (the only
// thread whose return value is the sum)
__device__ __forceinline__ double block_sum_ordered(double s, double* wave_sum) {
  for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
  if (lane_id() == 0) wave_sum[threadIdx.x / kWave] = s;
  __syncthreads();
  double sum = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < static_cast<int>(blockDim.x) / kWave; ++w) sum += wave_sum[w];
  __syncthreads();
  return sum;
}

// workgroup b: rows [b * rows_per_block, (b + 1) * rows_per_block) of the tables laid end to end; D / 4 lanes per row
__global__ __launch_bounds__(kSqThreads) void tables_sqnorm_kernel(SqTables tb, int S, int D, int64_t rows_per_block,
                                                                   double* __restrict__ partial) {
  __shared__ double wave_sum[kSqThreads / kWave];
  const int lpr = D / 4, rpi = kSqThreads / lpr;           // lanes per row, rows per iteration
  const int q = threadIdx.x % lpr, r = threadIdx.x / lpr;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * rows_per_block;
  const int64_t hi = lo + rows_per_block < tb.first[S] ? lo + rows_per_block : tb.first[S];
  double s = 0.0;
  if (r < rpi) {
    for (int f = 0; f < S; ++f) {
      const int64_t a = lo > tb.first[f] ? lo : tb.first[f];
      const int64_t b = hi < tb.first[f + 1] ? hi : tb.first[f + 1];
      const float* __restrict__ w2 = tb.w2[f];
      const float* __restrict__ w1 = tb.w1[f];
      const int64_t s2 = tb.stride2[f], s1 = tb.stride1[f];
#pragma unroll 4
      for (int64_t g = a + r; g < b; g += rpi) {
        const int64_t row = g - tb.first[f];
        s += sq4(ld4(w2 + row * s2 + 4 * q));
        if (q == 0) {
          const double x = w1[row * s1];
          s += x * x;
        }
      }
    }
  }
  const double sum = block_sum_ordered(s, wave_sum);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// out[0] = the partials added by one workgroup: thread t takes t, t + 1024, ..., then block_sum_ordered
__global__ __launch_bounds__(kLossThreads) void sqnorm_finish_kernel(const double* __restrict__ partial, int n,
                                                                     double* __restrict__ out) {
  __shared__ double wave_sum[kLossThreads / kWave];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kLossThreads) s += partial[i];
  const double sum = block_sum_ordered(s, wave_sum);
  if (threadIdx.x == 0) out[0] = sum;
}

// the entries the row-wise update touches (rowadam_apply_body's indexing: D / 4 lanes per entry, owned entries only)
__global__ __launch_bounds__(tail::kTailThreads) void rows_sqnorm_kernel(
    int own_blocks, tail::TableArgs tabs, int S, int D, int L, const int32_t* __restrict__ uniq_rows,
    const int32_t* __restrict__ num_uniq, const int32_t* __restrict__ owner_flag, double* __restrict__ partial) {
  __shared__ double wave_sum[tail::kTailThreads / kWave];
  const int blk = blockIdx.x;
  double s = 0.0;
  if (blk < own_blocks) {
    const int lpr = D / 4;
    const int64_t t = static_cast<int64_t>(blk) * tail::kTailThreads + threadIdx.x;
    const int q = static_cast<int>(t % lpr);
    const int64_t entry = t / lpr;
    const int64_t list = entry / tail::CH;
    const int u = static_cast<int>(entry % tail::CH);
    if (list < static_cast<int64_t>(L) * S && u < num_uniq[list] && owner_flag[list * tail::CH + u]) {
      const dfm_table tb = tabs.t[list % S];
      const int64_t row = uniq_rows[list * tail::CH + u];
      s = sq4(ld4(tb.w2 + row * tb.stride2 + q * 4));
      if (q == 0) {
        const double x = tb.w1[row * tb.stride1];
        s += x * x;
      }
    }
  }
  const double sum = block_sum_ordered(s, wave_sum);
  if (threadIdx.x == 0) partial[blk] = sum;          // blocks behind the step's own: 0
}

__global__ __launch_bounds__(kLossThreads) void loss_accumulate_tables_kernel(
    const float* __restrict__ loss, float l2, const float* __restrict__ p, int64_t n, int vec, double* __restrict__ S,
    double* __restrict__ old_partial, double* __restrict__ new_partial, int n_partials, double* __restrict__ acc) {
  __shared__ double wave_sum[kLossThreads / kWave];
  const int t = threadIdx.x;
  // the previous step's update of the tables, pending since its two dfm_rows_sqnorm passes
  double s_old = 0.0, s_new = 0.0;
  for (int i = t; i < n_partials; i += kLossThreads) {
    s_old += old_partial[i];
    s_new += new_partial[i];
    old_partial[i] = 0.0;
    new_partial[i] = 0.0;
  }
  const double sum_old = block_sum_ordered(s_old, wave_sum);
  const double sum_new = block_sum_ordered(s_new, wave_sum);
  // the dense embedding parameters: loss_accumulate_kernel's sum, term for term
  double s = 0.0;
  const int64_t n4 = vec ? n / 4 : 0;
#pragma unroll 4
  for (int64_t i = t; i < n4; i += kLossThreads) s += sq4(ld4(p + 4 * i));
  for (int64_t i = 4 * n4 + t; i < n; i += kLossThreads) {
    const double x = p[i];
    s += x * x;
  }
  const double dense = block_sum_ordered(s, wave_sum);
  if (t == 0) {
#pragma clang fp contract(off)
    const double tables = (S[0] + sum_new) - sum_old;
    S[0] = tables;
    const double bce = static_cast<double>(*loss);
    acc[0] += bce + static_cast<double>(l2) * (dense + tables);
    acc[1] += 1.0;
    acc[2] += bce;
  }
}

int fill_sq_tables(const dfm_table* tables, int S, int D, const int32_t* vocab, SqTables* out) {
  memset(out, 0, sizeof(*out));
  for (int s = 0; s < S; ++s) {
    DFM_REQUIRE(tables[s].w2 && tables[s].w1, "table %d: null weights", s);
    DFM_REQUIRE(vocab[s] > 0, "table %d: no rows", s);
    out->w2[s] = tables[s].w2;
    out->w1[s] = tables[s].w1;
    out->stride2[s] = tables[s].stride2 ? tables[s].stride2 : D;
    out->stride1[s] = tables[s].stride1 ? tables[s].stride1 : 1;
    DFM_REQUIRE(out->stride2[s] >= D && out->stride2[s] % 4 == 0 && out->stride1[s] >= 1, "table %d: bad row strides", s);
    DFM_REQUIRE((reinterpret_cast<uintptr_t>(tables[s].w2) & 15) == 0, "table %d: rows must be 16-byte aligned", s);
    out->first[s + 1] = out->first[s] + vocab[s];
  }
  return DFM_OK;
}

inline int64_t rows_sq_blocks(int S, int D, int L) {
  return (static_cast<int64_t>(L) * S * tail::CH * (D / 4) + tail::kTailThreads - 1) / tail::kTailThreads;
}

}  // namespace

extern "C" int64_t dfm_tables_sqnorm_num_partials(int64_t total_rows) { return sq_blocks(total_rows); }

extern "C" int dfm_tables_sqnorm(const dfm_table* tables, int num_sparse, int dim, const int32_t* vocab,
                                 double* d_partials, double* d_out, dfm_stream_t stream) {
  DFM_REQUIRE(tables && vocab && d_partials && d_out, "null argument");
  DFM_REQUIRE(num_sparse > 0 && num_sparse <= DFM_MAX_FIELDS, "bad table count");
  DFM_REQUIRE(dim > 0 && dim % 4 == 0 && dim <= 256, "dim must be a multiple of 4 and <= 256");
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(d_partials) % 8 == 0 && reinterpret_cast<uintptr_t>(d_out) % 8 == 0,
              "d_partials and d_out must be 8-byte aligned");
  SqTables tb;
  if (int rc = fill_sq_tables(tables, num_sparse, dim, vocab, &tb)) return rc;
  const int64_t total = tb.first[num_sparse], blocks = sq_blocks(total);
  const int64_t rows_per_block = (total + blocks - 1) / blocks;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(tables_sqnorm_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kSqThreads), 0, st, tb, num_sparse,
                     dim, rows_per_block, d_partials);
  DFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(sqnorm_finish_kernel, dim3(1), dim3(kLossThreads), 0, st, d_partials, static_cast<int>(blocks),
                     d_out);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_rows_sqnorm(const dfm_table* tables, int num_sparse, int dim, int num_lists,
                               const int32_t* d_uniq_rows, const int32_t* d_num_uniq, const int32_t* d_owner_flag,
                               double* d_partials, int64_t n_partials_total, dfm_stream_t stream) {
  DFM_REQUIRE(tables && d_uniq_rows && d_num_uniq && d_owner_flag && d_partials, "null argument");
  DFM_REQUIRE(num_sparse > 0 && num_sparse <= DFM_MAX_FIELDS && num_lists > 0, "bad sizes");
  DFM_REQUIRE(dim > 0 && dim % 4 == 0 && dim <= 256, "dim must be a multiple of 4 and <= 256");
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(d_partials) % 8 == 0, "d_partials must be 8-byte aligned");
  const int64_t own = rows_sq_blocks(num_sparse, dim, num_lists);
  DFM_REQUIRE(n_partials_total >= own && n_partials_total < (int64_t(1) << 31),
              "%lld partials do not hold this step's %lld", (long long)n_partials_total, (long long)own);
  tail::TableArgs ta;
  memset(&ta, 0, sizeof(ta));
  for (int s = 0; s < num_sparse; ++s) {
    DFM_REQUIRE(tables[s].w2 && tables[s].w1, "table %d: null weights", s);
    ta.t[s] = tables[s];
    if (ta.t[s].stride2 == 0) ta.t[s].stride2 = dim;
    if (ta.t[s].stride1 == 0) ta.t[s].stride1 = 1;
    DFM_REQUIRE(ta.t[s].stride2 >= dim && ta.t[s].stride2 % 4 == 0 && ta.t[s].stride1 >= 1, "table %d: bad row strides", s);
  }
  hipLaunchKernelGGL(rows_sqnorm_kernel, dim3(static_cast<unsigned>(n_partials_total)), dim3(tail::kTailThreads), 0,
                     as_stream(stream), static_cast<int>(own), ta, num_sparse, dim, num_lists, d_uniq_rows, d_num_uniq,
                     d_owner_flag, d_partials);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_loss_accumulate_tables(const float* d_loss, float l2, const float* d_p, int64_t n_l2, double* d_S,
                                          double* d_old_partials, double* d_new_partials, int64_t n_partials,
                                          double* d_acc, dfm_stream_t stream) {
  DFM_REQUIRE(d_loss && d_acc && d_S && d_old_partials && d_new_partials, "null argument");
  DFM_REQUIRE(n_l2 >= 0 && n_partials >= 0 && n_partials < (int64_t(1) << 31), "bad sizes");
  DFM_REQUIRE(reinterpret_cast<uintptr_t>(d_acc) % 8 == 0 && reinterpret_cast<uintptr_t>(d_S) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(d_old_partials) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(d_new_partials) % 8 == 0, "the doubles must be 8-byte aligned");
  const bool reads = n_l2 > 0 && l2 != 0.0f;
  DFM_REQUIRE(!reads || d_p, "d_p is NULL with n_l2 > 0 and l2 != 0");
  const int vec = reads && reinterpret_cast<uintptr_t>(d_p) % 16 == 0;
  hipLaunchKernelGGL(loss_accumulate_tables_kernel, dim3(1), dim3(kLossThreads), 0, as_stream(stream), d_loss, l2, d_p,
                     reads ? n_l2 : int64_t(0), vec, d_S, d_old_partials, d_new_partials, static_cast<int>(n_partials),
                     d_acc);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
