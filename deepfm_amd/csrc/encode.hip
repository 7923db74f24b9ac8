// Feature encoders on the device: the reference's LabelEncoder / MultiHotEncoder / MinMaxScaler
// (deepfm/data/transforms.py) as one table build and one encode launch, writing straight into DeviceColumns' matrices
// or a batch record in RecordLayout's byte format (data/packed.py).
//
//   vocab_build_kernel      one thread per key: claims the first free slot of its probe run with an integer CAS on the
//                           slot's index, then writes the key with a plain store.  No thread waits on another; a probe
//                           run is cut at `capacity` slots and counted.
//   encode_columns_kernel   one thread per (job, sample, position); blockIdx.y is the job, whose descriptor is read
//                           from the kernel-argument segment.  A slot is one aligned 16 bytes, so a probe touches one
//                           cache line.
#include "common.h"

namespace dfm {
namespace {

constexpr int kBlock = 256;
constexpr int64_t kMinCapacity = 16;
constexpr int64_t kMaxKeys = int64_t{1} << 30;

static_assert(sizeof(dfm_vocab_slot) == 16, "a slot is one 16-byte load");
static_assert(sizeof(dfm_encode_job) == 56, "64 jobs + the counts stay below 4 KiB of kernel arguments");

// include/deepfm_hip.h: the one mixer of the encoders (home slots and hashed buckets)
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}

__global__ __launch_bounds__(kBlock) void vocab_build_kernel(const int64_t* __restrict__ keys, int64_t n_keys,
                                                             dfm_vocab_slot* __restrict__ slots, int64_t capacity,
                                                             unsigned long long* __restrict__ status) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_keys) return;
  const int64_t key = keys[i];
  if (i > 0 && !(keys[i - 1] < key)) atomicAdd(&status[1], 1ull);
  const uint64_t mask = static_cast<uint64_t>(capacity) - 1;
  uint64_t pos = mix64(static_cast<uint64_t>(key)) & mask;
  const int index = static_cast<int>(i + 1);
  for (int64_t probe = 0; probe < capacity; ++probe) {
    if (atomicCAS(&slots[pos].index, 0, index) == 0) {
      slots[pos].key = key;                             // read by later launches only
      return;
    }
    pos = (pos + 1) & mask;
  }
  atomicAdd(&status[0], 1ull);
}

// The index of `key`, 0 if the table does not hold it.  An empty slot ends the probe run; so does `capacity` probes.
__device__ __forceinline__ int64_t vocab_lookup(const dfm_vocab_slot* __restrict__ slots, int log2_capacity,
                                                int64_t key) {
  const uint64_t capacity = uint64_t{1} << log2_capacity, mask = capacity - 1;
  uint64_t pos = mix64(static_cast<uint64_t>(key)) & mask;
  for (uint64_t probe = 0; probe < capacity; ++probe) {
    const int4 v = *reinterpret_cast<const int4*>(slots + pos);        // {key lo, key hi, index, pad}
    if (v.z == 0) return 0;
    const int64_t k = static_cast<int64_t>(static_cast<uint64_t>(static_cast<uint32_t>(v.x)) |
                                           (static_cast<uint64_t>(static_cast<uint32_t>(v.y)) << 32));
    if (k == key) return v.z;
    pos = (pos + 1) & mask;
  }
  return 0;
}

struct EncodeArgs {
  dfm_encode_job jobs[DFM_MAX_FIELDS];
  int64_t n, n_out;
};

__device__ __forceinline__ float scaled(double v, double lo, double hi) {
  const double denom = hi - lo;
  return denom == 0.0 ? 0.f : static_cast<float>((v - lo) / denom);
}

__global__ __launch_bounds__(kBlock) void encode_columns_kernel(EncodeArgs a) {
  const dfm_encode_job& job = a.jobs[blockIdx.y];
  const int64_t W = job.width;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= a.n_out * W) return;
  int64_t s = e, l = 0;
  if (W != 1) { s = e / W; l = e - s * W; }
  const bool live = s < a.n;
  const int64_t src = s * job.in_stride + l, dst = s * job.out_stride + l;
  switch (job.kind) {
    case DFM_ENC_LOOKUP: {
      int64_t v = 0;
      if (live) v = vocab_lookup(job.u.table.slots, job.log2_capacity, static_cast<const int64_t*>(job.in)[src]);
      static_cast<int64_t*>(job.out)[dst] = v;
      break;
    }
    case DFM_ENC_BAG: {
      int64_t v = 0;
      if (live) {
        int len = job.raw_width;
        if (job.u.table.lengths) len = min(max(job.u.table.lengths[s], 0), job.raw_width);
        if (l < len) v = vocab_lookup(job.u.table.slots, job.log2_capacity, static_cast<const int64_t*>(job.in)[src]);
      }
      static_cast<int64_t*>(job.out)[dst] = v;
      break;
    }
    case DFM_ENC_HASHED: {
      int64_t v = 0;
      if (live)
        v = static_cast<int64_t>(1 + mix64(static_cast<uint64_t>(static_cast<const int64_t*>(job.in)[src])) %
                                         job.u.num_buckets);
      static_cast<int64_t*>(job.out)[dst] = v;
      break;
    }
    case DFM_ENC_SCALE_F32:
      static_cast<float*>(job.out)[dst] =
          live ? scaled(static_cast<double>(static_cast<const float*>(job.in)[src]), job.u.scale.lo, job.u.scale.hi) : 0.f;
      break;
    case DFM_ENC_SCALE_F64:
      static_cast<float*>(job.out)[dst] =
          live ? scaled(static_cast<const double*>(job.in)[src], job.u.scale.lo, job.u.scale.hi) : 0.f;
      break;
    case DFM_ENC_COPY_F32:
      static_cast<float*>(job.out)[dst] = live ? static_cast<const float*>(job.in)[src] : 0.f;
      break;
    default:                                            // DFM_ENC_ZERO_F32
      static_cast<float*>(job.out)[dst] = 0.f;
      break;
  }
}

bool aligned(const void* p, size_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

}  // namespace
}  // namespace dfm

using namespace dfm;

extern "C" int64_t dfm_vocab_capacity(int64_t n_keys) {
  if (n_keys < 0 || n_keys > kMaxKeys) return 0;
  int64_t c = kMinCapacity;
  while (c < 2 * n_keys) c <<= 1;
  return c;
}

extern "C" int dfm_vocab_build(const int64_t* d_keys, int64_t n_keys, dfm_vocab_slot* d_slots, int64_t capacity,
                               uint64_t* d_status, dfm_stream_t stream) {
  DFM_REQUIRE(n_keys >= 0 && n_keys <= kMaxKeys, "n_keys = %lld outside [0, 2^30]", (long long)n_keys);
  DFM_REQUIRE(capacity == dfm_vocab_capacity(n_keys), "capacity %lld: %lld keys take dfm_vocab_capacity = %lld slots",
              (long long)capacity, (long long)n_keys, (long long)dfm_vocab_capacity(n_keys));
  DFM_REQUIRE(d_slots && d_status && (d_keys || n_keys == 0), "null argument");
  DFM_REQUIRE(aligned(d_slots, 16) && aligned(d_status, 8) && aligned(d_keys, 8), "misaligned argument");
  DFM_HIP_TRY(hipMemsetAsync(d_slots, 0, static_cast<size_t>(capacity) * sizeof(dfm_vocab_slot), as_stream(stream)));
  DFM_HIP_TRY(hipMemsetAsync(d_status, 0, 2 * sizeof(uint64_t), as_stream(stream)));
  if (n_keys == 0) return DFM_OK;
  const int64_t blocks = (n_keys + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(vocab_build_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, as_stream(stream),
                     d_keys, n_keys, d_slots, capacity, reinterpret_cast<unsigned long long*>(d_status));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_encode_columns(const dfm_encode_job* jobs, int num_jobs, int64_t n, int64_t n_out,
                                  dfm_stream_t stream) {
  DFM_REQUIRE(jobs && num_jobs >= 1 && num_jobs <= DFM_MAX_FIELDS, "num_jobs = %d outside [1, %d]", num_jobs,
              DFM_MAX_FIELDS);
  DFM_REQUIRE(n >= 0 && n <= n_out && n_out >= 1, "n = %lld, n_out = %lld: need 0 <= n <= n_out, n_out >= 1",
              (long long)n, (long long)n_out);
  EncodeArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  a.n_out = n_out;
  int64_t max_width = 1;
  for (int i = 0; i < num_jobs; ++i) {
    const dfm_encode_job& j = jobs[i];
    DFM_REQUIRE(j.kind >= DFM_ENC_LOOKUP && j.kind <= DFM_ENC_ZERO_F32, "job %d: kind %d", i, j.kind);
    const bool bag = j.kind == DFM_ENC_BAG, zero = j.kind == DFM_ENC_ZERO_F32;
    const bool table = bag || j.kind == DFM_ENC_LOOKUP;
    const bool ids = table || j.kind == DFM_ENC_HASHED;
    DFM_REQUIRE(j.width >= 1 && j.raw_width >= 1, "job %d: width %d, raw_width %d", i, j.width, j.raw_width);
    DFM_REQUIRE(bag || zero || (j.width == 1 && j.raw_width == 1), "job %d: only a bag has a width", i);
    DFM_REQUIRE(j.out && j.out_stride >= j.width, "job %d: out is null or its stride %d is below its width %d", i,
                j.out_stride, j.width);
    DFM_REQUIRE(zero || (j.in && j.in_stride >= j.raw_width),
                "job %d: in is null or its stride %d is below its width %d", i, j.in_stride, j.raw_width);
    const size_t in_size = (ids || j.kind == DFM_ENC_SCALE_F64) ? 8 : 4, out_size = ids ? 8 : 4;
    DFM_REQUIRE(aligned(j.out, out_size) && (zero || aligned(j.in, in_size)), "job %d: misaligned column", i);
    if (table) {
      DFM_REQUIRE(j.u.table.slots && aligned(j.u.table.slots, 16) && j.log2_capacity >= 4 && j.log2_capacity <= 31,
                  "job %d: table is null, misaligned or of 2^%d slots", i, j.log2_capacity);
      DFM_REQUIRE(!bag || aligned(j.u.table.lengths, 4), "job %d: misaligned lengths", i);
    }
    DFM_REQUIRE(j.kind != DFM_ENC_HASHED || j.u.num_buckets >= 1, "job %d: num_buckets must be positive", i);
    if (j.width > max_width) max_width = j.width;
    a.jobs[i] = j;
  }
  const int64_t blocks = (n_out * max_width + kBlock - 1) / kBlock;
  DFM_REQUIRE(blocks <= 0x7fffffff, "too many samples for one launch");
  hipLaunchKernelGGL(encode_columns_kernel, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(num_jobs)),
                     dim3(kBlock), 0, as_stream(stream), a);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
