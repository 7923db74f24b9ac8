// Permutation field importance: the device side that forms the shuffled batch records (include/deepfm_hip.h has the
// contract; training/importance.py the loop around it).
//
//   keys      key[i] = (mix32(seed * G + S + (repeat << 40) + i) >> 1) << 32 | i: the counter of bootstrap.hip with the
//             salt S = "PermKeys"; non-negative and distinct, so one ascending sort of them is the permutation of
//             (seed, repeat): perm[j] = low word of sorted[j]
//   permute   the record of samples [first, first + count) of a set of whole batch records: a field of `mask` takes
//             slot i from sample perm[first + i], every other field and the label from sample first + i, slots past
//             count are padding.  grid.y walks the segments of the record (a field's column, the labels, the empty
//             row of a kind the schema lacks), grid.x its words: a thread per 8-byte word (4-byte in DENSE and label
//             rows), coalesced stores, one gathered load per permuted word.  No atomics, no LDS.
//
// The launch moves at most 2 * record_bytes and is launch-bound at every batch size the predictors run; it is not
// tuned beyond that (tools/time_importance.py measures it beside an empty launch).
#include "dropout.h"
#include "metric_common.h"

using namespace dfm;

namespace {

constexpr int kPmThreads = 256;
constexpr int kPmMaxBlocks = 64;                              // per segment; the loop strides over the rest
constexpr uint64_t kPmGolden = 0x9E3779B97F4A7C15ull, kPmSalt = 0x5065726D4B657973ull;
constexpr int64_t kPmMaxN = (int64_t(1) << 31) - 1;
constexpr int64_t kPmMaxRepeat = int64_t(1) << 24;
constexpr int64_t kPmMaxBatch = int64_t(1) << 24;
constexpr int kPmMaxLength = 1 << 16;

constexpr int kSegNarrow = 1;                                 // 4-byte words (DENSE rows, the labels)
constexpr int kSegZero = 2;                                   // nothing is read: the empty row of a missing kind
constexpr int kSegMasked = 4;                                 // slots read through the permutation
constexpr int kPmMaxSegs = DFM_MAX_FIELDS + 3;                // the fields, the labels, two empty rows

// One contiguous block of a record, (batch_size, words) words: passed by value in the kernel-argument segment and
// indexed by blockIdx.y only, so the read is a scalar load.
struct PmSeg {
  int64_t offset;
  int32_t words;                                              // per slot: max_length of a SEQUENCE field, else 1
  int32_t flags;
};
struct PmSegs {
  PmSeg s[kPmMaxSegs];
};

__global__ __launch_bounds__(kPmThreads) void permutation_keys_kernel(uint64_t base, int64_t n,
                                                                      int64_t* __restrict__ keys) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kPmThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kPmThreads + threadIdx.x; i < n; i += stride) {
    const uint64_t h = mix32(base + static_cast<uint64_t>(i)) >> 1;
    keys[i] = static_cast<int64_t>((h << 32) | static_cast<uint64_t>(i));
  }
}

template <typename Word>
__device__ __forceinline__ void pm_move(const char* __restrict__ set, int64_t set_stride, const PmSeg& sg, int64_t batch,
                                        int64_t src, int64_t j, int64_t w, char* __restrict__ out) {
  Word v = 0;
  if (src >= 0) {
    const int64_t rec = src / batch;
    const int64_t word = (src - rec * batch) * sg.words + j;
    v = *reinterpret_cast<const Word*>(set + rec * set_stride + sg.offset + word * static_cast<int64_t>(sizeof(Word)));
  }
  *reinterpret_cast<Word*>(out + sg.offset + w * static_cast<int64_t>(sizeof(Word))) = v;
}

__global__ __launch_bounds__(kPmThreads) void records_permute_kernel(const char* __restrict__ set, int64_t set_stride,
                                                                     PmSegs segs, int64_t batch, int64_t n,
                                                                     const int64_t* __restrict__ sorted_keys,
                                                                     int64_t first, int64_t count,
                                                                     char* __restrict__ out) {
  const PmSeg sg = segs.s[blockIdx.y];
  const int64_t words = sg.words;
  const int64_t total = batch * words;
  const bool narrow = sg.flags & kSegNarrow, zero = sg.flags & kSegZero, masked = sg.flags & kSegMasked;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kPmThreads;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kPmThreads + threadIdx.x; w < total; w += stride) {
    const int64_t slot = words == 1 ? w : w / words;
    const int64_t j = w - slot * words;
    int64_t src = -1;                                         // padding
    if (!zero && slot < count) {
      src = first + slot;                                     // < n: checked on the host
      if (masked) {
        const int64_t p = static_cast<int64_t>(static_cast<uint64_t>(sorted_keys[src]) & 0xFFFFFFFFull);
        if (p < n) src = p;                                   // whatever the keys hold, no read leaves the set
      }
    }
    if (narrow)
      pm_move<uint32_t>(set, set_stride, sg, batch, src, j, w, out);
    else
      pm_move<uint64_t>(set, set_stride, sg, batch, src, j, w, out);
  }
}

}  // namespace

extern "C" int dfm_permutation_keys(uint64_t seed, int64_t repeat, int64_t n, int64_t* d_keys, dfm_stream_t stream) {
  DFM_REQUIRE(d_keys, "null argument");
  DFM_REQUIRE(n >= 1 && n <= kPmMaxN, "sample count %lld outside [1, 2^31)", (long long)n);
  DFM_REQUIRE(repeat >= 0 && repeat < kPmMaxRepeat, "repeat %lld outside [0, 2^24)", (long long)repeat);
  const uint64_t base = seed * kPmGolden + kPmSalt + (static_cast<uint64_t>(repeat) << 40);
  hipLaunchKernelGGL(permutation_keys_kernel, dim3(blocks_for(n, kPmThreads, 2048)), dim3(kPmThreads), 0,
                     as_stream(stream), base, n, d_keys);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_records_permute(const void* d_set, int64_t set_stride, const dfm_record_field* fields,
                                   int num_fields, int64_t batch_size, int64_t labels_offset, int64_t record_bytes,
                                   int64_t n, const int64_t* d_sorted_keys, uint64_t mask, int64_t first, int64_t count,
                                   void* d_out, dfm_stream_t stream) {
  DFM_REQUIRE(d_set && fields && d_out, "null argument");
  DFM_REQUIRE(num_fields >= 1 && num_fields <= DFM_MAX_FIELDS, "num_fields %d outside [1, %d]", num_fields,
              DFM_MAX_FIELDS);
  DFM_REQUIRE(num_fields == 64 || (mask >> num_fields) == 0, "mask names a field at or above num_fields = %d",
              num_fields);
  DFM_REQUIRE(mask == 0 || d_sorted_keys, "a mask needs the sorted keys");
  DFM_REQUIRE(batch_size >= 1 && batch_size <= kPmMaxBatch, "batch_size %lld outside [1, 2^24]", (long long)batch_size);
  DFM_REQUIRE(n >= 1 && n <= kPmMaxN, "sample count %lld outside [1, 2^31)", (long long)n);
  DFM_REQUIRE(first >= 0 && count >= 1 && count <= batch_size && first <= n - count,
              "samples [%lld, %lld + %lld) outside the set of %lld or more than one batch of %lld", (long long)first,
              (long long)first, (long long)count, (long long)n, (long long)batch_size);
  // the layout RecordLayout gives these kinds and lengths at this batch size; nothing else is accepted, so every
  // segment below lies inside [0, record_bytes) of d_out and of each of the set's records
  const int64_t B = batch_size;
  int ns = 0, nd = 0;
  for (int f = 0; f < num_fields; ++f) {
    const dfm_record_field& fd = fields[f];
    DFM_REQUIRE(fd.kind == DFM_SPARSE || fd.kind == DFM_DENSE || fd.kind == DFM_SEQUENCE, "field %d: kind %d", f, fd.kind);
    DFM_REQUIRE(fd.kind != DFM_SEQUENCE || (fd.max_length >= 1 && fd.max_length <= kPmMaxLength),
                "field %d: max_length %d outside [1, %d]", f, fd.max_length, kPmMaxLength);
    ns += fd.kind == DFM_SPARSE;
    nd += fd.kind == DFM_DENSE;
  }
  const int64_t o1 = (ns > 0 ? ns : 1) * B * 8;
  const int64_t o2 = o1 + (nd > 0 ? nd : 1) * B * 4;
  int64_t end = o2 + B * 4;
  DFM_REQUIRE(labels_offset == o2, "labels_offset %lld is not the layout's %lld", (long long)labels_offset, (long long)o2);
  PmSegs segs;
  int count_segs = 0, si = 0, di = 0;
  int64_t most = B;
  for (int f = 0; f < num_fields; ++f) {
    const dfm_record_field& fd = fields[f];
    int64_t want;
    PmSeg sg{0, 1, static_cast<int32_t>(((mask >> f) & 1) ? kSegMasked : 0)};
    if (fd.kind == DFM_SPARSE) {
      want = 8 * B * si++;
    } else if (fd.kind == DFM_DENSE) {
      want = o1 + 4 * B * di++;
      sg.flags |= kSegNarrow;
    } else {
      want = (end + 15) / 16 * 16;
      end = want + B * fd.max_length * 8;
      sg.words = fd.max_length;
      if (B * sg.words > most) most = B * sg.words;
    }
    DFM_REQUIRE(fd.offset == want, "field %d: offset %lld is not the layout's %lld", f, (long long)fd.offset,
                (long long)want);
    sg.offset = want;
    segs.s[count_segs++] = sg;
  }
  DFM_REQUIRE(record_bytes == end, "record_bytes %lld is not the layout's %lld", (long long)record_bytes, (long long)end);
  segs.s[count_segs++] = PmSeg{o2, 1, kSegNarrow};                            // the labels: never permuted
  if (ns == 0) segs.s[count_segs++] = PmSeg{0, 1, kSegZero};                  // the empty id row
  if (nd == 0) segs.s[count_segs++] = PmSeg{o1, 1, kSegNarrow | kSegZero};    // the empty dense row
  DFM_REQUIRE(set_stride >= record_bytes && set_stride % 16 == 0, "set_stride %lld: a multiple of 16, at least "
              "record_bytes = %lld", (long long)set_stride, (long long)record_bytes);
  DFM_REQUIRE((reinterpret_cast<uintptr_t>(d_set) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0,
              "the set and the output record must be 16-byte aligned");
  hipLaunchKernelGGL(records_permute_kernel, dim3(blocks_for(most, kPmThreads, kPmMaxBlocks), count_segs),
                     dim3(kPmThreads), 0, as_stream(stream), static_cast<const char*>(d_set), set_stride, segs, B, n,
                     d_sorted_keys, first, count, static_cast<char*>(d_out));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
