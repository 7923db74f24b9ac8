// The wavefront scan of the one-wavefront-per-user kernels (interactions.hip: seen_prefix_kernel; history.hip).
#pragma once

#include "common.h"

namespace dfm {

// Inclusive sum over the wavefront; every lane of it is active.
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t up = __shfl_up(v, d, kWave);
    if (lane >= d) v += up;
  }
  return v;
}

}  // namespace dfm
