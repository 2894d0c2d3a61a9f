// Device-side helpers shared by the measurement kernels K7 (k7_measure.hip) and K9 (k9_diameters.hip):
// the relaxed agent-scope accesses to the labelling scratch, wave64 reductions and the bit plane of
// one slice.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nm03/measure.h"

namespace nm03::gpu {
namespace {  // internal to each kernel file, as before the helpers were shared

// Parents and areas are read and written by many threads between barriers: relaxed device-scope
// accesses, which go to L2 where the atomics act (a plain load could be served a stale line).
__device__ __forceinline__ uint32_t ld(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ int32_t wave_min_i32(int32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int32_t wave_max_i32(int32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// One slice's plane: word (y, k) masked to the width, 0 outside the plane.
struct Plane {
  const uint64_t* p;
  int w, h, n;
  __device__ __forceinline__ uint64_t at(int y, int k) const {
    if (y < 0 || y >= h || k < 0 || k >= n) return 0ull;
    return p[(size_t)y * n + k] & row_word_mask(k, w);
  }
  // Column of the first pixel of the run that contains the set pixel (y, x): the position after the
  // highest clear bit below x, walking left through full words (at most n of them).
  __device__ __forceinline__ int run_start(int y, int x) const {
    int k = x >> 6;
    const int b = x & 63;
    uint64_t z = ~at(y, k) & ((b == 63) ? ~0ull : ((2ull << b) - 1ull));
    while (z == 0ull && k > 0) {
      --k;
      z = ~at(y, k);
    }
    return z == 0ull ? 0 : (k << 6) + 64 - __clzll((long long)z);
  }
};

}  // namespace
}  // namespace nm03::gpu
