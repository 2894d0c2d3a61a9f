// Device-side helpers shared by the measurement kernels K7 (k7_measure.hip), K9 (k9_diameters.hip), K11
// (k11_intensity.hip) and K12 (k12_texture.hip): the relaxed agent-scope accesses to the labelling
// scratch, wave64 reductions, the bit plane of one slice, and K11's and K12's sample walk and
// wave-combining LDS histogram add.
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

constexpr int kPeelRounds = 3;

// hist[key] += 1 for every lane with `on`, equal keys combined in the wave (k11_intensity.hip: "Bin contention").
// Called by all 64 lanes of a wave together.
// `give_up`: stop combining after a round that matched fewer than a quarter of the remaining lanes — the
// keys are spread, further rounds would cost more instructions than the adds they save (K12, whose
// pair cells of textured content rarely repeat within a word, calls it up to 13 times a word).
__device__ __forceinline__ void wave_hist_add(uint32_t* hist, uint32_t key, bool on, int lane, bool give_up = false) {
  uint64_t rest = __ballot(on);
#pragma unroll
  for (int r = 0; r < kPeelRounds; ++r) {
    if (rest == 0ull) return;  // uniform over the wave
    const int lead = __ffsll((long long)rest) - 1;
    const uint32_t k = (uint32_t)__shfl((int)key, lead, 64);
    const uint64_t same = __ballot(on && key == k) & rest;
    if (lane == lead) atomicAdd(hist + k, (uint32_t)__popcll(same));
    const bool spread = give_up && 4 * __popcll(same) < __popcll(rest);  // uniform
    rest &= ~same;
    if (spread) break;
  }
  if ((rest >> lane) & 1ull) atomicAdd(hist + key, 1u);
}

// The wave's non-empty words in turn, lane = bit: f(on, stored bits) for every lane, four words a round.
// `m`: the lane's own word (0 for none), `off`: the sample offset of its first pixel.
template <class F>
__device__ __forceinline__ void walk_samples(uint64_t m, uint32_t off, const uint16_t* __restrict__ px, int lane, F&& f) {
  for (uint64_t act = __ballot(m != 0ull); act;) {
    uint64_t mj[4];
    uint32_t oj[4];
    uint16_t rv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      mj[u] = 0ull;
      oj[u] = 0u;
      if (act) {
        const int j = __ffsll((long long)act) - 1;
        act &= act - 1;
        mj[u] = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(m >> 32), j, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)m, j, 64);
        oj[u] = (uint32_t)__shfl((int)off, j, 64);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) rv[u] = ((mj[u] >> lane) & 1ull) ? px[(size_t)oj[u] + (size_t)lane] : (uint16_t)0;
#pragma unroll
    for (int u = 0; u < 4; ++u) f(((mj[u] >> lane) & 1ull) != 0ull, rv[u]);
  }
}

}  // namespace
}  // namespace nm03::gpu
