// Device-side helpers shared by the volume measurement kernels K8 (k8_volume_measure.hip), K10
// (k10_volume_lesions.hip) and K13 (k13_volume_diameters.hip): the relaxed agent-scope accesses to the run
// union-find's scratch, wave64 reductions, the thread-per-word mapping and the layout of K10's work buffer.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"
#include "nm03/volume_measure_core.h"

namespace nm03::gpu {

constexpr int kVmThreads = 256;
constexpr int kVmWaves = kVmThreads / 64;

namespace {  // internal to each kernel file, as before the helpers were shared

using vmcore::BitVolume;

// Parents, areas and marks: relaxed agent-scope atomics (see K8's header comment).
struct DeviceParents {
  uint32_t* p;
  __device__ __forceinline__ uint32_t ld(uint32_t i) const {
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void st(uint32_t i, uint32_t v) const {
    __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ uint32_t fetch_min(uint32_t i, uint32_t v) const {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void add(uint32_t i, uint32_t v) const {
    (void)__hip_atomic_fetch_add(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    const uint64_t t = ((uint64_t)hi << 32) | lo;
    v = t > v ? t : v;
  }
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

// The thread's word: (z, y, k) of word i < total.
struct WordIndex {
  int z, y, k;
  bool valid;
};
__device__ __forceinline__ WordIndex my_word(const BitVolume& V) {
  const uint32_t total = (uint32_t)V.d * (uint32_t)V.h * (uint32_t)V.n;  // < 2^32 (launch_volume_measure)
  const uint32_t i = blockIdx.x * (uint32_t)kVmThreads + threadIdx.x;
  WordIndex w;
  w.valid = i < total;
  const uint32_t row = i / (uint32_t)V.n;
  w.k = (int)(i - row * (uint32_t)V.n);
  w.z = (int)(row / (uint32_t)V.h);
  w.y = (int)(row - (uint32_t)w.z * (uint32_t)V.h);
  return w;
}

// ---- K10's work buffer, read by K13 (k13_volume_diameters.hip) as well: the accumulators, then the control
// words and the chosen roots, then the candidate list.
constexpr int kVlAccWords = 16;  // u64 per lesion: 8 sums, then 8 i32 extrema, then unused

// Sums: u64 index in a lesion's accumulator. Extrema: i32 index after the sums — minima, then maxima.
enum : int { kLsVox = 0, kLsSumX, kLsSumY, kLsSumZ, kLsFacesX, kLsFacesY, kLsFacesZ, kLsRawSum, kLsNumSums };
enum : int { kLeX0 = 0, kLeY0, kLeZ0, kLeRawMin, kLeX1, kLeY1, kLeZ1, kLeRawMax, kLeNum };
static_assert(kLsNumSums == 8 && kLeNum == 8 && kLsNumSums + kLeNum / 2 <= kVlAccWords, "lesion accumulator layout");

// Control words and the chosen roots, after the accumulators in the work buffer.
struct LesionCtl {
  uint32_t candidates;  // keys in the candidate list
  uint32_t count;       // reported lesions, min(N, components)
  uint32_t pad[14];
  uint32_t sel_slot[kMaxVolumeLesions], sel_vox[kMaxVolumeLesions];  // in rank order
  uint32_t srt_slot[kMaxVolumeLesions], srt_rank[kMaxVolumeLesions];  // the same roots ascending by slot, and their rank
};

constexpr size_t kVlAccBytes = (size_t)kMaxVolumeLesions * kVlAccWords * sizeof(uint64_t);
constexpr size_t kVlCandOffset = kVlAccBytes + sizeof(LesionCtl);
static_assert(kVlCandOffset % 8 == 0, "candidate list alignment");

}  // namespace
}  // namespace nm03::gpu
