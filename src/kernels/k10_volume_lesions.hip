// K10 — one record per LESION of the dilated volume (nm03/measure.h VolumeLesion,
// --measure-volume-lesions N): the N largest connected components, largest first.
//
// K10 runs between K8's two passes (launch_volume_measure). After vm_roots_kernel of the mask pass the
// scratch holds the final labelling: every run's slot holds its root, the slot after a root the
// component's voxel count, and a root is the smallest slot of its component, which names its first
// voxel in raster order. The complement pass then overwrites all that; K10 reads it first and writes
// nothing into it. Like K8 it is MULTI-WORKGROUP with the phases as SEPARATE LAUNCHES, a thread per
// word (z, y, k): no grid barrier, no cooperative launch, no flag, no look-back, no spin — a kernel
// boundary is the only thing a phase ever waits for.
//
//   init        accumulators at their identities, candidate counter 0
//   candidates  every root is a key (voxels << 32 | ~slot: more voxels first, then the earlier first
//               voxel; slots are unique, so the keys are a total order). A workgroup picks its own best
//               min(N, roots) keys — rounds of a workgroup maximum, the owner of the winner moving on to
//               its next root — and appends them to the candidate list at a base it takes with ONE
//               atomicAdd. The list holds N keys per workgroup, so it cannot overflow; a lesion among the
//               volume's N best is among its workgroup's N best, so none is lost.
//   select      one workgroup: N rounds of a maximum over the list; a thread keeps the best of its
//               strided share and rescans the share only after it won. The result does not depend on
//               the order in which the workgroups appended. The chosen roots are also written sorted
//               by slot, for the next launch's lookup.
//   accumulate  per word: each stretch reads its run's root (one load: the runs were pointed at their
//               roots), looks it up among the N chosen slots in LDS (binary search) and adds its voxel
//               count, bounding box, coordinate sums and the word's open faces masked to its bits
//               (volume_measure_core.h lesion_bits_figures). The wave sums the lanes of one lesion, reads
//               their samples as K8 does (lane = bit, one coalesced load per word), and adds to the
//               workgroup's table in LDS; the workgroup then issues at most one global atomic per
//               non-zero figure and lesion. Never one atomic per stretch.
//   final       thread j turns accumulator j into record j with plain vector stores (device, pinned or
//               host-mapped memory); the first voxel is the root slot decoded.
//
// Every loop is bounded by the data: the rounds by N, a rescan by the list, the wave rounds by the
// lesions met in the wave (≤ 64), the lookups by log2(N).
#include <hip/hip_runtime.h>

#include <string>

#include "device_util.h"
#include "nm03/kernels.h"
#include "nm03/measure.h"
#include "nm03/volume_measure_core.h"
#include "volume_measure_util.h"

namespace nm03::gpu {

namespace {

constexpr int kVlSelectThreads = 1024;

__device__ __forceinline__ int32_t ext_identity(int j) {
  return j < kLeX1 ? 0x7FFFFFFF : (j == kLeRawMax ? (int32_t)0x80000000 : -1);
}

}  // namespace

__global__ void vl_init_kernel(uint64_t* __restrict__ acc, LesionCtl* __restrict__ ctl) {
  const int t = threadIdx.x;  // one thread per lesion
  if (t < kMaxVolumeLesions) {
    uint64_t* a = acc + (size_t)t * kVlAccWords;
    for (int j = 0; j < kLsNumSums; ++j) a[j] = 0ull;
    int32_t* e = reinterpret_cast<int32_t*>(a + kLsNumSums);
    for (int j = 0; j < kLeNum; ++j) e[j] = ext_identity(j);
  }
  if (t == 0) ctl->candidates = 0u, ctl->count = 0u;
}

__global__ __launch_bounds__(kVmThreads) void vl_candidates_kernel(BitVolume V, uint32_t* __restrict__ scratch, int nmax,
                                                                   LesionCtl* __restrict__ ctl, uint64_t* __restrict__ cand) {
  __shared__ uint64_t sh_best[kVmWaves];
  __shared__ uint32_t sh_cnt[kVmWaves];
  __shared__ uint32_t sh_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
  uint64_t roots = wi.valid ? vmcore::root_bits(V, par, wi.z, wi.y, wi.k) : 0ull;
  const uint32_t wcnt = (uint32_t)wave_sum_u64((uint64_t)vmcore::pop64(roots));
  if (lane == 0) sh_cnt[wave] = wcnt;
  __syncthreads();
  uint32_t total = 0;
  for (int wv = 0; wv < kVmWaves; ++wv) total += sh_cnt[wv];
  const uint32_t take = min((uint32_t)nmax, total);  // the same in every thread of the workgroup
  if (take == 0u) return;
  if (threadIdx.x == 0) sh_base = __hip_atomic_fetch_add(&ctl->candidates, take, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int bit = 0;
  uint64_t my = vmcore::best_root_key(V, par, wi.z, wi.y, wi.k, roots, bit);
  for (uint32_t r = 0; r < take; ++r) {
    const uint64_t wmax = wave_max_u64(my);
    if (lane == 0) sh_best[wave] = wmax;
    __syncthreads();  // also orders sh_base before its first read
    uint64_t best = sh_best[0];
    for (int wv = 1; wv < kVmWaves; ++wv) best = sh_best[wv] > best ? sh_best[wv] : best;
    if (my == best) {  // exactly one thread: keys are unique, and best ≠ 0 while r < total
      cand[(size_t)sh_base + r] = best;
      roots &= ~(1ull << bit);
      my = vmcore::best_root_key(V, par, wi.z, wi.y, wi.k, roots, bit);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kVlSelectThreads) void vl_select_kernel(int nmax, LesionCtl* __restrict__ ctl,
                                                                    const uint64_t* __restrict__ cand) {
  constexpr int kWaves = kVlSelectThreads / 64;
  __shared__ uint64_t sh_best[kWaves];
  __shared__ uint32_t sh_slot[kMaxVolumeLesions];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t total = ctl->candidates;
  const uint32_t count = min((uint32_t)nmax, total);
  // The best key of the thread's share below `bound`.
  auto scan = [&](uint64_t bound) {
    uint64_t b = 0ull;
    for (uint32_t i = threadIdx.x; i < total; i += kVlSelectThreads) {
      const uint64_t c = cand[i];
      if (c < bound && c > b) b = c;
    }
    return b;
  };
  uint64_t my = scan(~0ull);
  for (uint32_t r = 0; r < count; ++r) {
    const uint64_t wmax = wave_max_u64(my);
    if (lane == 0) sh_best[wave] = wmax;
    __syncthreads();
    uint64_t best = sh_best[0];
    for (int wv = 1; wv < kWaves; ++wv) best = sh_best[wv] > best ? sh_best[wv] : best;
    if (my == best) {  // exactly one thread; everything left in its share is smaller
      ctl->sel_slot[r] = vmcore::lesion_key_slot(best);
      ctl->sel_vox[r] = vmcore::lesion_key_area(best);
      sh_slot[r] = vmcore::lesion_key_slot(best);
      my = scan(best);
    }
    __syncthreads();
  }
  if (threadIdx.x < count) {
    const uint32_t s = sh_slot[threadIdx.x];
    uint32_t pos = 0;
    for (uint32_t j = 0; j < count; ++j) pos += sh_slot[j] < s;
    ctl->srt_slot[pos] = s;
    ctl->srt_rank[pos] = threadIdx.x;
  }
  if (threadIdx.x == 0) ctl->count = count;
}

__global__ __launch_bounds__(kVmThreads) void vl_accumulate_kernel(BitVolume V, const uint16_t* __restrict__ raw,
                                                                   uint32_t raw_plane_stride, uint8_t type, uint8_t stored_bits,
                                                                   uint32_t* __restrict__ scratch,
                                                                   const LesionCtl* __restrict__ ctl, uint64_t* __restrict__ acc) {
  __shared__ uint32_t sh_slot[kMaxVolumeLesions], sh_rank[kMaxVolumeLesions];
  __shared__ uint64_t sh_sum[kMaxVolumeLesions][kLsNumSums];
  __shared__ int32_t sh_ext[kMaxVolumeLesions][kLeNum];
  const int lane = threadIdx.x & 63;
  const int count = (int)ctl->count;  // the same in every thread
  if (count == 0) return;
  for (int i = threadIdx.x; i < count * kLsNumSums; i += kVmThreads) {
    sh_sum[i / kLsNumSums][i % kLsNumSums] = 0ull;
    sh_ext[i / kLeNum][i % kLeNum] = ext_identity(i % kLeNum);
  }
  if ((int)threadIdx.x < count) sh_slot[threadIdx.x] = ctl->srt_slot[threadIdx.x], sh_rank[threadIdx.x] = ctl->srt_rank[threadIdx.x];
  __syncthreads();
  // One lesion's figures into the workgroup's table (LDS atomics: four waves at most meet there).
  auto table_add = [&](int rank, const uint64_t (&s)[kLsNumSums], const int32_t (&e)[kLeNum]) {
#pragma unroll
    for (int j = 0; j < kLsNumSums; ++j)
      if (s[j]) (void)__hip_atomic_fetch_add(&sh_sum[rank][j], s[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
    for (int j = 0; j < kLeNum; ++j) {
      if (j < kLeX1)
        (void)__hip_atomic_fetch_min(&sh_ext[rank][j], e[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      else
        (void)__hip_atomic_fetch_max(&sh_ext[rank][j], e[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  };
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
  const uint64_t m = wi.valid ? V.at(wi.z, wi.y, wi.k) : 0ull;
  const uint32_t row_off =
      wi.valid ? (uint32_t)wi.z * raw_plane_stride + (uint32_t)wi.y * (uint32_t)V.w + (uint32_t)(wi.k << 6) : 0u;
  vmcore::WordFaces wf = {};
  if (m) wf = vmcore::word_faces(V, wi.z, wi.y, wi.k, m);
  // The thread's stretches of chosen lesions: those of one lesion are gathered in `bits`; a stretch of
  // ANOTHER chosen lesion in the same word (rare) sends the gathered ones to the table at once, with
  // their samples read by the thread itself.
  int cur = -1;
  uint64_t bits = 0ull;
  if (m)
    vmcore::lesion_stretches(V, par, wi.z, wi.y, wi.k, m, [&](uint32_t root, uint64_t sbits) {
      const int idx = vmcore::find_slot(sh_slot, count, root);
      if (idx < 0) return;
      const int rank = (int)sh_rank[idx];
      if (bits && rank != cur) {
        vmcore::LesionFigures f;
        vmcore::lesion_bits_figures(wi.z, wi.y, wi.k, wf, bits, f);
        int64_t rs = 0;
        int32_t r0 = 0x7FFFFFFF, r1 = (int32_t)0x80000000;
        for (uint64_t t = bits; t; t &= t - 1) {
          const int32_t v = stored_sample(raw[(size_t)row_off + (size_t)vmcore::ctz64(t)], type, stored_bits);
          rs += v;
          r0 = min(r0, v);
          r1 = max(r1, v);
        }
        const uint64_t s[kLsNumSums] = {f.vox, f.sum_x, f.sum_y, f.sum_z, f.faces_x, f.faces_y, f.faces_z, (uint64_t)rs};
        const int32_t e[kLeNum] = {f.x0, f.y0, f.z0, r0, f.x1, f.y1, f.z1, r1};
        table_add(cur, s, e);
        bits = 0ull;
      }
      cur = rank;
      bits |= sbits;
    });
  vmcore::LesionFigures f;
  if (bits) vmcore::lesion_bits_figures(wi.z, wi.y, wi.k, wf, bits, f);
  // Then by the wave: the first pending lane's lesion, every lane of that lesion summed, one update of
  // the table. At most `count` rounds; a wave inside one body takes one.
  for (uint64_t pending = __ballot(bits != 0ull); pending;) {
    const int leader = __ffsll((long long)pending) - 1;
    const int rank = __shfl(cur, leader, 64);
    const bool mine = bits != 0ull && cur == rank;
    const uint64_t members = __ballot(mine);
    // Samples: the members' words in turn, lane = bit, one coalesced 128-byte load each.
    int64_t rs = 0;
    int32_t r0 = 0x7FFFFFFF, r1 = (int32_t)0x80000000;
    for (uint64_t act = members; act; act &= act - 1) {
      const int j = __ffsll((long long)act) - 1;
      const uint64_t mj = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(bits >> 32), j, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)bits, j, 64);
      const uint32_t oj = (uint32_t)__shfl((int)row_off, j, 64);
      if ((mj >> lane) & 1ull) {
        const int32_t v = stored_sample(raw[(size_t)oj + (size_t)lane], type, stored_bits);
        rs += v;
        r0 = min(r0, v);
        r1 = max(r1, v);
      }
    }
    const vmcore::LesionFigures none;
    const vmcore::LesionFigures& g = mine ? f : none;
    const uint64_t s[kLsNumSums] = {wave_sum_u64(g.vox),     wave_sum_u64(g.sum_x),   wave_sum_u64(g.sum_y),
                                    wave_sum_u64(g.sum_z),   wave_sum_u64(g.faces_x), wave_sum_u64(g.faces_y),
                                    wave_sum_u64(g.faces_z), wave_sum_u64((uint64_t)rs)};
    const int32_t e[kLeNum] = {wave_min_i32(g.x0), wave_min_i32(g.y0), wave_min_i32(g.z0), wave_min_i32(r0),
                               wave_max_i32(g.x1), wave_max_i32(g.y1), wave_max_i32(g.z1), wave_max_i32(r1)};
    if (lane == leader) table_add(rank, s, e);
    pending &= ~members;
  }
  __syncthreads();
  // One atomic per non-zero figure, lesion and workgroup; a lesion the workgroup did not meet adds nothing.
  for (int i = threadIdx.x; i < count * kVlAccWords; i += kVmThreads) {
    const int rank = i / kVlAccWords, j = i % kVlAccWords;
    uint64_t* a = acc + (size_t)rank * kVlAccWords;
    if (j < kLsNumSums) {
      const uint64_t v = sh_sum[rank][j];
      if (v) (void)__hip_atomic_fetch_add(a + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (j < kLsNumSums + kLeNum) {
      const int k = j - kLsNumSums;
      const int32_t v = sh_ext[rank][k];
      int32_t* e = reinterpret_cast<int32_t*>(a + kLsNumSums);
      if (v == ext_identity(k)) continue;
      if (k < kLeX1)
        (void)__hip_atomic_fetch_min(e + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else
        (void)__hip_atomic_fetch_max(e + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void vl_final_kernel(BitVolume V, int nmax, const LesionCtl* __restrict__ ctl, const uint64_t* __restrict__ acc,
                                VolumeLesion* __restrict__ out, uint32_t* __restrict__ out_count) {
  const int t = threadIdx.x;  // one thread per record
  const int count = (int)ctl->count;
  if (t == 0) *out_count = (uint32_t)count;
  if (t >= nmax) return;
  VolumeLesion r = {};
  if (t < count) {
    const uint64_t* a = acc + (size_t)t * kVlAccWords;
    const int32_t* e = reinterpret_cast<const int32_t*>(a + kLsNumSums);
    r.voxels = a[kLsVox];
    vmcore::slot_voxel(V, ctl->sel_slot[t], r.first);
    for (int j = 0; j < 3; ++j) r.bbox[j] = e[kLeX0 + j], r.bbox[3 + j] = e[kLeX1 + j];
    r.sum_x = a[kLsSumX], r.sum_y = a[kLsSumY], r.sum_z = a[kLsSumZ];
    r.faces_x = a[kLsFacesX], r.faces_y = a[kLsFacesY], r.faces_z = a[kLsFacesZ];
    r.raw_sum = (int64_t)a[kLsRawSum];
    r.raw_min = e[kLeRawMin];
    r.raw_max = e[kLeRawMax];
  }
  out[t] = r;
}

namespace {
uint32_t word_grid(int w, int h, int d) {
  const uint64_t words = (uint64_t)((w + 63) / 64) * (uint64_t)h * (uint64_t)d;
  return (uint32_t)((words + kVmThreads - 1) / kVmThreads);
}
}  // namespace

size_t volume_lesions_work_bytes(int w, int h, int d, int max_lesions) {
  if (w <= 0 || h <= 0 || d <= 0 || max_lesions < 1 || max_lesions > kMaxVolumeLesions) return 0;
  return kVlCandOffset + (size_t)word_grid(w, h, d) * (size_t)max_lesions * sizeof(uint64_t);
}

void launch_volume_lesions(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d,
                           uint8_t type, uint8_t stored_bits, const uint32_t* scratch, const VolumeLesionWork& lesions,
                           hipStream_t stream) {
  if (lesions.max_lesions < 1 || lesions.max_lesions > kMaxVolumeLesions)
    throw DeviceError("launch_volume_lesions: lesions must be 1.." + std::to_string(kMaxVolumeLesions));
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("launch_volume_lesions: empty volume");
  if (stored_bits < 1 || stored_bits > 16) throw DeviceError("launch_volume_lesions: stored bits must be 1..16");
  if (volume_measure_scratch_words(w, h, d) == 0 || raw_plane_stride < (size_t)w * (size_t)h ||
      raw_plane_stride * (size_t)d > 0xFFFFFFFFull)
    throw DeviceError("launch_volume_lesions: a " + std::to_string(w) + " x " + std::to_string(h) + " x " +
                      std::to_string(d) + " volume is too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
  if (!dilated || !raw || !scratch || !lesions.work || !lesions.out || !lesions.out_count)
    throw DeviceError("launch_volume_lesions: null buffer");
  const int n = (w + 63) / 64, nmax = lesions.max_lesions;
  const uint32_t grid = word_grid(w, h, d);
  const BitVolume M{dilated, w, h, d, n, false};
  uint8_t* base = static_cast<uint8_t*>(lesions.work);
  uint64_t* acc = reinterpret_cast<uint64_t*>(base);
  LesionCtl* ctl = reinterpret_cast<LesionCtl*>(base + kVlAccBytes);
  uint64_t* cand = reinterpret_cast<uint64_t*>(base + kVlCandOffset);
  uint32_t* labels = const_cast<uint32_t*>(scratch);  // read only: DeviceParents' loads take a plain pointer
  vl_init_kernel<<<1, 64, 0, stream>>>(acc, ctl);
  check_launch("vl_init_kernel");
  vl_candidates_kernel<<<grid, kVmThreads, 0, stream>>>(M, labels, nmax, ctl, cand);
  check_launch("vl_candidates_kernel");
  vl_select_kernel<<<1, kVlSelectThreads, 0, stream>>>(nmax, ctl, cand);
  check_launch("vl_select_kernel");
  vl_accumulate_kernel<<<grid, kVmThreads, 0, stream>>>(M, raw, (uint32_t)raw_plane_stride, type, stored_bits, labels, ctl, acc);
  check_launch("vl_accumulate_kernel");
  vl_final_kernel<<<1, 64, 0, stream>>>(M, nmax, ctl, acc, lesions.out, lesions.out_count);
  check_launch("vl_final_kernel");
}

void preload_volume_lesions() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&vl_init_kernel), reinterpret_cast<const void*>(&vl_candidates_kernel),
                        reinterpret_cast<const void*>(&vl_select_kernel), reinterpret_cast<const void*>(&vl_accumulate_kernel),
                        reinterpret_cast<const void*>(&vl_final_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume lesion kernels");
}

}  // namespace nm03::gpu
