// K18 — lesion-wise detection scores for two bit volumes of one frame (nm03/volume_compare_lesions.h,
// --compare-lesions N): which components of each mask meet which of the other, for ALL components, and the N largest
// of each side in detail.
//
// Like K8 it is MULTI-WORKGROUP with the phases as SEPARATE LAUNCHES on the volume's stream, a thread per word
// (z, y, k): no cooperative launch, no grid barrier, no flag, no look-back, no spin — a kernel boundary is the only
// thing a phase ever waits for. Launches that do the same for each mask take both in one grid (blockIdx.y = the
// side). Ten launches:
//
//   init        the control block: candidate counters, totals and the global table, all 0
//   runs        both masks: every run's parent = itself, area = 0 (vmcore::init_runs)
//   unions      both masks: K8's union-find at the connectivity asked for (vmcore::unite_word, relaxed agent-scope
//               atomics, see K8's header comment for why that is enough)
//   compress    both masks: every run pointed straight at its root (vmcore::compress_runs); the roots are final, so
//               the same thread also sets the SIDE DATA of the roots that start in its word: overlap counter 0,
//               partner cell 0 (vclcore::init_side). The roots' own slots are never written by this launch.
//   areas       both masks: every in-word stretch adds its length at its root, those of one root summed in the wave
//               first (vmcore::stretch_areas, as vm_areas_kernel)
//   candidates  both masks: every workgroup's N best lesion keys into the side's candidate list at a base taken with
//               ONE atomicAdd (K10's scheme: N keys per workgroup, so the list cannot overflow)
//   select      one workgroup per side: N rounds of a maximum; the chosen roots in rank order and sorted by slot
//   join        a thread per word takes every in-word stretch of A ∧ B (vclcore::join_stretches): both roots (one
//               load each), then length to both overlap counters, both partner cells (atomicCAS, at most two changes
//               per cell, a settled cell is only read), and the cell (rank of A's root or N, rank of B's root or N)
//               of the workgroup's LDS table of (64 + 1)² u32 = 16.9 KB. The stretches of one (A root, B root) pair
//               are summed by the thread, then by the wave — one large overlapping body costs one round of global
//               atomics per wave, not one per stretch. The workgroup flushes with at most one global u64 atomic per
//               non-zero cell. Grid: min(ceil(words / 256), 1024 or max_blocks) workgroups striding over the
//               256-word blocks.
//   count       both masks: the roots that start in a word — lesions, those with an overlap (hit), those whose
//               partner cell says several (multi) — reduced in the wave, then through LDS, then one atomic per
//               figure and workgroup
//   final       ONE workgroup writes the head, the 2 · N lesion records (zero past the reported count) and the table
//               with plain vector stores (device, pinned or host-mapped memory)
//
// WORK BUFFER: per mask a u32 labelling and a u32 side-data array of K8's layout ((w + 1)·h·d + 1 slots each) —
// 16 bytes per slot for both masks — then the 35 KiB control block and the two candidate lists (N keys per
// workgroup: at most 2 more bytes per slot). Within the 24 bytes per slot the design allows.
//
// Every loop is bounded by the data: K8's finds and unions, the rounds by N, a rescan by the list, the wave rounds by
// the pairs met in the wave (≤ 64), the lookups by log2(N), a partner cell's transitions by two.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "device_util.h"
#include "nm03/kernels.h"
#include "nm03/measure.h"
#include "nm03/volume_compare_lesions.h"
#include "nm03/volume_compare_lesions_core.h"
#include "nm03/volume_measure_core.h"
#include "volume_measure_util.h"

namespace nm03::gpu {

namespace {

constexpr int kClSelectThreads = 1024;
constexpr uint32_t kClMaxBlocks = 1024;  // workgroups of the join: each flushes its table once
constexpr int kClStrideMax = kMaxVolumeLesions + 1;
constexpr int kClCells = kClStrideMax * kClStrideMax;
constexpr int kClFinalThreads = 256;
static_assert(kClFinalThreads >= 2 * kMaxVolumeLesions, "a thread per record");

// The side data: relaxed agent-scope atomics, as the labelling (K8's header comment).
struct DeviceSide {
  uint32_t* p;
  __device__ __forceinline__ uint32_t ld(uint32_t i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void st(uint32_t i, uint32_t v) const {
    __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void add(uint32_t i, uint32_t v) const {
    (void)__hip_atomic_fetch_add(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ uint32_t cas(uint32_t i, uint32_t expected, uint32_t desired) const {
    (void)__hip_atomic_compare_exchange_strong(p + i, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expected;  // the old value, whether the exchange happened or not
  }
};

// Both masks of a launch; blockIdx.y picks one.
struct ClSides {
  BitVolume V[2];
  uint32_t* labels[2];
  uint32_t* side[2];
};

struct ClSideCtl {
  uint32_t candidates;  // keys in the candidate list
  uint32_t count;       // reported lesions, min(N, components)
  uint32_t lesions, hit, multi;
  uint32_t pad[11];
  uint32_t sel_slot[kMaxVolumeLesions], sel_vox[kMaxVolumeLesions];   // in rank order
  uint32_t srt_slot[kMaxVolumeLesions], srt_rank[kMaxVolumeLesions];  // the same roots ascending by slot, and their rank
};

struct ClCtl {
  ClSideCtl side[2];
  uint64_t table[kClCells];  // the first (N + 1)² cells, row (A) major with stride N + 1
};
static_assert(sizeof(ClCtl) % 8 == 0 && offsetof(ClCtl, table) % 8 == 0, "control block layout");

__device__ __forceinline__ WordIndex word_at_index(const BitVolume& V, uint32_t i) {
  const uint32_t total = (uint32_t)V.d * (uint32_t)V.h * (uint32_t)V.n;
  WordIndex w;
  w.valid = i < total;
  const uint32_t row = i / (uint32_t)V.n;
  w.k = (int)(i - row * (uint32_t)V.n);
  w.z = (int)(row / (uint32_t)V.h);
  w.y = (int)(row - (uint32_t)w.z * (uint32_t)V.h);
  return w;
}

}  // namespace

__global__ __launch_bounds__(kVmThreads) void cl_init_kernel(ClCtl* __restrict__ ctl) {
  uint32_t* w = reinterpret_cast<uint32_t*>(ctl);
  const uint32_t n = (uint32_t)(sizeof(ClCtl) / 4);
  for (uint32_t i = blockIdx.x * (uint32_t)kVmThreads + threadIdx.x; i < n; i += gridDim.x * (uint32_t)kVmThreads) w[i] = 0u;
}

__global__ __launch_bounds__(kVmThreads) void cl_runs_kernel(ClSides S) {
  const int s = (int)blockIdx.y;
  const BitVolume V = s ? S.V[1] : S.V[0];
  const WordIndex wi = my_word(V);
  DeviceParents par{s ? S.labels[1] : S.labels[0]};
  if (wi.valid) vmcore::init_runs(V, wi.z, wi.y, wi.k, par);
}

__global__ __launch_bounds__(kVmThreads) void cl_unions_kernel(ClSides S, int conn26) {
  const int s = (int)blockIdx.y;
  const BitVolume V = s ? S.V[1] : S.V[0];
  const WordIndex wi = my_word(V);
  DeviceParents par{s ? S.labels[1] : S.labels[0]};
  if (wi.valid) vmcore::unite_word(V, par, wi.z, wi.y, wi.k, conn26 != 0);
}

__global__ __launch_bounds__(kVmThreads) void cl_compress_kernel(ClSides S) {
  const int s = (int)blockIdx.y;
  const BitVolume V = s ? S.V[1] : S.V[0];
  const WordIndex wi = my_word(V);
  DeviceParents par{s ? S.labels[1] : S.labels[0]};
  DeviceSide side{s ? S.side[1] : S.side[0]};
  if (wi.valid) {
    vmcore::compress_runs(V, par, wi.z, wi.y, wi.k);
    vclcore::init_side(V, par, side, wi.z, wi.y, wi.k);
  }
}

__global__ __launch_bounds__(kVmThreads) void cl_areas_kernel(ClSides S) {
  const int lane = threadIdx.x & 63;
  const int s = (int)blockIdx.y;
  const BitVolume V = s ? S.V[1] : S.V[0];
  const WordIndex wi = my_word(V);
  DeviceParents par{s ? S.labels[1] : S.labels[0]};
  // The thread's stretches, those of one root summed; a stretch of another root flushes the sum.
  uint32_t root = 0, len = 0;
  if (wi.valid)
    vmcore::stretch_areas(V, par, wi.z, wi.y, wi.k, [&](uint32_t r, uint32_t n) {
      if (len && r != root) {
        par.add(root + 1u, len);
        len = 0;
      }
      root = r;
      len += n;
    });
  // Then by the wave: the first pending lane's root, every lane with that root summed, one atomic.
  for (uint64_t pending = __ballot(len != 0u); pending;) {
    const int leader = __ffsll((long long)pending) - 1;
    const uint32_t r = (uint32_t)__shfl((int)root, leader, 64);
    const bool mine = len != 0u && root == r;
    const uint32_t sum = (uint32_t)wave_sum_u64(mine ? len : 0u);
    if (lane == leader) par.add(r + 1u, sum);
    pending &= ~__ballot(mine);
  }
}

__global__ __launch_bounds__(kVmThreads) void cl_candidates_kernel(ClSides S, int nmax, ClCtl* __restrict__ ctl, uint64_t* __restrict__ cand_a,
                                                                   uint64_t* __restrict__ cand_b) {
  __shared__ uint64_t sh_best[kVmWaves];
  __shared__ uint32_t sh_cnt[kVmWaves];
  __shared__ uint32_t sh_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = (int)blockIdx.y;
  const BitVolume V = s ? S.V[1] : S.V[0];
  uint64_t* cand = s ? cand_b : cand_a;
  ClSideCtl* sc = &ctl->side[s];
  const WordIndex wi = my_word(V);
  DeviceParents par{s ? S.labels[1] : S.labels[0]};
  uint64_t roots = wi.valid ? vmcore::root_bits(V, par, wi.z, wi.y, wi.k) : 0ull;
  const uint32_t wcnt = (uint32_t)wave_sum_u64((uint64_t)vmcore::pop64(roots));
  if (lane == 0) sh_cnt[wave] = wcnt;
  __syncthreads();
  uint32_t total = 0;
  for (int wv = 0; wv < kVmWaves; ++wv) total += sh_cnt[wv];
  const uint32_t take = min((uint32_t)nmax, total);  // the same in every thread of the workgroup
  if (take == 0u) return;
  if (threadIdx.x == 0) sh_base = __hip_atomic_fetch_add(&sc->candidates, take, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// One workgroup per side (blockIdx.x).
__global__ __launch_bounds__(kClSelectThreads) void cl_select_kernel(int nmax, ClCtl* __restrict__ ctl, const uint64_t* __restrict__ cand_a,
                                                                    const uint64_t* __restrict__ cand_b) {
  constexpr int kWaves = kClSelectThreads / 64;
  __shared__ uint64_t sh_best[kWaves];
  __shared__ uint32_t sh_slot[kMaxVolumeLesions];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t* cand = blockIdx.x ? cand_b : cand_a;
  ClSideCtl* sc = &ctl->side[blockIdx.x];
  const uint32_t total = sc->candidates;
  const uint32_t count = min((uint32_t)nmax, total);
  // The best key of the thread's share below `bound`.
  auto scan = [&](uint64_t bound) {
    uint64_t b = 0ull;
    for (uint32_t i = threadIdx.x; i < total; i += kClSelectThreads) {
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
      sc->sel_slot[r] = vmcore::lesion_key_slot(best);
      sc->sel_vox[r] = vmcore::lesion_key_area(best);
      sh_slot[r] = vmcore::lesion_key_slot(best);
      my = scan(best);
    }
    __syncthreads();
  }
  if (threadIdx.x < count) {
    const uint32_t s = sh_slot[threadIdx.x];
    uint32_t pos = 0;
    for (uint32_t j = 0; j < count; ++j) pos += sh_slot[j] < s;
    sc->srt_slot[pos] = s;
    sc->srt_rank[pos] = threadIdx.x;
  }
  if (threadIdx.x == 0) sc->count = count;
}

__global__ __launch_bounds__(kVmThreads) void cl_join_kernel(ClSides S, uint32_t nblocks, int nmax, ClCtl* __restrict__ ctl) {
  __shared__ uint32_t sh_slot[2][kMaxVolumeLesions], sh_rank[2][kMaxVolumeLesions];
  __shared__ uint32_t sh_table[kClCells];
  const int lane = threadIdx.x & 63;
  const int stride = nmax + 1, cells = stride * stride;
  const int count_a = (int)ctl->side[0].count, count_b = (int)ctl->side[1].count;  // the same in every thread
  for (int i = threadIdx.x; i < cells; i += kVmThreads) sh_table[i] = 0u;
  if ((int)threadIdx.x < count_a) sh_slot[0][threadIdx.x] = ctl->side[0].srt_slot[threadIdx.x], sh_rank[0][threadIdx.x] = ctl->side[0].srt_rank[threadIdx.x];
  if ((int)threadIdx.x < count_b) sh_slot[1][threadIdx.x] = ctl->side[1].srt_slot[threadIdx.x], sh_rank[1][threadIdx.x] = ctl->side[1].srt_rank[threadIdx.x];
  __syncthreads();
  DeviceParents para{S.labels[0]}, parb{S.labels[1]};
  DeviceSide sa{S.side[0]}, sb{S.side[1]};
  // n voxels shared by the components at roots ra (of A) and rb (of B).
  auto apply = [&](uint32_t ra, uint32_t rb, uint32_t n) {
    sa.add(ra, n);
    sb.add(rb, n);
    vclcore::partner_update(sa, ra, rb);
    vclcore::partner_update(sb, rb, ra);
    const int ia = vclcore::lesion_rank(sh_slot[0], sh_rank[0], count_a, ra, nmax);
    const int ib = vclcore::lesion_rank(sh_slot[1], sh_rank[1], count_b, rb, nmax);
    (void)__hip_atomic_fetch_add(&sh_table[ia * stride + ib], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  for (uint32_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {  // the same trips for every wave (ballots inside)
    const WordIndex wi = word_at_index(S.V[0], blk * (uint32_t)kVmThreads + threadIdx.x);
    // The thread's stretches, those of one pair of roots summed; a stretch of another pair flushes the sum.
    uint32_t ra = 0, rb = 0, len = 0;
    if (wi.valid)
      vclcore::join_stretches(S.V[0], S.V[1], para, parb, wi.z, wi.y, wi.k, [&](uint32_t qa, uint32_t qb, uint32_t n) {
        if (len && (qa != ra || qb != rb)) {
          apply(ra, rb, len);
          len = 0;
        }
        ra = qa, rb = qb;
        len += n;
      });
    // Then by the wave: the first pending lane's pair, every lane with that pair summed, one lane applies.
    for (uint64_t pending = __ballot(len != 0u); pending;) {
      const int leader = __ffsll((long long)pending) - 1;
      const uint32_t qa = (uint32_t)__shfl((int)ra, leader, 64), qb = (uint32_t)__shfl((int)rb, leader, 64);
      const bool mine = len != 0u && ra == qa && rb == qb;
      const uint32_t sum = (uint32_t)wave_sum_u64(mine ? len : 0u);
      if (lane == leader) apply(qa, qb, sum);
      pending &= ~__ballot(mine);
    }
  }
  __syncthreads();
  // At most one global atomic per non-zero cell and workgroup.
  for (int i = threadIdx.x; i < cells; i += kVmThreads) {
    const uint32_t v = sh_table[i];
    if (v) (void)__hip_atomic_fetch_add(ctl->table + i, (uint64_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kVmThreads) void cl_count_kernel(ClSides S, ClCtl* __restrict__ ctl) {
  __shared__ uint32_t sh[3][kVmWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = (int)blockIdx.y;
  const BitVolume V = s ? S.V[1] : S.V[0];
  const WordIndex wi = my_word(V);
  DeviceParents par{s ? S.labels[1] : S.labels[0]};
  DeviceSide side{s ? S.side[1] : S.side[0]};
  uint32_t lesions = 0, hit = 0, multi = 0;
  if (wi.valid) vclcore::count_side(V, par, side, wi.z, wi.y, wi.k, lesions, hit, multi);
  lesions = (uint32_t)wave_sum_u64(lesions);
  hit = (uint32_t)wave_sum_u64(hit);
  multi = (uint32_t)wave_sum_u64(multi);
  if (lane == 0) sh[0][wave] = lesions, sh[1][wave] = hit, sh[2][wave] = multi;
  __syncthreads();
  if (threadIdx.x < 3) {
    uint32_t t = 0;
    for (int wv = 0; wv < kVmWaves; ++wv) t += sh[threadIdx.x][wv];
    uint32_t* dst = threadIdx.x == 0 ? &ctl->side[s].lesions : threadIdx.x == 1 ? &ctl->side[s].hit : &ctl->side[s].multi;
    if (t) (void)__hip_atomic_fetch_add(dst, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One workgroup: thread j < 64 writes record j of A, thread 64 + j record j of B.
__global__ __launch_bounds__(kClFinalThreads) void cl_final_kernel(ClSides S, int nmax, int connectivity, const ClCtl* __restrict__ ctl,
                                                                  uint8_t* __restrict__ out) {
  const int stride = nmax + 1, cells = stride * stride;
  auto* head = reinterpret_cast<VolumeCompareLesionsHead*>(out);
  auto* recs = reinterpret_cast<VolumeCompareLesion*>(out + sizeof(VolumeCompareLesionsHead));
  auto* table = reinterpret_cast<uint64_t*>(out + sizeof(VolumeCompareLesionsHead) + 2 * (size_t)nmax * sizeof(VolumeCompareLesion));
  const int count_a = (int)ctl->side[0].count, count_b = (int)ctl->side[1].count;
  if (threadIdx.x == 0) {
    VolumeCompareLesionsHead hd = {};
    hd.connectivity = (uint32_t)connectivity, hd.max_lesions = (uint32_t)nmax;
    hd.lesions_a = ctl->side[0].lesions, hd.hit_a = ctl->side[0].hit, hd.multi_a = ctl->side[0].multi;
    hd.lesions_b = ctl->side[1].lesions, hd.hit_b = ctl->side[1].hit, hd.multi_b = ctl->side[1].multi;
    hd.reported_a = (uint32_t)count_a, hd.reported_b = (uint32_t)count_b;
    *head = hd;
  }
  const int s = (int)threadIdx.x >> 6, j = (int)threadIdx.x & 63;
  if (s < 2 && j < nmax) {
    VolumeCompareLesion r = {};
    const ClSideCtl& sc = ctl->side[s];
    if (j < (s ? count_b : count_a)) {
      const uint32_t slot = sc.sel_slot[j];
      const uint32_t* side = s ? S.side[1] : S.side[0];
      const BitVolume V = s ? S.V[1] : S.V[0];
      r = s ? vclcore::lesion_record(V, slot, sc.sel_vox[j], side[slot], side[slot + 1u], ctl->table + j, stride, count_a, nmax)
            : vclcore::lesion_record(V, slot, sc.sel_vox[j], side[slot], side[slot + 1u], ctl->table + (size_t)j * stride, 1, count_b, nmax);
    }
    recs[(size_t)s * nmax + j] = r;
  }
  for (int i = threadIdx.x; i < cells; i += kClFinalThreads) table[i] = ctl->table[i];
}

namespace {

struct ClLayout {
  size_t slots = 0;
  uint32_t grid = 0;
  size_t off_labels[2], off_side[2], off_ctl, off_cand[2], bytes = 0;
};

ClLayout cl_layout(int w, int h, int d, int max_lesions) {
  ClLayout L;
  L.slots = volume_measure_scratch_words(w, h, d);
  const uint64_t words = (uint64_t)((w + 63) / 64) * (uint64_t)h * (uint64_t)d;
  L.grid = (uint32_t)((words + kVmThreads - 1) / kVmThreads);
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  size_t off = 0;
  for (int s = 0; s < 2; ++s) L.off_labels[s] = off, off += up(L.slots * 4);
  for (int s = 0; s < 2; ++s) L.off_side[s] = off, off += up(L.slots * 4);
  L.off_ctl = off, off += up(sizeof(ClCtl));
  for (int s = 0; s < 2; ++s) L.off_cand[s] = off, off += up((size_t)L.grid * (size_t)max_lesions * 8);
  L.bytes = off;
  return L;
}

}  // namespace

size_t volume_compare_lesions_work_bytes(int w, int h, int d, int max_lesions) {
  if (w <= 0 || h <= 0 || d <= 0 || max_lesions < 1 || max_lesions > kMaxVolumeLesions || volume_measure_scratch_words(w, h, d) == 0)
    return 0;
  return cl_layout(w, h, d, max_lesions).bytes;
}

void launch_volume_compare_lesions(const uint64_t* a, const uint64_t* b, int w, int h, int d, int max_lesions, int connectivity, void* work,
                                   void* out, hipStream_t stream, int max_blocks) {
  if (max_lesions < 1 || max_lesions > kMaxVolumeLesions)
    throw DeviceError("launch_volume_compare_lesions: lesions must be 1.." + std::to_string(kMaxVolumeLesions));
  if (connectivity != 6 && connectivity != 26) throw DeviceError("launch_volume_compare_lesions: connectivity must be 6 or 26");
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("launch_volume_compare_lesions: empty volume");
  if (volume_measure_scratch_words(w, h, d) == 0)
    throw DeviceError("launch_volume_compare_lesions: a " + std::to_string(w) + " x " + std::to_string(h) + " x " + std::to_string(d) +
                      " volume is too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
  if (!a || !b || !work || !out) throw DeviceError("launch_volume_compare_lesions: null buffer");
  if (max_blocks < 0) throw DeviceError("launch_volume_compare_lesions: max_blocks must not be negative");
  const ClLayout L = cl_layout(w, h, d, max_lesions);
  uint8_t* base = static_cast<uint8_t*>(work);
  const int n = (w + 63) / 64;
  ClSides S;
  S.V[0] = BitVolume{a, w, h, d, n, false};
  S.V[1] = BitVolume{b, w, h, d, n, false};
  for (int s = 0; s < 2; ++s) {
    S.labels[s] = reinterpret_cast<uint32_t*>(base + L.off_labels[s]);
    S.side[s] = reinterpret_cast<uint32_t*>(base + L.off_side[s]);
  }
  ClCtl* ctl = reinterpret_cast<ClCtl*>(base + L.off_ctl);
  uint64_t* cand_a = reinterpret_cast<uint64_t*>(base + L.off_cand[0]);
  uint64_t* cand_b = reinterpret_cast<uint64_t*>(base + L.off_cand[1]);
  uint32_t cap = kClMaxBlocks;
  if (max_blocks > 0 && (uint32_t)max_blocks < cap) cap = (uint32_t)max_blocks;
  const uint32_t join_grid = L.grid < cap ? L.grid : cap;
  const dim3 both(L.grid, 2);
  cl_init_kernel<<<(uint32_t)((sizeof(ClCtl) / 4 + kVmThreads - 1) / kVmThreads), kVmThreads, 0, stream>>>(ctl);
  check_launch("cl_init_kernel");
  cl_runs_kernel<<<both, kVmThreads, 0, stream>>>(S);
  check_launch("cl_runs_kernel");
  cl_unions_kernel<<<both, kVmThreads, 0, stream>>>(S, connectivity == 26);
  check_launch("cl_unions_kernel");
  cl_compress_kernel<<<both, kVmThreads, 0, stream>>>(S);
  check_launch("cl_compress_kernel");
  cl_areas_kernel<<<both, kVmThreads, 0, stream>>>(S);
  check_launch("cl_areas_kernel");
  cl_candidates_kernel<<<both, kVmThreads, 0, stream>>>(S, max_lesions, ctl, cand_a, cand_b);
  check_launch("cl_candidates_kernel");
  cl_select_kernel<<<2, kClSelectThreads, 0, stream>>>(max_lesions, ctl, cand_a, cand_b);
  check_launch("cl_select_kernel");
  cl_join_kernel<<<join_grid, kVmThreads, 0, stream>>>(S, L.grid, max_lesions, ctl);
  check_launch("cl_join_kernel");
  cl_count_kernel<<<both, kVmThreads, 0, stream>>>(S, ctl);
  check_launch("cl_count_kernel");
  cl_final_kernel<<<1, kClFinalThreads, 0, stream>>>(S, max_lesions, connectivity, ctl, static_cast<uint8_t*>(out));
  check_launch("cl_final_kernel");
}

void preload_volume_compare_lesions() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&cl_init_kernel), reinterpret_cast<const void*>(&cl_runs_kernel),
                        reinterpret_cast<const void*>(&cl_unions_kernel), reinterpret_cast<const void*>(&cl_compress_kernel),
                        reinterpret_cast<const void*>(&cl_areas_kernel), reinterpret_cast<const void*>(&cl_candidates_kernel),
                        reinterpret_cast<const void*>(&cl_select_kernel), reinterpret_cast<const void*>(&cl_join_kernel),
                        reinterpret_cast<const void*>(&cl_count_kernel), reinterpret_cast<const void*>(&cl_final_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume lesion comparison kernels");
}

}  // namespace nm03::gpu
