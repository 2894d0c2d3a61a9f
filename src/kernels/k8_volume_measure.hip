// K8 — measurements of the dilated VOLUME of the 3D mode (nm03/measure.h VolumeMeasure,
// --measure-volume), on the bit volumes K5 leaves on the device (u64 words, LSB = left-most voxel).
//
// K7 measures a slice with one workgroup; a volume is 1.6 M voxels for a cohort series and 256³ for
// config 5, where one workgroup would be a long chain of dependent L2 round trips. K8 is a
// MULTI-WORKGROUP design whose phases are SEPARATE LAUNCHES on the volume's stream, a thread per
// word (z, y, k). A kernel boundary makes everything one phase wrote visible to the next on every
// XCD: there is no grid barrier, no cooperative launch, no flag and no spin anywhere, so no thread
// ever waits for another workgroup and nothing depends on dispatch order or workgroup placement.
//
//   init     the accumulator record (sums 0, minima / maxima at their identities)
//   A        per word, masked to the width: popcounts, bounding box, coordinate sums, the faces
//            against the six neighbours, the Euler window counts (measure.h euler_word; the padding
//            row, plane and column past the last voxel are counted by the last row's / plane's /
//            word's thread) and the intensity walk (the wave's non-empty words in turn, lane = bit,
//            one coalesced load each); every run's parent = itself, area = 0. Reduced in the wave,
//            then in the workgroup (LDS), then one integer atomic per figure and workgroup.
//   B        unions: each run with the runs it touches in row (y − 1, z) and in plane z − 1, one union
//            per stretch of contact (volume_measure_core.h unite_word)
//   C        the forest is final after B's kernel boundary, so there is no pointer-jumping loop and no
//            flatten barrier: one launch points every run straight at its root (the chain is walked
//            once per run), the next has every in-word stretch add its length at the root — the
//            lengths that share a root are summed in the wave first, so one large body costs one
//            atomic per wave, not one per stretch
//   D        roots are counted and their areas maximised
//   (lesions  optional, --measure-volume-lesions: K10's launches (k10_volume_lesions.hip) go here, between the
//            mask pass's root count and the complement pass, which overwrites the labelling they read; with
//            --measure-volume-diameters K13's (k13_volume_diameters.hip) follow them directly)
//   cavities the scratch is reused for the COMPLEMENT inside the frame (~word & row_word_mask) at the
//            dual connectivity: init runs, B, runs pointed at their roots, then every stretch on a
//            frame face marks its root (second slot = 1; one store per root and wave) and the
//            unmarked roots are counted
//   final    one thread turns the accumulators into the VolumeMeasure record with plain vector stores
//            (device, pinned or host-mapped memory)
//
// Union-find: the nodes are the horizontal runs, named by the slot of their first voxel in a layout
// of w + 1 slots per row (the slot right of it holds the area). A union is the atomicMin form: find
// both roots, atomicMin the smaller into the larger root's parent; finds halve the paths they walk.
// Why this is correct with thousands of workgroups on eight XCDs: EVERY access to a parent is a
// relaxed agent-scope atomic, which acts in L2 / memory and is never served from a stale L1 line;
// parents only ever DECREASE, so whatever value a thread reads — however old — is still an ancestor
// of the node, and a find that follows it ends at a node that was a root when it was read; the value
// the atomicMin RETURNS decides how the union continues: equal to the node, the link was made;
// smaller, another thread linked the node first, and joining that older parent with the other root
// restores what is owed while max(a, b) strictly decreases. All figures are integers and do not
// depend on the order of the unions or of the atomics.
//
// Every loop is bounded by the data: a find walks strictly decreasing slots, a failed union
// continues from a strictly smaller pair, a run-start search walks left through at most the row's words.
#include <hip/hip_runtime.h>

#include <string>

#include "device_util.h"
#include "nm03/kernels.h"
#include "nm03/measure.h"
#include "nm03/volume_measure_core.h"
#include "volume_measure_util.h"

namespace nm03::gpu {

namespace {

// Accumulator record (kVolumeMeasureAccWords u64): sums in u64 words, then the extrema as i32.
enum : int {
  kAccVox = 0, kAccRegion, kAccSumX, kAccSumY, kAccSumZ, kAccFacesX, kAccFacesY, kAccFacesZ, kAccN2, kAccN1, kAccN0,
  kAccRawSum, kAccComponents, kAccLargest, kAccCavities, kAccNumSums,
  kAccExtrema = 16,  // u64 index where the i32 extrema start: x0 y0 z0 raw_min (minima), x1 y1 z1 raw_max (maxima)
};
static_assert(kAccNumSums <= kAccExtrema && kAccExtrema + 4 <= kVolumeMeasureAccWords, "accumulator layout");

__device__ __forceinline__ void acc_add(uint64_t* acc, int i, uint64_t v) {
  if (v) (void)__hip_atomic_fetch_add(acc + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

__global__ void vm_init_kernel(uint64_t* __restrict__ acc) {
  const int t = threadIdx.x;
  if (t < kAccExtrema) acc[t] = 0ull;
  int32_t* ext = reinterpret_cast<int32_t*>(acc + kAccExtrema);
  if (t < 4) ext[t] = 0x7FFFFFFF;
  if (t >= 4 && t < 8) ext[t] = t == 7 ? (int32_t)0x80000000 : -1;
}

__global__ __launch_bounds__(kVmThreads) void vm_figures_kernel(BitVolume V, const uint64_t* __restrict__ region,
                                                                const uint16_t* __restrict__ raw, uint32_t raw_plane_stride,
                                                                uint8_t type, uint8_t stored_bits, int all,
                                                                uint32_t* __restrict__ scratch, uint64_t* __restrict__ acc) {
  __shared__ uint64_t sh_sum[12][kVmWaves];
  __shared__ int32_t sh_ext[8][kVmWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
  vmcore::WordFigures f;
  uint64_t m = 0ull;
  uint32_t row_off = 0;  // sample offset of the word's first voxel
  if (wi.valid) {
    m = vmcore::word_figures(V, region, wi.z, wi.y, wi.k, all != 0, f);
    vmcore::init_runs(V, wi.z, wi.y, wi.k, par);
    row_off = (uint32_t)wi.z * raw_plane_stride + (uint32_t)wi.y * (uint32_t)V.w + (uint32_t)(wi.k << 6);
  }
  // Intensities, by the wave: each of its non-empty words in turn, lane = bit, so a word's samples are
  // one coalesced 128-byte load; four words per round keep four loads in flight.
  int64_t raw_sum = 0;
  int32_t r0 = 0x7FFFFFFF, r1 = (int32_t)0x80000000;
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
        oj[u] = (uint32_t)__shfl((int)row_off, j, 64);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) rv[u] = ((mj[u] >> lane) & 1ull) ? raw[(size_t)oj[u] + (size_t)lane] : (uint16_t)0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if ((mj[u] >> lane) & 1ull) {
        const int32_t v = stored_sample(rv[u], type, stored_bits);
        raw_sum += v;
        r0 = min(r0, v);
        r1 = max(r1, v);
      }
  }
  {
    const uint64_t s[12] = {f.vox, f.region, f.sum_x, f.sum_y, f.sum_z, f.faces_x, f.faces_y, f.faces_z,
                            f.e.n2, f.e.n1, f.e.n0, (uint64_t)raw_sum};
    const int32_t e[8] = {f.x0, f.y0, f.z0, r0, f.x1, f.y1, f.z1, r1};
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      const uint64_t t = wave_sum_u64(s[j]);
      if (lane == 0) sh_sum[j][wave] = t;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int32_t t = j < 4 ? wave_min_i32(e[j]) : wave_max_i32(e[j]);
      if (lane == 0) sh_ext[j][wave] = t;
    }
  }
  __syncthreads();
  // One atomic per figure and workgroup; an empty workgroup adds nothing.
  if (threadIdx.x < 12) {
    uint64_t t = 0;
    for (int wv = 0; wv < kVmWaves; ++wv) t += sh_sum[threadIdx.x][wv];
    static_assert(kAccVox == 0 && kAccRawSum == 11, "sh_sum order = accumulator order");
    acc_add(acc, (int)threadIdx.x, t);
  } else if (threadIdx.x >= 64 && threadIdx.x < 72) {
    const int j = (int)threadIdx.x - 64;
    int32_t* ext = reinterpret_cast<int32_t*>(acc + kAccExtrema);
    int32_t t = sh_ext[j][0];
    for (int wv = 1; wv < kVmWaves; ++wv) t = j < 4 ? min(t, sh_ext[j][wv]) : max(t, sh_ext[j][wv]);
    if (j < 4) {
      if (t != 0x7FFFFFFF) (void)__hip_atomic_fetch_min(ext + j, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (t != (j == 7 ? (int32_t)0x80000000 : -1)) {
      (void)__hip_atomic_fetch_max(ext + j, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Complement pass: every run of the complement, parent = itself, mark = 0.
__global__ __launch_bounds__(kVmThreads) void vm_init_runs_kernel(BitVolume V, uint32_t* __restrict__ scratch) {
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
  if (wi.valid) vmcore::init_runs(V, wi.z, wi.y, wi.k, par);
}

__global__ __launch_bounds__(kVmThreads) void vm_unions_kernel(BitVolume V, int conn26, uint32_t* __restrict__ scratch) {
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
  if (wi.valid) vmcore::unite_word(V, par, wi.z, wi.y, wi.k, conn26 != 0);
}

__global__ __launch_bounds__(kVmThreads) void vm_compress_kernel(BitVolume V, uint32_t* __restrict__ scratch) {
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
  if (wi.valid) vmcore::compress_runs(V, par, wi.z, wi.y, wi.k);
}

__global__ __launch_bounds__(kVmThreads) void vm_areas_kernel(BitVolume V, uint32_t* __restrict__ scratch) {
  const int lane = threadIdx.x & 63;
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
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
  // At most 64 rounds; a wave inside one body takes one.
  for (uint64_t pending = __ballot(len != 0u); pending;) {
    const int leader = __ffsll((long long)pending) - 1;
    const uint32_t r = (uint32_t)__shfl((int)root, leader, 64);
    const bool mine = len != 0u && root == r;
    const uint32_t sum = (uint32_t)wave_sum_u64(mine ? len : 0u);
    if (lane == leader) par.add(r + 1u, sum);
    pending &= ~__ballot(mine);
  }
}

__global__ __launch_bounds__(kVmThreads) void vm_mark_kernel(BitVolume V, uint32_t* __restrict__ scratch) {
  const int lane = threadIdx.x & 63;
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
  // The thread's face stretches: a root other than the last one seen is marked at once, the last is
  // left to the wave, where one lane stores for all that share it (as vm_areas_kernel adds).
  uint32_t root = 0;
  bool have = false;
  if (wi.valid)
    vmcore::frame_stretches(V, par, wi.z, wi.y, wi.k, [&](uint32_t r) {
      if (have && r != root && par.ld(root + 1u) == 0u) par.st(root + 1u, 1u);
      root = r;
      have = true;
    });
  for (uint64_t pending = __ballot(have); pending;) {
    const int leader = __ffsll((long long)pending) - 1;
    const uint32_t r = (uint32_t)__shfl((int)root, leader, 64);
    // Same-address stores from thousands of waves queue up behind each other: a root already marked
    // is left alone (the mark is idempotent; a race only repeats the store).
    if (lane == leader && par.ld(r + 1u) == 0u) par.st(r + 1u, 1u);
    pending &= ~__ballot(have && root == r);
  }
}

// Mask pass: components and the largest area. Complement pass (V.inv): the unmarked roots = cavities.
__global__ __launch_bounds__(kVmThreads) void vm_roots_kernel(BitVolume V, uint32_t* __restrict__ scratch,
                                                              uint64_t* __restrict__ acc) {
  __shared__ uint32_t sh[3][kVmWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
  uint32_t roots = 0, largest = 0, unmarked = 0;
  if (wi.valid) vmcore::count_roots(V, par, wi.z, wi.y, wi.k, roots, largest, unmarked);
  roots = (uint32_t)wave_sum_u64(roots);
  unmarked = (uint32_t)wave_sum_u64(unmarked);
  largest = wave_max_u32(largest);
  if (lane == 0) sh[0][wave] = roots, sh[1][wave] = largest, sh[2][wave] = unmarked;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t r = 0, l = 0, u = 0;
    for (int wv = 0; wv < kVmWaves; ++wv) r += sh[0][wv], l = max(l, sh[1][wv]), u += sh[2][wv];
    if (V.inv) {
      acc_add(acc, kAccCavities, u);
    } else {
      acc_add(acc, kAccComponents, r);
      if (l)
        (void)__hip_atomic_fetch_max(acc + kAccLargest, (uint64_t)l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void vm_final_kernel(const uint64_t* __restrict__ acc, int connectivity, VolumeMeasure* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int32_t* ext = reinterpret_cast<const int32_t*>(acc + kAccExtrema);
  const bool any = acc[kAccVox] > 0;
  VolumeMeasure r = {};
  r.volume_vox = acc[kAccVox];
  r.region_vox = acc[kAccRegion];
  for (int j = 0; j < 3; ++j) {
    r.bbox[j] = any ? ext[j] : -1;
    r.bbox[3 + j] = any ? ext[4 + j] : -1;
  }
  r.components = (uint32_t)acc[kAccComponents];
  r.cavities = (uint32_t)acc[kAccCavities];
  r.sum_x = acc[kAccSumX];
  r.sum_y = acc[kAccSumY];
  r.sum_z = acc[kAccSumZ];
  r.faces_x = acc[kAccFacesX];
  r.faces_y = acc[kAccFacesY];
  r.faces_z = acc[kAccFacesZ];
  r.largest_vox = acc[kAccLargest];
  EulerCounts e;
  e.n2 = acc[kAccN2], e.n1 = acc[kAccN1], e.n0 = acc[kAccN0];
  r.euler = euler_from_counts(e, acc[kAccVox], connectivity);
  r.raw_sum = any ? (int64_t)acc[kAccRawSum] : 0;
  r.raw_min = any ? ext[3] : 0;
  r.raw_max = any ? ext[7] : 0;
  *out = r;
}

void launch_volume_measure(const uint64_t* dilated, const uint64_t* region, const uint16_t* raw, size_t raw_plane_stride,
                           int w, int h, int d, uint8_t type, uint8_t stored_bits, int connectivity, uint32_t* scratch,
                           uint64_t* acc, VolumeMeasure* out, hipStream_t stream, const VolumeLesionWork* lesions) {
  if (connectivity != 6 && connectivity != 26) throw DeviceError("launch_volume_measure: connectivity must be 6 or 26");
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("launch_volume_measure: empty volume");
  if (stored_bits < 1 || stored_bits > 16) throw DeviceError("launch_volume_measure: stored bits must be 1..16");
  // The runs are named by 32-bit slots, and the samples are addressed by 32-bit offsets.
  if (volume_measure_scratch_words(w, h, d) == 0 || raw_plane_stride < (size_t)w * (size_t)h ||
      raw_plane_stride * (size_t)d > 0xFFFFFFFFull)
    throw DeviceError("launch_volume_measure: a " + std::to_string(w) + " x " + std::to_string(h) + " x " +
                      std::to_string(d) + " volume is too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
  if (!dilated || !region || !raw || !scratch || !acc || !out) throw DeviceError("launch_volume_measure: null buffer");
  if (lesions && lesions->diameters) validate_volume_diameters(dilated, w, h, d, scratch, *lesions);
  const int n = (w + 63) / 64;
  const uint64_t words = (uint64_t)n * (uint64_t)h * (uint64_t)d;  // ≤ voxels < 2^32
  const uint32_t grid = (uint32_t)((words + kVmThreads - 1) / kVmThreads);
  const BitVolume M{dilated, w, h, d, n, false};
  const BitVolume C{dilated, w, h, d, n, true};
  const int conn26 = connectivity == 26;
  vm_init_kernel<<<1, 64, 0, stream>>>(acc);
  check_launch("vm_init_kernel");
  vm_figures_kernel<<<grid, kVmThreads, 0, stream>>>(M, region, raw, (uint32_t)raw_plane_stride, type, stored_bits,
                                                    connectivity == 6, scratch, acc);
  check_launch("vm_figures_kernel");
  vm_unions_kernel<<<grid, kVmThreads, 0, stream>>>(M, conn26, scratch);
  check_launch("vm_unions_kernel");
  vm_compress_kernel<<<grid, kVmThreads, 0, stream>>>(M, scratch);
  check_launch("vm_compress_kernel");
  vm_areas_kernel<<<grid, kVmThreads, 0, stream>>>(M, scratch);
  check_launch("vm_areas_kernel");
  vm_roots_kernel<<<grid, kVmThreads, 0, stream>>>(M, scratch, acc);
  check_launch("vm_roots_kernel");
  // The per-lesion phase (K10) reads the mask pass's labelling — every run at its root, the area in the
  // slot after a root — before the complement pass overwrites the scratch.
  if (lesions) {
    launch_volume_lesions(dilated, raw, raw_plane_stride, w, h, d, type, stored_bits, scratch, *lesions, stream);
    // The lesions' lengths (K13) need the same labelling, and K10's chosen roots and bounding boxes.
    if (lesions->diameters) launch_volume_diameters(dilated, w, h, d, scratch, *lesions, stream);
  }
  // Cavities: the complement at the dual connectivity, on the same scratch.
  vm_init_runs_kernel<<<grid, kVmThreads, 0, stream>>>(C, scratch);
  check_launch("vm_init_runs_kernel");
  vm_unions_kernel<<<grid, kVmThreads, 0, stream>>>(C, !conn26, scratch);
  check_launch("vm_unions_kernel (complement)");
  vm_compress_kernel<<<grid, kVmThreads, 0, stream>>>(C, scratch);
  check_launch("vm_compress_kernel (complement)");
  vm_mark_kernel<<<grid, kVmThreads, 0, stream>>>(C, scratch);
  check_launch("vm_mark_kernel");
  vm_roots_kernel<<<grid, kVmThreads, 0, stream>>>(C, scratch, acc);
  check_launch("vm_roots_kernel (complement)");
  vm_final_kernel<<<1, 64, 0, stream>>>(acc, connectivity, out);
  check_launch("vm_final_kernel");
}

void preload_volume_measure() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&vm_init_kernel), reinterpret_cast<const void*>(&vm_figures_kernel),
                        reinterpret_cast<const void*>(&vm_init_runs_kernel), reinterpret_cast<const void*>(&vm_unions_kernel),
                        reinterpret_cast<const void*>(&vm_compress_kernel), reinterpret_cast<const void*>(&vm_areas_kernel),
                        reinterpret_cast<const void*>(&vm_mark_kernel),
                        reinterpret_cast<const void*>(&vm_roots_kernel), reinterpret_cast<const void*>(&vm_final_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume measure kernels");
}

}  // namespace nm03::gpu
