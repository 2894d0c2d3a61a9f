// K17 — overlap and surface distances between two bit volumes of one frame (nm03/volume_compare.h, --compare-to).
//
// LAUNCHES on the volume's stream, separated by kernel boundaries; all per-word and per-key arithmetic is
// nm03/volume_compare_core.h, shared with the host:
//   vcmp_init      zero the accumulators (counts, sums, histograms)
//   vcmp_surface   a thread per u64 word (z, y, k): the A and B words and their six neighbours (the x neighbours
//                  take the carry bit of the adjacent words; rows and planes are plain words; outside the frame is
//                  0), the S(A) and S(B) words stored with the bits past the width zero, the popcounts of A, B,
//                  A ∧ B, S(A), S(B) summed over the wave, then over LDS: one global atomic per non-zero figure
//                  and workgroup
//   then per direction (A→B, then B→A with the roles swapped; the map buffer is reused):
//   K16's launch_volume_distance(S(to), foreground, no cap) → the i64 map (three launches, k16 untouched)
//   vcmp_hist<0>   the sampling pass over the set bits of S(from): s = ⌊√map⌋, Σ s, the best (value, smallest
//                  position) into the workgroup's own slot as K16's thickness ending does, and the histogram of
//                  the key's first digit
//   vcmp_select    ONE workgroup locates the rank in the histogram (icore::select_bin on a thread's bins after a
//                  block scan) and leaves the digit and the rank inside it
//   vcmp_hist<1>, vcmp_select, vcmp_hist<2>   the next digits over the keys that agree with the digits found
//   vcmp_final     ONE workgroup locates the last digit, reduces the slots and writes the directed record (the
//                  first direction also the overlap head) with plain vector stores; found = 0 when either surface
//                  is empty (the sampling and select launches then return at once: the counts were written by an
//                  earlier launch, so the test is uniform over the grid)
// No cooperative launch, grid barrier, flag, look-back or spin: the only cross-workgroup traffic is a slot per
// workgroup that one workgroup reduces in a LATER launch, and relaxed atomic adds (at most one per figure or
// non-zero bin and workgroup) on counters nobody reads before the next kernel boundary. Every loop is bounded
// by the data.
//
// DIGIT WIDTH: 11 + 11 + 10 bits, three histogram passes, not 4 × 8. Every pass walks S(from) and reads the
// 8-byte map value of each surface voxel again, so a pass less is a quarter of that traffic saved. What limits
// the width is LDS: a 2048-bin u32 histogram is 8 KiB per workgroup, which still lets every wave slot of a
// CU be filled (a 16-bit digit would need 256 KiB, more than a CU has). With 8 KiB there is one histogram per
// workgroup, not one per wave as in K11's 256-bin pass; the wave-combining add (wave_hist_add) keeps the
// common case — neighbouring surface voxels with the same high digits — at one LDS atomic per wave and word.
//
// GRID of vcmp_hist: min(ceil(words / 256), kCmpMaxBlocks) workgroups, each striding over the 256-word blocks, so
// that ONE workgroup can reduce the slots and a workgroup flushes its histogram once. A volume needs more than
// kCmpMaxBlocks · 256 = 262 144 words (256 × 256 × 257 voxels) before a workgroup takes a second trip with the
// default; `max_blocks` of the launcher lowers the cap (the results do not depend on it), and the tests run a
// 130 × 40 × 24 volume (2880 words, 12 blocks) at max_blocks = 5: three trips, the last one partial.
#include <hip/hip_runtime.h>

#include <string>

#include "device_util.h"
#include "measure_util.h"
#include "nm03/intensity_core.h"
#include "nm03/kernels.h"
#include "nm03/volume_compare.h"
#include "nm03/volume_compare_core.h"
#include "nm03/volume_distance_core.h"

namespace nm03::gpu {

constexpr int kCmpThreads = 256;
constexpr int kCmpWaves = kCmpThreads / 64;
constexpr uint32_t kCmpMaxBlocks = 1024;  // workgroups of vcmp_hist: what ONE workgroup reduces afterwards
static_assert(vcmp::kMaxBins % kCmpThreads == 0 && vcmp::kMaxBins / kCmpThreads <= 8, "a thread owns at most 8 bins");

namespace {

struct CmpGeom {
  int w, h, d, wpr;
  uint32_t words;  // wpr · h · d
};

enum { kCntA = 0, kCntB = 1, kCntTp = 2, kCntSa = 3, kCntSb = 4, kCmpCounts = 5 };

// The accumulators (device memory, zeroed by vcmp_init). Index [dir]: 0 = A→B, 1 = B→A.
struct CmpAcc {
  uint64_t counts[kCmpCounts + 1];
  uint64_t sum[2];
  uint64_t rank[2];    // the rank left inside the digits found so far
  uint32_t prefix[2];  // the digits found so far, in place
  uint32_t pad[2];
  uint32_t hist[2][vcmp::kPasses][vcmp::kMaxBins];
};
static_assert(sizeof(CmpAcc) % 4 == 0, "zeroed by words");

struct CmpSlot {
  int64_t value;
  uint64_t pos;  // raster voxel index, vdist::kNoCandidate = none
};

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(uint64_t)v, o, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), o, 64);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ void add_u32(uint32_t* p, uint32_t v) {
  if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void add_u64(uint64_t* p, uint64_t v) {
  if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The best of the workgroup's candidates in thread 0 (vdist::better: larger value, then smaller position).
__device__ __forceinline__ void block_best(int64_t& bv, uint64_t& bp, int64_t* sh_v, uint64_t* sh_p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t ov = shfl_xor_i64(bv, o);
    const uint64_t op = (uint64_t)shfl_xor_i64((int64_t)bp, o);
    if (vdist::better(ov, op, bv, bp)) bv = ov, bp = op;
  }
  if (lane == 0) sh_v[wave] = bv, sh_p[wave] = bp;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int wv = 1; wv < kCmpWaves; ++wv)
      if (vdist::better(sh_v[wv], sh_p[wv], bv, bp)) bv = sh_v[wv], bp = sh_p[wv];
}

// The rank's bin among `bins` counters by one workgroup: thread t owns bins t · per … t · per + per − 1, a block
// scan finds the thread whose bins hold the rank, and that thread finishes with icore::select_bin on its own and
// calls found(bin, rank left). `rank` is 1 … Σ hist. Called by all threads.
template <class F>
__device__ __forceinline__ void block_select_bin(const uint32_t* hist, uint32_t bins, uint64_t rank, uint32_t* sh_scan, F&& found) {
  const uint32_t per = bins / (uint32_t)kCmpThreads;  // 8 or 4
  uint32_t c[8];
  uint32_t s = 0;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) {
    c[i] = i < per ? hist[threadIdx.x * per + i] : 0u;
    s += c[i];
  }
  uint32_t total;
  const uint32_t exc = block_exclusive_scan(s, sh_scan, &total);
  if (rank > (uint64_t)exc && rank <= (uint64_t)exc + (uint64_t)s) {  // at most one thread
    const icore::BinRank l = icore::select_bin(c, (int)per, rank - (uint64_t)exc);
    found(threadIdx.x * per + l.bin, l.rank);
  }
}

}  // namespace

__global__ __launch_bounds__(kCmpThreads) void vcmp_init_kernel(CmpAcc* __restrict__ acc) {
  uint32_t* w = reinterpret_cast<uint32_t*>(acc);
  const uint32_t n = (uint32_t)(sizeof(CmpAcc) / 4);
  for (uint32_t i = blockIdx.x * (uint32_t)kCmpThreads + threadIdx.x; i < n; i += gridDim.x * (uint32_t)kCmpThreads) w[i] = 0u;
}

__global__ __launch_bounds__(kCmpThreads) void vcmp_surface_kernel(CmpGeom G, const uint64_t* __restrict__ a,
                                                                   const uint64_t* __restrict__ b, uint64_t* __restrict__ sa,
                                                                   uint64_t* __restrict__ sb, CmpAcc* __restrict__ acc) {
  __shared__ uint32_t sh_c[kCmpCounts][kCmpWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * (uint32_t)kCmpThreads + threadIdx.x;
  uint32_t c[kCmpCounts] = {0u, 0u, 0u, 0u, 0u};
  if (i < G.words) {
    const uint32_t row = i / (uint32_t)G.wpr;
    const int k = (int)(i - row * (uint32_t)G.wpr);
    const int z = (int)(row / (uint32_t)G.h);
    const int y = (int)(row - (uint32_t)z * (uint32_t)G.h);
    const uint64_t wa = vcmp::word_at(a, G.w, G.h, G.d, G.wpr, z, y, k), wb = vcmp::word_at(b, G.w, G.h, G.d, G.wpr, z, y, k);
    const uint64_t xa = vcmp::surface_at(a, G.w, G.h, G.d, G.wpr, z, y, k), xb = vcmp::surface_at(b, G.w, G.h, G.d, G.wpr, z, y, k);
    sa[i] = xa;
    sb[i] = xb;
    c[kCntA] = (uint32_t)__popcll(wa), c[kCntB] = (uint32_t)__popcll(wb), c[kCntTp] = (uint32_t)__popcll(wa & wb);
    c[kCntSa] = (uint32_t)__popcll(xa), c[kCntSb] = (uint32_t)__popcll(xb);
  }
#pragma unroll
  for (int f = 0; f < kCmpCounts; ++f) {
    const uint32_t s = wave_sum_u32(c[f]);
    if (lane == 0) sh_c[f][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x < kCmpCounts) {
    uint32_t s = 0;
    for (int wv = 0; wv < kCmpWaves; ++wv) s += sh_c[threadIdx.x][wv];
    add_u64(acc->counts + threadIdx.x, (uint64_t)s);
  }
}

// PASS 0: the sampling pass (Σ s, the best (value, position) into slots[blockIdx.x], the first digit's histogram).
// PASS 1, 2: the histogram of that digit over the keys that agree with acc->prefix[dir]. `surf` = S(from), `map` =
// the distance map of S(to). The grid may be smaller than `nblocks`: a workgroup strides over the rest.
template <int PASS>
__global__ __launch_bounds__(kCmpThreads) void vcmp_hist_kernel(CmpGeom G, uint32_t nblocks, int dir, const uint64_t* __restrict__ surf,
                                                                const int64_t* __restrict__ map, CmpAcc* __restrict__ acc,
                                                                CmpSlot* __restrict__ slots) {
  __shared__ uint32_t sh_hist[vcmp::kMaxBins];
  __shared__ int64_t sh_v[kCmpWaves];
  __shared__ uint64_t sh_p[kCmpWaves];
  __shared__ uint64_t sh_sum[kCmpWaves];
  if (acc->counts[kCntSa] == 0ull || acc->counts[kCntSb] == 0ull) return;  // uniform over the grid: an earlier launch wrote them
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t prefix = PASS == 0 ? 0u : acc->prefix[dir];
  for (int i = threadIdx.x; i < vcmp::kMaxBins; i += kCmpThreads) sh_hist[i] = 0u;
  __syncthreads();
  uint64_t sum = 0;
  int64_t bv = 0;
  uint64_t bp = vdist::kNoCandidate;
  for (uint32_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {  // the same trips for every wave (ballots inside)
    const uint32_t i = blk * (uint32_t)kCmpThreads + threadIdx.x;
    uint64_t m = 0ull;
    uint32_t base = 0u;  // the raster index of the word's first voxel (voxels < 2^32, volume_compare_layout)
    if (i < G.words) {
      m = surf[i];
      const uint32_t row = i / (uint32_t)G.wpr;
      base = row * (uint32_t)G.w + ((i - row * (uint32_t)G.wpr) << 6);
    }
    // The wave's non-empty words in turn, lane = bit: a word's map values are one coalesced load, four in flight.
    for (uint64_t act = __ballot(m != 0ull); act;) {
      uint64_t mj[4];
      uint32_t oj[4];
      int64_t dv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        mj[u] = 0ull;
        oj[u] = 0u;
        if (act) {
          const int j = __ffsll((long long)act) - 1;
          act &= act - 1;
          mj[u] = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(m >> 32), j, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)m, j, 64);
          oj[u] = (uint32_t)__shfl((int)base, j, 64);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) dv[u] = ((mj[u] >> lane) & 1ull) ? map[(size_t)oj[u] + (size_t)lane] : (int64_t)0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool on = ((mj[u] >> lane) & 1ull) != 0ull;
        const uint32_t key = on ? vcmp::isqrt_um(dv[u]) : 0u;
        if constexpr (PASS == 0) {
          const uint64_t pos = (uint64_t)oj[u] + (uint64_t)lane;
          if (on) {
            sum += (uint64_t)key;
            if (vdist::better(dv[u], pos, bv, bp)) bv = dv[u], bp = pos;
          }
        }
        wave_hist_add(sh_hist, vcmp::digit(key, PASS), on && vcmp::in_prefix(key, prefix, PASS), lane);
      }
    }
  }
  if constexpr (PASS == 0) {
    sum = wave_sum_u64(sum);
    if (lane == 0) sh_sum[wave] = sum;
    block_best(bv, bp, sh_v, sh_p);  // a barrier inside
    if (threadIdx.x == 0) {
      slots[blockIdx.x].value = bv;
      slots[blockIdx.x].pos = bp;
      uint64_t s = 0;
      for (int wv = 0; wv < kCmpWaves; ++wv) s += sh_sum[wv];
      add_u64(acc->sum + dir, s);
    }
  }
  __syncthreads();
  // At most one atomic per non-zero bin and workgroup.
  for (uint32_t i = threadIdx.x; i < vcmp::digit_bins(PASS); i += kCmpThreads) add_u32(&acc->hist[dir][PASS][i], sh_hist[i]);
}

// One workgroup: the digit of `pass` (0 or 1) and the rank left inside it.
__global__ __launch_bounds__(kCmpThreads) void vcmp_select_kernel(int pass, int dir, CmpAcc* __restrict__ acc) {
  __shared__ uint32_t sh_scan[17];
  const uint64_t n_from = acc->counts[dir == 0 ? kCntSa : kCntSb], n_to = acc->counts[dir == 0 ? kCntSb : kCntSa];
  if (n_from == 0ull || n_to == 0ull) return;  // uniform
  // read before the scan's first barrier; the one thread that writes does so after its last
  const uint64_t rank = pass == 0 ? icore::percentile_rank(vcmp::kPercentile, n_from) : acc->rank[dir];
  const uint32_t prefix = pass == 0 ? 0u : acc->prefix[dir];
  block_select_bin(acc->hist[dir][pass], vcmp::digit_bins(pass), rank, sh_scan, [&](uint32_t bin, uint64_t left) {
    acc->prefix[dir] = prefix | (bin << vcmp::digit_shift(pass));
    acc->rank[dir] = left;
  });
}

// One workgroup: the last digit, the best of the `nslots` slots, the directed record; dir 0 also writes the head.
__global__ __launch_bounds__(kCmpThreads) void vcmp_final_kernel(CmpGeom G, int dir, const CmpAcc* __restrict__ acc,
                                                                 const CmpSlot* __restrict__ slots, uint32_t nslots,
                                                                 VolumeCompare* __restrict__ out) {
  __shared__ uint32_t sh_scan[17];
  __shared__ int64_t sh_v[kCmpWaves];
  __shared__ uint64_t sh_p[kCmpWaves];
  __shared__ uint32_t sh_key;
  const uint64_t n_from = acc->counts[dir == 0 ? kCntSa : kCntSb], n_to = acc->counts[dir == 0 ? kCntSb : kCntSa];
  const bool found = n_from != 0ull && n_to != 0ull;  // uniform
  int64_t bv = 0;
  uint64_t bp = vdist::kNoCandidate;
  if (found) {
    if (threadIdx.x == 0) sh_key = 0u;
    __syncthreads();
    const uint32_t prefix = acc->prefix[dir];
    block_select_bin(acc->hist[dir][vcmp::kPasses - 1], vcmp::digit_bins(vcmp::kPasses - 1), acc->rank[dir], sh_scan,
                     [&](uint32_t bin, uint64_t) { sh_key = prefix | bin; });
    for (uint32_t i = threadIdx.x; i < nslots; i += (uint32_t)kCmpThreads) {
      const CmpSlot s = slots[i];
      if (vdist::better(s.value, s.pos, bv, bp)) bv = s.value, bp = s.pos;
    }
  }
  block_best(bv, bp, sh_v, sh_p);  // a barrier inside: sh_key is visible to thread 0 after it
  if (threadIdx.x == 0) {
    VolumeCompareDirected r;
    const bool ok = found && bp != vdist::kNoCandidate;
    const uint64_t row = ok ? bp / (uint64_t)G.w : 0ull;
    r.max_um2 = ok ? (uint64_t)bv : 0ull;
    r.sum_um = ok ? acc->sum[dir] : 0ull;
    r.n = ok ? (uint32_t)n_from : 0u;
    r.p95_um = ok ? sh_key : 0u;
    r.worst[0] = ok ? (int32_t)(bp - row * (uint64_t)G.w) : -1;
    r.worst[1] = ok ? (int32_t)(row % (uint64_t)G.h) : -1;
    r.worst[2] = ok ? (int32_t)(row / (uint64_t)G.h) : -1;
    r.found = ok ? 1 : 0;
    if (dir == 0) {
      const uint64_t na = acc->counts[kCntA], nb = acc->counts[kCntB], tp = acc->counts[kCntTp];
      out->a_vox = na, out->b_vox = nb, out->tp_vox = tp, out->fp_vox = na - tp, out->fn_vox = nb - tp;
      out->surface_a = acc->counts[kCntSa], out->surface_b = acc->counts[kCntSb];
      out->ab = r;
    } else {
      out->ba = r;
      out->pad = 0ull;
    }
  }
}

namespace {

uint8_t* at(void* work, size_t off) { return static_cast<uint8_t*>(work) + off; }

}  // namespace

VolumeCompareLayout volume_compare_layout(int w, int h, int d) {
  VolumeCompareLayout L;
  L.dist = volume_distance_layout(w, h, d);  // throws for an empty volume, a width above 65535, 2^31 words
  const uint64_t voxels = (uint64_t)w * (uint64_t)h * (uint64_t)d;
  if (voxels >= (1ull << 32))
    throw DeviceError("volume compare: a " + std::to_string(w) + " x " + std::to_string(h) + " x " + std::to_string(d) +
                      " volume has 2^32 voxels or more");
  L.blocks = (L.dist.words + kCmpThreads - 1) / kCmpThreads;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  L.off_surface_a = 0;
  L.off_surface_b = up((size_t)L.dist.words * 8);
  L.off_acc = L.off_surface_b + up((size_t)L.dist.words * 8);
  L.off_slots = L.off_acc + up(sizeof(CmpAcc));
  L.off_map = L.off_slots + up((size_t)kCmpMaxBlocks * sizeof(CmpSlot));
  L.off_dist = L.off_map + up((size_t)voxels * sizeof(int64_t));
  L.bytes = L.off_dist + L.dist.bytes;
  return L;
}

size_t volume_compare_work_bytes(int w, int h, int d) { return volume_compare_layout(w, h, d).bytes; }

void launch_volume_compare(const uint64_t* a, const uint64_t* b, const VolumeCompareLayout& L, const uint32_t um[3], void* work,
                           VolumeCompare* out, hipStream_t stream, int max_blocks) {
  const VolumeDistanceLayout& D = L.dist;
  if (D.w <= 0 || D.h <= 0 || D.d <= 0 || D.wpr != (D.w + 63) / 64 || (uint64_t)D.wpr * (uint64_t)D.h * (uint64_t)D.d != D.words ||
      L.blocks != (D.words + kCmpThreads - 1) / kCmpThreads || (uint64_t)D.w * (uint64_t)D.h * (uint64_t)D.d >= (1ull << 32))
    throw DeviceError("launch_volume_compare: not a layout of volume_compare_layout");
  for (int x = 0; x < 3; ++x)
    if (um[x] < 1u) throw DeviceError("launch_volume_compare: a spacing must be at least 1 um");
  const std::string ext = measure::volume_distance_extent_error(D.w, D.h, D.d, um);
  if (!ext.empty()) throw DeviceError("launch_volume_compare: " + ext);
  if (!a || !b || !work || !out) throw DeviceError("launch_volume_compare: null buffer");
  if (max_blocks < 0) throw DeviceError("launch_volume_compare: max_blocks must not be negative");
  CmpGeom G;
  G.w = D.w, G.h = D.h, G.d = D.d, G.wpr = D.wpr, G.words = D.words;
  auto* sa = reinterpret_cast<uint64_t*>(at(work, L.off_surface_a));
  auto* sb = reinterpret_cast<uint64_t*>(at(work, L.off_surface_b));
  auto* acc = reinterpret_cast<CmpAcc*>(at(work, L.off_acc));
  auto* slots = reinterpret_cast<CmpSlot*>(at(work, L.off_slots));
  auto* map = reinterpret_cast<int64_t*>(at(work, L.off_map));
  void* dist_work = at(work, L.off_dist);
  uint32_t cap = kCmpMaxBlocks;
  if (max_blocks > 0 && (uint32_t)max_blocks < cap) cap = (uint32_t)max_blocks;
  const uint32_t grid = L.blocks < cap ? L.blocks : cap;
  vcmp_init_kernel<<<(uint32_t)((sizeof(CmpAcc) / 4 + kCmpThreads - 1) / kCmpThreads), kCmpThreads, 0, stream>>>(acc);
  check_launch("vcmp_init_kernel");
  vcmp_surface_kernel<<<L.blocks, kCmpThreads, 0, stream>>>(G, a, b, sa, sb, acc);
  check_launch("vcmp_surface_kernel");
  for (int dir = 0; dir < 2; ++dir) {
    const uint64_t* from = dir == 0 ? sa : sb;
    const uint64_t* to = dir == 0 ? sb : sa;
    launch_volume_distance(to, D, um, false, -1, dist_work, map, stream);
    vcmp_hist_kernel<0><<<grid, kCmpThreads, 0, stream>>>(G, L.blocks, dir, from, map, acc, slots);
    check_launch("vcmp_hist_kernel<0>");
    vcmp_select_kernel<<<1, kCmpThreads, 0, stream>>>(0, dir, acc);
    check_launch("vcmp_select_kernel");
    vcmp_hist_kernel<1><<<grid, kCmpThreads, 0, stream>>>(G, L.blocks, dir, from, map, acc, slots);
    check_launch("vcmp_hist_kernel<1>");
    vcmp_select_kernel<<<1, kCmpThreads, 0, stream>>>(1, dir, acc);
    check_launch("vcmp_select_kernel");
    vcmp_hist_kernel<2><<<grid, kCmpThreads, 0, stream>>>(G, L.blocks, dir, from, map, acc, slots);
    check_launch("vcmp_hist_kernel<2>");
    vcmp_final_kernel<<<1, kCmpThreads, 0, stream>>>(G, dir, acc, slots, grid, out);
    check_launch("vcmp_final_kernel");
  }
}

void preload_volume_compare() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&vcmp_init_kernel), reinterpret_cast<const void*>(&vcmp_surface_kernel),
                        reinterpret_cast<const void*>(&vcmp_hist_kernel<0>), reinterpret_cast<const void*>(&vcmp_hist_kernel<1>),
                        reinterpret_cast<const void*>(&vcmp_hist_kernel<2>), reinterpret_cast<const void*>(&vcmp_select_kernel),
                        reinterpret_cast<const void*>(&vcmp_final_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume compare kernels");
}

}  // namespace nm03::gpu
