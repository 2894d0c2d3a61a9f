// K13 — the lengths of every LESION of the dilated volume (nm03/measure.h VolumeLesionDiameters,
// --measure-volume-diameters): the 3D major diameter, the largest axial diameter and its perpendicular,
// maximised in integer micrometres. The definitions and the worked example are at the record.
//
// K13 runs directly after K10, between K8's two passes (launch_volume_measure): it reads the mask
// pass's labelling in K8's scratch, K10's chosen roots (LesionCtl) and K10's accumulators (the bounding
// boxes), and writes into none of them. Like K8 and K10 it is MULTI-WORKGROUP with the phases as
// SEPARATE LAUNCHES: no grid barrier, no cooperative launch, no flag, no look-back, no spin; no
// workgroup reads in a launch what another writes in it (the table's atomics return nothing anyone
// uses). The arithmetic is nm03/volume_diameters_core.h, which the host runs too.
//
//   init    the (xlo, xhi) table of the chosen lesions' bounding-box rows at its identities
//   rows    a thread per word (z, y, k): every in-word stretch looks its root up among the chosen slots;
//           the stretches of one lesion are merged in the thread, a lane whose left / right neighbour
//           lane holds the same row and lesion leaves the minimum / maximum to it, the others issue
//           one atomicMin / atomicMax on the row's entry. The candidates of a lesion are the two
//           extremes of each of its rows (why they suffice, ties included: the core header).
//   tiles   the bounding box of every tile of kTileRows consecutive rows
//   bound   a workgroup per 2048 rows of a lesion: the extremes of 13 directions (26 voxels) in one pass,
//           into the workgroup's own slots
//   planes  a lesion's first workgroup merges those slots: l3 is the best squared distance among the 26
//           voxels. Then a wave per plane of a lesion: the extremes of the 4 directions in the plane (8
//           voxels), the best squared distance among them, one atomicMax on the lesion's l2. Both bounds
//           are lengths some pair of candidates really has.
//   pairs   a fixed grid shares out the tile pairs (I, J ≥ I) of all lesions, pair i to workgroup i mod
//           grid: a thread tests one pair against the bounds of the launches before (strictly below →
//           skipped, so every tie survives), the survivors are compared from LDS, thread t holding candidate
//           t of tile I against a quarter of tile J (a pair is four items); same-plane pairs feed the axial maximum in the same walk.
//           Every workgroup writes its best per lesion into its own slots with plain stores.
//   final   one workgroup per record: the best of the partial slots, then the perpendicular over the row
//           extremes of plane axial_z, then one plain 128-byte store (device, pinned or host-mapped).
//
// Every loop is bounded by the data: rows and tiles by the bounding boxes, the chunks by the tile
// pairs, the compare by the tile size, the lookups by log2(N).
#include <hip/hip_runtime.h>

#include <string>

#include "device_util.h"
#include "nm03/kernels.h"
#include "nm03/measure.h"
#include "nm03/volume_diameters_core.h"
#include "nm03/volume_measure_core.h"
#include "volume_measure_util.h"

namespace nm03::gpu {

namespace {

using vdcore::Best;
using vdcore::Cand;
using vdcore::Extreme;
using vdcore::Grid;
using vdcore::RowExt;
using vdcore::Rows;
using vdcore::TileBox;

constexpr int kVdTile = vdcore::kTileRows;
constexpr int kVdCands = 2 * kVdTile;  // candidates of a tile = threads of a pairs workgroup
constexpr int kVdPairGrid = 1024;      // workgroups of the pairs launch, at most
constexpr int kVdBoundRows = 8 * kVmThreads;  // rows per workgroup of the bound launch
constexpr int kVdSplit = 4;                   // a surviving tile pair is shared out to this many workgroups
constexpr int kVdFinalThreads = 256;
static_assert(kVdCands == kVmThreads, "a pairs workgroup holds one candidate per thread");

// The rows of lesion `rank`'s bounding box, from K10's accumulator.
__device__ __forceinline__ Rows lesion_rows(const uint64_t* __restrict__ acc, int rank) {
  const int32_t* e = reinterpret_cast<const int32_t*>(acc + (size_t)rank * kVlAccWords + kLsNumSums);
  const int32_t lo[3] = {e[kLeX0], e[kLeY0], e[kLeZ0]}, hi[3] = {e[kLeX1], e[kLeY1], e[kLeZ1]};
  return vdcore::rows_of(lo, hi);
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const Best t{shfl_xor_u64(b.d2, o), shfl_xor_u64(b.key, o)};
    vdcore::best_take(t, b);
  }
  return b;
}
__device__ __forceinline__ Extreme wave_extreme(Extreme e) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const Extreme t{(int64_t)shfl_xor_u64((uint64_t)e.proj, o), (uint32_t)__shfl_xor((int)e.pos, o, 64)};
    if (vdcore::extreme_beats(t, e)) e = t;
  }
  return e;
}
// The workgroup's best in every thread; `sh` holds one entry per wave. Two barriers.
template <int kWaves>
__device__ __forceinline__ Best block_best(Best b, Best* sh) {
  b = wave_best(b);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = b;
  __syncthreads();
  Best r = sh[0];
  for (int wv = 1; wv < kWaves; ++wv) vdcore::best_take(sh[wv], r);
  __syncthreads();
  return r;
}
template <int kWaves>
__device__ __forceinline__ Extreme block_extreme(Extreme e, Extreme* sh) {
  e = wave_extreme(e);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = e;
  __syncthreads();
  Extreme r = sh[0];
  for (int wv = 1; wv < kWaves; ++wv)
    if (vdcore::extreme_beats(sh[wv], r)) r = sh[wv];
  __syncthreads();
  return r;
}
template <int kWaves>
__device__ __forceinline__ uint64_t block_max_u64(uint64_t v, uint64_t* sh) {
  v = wave_max_u64(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t r = sh[0];
  for (int wv = 1; wv < kWaves; ++wv) r = sh[wv] > r ? sh[wv] : r;
  __syncthreads();
  return r;
}

}  // namespace

__global__ __launch_bounds__(kVmThreads) void vd_init_kernel(Grid g, int nmax, const LesionCtl* __restrict__ ctl,
                                                             const uint64_t* __restrict__ acc, RowExt* __restrict__ table,
                                                             uint64_t* __restrict__ bounds) {
  const uint64_t rows = (uint64_t)g.h * (uint64_t)g.d;
  const uint64_t i = (uint64_t)blockIdx.x * kVmThreads + threadIdx.x;  // entry (rank, z, y)
  if (i < (uint64_t)kMaxVolumeLesions) bounds[2 * i] = 0ull, bounds[2 * i + 1] = 0ull;
  const uint64_t rank = i / rows;
  if (rank >= (uint64_t)min((uint32_t)nmax, ctl->count)) return;
  const uint32_t row = (uint32_t)(i - rank * rows);
  const int z = (int)(row / (uint32_t)g.h), y = (int)(row - (uint32_t)z * (uint32_t)g.h);
  const Rows r = lesion_rows(acc, (int)rank);
  if (z < r.z0 || z >= r.z0 + r.nz || y < r.y0 || y >= r.y0 + r.ny) return;
  table[i] = RowExt{vdcore::kRowNoLo, vdcore::kRowNoHi};
}

__global__ __launch_bounds__(kVmThreads) void vd_rows_kernel(BitVolume V, uint32_t* __restrict__ scratch,
                                                             const LesionCtl* __restrict__ ctl, RowExt* __restrict__ table) {
  __shared__ uint32_t sh_slot[kMaxVolumeLesions], sh_rank[kMaxVolumeLesions];
  const int lane = threadIdx.x & 63;
  const int count = (int)ctl->count;  // the same in every thread
  if (count == 0) return;
  if ((int)threadIdx.x < count) sh_slot[threadIdx.x] = ctl->srt_slot[threadIdx.x], sh_rank[threadIdx.x] = ctl->srt_rank[threadIdx.x];
  __syncthreads();
  const WordIndex wi = my_word(V);
  DeviceParents par{scratch};
  const uint64_t m = wi.valid ? V.at(wi.z, wi.y, wi.k) : 0ull;
  auto row_min = [&](int rank, int32_t lo) {
    (void)__hip_atomic_fetch_min(&table[vdcore::row_index(rank, wi.z, wi.y, V.h, V.d)].lo, lo, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
  };
  auto row_max = [&](int rank, int32_t hi) {
    (void)__hip_atomic_fetch_max(&table[vdcore::row_index(rank, wi.z, wi.y, V.h, V.d)].hi, hi, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
  };
  // The thread's stretches of chosen lesions: those of one lesion are merged; a stretch of ANOTHER
  // chosen lesion in the same word (rare) sends the merged ones to the table at once.
  int cur = -1;
  int32_t lo = 0, hi = 0;
  if (m)
    vmcore::lesion_stretches(V, par, wi.z, wi.y, wi.k, m, [&](uint32_t root, uint64_t sbits) {
      const int idx = vmcore::find_slot(sh_slot, count, root);
      if (idx < 0) return;
      const int rank = (int)sh_rank[idx];
      const int32_t s0 = (wi.k << 6) + vmcore::ctz64(sbits), s1 = (wi.k << 6) + 63 - vmcore::clz64(sbits);
      if (cur >= 0 && rank != cur) {
        row_min(cur, lo);
        row_max(cur, hi);
        cur = -1;
      }
      if (cur < 0) cur = rank, lo = s0, hi = s1;
      else lo = min(lo, s0), hi = max(hi, s1);
    });
  // Neighbour lanes hold neighbour words: where the lane to the left has the same row and lesion its
  // minimum is the smaller one, where the lane to the right has, its maximum is the larger one.
  const uint32_t row = wi.valid ? (uint32_t)wi.z * (uint32_t)V.h + (uint32_t)wi.y : 0xFFFFFFFFu;
  const uint32_t row_l = (uint32_t)__shfl_up((int)row, 1, 64), row_r = (uint32_t)__shfl_down((int)row, 1, 64);
  const int cur_l = __shfl_up(cur, 1, 64), cur_r = __shfl_down(cur, 1, 64);
  if (cur < 0) return;
  if (!(lane > 0 && row_l == row && cur_l == cur)) row_min(cur, lo);
  if (!(lane < 63 && row_r == row && cur_r == cur)) row_max(cur, hi);
}

__global__ __launch_bounds__(kVdTile) void vd_tiles_kernel(Grid g, uint32_t ntmax, const LesionCtl* __restrict__ ctl,
                                                           const uint64_t* __restrict__ acc, const RowExt* __restrict__ table,
                                                           TileBox* __restrict__ tiles) {
  __shared__ int32_t sh[kVdTile / 64][6];
  const int rank = (int)(blockIdx.x / ntmax);
  const uint32_t tile = blockIdx.x - (uint32_t)rank * ntmax;
  if (rank >= (int)ctl->count) return;
  const Rows rows = lesion_rows(acc, rank);
  if (tile >= rows.tiles()) return;
  TileBox t = vdcore::tile_none();
  const uint32_t r = tile * (uint32_t)kVdTile + threadIdx.x;
  if (r < rows.count()) {
    int y, z;
    rows.row(r, y, z);
    vdcore::tile_add(z, y, table[vdcore::row_index(rank, z, y, g.h, g.d)], t);
  }
  const int32_t v[6] = {wave_min_i32(t.x0), wave_min_i32(t.y0), wave_min_i32(t.z0),
                        wave_max_i32(t.x1), wave_max_i32(t.y1), wave_max_i32(t.z1)};
  if ((threadIdx.x & 63) == 0)
    for (int j = 0; j < 6; ++j) sh[threadIdx.x >> 6][j] = v[j];
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t o[6];
    for (int j = 0; j < 6; ++j) {
      o[j] = sh[0][j];
      for (int wv = 1; wv < kVdTile / 64; ++wv) o[j] = j < 3 ? min(o[j], sh[wv][j]) : max(o[j], sh[wv][j]);
    }
    tiles[(size_t)rank * ntmax + tile] = TileBox{o[0], o[1], o[2], o[3], o[4], o[5], {0, 0}};
  }
}

__global__ __launch_bounds__(kVmThreads) void vd_bound_kernel(Grid g, uint32_t bchunks, const LesionCtl* __restrict__ ctl,
                                                              const uint64_t* __restrict__ acc, const RowExt* __restrict__ table,
                                                              Extreme* __restrict__ bpart) {
  constexpr int kPts = 2 * vdcore::kNumDirs;
  __shared__ Extreme sh_w[kVmWaves][kPts];
  const int rank = (int)(blockIdx.x / bchunks);
  const uint32_t chunk = blockIdx.x - (uint32_t)rank * bchunks;
  if (rank >= (int)ctl->count) return;
  const Rows rows = lesion_rows(acc, rank);
  const uint32_t nrows = rows.count(), r0 = chunk * (uint32_t)kVdBoundRows;
  if (r0 >= nrows) return;
  const uint32_t r1 = min(nrows, r0 + (uint32_t)kVdBoundRows);
  // One pass over the chunk's rows: the extremes of the 13 directions, 26 voxels, in registers.
  Extreme e[kPts];
#pragma unroll
  for (int i = 0; i < kPts; ++i) e[i] = vdcore::extreme_none();
  for (uint32_t r = r0 + threadIdx.x; r < r1; r += kVmThreads) {
    int y, z;
    rows.row(r, y, z);
    const RowExt row = table[vdcore::row_index(rank, z, y, g.h, g.d)];
#pragma unroll
    for (int dir = 0; dir < vdcore::kNumDirs; ++dir) {
      int dx, dy, dz;
      vdcore::direction(dir, dx, dy, dz);
      vdcore::extreme_row(g, z, y, row, dx, dy, dz, e[2 * dir], e[2 * dir + 1]);
    }
  }
#pragma unroll
  for (int i = 0; i < kPts; ++i) {
    const Extreme w = wave_extreme(e[i]);
    if ((threadIdx.x & 63) == 0) sh_w[threadIdx.x >> 6][i] = w;
  }
  __syncthreads();
  if (threadIdx.x < kPts) {  // the chunk's 26 extremes into its own slots, plain stores
    Extreme r = sh_w[0][threadIdx.x];
    for (int wv = 1; wv < kVmWaves; ++wv)
      if (vdcore::extreme_beats(sh_w[wv][threadIdx.x], r)) r = sh_w[wv][threadIdx.x];
    bpart[((size_t)rank * bchunks + chunk) * kPts + threadIdx.x] = r;
  }
}

// The axial bound: a wave per plane of a lesion — the extremes of the 4 directions of the plane over the plane's
// rows, the best pair among those 8 voxels — and one atomicMax (nobody reads its result) on the lesion's l2, which
// vd_init_kernel set to 0. A lesion's first workgroup first merges the chunks' 3D extremes of the launch before and
// stores l3, the best squared distance among the 26 voxels.
__global__ __launch_bounds__(kVmThreads) void vd_plane_bound_kernel(Grid g, uint32_t plane_blocks, uint32_t bchunks,
                                                                    const LesionCtl* __restrict__ ctl,
                                                                    const uint64_t* __restrict__ acc,
                                                                    const RowExt* __restrict__ table,
                                                                    const Extreme* __restrict__ bpart, uint64_t* __restrict__ bounds) {
  constexpr int kPts = 2 * vdcore::kNumPlaneDirs;
  constexpr int kPts3 = 2 * vdcore::kNumDirs;
  __shared__ uint32_t sh_pt[kPts3];
  __shared__ uint64_t sh_m[kVmWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rank = (int)(blockIdx.x / plane_blocks);
  if (rank >= (int)ctl->count) return;
  const Rows rows = lesion_rows(acc, rank);
  if (blockIdx.x == (uint32_t)rank * plane_blocks) {  // the whole workgroup
    const uint32_t used = (rows.count() + (uint32_t)kVdBoundRows - 1u) / (uint32_t)kVdBoundRows;  // chunks that wrote
    if (threadIdx.x < kPts3) {
      Extreme r = vdcore::extreme_none();
      for (uint32_t c = 0; c < used; ++c) {
        const Extreme x = bpart[((size_t)rank * bchunks + c) * kPts3 + threadIdx.x];
        if (vdcore::extreme_beats(x, r)) r = x;
      }
      sh_pt[threadIdx.x] = r.pos;
    }
    __syncthreads();
    uint64_t l3 = 0ull;
    for (int i = (int)threadIdx.x; i < kPts3 * kPts3; i += kVmThreads) {
      const uint64_t v = vdcore::extreme_d2(g, sh_pt[i / kPts3], sh_pt[i % kPts3], false);
      l3 = v > l3 ? v : l3;
    }
    l3 = block_max_u64<kVmWaves>(l3, sh_m);
    if (threadIdx.x == 0) bounds[2 * rank] = l3;
  }
  const int pz = (int)(blockIdx.x - (uint32_t)rank * plane_blocks) * kVmWaves + wave;  // the same in the whole wave
  if (pz >= rows.nz) return;
  const int z = rows.z0 + pz;
  Extreme e[kPts];
#pragma unroll
  for (int i = 0; i < kPts; ++i) e[i] = vdcore::extreme_none();
  for (int y = rows.y0 + lane; y < rows.y0 + rows.ny; y += 64) {
    const RowExt row = table[vdcore::row_index(rank, z, y, g.h, g.d)];
#pragma unroll
    for (int dir = 0; dir < vdcore::kNumPlaneDirs; ++dir) {
      int dx, dy, dz;
      vdcore::direction(dir, dx, dy, dz);
      vdcore::extreme_row(g, z, y, row, dx, dy, 0, e[2 * dir], e[2 * dir + 1]);
    }
  }
  uint32_t mine = vdcore::kNoPos;  // lane i < 8 keeps voxel i
#pragma unroll
  for (int i = 0; i < kPts; ++i) {
    const Extreme w = wave_extreme(e[i]);
    if (lane == i) mine = w.pos;
  }
  uint64_t l2 = 0ull;
#pragma unroll
  for (int j = 0; j < kPts; ++j) {
    const uint32_t other = (uint32_t)__shfl((int)mine, j, 64);
    const uint64_t v = vdcore::extreme_d2(g, mine, other, true);
    l2 = v > l2 ? v : l2;
  }
  l2 = wave_max_u64(l2);
  if (lane == 0 && l2)
    (void)__hip_atomic_fetch_max(&bounds[2 * rank + 1], l2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kVmThreads) void vd_pairs_kernel(Grid g, int nmax, uint32_t ntmax, int brute_force,
                                                              const LesionCtl* __restrict__ ctl, const uint64_t* __restrict__ acc,
                                                              const RowExt* __restrict__ table, const TileBox* __restrict__ tiles,
                                                              const uint64_t* __restrict__ bounds, Best* __restrict__ partial) {
  __shared__ Rows sh_rows[kMaxVolumeLesions];
  __shared__ uint64_t sh_first[kMaxVolumeLesions + 1];  // lesion r's tile pairs are items first[r] … first[r + 1]
  __shared__ uint64_t sh_l3[kMaxVolumeLesions], sh_l2[kMaxVolumeLesions];
  __shared__ Best sh_b3[kMaxVolumeLesions], sh_b2[kMaxVolumeLesions];
  __shared__ Cand sh_a[kVdCands], sh_b[kVdCands];
  __shared__ uint32_t sh_lr[kVmThreads], sh_li[kVmThreads], sh_lj[kVmThreads];  // the chunk's surviving pairs
  __shared__ uint32_t sh_wcnt[kVmWaves];
  __shared__ Best sh_red[kVmWaves];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int count = (int)min((uint32_t)nmax, ctl->count);  // the same in every thread
  if (t < count) {
    sh_rows[t] = lesion_rows(acc, t);
    sh_l3[t] = brute_force ? 0ull : bounds[2 * t];
    sh_l2[t] = brute_force ? 0ull : bounds[2 * t + 1];
    sh_b3[t] = vdcore::best_none(), sh_b2[t] = vdcore::best_none();
  }
  __syncthreads();
  if (t == 0) {
    uint64_t f = 0ull;
    for (int r = 0; r < count; ++r) {
      sh_first[r] = f;
      const uint64_t nt = sh_rows[r].tiles();
      f += nt * nt * (uint64_t)kVdSplit;
    }
    sh_first[count] = f;
  }
  __syncthreads();
  const uint64_t total = sh_first[count];
  // Item i belongs to workgroup i mod gridDim.x: the survivors, which come in runs of neighbouring J, spread over
  // the workgroups. A round gives every thread of every workgroup one item.
  for (uint64_t base = 0; base < total; base += (uint64_t)kVmThreads * gridDim.x) {
    // One tile pair per thread against the bounds.
    const uint64_t item = base + (uint64_t)t * gridDim.x + blockIdx.x;
    bool live = false;
    uint32_t lr = 0, li = 0, lj = 0;  // lj: tile J, and in its low bits which part of J's candidates
    if (item < total) {
      int lo = 0, hi = count - 1;  // the last lesion whose first item is ≤ item
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sh_first[mid] <= item) lo = mid;
        else hi = mid - 1;
      }
      lr = (uint32_t)lo;
      const uint32_t nt = sh_rows[lr].tiles();
      const uint64_t q = (item - sh_first[lr]) / (uint64_t)kVdSplit;
      const uint32_t part = (uint32_t)((item - sh_first[lr]) - q * (uint64_t)kVdSplit);
      li = (uint32_t)(q / nt), lj = (uint32_t)(q - (uint64_t)li * nt);
      if (lj >= li) {
        const TileBox A = tiles[(size_t)lr * ntmax + li], B = tiles[(size_t)lr * ntmax + lj];
        live = !vdcore::tile_pair_skipped(A, B, g, sh_l3[lr], sh_l2[lr]);
      }
      lj = lj * (uint32_t)kVdSplit + part;
    }
    const uint64_t mask = __ballot(live);
    if (lane == 0) sh_wcnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t off = 0, nlist = 0;
    for (int wv = 0; wv < kVmWaves; ++wv) {
      if (wv < wave) off += sh_wcnt[wv];
      nlist += sh_wcnt[wv];
    }
    if (live) {
      off += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      sh_lr[off] = lr, sh_li[off] = li, sh_lj[off] = lj;
    }
    __syncthreads();
    // The survivors one after the other: thread t holds candidate t of tile I against its part of tile J.
    for (uint32_t s = 0; s < nlist; ++s) {
      const int rank = (int)sh_lr[s];
      const Rows rows = sh_rows[rank];
      auto cand_of = [&](uint32_t tile) {
        Cand c{0u, 0u, 0u, vdcore::kNoPos};
        const uint32_t r = tile * (uint32_t)kVdTile + (uint32_t)(t >> 1);
        if (r < rows.count()) {
          int y, z;
          rows.row(r, y, z);
          const RowExt e = table[vdcore::row_index(rank, z, y, g.h, g.d)];
          if (e.lo <= e.hi && !((t & 1) && e.lo == e.hi)) c = g.cand((t & 1) ? e.hi : e.lo, y, z);
        }
        return c;
      };
      sh_a[t] = cand_of(sh_li[s]);
      sh_b[t] = cand_of(sh_lj[s] / (uint32_t)kVdSplit);
      const int j0 = (int)(sh_lj[s] % (uint32_t)kVdSplit) * (kVdCands / kVdSplit);
      __syncthreads();
      // The candidates of a tile stand in raster order, so of equal lengths the first met is the one to keep: a
      // strict comparison of d² + 1 (0 = not a pair to look at) is the whole tie rule inside a thread.
      const Cand a = sh_a[t];
      uint64_t v3 = 0ull, v2 = 0ull;
      uint32_t p3 = vdcore::kNoPos, p2 = vdcore::kNoPos;
      if (a.pos != vdcore::kNoPos) {
#pragma unroll 4
        for (int j = j0; j < j0 + kVdCands / kVdSplit; ++j) {
          const Cand b = sh_b[j];
          uint64_t w3, w2;
          vdcore::pair_values(a, b, w3, w2);
          if (w3 > v3) v3 = w3, p3 = b.pos;
          if (w2 > v2) v2 = w2, p2 = b.pos;
        }
      }
      Best b3 = v3 ? Best{v3 - 1ull, ((uint64_t)a.pos << 32) | p3} : vdcore::best_none();
      Best b2 = v2 ? Best{v2 - 1ull, ((uint64_t)a.pos << 32) | p2} : vdcore::best_none();
      b3 = block_best<kVmWaves>(b3, sh_red);
      b2 = block_best<kVmWaves>(b2, sh_red);  // its barriers also free sh_a / sh_b for the next pair
      if (t == 0) vdcore::best_take(b3, sh_b3[rank]), vdcore::best_take(b2, sh_b2[rank]);
    }
    __syncthreads();
  }
  __syncthreads();
  if (t < count) {
    Best* p = partial + ((size_t)blockIdx.x * (size_t)nmax + (size_t)t) * 2;
    p[0] = sh_b3[t], p[1] = sh_b2[t];
  }
}

__global__ __launch_bounds__(kVdFinalThreads) void vd_final_kernel(Grid g, int nmax, uint32_t pair_grid,
                                                                   const LesionCtl* __restrict__ ctl,
                                                                   const uint64_t* __restrict__ acc, const RowExt* __restrict__ table,
                                                                   const Best* __restrict__ partial,
                                                                   VolumeLesionDiameters* __restrict__ out) {
  constexpr int kWaves = kVdFinalThreads / 64;
  __shared__ Best sh_b[kWaves];
  __shared__ Extreme sh_e[kWaves];
  const int rank = (int)blockIdx.x;  // one workgroup per record, rank < nmax
  if (rank >= (int)ctl->count) {
    if (threadIdx.x == 0) out[rank] = VolumeLesionDiameters{};
    return;
  }
  Best b3 = vdcore::best_none(), b2 = vdcore::best_none();
  for (uint32_t w = threadIdx.x; w < pair_grid; w += kVdFinalThreads) {
    const Best* p = partial + ((size_t)w * (size_t)nmax + (size_t)rank) * 2;
    vdcore::best_take(p[0], b3);
    vdcore::best_take(p[1], b2);
  }
  b3 = block_best<kWaves>(b3, sh_b);
  b2 = block_best<kWaves>(b2, sh_b);
  if (b3.key == ~0ull || b2.key == ~0ull) {  // cannot happen (a lesion has a voxel); never decode "no pair"
    if (threadIdx.x == 0) out[rank] = VolumeLesionDiameters{};
    return;
  }
  int32_t xa, ya, za, xb, yb, zb;
  g.voxel((uint32_t)(b2.key >> 32), xa, ya, za);
  g.voxel((uint32_t)b2.key, xb, yb, zb);
  // The perpendicular: the row extremes of plane axial_z projected on the normal of b − a.
  const Rows rows = lesion_rows(acc, rank);
  const int32_t dx = xb - xa, dy = yb - ya;
  Extreme hi = vdcore::extreme_none(), lo = vdcore::extreme_none();
  for (int y = rows.y0 + (int)threadIdx.x; y < rows.y0 + rows.ny; y += kVdFinalThreads) {
    const RowExt e = table[vdcore::row_index(rank, za, y, g.h, g.d)];
    if (e.lo > e.hi) continue;
    for (int s = 0; s < 2; ++s) {
      const int32_t x = s ? e.hi : e.lo;
      const int64_t p = vdcore::perp_proj(dx, dy, x, y);
      const Extreme c{p, g.pos(x, y, za)}, n{-p, g.pos(x, y, za)};
      if (vdcore::extreme_beats(c, hi)) hi = c;
      if (vdcore::extreme_beats(n, lo)) lo = n;
    }
  }
  hi = block_extreme<kWaves>(hi, sh_e);
  lo = block_extreme<kWaves>(lo, sh_e);
  if (threadIdx.x != 0) return;
  VolumeLesionDiameters r = {};
  r.major_um2 = b3.d2;
  r.axial_um2 = b2.d2;
  r.axial_perp_extent = hi.proj + lo.proj;  // max p − min p
  g.voxel((uint32_t)(b3.key >> 32), r.major[0], r.major[1], r.major[2]);
  g.voxel((uint32_t)b3.key, r.major[3], r.major[4], r.major[5]);
  r.axial_z = za;
  r.axial[0] = xa, r.axial[1] = ya, r.axial[2] = xb, r.axial[3] = yb;
  int32_t z;
  g.voxel(lo.pos, r.axial_perp[0], r.axial_perp[1], z);
  g.voxel(hi.pos, r.axial_perp[2], r.axial_perp[3], z);
  out[rank] = r;
}

namespace {
struct VdLayout {
  size_t table, bounds, tiles, bpart, partial, total;
  uint32_t ntmax, pair_grid, bchunks;
};
// The work buffer: the row table, the bounds, the tile boxes, the partial slots of the pairs launch.
VdLayout vd_layout(int w, int h, int d, int nmax) {
  (void)w;
  VdLayout l;
  const uint64_t rows = (uint64_t)h * (uint64_t)d;
  l.ntmax = (uint32_t)((rows + kVdTile - 1) / kVdTile);
  l.bchunks = (uint32_t)((rows + kVdBoundRows - 1) / kVdBoundRows);
  const uint64_t chunks = ((uint64_t)nmax * l.ntmax * l.ntmax * kVdSplit + kVmThreads - 1) / kVmThreads;
  l.pair_grid = (uint32_t)(chunks < (uint64_t)kVdPairGrid ? chunks : (uint64_t)kVdPairGrid);
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  l.table = 0;
  l.bounds = up((size_t)nmax * rows * sizeof(RowExt));
  l.tiles = l.bounds + up((size_t)kMaxVolumeLesions * 2 * sizeof(uint64_t));
  l.bpart = l.tiles + up((size_t)nmax * l.ntmax * sizeof(TileBox));
  l.partial = l.bpart + up((size_t)nmax * l.bchunks * 2 * vdcore::kNumDirs * sizeof(Extreme));
  l.total = l.partial + up((size_t)l.pair_grid * (size_t)nmax * 2 * sizeof(Best));
  return l;
}
}  // namespace

size_t volume_diameters_work_bytes(int w, int h, int d, int max_lesions) {
  if (w <= 0 || h <= 0 || d <= 0 || max_lesions < 1 || max_lesions > kMaxVolumeLesions) return 0;
  return vd_layout(w, h, d, max_lesions).total;
}

void validate_volume_diameters(const uint64_t* dilated, int w, int h, int d, const uint32_t* scratch,
                                const VolumeLesionWork& lesions) {
  const VolumeDiametersWork* dw = lesions.diameters;
  if (!dw) throw DeviceError("launch_volume_diameters: no diameter work");
  if (lesions.max_lesions < 1 || lesions.max_lesions > kMaxVolumeLesions)
    throw DeviceError("launch_volume_diameters: lesions must be 1.." + std::to_string(kMaxVolumeLesions));
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("launch_volume_diameters: empty volume");
  if (volume_measure_scratch_words(w, h, d) == 0)
    throw DeviceError("launch_volume_diameters: a " + std::to_string(w) + " x " + std::to_string(h) + " x " +
                      std::to_string(d) + " volume is too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
  for (int a = 0; a < 3; ++a)
    if (dw->spacing_um[a] < 1u) throw DeviceError("launch_volume_diameters: a spacing must be at least 1 um");
  const std::string ext = measure::volume_diameters_extent_error(w, h, d, dw->spacing_um);
  if (!ext.empty()) throw DeviceError("launch_volume_diameters: " + ext);
  if (!dilated || !scratch || !lesions.work || !dw->work || !dw->out) throw DeviceError("launch_volume_diameters: null buffer");
  const VdLayout l = vd_layout(w, h, d, lesions.max_lesions);
  const uint64_t entries = (uint64_t)lesions.max_lesions * (uint64_t)h * (uint64_t)d;
  if ((entries + kVmThreads - 1) / kVmThreads > 0x7FFFFFFFull || (uint64_t)lesions.max_lesions * l.ntmax > 0x7FFFFFFFull ||
      (uint64_t)lesions.max_lesions * (((uint64_t)d + kVmWaves - 1) / kVmWaves) > 0x7FFFFFFFull)
    throw DeviceError("launch_volume_diameters: too many rows for " + std::to_string(lesions.max_lesions) + " lesions");
}

void launch_volume_diameters(const uint64_t* dilated, int w, int h, int d, const uint32_t* scratch,
                             const VolumeLesionWork& lesions, hipStream_t stream) {
  validate_volume_diameters(dilated, w, h, d, scratch, lesions);
  const VolumeDiametersWork* dw = lesions.diameters;
  const int n = (w + 63) / 64, nmax = lesions.max_lesions;
  const uint64_t words = (uint64_t)n * (uint64_t)h * (uint64_t)d;
  const uint32_t word_grid = (uint32_t)((words + kVmThreads - 1) / kVmThreads);
  const VdLayout l = vd_layout(w, h, d, nmax);
  const uint64_t entries = (uint64_t)nmax * (uint64_t)h * (uint64_t)d;
  const uint64_t init_grid = (entries + kVmThreads - 1) / kVmThreads, tile_grid = (uint64_t)nmax * l.ntmax;
  const uint32_t plane_blocks = ((uint32_t)d + kVmWaves - 1) / kVmWaves;
  const BitVolume M{dilated, w, h, d, n, false};
  const Grid g{w, h, d, dw->spacing_um[0], dw->spacing_um[1], dw->spacing_um[2]};
  const uint8_t* kbase = static_cast<const uint8_t*>(lesions.work);
  const uint64_t* acc = reinterpret_cast<const uint64_t*>(kbase);
  const LesionCtl* ctl = reinterpret_cast<const LesionCtl*>(kbase + kVlAccBytes);
  uint8_t* base = static_cast<uint8_t*>(dw->work);
  RowExt* table = reinterpret_cast<RowExt*>(base + l.table);
  uint64_t* bounds = reinterpret_cast<uint64_t*>(base + l.bounds);
  TileBox* tiles = reinterpret_cast<TileBox*>(base + l.tiles);
  Extreme* bpart = reinterpret_cast<Extreme*>(base + l.bpart);
  Best* partial = reinterpret_cast<Best*>(base + l.partial);
  uint32_t* labels = const_cast<uint32_t*>(scratch);  // read only: DeviceParents' loads take a plain pointer
  vd_init_kernel<<<(uint32_t)init_grid, kVmThreads, 0, stream>>>(g, nmax, ctl, acc, table, bounds);
  check_launch("vd_init_kernel");
  vd_rows_kernel<<<word_grid, kVmThreads, 0, stream>>>(M, labels, ctl, table);
  check_launch("vd_rows_kernel");
  vd_tiles_kernel<<<(uint32_t)tile_grid, kVdTile, 0, stream>>>(g, l.ntmax, ctl, acc, table, tiles);
  check_launch("vd_tiles_kernel");
  vd_bound_kernel<<<(uint32_t)nmax * l.bchunks, kVmThreads, 0, stream>>>(g, l.bchunks, ctl, acc, table, bpart);
  check_launch("vd_bound_kernel");
  vd_plane_bound_kernel<<<(uint32_t)nmax * plane_blocks, kVmThreads, 0, stream>>>(g, plane_blocks, l.bchunks, ctl, acc, table,
                                                                                 bpart, bounds);
  check_launch("vd_plane_bound_kernel");
  vd_pairs_kernel<<<l.pair_grid, kVmThreads, 0, stream>>>(g, nmax, l.ntmax, dw->brute_force ? 1 : 0, ctl, acc, table, tiles,
                                                          bounds, partial);
  check_launch("vd_pairs_kernel");
  vd_final_kernel<<<nmax, kVdFinalThreads, 0, stream>>>(g, nmax, l.pair_grid, ctl, acc, table, partial, dw->out);
  check_launch("vd_final_kernel");
}

void preload_volume_diameters() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&vd_init_kernel), reinterpret_cast<const void*>(&vd_rows_kernel),
                        reinterpret_cast<const void*>(&vd_tiles_kernel), reinterpret_cast<const void*>(&vd_bound_kernel),
                        reinterpret_cast<const void*>(&vd_plane_bound_kernel),
                        reinterpret_cast<const void*>(&vd_pairs_kernel), reinterpret_cast<const void*>(&vd_final_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume diameter kernels");
}

}  // namespace nm03::gpu
