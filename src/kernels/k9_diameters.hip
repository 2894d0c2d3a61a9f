// K9 — bidimensional diameters of the lesion (nm03/measure.h SliceDiameters, --measure-diameters): ONE
// WORKGROUP PER SLICE, descriptor-driven like K7 and launched directly after it. K7 leaves a finished
// labelling of the dilated plane in its scratch: the slot of every run's first pixel holds the run's
// root (the smallest slot of its component) and the slot after a root the component's area.
//
// Phase 1, the lesion: over the run starts that are roots, the maximum of (area, −slot).
// Phase 2, candidates: xlo[y] / xhi[y] in LDS, the leftmost and the rightmost LESION pixel of row y
//   (runs of other components in the row do not count): every in-word stretch whose run's root is the
//   lesion's does an LDS atomicMin / atomicMax. A component occupies consecutive rows, so the
//   candidates are the 2·R row extremes of rows ymin … ymax, in (y, x) order by construction. They hold
//   every convex-hull vertex of the lesion (a vertex is an extreme pixel of its row), hence a pair at
//   maximum distance, the extremes of every linear functional, and — the lexicographic minimum over
//   a hull edge being an endpoint — the pairs and points the tie-breaks ask for.
// Phase 3, major diameter: thread t owns the candidates i = t, t + 1024, … and compares each with
//   every candidate j ≥ i. A wave walks j from its first i, so the LDS reads are broadcasts. A strict
//   comparison keeps a thread's first, i.e. lexicographically smallest, best pair; across threads a
//   max reduction of d² and then a min reduction of the 48-bit key (ya, xa, yb, xb) of the pairs that
//   attain it (d² < 2²⁵ and the key do not fit one 64-bit word).
// Phase 4, perpendicular extent: p = −dy·x + dx·y over the candidates (|p| < 2²⁶); the minimum and the
//   maximum with their smallest (y, x) as min reductions of (p + 2²⁶ | y | x) and (2²⁶ − p | y | x).
// Phase 5: thread 0 writes the 64-byte record.
//
// Workgroup barriers are the only synchronisation; every loop is bounded by the data. The kernel
// writes nothing but its record, so K7's scratch stays as K7 left it.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "measure_util.h"
#include "nm03/gpu_types.h"
#include "nm03/kernels.h"
#include "nm03/measure.h"

namespace nm03::gpu {

constexpr int kDiamThreads = 1024;
constexpr int kDiamWaves = kDiamThreads / 64;

namespace {

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
  return ((uint64_t)hi << 32) | lo;
}

// Maximum / minimum of v over the workgroup, in every thread. `sh` (kDiamWaves words) is free again
// when the call returns.
__device__ __forceinline__ uint64_t block_max_u64(uint64_t v, uint64_t* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, shfl_xor_u64(v, o));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t r = sh[0];
#pragma unroll
  for (int k = 1; k < kDiamWaves; ++k) r = max(r, sh[k]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ uint64_t block_min_u64(uint64_t v, uint64_t* sh) { return ~block_max_u64(~v, sh); }

}  // namespace

__global__ __launch_bounds__(kDiamThreads) void diameters_kernel(const uint64_t* __restrict__ dilated,
                                                                 const SliceDesc* __restrict__ descs,
                                                                 SliceDiameters* __restrict__ out,
                                                                 const uint32_t* __restrict__ scratch, size_t scratch_stride) {
  __shared__ int32_t xlo[kMaxSliceDim], xhi[kMaxSliceDim];  // row extremes of the lesion (rows ymin … ymax)
  __shared__ uint64_t sh_red[kDiamWaves];
  __shared__ int32_t sh_y[2];  // ymin, ymax of the lesion
  const SliceDesc d = descs[blockIdx.x];
  const int W = d.w, H = d.h, n = d.wpr, words = H * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Plane M{dilated + d.mask_off, W, H, n};
  const uint32_t* __restrict__ par = scratch + (size_t)blockIdx.x * scratch_stride;
  const uint32_t stride = (uint32_t)W + 1u;  // K7's slots per row
  // A slice K7 did not label (it does not fit the scratch) is not measured either, and one beyond the
  // row arrays cannot be: the record says so. Uniform over the workgroup, before any barrier.
  if ((size_t)stride * (size_t)H + 1 > scratch_stride || W <= 0 || H <= 0 || W > kMaxSliceDim || H > kMaxSliceDim) {
    if (threadIdx.x == 0) {
      SliceDiameters r = {};
      r.lesion_px = kDiametersNotMeasured;
      out[blockIdx.x] = r;
    }
    return;
  }

  // ---- phase 1: the lesion's root: maximum area, then minimum slot ------------------------------------
  uint64_t best = 0ull;  // area << 32 | ~slot; 0 = no root (an area is at least 1)
  for (int i = threadIdx.x; i < words; i += kDiamThreads) {
    const int y = i / n, k = i - y * n;
    const uint64_t m = M.at(y, k);
    if (m == 0ull) continue;
    const uint64_t ml = M.at(y, k - 1);
    for (uint64_t t = m & ~((m << 1) | (ml >> 63)); t; t &= t - 1) {
      const uint32_t s = (uint32_t)y * stride + (uint32_t)((k << 6) + __ffsll((long long)t) - 1);
      if (par[s] != s) continue;
      best = max(best, ((uint64_t)par[s + 1] << 32) | (uint64_t)(0xFFFFFFFFu - s));
    }
  }
  for (int y = threadIdx.x; y < H; y += kDiamThreads) xlo[y] = 0x7FFFFFFF, xhi[y] = -1;
  if (threadIdx.x == 0) sh_y[0] = 0x7FFFFFFF, sh_y[1] = -1;
  best = block_max_u64(best, sh_red);  // its barriers also publish the initialised row arrays
  if (best == 0ull) {  // empty mask (uniform)
    if (threadIdx.x == 0) {
      SliceDiameters r = {};
      r.lesion_first[0] = r.lesion_first[1] = -1;
      for (int k = 0; k < 4; ++k) r.major[k] = r.perp[k] = -1;
      out[blockIdx.x] = r;
    }
    return;
  }
  const uint32_t root = 0xFFFFFFFFu - (uint32_t)best;
  const uint32_t lesion_px = (uint32_t)(best >> 32);

  // ---- phase 2: row extremes of the lesion -----------------------------------------------------------
  int32_t y0 = 0x7FFFFFFF, y1 = -1;
  for (int i = threadIdx.x; i < words; i += kDiamThreads) {
    const int y = i / n, k = i - y * n;
    const uint64_t m = M.at(y, k);
    if (m == 0ull) continue;
    const int xb = k << 6;
    for (uint64_t t = m & ~(m << 1); t; t &= t - 1) {  // in-word stretches
      const int b = __ffsll((long long)t) - 1;
      const uint32_t s = (uint32_t)y * stride + (uint32_t)M.run_start(y, xb + b);
      if (par[s] != root) continue;  // a run of another component
      const uint64_t rest = ~(m >> b);  // bit j clear while pixel b + j is set
      const int len = rest == 0ull ? 64 - b : min((int)__ffsll((long long)rest) - 1, 64 - b);
      atomicMin(&xlo[y], xb + b);
      atomicMax(&xhi[y], xb + b + len - 1);
      y0 = min(y0, y);
      y1 = max(y1, y);
    }
  }
  y0 = wave_min_i32(y0);
  y1 = wave_max_i32(y1);
  if (lane == 0 && y1 >= 0) {
    atomicMin(&sh_y[0], y0);
    atomicMax(&sh_y[1], y1);
  }
  __syncthreads();  // the candidates are final
  const int ymin = sh_y[0];
  const int R = sh_y[1] - ymin + 1;  // ≥ 1: the root's row holds a lesion run
  const int nc = 2 * R;              // candidate c: row ymin + c / 2, its left (c even) or right (c odd) extreme

  // ---- phase 3: the pair at maximum distance ---------------------------------------------------------
  int32_t bd2 = -1;
  uint64_t bkey = ~0ull;
  for (int ibase = 0; ibase < nc; ibase += kDiamThreads) {
    const int i = ibase + (int)threadIdx.x;
    const bool act = i < nc;
    const int yi = ymin + (min(i, nc - 1) >> 1);
    const int xi = (i & 1) ? xhi[yi] : xlo[yi];
    for (int rj = (ibase >> 1) + (wave << 5); rj < R; ++rj) {  // from the row of the wave's first i: uniform trips
      const int yj = ymin + rj;
      const int xl = xlo[yj], xh = xhi[yj];
      const int ey = yj - yi;
      if (act && 2 * rj >= i) {
        const int ex = xl - xi;
        const int32_t d2 = ex * ex + ey * ey;
        if (d2 > bd2) bd2 = d2, bkey = ((uint64_t)yi << 36) | ((uint64_t)xi << 24) | ((uint64_t)yj << 12) | (uint64_t)xl;
      }
      if (act && 2 * rj + 1 >= i) {
        const int ex = xh - xi;
        const int32_t d2 = ex * ex + ey * ey;
        if (d2 > bd2) bd2 = d2, bkey = ((uint64_t)yi << 36) | ((uint64_t)xi << 24) | ((uint64_t)yj << 12) | (uint64_t)xh;
      }
    }
  }
  const uint32_t major_px2 = (uint32_t)block_max_u64((uint64_t)(uint32_t)(bd2 + 1), sh_red) - 1u;  // candidate 0 pairs with itself
  const uint64_t key = block_min_u64((uint32_t)bd2 == major_px2 ? bkey : ~0ull, sh_red);
  const int ya = (int)(key >> 36) & 0xFFF, xa = (int)(key >> 24) & 0xFFF, yb = (int)(key >> 12) & 0xFFF, xb = (int)key & 0xFFF;

  // ---- phase 4: the projection on n = (−dy, dx) ------------------------------------------------------
  const int ex = xb - xa, ey = yb - ya;
  uint64_t kmin = ~0ull, kmax = ~0ull;
  for (int c = threadIdx.x; c < nc; c += kDiamThreads) {
    const int y = ymin + (c >> 1);
    const int x = (c & 1) ? xhi[y] : xlo[y];
    const int32_t p = -ey * x + ex * y;  // |p| < 2^26
    const uint64_t yx = ((uint64_t)y << 12) | (uint64_t)x;
    kmin = min(kmin, ((uint64_t)(uint32_t)(p + (1 << 26)) << 24) | yx);
    kmax = min(kmax, ((uint64_t)(uint32_t)((1 << 26) - p) << 24) | yx);
  }
  kmin = block_min_u64(kmin, sh_red);
  kmax = block_min_u64(kmax, sh_red);

  // ---- phase 5: the record --------------------------------------------------------------------------
  if (threadIdx.x == 0) {
    const int32_t pmin = (int32_t)(kmin >> 24) - (1 << 26), pmax = (1 << 26) - (int32_t)(kmax >> 24);
    SliceDiameters r = {};
    r.lesion_px = lesion_px;
    r.lesion_first[0] = (int32_t)(root % stride);
    r.lesion_first[1] = (int32_t)(root / stride);
    r.major_px2 = major_px2;
    r.perp_extent = (uint32_t)(pmax - pmin);
    r.major[0] = xa, r.major[1] = ya, r.major[2] = xb, r.major[3] = yb;
    r.perp[0] = (int32_t)kmin & 0xFFF, r.perp[1] = (int32_t)(kmin >> 12) & 0xFFF;
    r.perp[2] = (int32_t)kmax & 0xFFF, r.perp[3] = (int32_t)(kmax >> 12) & 0xFFF;
    out[blockIdx.x] = r;
  }
}

void launch_measure_diameters(const uint64_t* dilated, const SliceDesc* descs, int nslices, SliceDiameters* out,
                              const uint32_t* scratch, int max_w, int max_h, hipStream_t stream) {
  if (nslices <= 0) return;
  if (max_w <= 0 || max_h <= 0 || max_w > kMaxSliceDim || max_h > kMaxSliceDim)
    throw DeviceError("launch_measure_diameters: slice larger than " + std::to_string(kMaxSliceDim));
  if (!dilated || !descs || !out || !scratch) throw DeviceError("launch_measure_diameters: null buffer");
  diameters_kernel<<<nslices, kDiamThreads, 0, stream>>>(dilated, descs, out, scratch, measure_scratch_words(max_w, max_h));
  check_launch("diameters_kernel");
}

void preload_measure_diameters() {
  hipFuncAttributes a;
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&diameters_kernel)), "preload diameters_kernel");
}

}  // namespace nm03::gpu
