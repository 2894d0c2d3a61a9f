// K7 — per-slice measurements of the dilated mask (nm03/measure.h, --measure): ONE WORKGROUP PER
// SLICE, descriptor-driven like K2, on the bit planes K2 leaves (u64 words, LSB = left-most pixel).
//
// Phase A, word-parallel: each thread owns words of the plane. Area, bounding box, coordinate sums,
// perimeter edges (m & ~(m << 1) and friends, with the neighbour words' carry bits and the rows above
// and below) and the bit-quad counts are integer word operations. The intensity statistics walk the
// set bits by the wave: its non-empty words in turn, lane = bit, so a word's samples are one coalesced
// load. The last word of a row is masked to the width. Wave reductions, then one LDS step across the waves.
//
// Phases B–D, labelling: union-find whose nodes are the HORIZONTAL RUNS of the mask, named by the
// linear index of their first pixel (so a component's label is its smallest index). A run needs no
// merge within its row; only contacts with the row above do, and a contact between two runs needs
// one union however long it is: the first bit of every stretch of m & above (vertical contacts) and,
// at 8-connectivity, the diagonal contacts that no vertical one already implies. A union is the
// atomicMin form (Komura): find both roots, atomicMin the smaller into the larger root's parent, and
// if another thread got there first carry on with what it wrote; finds halve the paths they walk. The
// forest is then flattened by pointer jumping (every run at its grandparent until a round changes
// nothing: about log2 of the deepest path rounds, a workgroup barrier each), every in-word stretch of a
// run adds its length at its root (atomicAdd), and the roots are counted and their areas maximised.
// The run's parent sits at its first pixel's slot of `scratch`, its area one slot further — free,
// because the pixel right of a run's first pixel never starts a run (rows are w + 1 slots apart).
//
// No thread waits on another thread's progress except at workgroup barriers: a find walks strictly
// decreasing indices, a failed union continues from a strictly smaller pair, a run-start search
// walks left through at most the row's words, a flatten round strictly lowers some parent or is the
// last. Every loop is bounded by the data; nothing spins on a flag. The results are integers that do not depend on the order of the unions.
#include <hip/hip_runtime.h>

#include "device_util.h"
#include "measure_util.h"
#include "nm03/gpu_types.h"
#include "nm03/kernels.h"
#include "nm03/measure.h"

namespace nm03::gpu {

constexpr int kMeasureThreads = 1024;
constexpr int kMeasureWaves = kMeasureThreads / 64;

namespace {

// Σ of the positions of the set bits of m: six masked popcounts (bit j of the position).
__device__ __forceinline__ uint32_t bit_position_sum(uint64_t m) {
  return (uint32_t)__popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2u * (uint32_t)__popcll(m & 0xCCCCCCCCCCCCCCCCull) +
         4u * (uint32_t)__popcll(m & 0xF0F0F0F0F0F0F0F0ull) + 8u * (uint32_t)__popcll(m & 0xFF00FF00FF00FF00ull) +
         16u * (uint32_t)__popcll(m & 0xFFFF0000FFFF0000ull) + 32u * (uint32_t)__popcll(m & 0xFFFFFFFF00000000ull);
}

// Root of x, halving the path on the way: a node passed over is pointed at its grandparent with an
// atomicMin that returns nothing (no wait), so parents only ever decrease and stay ancestors.
__device__ __forceinline__ uint32_t find_root(uint32_t* par, uint32_t x) {
  uint32_t p = ld(par + x);
  while (p != x) {  // parents are strictly smaller than their children: at most x steps
    const uint32_t g = ld(par + p);
    if (g != p) (void)__hip_atomic_fetch_min(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

// Union of the runs a and b. After a failed atomicMin (another thread lowered the parent of `a`
// first, to `old` < a) the link a → old stands or has been replaced by a → b; either way joining old
// and b restores what is owed, and max(a, b) has strictly decreased: the loop ends.
__device__ __forceinline__ void unite(uint32_t* par, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(par, a);
    b = find_root(par, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicMin(par + a, b);
    if (old == a) return;
    a = old;
  }
}

}  // namespace

__global__ __launch_bounds__(kMeasureThreads) void measure_kernel(const uint64_t* __restrict__ dilated,
                                                                  const uint64_t* __restrict__ region,
                                                                  const uint16_t* __restrict__ raw,
                                                                  const SliceDesc* __restrict__ descs, int connectivity,
                                                                  SliceMeasure* __restrict__ out,
                                                                  uint32_t* __restrict__ scratch, size_t scratch_stride) {
  __shared__ uint64_t sh_u64[3][kMeasureWaves];   // sum_x, sum_y, raw_sum
  __shared__ uint32_t sh_u32[9][kMeasureWaves];   // area, region, perimeter, q1, q3, qd | components, largest
  __shared__ int32_t sh_i32[6][kMeasureWaves];    // x0, y0, raw_min (min) | x1, y1, raw_max (max)
  const SliceDesc d = descs[blockIdx.x];
  const int W = d.w, H = d.h, n = d.wpr, words = H * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Plane M{dilated + d.mask_off, W, H, n};
  const uint64_t* __restrict__ R = region + d.mask_off;
  const uint16_t* __restrict__ px = raw + d.raw_off;
  uint32_t* par = scratch + (size_t)blockIdx.x * scratch_stride;
  const uint32_t stride = (uint32_t)W + 1u;  // slots per row: the slot after a row's last pixel holds an area
  const bool full_last = (W & 63) == 0;
  // A slice that does not fit its scratch (the caller sized it for smaller slices) is not measured:
  // its record says so with components = 0xFFFFFFFF. Uniform over the workgroup, before any barrier.
  if ((size_t)stride * (size_t)H + 1 > scratch_stride || W <= 0 || H <= 0) {
    if (threadIdx.x == 0) {
      SliceMeasure r = {};
      r.components = 0xFFFFFFFFu;
      out[blockIdx.x] = r;
    }
    return;
  }

  // ---- phase A: word-parallel figures, and every run's parent = itself, area = 0 -----------------
  uint32_t area = 0, reg = 0, perim = 0;
  uint64_t sum_x = 0, sum_y = 0;
  int64_t raw_sum = 0;
  int32_t x0 = 0x7FFFFFFF, y0 = 0x7FFFFFFF, r0 = 0x7FFFFFFF, x1 = -1, y1 = -1, r1 = (int32_t)0x80000000;
  QuadCounts q;
  for (int base = 0; base < words; base += kMeasureThreads) {  // the same trips for every wave (ballot below)
    const int i = base + (int)threadIdx.x;
    uint64_t m = 0ull;
    uint32_t row_off = 0;  // sample offset of the word's first pixel
    if (i < words) {
      const int y = i / n, k = i - y * n;
      m = M.at(y, k);
      row_off = (uint32_t)y * (uint32_t)W + (uint32_t)(k << 6);
      const uint64_t ml = M.at(y, k - 1), mr = M.at(y, k + 1);
      const uint64_t a = M.at(y - 1, k), al = M.at(y - 1, k - 1), dn = M.at(y + 1, k);
      reg += (uint32_t)__popcll(R[i] & row_word_mask(k, W));
      // Windows of the row pair (y − 1, y); the last row also closes the pair (H − 1, padding).
      quad_word(al, a, ml, m, full_last && k == n - 1, q);
      if (y == H - 1) quad_word(ml, m, 0ull, 0ull, full_last && k == n - 1, q);
      if (m != 0ull) {
        const uint32_t c = (uint32_t)__popcll(m);
        area += c;
        sum_x += (uint64_t)c * (uint32_t)(k << 6) + bit_position_sum(m);
        sum_y += (uint64_t)c * (uint32_t)y;
        x0 = min(x0, (k << 6) + (int)__ffsll((long long)m) - 1);
        x1 = max(x1, (k << 6) + 63 - (int)__clzll((long long)m));
        y0 = min(y0, y);
        y1 = max(y1, y);
        const uint64_t starts = m & ~((m << 1) | (ml >> 63));
        perim += (uint32_t)__popcll(starts) + (uint32_t)__popcll(m & ~((m >> 1) | (mr << 63))) +
                 (uint32_t)__popcll(m & ~a) + (uint32_t)__popcll(m & ~dn);
        for (uint64_t t = starts; t; t &= t - 1) {
          const uint32_t s = (uint32_t)y * stride + (uint32_t)((k << 6) + __ffsll((long long)t) - 1);
          st(par + s, s);
          st(par + s + 1, 0u);
        }
      }
    }
    // Intensities, by the wave: each of its non-empty words in turn, lane = bit, so a word's samples are
    // one coalesced 128-byte load; four words per round keep four loads in flight.
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
      for (int u = 0; u < 4; ++u) rv[u] = ((mj[u] >> lane) & 1ull) ? px[oj[u] + (uint32_t)lane] : (uint16_t)0;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if ((mj[u] >> lane) & 1ull) {
          const int32_t v = stored_sample(rv[u], d.type, d.stored_bits);
          raw_sum += v;
          r0 = min(r0, v);
          r1 = max(r1, v);
        }
    }
  }
  {
    const uint64_t s0 = wave_sum_u64(sum_x), s1 = wave_sum_u64(sum_y), s2 = wave_sum_u64((uint64_t)raw_sum);
    const uint32_t u0 = wave_sum_u32(area), u1 = wave_sum_u32(reg), u2 = wave_sum_u32(perim), u3 = wave_sum_u32(q.q1),
                   u4 = wave_sum_u32(q.q3), u5 = wave_sum_u32(q.qd);
    const int32_t i0 = wave_min_i32(x0), i1 = wave_min_i32(y0), i2 = wave_min_i32(r0), i3 = wave_max_i32(x1),
                  i4 = wave_max_i32(y1), i5 = wave_max_i32(r1);
    if (lane == 0) {
      sh_u64[0][wave] = s0, sh_u64[1][wave] = s1, sh_u64[2][wave] = s2;
      sh_u32[0][wave] = u0, sh_u32[1][wave] = u1, sh_u32[2][wave] = u2, sh_u32[3][wave] = u3, sh_u32[4][wave] = u4,
      sh_u32[5][wave] = u5;
      sh_i32[0][wave] = i0, sh_i32[1][wave] = i1, sh_i32[2][wave] = i2, sh_i32[3][wave] = i3, sh_i32[4][wave] = i4,
      sh_i32[5][wave] = i5;
    }
  }
  __syncthreads();  // every run's parent and area slot are initialised

  // ---- phase B: unions with the row above -----------------------------------------------------------
  for (int i = threadIdx.x + n; i < words; i += kMeasureThreads) {  // rows 1 … H − 1
    const int y = i / n, k = i - y * n;
    const uint64_t m = M.at(y, k);
    if (m == 0ull) continue;
    const uint64_t a = M.at(y - 1, k);
    const int xb = k << 6;
    // Vertical contacts: the first bit of every stretch of m & a (a stretch lies in one run of each row).
    const uint64_t v = m & a;
    for (uint64_t t = v & ~(v << 1); t; t &= t - 1) {
      const int x = xb + __ffsll((long long)t) - 1;
      unite(par, (uint32_t)y * stride + (uint32_t)M.run_start(y, x), (uint32_t)(y - 1) * stride + (uint32_t)M.run_start(y - 1, x));
    }
    if (connectivity == 8) {
      const uint64_t ml = M.at(y, k - 1), mr = M.at(y, k + 1), al = M.at(y - 1, k - 1), ar = M.at(y - 1, k + 1);
      // Pixel x touching (y − 1, x − 1): owed only when neither (y − 1, x) nor (y, x − 1) is set (either
      // one already links the two runs through a vertical contact or by being the same run).
      const uint64_t ul = m & ((a << 1) | (al >> 63)) & ~a & ~((m << 1) | (ml >> 63));
      for (uint64_t t = ul; t; t &= t - 1) {
        const int x = xb + __ffsll((long long)t) - 1;
        unite(par, (uint32_t)y * stride + (uint32_t)M.run_start(y, x), (uint32_t)(y - 1) * stride + (uint32_t)M.run_start(y - 1, x - 1));
      }
      const uint64_t ur = m & ((a >> 1) | (ar << 63)) & ~a & ~((m >> 1) | (mr << 63));
      for (uint64_t t = ur; t; t &= t - 1) {
        const int x = xb + __ffsll((long long)t) - 1;
        unite(par, (uint32_t)y * stride + (uint32_t)M.run_start(y, x), (uint32_t)(y - 1) * stride + (uint32_t)M.run_start(y - 1, x + 1));
      }
    }
  }
  __syncthreads();  // the forest is final

  // ---- phase C: flatten by pointer jumping (every run at its grandparent, until a round changes nothing:
  // about log2 of the deepest path rounds, each ended by a workgroup barrier), then every in-word stretch
  // of a run adds its length at its root ------------------------------------------------------------------
  for (int changed = 1; changed;) {
    changed = 0;
    for (int i = threadIdx.x; i < words; i += kMeasureThreads) {
      const int y = i / n, k = i - y * n;
      const uint64_t m = M.at(y, k);
      if (m == 0ull) continue;
      const uint64_t ml = M.at(y, k - 1);
      for (uint64_t t = m & ~((m << 1) | (ml >> 63)); t; t &= t - 1) {
        const uint32_t s = (uint32_t)y * stride + (uint32_t)((k << 6) + __ffsll((long long)t) - 1);
        const uint32_t p = ld(par + s);
        if (p == s) continue;
        const uint32_t g = ld(par + p);
        if (g == p) continue;
        st(par + s, g);  // an ancestor still; a reader of this round sees p or g
        changed = 1;
      }
    }
    changed = __syncthreads_or(changed);
  }
  for (int i = threadIdx.x; i < words; i += kMeasureThreads) {
    const int y = i / n, k = i - y * n;
    const uint64_t m = M.at(y, k);
    if (m == 0ull) continue;
    const int xb = k << 6;
    for (uint64_t t = m & ~(m << 1); t; t &= t - 1) {
      const int b = __ffsll((long long)t) - 1;
      const uint64_t rest = ~(m >> b);  // bit j clear while pixel b + j is set
      const uint32_t len = rest == 0ull ? 64u - (uint32_t)b : min((uint32_t)__ffsll((long long)rest) - 1u, 64u - (uint32_t)b);
      const uint32_t s = (uint32_t)y * stride + (uint32_t)M.run_start(y, xb + b);
      atomicAdd(par + ld(par + s) + 1, len);  // flattened: a run's parent is its root
    }
  }
  __syncthreads();  // areas are final

  // ---- phase D: count the roots, take the largest area ------------------------------------------------
  uint32_t comps = 0, largest = 0;
  for (int i = threadIdx.x; i < words; i += kMeasureThreads) {
    const int y = i / n, k = i - y * n;
    const uint64_t m = M.at(y, k);
    if (m == 0ull) continue;
    const uint64_t ml = M.at(y, k - 1);
    for (uint64_t t = m & ~((m << 1) | (ml >> 63)); t; t &= t - 1) {
      const uint32_t s = (uint32_t)y * stride + (uint32_t)((k << 6) + __ffsll((long long)t) - 1);
      if (ld(par + s) != s) continue;
      ++comps;
      largest = max(largest, ld(par + s + 1));
    }
  }
  comps = wave_sum_u32(comps);
  largest = wave_max_u32(largest);
  if (lane == 0) sh_u32[6][wave] = comps, sh_u32[7][wave] = largest;
  __syncthreads();

  if (threadIdx.x == 0) {
    uint64_t s0 = 0, s1 = 0, s2 = 0;
    uint32_t u[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int32_t mn[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, mx[3] = {-1, -1, (int32_t)0x80000000};
    for (int wv = 0; wv < kMeasureWaves; ++wv) {
      s0 += sh_u64[0][wv], s1 += sh_u64[1][wv], s2 += sh_u64[2][wv];
      for (int j = 0; j < 7; ++j) u[j] += sh_u32[j][wv];
      u[7] = max(u[7], sh_u32[7][wv]);
      for (int j = 0; j < 3; ++j) mn[j] = min(mn[j], sh_i32[j][wv]), mx[j] = max(mx[j], sh_i32[3 + j][wv]);
    }
    QuadCounts qt;
    qt.q1 = u[3], qt.q3 = u[4], qt.qd = u[5];
    const bool any = u[0] > 0;
    SliceMeasure r = {};
    r.area_px = u[0];
    r.region_px = u[1];
    r.bbox[0] = any ? mn[0] : -1;
    r.bbox[1] = any ? mn[1] : -1;
    r.bbox[2] = any ? mx[0] : -1;
    r.bbox[3] = any ? mx[1] : -1;
    r.sum_x = s0;
    r.sum_y = s1;
    r.perimeter_edges = u[2];
    r.components = u[6];
    r.largest_px = u[7];
    r.holes = (uint32_t)((int64_t)u[6] - euler_from_quads(qt, connectivity));
    r.raw_sum = any ? (int64_t)s2 : 0;
    r.raw_min = any ? mn[2] : 0;
    r.raw_max = any ? mx[2] : 0;
    out[blockIdx.x] = r;
  }
}

size_t measure_scratch_words(int max_w, int max_h) {
  // One slot per pixel plus one per row (rows are w + 1 slots apart), one more for the last area slot.
  return (((size_t)max_w + 1) * (size_t)max_h + 1 + 3) & ~(size_t)3;
}

void launch_measure(const uint64_t* dilated, const uint64_t* region, const uint16_t* raw, const SliceDesc* descs, int nslices,
                    int connectivity, SliceMeasure* out, uint32_t* scratch, int max_w, int max_h, hipStream_t stream) {
  if (nslices <= 0) return;
  if (connectivity != 4 && connectivity != 8) throw DeviceError("launch_measure: connectivity must be 4 or 8");
  if (max_w <= 0 || max_h <= 0 || max_w > kMaxSliceDim || max_h > kMaxSliceDim)
    throw DeviceError("launch_measure: slice larger than " + std::to_string(kMaxSliceDim));
  if (!dilated || !region || !raw || !descs || !out || !scratch) throw DeviceError("launch_measure: null buffer");
  measure_kernel<<<nslices, kMeasureThreads, 0, stream>>>(dilated, region, raw, descs, connectivity, out, scratch,
                                                          measure_scratch_words(max_w, max_h));
  check_launch("measure_kernel");
}

void preload_measure() {
  hipFuncAttributes a;
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&measure_kernel)), "preload measure_kernel");
}

}  // namespace nm03::gpu
