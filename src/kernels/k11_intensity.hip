// K11 — first-order intensity statistics of the samples under the dilated mask (nm03/measure.h
// IntensityStats, --measure-intensity): Σ v² and the exact 10th / 25th / 50th / 75th / 90th percentile.
//
// Exact order statistics of 16-bit samples are a histogram problem, and a full 16-bit histogram does
// not fit LDS, so the selection is a TWO-PASS RADIX SELECT (nm03/intensity_core.h): pass 1 histograms
// the high byte of every sample's key and sums the squares; the five target ranks are then located in
// the 256 bins (bin and the rank left inside it); pass 2 histograms the low byte of the samples whose
// high byte is a target's bin (targets in one bin share a histogram), and the five keys are resolved.
// Both passes walk the samples as K7 and K8 do: by the wave, each of its non-empty words in turn,
// lane = bit, so a word's samples are one coalesced 128-byte load, four loads in flight.
//
// Bin contention. A homogeneous lesion puts nearly every sample of a wave into one bin, and 64 LDS
// atomics on one address serialise. So the wave combines equal keys before it adds: up to kPeelRounds
// times the first remaining lane broadcasts its key, a ballot finds the lanes that hold the same key,
// and that lane alone adds their count; only lanes whose key is still unmatched after that add 1 each.
// A homogeneous word costs one atomic, a word of all-different keys 64 atomics on 64 addresses. In pass
// 1 every wave also has a private histogram (2D: 16 × 256 × 4 B = 16 KiB), so waves never meet on an
// address; pass 2 uses five shared histograms in the same LDS (5 KiB) with the same combining.
//
// 2D, intensity_kernel: ONE 1024-THREAD WORKGROUP PER SLICE, descriptor-driven like measure_kernel
// (SliceDesc::w, h, wpr, mask_off, raw_off, type, stored_bits; slices of different sizes in one launch).
// No global scratch. Workgroup barriers are the only synchronisation.
//
// 3D: FIVE LAUNCHES on the volume's stream in K8's style, 256-thread workgroups, a thread per u64 word
// (z, y, k): init (zero the accumulators), hist_hi (per-workgroup LDS histogram, then at most one global
// atomic per non-zero bin and workgroup), select (one workgroup), hist_lo (the same walk for the targets'
// bins), final (resolve, plain vector stores). Locating a rank in 256 bins is a wave's job everywhere
// (wave_select_bin), wave j for target j. No cooperative launch, no grid barrier, no flag, no
// look-back, no spin: the only cross-workgroup traffic is relaxed atomic adds on counters that nobody
// reads before the next kernel boundary. Every loop is bounded by the data.
#include <hip/hip_runtime.h>

#include <string>

#include "device_util.h"
#include "measure_util.h"
#include "nm03/gpu_types.h"
#include "nm03/intensity_core.h"
#include "nm03/kernels.h"
#include "nm03/measure.h"
#include "nm03/volume_measure_core.h"

namespace nm03::gpu {

constexpr int kIntensityThreads = 1024;
constexpr int kIntensityWaves = kIntensityThreads / 64;
constexpr int kViThreads = 256;  // K8's and K10's workgroup (volume_measure_util.h kVmThreads)
constexpr int kViWaves = kViThreads / 64;

namespace {

using icore::BinRank;
using icore::kBins;
using icore::kPercentiles;
using vmcore::BitVolume;

// Pass 1 of one word: Σ v², the count and the high-byte histogram.
__device__ __forceinline__ void pass_hi(uint64_t m, uint32_t off, const uint16_t* __restrict__ px, uint8_t type,
                                        uint8_t stored_bits, int lane, uint32_t* hist, uint64_t& sum_sq, uint32_t& count) {
  walk_samples(m, off, px, lane, [&](bool on, uint16_t rv) {
    uint32_t hi = 0u;
    if (on) {
      const int32_t v = stored_sample(rv, type, stored_bits);
      sum_sq += (uint64_t)((int64_t)v * (int64_t)v);
      ++count;
      hi = (uint32_t)icore::sample_key(v, type) >> 8;
    }
    wave_hist_add(hist, hi, on, lane);
  });
}

// Pass 2 of one word: the low-byte histogram `slot` of every sample whose high byte is a target's bin.
__device__ __forceinline__ void pass_lo(uint64_t m, uint32_t off, const uint16_t* __restrict__ px, uint8_t type,
                                        uint8_t stored_bits, int lane, const BinRank* t, uint32_t* hist) {
  walk_samples(m, off, px, lane, [&](bool on, uint16_t rv) {
    uint32_t idx = 0u;
    bool hit = false;
    if (on) {
      const uint32_t key = icore::sample_key(stored_sample(rv, type, stored_bits), type);
      const int s = icore::slot_of(t, key >> 8);
      hit = s >= 0;
      if (hit) idx = (uint32_t)s * (uint32_t)kBins + (key & 255u);
    }
    wave_hist_add(hist, idx, hit, lane);
  });
}

// icore::select_bin over kBins counters by ONE WAVE: lane l owns bins 4l … 4l + 3, a prefix sum over the
// lanes finds the lane whose bins hold the rank, and that lane finishes with select_bin on its four. (One
// thread walking 256 counters is 256 dependent LDS or L2 round trips: it cost more than both sample
// walks.) Counts and ranks stay below 2^32. Rank 0 (an empty mask) gives {0, 0}, as select_bin does.
__device__ __forceinline__ BinRank wave_select_bin(const uint32_t* hist, uint32_t rank, int lane) {
  static_assert(kBins == 4 * 64, "four bins a lane");
  uint32_t c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = hist[4 * lane + i];
  const uint32_t s = c[0] + c[1] + c[2] + c[3];
  const uint32_t inc = wave_inclusive_scan(s, lane), exc = inc - s;
  const bool mine = rank > exc && rank <= inc;  // at most one lane
  uint32_t bin = 0u, left = 0u;
  if (mine) {
    const BinRank l = icore::select_bin(c, 4, (uint64_t)(rank - exc));
    bin = 4u * (uint32_t)lane + l.bin;
    left = (uint32_t)l.rank;
  }
  const uint64_t who = __ballot(mine);
  const int src = who ? __ffsll((long long)who) - 1 : 0;
  BinRank r;
  r.bin = (uint32_t)__shfl((int)bin, src, 64);
  r.rank = (uint64_t)(uint32_t)__shfl((int)left, src, 64);
  return r;
}

// Percentile j from the located bins `t` and the low-byte histograms `lo` (kPercentiles × kBins), by one wave.
__device__ __forceinline__ int32_t wave_resolve(const BinRank* t, const uint32_t* lo, int j, uint8_t type, int lane) {
  const BinRank me = t[j];
  int slot = j;  // icore::share_slots: the first target of the same bin (read from memory: j is not a constant)
  while (slot > 0 && t[slot - 1].bin == me.bin) --slot;
  const BinRank l = wave_select_bin(lo + slot * kBins, (uint32_t)me.rank, lane);
  return icore::key_sample((uint16_t)((me.bin << 8) | l.bin), type);
}

// The accumulators of the 3D launches (device memory, kVolumeIntensityAccBytes).
struct ViAcc {
  uint64_t sum_sq, count;
  uint32_t hi[kBins];
  uint32_t lo[kPercentiles * kBins];
  BinRank target[kPercentiles];
};
static_assert(sizeof(ViAcc) <= kVolumeIntensityAccBytes && sizeof(ViAcc) % 4 == 0, "intensity accumulator layout");

// The thread's word (z, y, k) of the volume, as K8's my_word.
struct ViWord {
  uint64_t m;
  uint32_t off;
};
__device__ __forceinline__ ViWord vi_word(const BitVolume& V, uint32_t raw_plane_stride) {
  const uint32_t total = (uint32_t)V.d * (uint32_t)V.h * (uint32_t)V.n;  // < 2^32 (launch_volume_intensity)
  const uint32_t i = blockIdx.x * (uint32_t)kViThreads + threadIdx.x;
  ViWord w{0ull, 0u};
  if (i < total) {
    const uint32_t row = i / (uint32_t)V.n;
    const int k = (int)(i - row * (uint32_t)V.n);
    const int z = (int)(row / (uint32_t)V.h);
    const int y = (int)(row - (uint32_t)z * (uint32_t)V.h);
    w.m = V.at(z, y, k);
    w.off = (uint32_t)z * raw_plane_stride + (uint32_t)y * (uint32_t)V.w + (uint32_t)(k << 6);
  }
  return w;
}

__device__ __forceinline__ void add_u32(uint32_t* p, uint32_t v) {
  if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void add_u64(uint64_t* p, uint64_t v) {
  if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

__global__ __launch_bounds__(kIntensityThreads) void intensity_kernel(const uint64_t* __restrict__ dilated,
                                                                      const uint16_t* __restrict__ raw,
                                                                      const SliceDesc* __restrict__ descs,
                                                                      IntensityStats* __restrict__ out) {
  __shared__ uint32_t sh_hist[kIntensityWaves * kBins];  // pass 1: a histogram per wave; pass 2: kPercentiles shared ones
  __shared__ uint32_t sh_hi[kBins];
  __shared__ uint64_t sh_sq[kIntensityWaves];
  __shared__ uint32_t sh_cnt[kIntensityWaves];
  __shared__ BinRank sh_t[kPercentiles];
  __shared__ int32_t sh_pct[kPercentiles];
  static_assert(kPercentiles * kBins <= kIntensityWaves * kBins, "pass 2 reuses pass 1's histograms");
  const SliceDesc d = descs[blockIdx.x];
  const int W = d.w, H = d.h, n = d.wpr, words = H * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (W <= 0 || H <= 0) {  // uniform over the workgroup, before any barrier
    if (threadIdx.x == 0) out[blockIdx.x] = IntensityStats{};
    return;
  }
  const Plane M{dilated + d.mask_off, W, H, n};
  const uint16_t* __restrict__ px = raw + d.raw_off;
  for (int i = threadIdx.x; i < kIntensityWaves * kBins; i += kIntensityThreads) sh_hist[i] = 0u;
  __syncthreads();

  // ---- pass 1: Σ v², the count, the high bytes ---------------------------------------------------------
  uint64_t sum_sq = 0;
  uint32_t count = 0;
  for (int base = 0; base < words; base += kIntensityThreads) {  // the same trips for every wave (ballots inside)
    const int i = base + (int)threadIdx.x;
    uint64_t m = 0ull;
    uint32_t off = 0;
    if (i < words) {
      const int y = i / n, k = i - y * n;
      m = M.at(y, k);
      off = (uint32_t)y * (uint32_t)W + (uint32_t)(k << 6);
    }
    pass_hi(m, off, px, d.type, d.stored_bits, lane, sh_hist + wave * kBins, sum_sq, count);
  }
  sum_sq = wave_sum_u64(sum_sq);
  count = wave_sum_u32(count);
  if (lane == 0) sh_sq[wave] = sum_sq, sh_cnt[wave] = count;
  __syncthreads();
  if (threadIdx.x < kBins) {
    uint32_t c = 0;
    for (int wv = 0; wv < kIntensityWaves; ++wv) c += sh_hist[wv * kBins + (int)threadIdx.x];
    sh_hi[threadIdx.x] = c;
  }
  __syncthreads();

  // ---- the five targets; the low-byte histograms take over the LDS of pass 1 ------------------------------
  for (int i = threadIdx.x; i < kPercentiles * kBins; i += kIntensityThreads) sh_hist[i] = 0u;
  uint32_t total = 0;
  for (int wv = 0; wv < kIntensityWaves; ++wv) total += sh_cnt[wv];
  if (wave < kPercentiles) {  // wave j locates target j
    const BinRank t = wave_select_bin(sh_hi, (uint32_t)icore::percentile_rank(icore::percentile_of(wave), total), lane);
    if (lane == 0) sh_t[wave] = t;
  }
  __syncthreads();

  // ---- pass 2: the low bytes inside the targets' bins ----------------------------------------------------
  if (total != 0u) {  // uniform
    BinRank t[kPercentiles];
    for (int j = 0; j < kPercentiles; ++j) t[j] = sh_t[j];
    for (int base = 0; base < words; base += kIntensityThreads) {
      const int i = base + (int)threadIdx.x;
      uint64_t m = 0ull;
      uint32_t off = 0;
      if (i < words) {
        const int y = i / n, k = i - y * n;
        m = M.at(y, k);
        off = (uint32_t)y * (uint32_t)W + (uint32_t)(k << 6);
      }
      pass_lo(m, off, px, d.type, d.stored_bits, lane, t, sh_hist);
    }
  }
  __syncthreads();

  if (wave < kPercentiles) {  // wave j resolves percentile j
    const int32_t v = total ? wave_resolve(sh_t, sh_hist, wave, d.type, lane) : 0;
    if (lane == 0) sh_pct[wave] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t sq = 0;
    for (int wv = 0; wv < kIntensityWaves; ++wv) sq += sh_sq[wv];
    IntensityStats r = {};
    r.count = total;
    r.sum_sq = total ? sq : 0ull;
    for (int j = 0; j < kPercentiles; ++j) r.pct[j] = sh_pct[j];
    out[blockIdx.x] = r;
  }
}

// ---- 3D ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kViThreads) void vi_init_kernel(ViAcc* __restrict__ acc) {
  uint32_t* w = reinterpret_cast<uint32_t*>(acc);
  for (uint32_t i = threadIdx.x; i < (uint32_t)(sizeof(ViAcc) / 4); i += kViThreads) w[i] = 0u;
}

__global__ __launch_bounds__(kViThreads) void vi_hist_hi_kernel(BitVolume V, const uint16_t* __restrict__ raw,
                                                                uint32_t raw_plane_stride, uint8_t type, uint8_t stored_bits,
                                                                ViAcc* __restrict__ acc) {
  __shared__ uint32_t sh_hist[kViWaves * kBins];  // a histogram per wave
  __shared__ uint64_t sh_sq[kViWaves];
  __shared__ uint32_t sh_cnt[kViWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kViWaves * kBins; i += kViThreads) sh_hist[i] = 0u;
  __syncthreads();
  const ViWord w = vi_word(V, raw_plane_stride);
  uint64_t sum_sq = 0;
  uint32_t count = 0;
  pass_hi(w.m, w.off, raw, type, stored_bits, lane, sh_hist + wave * kBins, sum_sq, count);
  sum_sq = wave_sum_u64(sum_sq);
  count = wave_sum_u32(count);
  if (lane == 0) sh_sq[wave] = sum_sq, sh_cnt[wave] = count;
  __syncthreads();
  // At most one atomic per non-zero bin and workgroup; an empty workgroup adds nothing.
  static_assert(kViThreads == kBins, "a thread per bin");
  uint32_t c = 0;
  for (int wv = 0; wv < kViWaves; ++wv) c += sh_hist[wv * kBins + (int)threadIdx.x];
  add_u32(acc->hi + threadIdx.x, c);
  if (threadIdx.x == 0) {
    uint64_t sq = 0, cn = 0;
    for (int wv = 0; wv < kViWaves; ++wv) sq += sh_sq[wv], cn += sh_cnt[wv];
    add_u64(&acc->sum_sq, sq);
    add_u64(&acc->count, cn);
  }
}

// One workgroup of kPercentiles waves: wave j locates target j.
__global__ __launch_bounds__(kPercentiles * 64) void vi_select_kernel(ViAcc* __restrict__ acc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const BinRank t = wave_select_bin(acc->hi, (uint32_t)icore::percentile_rank(icore::percentile_of(wave), acc->count), lane);
  if (lane == 0) acc->target[wave] = t;
}

__global__ __launch_bounds__(kViThreads) void vi_hist_lo_kernel(BitVolume V, const uint16_t* __restrict__ raw,
                                                                uint32_t raw_plane_stride, uint8_t type, uint8_t stored_bits,
                                                                ViAcc* __restrict__ acc) {
  __shared__ uint32_t sh_hist[kPercentiles * kBins];
  const int lane = threadIdx.x & 63;
  if (acc->count == 0ull) return;  // uniform over the grid: written by an earlier launch
  for (int i = threadIdx.x; i < kPercentiles * kBins; i += kViThreads) sh_hist[i] = 0u;
  BinRank t[kPercentiles];
  for (int j = 0; j < kPercentiles; ++j) t[j] = acc->target[j];
  __syncthreads();
  const ViWord w = vi_word(V, raw_plane_stride);
  pass_lo(w.m, w.off, raw, type, stored_bits, lane, t, sh_hist);
  __syncthreads();
  for (int i = threadIdx.x; i < kPercentiles * kBins; i += kViThreads) add_u32(acc->lo + i, sh_hist[i]);
}

// One workgroup of kPercentiles waves: wave j resolves percentile j, thread 0 writes the record.
__global__ __launch_bounds__(kPercentiles * 64) void vi_final_kernel(const ViAcc* __restrict__ acc, uint8_t type,
                                                                     IntensityStats* __restrict__ out) {
  __shared__ int32_t sh_pct[kPercentiles];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t count = acc->count;
  const int32_t v = count ? wave_resolve(acc->target, acc->lo, wave, type, lane) : 0;
  if (lane == 0) sh_pct[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    IntensityStats r = {};
    r.count = count;
    r.sum_sq = count ? acc->sum_sq : 0ull;
    for (int j = 0; j < kPercentiles; ++j) r.pct[j] = sh_pct[j];
    *out = r;
  }
}

void launch_measure_intensity(const uint64_t* dilated, const uint16_t* raw, const SliceDesc* descs, int nslices,
                              IntensityStats* out, hipStream_t stream) {
  if (nslices <= 0) return;
  if (!dilated || !raw || !descs || !out) throw DeviceError("launch_measure_intensity: null buffer");
  intensity_kernel<<<nslices, kIntensityThreads, 0, stream>>>(dilated, raw, descs, out);
  check_launch("intensity_kernel");
}

void launch_volume_intensity(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d,
                             uint8_t type, uint8_t stored_bits, void* acc, IntensityStats* out, hipStream_t stream) {
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("launch_volume_intensity: empty volume");
  if (stored_bits < 1 || stored_bits > 16) throw DeviceError("launch_volume_intensity: stored bits must be 1..16");
  // The samples are addressed by 32-bit offsets and counted in 32-bit bins, as K8 names its runs.
  if (volume_measure_scratch_words(w, h, d) == 0 || raw_plane_stride < (size_t)w * (size_t)h ||
      raw_plane_stride * (size_t)d > 0xFFFFFFFFull)
    throw DeviceError("launch_volume_intensity: a " + std::to_string(w) + " x " + std::to_string(h) + " x " +
                      std::to_string(d) + " volume is too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
  if (!dilated || !raw || !acc || !out) throw DeviceError("launch_volume_intensity: null buffer");
  const int n = (w + 63) / 64;
  const uint64_t words = (uint64_t)n * (uint64_t)h * (uint64_t)d;  // ≤ voxels < 2^32
  const uint32_t grid = (uint32_t)((words + kViThreads - 1) / kViThreads);
  const BitVolume M{dilated, w, h, d, n, false};
  ViAcc* a = static_cast<ViAcc*>(acc);
  vi_init_kernel<<<1, kViThreads, 0, stream>>>(a);
  check_launch("vi_init_kernel");
  vi_hist_hi_kernel<<<grid, kViThreads, 0, stream>>>(M, raw, (uint32_t)raw_plane_stride, type, stored_bits, a);
  check_launch("vi_hist_hi_kernel");
  vi_select_kernel<<<1, kPercentiles * 64, 0, stream>>>(a);
  check_launch("vi_select_kernel");
  vi_hist_lo_kernel<<<grid, kViThreads, 0, stream>>>(M, raw, (uint32_t)raw_plane_stride, type, stored_bits, a);
  check_launch("vi_hist_lo_kernel");
  vi_final_kernel<<<1, kPercentiles * 64, 0, stream>>>(a, type, out);
  check_launch("vi_final_kernel");
}

void preload_measure_intensity() {
  hipFuncAttributes a;
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&intensity_kernel)), "preload intensity_kernel");
}

void preload_volume_intensity() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&vi_init_kernel), reinterpret_cast<const void*>(&vi_hist_hi_kernel),
                        reinterpret_cast<const void*>(&vi_select_kernel), reinterpret_cast<const void*>(&vi_hist_lo_kernel),
                        reinterpret_cast<const void*>(&vi_final_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume intensity kernels");
}

}  // namespace nm03::gpu
