// K12 — second-order texture of the samples under the dilated mask (nm03/measure.h TextureGlcm,
// --measure-texture): the grey-level co-occurrence matrix (GLCM) at Ng grey levels, merged over the
// forward directions (4 in 2D, 13 in 3D) and symmetric. The definition, the discretisation and the
// per-word pair logic are in nm03/texture_core.h; the doubles are made on the host (measure::glcm_features).
//
// Mapping. A histogram of PAIRS of neighbouring samples. Two walks over the samples, by the wave, each
// of its non-empty u64 mask words in turn, lane = bit. Walk 1 (walk_samples, as K11) finds the smallest
// and largest key, which fix the levels. Walk 2 takes a word (z, y, k) and the five rows that hold its
// forward partners (its own, (y + 1, z), (y − 1 … y + 1, z + 1)): per row one coalesced load of the 64
// samples of word k, lane 0 the sample left of it and lane 63 the sample right of it, the ±1 partners by
// wave shuffle. tcore::neighbour_word gives, per direction, the bits of the word that have a partner;
// a row without any is not loaded. In 2D the rows of plane z + 1 do not exist and drop out the same way.
// A wave takes its words one after the other, so neighbouring words are dealt to different waves.
//
// Contention. The counts are DIRECTED, D[a][b] with a the word's own voxel, and symmetrised once at the
// end (C = D + Dᵀ): half the atomics. A homogeneous lesion sends nearly every pair of a wave to one
// diagonal cell, and 64 LDS atomics on one address serialise, so equal cells are combined in the wave
// before the add (wave_hist_add, as K11; it gives up on words whose cells are spread). In 2D waves also
// have private histograms where LDS allows: min(16, 64 KiB / (4 · Ng²)) copies (Ng = 64: four copies,
// four waves each), summed at the end. The walk is bound by the instructions of these adds, four per
// word in 2D and thirteen in 3D (profiles/k12_texture/timings.md).
//
// 2D, texture_kernel: ONE 1024-THREAD WORKGROUP PER SLICE, descriptor-driven like measure_kernel and
// intensity_kernel, slices of different sizes and sample formats (and, for the Python op, level counts)
// in one launch. All 64 KiB of LDS are histograms; the few words the reductions need are borrowed from
// them before they are zeroed and after they are summed. No global scratch. The matrix goes out as
// coalesced vector stores by the whole workgroup, thread 0 writes the header.
//
// 3D: FOUR LAUNCHES on the volume's stream in K8's and K11's style, 256-thread workgroups, a thread per
// word (z, y, k): init, range (one relaxed global min and max per workgroup), hist (a per-workgroup
// histogram in LDS, then at most one global atomic per non-zero cell and workgroup, into one of sixteen
// copies of the matrix), final (sum the copies, symmetrise, plain vector stores). No cooperative launch, no grid barrier, no flag, no look-back, no spin: the only
// cross-workgroup traffic is relaxed atomics on words that nobody reads before the next kernel boundary.
// Workgroup barriers are the only synchronisation. Every loop is bounded by the data.
#include <hip/hip_runtime.h>

#include <string>

#include "device_util.h"
#include "measure_util.h"
#include "nm03/gpu_types.h"
#include "nm03/intensity_core.h"
#include "nm03/kernels.h"
#include "nm03/measure.h"
#include "nm03/texture_core.h"
#include "nm03/volume_measure_core.h"

namespace nm03::gpu {

constexpr int kTextureThreads = 1024;
constexpr int kTextureWaves = kTextureThreads / 64;
constexpr int kTextureLdsWords = 16384;  // 64 KiB of histograms
constexpr int kVtThreads = 256;          // K8's and K11's workgroup
constexpr int kVtWaves = kVtThreads / 64;
constexpr int kVtAccCopies = 16;       // copies of the global accumulator matrix (VtAcc::dir)
constexpr uint32_t kVtInitGrid = 64;
constexpr int kVtLdsWords = tcore::kMaxLevels * tcore::kMaxLevels;  // 16 KiB
constexpr int kHeadWords = (int)(sizeof(TextureGlcm) / 4);

namespace {

using vmcore::BitVolume;

static_assert(kTextureLdsWords >= 4 * tcore::kMaxLevels * tcore::kMaxLevels, "four copies at 64 levels");
static_assert(kTextureLdsWords >= 3 * kTextureWaves, "walk 1's reduction borrows the histograms");

__device__ __forceinline__ uint32_t key_of(uint16_t rv, uint8_t type, uint8_t stored_bits) {
  return (uint32_t)icore::sample_key(stored_sample(rv, type, stored_bits), type);
}

struct Range {
  uint32_t lo, hi, count;
};

// Walk 1 of one word per lane: the smallest and largest key and the number of samples.
__device__ __forceinline__ void walk_range(uint64_t m, uint32_t off, const uint16_t* __restrict__ px, uint8_t type,
                                           uint8_t stored_bits, int lane, Range& r) {
  walk_samples(m, off, px, lane, [&](bool on, uint16_t rv) {
    if (on) {
      const uint32_t key = key_of(rv, type, stored_bits);
      r.lo = min(r.lo, key);
      r.hi = max(r.hi, key);
      ++r.count;
    }
  });
}

// Walk 2 works on kPairBatch words of the wave at a time, in three phases, so that one memory round trip
// serves the whole batch: the mask words of every row of every word (uniform over the wave: scalar loads),
// then the samples (lane = bit), then the levels, shuffles and adds. A batch of four measured what a
// batch of one does (148 against 145 µs per 93-slice batch, its uniform state spilling to vector
// registers): the walk is bound by the instructions of the adds, not by the round trips. So one.
constexpr int kPairBatch = 1;

// What phase 1 keeps of a word (z, y, k): uniform over the wave.
struct PairWord {
  uint64_t cur[tcore::kPairRows];  // word k of every partner row; cur[0]: the word itself (0: no word)
  uint32_t off[tcore::kPairRows];  // sample offset of bit 0 of cur[r]
  uint32_t edges;                  // bit r: the voxel left of cur[r] is set; bit 8 + r: the one right of it
};

__device__ __forceinline__ uint64_t pair_mask(const PairWord& p, int r, int dx) {
  const uint64_t prev = (uint64_t)((p.edges >> r) & 1u) << 63, next = (uint64_t)((p.edges >> (8 + r)) & 1u);
  return p.cur[0] & tcore::neighbour_word(prev, p.cur[r], next, dx);
}

// Phase 1 of word (z, y, k): `own` is the word, masked to the width. `plane_stride`: samples between
// planes. Sample offsets stay below 2^32 (the launchers check).
__device__ __forceinline__ PairWord pair_word(const BitVolume& V, uint32_t plane_stride, int z, int y, int k, uint64_t own) {
  PairWord p;
  p.edges = 0u;
#pragma unroll
  for (int r = 0; r < tcore::kPairRows; ++r) {
    const int y2 = y + tcore::pair_row_dy(r), z2 = z + tcore::pair_row_dz(r);
    p.cur[r] = r == 0 ? own : V.at(z2, y2, k);
    if (r != 0 && (V.at(z2, y2, k - 1) >> 63)) p.edges |= 1u << r;
    if (V.at(z2, y2, k + 1) & 1ull) p.edges |= 1u << (8 + r);
    p.off[r] = (uint32_t)z2 * plane_stride + (uint32_t)y2 * (uint32_t)V.w + (uint32_t)(k << 6);
  }
  return p;
}

// Does row r hold a partner of the word in any direction? Uniform.
__device__ __forceinline__ bool pair_row_any(const PairWord& p, int r) {
  uint64_t any = 0ull;
#pragma unroll
  for (int dx = -1; dx <= 1; ++dx)
    if (dx >= tcore::pair_row_first_dx(r)) any |= pair_mask(p, r, dx);
  return any != 0ull;
}

// The wave's non-empty words, kPairBatch at a time, lane = bit: the directed counts of their forward pairs
// into `hist` (ng × ng). `m`: the lane's own word (0 for none), `i`: its index (z · h + y) · n + k.
__device__ __forceinline__ void walk_pairs(const BitVolume& V, const uint16_t* __restrict__ px, uint32_t plane_stride,
                                           uint64_t m, uint32_t i, uint8_t type, uint8_t stored_bits, const tcore::Leveler& level,
                                           uint32_t* hist, int lane) {
  for (uint64_t act = __ballot(m != 0ull); act;) {
    PairWord w[kPairBatch];
#pragma unroll
    for (int u = 0; u < kPairBatch; ++u) {
      if (act) {  // uniform
        const int j = __ffsll((long long)act) - 1;
        act &= act - 1;
        const uint32_t wi = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)i, j, 64));
        const uint32_t row = wi / (uint32_t)V.n;
        const int k = (int)(wi - row * (uint32_t)V.n);
        const int z = (int)(row / (uint32_t)V.h);
        const int y = (int)(row - (uint32_t)z * (uint32_t)V.h);
        w[u] = pair_word(V, plane_stride, z, y, k, V.at(z, y, k));
      } else {
        w[u] = PairWord{};  // no word: no bit, no load, no pair
      }
    }
    // Only set bits are loaded: they are inside the frame (V.at masks to the width and the extents).
    uint16_t smid[kPairBatch][tcore::kPairRows], sedge[kPairBatch][tcore::kPairRows];
#pragma unroll
    for (int u = 0; u < kPairBatch; ++u)
#pragma unroll
      for (int r = 0; r < tcore::kPairRows; ++r) {
        smid[u][r] = 0;
        sedge[u][r] = 0;  // lane 0: the sample left of the word; lane 63: the sample right of it
        if (r == 0 || pair_row_any(w[u], r)) {  // uniform; row 0, the word itself, gives the pairs' first members
          if ((w[u].cur[r] >> lane) & 1ull) smid[u][r] = px[(size_t)w[u].off[r] + (size_t)lane];
          if (lane == 0 && ((w[u].edges >> r) & 1u)) sedge[u][r] = px[(size_t)w[u].off[r] - 1u];
          if (lane == 63 && ((w[u].edges >> (8 + r)) & 1u)) sedge[u][r] = px[(size_t)w[u].off[r] + 64u];
        }
      }
#pragma unroll
    for (int u = 0; u < kPairBatch; ++u) {
      if (w[u].cur[0] == 0ull) continue;  // uniform
      const uint32_t a = level(key_of(smid[u][0], type, stored_bits));  // used only where the word's bit is set
#pragma unroll
      for (int r = 0; r < tcore::kPairRows; ++r) {
        if (!pair_row_any(w[u], r)) continue;  // uniform
        const uint32_t mid = r == 0 ? a : level(key_of(smid[u][r], type, stored_bits));
        const uint32_t edge = level(key_of(sedge[u][r], type, stored_bits));
        const uint32_t up = (uint32_t)__shfl((int)mid, (lane + 1) & 63, 64);
        const uint32_t dn = (uint32_t)__shfl((int)mid, (lane + 63) & 63, 64);
        const uint32_t right = lane == 63 ? edge : up, left = lane == 0 ? edge : dn;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (dx < tcore::pair_row_first_dx(r)) continue;
          const uint32_t b = dx < 0 ? left : dx == 0 ? mid : right;
          wave_hist_add(hist, a * level.ng + b, ((pair_mask(w[u], r, dx) >> lane) & 1ull) != 0ull, lane, true);
        }
      }
    }
  }
}

// The header of a record as 32-bit words (a record may lie at any 4-byte aligned address).
__device__ __forceinline__ void write_head(uint32_t* rec, uint32_t ng, uint32_t lo, uint32_t hi, uint64_t samples,
                                           uint64_t pairs) {
  static_assert(kHeadWords == 16, "TextureGlcm layout");
  const bool any = samples != 0ull;
  rec[0] = ng;
  rec[1] = any ? lo : 0u;
  rec[2] = any ? hi : 0u;
  rec[3] = 0u;
  rec[4] = (uint32_t)samples;
  rec[5] = (uint32_t)(samples >> 32);
  rec[6] = (uint32_t)pairs;
  rec[7] = (uint32_t)(pairs >> 32);
  for (int i = 8; i < kHeadWords; ++i) rec[i] = 0u;
}

// The accumulators of the 3D launches (device memory, kVolumeTextureAccBytes).
struct VtAcc {
  uint32_t lo, hi;
  uint64_t samples;
  // D in kVtAccCopies copies (ng × ng of each used), workgroup b adds into copy b mod kVtAccCopies: the
  // adds of all workgroups on one copy measured 3× the whole of K8 (the lines serialise at the memory side).
  uint32_t dir[kVtAccCopies][tcore::kMaxLevels * tcore::kMaxLevels];
};
static_assert(sizeof(VtAcc) <= kVolumeTextureAccBytes && sizeof(VtAcc) % 4 == 0, "texture accumulator layout");

// The thread's word (z, y, k) of the volume and its index, as K11's vi_word.
struct VtWord {
  uint64_t m;
  uint32_t i, off;
};
__device__ __forceinline__ VtWord vt_word(const BitVolume& V, uint32_t raw_plane_stride, uint64_t i) {
  const uint32_t total = (uint32_t)V.d * (uint32_t)V.h * (uint32_t)V.n;  // < 2^32 (launch_volume_texture)
  VtWord w{0ull, 0u, 0u};
  if (i < (uint64_t)total) {
    const uint32_t row = (uint32_t)i / (uint32_t)V.n;
    const int k = (int)((uint32_t)i - row * (uint32_t)V.n);
    const int z = (int)(row / (uint32_t)V.h);
    const int y = (int)(row - (uint32_t)z * (uint32_t)V.h);
    w.m = V.at(z, y, k);
    w.i = (uint32_t)i;
    w.off = (uint32_t)z * raw_plane_stride + (uint32_t)y * (uint32_t)V.w + (uint32_t)(k << 6);
  }
  return w;
}

}  // namespace

__global__ __launch_bounds__(kTextureThreads) void texture_kernel(const uint64_t* __restrict__ dilated,
                                                                  const uint16_t* __restrict__ raw,
                                                                  const SliceDesc* __restrict__ descs,
                                                                  const TextureSlot* __restrict__ slots, uint32_t levels,
                                                                  uint32_t* __restrict__ out) {
  __shared__ uint32_t sh[kTextureLdsWords];
  const SliceDesc d = descs[blockIdx.x];
  const uint32_t ng = slots ? slots[blockIdx.x].levels : levels;
  const uint32_t cells = ng * ng;
  uint32_t* __restrict__ rec = out + (slots ? (size_t)slots[blockIdx.x].word_off : (size_t)blockIdx.x * (size_t)(kHeadWords + cells));
  const int W = d.w, H = d.h, n = d.wpr, words = H * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (W <= 0 || H <= 0) {  // uniform over the workgroup, before any barrier
    for (uint32_t c = threadIdx.x; c < cells; c += kTextureThreads) rec[kHeadWords + c] = 0u;
    if (threadIdx.x == 0) write_head(rec, ng, 0u, 0u, 0ull, 0ull);
    return;
  }
  const BitVolume V{dilated + d.mask_off, W, H, 1, n, false};  // a slice is a one-plane volume
  const uint16_t* __restrict__ px = raw + d.raw_off;

  // ---- walk 1: the range of the keys and the count ------------------------------------------------------
  Range r{0xFFFFFFFFu, 0u, 0u};
  for (int base = 0; base < words; base += kTextureThreads) {  // the same trips for every wave (ballots inside)
    const int i = base + lane * kTextureWaves + wave;  // neighbouring words go to different waves (see walk 2)
    uint64_t m = 0ull;
    uint32_t off = 0;
    if (i < words) {
      const int y = i / n, k = i - y * n;
      m = V.at(0, y, k);
      off = (uint32_t)y * (uint32_t)W + (uint32_t)(k << 6);
    }
    walk_range(m, off, px, d.type, d.stored_bits, lane, r);
  }
  r.lo = wave_min_u32(r.lo);
  r.hi = wave_max_u32(r.hi);
  r.count = wave_sum_u32(r.count);
  if (lane == 0) sh[3 * wave] = r.lo, sh[3 * wave + 1] = r.hi, sh[3 * wave + 2] = r.count;
  __syncthreads();
  uint32_t lo = 0xFFFFFFFFu, hi = 0u, total = 0u;
  for (int wv = 0; wv < kTextureWaves; ++wv) {
    lo = min(lo, sh[3 * wv]);
    hi = max(hi, sh[3 * wv + 1]);
    total += sh[3 * wv + 2];
  }
  __syncthreads();

  // ---- walk 2: directed pair counts, a histogram per group of waves ---------------------------------------
  const uint32_t fit = (uint32_t)kTextureLdsWords / cells;  // ≥ 4
  const uint32_t copies = fit < (uint32_t)kTextureWaves ? fit : (uint32_t)kTextureWaves;
  for (uint32_t c = threadIdx.x; c < copies * cells; c += kTextureThreads) sh[c] = 0u;
  __syncthreads();
  if (total != 0u) {  // uniform
    uint32_t* hist = sh + ((uint32_t)wave % copies) * cells;
    const tcore::Leveler level(lo, hi, ng);  // one division a workgroup, none a sample
    // A lesion's words are neighbours in index order, and a wave takes its non-empty words one after the
    // other: word i of a trip goes to wave i mod 16, so every wave gets its share of them.
    for (int base = 0; base < words; base += kTextureThreads) {
      const int i = base + lane * kTextureWaves + wave;
      uint64_t m = 0ull;
      if (i < words) {
        const int y = i / n, k = i - y * n;
        m = V.at(0, y, k);
      }
      walk_pairs(V, px, 0u, m, (uint32_t)i, d.type, d.stored_bits, level, hist, lane);
    }
  }
  __syncthreads();

  // ---- D = Σ copies (into copy 0), pairs = Σ D, C = D + Dᵀ ------------------------------------------------
  uint64_t pairs = 0;
  for (uint32_t c = threadIdx.x; c < cells; c += kTextureThreads) {  // cell c is read and written by one thread only
    uint32_t v = 0;
    for (uint32_t q = 0; q < copies; ++q) v += sh[q * cells + c];
    sh[c] = v;
    pairs += v;
  }
  pairs = wave_sum_u64(pairs);
  __syncthreads();
  uint32_t* part = sh + cells;  // copy 1 is free now
  if (lane == 0) part[2 * wave] = (uint32_t)pairs, part[2 * wave + 1] = (uint32_t)(pairs >> 32);
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < cells; c += kTextureThreads) {
    const uint32_t a = c / ng, b = c - a * ng;
    rec[kHeadWords + c] = sh[c] + sh[b * ng + a];
  }
  if (threadIdx.x == 0) {
    uint64_t p = 0;
    for (int wv = 0; wv < kTextureWaves; ++wv) p += ((uint64_t)part[2 * wv + 1] << 32) | part[2 * wv];
    write_head(rec, ng, lo, hi, (uint64_t)total, p);
  }
}

// ---- 3D ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kVtThreads) void vt_init_kernel(VtAcc* __restrict__ acc) {
  uint32_t* w = reinterpret_cast<uint32_t*>(acc);
  for (uint32_t i = blockIdx.x * kVtThreads + threadIdx.x; i < (uint32_t)(sizeof(VtAcc) / 4); i += gridDim.x * kVtThreads)
    w[i] = i == 0u ? 0xFFFFFFFFu : 0u;  // lo
}

__global__ __launch_bounds__(kVtThreads) void vt_range_kernel(BitVolume V, const uint16_t* __restrict__ raw,
                                                              uint32_t raw_plane_stride, uint8_t type, uint8_t stored_bits,
                                                              VtAcc* __restrict__ acc) {
  __shared__ uint32_t sh[3 * kVtWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const VtWord w = vt_word(V, raw_plane_stride, (uint64_t)blockIdx.x * kVtThreads + threadIdx.x);
  Range r{0xFFFFFFFFu, 0u, 0u};
  walk_range(w.m, w.off, raw, type, stored_bits, lane, r);
  r.lo = wave_min_u32(r.lo);
  r.hi = wave_max_u32(r.hi);
  r.count = wave_sum_u32(r.count);
  if (lane == 0) sh[3 * wave] = r.lo, sh[3 * wave + 1] = r.hi, sh[3 * wave + 2] = r.count;
  __syncthreads();
  if (threadIdx.x == 0) {  // one relaxed min, max and add per non-empty workgroup
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, total = 0u;
    for (int wv = 0; wv < kVtWaves; ++wv) {
      lo = min(lo, sh[3 * wv]);
      hi = max(hi, sh[3 * wv + 1]);
      total += sh[3 * wv + 2];
    }
    if (total) {
      (void)__hip_atomic_fetch_min(&acc->lo, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_max(&acc->hi, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(&acc->samples, (uint64_t)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ __launch_bounds__(kVtThreads) void vt_hist_kernel(BitVolume V, const uint16_t* __restrict__ raw,
                                                             uint32_t raw_plane_stride, uint8_t type, uint8_t stored_bits,
                                                             uint32_t ng, VtAcc* __restrict__ acc) {
  __shared__ uint32_t sh[kVtLdsWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (acc->samples == 0ull) return;  // uniform over the grid: written by an earlier launch
  const tcore::Leveler level(acc->lo, acc->hi, ng);
  const uint32_t cells = ng * ng;
  const uint32_t fit = (uint32_t)kVtLdsWords / cells;  // ≥ 1
  const uint32_t copies = fit < (uint32_t)kVtWaves ? fit : (uint32_t)kVtWaves;
  for (uint32_t c = threadIdx.x; c < copies * cells; c += kVtThreads) sh[c] = 0u;
  __syncthreads();
  // The workgroup's 256 consecutive words are dealt to its four waves like cards (word i to wave i mod 4):
  // the words of a lesion, neighbours in index order, do not queue up in one wave, and the rows the waves
  // read stay neighbours in memory. (Dealing them over the whole grid measured 2.7× slower on 256³.)
  const VtWord w = vt_word(V, raw_plane_stride, (uint64_t)blockIdx.x * kVtThreads + (uint64_t)(lane * kVtWaves + wave));
  walk_pairs(V, raw, raw_plane_stride, w.m, w.i, type, stored_bits, level, sh + ((uint32_t)wave % copies) * cells, lane);
  __syncthreads();
  // At most one atomic per non-zero cell and workgroup; a workgroup without pairs adds nothing.
  for (uint32_t c = threadIdx.x; c < cells; c += kVtThreads) {
    uint32_t v = 0;
    for (uint32_t q = 0; q < copies; ++q) v += sh[q * cells + c];
    if (v) (void)__hip_atomic_fetch_add(acc->dir[blockIdx.x % kVtAccCopies] + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One workgroup: D = Σ copies, C = D + Dᵀ, pairs = Σ D, the header.
__global__ __launch_bounds__(kVtThreads) void vt_final_kernel(const VtAcc* __restrict__ acc, uint32_t ng,
                                                              uint32_t* __restrict__ rec) {
  __shared__ uint64_t sh_pairs[kVtWaves];
  __shared__ uint32_t sh_d[kVtLdsWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t cells = ng * ng;
  uint64_t pairs = 0;
  for (uint32_t c = threadIdx.x; c < cells; c += kVtThreads) {
    uint32_t v = 0;
    for (int q = 0; q < kVtAccCopies; ++q) v += acc->dir[q][c];
    sh_d[c] = v;
    pairs += v;
  }
  pairs = wave_sum_u64(pairs);
  if (lane == 0) sh_pairs[wave] = pairs;
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < cells; c += kVtThreads) {
    const uint32_t a = c / ng, b = c - a * ng;
    rec[kHeadWords + c] = sh_d[c] + sh_d[b * ng + a];
  }
  if (threadIdx.x == 0) {
    uint64_t p = 0;
    for (int wv = 0; wv < kVtWaves; ++wv) p += sh_pairs[wv];
    write_head(rec, ng, acc->lo, acc->hi, acc->samples, p);
  }
}

namespace {
void check_texture_levels(int levels, const char* who) {
  if (levels < tcore::kMinLevels || levels > tcore::kMaxLevels)
    throw DeviceError(std::string(who) + ": texture levels must be 2..64 (got " + std::to_string(levels) + ")");
}
}  // namespace

void launch_measure_texture(const uint64_t* dilated, const uint16_t* raw, const SliceDesc* descs, int nslices,
                            const TextureSlot* slots, int levels, void* out, hipStream_t stream) {
  if (nslices <= 0) return;
  if (!slots) check_texture_levels(levels, "launch_measure_texture");
  if (!dilated || !raw || !descs || !out) throw DeviceError("launch_measure_texture: null buffer");
  if (reinterpret_cast<uintptr_t>(out) % 4 != 0) throw DeviceError("launch_measure_texture: records must be 4-byte aligned");
  texture_kernel<<<nslices, kTextureThreads, 0, stream>>>(dilated, raw, descs, slots, (uint32_t)levels, static_cast<uint32_t*>(out));
  check_launch("texture_kernel");
}

void launch_volume_texture(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d,
                           uint8_t type, uint8_t stored_bits, int levels, void* acc, void* out, hipStream_t stream) {
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("launch_volume_texture: empty volume");
  if (stored_bits < 1 || stored_bits > 16) throw DeviceError("launch_volume_texture: stored bits must be 1..16");
  check_texture_levels(levels, "launch_volume_texture");
  // The samples are addressed by 32-bit offsets, as K8 names its runs. That bounds the voxels, not the
  // 32-bit cells of the matrix: a cell can reach 2 · 13 · samples and is exact only for samples ≤
  // 165 191 049 (tcore::cells_exact). `samples` in the header is 64-bit and right in any case; the hosts
  // that read the record refuse one beyond the bound (measure::check_glcm_exact). Sparse masks in
  // larger volumes are fine, so nothing is refused by w · h · d here.
  if (volume_measure_scratch_words(w, h, d) == 0 || raw_plane_stride < (size_t)w * (size_t)h ||
      raw_plane_stride * (size_t)d > 0xFFFFFFFFull)
    throw DeviceError("launch_volume_texture: a " + std::to_string(w) + " x " + std::to_string(h) + " x " + std::to_string(d) +
                      " volume is too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
  if (!dilated || !raw || !acc || !out) throw DeviceError("launch_volume_texture: null buffer");
  const int n = (w + 63) / 64;
  const uint64_t words = (uint64_t)n * (uint64_t)h * (uint64_t)d;  // ≤ voxels < 2^32
  const uint32_t grid = (uint32_t)((words + kVtThreads - 1) / kVtThreads);
  const BitVolume M{dilated, w, h, d, n, false};
  VtAcc* a = static_cast<VtAcc*>(acc);
  vt_init_kernel<<<kVtInitGrid, kVtThreads, 0, stream>>>(a);
  check_launch("vt_init_kernel");
  vt_range_kernel<<<grid, kVtThreads, 0, stream>>>(M, raw, (uint32_t)raw_plane_stride, type, stored_bits, a);
  check_launch("vt_range_kernel");
  vt_hist_kernel<<<grid, kVtThreads, 0, stream>>>(M, raw, (uint32_t)raw_plane_stride, type, stored_bits, (uint32_t)levels, a);
  check_launch("vt_hist_kernel");
  vt_final_kernel<<<1, kVtThreads, 0, stream>>>(a, (uint32_t)levels, static_cast<uint32_t*>(out));
  check_launch("vt_final_kernel");
}

void preload_measure_texture() {
  hipFuncAttributes a;
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&texture_kernel)), "preload texture_kernel");
}

void preload_volume_texture() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&vt_init_kernel), reinterpret_cast<const void*>(&vt_range_kernel),
                        reinterpret_cast<const void*>(&vt_hist_kernel), reinterpret_cast<const void*>(&vt_final_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume texture kernels");
}

}  // namespace nm03::gpu
