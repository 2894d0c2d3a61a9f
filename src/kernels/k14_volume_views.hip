// K14 — the views of a volume that use its third axis (nm03/volume_views.h, --volume-views): the axial,
// coronal and sagittal plane through a point P and the projection of the samples (maximum as displayed)
// and of the dilated mask (OR) along z, y and x, written as sample planes and bit planes in the layout K3
// and K4 render from.
//
// FIVE LAUNCHES on the volume's stream, separated by kernel boundaries:
//   init      zero the 32-bit projection scratch and the mask words, reset the head
//   project   ONE read of the samples and of the bit planes. A workgroup of 128 threads owns 128 columns ×
//             kVvRows rows × kVvPlanes planes; thread = column, so a wave's row load is 128 contiguous
//             bytes. Per plane a thread loads its kVvRows samples (independent loads, all in flight), folds
//             them into kVvRows registers (the z-projection, over the chunk's planes), into one value (the
//             y-projection, over the band's rows) and, reduced across the wave by DPP / permlane swaps on
//             packed 16-bit pairs and across the waves through LDS, into the x-projection. The mask words
//             of a wave's 64 columns are one u64 per row: OR over the planes (z-shadow), OR over the rows
//             (y-shadow), "word != 0" as one bit per (z, y) (x-shadow), in the bit layout of the views.
//             A workgroup adds each partial result with ONE integer atomicMax / atomicOr per output element,
//             and only where the grid has more than one workgroup along the projected axis (else a plain
//             store); empty mask words add nothing.
//   point     one workgroup: the bounding box of the mask from the z-shadow (x, y) and the y-shadow (z),
//             then P (views::resolve_at) — in device memory, where the next launch reads it
//   extract   grid (chunks of 1024 pixels, 6): row i writes view i's samples (the plane through P — the
//             sagittal one a gather with stride w, 1/w of the volume — or the projection scratch narrowed back
//             to samples) and the mask words of the three planes (the sagittal ones a wave per word, lane =
//             row, the word by ballot), and folds the view's key min / max (per workgroup, then one
//             atomicMin / atomicMax)
//   count     one workgroup per view: the popcount of its mask words (a plain store: no atomic add)
// The projections hold key ^ flip with flip = 0xFFFF for an inverted volume, so the smallest key wins the
// same atomicMax and 0 is the neutral element of both. No cooperative launch, no grid barrier, no flag, no
// spin; the only cross-workgroup traffic is integer max / min / or on words nobody reads before the next
// kernel boundary, so the result does not depend on the order in which workgroups run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "device_util.h"
#include "nm03/gpu_types.h"
#include "nm03/kernels.h"
#include "nm03/pixel_math.h"
#include "nm03/volume_views.h"

namespace nm03::gpu {

constexpr int kVvThreads = 256;
constexpr int kVvWaves = kVvThreads / 64;
constexpr int kVvCols = 128;   // the projection workgroup: a thread per column, two waves
constexpr int kVvColWaves = kVvCols / 64;
constexpr int kVvRows = 16;    // rows of a workgroup's band; divides 64, so a band's x-shadow bits share a word
constexpr int kVvPlanes = 8;   // planes of a workgroup's chunk
constexpr int kVvChunk = 4 * kVvThreads;  // pixels of a view per extract workgroup
static_assert(64 % kVvRows == 0 && kVvRows % 2 == 0, "band layout");
static_assert(kVvPlanes * kVvRows == kVvCols, "a thread per (plane, row) of the x-projection");

namespace {

struct VvGeom {
  int w, h, d;
  int wpr, wpr_s;  // mask words per row of the volume (and of the w-wide views) and of the h-wide views
  uint32_t sample_off[kVolumeViewCount], mask_off[kVolumeViewCount], proj_off[3];
  uint32_t mask_words;  // of all six masks
  uint32_t proj_total;
};

// Bits of word k of a `width`-wide row that belong to the row.
__device__ __forceinline__ uint64_t word_mask(int k, int width) {
  const int left = width - (k << 6);
  return left >= 64 ? ~0ull : left <= 0 ? 0ull : ((1ull << left) - 1ull);
}

// max over the wave of two packed 16-bit values, without the LDS crossbar.
__device__ __forceinline__ uint32_t wave_max_u16x2(uint32_t v, int lane) {
  auto mx = [](uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, vmax(as_u16x2(a), as_u16x2(b))); };
  v = mx(v, lane_xor<1>(v, lane));
  v = mx(v, lane_xor<2>(v, lane));
  v = mx(v, lane_xor<4>(v, lane));
  v = mx(v, lane_xor<8>(v, lane));
  v = mx(v, lane_xor<16>(v, lane));
  v = mx(v, lane_xor<32>(v, lane));
  return v;
}

__device__ __forceinline__ void or_u64(uint64_t* p, uint64_t v) {
  if (v) (void)atomicOr(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

}  // namespace

__global__ __launch_bounds__(kVvThreads) void vv_init_kernel(VvGeom G, uint32_t* __restrict__ proj, uint64_t* __restrict__ bits,
                                                             VolumeViewsHead* __restrict__ head) {
  const uint32_t i0 = blockIdx.x * (uint32_t)kVvThreads + threadIdx.x, step = gridDim.x * (uint32_t)kVvThreads;
  for (uint32_t i = i0; i < G.proj_total; i += step) proj[i] = 0u;
  for (uint32_t i = i0; i < G.mask_words; i += step) bits[i] = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    VolumeViewsHead r = {};
    for (int v = 0; v < kVolumeViewCount; ++v) r.stats[v] = SliceStats{0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u};
    *head = r;
  }
}

__global__ __launch_bounds__(kVvCols) void vv_project_kernel(VvGeom G, const uint16_t* __restrict__ raw, size_t ps,
                                                                const uint64_t* __restrict__ dil, uint8_t type,
                                                                uint8_t stored_bits, uint32_t flip, uint32_t* __restrict__ proj,
                                                                uint64_t* __restrict__ bits) {
  __shared__ uint32_t sh_x[kVvPlanes][kVvColWaves][kVvRows / 2];  // packed pairs of rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = G.w, h = G.h, d = G.d, wpr = G.wpr;
  const int x = (int)blockIdx.x * kVvCols + (int)threadIdx.x;
  const int y0 = (int)blockIdx.y * kVvRows, z0 = (int)blockIdx.z * kVvPlanes;
  const int ny = min(kVvRows, h - y0), nz = min(kVvPlanes, d - z0);  // ≥ 1 by the grid
  const bool in = x < w;
  const int k = x >> 6;  // the wave's mask word: the same for its 64 lanes
  const bool has_k = k < wpr;
  const uint64_t valid = word_mask(k, w);
  uint32_t* __restrict__ pz = proj + G.proj_off[0];
  uint32_t* __restrict__ py = proj + G.proj_off[1];
  uint32_t* __restrict__ px = proj + G.proj_off[2];
  uint64_t* __restrict__ sz = bits + G.mask_off[3];
  uint64_t* __restrict__ sy = bits + G.mask_off[4];
  uint64_t* __restrict__ sx = bits + G.mask_off[5];
  uint32_t acc_z[kVvRows];
  uint64_t or_z[kVvRows];
#pragma unroll
  for (int yi = 0; yi < kVvRows; ++yi) acc_z[yi] = 0u, or_z[yi] = 0ull;
  for (int zi = 0; zi < kVvPlanes; ++zi) {
    const bool zin = zi < nz;  // uniform; the LDS slots of the missing planes are written (0) so the tail reads no garbage
    const int z = z0 + zi;
    uint32_t kk[kVvRows];
    uint64_t mm[kVvRows];
#pragma unroll
    for (int yi = 0; yi < kVvRows; ++yi) {
      kk[yi] = 0u;
      mm[yi] = 0ull;
      if (zin && yi < ny) {
        if (in)
          kk[yi] = (uint32_t)key_from_raw(raw[(size_t)z * ps + (size_t)(y0 + yi) * (size_t)w + (size_t)x], type, stored_bits) ^ flip;
        if (has_k) mm[yi] = dil[((size_t)z * (size_t)h + (size_t)(y0 + yi)) * (size_t)wpr + (size_t)k] & valid;
      }
    }
    uint32_t cy = 0u;
    uint64_t oy = 0ull, xbits = 0ull;
#pragma unroll
    for (int yi = 0; yi < kVvRows; ++yi) {
      acc_z[yi] = max(acc_z[yi], kk[yi]);
      cy = max(cy, kk[yi]);
      or_z[yi] |= mm[yi];
      oy |= mm[yi];
      if (mm[yi]) xbits |= 1ull << ((y0 + yi) & 63);
    }
    if (zin && in) {
      if (gridDim.y > 1) (void)atomicMax(&py[(size_t)z * (size_t)w + (size_t)x], cy);
      else py[(size_t)z * (size_t)w + (size_t)x] = cy;
    }
    if (zin && lane == 0) {
      or_u64(&sy[(size_t)z * (size_t)wpr + (size_t)k], oy);  // oy != 0 only with has_k
      or_u64(&sx[(size_t)z * (size_t)G.wpr_s + (size_t)(y0 >> 6)], xbits);
    }
#pragma unroll
    for (int j = 0; j < kVvRows / 2; ++j) {
      const uint32_t m = wave_max_u16x2(kk[2 * j] | (kk[2 * j + 1] << 16), lane);
      if (lane == 0) sh_x[zi][wave][j] = m;
    }
  }
#pragma unroll
  for (int yi = 0; yi < kVvRows; ++yi) {
    if (yi < ny && in) {
      const size_t o = (size_t)(y0 + yi) * (size_t)w + (size_t)x;
      if (gridDim.z > 1) (void)atomicMax(&pz[o], acc_z[yi]);
      else pz[o] = acc_z[yi];
    }
    if (yi < ny && lane == 0) or_u64(&sz[(size_t)(y0 + yi) * (size_t)wpr + (size_t)k], or_z[yi]);
  }
  __syncthreads();
  {  // the x-projection of (plane zi, row yi): over the workgroup's waves, then one atomic
    const int zi = (int)threadIdx.x / kVvRows, yi = (int)threadIdx.x % kVvRows;
    if (zi < nz && yi < ny) {
      uint32_t m = 0u;
#pragma unroll
      for (int wv = 0; wv < kVvColWaves; ++wv) m = max(m, (sh_x[zi][wv][yi >> 1] >> ((yi & 1) * 16)) & 0xFFFFu);
      const size_t o = (size_t)(z0 + zi) * (size_t)h + (size_t)(y0 + yi);
      if (gridDim.x > 1) (void)atomicMax(&px[o], m);
      else px[o] = m;
    }
  }
}

// One workgroup: the box of the mask and P.
__global__ __launch_bounds__(kVvThreads) void vv_point_kernel(VvGeom G, const uint64_t* __restrict__ bits, int mode, int ax,
                                                              int ay, int az, VolumeViewsHead* __restrict__ head) {
  __shared__ int lo[3], hi[3];
  if (threadIdx.x < 3) lo[threadIdx.x] = 0x7FFFFFFF, hi[threadIdx.x] = -1;
  __syncthreads();
  const uint64_t* __restrict__ sz = bits + G.mask_off[3];
  const uint64_t* __restrict__ sy = bits + G.mask_off[4];
  // a thread's own extremes first (min as it is, max as value + 1 so that 0 means none), then the wave's,
  // then one LDS atomic per wave: 256 threads on one LDS address serialise
  uint32_t tlo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, thi[3] = {0u, 0u, 0u};
  for (int i = threadIdx.x; i < G.h * G.wpr; i += kVvThreads) {
    const uint64_t m = sz[i];
    if (m) {
      const int y = i / G.wpr, k = i - y * G.wpr;
      tlo[1] = min(tlo[1], (uint32_t)y);
      thi[1] = max(thi[1], (uint32_t)y + 1u);
      tlo[0] = min(tlo[0], (uint32_t)((k << 6) + (__ffsll((long long)m) - 1)));
      thi[0] = max(thi[0], (uint32_t)((k << 6) + 64 - __clzll((long long)m)));
    }
  }
  for (int i = threadIdx.x; i < G.d * G.wpr; i += kVvThreads)
    if (sy[i]) {
      const int z = i / G.wpr;
      tlo[2] = min(tlo[2], (uint32_t)z);
      thi[2] = max(thi[2], (uint32_t)z + 1u);
    }
  for (int a = 0; a < 3; ++a) {
    const uint32_t l = wave_min_u32(tlo[a]), u = wave_max_u32(thi[a]);
    if ((threadIdx.x & 63) == 0 && u != 0u) {
      atomicMin(&lo[a], (int)l);
      atomicMax(&hi[a], (int)u - 1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool has = hi[0] >= 0;
    int box[6] = {0, 0, 0, 0, 0, 0};
    if (has)
      for (int a = 0; a < 3; ++a) box[a] = lo[a], box[3 + a] = hi[a];
    int at[3];
    views::resolve_at(mode, ax, ay, az, has, box, G.w, G.h, G.d, at);
    for (int a = 0; a < 3; ++a) head->at[a] = clampi(at[a], 0, (a == 0 ? G.w : a == 1 ? G.h : G.d) - 1);  // inside by construction
    head->has_box = has ? 1 : 0;
    for (int a = 0; a < 6; ++a) head->box[a] = box[a];
  }
}

__global__ __launch_bounds__(kVvThreads) void vv_extract_kernel(VvGeom G, const uint16_t* __restrict__ raw, size_t ps,
                                                                const uint64_t* __restrict__ dil, uint8_t type,
                                                                uint8_t stored_bits, uint32_t flip, const uint32_t* __restrict__ proj,
                                                                uint16_t* __restrict__ samples, uint64_t* __restrict__ bits,
                                                                VolumeViewsHead* __restrict__ head) {
  __shared__ uint32_t sh_lo[kVvWaves], sh_hi[kVvWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = G.w, h = G.h, d = G.d, wpr = G.wpr;
  const int Px = head->at[0], Py = head->at[1], Pz = head->at[2];  // written by the launch before this one
  const size_t pwords = (size_t)h * (size_t)wpr;                   // mask words of a plane of the volume
  const int v = (int)blockIdx.y;
  const int vw = views::view_width(v, w, h), vh = views::view_height(v, h, d), vn = (vw + 63) >> 6;
  const uint32_t npix = (uint32_t)vw * (uint32_t)vh, nwords = (uint32_t)vh * (uint32_t)vn;
  const uint32_t base = blockIdx.x * (uint32_t)kVvChunk;
  if (base >= npix) return;  // uniform; words ≤ pixels, so nothing is left either
  uint16_t* __restrict__ out = samples + G.sample_off[v];
  uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
  for (int j = 0; j < kVvChunk / kVvThreads; ++j) {
    const uint32_t i = base + (uint32_t)j * kVvThreads + threadIdx.x;
    if (i < npix) {
      const uint32_t r = i / (uint32_t)vw, c = i - r * (uint32_t)vw;
      uint16_t s;
      if (v == 0) s = raw[(size_t)Pz * ps + (size_t)r * w + c];
      else if (v == 1) s = raw[(size_t)r * ps + (size_t)Py * w + c];
      else if (v == 2) s = raw[(size_t)r * ps + (size_t)c * w + (size_t)Px];
      else s = views::sample_of_key((uint16_t)((proj[G.proj_off[v - 3] + i] ^ flip) & 0xFFFFu), type);
      out[i] = s;
      const uint32_t key = key_from_raw(s, type, stored_bits);
      kmin = min(kmin, key);
      kmax = max(kmax, key);
    }
  }
  if (v < 2) {  // the mask words of the axial and coronal plane (the projections' shadows are in place already)
    uint64_t* __restrict__ mo = bits + G.mask_off[v];
#pragma unroll
    for (int j = 0; j < kVvChunk / kVvThreads; ++j) {
      const uint32_t i = base + (uint32_t)j * kVvThreads + threadIdx.x;
      if (i < nwords) {
        const int r = (int)(i / (uint32_t)vn), k = (int)(i - (uint32_t)r * (uint32_t)vn);
        uint64_t m = 0ull;
        if (v == 0) m = dil[(size_t)Pz * pwords + (size_t)r * wpr + k] & word_mask(k, w);
        else m = dil[(size_t)r * pwords + (size_t)Py * wpr + k] & word_mask(k, w);
        mo[i] = m;
      }
    }
  }
  if (v == 2) {  // the sagittal mask: a wave per word (z, k), lane = row y of the volume, the word by ballot
    uint64_t* __restrict__ mo = bits + G.mask_off[2];
    const uint32_t nb = (npix + (uint32_t)kVvChunk - 1u) / (uint32_t)kVvChunk;  // the workgroups of this view that run
    for (uint32_t q = blockIdx.x * (uint32_t)kVvWaves + (uint32_t)wave; q < nwords; q += nb * (uint32_t)kVvWaves) {  // wave-uniform
      const int r = (int)(q / (uint32_t)vn), k = (int)(q - (uint32_t)r * (uint32_t)vn), y = (k << 6) + lane;
      bool bit = false;
      if (y < h) bit = ((dil[(size_t)r * pwords + (size_t)y * wpr + (Px >> 6)] >> (Px & 63)) & 1ull) != 0ull;
      const uint64_t m = __ballot(bit);
      if (lane == 0) mo[q] = m;
    }
  }
  kmin = wave_min_u32(kmin);
  kmax = wave_max_u32(kmax);
  if (lane == 0) sh_lo[wave] = kmin, sh_hi[wave] = kmax;
  __syncthreads();
  if (threadIdx.x == 0) {  // this workgroup has at least one pixel
    for (int wv = 1; wv < kVvWaves; ++wv) kmin = min(kmin, sh_lo[wv]), kmax = max(kmax, sh_hi[wv]);
    (void)atomicMin(&head->stats[v].key_min, kmin);
    (void)atomicMax(&head->stats[v].key_max, kmax);
  }
}

// One workgroup per view: the popcount of its mask words, as the launch before left them.
__global__ __launch_bounds__(kVvThreads) void vv_count_kernel(VvGeom G, const uint64_t* __restrict__ bits,
                                                              VolumeViewsHead* __restrict__ head) {
  __shared__ uint32_t sh_n[kVvWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int v = (int)blockIdx.x;  // < kVolumeViewCount by the grid
  const int vw = views::view_width(v, G.w, G.h), vh = views::view_height(v, G.h, G.d), vn = (vw + 63) >> 6;
  uint32_t n = 0;
  for (int i = threadIdx.x; i < vh * vn; i += kVvThreads) n += __popcll(bits[G.mask_off[v] + i] & word_mask(i % vn, vw));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o, 64);
  if (lane == 0) sh_n[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int wv = 0; wv < kVvWaves; ++wv) t += sh_n[wv];
    head->mask_px[v] = t;
  }
}

VolumeViewsLayout volume_views_layout(int w, int h, int d) {
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("volume views: empty volume");
  VolumeViewsLayout L;
  L.w = w, L.h = h, L.d = d;
  uint64_t so = 0, po = 0;
  for (int i = 0; i < kVolumeViewCount; ++i) {
    L.vw[i] = views::view_width(i, w, h);
    L.vh[i] = views::view_height(i, h, d);
    L.wpr[i] = (L.vw[i] + 63) / 64;
    if (L.vw[i] > 0xFFFF || L.vh[i] > 0xFFFF) throw DeviceError("volume views: a side above 65535 cannot be rendered");
    L.sample_off[i] = (uint32_t)so;
    so += ((uint64_t)L.vw[i] * (uint64_t)L.vh[i] + 7) / 8 * 8;
  }
  uint64_t mo = 0;
  for (int i : {0, 3, 1, 4, 2, 5}) {
    L.mask_off[i] = (uint32_t)mo;
    mo += (uint64_t)L.vh[i] * (uint64_t)L.wpr[i];
  }
  for (int a = 0; a < 3; ++a) {
    L.proj_off[a] = (uint32_t)po;
    po += (uint64_t)L.vw[3 + a] * (uint64_t)L.vh[3 + a];
  }
  if (so > 0xFFFFFFFFull || 2 * mo > 0xFFFFFFFFull || po > 0xFFFFFFFFull)
    throw DeviceError("volume views: a " + std::to_string(w) + " x " + std::to_string(h) + " x " + std::to_string(d) +
                      " volume has views too large for 32-bit offsets");
  L.border_off = (uint32_t)mo;
  L.samples = (size_t)so;
  L.bit_words = (size_t)(2 * mo);
  L.proj = (size_t)po;
  return L;
}

void launch_volume_views(const uint16_t* raw, size_t raw_plane_stride, const uint64_t* dilated, uint8_t type,
                         uint8_t stored_bits, bool inverted, const ViewsAt& at, const VolumeViewsLayout& L, uint16_t* samples,
                         uint64_t* bits, uint32_t* proj, VolumeViewsHead* head, hipStream_t stream) {
  const int w = L.w, h = L.h, d = L.d;
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("launch_volume_views: empty volume");
  if (stored_bits < 1 || stored_bits > 16) throw DeviceError("launch_volume_views: stored bits must be 1..16");
  if (raw_plane_stride < (size_t)w * (size_t)h || raw_plane_stride * (size_t)d > 0xFFFFFFFFull)
    throw DeviceError("launch_volume_views: a " + std::to_string(w) + " x " + std::to_string(h) + " x " + std::to_string(d) +
                      " volume at a plane stride of " + std::to_string(raw_plane_stride) +
                      " samples: the stride must cover a plane and stride * d must stay below 2^32");
  if (!raw || !dilated || !samples || !bits || !proj || !head) throw DeviceError("launch_volume_views: null buffer");
  const std::string err = views::at_error(at, w, h, d);
  if (!err.empty()) throw DeviceError("launch_volume_views: " + err);
  VvGeom G;
  G.w = w, G.h = h, G.d = d;
  G.wpr = (w + 63) / 64;
  G.wpr_s = (h + 63) / 64;
  for (int i = 0; i < kVolumeViewCount; ++i) G.sample_off[i] = L.sample_off[i], G.mask_off[i] = L.mask_off[i];
  for (int a = 0; a < 3; ++a) G.proj_off[a] = L.proj_off[a];
  G.mask_words = L.border_off;
  G.proj_total = (uint32_t)L.proj;
  const uint8_t t = type == kU8 ? (uint8_t)kU16 : type;
  const uint32_t flip = inverted ? 0xFFFFu : 0u;
  const uint32_t init_grid = (uint32_t)std::min<size_t>(1024, (std::max<size_t>(L.proj, L.border_off) + kVvThreads - 1) / kVvThreads);
  vv_init_kernel<<<init_grid, kVvThreads, 0, stream>>>(G, proj, bits, head);
  check_launch("vv_init_kernel");
  const dim3 pg((unsigned)((w + kVvCols - 1) / kVvCols), (unsigned)((h + kVvRows - 1) / kVvRows),
                (unsigned)((d + kVvPlanes - 1) / kVvPlanes));
  if (pg.y > 65535u || pg.z > 65535u) throw DeviceError("launch_volume_views: volume too large for the projection grid");
  vv_project_kernel<<<pg, kVvCols, 0, stream>>>(G, raw, raw_plane_stride, dilated, t, stored_bits, flip, proj, bits);
  check_launch("vv_project_kernel");
  vv_point_kernel<<<1, kVvThreads, 0, stream>>>(G, bits, at.mode, at.x, at.y, at.z, head);
  check_launch("vv_point_kernel");
  size_t most = 0;
  for (int i = 0; i < kVolumeViewCount; ++i) most = std::max(most, (size_t)L.vw[i] * (size_t)L.vh[i]);
  const dim3 eg((unsigned)((most + kVvChunk - 1) / kVvChunk), kVolumeViewCount);
  vv_extract_kernel<<<eg, kVvThreads, 0, stream>>>(G, raw, raw_plane_stride, dilated, t, stored_bits, flip, proj, samples, bits,
                                                   head);
  check_launch("vv_extract_kernel");
  vv_count_kernel<<<kVolumeViewCount, kVvThreads, 0, stream>>>(G, bits, head);
  check_launch("vv_count_kernel");
}

void preload_volume_views() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&vv_init_kernel), reinterpret_cast<const void*>(&vv_project_kernel),
                        reinterpret_cast<const void*>(&vv_point_kernel), reinterpret_cast<const void*>(&vv_extract_kernel),
                        reinterpret_cast<const void*>(&vv_count_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume views kernels");
}

}  // namespace nm03::gpu
