// K16 — the exact Euclidean distance map of a bit volume in physical space (nm03/volume_distance.h), with the
// margin in millimetres (--dilate-mm) and the thickness (--measure-volume-thickness) as epilogues of its last pass.
//
// A WAVE owns one u64 word of the volume (d planes of h rows of ceil(w / 64) words), lane = bit = voxel, in
// all three passes, so every load and store of a pass is 64 consecutive voxels of one row. All per-line
// arithmetic is nm03/volume_distance_core.h, shared with the host.
//
// LAUNCHES on the volume's stream, separated by kernel boundaries:
//   vdist_rows    g = the index distance along x to the nearest S voxel of the row: count-leading / trailing
//                 zeros inside the word, a wave-uniform walk through the row's words left and right of it
//                 (bounded by the words per row); one u16 per voxel, 0xFFFF = none in this row
//   vdist_cols    c = min over y′ of (g(x, y′)·ux)² + ((y − y′)·uy)², the outward search of the core with its
//                 stop rule; the loads of row y ± k are the 64 consecutive u16 of that row; one i64 per voxel
//   vdist_planes  D = min over z′ of c(x, y, z′) + ((z − z′)·uz)², the same search over the planes z ± k, then
//                 one of three epilogues:
//                   map        store the i64 value
//                   margin     compare with r² and store the BITS of the word by wave ballot (lanes past the
//                              width vote 0, so the last word of a row is masked); no map is materialised
//                   thickness  the best (value, smallest position) over the mask voxels of the words a workgroup
//                              strides over (at most kDistMaxSlots workgroups) into the workgroup's own slot
//   vdist_max_final  (thickness) ONE workgroup reduces the slots and writes the 32-byte record with plain
//                 vector stores
// No cooperative launch, grid barrier, flag, look-back, spin or atomic; every loop is bounded by the data
// (words per row, rows, planes) and the result does not depend on the order in which workgroups run.
#include <hip/hip_runtime.h>

#include <string>

#include "device_util.h"
#include "nm03/kernels.h"
#include "nm03/volume_distance.h"
#include "nm03/volume_distance_core.h"

namespace nm03::gpu {

constexpr int kDistThreads = 256;
constexpr int kDistWaves = kDistThreads / 64;
constexpr uint32_t kDistMaxSlots = 1024;  // workgroups of the thickness pass: what ONE workgroup reduces afterwards
static_assert(kDistWaves == kVolumeDistanceWordsPerBlock, "a wave per word");

namespace {

struct DistGeom {
  int w, h, d, wpr;
  uint32_t words;  // wpr · h · d
  uint32_t um[3];
};

struct DistSlot {
  int64_t value;
  uint64_t pos;  // raster voxel index, vdist::kNoCandidate = none
};

struct DistWord {
  uint32_t i;   // word index
  int kw, y, z;
  int x;        // the lane's voxel
  size_t vox;   // its raster index (valid when `in`)
  bool word_ok; // wave-uniform: the word exists
  bool in;      // the lane's voxel exists
};
__device__ __forceinline__ DistWord my_word(const DistGeom& G, uint32_t block) {
  DistWord r;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the word's coordinates (two divisions) are then computed once per wave
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  r.i = block * (uint32_t)kDistWaves + wave;
  r.word_ok = r.i < G.words;
  const uint32_t row = r.i / (uint32_t)G.wpr;
  r.kw = (int)(r.i - row * (uint32_t)G.wpr);
  r.z = (int)(row / (uint32_t)G.h);
  r.y = (int)(row - (uint32_t)r.z * (uint32_t)G.h);
  r.x = r.kw * 64 + lane;
  r.in = r.word_ok && r.x < G.w;
  r.vox = ((size_t)r.z * (size_t)G.h + (size_t)r.y) * (size_t)G.w + (size_t)r.x;
  return r;
}

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(uint64_t)v, o, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), o, 64);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

}  // namespace

__global__ __launch_bounds__(kDistThreads) void vdist_rows_kernel(DistGeom G, const uint64_t* __restrict__ bits, int to_background,
                                                                  uint16_t* __restrict__ g) {
  const DistWord wd = my_word(G, blockIdx.x);
  if (!wd.word_ok) return;  // wave-uniform
  const uint64_t* __restrict__ row = bits + ((size_t)wd.z * (size_t)G.h + (size_t)wd.y) * (size_t)G.wpr;
  const bool bg = to_background != 0;
  const uint64_t s = vdist::set_word(row, wd.kw, G.w, bg);
  // wave-uniform walks: every lane reads the same words
  const int32_t left = vdist::left_reach(row, G.w, bg, wd.kw), right = vdist::right_reach(row, G.wpr, G.w, bg, wd.kw);
  if (wd.in) g[wd.vox] = vdist::row_distance(s, threadIdx.x & 63, left, right);
}

__global__ __launch_bounds__(kDistThreads) void vdist_cols_kernel(DistGeom G, const uint16_t* __restrict__ g, int64_t cap2,
                                                                  int64_t* __restrict__ c) {
  const DistWord wd = my_word(G, blockIdx.x);
  if (!wd.in) return;
  const uint16_t* __restrict__ col = g + (size_t)wd.z * (size_t)G.h * (size_t)G.w + (size_t)wd.x;
  const size_t stride = (size_t)G.w;
  const uint32_t ux = G.um[0];
  const int64_t v = vdist::search_line(G.h, wd.y, G.um[1], cap2, [&](int j) { return vdist::row_value(col[(size_t)j * stride], ux); });
  c[wd.vox] = vdist::capped(v, cap2);
}

enum { kDistMap = 0, kDistMargin = 1, kDistThickness = 2 };

// D of the lane's voxel (kNoDistance for a lane without one).
__device__ __forceinline__ int64_t plane_value(const DistGeom& G, const DistWord& wd, const int64_t* __restrict__ c, int64_t cap2) {
  if (!wd.in) return kNoDistance;
  const size_t plane = (size_t)G.h * (size_t)G.w;
  const int64_t* __restrict__ line = c + (size_t)wd.y * (size_t)G.w + (size_t)wd.x;
  return vdist::capped(vdist::search_line(G.d, wd.z, G.um[2], cap2, [&](int j) { return line[(size_t)j * plane]; }), cap2);
}

// MODE kDistMap: out_map. kDistMargin: out_bits (cap2 = r²). kDistThickness: `mask` (the volume's own words)
// and `slots`, one per workgroup; the grid may be smaller than `nblocks`, a workgroup strides over the rest.
template <int MODE>
__global__ __launch_bounds__(kDistThreads) void vdist_planes_kernel(DistGeom G, uint32_t nblocks, const int64_t* __restrict__ c,
                                                                    int64_t cap2, int64_t* __restrict__ out_map,
                                                                    uint64_t* __restrict__ out_bits,
                                                                    const uint64_t* __restrict__ mask, DistSlot* __restrict__ slots) {
  if constexpr (MODE == kDistMap) {
    const DistWord wd = my_word(G, blockIdx.x);
    const int64_t v = plane_value(G, wd, c, cap2);
    if (wd.in) out_map[wd.vox] = v;
  } else if constexpr (MODE == kDistMargin) {
    const DistWord wd = my_word(G, blockIdx.x);
    if (!wd.word_ok) return;  // wave-uniform
    const int64_t v = plane_value(G, wd, c, cap2);
    const uint64_t word = __ballot(wd.in && v != kNoDistance);  // capped at r²: a distance left is inside the margin
    if ((threadIdx.x & 63) == 0) out_bits[wd.i] = word;
  } else {
    __shared__ int64_t sh_v[kDistWaves];
    __shared__ uint64_t sh_p[kDistWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t bv = 0;
    uint64_t bp = vdist::kNoCandidate;
    for (uint32_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {  // ascending positions per lane: a tie keeps the first
      const DistWord wd = my_word(G, blk);
      const int64_t v = plane_value(G, wd, c, cap2);
      if (wd.in && v != kNoDistance && ((mask[wd.i] >> lane) & 1ull) && vdist::better(v, (uint64_t)wd.vox, bv, bp))
        bv = v, bp = (uint64_t)wd.vox;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int64_t ov = shfl_xor_i64(bv, o);
      const uint64_t op = (uint64_t)shfl_xor_i64((int64_t)bp, o);
      if (vdist::better(ov, op, bv, bp)) bv = ov, bp = op;
    }
    if (lane == 0) sh_v[wave] = bv, sh_p[wave] = bp;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int wv = 1; wv < kDistWaves; ++wv)
        if (vdist::better(sh_v[wv], sh_p[wv], bv, bp)) bv = sh_v[wv], bp = sh_p[wv];
      slots[blockIdx.x].value = bv;
      slots[blockIdx.x].pos = bp;
    }
  }
}

// One workgroup: the best of the `n` slots → the record.
__global__ __launch_bounds__(kDistThreads) void vdist_max_final_kernel(DistGeom G, const DistSlot* __restrict__ slots, uint32_t n,
                                                                       VolumeThickness* __restrict__ out) {
  __shared__ int64_t sh_v[kDistWaves];
  __shared__ uint64_t sh_p[kDistWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t bv = 0;
  uint64_t bp = vdist::kNoCandidate;
  for (uint32_t i = threadIdx.x; i < n; i += (uint32_t)kDistThreads) {
    const DistSlot s = slots[i];
    if (vdist::better(s.value, s.pos, bv, bp)) bv = s.value, bp = s.pos;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t ov = shfl_xor_i64(bv, o);
    const uint64_t op = (uint64_t)shfl_xor_i64((int64_t)bp, o);
    if (vdist::better(ov, op, bv, bp)) bv = ov, bp = op;
  }
  if (lane == 0) sh_v[wave] = bv, sh_p[wave] = bp;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int wv = 1; wv < kDistWaves; ++wv)
      if (vdist::better(sh_v[wv], sh_p[wv], bv, bp)) bv = sh_v[wv], bp = sh_p[wv];
    const bool found = bp != vdist::kNoCandidate;
    const uint64_t row = found ? bp / (uint64_t)G.w : 0ull;
    uint4 a, b;  // the record as two 16-byte vector stores
    const uint64_t um2 = found ? (uint64_t)bv : 0ull;
    a.x = (uint32_t)um2, a.y = (uint32_t)(um2 >> 32);
    a.z = found ? (uint32_t)(bp - row * (uint64_t)G.w) : 0xFFFFFFFFu;
    a.w = found ? (uint32_t)(row % (uint64_t)G.h) : 0xFFFFFFFFu;
    b.x = found ? (uint32_t)(row / (uint64_t)G.h) : 0xFFFFFFFFu;
    b.y = found ? 1u : 0u;
    b.z = 0u, b.w = 0u;
    uint4* __restrict__ o = reinterpret_cast<uint4*>(out);
    o[0] = a;
    o[1] = b;
  }
}

namespace {

DistGeom geom_of(const VolumeDistanceLayout& L, const uint32_t um[3]) {
  DistGeom G;
  G.w = L.w, G.h = L.h, G.d = L.d, G.wpr = L.wpr;
  G.words = L.words;
  for (int a = 0; a < 3; ++a) G.um[a] = um[a];
  return G;
}

void check_common(const char* who, const VolumeDistanceLayout& L, const uint32_t um[3], const void* bits, const void* work) {
  if (L.w <= 0 || L.h <= 0 || L.d <= 0 || L.w > 65535 || L.wpr != (L.w + 63) / 64 ||
      (uint64_t)L.wpr * (uint64_t)L.h * (uint64_t)L.d != L.words || L.blocks != (L.words + kDistWaves - 1) / kDistWaves)
    throw DeviceError(std::string(who) + ": not a layout of volume_distance_layout");
  for (int a = 0; a < 3; ++a)
    if (um[a] < 1u) throw DeviceError(std::string(who) + ": a spacing must be at least 1 um");
  const std::string ext = measure::volume_distance_extent_error(L.w, L.h, L.d, um);
  if (!ext.empty()) throw DeviceError(std::string(who) + ": " + ext);
  if (!bits || !work) throw DeviceError(std::string(who) + ": null buffer");
}

int64_t cap_squared(int64_t cap_um) {
  if (cap_um < 0) return -1;
  return cap_um >= (1ll << 31) ? (1ll << 62) : cap_um * cap_um;  // every distance stays below 2^62
}

// The first two passes: bits → g → c.
void launch_rows_cols(const uint64_t* bits, const VolumeDistanceLayout& L, const DistGeom& G, bool to_background, int64_t cap2,
                      void* work, hipStream_t stream) {
  uint8_t* base = static_cast<uint8_t*>(work);
  auto* g = reinterpret_cast<uint16_t*>(base + L.off_rows);
  auto* c = reinterpret_cast<int64_t*>(base + L.off_cols);
  vdist_rows_kernel<<<L.blocks, kDistThreads, 0, stream>>>(G, bits, to_background ? 1 : 0, g);
  check_launch("vdist_rows_kernel");
  vdist_cols_kernel<<<L.blocks, kDistThreads, 0, stream>>>(G, g, cap2, c);
  check_launch("vdist_cols_kernel");
}

}  // namespace

VolumeDistanceLayout volume_distance_layout(int w, int h, int d) {
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("volume distance: empty volume");
  if (w > 65535) throw DeviceError("volume distance: a row holds at most 65535 voxels");
  VolumeDistanceLayout L;
  L.w = w, L.h = h, L.d = d;
  L.wpr = (w + 63) / 64;
  const uint64_t words = (uint64_t)L.wpr * (uint64_t)h * (uint64_t)d;
  if (words >= (1ull << 31))
    throw DeviceError("volume distance: a " + std::to_string(w) + " x " + std::to_string(h) + " x " + std::to_string(d) +
                      " volume has 2^31 words or more");
  L.words = (uint32_t)words;
  L.blocks = (L.words + kDistWaves - 1) / kDistWaves;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t voxels = (size_t)w * (size_t)h * (size_t)d;
  L.off_rows = 0;
  L.off_cols = up(voxels * sizeof(uint16_t));
  L.off_slots = L.off_cols + up(voxels * sizeof(int64_t));
  L.bytes = L.off_slots + up((size_t)kDistMaxSlots * sizeof(DistSlot));
  return L;
}

size_t volume_distance_work_bytes(int w, int h, int d) { return volume_distance_layout(w, h, d).bytes; }

void launch_volume_distance(const uint64_t* bits, const VolumeDistanceLayout& L, const uint32_t um[3], bool to_background,
                            int64_t cap_um, void* work, int64_t* out, hipStream_t stream) {
  check_common("launch_volume_distance", L, um, bits, work);
  if (!out) throw DeviceError("launch_volume_distance: null buffer");
  const DistGeom G = geom_of(L, um);
  const int64_t cap2 = cap_squared(cap_um);
  launch_rows_cols(bits, L, G, to_background, cap2, work, stream);
  const auto* c = reinterpret_cast<const int64_t*>(static_cast<uint8_t*>(work) + L.off_cols);
  vdist_planes_kernel<kDistMap><<<L.blocks, kDistThreads, 0, stream>>>(G, L.blocks, c, cap2, out, nullptr, nullptr, nullptr);
  check_launch("vdist_planes_kernel<map>");
}

void launch_volume_margin(const uint64_t* region, const VolumeDistanceLayout& L, const uint32_t um[3], int64_t radius_um, void* work,
                          uint64_t* dilated, hipStream_t stream) {
  check_common("launch_volume_margin", L, um, region, work);
  if (!dilated) throw DeviceError("launch_volume_margin: null buffer");
  if (radius_um < 0) throw DeviceError("launch_volume_margin: the radius must not be negative");
  const DistGeom G = geom_of(L, um);
  const int64_t r2 = cap_squared(radius_um);
  launch_rows_cols(region, L, G, false, r2, work, stream);
  const auto* c = reinterpret_cast<const int64_t*>(static_cast<uint8_t*>(work) + L.off_cols);
  vdist_planes_kernel<kDistMargin><<<L.blocks, kDistThreads, 0, stream>>>(G, L.blocks, c, r2, nullptr, dilated, nullptr, nullptr);
  check_launch("vdist_planes_kernel<margin>");
}

void launch_volume_thickness(const uint64_t* mask, const VolumeDistanceLayout& L, const uint32_t um[3], void* work,
                             VolumeThickness* out, hipStream_t stream) {
  check_common("launch_volume_thickness", L, um, mask, work);
  if (!out) throw DeviceError("launch_volume_thickness: null buffer");
  const DistGeom G = geom_of(L, um);
  launch_rows_cols(mask, L, G, true, -1, work, stream);
  uint8_t* base = static_cast<uint8_t*>(work);
  const auto* c = reinterpret_cast<const int64_t*>(base + L.off_cols);
  auto* slots = reinterpret_cast<DistSlot*>(base + L.off_slots);
  const uint32_t grid = L.blocks < kDistMaxSlots ? L.blocks : kDistMaxSlots;
  vdist_planes_kernel<kDistThickness><<<grid, kDistThreads, 0, stream>>>(G, L.blocks, c, -1, nullptr, nullptr, mask, slots);
  check_launch("vdist_planes_kernel<thickness>");
  vdist_max_final_kernel<<<1, kDistThreads, 0, stream>>>(G, slots, grid, out);
  check_launch("vdist_max_final_kernel");
}

void preload_volume_distance() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&vdist_rows_kernel), reinterpret_cast<const void*>(&vdist_cols_kernel),
                        reinterpret_cast<const void*>(&vdist_planes_kernel<kDistMap>),
                        reinterpret_cast<const void*>(&vdist_planes_kernel<kDistMargin>),
                        reinterpret_cast<const void*>(&vdist_planes_kernel<kDistThickness>),
                        reinterpret_cast<const void*>(&vdist_max_final_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume distance kernels");
}

}  // namespace nm03::gpu
