// K15 — the surface of the dilated bit volume as an indexed quad mesh (nm03/volume_mesh.h, --volume-mesh).
//
// A thread owns one u64 word of the LATTICE: (d + 1) planes of (h + 1) rows of ceil((w + 1) / 64) words,
// bit = corner. All per-word arithmetic is nm03/volume_mesh_core.h, shared with the host.
//
// LAUNCHES on the volume's stream, separated by kernel boundaries:
//   classify   the mixed word (any & ~all of the 8 voxel words of the windows) and the three face words,
//              masked to the lattice, stored with their four popcounts; the set-voxel count by wave sum, LDS
//              and one integer atomic add per workgroup (as K8 reduces its figures)
//   totals     a workgroup per scan block of `scan_block` lattice words: wave s sums count stream s
//   scan       ONE workgroup: wave s turns the block totals of stream s into exclusive offsets, 64 at a time
//              with a running u64 carry, and leaves the stream's total in the head
//   downsweep  a workgroup per scan block: wave s turns the counts of stream s into exclusive prefixes in
//              raster order, 64 at a time from the block's offset
//   (the head — four totals and the voxel count — goes to pinned memory; the host sizes the result)
//   vertices   every set bit of a mixed word writes its position at prefix + popcount(bits below)
//   quads      every set face bit writes four vertex indices as one 16-byte store; a thread holds the
//              prefixes and mixed words of its at most four lattice rows and the prefix of the word after
// No cooperative launch, grid barrier, flag, look-back or spin; every loop is bounded by the data. The
// voxel count is the only cross-workgroup atomic, an integer sum nobody reads before the copy.
#include <hip/hip_runtime.h>

#include <string>

#include "device_util.h"
#include "nm03/kernels.h"
#include "nm03/volume_mesh.h"
#include "nm03/volume_mesh_core.h"

namespace nm03::gpu {

constexpr int kMeshThreads = 256;
constexpr int kMeshWaves = kMeshThreads / 64;
static_assert(kMeshWaves == 4, "a wave per count stream");

namespace {

using meshcore::MeshGeom;

struct MeshWordIndex {
  uint32_t i;
  int k, j, kw;
  bool valid;
};
__device__ __forceinline__ MeshWordIndex my_lattice_word(const MeshGeom& G) {
  MeshWordIndex r;
  r.i = blockIdx.x * (uint32_t)kMeshThreads + threadIdx.x;
  r.valid = r.i < G.words;
  const uint32_t row = r.i / (uint32_t)G.lw;
  r.kw = (int)(r.i - row * (uint32_t)G.lw);
  r.k = (int)(row / (uint32_t)(G.h + 1));
  r.j = (int)(row - (uint32_t)r.k * (uint32_t)(G.h + 1));
  return r;
}

}  // namespace

__global__ __launch_bounds__(kMeshThreads) void mesh_classify_kernel(MeshGeom G, const uint64_t* __restrict__ vol,
                                                                     uint64_t* __restrict__ bits, uint32_t* __restrict__ cnt,
                                                                     VolumeMeshHead* __restrict__ head) {
  __shared__ uint32_t sh_vox[kMeshWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const MeshWordIndex wi = my_lattice_word(G);
  uint32_t vox = 0;
  if (wi.valid) {
    const meshcore::MeshWord r = meshcore::classify_word(vol, G, wi.k, wi.j, wi.kw);
    const size_t n = G.words;
    bits[wi.i] = r.mixed;
    bits[n + wi.i] = r.fx;
    bits[2 * n + wi.i] = r.fy;
    bits[3 * n + wi.i] = r.fz;
    cnt[wi.i] = (uint32_t)__popcll(r.mixed);
    cnt[n + wi.i] = (uint32_t)__popcll(r.fx);
    cnt[2 * n + wi.i] = (uint32_t)__popcll(r.fy);
    cnt[3 * n + wi.i] = (uint32_t)__popcll(r.fz);
    vox = r.voxels;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) vox += (uint32_t)__shfl_xor((int)vox, o, 64);
  if (lane == 0) sh_vox[wave] = vox;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int wv = 0; wv < kMeshWaves; ++wv) t += sh_vox[wv];
    if (t) (void)__hip_atomic_fetch_add(&head->voxels, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Block b, wave s: the sum of cnt[s][b · scan_block …) → bt[s][b].
__global__ __launch_bounds__(kMeshThreads) void mesh_totals_kernel(uint32_t words, uint32_t scan_block, uint32_t blocks,
                                                                   const uint32_t* __restrict__ cnt, uint32_t* __restrict__ bt) {
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const uint32_t b = blockIdx.x;  // < blocks by the grid
  const uint64_t lo = (uint64_t)b * scan_block, hi = min((uint64_t)words, lo + scan_block);
  uint32_t sum = 0;  // ≤ 64 · scan_block < 2^32
  for (uint64_t i = lo + (uint32_t)lane; i < hi; i += 64) sum += cnt[(size_t)s * words + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o, 64);
  if (lane == 0) bt[(size_t)s * blocks + b] = sum;
}

// One workgroup; wave s: bt[s][·] → exclusive offsets (low 32 bits), the total → head.
__global__ __launch_bounds__(kMeshThreads) void mesh_scan_kernel(uint32_t blocks, uint32_t* __restrict__ bt,
                                                                 VolumeMeshHead* __restrict__ head) {
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  uint32_t* __restrict__ t = bt + (size_t)s * blocks;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < blocks; base += 64) {  // wave-uniform
    const uint32_t i = base + (uint32_t)lane;
    const uint32_t v = i < blocks ? t[i] : 0u;
    const uint32_t inc = wave_inclusive_scan(v, lane);  // ≤ 64 · 64 · scan_block: fits with scan_block ≤ 2^20
    if (i < blocks) t[i] = (uint32_t)carry + (inc - v);
    carry += (uint32_t)__shfl((int)inc, 63, 64);
  }
  if (lane == 0) head->total[s] = carry;
}

// Block b, wave s: cnt[s][·] of the block → exclusive prefixes from bt[s][b].
__global__ __launch_bounds__(kMeshThreads) void mesh_downsweep_kernel(uint32_t words, uint32_t scan_block, uint32_t blocks,
                                                                      uint32_t* __restrict__ cnt, const uint32_t* __restrict__ bt) {
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const uint32_t b = blockIdx.x;
  const uint64_t lo = (uint64_t)b * scan_block, hi = min((uint64_t)words, lo + scan_block);
  uint32_t* __restrict__ c = cnt + (size_t)s * words;
  uint32_t run = bt[(size_t)s * blocks + b];
  for (uint64_t base = lo; base < hi; base += 64) {  // wave-uniform
    const uint64_t i = base + (uint32_t)lane;
    const uint32_t v = i < hi ? c[i] : 0u;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    if (i < hi) c[i] = run + (inc - v);
    run += (uint32_t)__shfl((int)inc, 63, 64);
  }
}

__global__ __launch_bounds__(kMeshThreads) void mesh_vertices_kernel(MeshGeom G, const uint64_t* __restrict__ vol,
                                                                     const uint64_t* __restrict__ bits,
                                                                     const uint32_t* __restrict__ pre, int placement, float sx,
                                                                     float sy, float sz, uint32_t nvert, float* __restrict__ positions) {
  const MeshWordIndex wi = my_lattice_word(G);
  if (!wi.valid) return;
  const uint64_t mixed = bits[wi.i];
  if (mixed == 0ull) return;
  const uint32_t first = pre[wi.i];
  if ((uint64_t)first + (uint32_t)__popcll(mixed) > nvert) return;  // never with a consistent scan: no store past the buffer
  meshcore::word_vertices(vol, G, wi.k, wi.j, wi.kw, mixed, first, placement, sx, sy, sz, positions);
}

__global__ __launch_bounds__(kMeshThreads) void mesh_quads_kernel(MeshGeom G, const uint64_t* __restrict__ vol,
                                                                  const uint64_t* __restrict__ bits,
                                                                  const uint32_t* __restrict__ pre, uint32_t qx, uint32_t qy,
                                                                  uint32_t nquads, uint32_t* __restrict__ quads) {
  const MeshWordIndex wi = my_lattice_word(G);
  if (!wi.valid) return;
  const size_t n = G.words;
  const uint64_t f[3] = {bits[n + wi.i], bits[2 * n + wi.i], bits[3 * n + wi.i]};
  if ((f[0] | f[1] | f[2]) == 0ull) return;
  const meshcore::QuadRows R = meshcore::quad_rows(G, bits, pre, wi.k, wi.j, wi.kw);
  const uint64_t up = meshcore::mask_word(vol, G, wi.k, wi.j, wi.kw);
  const uint32_t base[3] = {0u, qx, qx + qy};
  uint4* __restrict__ out = reinterpret_cast<uint4*>(quads);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (f[a] == 0ull) continue;
    const uint32_t first = base[a] + pre[(size_t)(1 + a) * n + wi.i];
    if ((uint64_t)first + (uint32_t)__popcll(f[a]) > nquads) continue;  // as in the vertex launch
    meshcore::word_quads(R, a, f[a], up, first, [&](uint32_t at, const meshcore::Quad& q) {
      out[at] = make_uint4(q.q[0], q.q[1], q.q[2], q.q[3]);
    });
  }
}

namespace {

MeshGeom geom_of(const VolumeMeshLayout& L) {
  MeshGeom G;
  G.w = L.w, G.h = L.h, G.d = L.d;
  G.n = (L.w + 63) / 64;
  G.lw = L.lw;
  G.words = L.words;
  return G;
}

void check_layout(const VolumeMeshLayout& L, const char* who) {
  if (L.w <= 0 || L.h <= 0 || L.d <= 0 || L.words == 0 || L.blocks == 0 || L.lw != (L.w + 64) / 64 ||
      (uint64_t)L.lw * (uint64_t)(L.h + 1) * (uint64_t)(L.d + 1) != L.words ||
      L.blocks != (L.words + L.scan_block - 1) / L.scan_block)
    throw DeviceError(std::string(who) + ": not a layout of volume_mesh_layout");
}

}  // namespace

VolumeMeshLayout volume_mesh_layout(int w, int h, int d, int scan_block) {
  if (w <= 0 || h <= 0 || d <= 0) throw DeviceError("volume mesh: empty volume");
  if (scan_block == 0) scan_block = kVolumeMeshScanBlock;
  if (scan_block < kVolumeMeshMinScanBlock || scan_block > kVolumeMeshMaxScanBlock)
    throw DeviceError("volume mesh: the scan block must be " + std::to_string(kVolumeMeshMinScanBlock) + " .. " +
                      std::to_string(kVolumeMeshMaxScanBlock) + " lattice words (got " + std::to_string(scan_block) + ")");
  VolumeMeshLayout L;
  L.w = w, L.h = h, L.d = d;
  L.lw = (w + 64) / 64;
  const uint64_t words = (uint64_t)L.lw * (uint64_t)(h + 1) * (uint64_t)(d + 1);
  if (words >= (1ull << 31))
    throw DeviceError("volume mesh: the lattice of a " + std::to_string(w) + " x " + std::to_string(h) + " x " + std::to_string(d) +
                      " volume has 2^31 words or more");
  L.words = (uint32_t)words;
  L.scan_block = (uint32_t)scan_block;
  L.blocks = (L.words + L.scan_block - 1) / L.scan_block;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  L.off_head = 0;
  L.off_bits = up(sizeof(VolumeMeshHead));
  L.off_counts = L.off_bits + up((size_t)4 * L.words * sizeof(uint64_t));
  L.off_blocks = L.off_counts + up((size_t)4 * L.words * sizeof(uint32_t));
  L.bytes = L.off_blocks + up((size_t)4 * L.blocks * sizeof(uint32_t));
  return L;
}

size_t volume_mesh_work_bytes(int w, int h, int d, int scan_block) { return volume_mesh_layout(w, h, d, scan_block).bytes; }

void launch_volume_mesh(const uint64_t* dilated, const VolumeMeshLayout& L, void* work, VolumeMeshHead* h_head,
                        hipStream_t stream) {
  check_layout(L, "launch_volume_mesh");
  if (!dilated || !work || !h_head) throw DeviceError("launch_volume_mesh: null buffer");
  const MeshGeom G = geom_of(L);
  uint8_t* base = static_cast<uint8_t*>(work);
  auto* head = reinterpret_cast<VolumeMeshHead*>(base + L.off_head);
  auto* bits = reinterpret_cast<uint64_t*>(base + L.off_bits);
  auto* cnt = reinterpret_cast<uint32_t*>(base + L.off_counts);
  auto* bt = reinterpret_cast<uint32_t*>(base + L.off_blocks);
  check_hip(hipMemsetAsync(head, 0, sizeof(VolumeMeshHead), stream), "volume mesh head");
  const uint32_t grid = (L.words + kMeshThreads - 1) / kMeshThreads;
  mesh_classify_kernel<<<grid, kMeshThreads, 0, stream>>>(G, dilated, bits, cnt, head);
  check_launch("mesh_classify_kernel");
  mesh_totals_kernel<<<L.blocks, kMeshThreads, 0, stream>>>(L.words, L.scan_block, L.blocks, cnt, bt);
  check_launch("mesh_totals_kernel");
  mesh_scan_kernel<<<1, kMeshThreads, 0, stream>>>(L.blocks, bt, head);
  check_launch("mesh_scan_kernel");
  mesh_downsweep_kernel<<<L.blocks, kMeshThreads, 0, stream>>>(L.words, L.scan_block, L.blocks, cnt, bt);
  check_launch("mesh_downsweep_kernel");
  check_hip(hipMemcpyAsync(h_head, head, sizeof(VolumeMeshHead), hipMemcpyDeviceToHost, stream), "D2H volume mesh head");
}

void launch_volume_mesh_emit(const uint64_t* dilated, const VolumeMeshLayout& L, const void* work, const VolumeMeshHead& totals,
                             int placement, float sx, float sy, float sz, float* positions, uint32_t* quads, hipStream_t stream) {
  check_layout(L, "launch_volume_mesh_emit");
  if (placement != kMeshCorner && placement != kMeshNets) throw DeviceError("launch_volume_mesh_emit: placement must be corner or nets");
  const uint64_t V = totals.total[0], Q = totals.total[1] + totals.total[2] + totals.total[3];
  const std::string err = mesh::size_error(V, Q, ~0ull);
  if (!err.empty()) throw DeviceError("launch_volume_mesh_emit: " + err);
  if (!dilated || !work || (V && !positions) || (Q && !quads)) throw DeviceError("launch_volume_mesh_emit: null buffer");
  if (V == 0 && Q == 0) return;  // an empty mask: nothing to write
  const MeshGeom G = geom_of(L);
  const uint8_t* base = static_cast<const uint8_t*>(work);
  const auto* bits = reinterpret_cast<const uint64_t*>(base + L.off_bits);
  const auto* pre = reinterpret_cast<const uint32_t*>(base + L.off_counts);
  const uint32_t grid = (L.words + kMeshThreads - 1) / kMeshThreads;
  mesh_vertices_kernel<<<grid, kMeshThreads, 0, stream>>>(G, dilated, bits, pre, placement, sx, sy, sz, (uint32_t)V, positions);
  check_launch("mesh_vertices_kernel");
  mesh_quads_kernel<<<grid, kMeshThreads, 0, stream>>>(G, dilated, bits, pre, (uint32_t)totals.total[1], (uint32_t)totals.total[2],
                                                       (uint32_t)Q, quads);
  check_launch("mesh_quads_kernel");
}

void preload_volume_mesh() {
  hipFuncAttributes a;
  for (const void* f : {reinterpret_cast<const void*>(&mesh_classify_kernel), reinterpret_cast<const void*>(&mesh_totals_kernel),
                        reinterpret_cast<const void*>(&mesh_scan_kernel), reinterpret_cast<const void*>(&mesh_downsweep_kernel),
                        reinterpret_cast<const void*>(&mesh_vertices_kernel), reinterpret_cast<const void*>(&mesh_quads_kernel)})
    check_hip(hipFuncGetAttributes(&a, f), "preload volume mesh kernels");
}

}  // namespace nm03::gpu
