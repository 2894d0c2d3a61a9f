// nm03/volume_mesh.h — the surface of the 3D mask as a closed quad mesh (--volume-mesh, K15).
//
// LATTICE AND VERTICES. The mask is w × h × d voxels; everything outside the volume is 0. Lattice corner
// (i, j, k) has 0 ≤ i ≤ w, 0 ≤ j ≤ h, 0 ≤ k ≤ d; its WINDOW is the 8 voxels (i−1…i, j−1…j, k−1…k). A corner
// is a vertex iff its window is mixed: neither all 0 nor all 1. Vertex indices are the ranks of the mixed
// corners in raster order (k, j, i).
//
// QUADS. For axis a in the order x, y, z and a lattice position p whose other two coordinates lie inside the
// volume and whose p_a lies in [0, dim_a], there is a face at (a, p) iff voxel p − e_a and voxel p differ.
// Quads are ordered by (a, p.z, p.y, p.x). With (a, b, c) cyclic (x → y, z; y → z, x; z → x, y) the corners
// are c0 = p, c1 = p + e_b, c2 = p + e_b + e_c, c3 = p + e_c. When the lower voxel p − e_a is set (outward
// normal +a) the quad is (c0, c1, c2, c3), when the upper voxel is set it is (c0, c3, c2, c1). The triangles
// of a quad are (q0, q1, q2) and (q0, q2, q3).
//
// INVARIANTS. Every corner of a quad is mixed and every mixed corner is used by a quad. The quads of axis
// x, y, z number faces_x, faces_y, faces_z of VolumeMeasure (nm03/measure.h). Every directed edge (u, v)
// occurs as often as (v, u): the mesh is closed (non-manifold only where voxels touch diagonally). With the
// corner positions doubled to integers, 2c − 1, the sum of det(v0, v1, v2) over all triangles is 48 · voxels.
//
// PLACEMENT. `corner`: the lattice corner itself, at c − ½ in voxel index space (voxel centres are at the
// integers). `nets` (naive surface nets): the mean of the midpoints of the window's crossing edges — the
// window has 12 edges, pairs of voxels that differ in one coordinate; an edge crosses when its two voxels
// differ; n is their number and S the sum over them of 2 · (midpoint − corner), each term in {−1, 0, 1}³.
// Per axis the position is N / (2n) with N = (2c − 1) · n + S; `corner` is the case n = 1, S = 0. The quads
// do not depend on the placement. mesh::position_mm, shared by host and device, turns N and n into
// millimetres: spacing · ((float)N / (float)(2n)), an IEEE f32 division and product (no contraction), with
// the spacing of the volume, sz cast to float. Patient orientation and position are not consulted.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "nm03/common.h"

namespace nm03 {

enum MeshPlacement : int { kMeshCorner = 0, kMeshNets = 1 };
enum MeshFormat : int { kMeshPly = 0, kMeshStl = 1 };

struct VolumeMesh {
  int w = 0, h = 0, d = 0;
  int placement = kMeshCorner;
  std::vector<float> positions;  // 3 · V, mm
  std::vector<uint32_t> quads;   // 4 · Q vertex indices: the x-quads, then the y-quads, then the z-quads
  uint64_t quads_x = 0, quads_y = 0, quads_z = 0;
  uint64_t voxels = 0;           // set voxels of the mask
  double k15_s = 0;              // GPU time of K15's launches (0 on the host paths)
  size_t vertices() const { return positions.size() / 3; }
  size_t quad_count() const { return quads.size() / 4; }
};

namespace mesh {

constexpr uint64_t kDefaultMaxMb = 512;
// Lattice words per block of the kernels' blocked scan: the default and the bounds a caller may ask for.
constexpr int kScanBlock = 1024, kMinScanBlock = 64, kMaxScanBlock = 1 << 19;
constexpr const char* kSidecarName = "mesh.json";

// The 8 voxels of a window as bits: bit (dx + 2·dy + 4·dz), d* = 1 for the upper voxel (i, j, k), 0 for the
// lower one (i − 1, j − 1, k − 1). Adds up the crossing edges: *n their number, S their 2 · (midpoint − corner).
NM03_HD void nets_sums(uint32_t win, int* n, int S[3]) {
  int cnt = 0, s0 = 0, s1 = 0, s2 = 0;
  for (int a = 0; a < 3; ++a) {
    const int bit = 1 << a;
    for (int v = 0; v < 8; ++v) {
      if (v & bit) continue;
      if ((((win >> v) ^ (win >> (v | bit))) & 1u) == 0u) continue;
      ++cnt;  // the edge from voxel v to voxel v | bit along axis a: its midpoint has offset 0 along a
      if (a != 0) s0 += (v & 1) ? 1 : -1;
      if (a != 1) s1 += (v & 2) ? 1 : -1;
      if (a != 2) s2 += (v & 4) ? 1 : -1;
    }
  }
  *n = cnt;
  S[0] = s0, S[1] = s1, S[2] = s2;
}

// One coordinate in mm from the numerator N = (2c − 1) · n + S and n.
NM03_HD float position_mm(float spacing, int32_t N, int32_t n) { return spacing * ((float)N / (float)(2 * n)); }

// The three coordinates of the vertex at corner (i, j, k) whose window is `win` (needed for `nets` only).
NM03_HD void vertex_mm(int placement, int i, int j, int k, uint32_t win, float sx, float sy, float sz, float out[3]) {
  int n = 1, S[3] = {0, 0, 0};
  if (placement == kMeshNets) nets_sums(win, &n, S);  // a mixed window has at least one crossing edge
  out[0] = position_mm(sx, (2 * i - 1) * n + S[0], n);
  out[1] = position_mm(sy, (2 * j - 1) * n + S[1], n);
  out[2] = position_mm(sz, (2 * k - 1) * n + S[2], n);
}

const char* placement_name(int p);  // "corner" | "nets"
const char* format_name(int f);     // "ply" | "stl"
const char* file_name(int f);       // "mesh.ply" | "mesh.stl"
bool parse_placement(const std::string& s, int* p);
bool parse_format(const std::string& s, int* f);

// Bytes of the device-side result, the figure --volume-mesh-max-mb caps: 12 · V + 16 · Q.
inline uint64_t result_bytes(uint64_t V, uint64_t Q) { return 12ull * V + 16ull * Q; }
// Empty, or why a mesh of V vertices and Q quads is refused: V and 2 · Q must stay below 2^31 and
// result_bytes within max_bytes. The message names V, Q and the cap.
std::string size_error(uint64_t V, uint64_t Q, uint64_t max_bytes);

// The one writer of each file, used by the GPU path, --cpu and Python: equal arrays give equal bytes.
// PLY: binary_little_endian 1.0, element vertex V (float x, y, z in mm), element face 2Q (list uchar int
// vertex_indices, the two triangles of every quad), fixed comment lines.
std::vector<uint8_t> ply_bytes(const VolumeMesh& m);
// Binary STL: 80 header bytes, the triangle count, then per triangle the f32 normalised cross product
// (v1 − v0) × (v2 − v0) — 0 0 0 for a degenerate triangle —, the three vertices and a zero attribute.
std::vector<uint8_t> stl_bytes(const VolumeMesh& m);
std::vector<uint8_t> file_bytes(const VolumeMesh& m, int format);
// mesh.json: one JSON object on one line (no newline), keys in fixed order — placement, format, file, bytes,
// vertices, quads_x, quads_y, quads_z, triangles, voxels, spacing [sx, sy, sz], bbox_mm [x0, y0, z0, x1, y1,
// z1] (min and max of the positions; null for an empty mesh), surface_mm2 (K8's formula from the quad
// counts), volume_mm3. Doubles as %.9g.
std::string to_json(const VolumeMesh& m, int format, uint64_t bytes, float sx, float sy, double sz);

}  // namespace mesh

namespace golden {

// The mesh of a d × h × w mask (0 / non-zero per voxel) by plain loops over corners and faces.
VolumeMesh volume_mesh(const uint8_t* mask, int w, int h, int d, float sx, float sy, double sz, int placement);

}  // namespace golden

namespace measure {

// The same mesh from the K15 kernels' per-word functions (nm03/volume_mesh_core.h) run on the host over
// the bit volume (d planes of h rows of ceil(w / 64) u64 words), with the kernels' blocked scan at
// `scan_block` lattice words per block (0 = the launcher's default).
VolumeMesh volume_mesh_words(const uint64_t* dilated, int w, int h, int d, float sx, float sy, double sz, int placement,
                             int scan_block = 0);

}  // namespace measure

}  // namespace nm03
