// The surface mesh of nm03/volume_mesh.h on the host: golden::volume_mesh by plain loops over corners and
// faces (the reference of every comparison), measure::volume_mesh_words by the K15 kernels' own per-word
// functions and blocked scan, and the writers of mesh.ply, mesh.stl and mesh.json that the GPU path, --cpu
// and Python share.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "nm03/volume_mesh.h"
#include "nm03/volume_mesh_core.h"

namespace nm03 {

namespace mesh {

const char* placement_name(int p) { return p == kMeshNets ? "nets" : "corner"; }
const char* format_name(int f) { return f == kMeshStl ? "stl" : "ply"; }
const char* file_name(int f) { return f == kMeshStl ? "mesh.stl" : "mesh.ply"; }

bool parse_placement(const std::string& s, int* p) {
  if (s == "corner") *p = kMeshCorner;
  else if (s == "nets") *p = kMeshNets;
  else return false;
  return true;
}

bool parse_format(const std::string& s, int* f) {
  if (s == "ply") *f = kMeshPly;
  else if (s == "stl") *f = kMeshStl;
  else return false;
  return true;
}

std::string size_error(uint64_t V, uint64_t Q, uint64_t max_bytes) {
  const uint64_t bytes = result_bytes(V, Q);
  const bool wide = V >= (1ull << 31) || 2ull * Q >= (1ull << 31);
  if (!wide && bytes <= max_bytes) return "";
  char buf[320];
  if (wide)
    std::snprintf(buf, sizeof buf,
                  "a mesh of %llu vertices and %llu quads does not fit 32-bit indices (vertices and 2 x quads must stay below "
                  "2^31; the cap is %llu bytes)",
                  (unsigned long long)V, (unsigned long long)Q, (unsigned long long)max_bytes);
  else
    std::snprintf(buf, sizeof buf,
                  "a mesh of %llu vertices and %llu quads takes %llu bytes, above the cap of %llu bytes (--volume-mesh-max-mb)",
                  (unsigned long long)V, (unsigned long long)Q, (unsigned long long)bytes, (unsigned long long)max_bytes);
  return buf;
}

namespace {

void put_bytes(std::vector<uint8_t>& o, const void* p, size_t n) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  o.insert(o.end(), b, b + n);
}

// The two triangles of quad q as vertex indices.
inline void quad_triangles(const uint32_t* q, uint32_t t[2][3]) {
  t[0][0] = q[0], t[0][1] = q[1], t[0][2] = q[2];
  t[1][0] = q[0], t[1][1] = q[2], t[1][2] = q[3];
}

}  // namespace

std::vector<uint8_t> ply_bytes(const VolumeMesh& m) {
  const size_t V = m.vertices(), Q = m.quad_count();
  char head[512];
  const int hn = std::snprintf(head, sizeof head,
                               "ply\nformat binary_little_endian 1.0\ncomment nm03 volume mesh\ncomment placement %s\n"
                               "comment units mm\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                               "element face %zu\nproperty list uchar int vertex_indices\nend_header\n",
                               placement_name(m.placement), V, 2 * Q);
  std::vector<uint8_t> o;
  o.reserve((size_t)hn + 12 * V + 26 * Q);
  put_bytes(o, head, (size_t)hn);
  put_bytes(o, m.positions.data(), 12 * V);
  for (size_t i = 0; i < Q; ++i) {
    uint32_t t[2][3];
    quad_triangles(&m.quads[4 * i], t);
    for (int k = 0; k < 2; ++k) {
      uint8_t rec[13];
      rec[0] = 3;
      const int32_t idx[3] = {(int32_t)t[k][0], (int32_t)t[k][1], (int32_t)t[k][2]};
      std::memcpy(rec + 1, idx, 12);
      put_bytes(o, rec, 13);
    }
  }
  return o;
}

std::vector<uint8_t> stl_bytes(const VolumeMesh& m) {
  const size_t Q = m.quad_count();
  std::vector<uint8_t> o(80, 0);
  const char* title = "nm03 volume mesh, binary STL, mm";
  std::memcpy(o.data(), title, std::strlen(title));
  o.reserve(84 + 100 * Q);
  const uint32_t ntri = (uint32_t)(2 * Q);
  put_bytes(o, &ntri, 4);
  for (size_t i = 0; i < Q; ++i) {
    uint32_t t[2][3];
    quad_triangles(&m.quads[4 * i], t);
    for (int k = 0; k < 2; ++k) {
      const float* a = &m.positions[3 * (size_t)t[k][0]];
      const float* b = &m.positions[3 * (size_t)t[k][1]];
      const float* c = &m.positions[3 * (size_t)t[k][2]];
      const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
      float nrm[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
      const float len = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
      if (len > 0.f && std::isfinite(len)) nrm[0] /= len, nrm[1] /= len, nrm[2] /= len;
      else nrm[0] = nrm[1] = nrm[2] = 0.f;
      float rec[12];
      std::memcpy(rec, nrm, 12);
      std::memcpy(rec + 3, a, 12);
      std::memcpy(rec + 6, b, 12);
      std::memcpy(rec + 9, c, 12);
      put_bytes(o, rec, 48);
      const uint16_t attr = 0;
      put_bytes(o, &attr, 2);
    }
  }
  return o;
}

std::vector<uint8_t> file_bytes(const VolumeMesh& m, int format) { return format == kMeshStl ? stl_bytes(m) : ply_bytes(m); }

std::string to_json(const VolumeMesh& m, int format, uint64_t bytes, float sx, float sy, double sz) {
  char buf[256];
  std::string s;
  const size_t V = m.vertices(), Q = m.quad_count();
  std::snprintf(buf, sizeof buf, "{\"placement\":\"%s\",\"format\":\"%s\",\"file\":\"%s\",\"bytes\":%llu", placement_name(m.placement),
                format_name(format), file_name(format), (unsigned long long)bytes);
  s += buf;
  std::snprintf(buf, sizeof buf, ",\"vertices\":%zu,\"quads_x\":%llu,\"quads_y\":%llu,\"quads_z\":%llu,\"triangles\":%zu,\"voxels\":%llu",
                V, (unsigned long long)m.quads_x, (unsigned long long)m.quads_y, (unsigned long long)m.quads_z, 2 * Q,
                (unsigned long long)m.voxels);
  s += buf;
  const double dx = (double)sx, dy = (double)sy, dz = sz;
  std::snprintf(buf, sizeof buf, ",\"spacing\":[%.9g,%.9g,%.9g]", dx, dy, dz);
  s += buf;
  if (V == 0) {
    s += ",\"bbox_mm\":null";
  } else {
    float lo[3] = {m.positions[0], m.positions[1], m.positions[2]}, hi[3] = {lo[0], lo[1], lo[2]};
    for (size_t i = 1; i < V; ++i)
      for (int a = 0; a < 3; ++a) {
        const float p = m.positions[3 * i + (size_t)a];
        lo[a] = p < lo[a] ? p : lo[a];
        hi[a] = p > hi[a] ? p : hi[a];
      }
    std::snprintf(buf, sizeof buf, ",\"bbox_mm\":[%.9g,%.9g,%.9g,%.9g,%.9g,%.9g]", (double)lo[0], (double)lo[1], (double)lo[2],
                  (double)hi[0], (double)hi[1], (double)hi[2]);
    s += buf;
  }
  std::snprintf(buf, sizeof buf, ",\"surface_mm2\":%.9g,\"volume_mm3\":%.9g}",
                (double)m.quads_x * dy * dz + (double)m.quads_y * dx * dz + (double)m.quads_z * dx * dy,
                (double)m.voxels * dx * dy * dz);
  s += buf;
  return s;
}

}  // namespace mesh

namespace golden {

VolumeMesh volume_mesh(const uint8_t* mask, int w, int h, int d, float sx, float sy, double sz, int placement) {
  if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("volume_mesh: empty volume");
  if (placement != kMeshCorner && placement != kMeshNets) throw std::invalid_argument("volume_mesh: placement must be corner or nets");
  if (((uint64_t)w + 1) * ((uint64_t)h + 1) * ((uint64_t)d + 1) >= (1ull << 31))
    throw std::invalid_argument("volume_mesh: the lattice must stay below 2^31 corners");
  auto vox = [&](int x, int y, int z) -> int {
    if (x < 0 || x >= w || y < 0 || y >= h || z < 0 || z >= d) return 0;
    return mask[((size_t)z * h + y) * (size_t)w + x] ? 1 : 0;
  };
  VolumeMesh m;
  m.w = w, m.h = h, m.d = d;
  m.placement = placement;
  const float fz = (float)sz;
  std::vector<int32_t> rank((size_t)(w + 1) * (h + 1) * (d + 1), -1);
  auto corner = [&](int i, int j, int k) -> size_t { return ((size_t)k * (h + 1) + j) * (size_t)(w + 1) + i; };
  int32_t next = 0;
  for (int k = 0; k <= d; ++k)
    for (int j = 0; j <= h; ++j)
      for (int i = 0; i <= w; ++i) {
        uint32_t win = 0;
        for (int v = 0; v < 8; ++v) win |= (uint32_t)vox(i - 1 + (v & 1), j - 1 + ((v >> 1) & 1), k - 1 + (v >> 2)) << v;
        if (win == 0u || win == 0xFFu) continue;
        rank[corner(i, j, k)] = next++;
        float p[3];
        mesh::vertex_mm(placement, i, j, k, win, sx, sy, fz, p);
        m.positions.insert(m.positions.end(), p, p + 3);
      }
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) m.voxels += (uint64_t)vox(x, y, z);
  const int e[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const int dim[3] = {w, h, d};
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    int top[3] = {w, h, d};  // exclusive bounds of p: the face axis reaches dim_a
    top[a] = dim[a] + 1;
    uint64_t count = 0;
    for (int pz = 0; pz < top[2]; ++pz)
      for (int py = 0; py < top[1]; ++py)
        for (int px = 0; px < top[0]; ++px) {
          const int lower = vox(px - e[a][0], py - e[a][1], pz - e[a][2]), upper = vox(px, py, pz);
          if (lower == upper) continue;
          const int c0[3] = {px, py, pz};
          int cs[4][3];
          for (int t = 0; t < 3; ++t) {
            cs[0][t] = c0[t];
            cs[1][t] = c0[t] + e[b][t];
            cs[2][t] = c0[t] + e[b][t] + e[c][t];
            cs[3][t] = c0[t] + e[c][t];
          }
          const int order_lower[4] = {0, 1, 2, 3}, order_upper[4] = {0, 3, 2, 1};
          const int* order = lower ? order_lower : order_upper;
          for (int t = 0; t < 4; ++t) {
            const int32_t r = rank[corner(cs[order[t]][0], cs[order[t]][1], cs[order[t]][2])];
            if (r < 0) throw std::logic_error("volume_mesh: a quad corner is not a vertex");
            m.quads.push_back((uint32_t)r);
          }
          ++count;
        }
    (a == 0 ? m.quads_x : a == 1 ? m.quads_y : m.quads_z) = count;
  }
  return m;
}

}  // namespace golden

namespace measure {

VolumeMesh volume_mesh_words(const uint64_t* dilated, int w, int h, int d, float sx, float sy, double sz, int placement,
                             int scan_block) {
  using namespace meshcore;
  if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("volume_mesh_words: empty volume");
  if (placement != kMeshCorner && placement != kMeshNets)
    throw std::invalid_argument("volume_mesh_words: placement must be corner or nets");
  if (scan_block == 0) scan_block = mesh::kScanBlock;
  if (scan_block < mesh::kMinScanBlock || scan_block > mesh::kMaxScanBlock)
    throw std::invalid_argument("volume_mesh_words: scan_block must be 64 .. 2^19");
  MeshGeom G;
  G.w = w, G.h = h, G.d = d;
  G.n = (w + 63) / 64;
  G.lw = (w + 1 + 63) / 64;
  const uint64_t words = (uint64_t)G.lw * (uint64_t)(h + 1) * (uint64_t)(d + 1);
  if (words >= (1ull << 31)) throw std::invalid_argument("volume_mesh_words: the lattice must stay below 2^31 words");
  G.words = (uint32_t)words;
  // launch 1
  std::vector<uint64_t> bits[4];
  std::vector<uint32_t> pre[4];
  for (int s = 0; s < 4; ++s) bits[s].resize(G.words), pre[s].resize(G.words);
  VolumeMesh m;
  m.w = w, m.h = h, m.d = d;
  m.placement = placement;
  for (int k = 0; k <= d; ++k)
    for (int j = 0; j <= h; ++j)
      for (int kw = 0; kw < G.lw; ++kw) {
        const MeshWord r = classify_word(dilated, G, k, j, kw);
        const uint32_t i = G.word_index(k, j, kw);
        bits[0][i] = r.mixed, bits[1][i] = r.fx, bits[2][i] = r.fy, bits[3][i] = r.fz;
        for (int s = 0; s < 4; ++s) pre[s][i] = (uint32_t)pop64(bits[s][i]);
        m.voxels += r.voxels;
      }
  // launch 2: block totals, the scan of the totals, the downsweep
  const uint32_t nb = (G.words + (uint32_t)scan_block - 1) / (uint32_t)scan_block;
  uint64_t total[4];
  for (int s = 0; s < 4; ++s) {
    std::vector<uint32_t> bt(nb, 0), off(nb, 0);
    for (uint32_t b = 0; b < nb; ++b)
      for (uint32_t i = b * (uint32_t)scan_block; i < std::min<uint64_t>(G.words, (uint64_t)(b + 1) * scan_block); ++i) bt[b] += pre[s][i];
    uint64_t carry = 0;
    for (uint32_t b = 0; b < nb; ++b) off[b] = (uint32_t)carry, carry += bt[b];
    total[s] = carry;
    for (uint32_t b = 0; b < nb; ++b) {
      uint32_t run = off[b];
      for (uint32_t i = b * (uint32_t)scan_block; i < std::min<uint64_t>(G.words, (uint64_t)(b + 1) * scan_block); ++i) {
        const uint32_t c = pre[s][i];
        pre[s][i] = run;
        run += c;
      }
    }
  }
  // launch 3: the host check of the index width (the byte cap is the caller's)
  const std::string err = mesh::size_error(total[0], total[1] + total[2] + total[3], ~0ull);
  if (!err.empty()) throw std::runtime_error("volume_mesh_words: " + err);
  m.quads_x = total[1], m.quads_y = total[2], m.quads_z = total[3];
  m.positions.resize(3 * (size_t)total[0]);
  m.quads.resize(4 * (size_t)(total[1] + total[2] + total[3]));
  const uint32_t base[3] = {0u, (uint32_t)total[1], (uint32_t)(total[1] + total[2])};
  const float fz = (float)sz;
  for (int k = 0; k <= d; ++k)
    for (int j = 0; j <= h; ++j)
      for (int kw = 0; kw < G.lw; ++kw) {
        const uint32_t i = G.word_index(k, j, kw);
        word_vertices(dilated, G, k, j, kw, bits[0][i], pre[0][i], placement, sx, sy, fz, m.positions.data());  // launch 4
        if ((bits[1][i] | bits[2][i] | bits[3][i]) == 0ull) continue;  // launch 5
        const QuadRows R = quad_rows(G, bits[0].data(), pre[0].data(), k, j, kw);
        const uint64_t up = mask_word(dilated, G, k, j, kw);
        for (int a = 0; a < 3; ++a)
          word_quads(R, a, bits[1 + a][i], up, base[a] + pre[1 + a][i], [&](uint32_t at, const Quad& q) {
            std::memcpy(&m.quads[4 * (size_t)at], q.q, 16);
          });
      }
  return m;
}

}  // namespace measure

}  // namespace nm03
