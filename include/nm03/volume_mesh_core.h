// nm03/volume_mesh_core.h — what one thread of the K15 kernels (src/kernels/k15_volume_mesh.hip) does for
// its word of the LATTICE, as host/device functions. measure::volume_mesh_words walks the words one after
// the other on the host, so the word arithmetic and the index rule are checked without a GPU.
//
// The mask is d planes of h rows of n = ceil(w / 64) u64 words (LSB = left-most voxel). The lattice is
// (d + 1) planes of (h + 1) rows of lw = ceil((w + 1) / 64) words: bit b of word (k, j, kw) is corner
// (i = 64·kw + b, j, k). For a lattice row the four mask rows of its windows are (j − 1 … j, k − 1 … k);
// word kw of a mask row holds the upper voxels x = i of the windows, the same row shifted up by one bit,
// with bit 63 of word kw − 1 carried in, the lower voxels x = i − 1.
#pragma once

#include <cstdint>

#include "nm03/measure.h"
#include "nm03/volume_mesh.h"

namespace nm03::meshcore {

NM03_HD int pop64(uint64_t v) { return __builtin_popcountll(v); }
NM03_HD int ctz64(uint64_t v) { return __builtin_ctzll(v); }
NM03_HD uint64_t below(int b) { return b >= 64 ? ~0ull : ((1ull << b) - 1ull); }  // the bits under bit b, 0 ≤ b ≤ 64

struct MeshGeom {
  int w, h, d;
  int n;           // mask words per row
  int lw;          // lattice words per row
  uint32_t words;  // lattice words: lw · (h + 1) · (d + 1)
  NM03_HD uint32_t word_index(int k, int j, int kw) const {
    return ((uint32_t)k * (uint32_t)(h + 1) + (uint32_t)j) * (uint32_t)lw + (uint32_t)kw;
  }
};

// Word (z, y, k) of the mask, masked to the width; 0 outside the volume.
NM03_HD uint64_t mask_word(const uint64_t* vol, const MeshGeom& G, int z, int y, int k) {
  if (z < 0 || z >= G.d || y < 0 || y >= G.h || k < 0 || k >= G.n) return 0ull;
  return vol[((size_t)z * (size_t)G.h + (size_t)y) * (size_t)G.n + (size_t)k] & row_word_mask(k, G.w);
}

// The 8 voxel words of lattice word (k, j, kw): index dx + 2·dy + 4·dz as in mesh::nets_sums, bit b of
// each the voxel of corner 64·kw + b.
struct WindowWords {
  uint64_t v[8];
};
NM03_HD WindowWords window_words(const uint64_t* vol, const MeshGeom& G, int k, int j, int kw) {
  WindowWords W;
  for (int dz = 0; dz < 2; ++dz)
    for (int dy = 0; dy < 2; ++dy) {
      const int z = k - 1 + dz, y = j - 1 + dy;
      const uint64_t cur = mask_word(vol, G, z, y, kw), prev = mask_word(vol, G, z, y, kw - 1);
      W.v[1 + 2 * dy + 4 * dz] = cur;
      W.v[0 + 2 * dy + 4 * dz] = (cur << 1) | (prev >> 63);
    }
  return W;
}
NM03_HD uint32_t window_bits(const WindowWords& W, int b) {
  uint32_t win = 0;
  for (int v = 0; v < 8; ++v) win |= (uint32_t)((W.v[v] >> b) & 1ull) << v;
  return win;
}

// ---- launch 1: classify -----------------------------------------------------------------------------
struct MeshWord {
  uint64_t mixed, fx, fy, fz;
  uint32_t voxels;  // set voxels of mask word (k, j, kw): every mask word belongs to one lattice word
};
NM03_HD MeshWord classify_word(const uint64_t* vol, const MeshGeom& G, int k, int j, int kw) {
  const WindowWords W = window_words(vol, G, k, j, kw);
  uint64_t any = 0ull, all = ~0ull;
  for (int v = 0; v < 8; ++v) any |= W.v[v], all &= W.v[v];
  const uint64_t lattice = row_word_mask(kw, G.w + 1);  // corners i ≤ w
  MeshWord r;
  r.mixed = any & ~all & lattice;
  const uint64_t up = W.v[7];  // voxel p itself: the upper voxel of every face at p
  r.fx = (j < G.h && k < G.d) ? (up ^ W.v[6]) & lattice : 0ull;  // against (i − 1, j, k), 0 ≤ i ≤ w
  r.fy = (k < G.d) ? (up ^ W.v[5]) : 0ull;                       // against (i, j − 1, k): both words end at i < w
  r.fz = (j < G.h) ? (up ^ W.v[3]) : 0ull;                       // against (i, j, k − 1)
  r.voxels = (uint32_t)pop64(up);
  return r;
}

// ---- launch 4: vertices -----------------------------------------------------------------------------
// Every mixed corner of lattice word (k, j, kw) = `mixed`, the first at vertex index `first`.
NM03_HD void word_vertices(const uint64_t* vol, const MeshGeom& G, int k, int j, int kw, uint64_t mixed, uint32_t first,
                           int placement, float sx, float sy, float sz, float* positions) {
  if (mixed == 0ull) return;
  WindowWords W;
  if (placement == kMeshNets) W = window_words(vol, G, k, j, kw);
  uint32_t at = first;
  for (uint64_t t = mixed; t; t &= t - 1, ++at) {
    const int b = ctz64(t);
    float p[3];
    mesh::vertex_mm(placement, (kw << 6) + b, j, k, placement == kMeshNets ? window_bits(W, b) : 0u, sx, sy, sz, p);
    positions[3 * (size_t)at + 0] = p[0];
    positions[3 * (size_t)at + 1] = p[1];
    positions[3 * (size_t)at + 2] = p[2];
  }
}

// ---- launch 5: quads ----------------------------------------------------------------------------------
// The mixed words and vertex prefixes of the lattice rows a word's quads touch: row r = dj + 2·dk is
// (j + dj, k + dk), word kw (m0, p0) and the word after it (m1, p1: corner i + 1 of bit 63).
struct QuadRows {
  uint64_t m0[4];
  uint32_t p0[4], p1[4];
  // Vertex index of corner bit b (0 … 64) of row r.
  NM03_HD uint32_t vid(int r, int b) const { return b >= 64 ? p1[r] : p0[r] + (uint32_t)pop64(m0[r] & below(b)); }
};
NM03_HD QuadRows quad_rows(const MeshGeom& G, const uint64_t* mixed, const uint32_t* prefix, int k, int j, int kw) {
  QuadRows R;
  for (int r = 0; r < 4; ++r) {
    const int jj = j + (r & 1), kk = k + (r >> 1);
    R.m0[r] = 0ull, R.p0[r] = 0u, R.p1[r] = 0u;
    if (jj > G.h || kk > G.d) continue;  // no face of this word reaches past the lattice
    const uint32_t i = G.word_index(kk, jj, kw);
    R.m0[r] = mixed[i];
    R.p0[r] = prefix[i];
    if (kw + 1 < G.lw) R.p1[r] = prefix[i + 1];
  }
  return R;
}

struct Quad {
  uint32_t q[4];
};
// The quad of the face at corner bit b along `axis`: `up` set = the upper voxel p is the set one.
NM03_HD Quad face_quad(const QuadRows& R, int axis, int b, bool up) {
  // rows: 0 = (j, k), 1 = (j + 1, k), 2 = (j, k + 1), 3 = (j + 1, k + 1)
  uint32_t c1, c2, c3;
  const uint32_t c0 = R.vid(0, b);
  if (axis == 0) c1 = R.vid(1, b), c2 = R.vid(3, b), c3 = R.vid(2, b);               // + e_y, + e_y + e_z, + e_z
  else if (axis == 1) c1 = R.vid(2, b), c2 = R.vid(2, b + 1), c3 = R.vid(0, b + 1);  // + e_z, + e_z + e_x, + e_x
  else c1 = R.vid(0, b + 1), c2 = R.vid(1, b + 1), c3 = R.vid(1, b);                 // + e_x, + e_x + e_y, + e_y
  Quad q;
  q.q[0] = c0, q.q[2] = c2;
  q.q[1] = up ? c3 : c1;
  q.q[3] = up ? c1 : c3;
  return q;
}
// Every face of one axis of a lattice word: `faces` its face word, `up` mask word (k, j, kw), the first
// at quad index `first`. store(index, quad).
template <class Store>
NM03_HD void word_quads(const QuadRows& R, int axis, uint64_t faces, uint64_t up, uint32_t first, Store&& store) {
  uint32_t at = first;
  for (uint64_t t = faces; t; t &= t - 1, ++at) {
    const int b = ctz64(t);
    store(at, face_quad(R, axis, b, ((up >> b) & 1ull) != 0ull));
  }
}

}  // namespace nm03::meshcore
