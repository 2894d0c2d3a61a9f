// nm03/volume_diameters_core.h — the arithmetic of the K13 kernels (src/kernels/k13_volume_diameters.hip,
// nm03/measure.h VolumeLesionDiameters) as host/device functions: the kernels call them from their
// threads, measure::volume_diameters_words calls them from plain loops, so the candidate logic, the
// bound and the tile rule are checked without a GPU.
//
// CANDIDATES. A lesion's candidates are the two extreme voxels (xlo, xhi) of each of its rows (z, y): a
// squared distance to a fixed voxel is strictly convex in x, so on a row it is largest ONLY at an
// extreme, and every pair that attains a maximum — the ties too — is a pair of candidates. The same
// holds inside a plane, and the projection on a normal is linear in x, so the perpendicular's ends are
// row extremes as well (with dy = 0 a whole row ties and its smallest voxel is xlo). The rows of a lesion
// are kept in a table of (xlo, xhi) per (rank, z, y); the ROW SLOTS of a lesion are the rows of its
// bounding box in raster order, slot r ↔ (z0 + r / ny, y0 + r mod ny), empty ones (xlo > xhi) included.
//
// ORDER. A pair is ranked by its squared distance, then by key = pos(a) << 32 | pos(b) with
// pos = (z·h + y)·w + x < 2^32 — the lexicographic (za, ya, xa, zb, yb, xb) of the definition, and inside
// one plane (z, ya, xa, yb, xb). Only pairs with pos(a) ≤ pos(b) are looked at.
//
// TILES. kTileRows consecutive row slots are a tile with a bounding box. A tile pair is skipped when the
// largest distance between the two boxes is STRICTLY below the lesion's bound — a squared distance that
// some pair of candidates really has (the best among the extremes of 13 directions, and per plane of 4),
// so every pair that ties with the maximum survives — and, for the axial search, also when the tiles
// share no plane.
#pragma once

#include <cstdint>

#include "nm03/measure.h"

namespace nm03::vdcore {

constexpr int kTileRows = 128;  // row slots per tile: at most 256 candidates
constexpr int kNumDirs = 13;    // the forward directions of the 26-neighbourhood
constexpr int kNumPlaneDirs = 4;
constexpr int32_t kRowNoLo = 0x7FFFFFFF, kRowNoHi = -1;  // an empty row of the table
constexpr uint32_t kNoPos = 0xFFFFFFFFu;                 // no voxel: w·h·d < 2^32 − 1

struct RowExt {
  int32_t lo, hi;
};

// dir(i) = (dx, dy, dz); the first kNumPlaneDirs lie in the plane.
NM03_HD void direction(int i, int& dx, int& dy, int& dz) {
  // packed two bits per component (0, 1, 3 = −1): x | y << 2 | z << 4
  constexpr uint8_t t[kNumDirs] = {0x01, 0x04, 0x05, 0x0D, 0x10, 0x11, 0x31, 0x14, 0x34, 0x15, 0x35, 0x1D, 0x3D};
  const int v = t[i];
  auto c = [](int b) { return b == 3 ? -1 : b; };
  dx = c(v & 3), dy = c((v >> 2) & 3), dz = c((v >> 4) & 3);
}

// A candidate: its centre in micrometres (each below 2^31) and its position.
struct Cand {
  uint32_t X, Y, Z, pos;
};

struct Grid {
  int w, h, d;
  uint32_t ux, uy, uz;
  NM03_HD uint32_t pos(int x, int y, int z) const { return ((uint32_t)z * (uint32_t)h + (uint32_t)y) * (uint32_t)w + (uint32_t)x; }
  NM03_HD Cand cand(int x, int y, int z) const {
    return Cand{(uint32_t)x * ux, (uint32_t)y * uy, (uint32_t)z * uz, pos(x, y, z)};
  }
  NM03_HD void voxel(uint32_t p, int32_t& x, int32_t& y, int32_t& z) const {
    const uint32_t row = p / (uint32_t)w;
    x = (int32_t)(p - row * (uint32_t)w);
    z = (int32_t)(row / (uint32_t)h);
    y = (int32_t)(row - (uint32_t)z * (uint32_t)h);
  }
};

// Axis (0, 1, 2) whose (dim − 1) · u reaches 2^31, −1 when none does.
NM03_HD int extent_overflow(int w, int h, int d, const uint32_t um[3]) {
  const int dim[3] = {w, h, d};
  for (int a = 0; a < 3; ++a)
    if ((uint64_t)(dim[a] - 1) * (uint64_t)um[a] >= (1ull << 31)) return a;
  return -1;
}

// The rows of a lesion's bounding box.
struct Rows {
  int32_t y0, z0, ny, nz;
  NM03_HD uint32_t count() const { return (uint32_t)ny * (uint32_t)nz; }
  NM03_HD uint32_t tiles() const { return (count() + (uint32_t)kTileRows - 1u) / (uint32_t)kTileRows; }
  NM03_HD void row(uint32_t r, int& y, int& z) const {
    const uint32_t q = r / (uint32_t)ny;
    z = z0 + (int)q;
    y = y0 + (int)(r - q * (uint32_t)ny);
  }
};
NM03_HD Rows rows_of(const int32_t bbox_lo[3], const int32_t bbox_hi[3]) {
  return Rows{bbox_lo[1], bbox_lo[2], bbox_hi[1] - bbox_lo[1] + 1, bbox_hi[2] - bbox_lo[2] + 1};
}
// Index of row (rank, z, y) in the table.
NM03_HD size_t row_index(int rank, int z, int y, int h, int d) {
  return ((size_t)rank * (size_t)d + (size_t)z) * (size_t)h + (size_t)y;
}

// A best pair: d2 and key; `none` loses against every pair.
struct Best {
  uint64_t d2, key;
};
NM03_HD Best best_none() { return Best{0ull, ~0ull}; }
NM03_HD bool best_beats(uint64_t d2, uint64_t key, const Best& b) { return d2 > b.d2 || (d2 == b.d2 && key < b.key); }
NM03_HD void best_take(const Best& c, Best& b) {
  if (best_beats(c.d2, c.key, b)) b = c;
}

NM03_HD uint64_t sq_diff(uint32_t a, uint32_t b) {
  const uint32_t t = a > b ? a - b : b - a;  // < 2^31
  return (uint64_t)t * (uint64_t)t;
}

// The pair (a, b) as d² + 1 for the 3D and the axial search; 0 = not a pair to look at: b is no voxel, a comes
// after b (the business of the reversed call) or, for v2, the two lie in different planes.
NM03_HD void pair_values(const Cand& a, const Cand& b, uint64_t& v3, uint64_t& v2) {
  const bool ok = b.pos != kNoPos && a.pos <= b.pos;
  const uint64_t dxy = sq_diff(a.X, b.X) + sq_diff(a.Y, b.Y);
  v3 = ok ? dxy + sq_diff(a.Z, b.Z) + 1ull : 0ull;
  v2 = ok && a.Z == b.Z ? dxy + 1ull : 0ull;
}
// The pair into the 3D and the axial best.
NM03_HD void pair_update(const Cand& a, const Cand& b, Best& b3, Best& b2) {
  uint64_t v3, v2;
  pair_values(a, b, v3, v2);
  const uint64_t key = ((uint64_t)a.pos << 32) | (uint64_t)b.pos;
  if (v3 && best_beats(v3 - 1ull, key, b3)) b3 = Best{v3 - 1ull, key};
  if (v2 && best_beats(v2 - 1ull, key, b2)) b2 = Best{v2 - 1ull, key};
}

// ---- the bound ------------------------------------------------------------------------------------
// An extreme of a direction: the projection and the voxel; larger projection first, then the earlier
// voxel. The minimum is the maximum of the negated direction.
struct Extreme {
  int64_t proj;
  uint32_t pos;
};
NM03_HD Extreme extreme_none() { return Extreme{INT64_MIN, kNoPos}; }
NM03_HD bool extreme_beats(const Extreme& c, const Extreme& e) { return c.proj > e.proj || (c.proj == e.proj && c.pos < e.pos); }
NM03_HD int64_t project(const Cand& c, int dx, int dy, int dz) {
  return (int64_t)dx * (int64_t)c.X + (int64_t)dy * (int64_t)c.Y + (int64_t)dz * (int64_t)c.Z;
}
// Row (z, y) = e into the two extremes (along +dir and −dir) of a direction.
NM03_HD void extreme_row(const Grid& g, int z, int y, const RowExt& e, int dx, int dy, int dz, Extreme& hi, Extreme& lo) {
  if (e.lo > e.hi) return;
  for (int s = 0; s < 2; ++s) {
    const Cand c = g.cand(s ? e.hi : e.lo, y, z);
    const int64_t p = project(c, dx, dy, dz);
    const Extreme a{p, c.pos}, b{-p, c.pos};
    if (extreme_beats(a, hi)) hi = a;
    if (extreme_beats(b, lo)) lo = b;
  }
}
// The squared distance of two extreme voxels (none: 0); `axial` drops z.
NM03_HD uint64_t extreme_d2(const Grid& g, uint32_t pa, uint32_t pb, bool axial) {
  if (pa == kNoPos || pb == kNoPos) return 0ull;
  int32_t xa, ya, za, xb, yb, zb;
  g.voxel(pa, xa, ya, za);
  g.voxel(pb, xb, yb, zb);
  const Cand a = g.cand(xa, ya, za), b = g.cand(xb, yb, zb);
  const uint64_t dxy = sq_diff(a.X, b.X) + sq_diff(a.Y, b.Y);
  return axial ? dxy : dxy + sq_diff(a.Z, b.Z);
}

// ---- tiles ----------------------------------------------------------------------------------------
struct TileBox {
  int32_t x0, y0, z0, x1, y1, z1;  // inclusive; x0 > x1: no candidate
  int32_t pad[2];
};
NM03_HD TileBox tile_none() { return TileBox{0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF, -1, -1, -1, {0, 0}}; }
NM03_HD void tile_add(int z, int y, const RowExt& e, TileBox& t) {
  if (e.lo > e.hi) return;
  t.x0 = e.lo < t.x0 ? e.lo : t.x0, t.x1 = e.hi > t.x1 ? e.hi : t.x1;
  t.y0 = y < t.y0 ? y : t.y0, t.y1 = y > t.y1 ? y : t.y1;
  t.z0 = z < t.z0 ? z : t.z0, t.z1 = z > t.z1 ? z : t.z1;
}
// The largest |a − b|·u over a in [a0, a1], b in [b0, b1], squared.
NM03_HD uint64_t far_sq(int32_t a0, int32_t a1, int32_t b0, int32_t b1, uint32_t u) {
  const int32_t m1 = a1 - b0, m2 = b1 - a0;  // one of them is ≥ 0
  const uint32_t t = (uint32_t)(m1 > m2 ? m1 : m2) * u;
  return (uint64_t)t * (uint64_t)t;
}
// Whether the pair of tiles A, B can hold neither a 3D pair at or above l3 nor an axial pair at or
// above l2. With l3 = l2 = 0 (the brute-force switch) only pairs with an empty tile are skipped.
NM03_HD bool tile_pair_skipped(const TileBox& A, const TileBox& B, const Grid& g, uint64_t l3, uint64_t l2) {
  if (A.x0 > A.x1 || B.x0 > B.x1) return true;
  const uint64_t fxy = far_sq(A.x0, A.x1, B.x0, B.x1, g.ux) + far_sq(A.y0, A.y1, B.y0, B.y1, g.uy);
  const uint64_t f3 = fxy + far_sq(A.z0, A.z1, B.z0, B.z1, g.uz);
  const bool share_plane = A.z0 <= B.z1 && B.z0 <= A.z1;
  return f3 < l3 && (!share_plane || fxy < l2);
}

// ---- the perpendicular ------------------------------------------------------------------------------
// p of voxel (x, y) for the axial pair's (dx, dy): |dx·y|, |dy·x| < w·h < 2^32.
NM03_HD int64_t perp_proj(int32_t dx, int32_t dy, int32_t x, int32_t y) {
  return -(int64_t)dy * (int64_t)x + (int64_t)dx * (int64_t)y;
}

}  // namespace nm03::vdcore
