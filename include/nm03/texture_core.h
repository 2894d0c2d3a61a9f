// nm03/texture_core.h — the arithmetic the K12 kernels (src/kernels/k12_texture.hip), the host emulation
// measure::texture_words and the golden model (src/golden/texture.cpp) share for the grey-level
// co-occurrence matrix (GLCM) of TextureGlcm (nm03/measure.h): the discretisation of a sample's key
// and, for the kernels and their emulation only, the per-word pair logic.
//
// Levels. Ng = the number of grey levels (2 … 64), lo / hi = the keys (icore::sample_key) of the
// smallest and largest sample under the mask:
//   level(key) = (hi == lo) ? 0 : min(Ng − 1, ((key − lo) · Ng) / (hi − lo))
// in 32-bit unsigned arithmetic (the largest product is 65535 · 64): IBSI's "fixed bin number",
// 0-based. key == hi gives Ng before the clamp; the clamp exists for that case.
//
// Pairs. Two voxels that are both set, both inside the frame and one index step apart in a FORWARD
// direction: the (dx, dy, dz) with components in {−1, 0, 1} and dz = 1, or dz = 0 and dy = 1, or
// dz = dy = 0 and dx = 1 — thirteen in 3D, the four with dz = 0 in 2D. Pixel spacing is not consulted.
// A pair with levels (a, b) adds 1 to C[a][b] and 1 to C[b][a]: one matrix merged over all directions.
//
// Words. The kernels take a u64 mask word (z, y, k), bit = x − 64k, and meet its forward partners in
// five rows: its own row (dx = 1 only) and the rows (y + 1, z), (y − 1, z + 1), (y, z + 1), (y + 1, z + 1)
// (dx = −1, 0, 1 each): 1 + 3 + 3 · 3 = 13. For a row with words `prev`, `cur`, `next` at k − 1, k, k + 1,
// neighbour_word(prev, cur, next, dx) has bit b set when the voxel at x + dx of that row is set, so
// `own & neighbour_word(...)` are the bits of the word that have a partner in that direction. They
// accumulate DIRECTED counts D[a][b] (a = the word's own voxel) and symmetrise once: C = D + Dᵀ.
//
// Hand-checkable example (Haralick 1973): the image
//   0 0 1 1
//   0 0 1 1
//   0 2 2 2
//   2 2 3 3
// with a full mask and Ng = 4. lo = 0, hi = 3, the levels are the values. pairs = 42: 12 for (1,0), 9 for
// (1,1), 12 for (0,1), 9 for (−1,1). The merged matrix is
//   16  4  6  0
//    4 12  5  0
//    6  5 12  6
//    0  0  6  2
// with contrast 0.928571429, angular second moment 0.109693878 and joint entropy 3.37687122 bits; the
// matrix of direction (1,0) alone is the textbook [[4,2,1,0],[2,4,0,0],[1,0,6,1],[0,0,1,2]].
#pragma once

#include <cstdint>

#include "nm03/common.h"

namespace nm03::tcore {

constexpr int kMinLevels = 2;
constexpr int kMaxLevels = 64;
constexpr int kDefaultLevels = 32;

// The 32-bit cells. A voxel is the first member of at most `dirs` forward pairs and every pair adds 2 to
// a diagonal cell when both levels are equal, so a cell can reach 2 · dirs · samples (a homogeneous full
// mask comes close). The matrix is exact while that fits a uint32: always in 2D (8 · 4096² < 2^32), and
// for samples ≤ kMaxExactSamples3D = 165 191 049 over the thirteen directions of 3D. Beyond it a cell may
// have wrapped, in the kernels and in the golden model alike, so such a record is refused
// (measure::check_glcm_exact) wherever one becomes a result, never turned into features.
constexpr uint32_t kDirections2D = 4u;
constexpr uint32_t kDirections3D = 13u;
NM03_HD bool cells_exact(uint64_t samples, uint32_t dirs) {  // samples < 2^32 (voxels of a volume)
  return samples <= 0xFFFFFFFFull / (2ull * (uint64_t)dirs);
}
constexpr uint64_t kMaxExactSamples3D = 0xFFFFFFFFull / (2ull * kDirections3D);
static_assert(kMaxExactSamples3D == 165191049ull, "the 3D bound of the 32-bit cells");

NM03_HD uint32_t level(uint32_t key, uint32_t lo, uint32_t hi, uint32_t ng) {
  if (hi == lo) return 0u;
  const uint32_t l = ((key - lo) * ng) / (hi - lo);
  return l < ng - 1u ? l : ng - 1u;
}

// level() for many keys of one (lo, hi, ng) without a division per key: (key − lo) · ng < 2^22 and
// hi − lo < 2^16, so with M = ⌊2^40 / (hi − lo)⌋ + 1 the quotient is ((key − lo) · ng · M) >> 40 exactly
// (Granlund & Montgomery 1994: 2^40 ≥ 2^22 · 2^16; the product stays below 2^63). The kernels and their
// host emulation use it; the golden model divides.
struct Leveler {
  uint32_t lo, ng, top;  // top = ng − 1
  uint64_t magic;        // 0: hi == lo, every level is 0
  NM03_HD Leveler(uint32_t lo_, uint32_t hi_, uint32_t ng_)
      : lo(lo_), ng(ng_), top(ng_ - 1u), magic(hi_ == lo_ ? 0ull : (1ull << 40) / (uint64_t)(hi_ - lo_) + 1ull) {}
  NM03_HD uint32_t operator()(uint32_t key) const {  // key in [lo, hi]
    const uint32_t l = (uint32_t)(((uint64_t)((key - lo) * ng) * magic) >> 40);
    return l < top ? l : top;
  }
};

// The rows a word meets its forward partners in, as (dy, dz); row 0 (its own) only with dx = 1.
constexpr int kPairRows = 5;
NM03_HD int pair_row_dy(int r) { return r == 0 ? 0 : r == 1 ? 1 : r - 3; }
NM03_HD int pair_row_dz(int r) { return r < 2 ? 0 : 1; }
NM03_HD int pair_row_first_dx(int r) { return r == 0 ? 1 : -1; }

// Bit b: the voxel at x + dx of a row whose words k − 1, k, k + 1 are prev, cur, next (0 outside the frame).
NM03_HD uint64_t neighbour_word(uint64_t prev, uint64_t cur, uint64_t next, int dx) {
  if (dx == 0) return cur;
  if (dx > 0) return (cur >> 1) | (next << 63);
  return (cur << 1) | (prev >> 63);
}

}  // namespace nm03::tcore
