// nm03/volume_distance_core.h — the per-line arithmetic of the K16 kernels (src/kernels/k16_volume_distance.hip)
// as host/device functions. measure::volume_distance_words runs exactly these on the host over a plain
// array, so the in-word nearest bit, the word walk, the outward search with its stop rule and the
// (value, position) order are checked without a GPU. Definitions: nm03/volume_distance.h.
//
// The mask is d planes of h rows of wpr = ceil(w / 64) u64 words (LSB = left-most voxel). The map is built
// by three separable passes:
//   rows    g(x, y, z) = the index distance along x to the nearest S voxel of the row, kNoRow for none
//   cols    c(x, y, z) = min over y′ of (g(x, y′, z)·ux)² + ((y − y′)·uy)²
//   planes  D(x, y, z) = min over z′ of c(x, y, z′) + ((z − z′)·uz)²
// The two minimisations walk outward from the voxel itself, k = 0, 1, 2 …, and stop at the first k with
// (k·u)² ≥ best: every candidate at distance k′ ≥ k along the line adds at least (k·u)² to a non-negative
// value, so none of them can lie below `best`, and the result is the minimum over the whole line. With a
// cap c they also stop at the first k with (k·u)² > c²: what lies further is above the cap whatever it
// holds, and every value above c² is replaced by kNoDistance at the end of the pass, so a minimum ≤ c² is
// never missed and a value > c² never leaves a pass.
#pragma once

#include <cstdint>

#include "nm03/measure.h"
#include "nm03/volume_distance.h"

namespace nm03::vdist {

constexpr uint16_t kNoRow = 0xFFFFu;   // no S voxel in this row (a row holds at most 65535 voxels)
constexpr int kNoneInWord = 64;        // nearest_in_word: the word holds no S bit
constexpr int32_t kNoWordWalk = -1;    // left_reach / right_reach: no S bit on that side

// Word k of a row of S: the mask word or, for the background, its complement, masked to the width.
NM03_HD uint64_t set_word(const uint64_t* row, int k, int w, bool to_background) {
  const uint64_t v = row[k];
  return (to_background ? ~v : v) & row_word_mask(k, w);
}

// The index distance from bit b (0 … 63) to the nearest set bit of s, kNoneInWord when s is 0: the highest
// set bit at or below b by count-leading-zeros, the lowest at or above b by count-trailing-zeros.
NM03_HD int nearest_in_word(uint64_t s, int b) {
  const uint64_t at_or_below = s & ((2ull << b) - 1ull);  // b = 63: 2 << 63 wraps to 0, the mask is all ones
  const uint64_t at_or_above = s >> b;
  int best = kNoneInWord;
  if (at_or_below) best = b - (63 - __builtin_clzll(at_or_below));
  if (at_or_above) {
    const int r = __builtin_ctzll(at_or_above);
    if (r < best) best = r;
  }
  return best;
}

// The index distance from bit 0 of word kw to the highest bit of the non-zero word s = word k < kw, and from bit
// 63 of word kw to the lowest bit of s = word k > kw (both ≥ 1).
NM03_HD int32_t left_reach_of(int kw, int k, uint64_t s) { return 64 * (kw - 1 - k) + 1 + __builtin_clzll(s); }
NM03_HD int32_t right_reach_of(int kw, int k, uint64_t s) { return 64 * (k - 1 - kw) + 1 + __builtin_ctzll(s); }
// The index distance from bit 0 of word kw to the nearest S bit in the words before it (≥ 1), or kNoWordWalk:
// a walk to the left through the row's words to the first non-zero one, bounded by the words per row.
NM03_HD int32_t left_reach(const uint64_t* row, int w, bool to_background, int kw) {
  for (int k = kw - 1; k >= 0; --k) {
    const uint64_t s = set_word(row, k, w, to_background);
    if (s) return left_reach_of(kw, k, s);
  }
  return kNoWordWalk;
}
// The index distance from bit 63 of word kw to the nearest S bit in the words after it (≥ 1), or kNoWordWalk.
NM03_HD int32_t right_reach(const uint64_t* row, int wpr, int w, bool to_background, int kw) {
  for (int k = kw + 1; k < wpr; ++k) {
    const uint64_t s = set_word(row, k, w, to_background);
    if (s) return right_reach_of(kw, k, s);
  }
  return kNoWordWalk;
}
// g of bit b of a word: the nearest of the word's own bits and the two reaches.
NM03_HD uint16_t row_distance(uint64_t s, int b, int32_t left, int32_t right) {
  int32_t best = nearest_in_word(s, b);
  bool any = best != kNoneInWord;
  if (left != kNoWordWalk && (!any || b + left < best)) best = b + left, any = true;
  if (right != kNoWordWalk && (!any || 63 - b + right < best)) best = 63 - b + right, any = true;
  return any ? (uint16_t)best : kNoRow;
}

// (steps · u)² for 0 ≤ steps < the line's length: the product stays below 2^31 by the extent rule, so one 32-bit
// and one 32 × 32 → 64-bit multiplication do.
NM03_HD int64_t square_um(int steps, uint32_t u) {
  const uint32_t v = (uint32_t)steps * u;
  return (int64_t)((uint64_t)v * (uint64_t)v);
}
// The cols pass's value of a row distance.
NM03_HD int64_t row_value(uint16_t g, uint32_t ux) { return g == kNoRow ? kNoDistance : square_um((int)g, ux); }

// min over j of at(j) + ((i − j)·u)² along a line of n values (kNoDistance = none), walking outward with the
// stop rule above. cap2 < 0 = no cap.
template <class F>
NM03_HD int64_t search_line(int n, int i, uint32_t u, int64_t cap2, F at) {
  int64_t best = at(i);
  for (int k = 1; k < n; ++k) {  // bounded by the line
    const int64_t s = square_um(k, u);
    if (s >= best) break;
    if (cap2 >= 0 && s > cap2) break;
    const bool lo = i - k >= 0, hi = i + k < n;
    if (!lo && !hi) break;
    if (lo) {
      const int64_t v = at(i - k);
      if (v != kNoDistance && v + s < best) best = v + s;
    }
    if (hi) {
      const int64_t v = at(i + k);
      if (v != kNoDistance && v + s < best) best = v + s;
    }
  }
  return best;
}
// The end of a pass: a value above the cap is none.
NM03_HD int64_t capped(int64_t v, int64_t cap2) { return cap2 >= 0 && v > cap2 ? kNoDistance : v; }

// The thickness order: the larger value wins, a tie goes to the smaller raster position. A candidate is a
// mask voxel whose value is a distance; `kNoCandidate` as position marks "none yet" and loses to any.
constexpr uint64_t kNoCandidate = ~0ull;
NM03_HD bool better(int64_t va, uint64_t pa, int64_t vb, uint64_t pb) {
  if (pa == kNoCandidate) return false;
  if (pb == kNoCandidate) return true;
  return va > vb || (va == vb && pa < pb);
}

}  // namespace nm03::vdist
