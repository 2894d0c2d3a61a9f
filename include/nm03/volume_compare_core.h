// nm03/volume_compare_core.h — the arithmetic of the K17 kernels (src/kernels/k17_volume_compare.hip) as host/device
// functions. measure::volume_compare_words runs exactly these on the host, so the surface word with its carries,
// the integer square root, the digits of the radix select and the (value, position) order are checked without a
// GPU. Definitions: nm03/volume_compare.h.
//
// The masks are d planes of h rows of wpr = ceil(w / 64) u64 words (LSB = left-most voxel), K5's layout.
//
// The select. The key of a surface voxel is s = ⌊√D⌋ < 2^31, 32 bits. The k-th smallest key is found digit by
// digit from the top, 11 + 11 + 10 bits: a histogram of the digit over the keys that agree with the digits
// found so far gives the digit (icore::select_bin: the first bin whose running total reaches the rank) and the
// rank that is left inside it.
#pragma once

#include <cmath>
#include <cstdint>

#include "nm03/common.h"
#include "nm03/intensity_core.h"
#include "nm03/measure.h"
#include "nm03/volume_distance_core.h"

namespace nm03::vcmp {

constexpr int kPasses = 3;
constexpr int kMaxBins = 2048;  // 11 bits
constexpr uint32_t kPercentile = 95u;

NM03_HD uint32_t digit_shift(int pass) { return pass == 0 ? 21u : pass == 1 ? 10u : 0u; }
NM03_HD uint32_t digit_bins(int pass) { return pass == 2 ? 1024u : 2048u; }
NM03_HD uint32_t digit(uint32_t key, int pass) { return (key >> digit_shift(pass)) & (digit_bins(pass) - 1u); }
// Whether `key` counts in the histogram of `pass`: its digits above that pass's equal those of `prefix` (the digits
// found so far, in place, zeros below).
NM03_HD bool in_prefix(uint32_t key, uint32_t prefix, int pass) {
  return pass == 0 || (key >> digit_shift(pass - 1)) == (prefix >> digit_shift(pass - 1));
}

// ⌊√v⌋ for 0 ≤ v < 2^62: the double square root is off by at most a few units for v above 2^53, the two loops
// make it exact. The result is below 2^31.
NM03_HD uint32_t isqrt_um(int64_t v) {
  const uint64_t u = (uint64_t)v;
  uint64_t r = (uint64_t)sqrt((double)u);
  while (r * r > u) --r;
  while ((r + 1ull) * (r + 1ull) <= u) ++r;
  return (uint32_t)r;
}

// The surface bits of a word m of M from its neighbours, every word masked to the width and 0 outside the
// frame: `prev` / `next` the words before and after it in the row (their bit 63 / bit 0 carry into the x
// neighbours), `up` / `down` the same word of rows y − 1 / y + 1, `back` / `front` of planes z − 1 / z + 1.
NM03_HD uint64_t surface_word(uint64_t m, uint64_t prev, uint64_t next, uint64_t up, uint64_t down, uint64_t back, uint64_t front) {
  const uint64_t left = (m << 1) | (prev >> 63);   // bit x = M(x − 1)
  const uint64_t right = (m >> 1) | (next << 63);  // bit x = M(x + 1)
  return m & ~(left & right & up & down & back & front);
}

// Word (z, y, k) of a bit volume masked to the width, 0 outside the frame.
NM03_HD uint64_t word_at(const uint64_t* bits, int w, int h, int d, int wpr, int z, int y, int k) {
  if (z < 0 || z >= d || y < 0 || y >= h || k < 0 || k >= wpr) return 0ull;
  return bits[((size_t)z * (size_t)h + (size_t)y) * (size_t)wpr + (size_t)k] & row_word_mask(k, w);
}
// S(M)'s word (z, y, k).
NM03_HD uint64_t surface_at(const uint64_t* bits, int w, int h, int d, int wpr, int z, int y, int k) {
  return surface_word(word_at(bits, w, h, d, wpr, z, y, k), word_at(bits, w, h, d, wpr, z, y, k - 1), word_at(bits, w, h, d, wpr, z, y, k + 1),
                      word_at(bits, w, h, d, wpr, z, y - 1, k), word_at(bits, w, h, d, wpr, z, y + 1, k),
                      word_at(bits, w, h, d, wpr, z - 1, y, k), word_at(bits, w, h, d, wpr, z + 1, y, k));
}

}  // namespace nm03::vcmp
