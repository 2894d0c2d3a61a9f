// nm03/intensity_core.h — the arithmetic the K11 kernels (src/kernels/k11_intensity.hip), the host
// emulation measure::intensity_words and the golden model's checks share for the exact order statistics
// of IntensityStats (nm03/measure.h): the 16-bit key of a sample and its inverse, the rank of a
// percentile and the bin search of the two-pass radix select.
//
// The select: a 256-bin histogram of key >> 8 over all samples gives, for each target rank, the high
// byte of the answer (the first bin whose running total reaches the rank) and the rank that is left
// inside that bin; a 256-bin histogram of key & 255 over the samples of that bin gives the low byte the
// same way. Two byte-wide passes instead of one 16-bit histogram: 65536 u32 counters are 256 KiB, more
// than a CU's LDS, while 256 are 1 KiB.
#pragma once

#include <cstdint>

#include "nm03/common.h"
#include "nm03/measure.h"

namespace nm03::icore {

constexpr int kPercentiles = 5;
constexpr int kBins = 256;

// p of pct[j].
NM03_HD uint32_t percentile_of(int j) { return j == 0 ? 10u : j == 1 ? 25u : j == 2 ? 50u : j == 3 ? 75u : 90u; }

// Key order is value order for every pixel type: unsigned values as they are, signed values with the
// sign bit flipped. A slice or a volume has one type.
NM03_HD uint16_t sample_key(int32_t v, uint8_t type) { return (uint16_t)((uint16_t)v ^ (type == kI16 ? 0x8000u : 0u)); }
NM03_HD int32_t key_sample(uint16_t key, uint8_t type) {
  return type == kI16 ? (int32_t)(int16_t)(uint16_t)(key ^ 0x8000u) : (int32_t)key;
}

// Nearest rank, 1-based: k = ceil(p · n / 100) in 64-bit integers; 0 only for n = 0.
NM03_HD uint64_t percentile_rank(uint32_t p, uint64_t n) { return ((uint64_t)p * n + 99u) / 100u; }

struct BinRank {
  uint32_t bin;   // the first bin whose running total reaches the rank
  uint64_t rank;  // the rank inside that bin, 1-based
};

// `rank` is 1 … Σ hist. A rank past the total (never asked for) gives the last bin.
template <class Count>
NM03_HD BinRank select_bin(const Count* hist, int bins, uint64_t rank) {
  uint64_t below = 0;
  int b = 0;
  for (; b < bins - 1; ++b) {
    const uint64_t c = (uint64_t)hist[b];
    if (below + c >= rank) break;
    below += c;
  }
  BinRank r;
  r.bin = (uint32_t)b;
  r.rank = rank - below;
  return r;
}

// Targets that fall into one high-byte bin share the low-byte histogram of the first of them:
// slot[j] = the smallest i ≤ j with bin[i] = bin[j] (ranks grow with j, so equal bins are neighbours).
NM03_HD void share_slots(const BinRank* t, uint32_t* slot) {
  for (int j = 0; j < kPercentiles; ++j) {
    int i = j;
    while (i > 0 && t[i - 1].bin == t[j].bin) --i;
    slot[j] = (uint32_t)i;
  }
}

// The low-byte histogram a sample with high byte `hi` counts in, or −1: the first target in its bin.
NM03_HD int slot_of(const BinRank* t, uint32_t hi) {
  for (int j = 0; j < kPercentiles; ++j)
    if (t[j].bin == hi) return j;
  return -1;
}

}  // namespace nm03::icore
