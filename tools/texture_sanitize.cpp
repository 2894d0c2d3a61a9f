// Stand-alone host check of the texture code (nm03/texture_core.h, src/golden/texture.cpp) for sanitizer
// builds: the golden model, the host emulation of K12's per-word pair logic and the feature derivation on
// a few shapes that reach every edge of the word logic (a width that is no multiple of 64, a second word,
// one-pixel extents, an empty mask, signed samples, 2 and 64 levels, a volume). It needs no GPU and no
// Python. Build it with the host sources it calls and run it:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/texture_sanitize.cpp src/golden/texture.cpp src/golden/intensity.cpp src/golden/measure.cpp \
//       src/golden/diameters.cpp src/golden/volume_measure.cpp -o texture_sanitize && ./texture_sanitize
//
// It prints one line per case and exits 0 when the emulation equals the golden model everywhere.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "nm03/golden.h"
#include "nm03/measure.h"
#include "nm03/texture_core.h"
#include "nm03/volume.h"

using namespace nm03;

namespace {

uint32_t rng_state = 12345u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

struct Case {
  const char* name;
  int w, h, d;
  PixelType type;
  int stored_bits, levels;
  int density;  // percent of voxels set; 0 = empty mask
};

bool run(const Case& c) {
  const size_t n = (size_t)c.w * c.h * c.d;
  std::vector<uint8_t> mask(n);
  std::vector<uint16_t> raw(n);
  for (size_t i = 0; i < n; ++i) {
    mask[i] = (int)(rnd() % 100u) < c.density;
    raw[i] = (uint16_t)rnd();  // junk above stored_bits included
  }
  measure::Glcm gold;
  if (c.d == 1) {
    golden::SliceInput s;
    s.w = c.w, s.h = c.h, s.type = c.type, s.stored_bits = c.stored_bits, s.raw = raw;
    gold = golden::measure_texture(mask, s, c.levels);
  } else {
    VolumeInput v;
    v.w = c.w, v.h = c.h, v.d = c.d, v.type = c.type, v.stored_bits = c.stored_bits, v.raw = raw;
    gold = golden::measure_texture(mask, v, c.levels);
  }
  // Bit planes with every storage bit past the width set, as a kernel may find them.
  const int wpr = (c.w + 63) / 64;
  std::vector<uint64_t> planes((size_t)c.d * c.h * wpr, 0ull);
  for (int z = 0; z < c.d; ++z)
    for (int y = 0; y < c.h; ++y) {
      uint64_t* row = planes.data() + ((size_t)z * c.h + y) * wpr;
      for (int x = 0; x < c.w; ++x)
        if (mask[((size_t)z * c.h + y) * c.w + x]) row[x >> 6] |= 1ull << (x & 63);
      row[wpr - 1] |= ~row_word_mask(wpr - 1, c.w);
    }
  const measure::Glcm emu = measure::texture_words(planes.data(), raw.data(), (size_t)c.w * c.h, c.w, c.h, c.d, wpr,
                                                   (uint8_t)c.type, (uint8_t)c.stored_bits, c.levels);
  const measure::GlcmFeatures f = measure::glcm_features(gold.c.data(), c.levels);
  const std::string keys = measure::texture_keys(gold.c.data(), c.levels);
  const bool ok = gold.c == emu.c && gold.head.pairs == emu.head.pairs && gold.head.samples == emu.head.samples &&
                  gold.head.key_lo == emu.head.key_lo && gold.head.key_hi == emu.head.key_hi && f.pairs == gold.head.pairs &&
                  !keys.empty();
  std::printf("%-22s samples %8llu pairs %9llu nonzero %5llu contrast %.9g  %s\n", c.name, (unsigned long long)gold.head.samples,
              (unsigned long long)gold.head.pairs, (unsigned long long)f.nonzero, f.contrast, ok ? "ok" : "MISMATCH");
  return ok;
}

}  // namespace

int main() {
  const Case cases[] = {
      {"1x1", 1, 1, 1, kU16, 16, 32, 100},        {"2x2", 2, 2, 1, kU16, 16, 32, 100},
      {"65x2", 65, 2, 1, kU16, 16, 32, 100},      {"128x3", 128, 3, 1, kU16, 16, 8, 100},
      {"70x5", 70, 5, 1, kU16, 16, 32, 70},       {"empty", 70, 5, 1, kU16, 16, 32, 0},
      {"i16_12_junk", 70, 7, 1, kI16, 12, 16, 70}, {"levels_2", 130, 9, 1, kU16, 16, 2, 70},
      {"levels_64", 130, 9, 1, kU16, 16, 64, 70}, {"3x300", 3, 300, 1, kU16, 12, 63, 60},
      {"2x2x2", 2, 2, 2, kU16, 16, 32, 100},      {"70x9x12", 70, 9, 12, kU16, 16, 32, 70},
      {"i16_130x5x3", 130, 5, 3, kI16, 16, 64, 80}, {"1x1x2", 1, 1, 2, kU16, 16, 4, 100},
  };
  bool ok = true;
  for (const Case& c : cases) ok = run(c) && ok;
  std::printf("%s\n", ok ? "texture_sanitize: all cases agree" : "texture_sanitize: MISMATCH");
  return ok ? 0 : 1;
}
