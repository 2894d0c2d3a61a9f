// Stand-alone host check of the per-lesion diameter code (nm03/volume_diameters_core.h,
// src/golden/volume_diameters.cpp) for sanitizer builds: the golden model against the host run of K13's
// candidate, bound and tile logic, with the tile skipping on and off, on a few shapes that reach the edges
// of the word and tile logic (a width that is no multiple of 64, a second word, one-voxel lesions, an empty
// and a full mask, more rows than a tile, anisotropic spacing, spacings just below the 2^31 bound), and the
// sidecar text. It needs no GPU and no Python. Build it with the host sources it calls and run it:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/volume_diameters_sanitize.cpp src/golden/volume_diameters.cpp src/golden/volume_measure.cpp \
//       src/golden/measure.cpp -o volume_diameters_sanitize && ./volume_diameters_sanitize
//
// It prints one line per case and exits 0 when the host run equals the golden model everywhere.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "nm03/golden.h"
#include "nm03/measure.h"

using namespace nm03;

namespace {

uint32_t rng_state = 2463534242u;
uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

struct Case {
  const char* name;
  int w, h, d;
  int density;  // percent of voxels set; 0 = empty, 100 = full, −1 = an ellipsoid that fills the frame
  int lesions, connectivity;
  uint32_t um[3];
};

bool run(const Case& c) {
  const size_t n = (size_t)c.w * c.h * c.d;
  std::vector<uint8_t> mask(n, 0);
  for (int z = 0; z < c.d; ++z)
    for (int y = 0; y < c.h; ++y)
      for (int x = 0; x < c.w; ++x) {
        bool set;
        if (c.density < 0) {
          const double fx = (x + 0.5) / c.w * 2 - 1, fy = (y + 0.5) / c.h * 2 - 1, fz = (z + 0.5) / c.d * 2 - 1;
          set = fx * fx + fy * fy + fz * fz <= 1.0;
        } else {
          set = (int)(rnd() % 100u) < c.density;
        }
        mask[((size_t)z * c.h + y) * c.w + x] = set;
      }
  const int wpr = (c.w + 63) / 64;
  std::vector<uint64_t> words((size_t)c.d * c.h * wpr, 0ull);
  for (int z = 0; z < c.d; ++z)
    for (int y = 0; y < c.h; ++y)
      for (int x = 0; x < c.w; ++x)
        if (mask[((size_t)z * c.h + y) * c.w + x]) words[((size_t)z * c.h + y) * wpr + (x >> 6)] |= 1ull << (x & 63);
  const std::vector<VolumeLesionDiameters> gold =
      golden::measure_volume_diameters(mask, c.w, c.h, c.d, c.connectivity, c.lesions, c.um);
  bool ok = true;
  uint64_t skipped[2] = {0, 0};
  for (int brute = 0; brute < 2; ++brute) {
    std::vector<VolumeLesionDiameters> out((size_t)c.lesions);
    const int count = measure::volume_diameters_words(words.data(), c.w, c.h, c.d, wpr, c.connectivity, c.lesions, c.um,
                                                      brute != 0, out.data(), &skipped[brute]);
    ok = ok && count == (int)gold.size();
    for (int i = 0; ok && i < count; ++i) ok = std::memcmp(&out[(size_t)i], &gold[(size_t)i], sizeof(VolumeLesionDiameters)) == 0;
  }
  ok = ok && skipped[1] == 0;
  // The sidecar text: the lesion keys of as many empty lesion objects, then the diameter keys put in.
  std::string text = "{\"mean\":null,\"lesions_max\":" + std::to_string(c.lesions) + ",\"lesions\":[";
  for (size_t i = 0; i < gold.size(); ++i) text += std::string(i ? "," : "") + "{\"voxels\":1,\"mean\":0}";
  text += "]}\n";
  const std::string with = measure::insert_diameter_keys(text, gold.data(), (int)gold.size(), c.um);
  ok = ok && with.size() > text.size() && with.find("\"diameters_spacing_um\"") != std::string::npos;
  std::printf("%-22s %3d x %3d x %3d  lesions %2zu  skipped %4llu  %s\n", c.name, c.w, c.h, c.d, gold.size(),
              (unsigned long long)skipped[0], ok ? "ok" : "MISMATCH");
  return ok;
}

}  // namespace

int main() {
  const Case cases[] = {
      {"one word", 40, 9, 5, 30, 8, 26, {1000, 1000, 1000}},
      {"word edge", 65, 7, 4, 50, 64, 6, {977, 1020, 3300}},
      {"three words", 130, 5, 3, 90, 3, 26, {500, 500, 5000}},
      {"specks", 70, 13, 7, 3, 64, 26, {1000, 1000, 1000}},
      {"empty", 70, 5, 3, 0, 3, 26, {1000, 1000, 1000}},
      {"full", 66, 5, 4, 100, 2, 6, {1000, 1000, 1000}},
      {"one voxel wide", 1, 1, 9, 100, 1, 6, {1, 1, 1}},
      {"ellipsoid, many tiles", 40, 37, 61, -1, 2, 26, {500, 500, 5000}},
      {"ellipsoid, word edge", 80, 39, 30, -1, 1, 6, {977, 1020, 3300}},
      {"just below 2^31", 3, 2, 2, 100, 1, 26, {(1u << 30) - 1u, (1u << 31) - 1u, (1u << 31) - 1u}},
  };
  bool ok = true;
  for (const Case& c : cases) ok = run(c) && ok;
  // The refusal at (dim − 1) · u ≥ 2^31.
  try {
    const uint32_t um[3] = {1u << 30, 1000u, 1000u};
    (void)golden::measure_volume_diameters(std::vector<uint8_t>(12, 1), 3, 2, 2, 26, 1, um);
    ok = false;
    std::printf("the refusal did not come\n");
  } catch (const std::invalid_argument&) {
  }
  std::printf("%s\n", ok ? "volume_diameters_sanitize: all cases agree" : "volume_diameters_sanitize: MISMATCH");
  return ok ? 0 : 1;
}
