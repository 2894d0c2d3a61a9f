// Stand-alone host check of the distance-map code (nm03/volume_distance_core.h, src/golden/volume_distance.cpp) for
// sanitizer builds: the host run of K16's per-line functions against the golden model (both polarities, capped and
// not, with every storage bit past the width set), the direct margin against the threshold of the map, the
// thickness in both forms and the sidecar keys, on a few shapes that reach every edge of the word and line logic
// (a width that is no multiple of 64, a second and third word, lines of length 1, an empty and a full mask, one
// voxel in a corner, spacings near the extent rule's bound). It needs no GPU and no Python. Build it with the host
// source it calls and run it:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/volume_distance_sanitize.cpp src/golden/volume_distance.cpp -o volume_distance_sanitize \
//       && ./volume_distance_sanitize
//
// It prints one line per case and exits 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "nm03/volume_distance.h"
#include "nm03/volume_distance_core.h"

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
  uint32_t um[3];
  int per_mille;  // voxels set per thousand; 0 = empty, 1000 = full, −1 = one voxel in the corner
};

bool run(const Case& c) {
  const size_t n = (size_t)c.w * c.h * c.d;
  std::vector<uint8_t> mask(n, 0);
  if (c.per_mille < 0) mask[0] = 1;
  else
    for (size_t i = 0; i < n; ++i) mask[i] = (int)(rnd() % 1000u) < c.per_mille;
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
  bool ok = true;
  std::vector<int64_t> emu(n);
  const int64_t caps[] = {-1, 0, (int64_t)c.um[0], (int64_t)c.um[0] + c.um[0] / 2, (int64_t)1 << 40};
  for (int bg = 0; bg < 2; ++bg)
    for (int64_t cap : caps) {
      const std::vector<int64_t> gold = golden::volume_distance(mask, c.w, c.h, c.d, c.um, bg != 0, cap);
      measure::volume_distance_words(planes.data(), c.w, c.h, c.d, wpr, c.um, bg != 0, cap, emu.data());
      ok = ok && gold == emu;
    }
  const std::vector<int64_t> D = golden::volume_distance(mask, c.w, c.h, c.d, c.um, false, -1);
  size_t margin_vox = 0;
  for (int64_t r : {(int64_t)0, (int64_t)c.um[0], (int64_t)c.um[2], 2 * (int64_t)c.um[1] + 1}) {
    const std::vector<uint8_t> m = golden::dilate3d_mm(mask, c.w, c.h, c.d, c.um, r);
    margin_vox = 0;
    for (size_t i = 0; i < n; ++i) {
      ok = ok && (m[i] != 0) == (D[i] <= r * r);
      margin_vox += m[i];
    }
  }
  const VolumeThickness tg = golden::volume_thickness(mask, c.w, c.h, c.d, c.um);
  const VolumeThickness tw = measure::volume_thickness_words(planes.data(), c.w, c.h, c.d, wpr, c.um);
  ok = ok && tg.inscribed_um2 == tw.inscribed_um2 && tg.found == tw.found && tg.at[0] == tw.at[0] && tg.at[1] == tw.at[1] &&
       tg.at[2] == tw.at[2];
  const std::string base = "{\"width\":1,\"mean\":null,\"lesions_max\":1,\"lesions\":[]}\n";
  const std::string text = measure::insert_thickness_keys(base, tg, c.um);
  const std::string keys = measure::thickness_keys(tg, c.um);
  ok = ok && text.size() == base.size() + keys.size() && text.find(keys + ",\"lesions_max\":1") != std::string::npos;
  ok = ok && measure::insert_thickness_keys("{\"width\":1}\n", tg, c.um) == "{\"width\":1" + keys + "}\n";
  std::printf("%-18s %4d x %3d x %3d  margin %7zu  inscribed_um2 %14llu at (%d, %d, %d)  %s\n", c.name, c.w, c.h, c.d, margin_vox,
              (unsigned long long)tg.inscribed_um2, tg.at[0], tg.at[1], tg.at[2], ok ? "ok" : "MISMATCH");
  return ok;
}

}  // namespace

int main() {
  const Case cases[] = {
      {"1x1x1", 1, 1, 1, {1000, 1000, 1000}, 1000},    {"1x1x1_empty", 1, 1, 1, {1000, 1000, 1000}, 0},
      {"line_x_200", 200, 1, 1, {700, 1000, 1000}, 20}, {"line_y_37", 1, 37, 1, {1000, 300, 1000}, 200},
      {"line_z_9", 1, 1, 9, {1000, 1000, 2500}, 200},   {"64x3x2", 64, 3, 2, {500, 500, 5000}, 300},
      {"65x3x2", 65, 3, 2, {500, 500, 5000}, 300},      {"70x9x3", 70, 9, 3, {391, 703, 6500}, 300},
      {"130x20x6", 130, 20, 6, {391, 703, 6500}, 50},   {"130x20x6_sparse", 130, 20, 6, {1000, 1000, 1000}, 2},
      {"empty", 70, 5, 4, {1000, 1000, 1000}, 0},       {"full", 70, 5, 4, {1000, 1000, 1000}, 1000},
      {"corner_voxel", 130, 20, 6, {391, 703, 6500}, -1}, {"2x300x1", 2, 300, 1, {1000, 800, 1000}, 10},
      {"near_the_bound", 9, 5, 3, {150000000u, 200000000u, 400000000u}, 300},
  };
  bool ok = true;
  for (const Case& c : cases) ok = run(c) && ok;
  // the extent rule: (8 · 2^28)² = 2^62 is refused, one voxel less is not
  const uint32_t big[3] = {1u << 28, 1, 1};
  ok = ok && !measure::volume_distance_extent_error(9, 1, 1, big).empty() && measure::volume_distance_extent_error(8, 1, 1, big).empty();
  std::printf("%s\n", ok ? "volume_distance_sanitize: all cases agree" : "volume_distance_sanitize: MISMATCH");
  return ok ? 0 : 1;
}
