// Stand-alone host check of the comparison code (nm03/volume_compare_core.h, src/golden/volume_compare.cpp) for
// sanitizer builds: the host run of K17's functions (the surface word with its carries, the integer square root, the
// 11 + 11 + 10 bit radix select, the (value, position) order) against the golden model (six-neighbour test, whole-line
// distance map, a sort), with every storage bit past the width set, the surface words against the golden surface,
// compare(A, B) against compare(B, A), the three worked examples of nm03/volume_compare.h and the writer of
// compare.json and comparisons.csv, on shapes that reach every edge of the word logic (widths 1, 63, 64, 65 and 130,
// one plane, one row, empty and full masks, keys above 2^24, spacings near the extent rule's bound). It needs no GPU
// and no Python. Build it with the host sources it calls and run it:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/volume_compare_sanitize.cpp src/golden/volume_compare.cpp src/golden/volume_compare_lesions.cpp \
//       src/golden/volume_distance.cpp \
//       -o volume_compare_sanitize && ./volume_compare_sanitize
//
// It prints one line per case and exits 0 when everything agrees.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "nm03/volume_compare.h"
#include "nm03/volume_compare_core.h"

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
  int a_per_mille, b_per_mille;  // voxels set per thousand; 0 = empty, 1000 = full, −1 = one voxel in a corner
};

std::vector<uint8_t> make_mask(const Case& c, int per_mille, bool far_corner) {
  const size_t n = (size_t)c.w * c.h * c.d;
  std::vector<uint8_t> m(n, 0);
  if (per_mille < 0) m[far_corner ? n - 1 : 0] = 1;
  else
    for (size_t i = 0; i < n; ++i) m[i] = (int)(rnd() % 1000u) < per_mille;
  return m;
}

// Bit planes with every storage bit past the width set, as a kernel may find them.
std::vector<uint64_t> pack_with_junk(const std::vector<uint8_t>& mask, int w, int h, int d) {
  const int wpr = (w + 63) / 64;
  std::vector<uint64_t> planes((size_t)d * h * wpr, 0ull);
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y) {
      uint64_t* row = planes.data() + ((size_t)z * h + y) * wpr;
      for (int x = 0; x < w; ++x)
        if (mask[((size_t)z * h + y) * w + x]) row[x >> 6] |= 1ull << (x & 63);
      row[wpr - 1] |= ~row_word_mask(wpr - 1, w);
    }
  return planes;
}

bool same(const VolumeCompareDirected& p, const VolumeCompareDirected& q) {
  return p.max_um2 == q.max_um2 && p.sum_um == q.sum_um && p.n == q.n && p.p95_um == q.p95_um && p.found == q.found &&
         p.worst[0] == q.worst[0] && p.worst[1] == q.worst[1] && p.worst[2] == q.worst[2];
}
bool same(const VolumeCompare& p, const VolumeCompare& q) {
  return p.a_vox == q.a_vox && p.b_vox == q.b_vox && p.tp_vox == q.tp_vox && p.fp_vox == q.fp_vox && p.fn_vox == q.fn_vox &&
         p.surface_a == q.surface_a && p.surface_b == q.surface_b && same(p.ab, q.ab) && same(p.ba, q.ba);
}

bool run(const Case& c) {
  const std::vector<uint8_t> a = make_mask(c, c.a_per_mille, false), b = make_mask(c, c.b_per_mille, true);
  const int wpr = (c.w + 63) / 64;
  const std::vector<uint64_t> wa = pack_with_junk(a, c.w, c.h, c.d), wb = pack_with_junk(b, c.w, c.h, c.d);
  std::vector<uint64_t> sa(wa.size()), sb(wb.size());
  const VolumeCompare g = golden::compare_volumes(a, b, c.w, c.h, c.d, c.um);
  const VolumeCompare e = measure::volume_compare_words(wa.data(), wb.data(), c.w, c.h, c.d, wpr, c.um, sa.data(), sb.data());
  bool ok = same(g, e);
  // the surface words: the golden surface, and nothing past the width
  const std::vector<uint8_t> ga = golden::volume_surface(a, c.w, c.h, c.d), gb = golden::volume_surface(b, c.w, c.h, c.d);
  for (int z = 0; z < c.d; ++z)
    for (int y = 0; y < c.h; ++y)
      for (int x = 0; x < wpr * 64; ++x) {
        const size_t wi = ((size_t)z * c.h + y) * wpr + (x >> 6);
        const bool ba = (sa[wi] >> (x & 63)) & 1ull, bb = (sb[wi] >> (x & 63)) & 1ull;
        const size_t p = ((size_t)z * c.h + y) * c.w + x;
        ok = ok && ba == (x < c.w && ga[p]) && bb == (x < c.w && gb[p]);
      }
  // the other order
  const VolumeCompare r = measure::volume_compare_words(wb.data(), wa.data(), c.w, c.h, c.d, wpr, c.um);
  ok = ok && r.a_vox == g.b_vox && r.b_vox == g.a_vox && r.fp_vox == g.fn_vox && r.fn_vox == g.fp_vox && same(r.ab, g.ba) && same(r.ba, g.ab);
  // the writer
  const std::string text = compare::to_json(g, c.w, c.h, c.d, c.um, "ref \"dir\"/mask.mhd");
  const std::string row = compare::csv_fields(g, c.w, c.h, c.d, c.um, "ref,dir");
  ok = ok && text.size() > 2 && text.back() == '\n' && text.find("\"assd_mm\":") != std::string::npos && !row.empty();
  ok = ok && (g.ab.found != 0) == (text.find("\"hausdorff_mm\":null") == std::string::npos);
  std::printf("%-16s %4d x %3d x %3d  a %6llu b %6llu tp %6llu  S %5llu %5llu  max %20llu p95 %10u  %s\n", c.name, c.w, c.h, c.d,
              (unsigned long long)g.a_vox, (unsigned long long)g.b_vox, (unsigned long long)g.tp_vox, (unsigned long long)g.surface_a,
              (unsigned long long)g.surface_b, (unsigned long long)g.ab.max_um2, g.ab.p95_um, ok ? "ok" : "MISMATCH");
  return ok;
}

std::vector<uint8_t> box(int w, int h, int d, int x0, int x1, int y0, int y1, int z0, int z1) {
  std::vector<uint8_t> m((size_t)w * h * d, 0);
  for (int z = z0; z <= z1; ++z)
    for (int y = y0; y <= y1; ++y)
      for (int x = x0; x <= x1; ++x) m[((size_t)z * h + y) * w + x] = 1;
  return m;
}

bool worked_examples() {
  bool ok = true;
  {
    const uint32_t um[3] = {1000, 1000, 2500};
    const std::vector<uint8_t> a = box(16, 8, 5, 0, 9, 0, 3, 0, 2);
    std::vector<uint8_t> b = box(16, 8, 5, 2, 13, 1, 6, 1, 4);
    b[((size_t)4 * 8 + 6) * 16 + 15] = 1;
    const VolumeCompare g = golden::compare_volumes(a, b, 16, 8, 5, um);
    ok = ok && g.a_vox == 120 && g.b_vox == 289 && g.tp_vox == 48 && g.fp_vox == 72 && g.fn_vox == 241 && g.surface_a == 104 &&
         g.surface_b == 209 && g.ab.max_um2 == 11250000ull && g.ab.sum_um == 164741ull && g.ab.p95_um == 2692u &&
         g.ba.max_um2 == 70000000ull && g.ba.sum_um == 716543ull && g.ba.p95_um == 5916u;
  }
  {
    const uint32_t um[3] = {1000, 1000, 1000};
    const VolumeCompare g = golden::compare_volumes(box(11, 11, 11, 4, 6, 4, 6, 4, 6), box(11, 11, 11, 1, 9, 1, 9, 1, 9), 11, 11, 11, um);
    ok = ok && g.tp_vox == 27 && g.ab.n == 26 && g.ab.sum_um == 78000ull && g.ab.max_um2 == 9000000ull && g.ab.p95_um == 3000u &&
         g.ba.n == 386 && g.ba.max_um2 == 27000000ull && g.ba.sum_um == 1418760ull && g.ba.p95_um == 4690u;
  }
  {
    const uint32_t um[3] = {4000000, 1000, 1000};
    const VolumeCompare g = golden::compare_volumes(box(8, 1, 1, 0, 0, 0, 0, 0, 0), box(8, 1, 1, 7, 7, 0, 0, 0, 0), 8, 1, 1, um);
    ok = ok && g.ab.n == 1 && g.ba.n == 1 && g.ab.max_um2 == 784000000000000ull && g.ba.max_um2 == 784000000000000ull &&
         g.ab.p95_um == 28000000u && g.ba.sum_um == 28000000ull;
  }
  ok = ok && vcmp::isqrt_um(11250000) == 3354u && vcmp::isqrt_um(70000000) == 8366u && vcmp::isqrt_um((1ll << 62) - 1) == 0x7FFFFFFFu;
  for (uint64_t r : {0ull, 1ull, 94906265ull, 94906266ull, 94906267ull, 2000000011ull, 2147483647ull})
    for (int64_t dv = -1; dv <= 1; ++dv) {
      const int64_t v = (int64_t)(r * r) + dv;
      if (v < 0) continue;
      const uint64_t q = vcmp::isqrt_um(v);
      ok = ok && q * q <= (uint64_t)v && (q + 1) * (q + 1) > (uint64_t)v;
    }
  std::printf("worked examples and isqrt  %s\n", ok ? "ok" : "MISMATCH");
  return ok;
}

}  // namespace

int main() {
  const Case cases[] = {
      {"1x1x1", 1, 1, 1, {1000, 1000, 1000}, 1000, 1000},    {"1x1x1_a_empty", 1, 1, 1, {1000, 1000, 1000}, 0, 1000},
      {"width_1", 1, 7, 3, {1000, 900, 800}, 500, 500},       {"width_63", 63, 4, 3, {1000, 1000, 1000}, 600, 700},
      {"width_64", 64, 4, 3, {500, 500, 5000}, 600, 700},     {"width_65", 65, 4, 3, {500, 500, 5000}, 600, 700},
      {"width_130", 130, 5, 4, {391, 703, 6500}, 700, 300},   {"one_plane", 70, 9, 1, {391, 703, 6500}, 400, 400},
      {"one_row", 70, 1, 5, {391, 703, 6500}, 400, 400},      {"both_empty", 70, 5, 4, {1000, 1000, 1000}, 0, 0},
      {"b_empty", 70, 5, 4, {1000, 1000, 1000}, 300, 0},      {"both_full", 70, 5, 4, {1000, 1000, 1000}, 1000, 1000},
      {"corners", 130, 20, 6, {391, 703, 6500}, -1, -1},      {"sparse", 130, 20, 6, {1000, 1000, 1000}, 2, 3},
      {"noise_50", 67, 11, 5, {500, 750, 5000}, 500, 500},    {"keys_above_2_24", 8, 2, 2, {4000000u, 1000, 1000}, -1, -1},
      {"near_the_bound", 9, 5, 3, {150000000u, 200000000u, 400000000u}, -1, -1},
      {"near_bound_noise", 9, 5, 3, {150000000u, 200000000u, 400000000u}, 300, 300},
  };
  bool ok = worked_examples();
  for (const Case& c : cases) ok = run(c) && ok;
  std::printf("%s\n", ok ? "volume_compare_sanitize: all cases agree" : "volume_compare_sanitize: MISMATCH");
  return ok ? 0 : 1;
}
