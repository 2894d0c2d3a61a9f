// Stand-alone host check of the lesion-wise comparison code (nm03/volume_compare_lesions_core.h,
// src/golden/volume_compare_lesions.cpp) for sanitizer builds: the host run of K18's functions (K8's run union-find
// on both masks, the selection by lesion key, the stretch walk of the join across word edges, the partner-cell
// transitions, the rank lookup, the best partner with its tie rule) against the golden model (flood fills, plain
// loops, a sort), with every storage bit past the width set, at both connectivities and N = 1, 2 and 64, compare(A, B)
// against compare(B, A), Σ table against the overlap count, the two worked examples of
// nm03/volume_compare_lesions.h, the unpacking of the kernels' record and the writers of the lesion keys of
// compare.json, the lesion columns of comparisons.csv and compare_lesions.csv, on shapes that reach every edge of the
// word logic (widths 1, 63, 64, 65 and 130, one plane, one row, empty and full masks, more than 64 components). It
// needs no GPU and no Python. Build it with the host sources it calls and run it:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/volume_compare_lesions_sanitize.cpp src/golden/volume_compare_lesions.cpp src/golden/volume_compare.cpp \
//       src/golden/volume_distance.cpp -o volume_compare_lesions_sanitize && ./volume_compare_lesions_sanitize
//
// It prints one line per case and exits 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "nm03/volume_compare.h"
#include "nm03/volume_compare_lesions.h"
#include "nm03/volume_compare_lesions_core.h"

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
  int a_per_mille, b_per_mille;  // voxels set per thousand; 0 = empty, 1000 = full
};

std::vector<uint8_t> make_mask(const Case& c, int per_mille) {
  std::vector<uint8_t> m((size_t)c.w * c.h * c.d, 0);
  for (size_t i = 0; i < m.size(); ++i) m[i] = (int)(rnd() % 1000u) < per_mille;
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

bool same(const VolumeCompareLesion& p, const VolumeCompareLesion& q) {
  return p.voxels == q.voxels && p.overlap_vox == q.overlap_vox && p.overlap_other_vox == q.overlap_other_vox &&
         p.best_overlap_vox == q.best_overlap_vox && p.first[0] == q.first[0] && p.first[1] == q.first[1] && p.first[2] == q.first[2] &&
         p.partners_reported == q.partners_reported && p.multi == q.multi && p.best == q.best;
}
bool same(const std::vector<VolumeCompareLesion>& p, const std::vector<VolumeCompareLesion>& q) {
  if (p.size() != q.size()) return false;
  for (size_t i = 0; i < p.size(); ++i)
    if (!same(p[i], q[i])) return false;
  return true;
}
bool same(const VolumeCompareLesions& p, const VolumeCompareLesions& q) {
  const VolumeCompareLesionsHead &a = p.head, &b = q.head;
  return a.connectivity == b.connectivity && a.max_lesions == b.max_lesions && a.lesions_a == b.lesions_a && a.hit_a == b.hit_a &&
         a.multi_a == b.multi_a && a.lesions_b == b.lesions_b && a.hit_b == b.hit_b && a.multi_b == b.multi_b &&
         a.reported_a == b.reported_a && a.reported_b == b.reported_b && same(p.a, q.a) && same(p.b, q.b) && p.table == q.table;
}

// compare(B, A) from compare(A, B): the sides exchanged, the table transposed.
VolumeCompareLesions swapped(const VolumeCompareLesions& l) {
  VolumeCompareLesions s = l;
  s.head.lesions_a = l.head.lesions_b, s.head.hit_a = l.head.hit_b, s.head.multi_a = l.head.multi_b;
  s.head.lesions_b = l.head.lesions_a, s.head.hit_b = l.head.hit_a, s.head.multi_b = l.head.multi_a;
  s.head.reported_a = l.head.reported_b, s.head.reported_b = l.head.reported_a;
  s.a = l.b, s.b = l.a;
  const size_t n1 = (size_t)l.head.max_lesions + 1;
  for (size_t i = 0; i < n1; ++i)
    for (size_t j = 0; j < n1; ++j) s.table[i * n1 + j] = l.table[j * n1 + i];
  return s;
}

// The kernels' record in memory from the host form, and back through measure::unpack_compare_lesions.
bool round_trip(const VolumeCompareLesions& l) {
  const int n = (int)l.head.max_lesions;
  std::vector<uint8_t> rec(volume_compare_lesions_record_bytes(n), 0);
  uint8_t* p = rec.data();
  std::memcpy(p, &l.head, sizeof l.head);
  p += sizeof l.head;
  if (!l.a.empty()) std::memcpy(p, l.a.data(), l.a.size() * sizeof(VolumeCompareLesion));
  p += (size_t)n * sizeof(VolumeCompareLesion);
  if (!l.b.empty()) std::memcpy(p, l.b.data(), l.b.size() * sizeof(VolumeCompareLesion));
  p += (size_t)n * sizeof(VolumeCompareLesion);
  std::memcpy(p, l.table.data(), l.table.size() * sizeof(uint64_t));
  return same(measure::unpack_compare_lesions(rec.data(), n), l);
}

bool check(const char* name, const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int w, int h, int d) {
  const int wpr = (w + 63) / 64;
  const std::vector<uint64_t> wa = pack_with_junk(a, w, h, d), wb = pack_with_junk(b, w, h, d);
  uint64_t tp = 0;
  for (size_t i = 0; i < a.size(); ++i) tp += a[i] && b[i];
  const uint32_t um[3] = {1000, 1000, 1000};
  bool ok = true;
  VolumeCompareLesions last;
  for (int conn : {6, 26})
    for (int n : {1, 2, 64}) {
      const VolumeCompareLesions g = golden::compare_volume_lesions(a, b, w, h, d, n, conn);
      const VolumeCompareLesions e = measure::volume_compare_lesions_words(wa.data(), wb.data(), w, h, d, wpr, n, conn);
      const VolumeCompareLesions r = measure::volume_compare_lesions_words(wb.data(), wa.data(), w, h, d, wpr, n, conn);
      ok = ok && same(g, e) && same(r, swapped(g)) && round_trip(g);
      uint64_t sum = 0;
      for (uint64_t v : g.table) sum += v;
      ok = ok && sum == tp && g.table.size() == (size_t)(n + 1) * (n + 1);
      // the writers
      const VolumeCompare c = golden::compare_volumes(a, b, w, h, d, um);
      const std::string text = compare::to_json(c, w, h, d, um, "ref", &g), old = compare::to_json(c, w, h, d, um, "ref");
      const size_t cut = text.find(",\"lesions_connectivity\"");
      ok = ok && cut != std::string::npos && text.substr(0, cut) + "}\n" == old && text.find("\"b_lesions\":[") != std::string::npos;
      const std::string row = compare::csv_fields(c, w, h, d, um, "ref", &g), old_row = compare::csv_fields(c, w, h, d, um, "ref");
      ok = ok && row.compare(0, old_row.size(), old_row) == 0 && row.size() > old_row.size();
      const std::string rows = compare::lesions_table_rows("P", g);
      size_t lines = 0;
      for (char ch : rows) lines += ch == '\n';
      ok = ok && lines == g.a.size() + g.b.size();
      last = g;
    }
  std::printf("%-16s %4d x %3d x %3d  tp %6llu  lesions %4u %4u  hit %4u %4u  multi %3u %3u  %s\n", name, w, h, d, (unsigned long long)tp,
              last.head.lesions_a, last.head.lesions_b, last.head.hit_a, last.head.hit_b, last.head.multi_a, last.head.multi_b,
              ok ? "ok" : "MISMATCH");
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
    const std::vector<uint8_t> a = box(16, 8, 5, 0, 9, 0, 3, 0, 2);
    std::vector<uint8_t> b = box(16, 8, 5, 2, 13, 1, 6, 1, 4);
    b[((size_t)4 * 8 + 6) * 16 + 15] = 1;
    const VolumeCompareLesions g = golden::compare_volume_lesions(a, b, 16, 8, 5, 2, 26);
    ok = ok && g.head.lesions_a == 1 && g.head.hit_a == 1 && g.head.multi_a == 0 && g.head.lesions_b == 2 && g.head.hit_b == 1 &&
         g.head.multi_b == 0 && g.cell(0, 0) == 48;
    uint64_t sum = 0;
    for (uint64_t v : g.table) sum += v;
    ok = ok && sum == 48;
    const compare::LesionsDerived v = compare::derive_lesions(g);
    ok = ok && v.sensitivity == 0.5 && v.precision == 1.0 && v.f1 == 2.0 / 3.0;
  }
  {
    std::vector<uint8_t> a(12, 0), b(12, 0);
    for (int x : {0, 1, 2, 4, 5, 6, 9}) a[(size_t)x] = 1;
    for (int x : {2, 3, 4, 11}) b[(size_t)x] = 1;
    const VolumeCompareLesions g = golden::compare_volume_lesions(a, b, 12, 1, 1, 2, 6);
    ok = ok && g.head.lesions_a == 3 && g.head.hit_a == 2 && g.head.multi_a == 0 && g.head.lesions_b == 2 && g.head.hit_b == 1 &&
         g.head.multi_b == 1;
    const VolumeCompareLesion& b0 = g.b[0];
    ok = ok && b0.voxels == 3 && b0.first[0] == 2 && b0.overlap_vox == 2 && b0.partners_reported == 2 && b0.overlap_other_vox == 0 &&
         b0.multi == 1 && b0.best == 0 && b0.best_overlap_vox == 1 && g.b[1].overlap_vox == 0 && g.b[1].best == -1;
    const VolumeCompareLesions g1 = golden::compare_volume_lesions(a, b, 12, 1, 1, 1, 6);
    ok = ok && g1.b[0].partners_reported == 1 && g1.b[0].overlap_other_vox == 1 && g1.b[0].multi == 1;
    const compare::LesionsDerived v = compare::derive_lesions(g);
    ok = ok && v.sensitivity == 0.5 && v.precision == 2.0 / 3.0 && v.f1 == 0.5;
  }
  // the partner cell: none → one → the same one → several → several
  uint32_t cell = 0;
  cell = vclcore::partner_next(cell, 7), ok = ok && cell == 8u;
  cell = vclcore::partner_next(cell, 7), ok = ok && cell == 8u;
  cell = vclcore::partner_next(cell, 0), ok = ok && cell == vclcore::kSeveral;
  cell = vclcore::partner_next(cell, 7), ok = ok && cell == vclcore::kSeveral;
  // the best partner: a tie goes to the smaller index, zeros are no partners
  const uint64_t line[5] = {0, 4, 9, 9, 1};
  uint32_t partners = 0;
  uint64_t best = 0;
  ok = ok && vclcore::best_partner(line, 1, 5, partners, best) == 2 && partners == 4 && best == 9;
  ok = ok && vclcore::best_partner(line, 1, 1, partners, best) == -1 && partners == 0 && best == 0;
  ok = ok && vclcore::best_partner(line, 2, 3, partners, best) == 1 && partners == 2 && best == 9;  // cells 0, 9, 1
  std::printf("worked examples, partner cell, best partner  %s\n", ok ? "ok" : "MISMATCH");
  return ok;
}

}  // namespace

int main() {
  const Case cases[] = {
      {"1x1x1", 1, 1, 1, 1000, 1000},        {"1x1x1_a_empty", 1, 1, 1, 0, 1000},  {"width_1", 1, 7, 3, 500, 500},
      {"width_63", 63, 4, 3, 600, 700},      {"width_64", 64, 4, 3, 600, 700},     {"width_65", 65, 4, 3, 600, 700},
      {"width_130", 130, 5, 4, 700, 300},    {"one_plane", 70, 9, 1, 400, 400},    {"one_row", 70, 1, 5, 400, 400},
      {"both_empty", 70, 5, 4, 0, 0},        {"b_empty", 70, 5, 4, 300, 0},        {"both_full", 70, 5, 4, 1000, 1000},
      {"sparse", 130, 20, 6, 20, 30},        {"many_lesions", 130, 20, 6, 150, 120}, {"noise_50", 67, 11, 5, 500, 500},
      {"long_runs", 200, 6, 3, 950, 930},
  };
  bool ok = worked_examples();
  for (const Case& c : cases) {
    const std::vector<uint8_t> a = make_mask(c, c.a_per_mille), b = make_mask(c, c.b_per_mille);
    ok = check(c.name, a, b, c.w, c.h, c.d) && ok;
  }
  std::printf("%s\n", ok ? "volume_compare_lesions_sanitize: all cases agree" : "volume_compare_lesions_sanitize: MISMATCH");
  return ok ? 0 : 1;
}
