// Lesion-wise comparison of two volume masks (nm03/volume_compare_lesions.h): the golden model (flood fills, plain
// loops over voxels, a sort), the host run of the K18 kernels' functions and the writers of the lesion keys of
// compare.json, the lesion columns of comparisons.csv and compare_lesions.csv.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "nm03/volume_compare_lesions.h"
#include "nm03/volume_compare_lesions_core.h"
#include "nm03/volume_measure_core.h"

namespace nm03 {

namespace {

void check_args(const char* who, int w, int h, int d, int max_lesions, int connectivity) {
  if (w < 1 || h < 1 || d < 1) throw std::invalid_argument(std::string(who) + ": empty volume");
  if (max_lesions < 1 || max_lesions > kMaxVolumeLesions)
    throw std::invalid_argument(std::string(who) + ": max_lesions must be 1.." + std::to_string(kMaxVolumeLesions));
  if (connectivity != 6 && connectivity != 26) throw std::invalid_argument(std::string(who) + ": connectivity must be 6 or 26");
  if (volume_measure_scratch_words(w, h, d) == 0)
    throw std::invalid_argument(std::string(who) + ": (w + 1) * h * d + 1 must stay below 2^32");
}

std::string num(double v, bool ok) {
  if (!ok) return "null";
  char b[64];
  std::snprintf(b, sizeof b, "%.9g", v);
  return b;
}

// coverage and best_dice of one record; `other` = the other side's reported records.
void lesion_derived(const VolumeCompareLesion& r, const std::vector<VolumeCompareLesion>& other, std::string* coverage, std::string* best_dice) {
  *coverage = num(r.voxels ? (double)r.overlap_vox / (double)r.voxels : 0.0, r.voxels != 0);
  const bool ok = r.best >= 0 && (size_t)r.best < other.size() && r.voxels + other[(size_t)r.best].voxels != 0;
  *best_dice = num(ok ? 2.0 * (double)r.best_overlap_vox / ((double)r.voxels + (double)other[(size_t)r.best].voxels) : 0.0, ok);
}

// The host's plain accesses in place of the kernels' relaxed atomics.
struct HostStore {
  uint32_t* p;
  uint32_t ld(uint32_t i) const { return p[i]; }
  void st(uint32_t i, uint32_t v) const { p[i] = v; }
  uint32_t fetch_min(uint32_t i, uint32_t v) const {
    const uint32_t o = p[i];
    if (v < o) p[i] = v;
    return o;
  }
  void add(uint32_t i, uint32_t v) const { p[i] += v; }
  uint32_t cas(uint32_t i, uint32_t expected, uint32_t desired) const {
    const uint32_t o = p[i];
    if (o == expected) p[i] = desired;
    return o;
  }
};

}  // namespace

namespace measure {

VolumeCompareLesions unpack_compare_lesions(const void* record, int max_lesions) {
  if (!record || max_lesions < 1 || max_lesions > kMaxVolumeLesions) throw std::invalid_argument("unpack_compare_lesions: bad arguments");
  const uint8_t* p = static_cast<const uint8_t*>(record);
  VolumeCompareLesions l;
  std::memcpy(&l.head, p, sizeof l.head);
  p += sizeof l.head;
  const size_t na = std::min<size_t>(l.head.reported_a, (size_t)max_lesions), nb = std::min<size_t>(l.head.reported_b, (size_t)max_lesions);
  l.a.resize(na), l.b.resize(nb);
  if (na) std::memcpy(l.a.data(), p, na * sizeof(VolumeCompareLesion));
  p += (size_t)max_lesions * sizeof(VolumeCompareLesion);
  if (nb) std::memcpy(l.b.data(), p, nb * sizeof(VolumeCompareLesion));
  p += (size_t)max_lesions * sizeof(VolumeCompareLesion);
  l.table.resize((size_t)(max_lesions + 1) * (size_t)(max_lesions + 1));
  std::memcpy(l.table.data(), p, l.table.size() * sizeof(uint64_t));
  return l;
}

VolumeCompareLesions volume_compare_lesions_words(const uint64_t* a, const uint64_t* b, int w, int h, int d, int wpr, int max_lesions,
                                                  int connectivity) {
  check_args("volume_compare_lesions_words", w, h, d, max_lesions, connectivity);
  if (wpr != (w + 63) / 64) throw std::invalid_argument("volume_compare_lesions_words: wpr must be ceil(w / 64)");
  if (!a || !b) throw std::invalid_argument("volume_compare_lesions_words: null buffer");
  using namespace vmcore;
  const size_t slots = volume_measure_scratch_words(w, h, d);
  const int N = max_lesions, stride = N + 1;
  const BitVolume V[2] = {BitVolume{a, w, h, d, wpr, false}, BitVolume{b, w, h, d, wpr, false}};
  std::vector<uint32_t> labels[2] = {std::vector<uint32_t>(slots, 0xDEADBEEFu), std::vector<uint32_t>(slots, 0xDEADBEEFu)};
  std::vector<uint32_t> sides[2] = {std::vector<uint32_t>(slots, 0xDEADBEEFu), std::vector<uint32_t>(slots, 0xDEADBEEFu)};
  auto each_word = [&](auto&& fn) {  // a thread of a launch per word
    for (int z = 0; z < d; ++z)
      for (int y = 0; y < h; ++y)
        for (int k = 0; k < wpr; ++k) fn(z, y, k);
  };
  // The chosen roots per side: in rank order, and ascending by slot with their ranks (the select launch).
  std::vector<uint32_t> sel_slot[2], sel_vox[2], srt_slot[2], srt_rank[2];
  for (int s = 0; s < 2; ++s) {
    HostStore par{labels[s].data()}, side{sides[s].data()};
    each_word([&](int z, int y, int k) { init_runs(V[s], z, y, k, par); });
    each_word([&](int z, int y, int k) { unite_word(V[s], par, z, y, k, connectivity == 26); });
    each_word([&](int z, int y, int k) {
      compress_runs(V[s], par, z, y, k);
      vclcore::init_side(V[s], par, side, z, y, k);
    });
    each_word([&](int z, int y, int k) { stretch_areas(V[s], par, z, y, k, [&](uint32_t r, uint32_t n) { par.add(r + 1u, n); }); });
    // Candidates and selection: every root's key, the N largest (the kernels reach the same set through the
    // workgroups' own best N).
    std::vector<uint64_t> keys;
    each_word([&](int z, int y, int k) {
      uint64_t roots = root_bits(V[s], par, z, y, k);
      while (roots) {
        int bit = 0;
        keys.push_back(best_root_key(V[s], par, z, y, k, roots, bit));
        roots &= ~(1ull << bit);
      }
    });
    std::sort(keys.begin(), keys.end(), [](uint64_t x, uint64_t y) { return x > y; });
    if (keys.size() > (size_t)N) keys.resize((size_t)N);
    for (uint64_t key : keys) sel_slot[s].push_back(lesion_key_slot(key)), sel_vox[s].push_back(lesion_key_area(key));
    srt_slot[s] = sel_slot[s];
    std::sort(srt_slot[s].begin(), srt_slot[s].end());
    for (uint32_t sl : srt_slot[s])
      srt_rank[s].push_back((uint32_t)(std::find(sel_slot[s].begin(), sel_slot[s].end(), sl) - sel_slot[s].begin()));
  }
  HostStore para{labels[0].data()}, parb{labels[1].data()}, sa{sides[0].data()}, sb{sides[1].data()};
  VolumeCompareLesions l;
  l.table.assign((size_t)stride * stride, 0ull);
  const int count_a = (int)sel_slot[0].size(), count_b = (int)sel_slot[1].size();
  each_word([&](int z, int y, int k) {  // the join
    vclcore::join_stretches(V[0], V[1], para, parb, z, y, k, [&](uint32_t ra, uint32_t rb, uint32_t n) {
      sa.add(ra, n);
      sb.add(rb, n);
      vclcore::partner_update(sa, ra, rb);
      vclcore::partner_update(sb, rb, ra);
      const int ia = vclcore::lesion_rank(srt_slot[0].data(), srt_rank[0].data(), count_a, ra, N);
      const int ib = vclcore::lesion_rank(srt_slot[1].data(), srt_rank[1].data(), count_b, rb, N);
      l.table[(size_t)ia * stride + ib] += n;
    });
  });
  l.head.connectivity = (uint32_t)connectivity, l.head.max_lesions = (uint32_t)N;
  each_word([&](int z, int y, int k) {  // the count
    vclcore::count_side(V[0], para, sa, z, y, k, l.head.lesions_a, l.head.hit_a, l.head.multi_a);
    vclcore::count_side(V[1], parb, sb, z, y, k, l.head.lesions_b, l.head.hit_b, l.head.multi_b);
  });
  l.head.reported_a = (uint32_t)count_a, l.head.reported_b = (uint32_t)count_b;
  for (int j = 0; j < count_a; ++j) {
    const uint32_t slot = sel_slot[0][(size_t)j];
    l.a.push_back(vclcore::lesion_record(V[0], slot, sel_vox[0][(size_t)j], sides[0][slot], sides[0][slot + 1u],
                                         l.table.data() + (size_t)j * stride, 1, count_b, N));
  }
  for (int j = 0; j < count_b; ++j) {
    const uint32_t slot = sel_slot[1][(size_t)j];
    l.b.push_back(vclcore::lesion_record(V[1], slot, sel_vox[1][(size_t)j], sides[1][slot], sides[1][slot + 1u], l.table.data() + j, stride,
                                         count_a, N));
  }
  return l;
}

}  // namespace measure

namespace compare {

LesionsDerived derive_lesions(const VolumeCompareLesions& l) {
  LesionsDerived v{};
  const VolumeCompareLesionsHead& hd = l.head;
  v.sensitivity_ok = hd.lesions_b != 0;
  v.precision_ok = hd.lesions_a != 0;
  const double den = 2.0 * (double)hd.hit_b + ((double)hd.lesions_a - (double)hd.hit_a) + ((double)hd.lesions_b - (double)hd.hit_b);
  v.f1_ok = den != 0.0;
  if (v.sensitivity_ok) v.sensitivity = (double)hd.hit_b / (double)hd.lesions_b;
  if (v.precision_ok) v.precision = (double)hd.hit_a / (double)hd.lesions_a;
  if (v.f1_ok) v.f1 = 2.0 * (double)hd.hit_b / den;
  return v;
}

namespace {

std::string lesion_object(const VolumeCompareLesion& r, const std::vector<VolumeCompareLesion>& other) {
  std::string cov, dice;
  lesion_derived(r, other, &cov, &dice);
  return "{\"voxels\":" + std::to_string(r.voxels) + ",\"first\":[" + std::to_string(r.first[0]) + "," + std::to_string(r.first[1]) + "," +
         std::to_string(r.first[2]) + "],\"overlap_vox\":" + std::to_string(r.overlap_vox) +
         ",\"partners_reported\":" + std::to_string(r.partners_reported) + ",\"overlap_other_vox\":" + std::to_string(r.overlap_other_vox) +
         ",\"multi\":" + std::to_string(r.multi) + ",\"best\":" + std::to_string(r.best) +
         ",\"best_overlap_vox\":" + std::to_string(r.best_overlap_vox) + ",\"coverage\":" + cov + ",\"best_dice\":" + dice + "}";
}

std::string lesion_array(const std::vector<VolumeCompareLesion>& mine, const std::vector<VolumeCompareLesion>& other) {
  std::string s = "[";
  for (size_t i = 0; i < mine.size(); ++i) {
    if (i) s += ',';
    s += lesion_object(mine[i], other);
  }
  return s + "]";
}

}  // namespace

std::string lesions_json_keys(const VolumeCompareLesions& l) {
  const VolumeCompareLesionsHead& hd = l.head;
  const LesionsDerived v = derive_lesions(l);
  std::string s;
  auto u = [&](const char* k, uint64_t x) { s += std::string(",\"") + k + "\":" + std::to_string(x); };
  u("lesions_connectivity", hd.connectivity), u("lesions_max", hd.max_lesions);
  u("lesions_a", hd.lesions_a), u("hit_a", hd.hit_a), u("multi_a", hd.multi_a);
  u("lesions_b", hd.lesions_b), u("hit_b", hd.hit_b), u("multi_b", hd.multi_b);
  s += ",\"lesion_sensitivity\":" + num(v.sensitivity, v.sensitivity_ok);
  s += ",\"lesion_precision\":" + num(v.precision, v.precision_ok);
  s += ",\"lesion_f1\":" + num(v.f1, v.f1_ok);
  s += ",\"a_lesions\":" + lesion_array(l.a, l.b);
  s += ",\"b_lesions\":" + lesion_array(l.b, l.a);
  return s;
}

std::string lesions_csv_header_fields() {
  return ",lesions_a,hit_a,multi_a,lesions_b,hit_b,multi_b,lesion_sensitivity,lesion_precision,lesion_f1";
}

std::string lesions_csv_fields(const VolumeCompareLesions& l) {
  const VolumeCompareLesionsHead& hd = l.head;
  const LesionsDerived v = derive_lesions(l);
  auto real = [](double x, bool ok) { return ok ? num(x, true) : std::string(); };
  return "," + std::to_string(hd.lesions_a) + "," + std::to_string(hd.hit_a) + "," + std::to_string(hd.multi_a) + "," +
         std::to_string(hd.lesions_b) + "," + std::to_string(hd.hit_b) + "," + std::to_string(hd.multi_b) + "," +
         real(v.sensitivity, v.sensitivity_ok) + "," + real(v.precision, v.precision_ok) + "," + real(v.f1, v.f1_ok);
}

std::string lesions_table_header() {
  return "patient,side,lesion,voxels,first_x,first_y,first_z,overlap_vox,partners_reported,overlap_other_vox,multi,best,best_overlap_vox";
}

std::string lesions_table_rows(const std::string& patient, const VolumeCompareLesions& l) {
  std::string s;
  const std::vector<VolumeCompareLesion>* sides[2] = {&l.a, &l.b};
  for (int sd = 0; sd < 2; ++sd)
    for (size_t i = 0; i < sides[sd]->size(); ++i) {
      const VolumeCompareLesion& r = (*sides[sd])[i];
      s += patient + "," + (sd ? "b" : "a") + "," + std::to_string(i) + "," + std::to_string(r.voxels) + "," + std::to_string(r.first[0]) +
           "," + std::to_string(r.first[1]) + "," + std::to_string(r.first[2]) + "," + std::to_string(r.overlap_vox) + "," +
           std::to_string(r.partners_reported) + "," + std::to_string(r.overlap_other_vox) + "," + std::to_string(r.multi) + "," +
           std::to_string(r.best) + "," + std::to_string(r.best_overlap_vox) + "\n";
    }
  return s;
}

}  // namespace compare

namespace golden {

namespace {

struct Labelled {
  std::vector<int32_t> label;    // per voxel, −1 = background; labels in the order of the first voxels
  std::vector<uint64_t> voxels;  // per label
  std::vector<uint64_t> first;   // per label: raster index of the first voxel
};

Labelled flood_fill(const std::vector<uint8_t>& m, int w, int h, int d, int connectivity) {
  Labelled L;
  const size_t plane = (size_t)w * h;
  L.label.assign(m.size(), -1);
  std::vector<size_t> stack;
  for (size_t p0 = 0; p0 < m.size(); ++p0) {
    if (!m[p0] || L.label[p0] >= 0) continue;
    const int32_t id = (int32_t)L.voxels.size();
    L.voxels.push_back(0), L.first.push_back((uint64_t)p0);
    L.label[p0] = id;
    stack.push_back(p0);
    while (!stack.empty()) {
      const size_t p = stack.back();
      stack.pop_back();
      ++L.voxels[(size_t)id];
      const int x = (int)(p % (size_t)w), y = (int)(p / (size_t)w % (size_t)h), z = (int)(p / plane);
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int steps = (dx != 0) + (dy != 0) + (dz != 0);
            if (steps == 0 || (connectivity == 6 && steps != 1)) continue;
            const int xx = x + dx, yy = y + dy, zz = z + dz;
            if (xx < 0 || xx >= w || yy < 0 || yy >= h || zz < 0 || zz >= d) continue;
            const size_t q = (size_t)zz * plane + (size_t)yy * w + (size_t)xx;
            if (!m[q] || L.label[q] >= 0) continue;
            L.label[q] = id;
            stack.push_back(q);
          }
    }
  }
  return L;
}

// The labels in reporting order: more voxels first, then the earlier first voxel.
std::vector<int32_t> reporting_order(const Labelled& L) {
  std::vector<int32_t> order(L.voxels.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
  std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
    if (L.voxels[(size_t)x] != L.voxels[(size_t)y]) return L.voxels[(size_t)x] > L.voxels[(size_t)y];
    return L.first[(size_t)x] < L.first[(size_t)y];
  });
  return order;
}

}  // namespace

VolumeCompareLesions compare_volume_lesions(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int w, int h, int d, int max_lesions,
                                            int connectivity) {
  check_args("golden::compare_volume_lesions", w, h, d, max_lesions, connectivity);
  const size_t n = (size_t)w * h * d;
  if (a.size() != n || b.size() != n) throw std::invalid_argument("golden::compare_volume_lesions: both masks must hold w * h * d voxels");
  const Labelled LA = flood_fill(a, w, h, d, connectivity), LB = flood_fill(b, w, h, d, connectivity);
  const size_t N = (size_t)max_lesions, stride = N + 1;
  // Pair counts over the voxels of A ∩ B.
  std::map<std::pair<int32_t, int32_t>, uint64_t> pairs;
  for (size_t p = 0; p < n; ++p)
    if (LA.label[p] >= 0 && LB.label[p] >= 0) ++pairs[{LA.label[p], LB.label[p]}];
  std::vector<uint64_t> overlap_a(LA.voxels.size(), 0), overlap_b(LB.voxels.size(), 0);
  std::vector<uint32_t> partners_a(LA.voxels.size(), 0), partners_b(LB.voxels.size(), 0);
  for (const auto& kv : pairs) {
    overlap_a[(size_t)kv.first.first] += kv.second, overlap_b[(size_t)kv.first.second] += kv.second;
    ++partners_a[(size_t)kv.first.first], ++partners_b[(size_t)kv.first.second];
  }
  VolumeCompareLesions l;
  VolumeCompareLesionsHead& hd = l.head;
  hd.connectivity = (uint32_t)connectivity, hd.max_lesions = (uint32_t)max_lesions;
  hd.lesions_a = (uint32_t)LA.voxels.size(), hd.lesions_b = (uint32_t)LB.voxels.size();
  for (size_t i = 0; i < LA.voxels.size(); ++i) hd.hit_a += overlap_a[i] >= 1, hd.multi_a += partners_a[i] >= 2;
  for (size_t i = 0; i < LB.voxels.size(); ++i) hd.hit_b += overlap_b[i] >= 1, hd.multi_b += partners_b[i] >= 2;
  const std::vector<int32_t> order_a = reporting_order(LA), order_b = reporting_order(LB);
  const size_t na = std::min(N, order_a.size()), nb = std::min(N, order_b.size());
  hd.reported_a = (uint32_t)na, hd.reported_b = (uint32_t)nb;
  std::vector<size_t> rank_a(LA.voxels.size(), N), rank_b(LB.voxels.size(), N);  // N = unreported
  for (size_t i = 0; i < na; ++i) rank_a[(size_t)order_a[i]] = i;
  for (size_t i = 0; i < nb; ++i) rank_b[(size_t)order_b[i]] = i;
  l.table.assign(stride * stride, 0ull);
  for (const auto& kv : pairs) l.table[rank_a[(size_t)kv.first.first] * stride + rank_b[(size_t)kv.first.second]] += kv.second;
  auto record = [&](const Labelled& L, int32_t id, uint64_t overlap, uint32_t partners, bool is_a, size_t idx, size_t others) {
    VolumeCompareLesion r{};
    r.voxels = L.voxels[(size_t)id];
    const uint64_t p = L.first[(size_t)id];
    r.first[0] = (int32_t)(p % (uint64_t)w), r.first[1] = (int32_t)(p / (uint64_t)w % (uint64_t)h);
    r.first[2] = (int32_t)(p / ((uint64_t)w * (uint64_t)h));
    r.overlap_vox = overlap;
    r.multi = partners >= 2 ? 1 : 0;
    r.best = -1;
    auto cell = [&](size_t j) { return is_a ? l.table[idx * stride + j] : l.table[j * stride + idx]; };
    r.overlap_other_vox = cell(N);
    for (size_t j = 0; j < others; ++j) {
      if (cell(j) == 0) continue;
      ++r.partners_reported;
      if (cell(j) > r.best_overlap_vox) r.best_overlap_vox = cell(j), r.best = (int32_t)j;  // a tie keeps the smaller index
    }
    return r;
  };
  for (size_t i = 0; i < na; ++i) l.a.push_back(record(LA, order_a[i], overlap_a[(size_t)order_a[i]], partners_a[(size_t)order_a[i]], true, i, nb));
  for (size_t i = 0; i < nb; ++i) l.b.push_back(record(LB, order_b[i], overlap_b[(size_t)order_b[i]], partners_b[(size_t)order_b[i]], false, i, na));
  return l;
}

}  // namespace golden
}  // namespace nm03
