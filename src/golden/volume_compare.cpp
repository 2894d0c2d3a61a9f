// Overlap and surface distances between two volume masks (nm03/volume_compare.h): the golden model (plain loops, a
// sort), the host run of the K17 kernels' functions and the one writer of compare.json and comparisons.csv.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "nm03/intensity_core.h"
#include "nm03/volume_compare.h"
#include "nm03/volume_compare_core.h"
#include "nm03/volume_compare_lesions.h"
#include "nm03/volume_distance.h"
#include "nm03/volume_distance_core.h"

namespace nm03 {

namespace {

void check_args(const char* who, int w, int h, int d, const uint32_t um[3]) {
  if (w < 1 || h < 1 || d < 1) throw std::invalid_argument(std::string(who) + ": empty volume");
  if (w > 65535) throw std::invalid_argument(std::string(who) + ": a row holds at most 65535 voxels");
  if ((uint64_t)w * (uint64_t)h * (uint64_t)d >= (1ull << 32)) throw std::invalid_argument(std::string(who) + ": 2^32 voxels or more");
  for (int a = 0; a < 3; ++a)
    if (um[a] < 1u) throw std::invalid_argument(std::string(who) + ": a spacing must be at least 1 um");
  const std::string ext = measure::volume_distance_extent_error(w, h, d, um);
  if (!ext.empty()) throw std::invalid_argument(std::string(who) + ": " + ext);
}

VolumeCompareDirected not_found() {
  VolumeCompareDirected r{};
  r.worst[0] = r.worst[1] = r.worst[2] = -1;
  return r;
}

void set_worst(VolumeCompareDirected& r, uint64_t p, int w, int h) {
  r.worst[0] = (int32_t)(p % (uint64_t)w);
  r.worst[1] = (int32_t)(p / (uint64_t)w % (uint64_t)h);
  r.worst[2] = (int32_t)(p / ((uint64_t)w * (uint64_t)h));
}

// One direction of the host run: the kernels' sampling pass and radix select over S(from) and the map of S(to).
VolumeCompareDirected directed_words(const uint64_t* from, const std::vector<int64_t>& map, uint64_t n_from, uint64_t n_to, int w, int h,
                                     int d, int wpr) {
  if (n_from == 0 || n_to == 0) return not_found();
  VolumeCompareDirected r{};
  const size_t words = (size_t)wpr * h * d;
  auto each = [&](auto&& f) {  // f(raster position, D) for every set bit, in word order
    for (size_t i = 0; i < words; ++i) {
      const size_t row = i / (size_t)wpr;
      const size_t base = row * (size_t)w + ((i - row * (size_t)wpr) << 6);
      for (uint64_t m = from[i]; m; m &= m - 1) {
        const size_t p = base + (size_t)__builtin_ctzll(m);
        f((uint64_t)p, map[p]);
      }
    }
  };
  int64_t bv = 0;
  uint64_t bp = vdist::kNoCandidate;
  uint64_t sum = 0;
  uint32_t prefix = 0;
  uint64_t rank = icore::percentile_rank(vcmp::kPercentile, n_from);
  for (int pass = 0; pass < vcmp::kPasses; ++pass) {
    std::vector<uint32_t> hist(vcmp::digit_bins(pass), 0u);
    each([&](uint64_t p, int64_t D) {
      const uint32_t key = vcmp::isqrt_um(D);
      if (pass == 0) {
        sum += key;
        if (vdist::better(D, p, bv, bp)) bv = D, bp = p;
      }
      if (vcmp::in_prefix(key, prefix, pass)) ++hist[vcmp::digit(key, pass)];
    });
    const icore::BinRank l = icore::select_bin(hist.data(), (int)hist.size(), rank);
    prefix |= l.bin << vcmp::digit_shift(pass);
    rank = l.rank;
  }
  r.max_um2 = (uint64_t)bv;
  r.sum_um = sum;
  r.n = (uint32_t)n_from;
  r.p95_um = prefix;
  set_worst(r, bp, w, h);
  r.found = 1;
  return r;
}

std::string num(double v, bool ok) {
  if (!ok) return "null";
  char b[64];
  std::snprintf(b, sizeof b, "%.9g", v);
  return b;
}

std::string json_text(const std::string& s) {
  std::string o = "\"";
  for (unsigned char c : s) {
    if (c == '"' || c == '\\') o += '\\', o += (char)c;
    else if (c < 0x20) {
      char b[8];
      std::snprintf(b, sizeof b, "\\u%04x", c);
      o += b;
    } else o += (char)c;
  }
  return o + "\"";
}

std::string csv_text(const std::string& s) {
  if (s.find_first_of(",\"\n") == std::string::npos) return s;
  std::string o = "\"";
  for (char c : s) {
    if (c == '"') o += '"';
    o += c;
  }
  return o + "\"";
}

struct Field {
  const char* key;
  std::string json;  // as the sidecar writes it
  std::string csv;   // flattened; null → empty
  int columns;       // 1, or 3 for an array
};

std::vector<Field> fields(const VolumeCompare& c, int w, int h, int d, const uint32_t um[3], const std::string& reference) {
  std::vector<Field> f;
  auto u = [&](const char* k, uint64_t v) { f.push_back({k, std::to_string(v), std::to_string(v), 1}); };
  auto arr = [&](const char* k, long long x, long long y, long long z) {
    const std::string a = std::to_string(x), b = std::to_string(y), e = std::to_string(z);
    f.push_back({k, "[" + a + "," + b + "," + e + "]", a + "," + b + "," + e, 3});
  };
  auto real = [&](const char* k, double v, bool ok) { f.push_back({k, num(v, ok), ok ? num(v, true) : std::string(), 1}); };
  u("width", (uint64_t)w), u("height", (uint64_t)h), u("depth", (uint64_t)d);
  arr("compare_spacing_um", um[0], um[1], um[2]);
  f.push_back({"reference", json_text(reference), csv_text(reference), 1});
  u("a_vox", c.a_vox), u("b_vox", c.b_vox), u("tp_vox", c.tp_vox), u("fp_vox", c.fp_vox), u("fn_vox", c.fn_vox);
  u("surface_a", c.surface_a), u("surface_b", c.surface_b);
  u("n_ab", c.ab.n), u("max_um2_ab", c.ab.max_um2);
  arr("worst_ab", c.ab.worst[0], c.ab.worst[1], c.ab.worst[2]);
  u("sum_um_ab", c.ab.sum_um), u("p95_um_ab", c.ab.p95_um), u("found_ab", (uint64_t)c.ab.found);
  u("n_ba", c.ba.n), u("max_um2_ba", c.ba.max_um2);
  arr("worst_ba", c.ba.worst[0], c.ba.worst[1], c.ba.worst[2]);
  u("sum_um_ba", c.ba.sum_um), u("p95_um_ba", c.ba.p95_um), u("found_ba", (uint64_t)c.ba.found);
  const compare::Derived v = compare::derive(c, um);
  real("dice", v.dice, v.dice_ok), real("jaccard", v.jaccard, v.jaccard_ok), real("sensitivity", v.sensitivity, v.sensitivity_ok);
  real("precision", v.precision, v.precision_ok);
  real("volume_a_mm3", v.volume_a_mm3, true), real("volume_b_mm3", v.volume_b_mm3, true), real("volume_diff_mm3", v.volume_diff_mm3, true);
  real("hausdorff_mm", v.hausdorff_mm, v.distances_ok), real("hd95_mm", v.hd95_mm, v.distances_ok);
  real("msd_ab_mm", v.msd_ab_mm, v.distances_ok), real("msd_ba_mm", v.msd_ba_mm, v.distances_ok), real("assd_mm", v.assd_mm, v.distances_ok);
  return f;
}

}  // namespace

namespace measure {

VolumeCompare volume_compare_words(const uint64_t* a, const uint64_t* b, int w, int h, int d, int wpr, const uint32_t um[3],
                                   uint64_t* surface_a, uint64_t* surface_b) {
  check_args("volume_compare_words", w, h, d, um);
  if (wpr != (w + 63) / 64) throw std::invalid_argument("volume_compare_words: wpr must be ceil(w / 64)");
  if (!a || !b) throw std::invalid_argument("volume_compare_words: null buffer");
  const size_t words = (size_t)wpr * h * d, n = (size_t)w * h * d;
  std::vector<uint64_t> sa(words), sb(words);
  VolumeCompare c{};
  for (int z = 0; z < d; ++z)  // a thread of the surface kernel per word
    for (int y = 0; y < h; ++y)
      for (int k = 0; k < wpr; ++k) {
        const size_t i = ((size_t)z * h + y) * wpr + k;
        const uint64_t wa = vcmp::word_at(a, w, h, d, wpr, z, y, k), wb = vcmp::word_at(b, w, h, d, wpr, z, y, k);
        sa[i] = vcmp::surface_at(a, w, h, d, wpr, z, y, k);
        sb[i] = vcmp::surface_at(b, w, h, d, wpr, z, y, k);
        c.a_vox += (uint64_t)__builtin_popcountll(wa), c.b_vox += (uint64_t)__builtin_popcountll(wb);
        c.tp_vox += (uint64_t)__builtin_popcountll(wa & wb);
        c.surface_a += (uint64_t)__builtin_popcountll(sa[i]), c.surface_b += (uint64_t)__builtin_popcountll(sb[i]);
      }
  c.fp_vox = c.a_vox - c.tp_vox, c.fn_vox = c.b_vox - c.tp_vox;
  if (surface_a) std::copy(sa.begin(), sa.end(), surface_a);
  if (surface_b) std::copy(sb.begin(), sb.end(), surface_b);
  c.ab = c.ba = not_found();
  if (c.surface_a && c.surface_b) {
    std::vector<int64_t> map(n);
    volume_distance_words(sb.data(), w, h, d, wpr, um, false, -1, map.data());
    c.ab = directed_words(sa.data(), map, c.surface_a, c.surface_b, w, h, d, wpr);
    volume_distance_words(sa.data(), w, h, d, wpr, um, false, -1, map.data());
    c.ba = directed_words(sb.data(), map, c.surface_b, c.surface_a, w, h, d, wpr);
  }
  return c;
}

}  // namespace measure

namespace compare {

Derived derive(const VolumeCompare& c, const uint32_t um[3]) {
  Derived v{};
  const double a = (double)c.a_vox, b = (double)c.b_vox, tp = (double)c.tp_vox;
  v.dice_ok = c.a_vox + c.b_vox != 0;
  v.jaccard_ok = c.a_vox + c.b_vox - c.tp_vox != 0;
  v.sensitivity_ok = c.b_vox != 0;
  v.precision_ok = c.a_vox != 0;
  if (v.dice_ok) v.dice = 2.0 * tp / (a + b);
  if (v.jaccard_ok) v.jaccard = tp / (a + b - tp);
  if (v.sensitivity_ok) v.sensitivity = tp / b;
  if (v.precision_ok) v.precision = tp / a;
  const double voxel_mm3 = (double)um[0] * (double)um[1] * (double)um[2] / 1e9;
  v.volume_a_mm3 = a * voxel_mm3;
  v.volume_b_mm3 = b * voxel_mm3;
  v.volume_diff_mm3 = (a - b) * voxel_mm3;
  v.distances_ok = c.ab.found && c.ba.found && c.ab.n && c.ba.n;
  if (v.distances_ok) {
    v.hausdorff_mm = std::sqrt((double)std::max(c.ab.max_um2, c.ba.max_um2)) / 1000.0;
    v.hd95_mm = (double)std::max(c.ab.p95_um, c.ba.p95_um) / 1000.0;
    v.msd_ab_mm = (double)c.ab.sum_um / (double)c.ab.n / 1000.0;
    v.msd_ba_mm = (double)c.ba.sum_um / (double)c.ba.n / 1000.0;
    v.assd_mm = (double)(c.ab.sum_um + c.ba.sum_um) / ((double)c.ab.n + (double)c.ba.n) / 1000.0;
  }
  return v;
}

std::string to_json(const VolumeCompare& c, int w, int h, int d, const uint32_t um[3], const std::string& reference,
                    const VolumeCompareLesions* lesions) {
  std::string s = "{";
  bool first = true;
  for (const Field& f : fields(c, w, h, d, um, reference)) {
    if (!first) s += ',';
    first = false;
    s += '"';
    s += f.key;
    s += "\":";
    s += f.json;
  }
  if (lesions) s += lesions_json_keys(*lesions);
  return s + "}\n";
}

std::string csv_header(bool lesions) {
  static const char* axes[3] = {"_x", "_y", "_z"};
  const uint32_t um[3] = {1, 1, 1};
  std::string s = "patient,status";
  for (const Field& f : fields(VolumeCompare{}, 1, 1, 1, um, std::string())) {
    if (f.columns == 1) s += std::string(",") + f.key;
    else
      for (const char* ax : axes) s += std::string(",") + f.key + ax;
  }
  if (lesions) s += lesions_csv_header_fields();
  return s;
}

std::string csv_fields(const VolumeCompare& c, int w, int h, int d, const uint32_t um[3], const std::string& reference,
                       const VolumeCompareLesions* lesions) {
  std::string s;
  bool first = true;
  for (const Field& f : fields(c, w, h, d, um, reference)) {
    if (!first) s += ',';
    first = false;
    s += f.csv;
  }
  if (lesions) s += lesions_csv_fields(*lesions);
  return s;
}

}  // namespace compare

namespace golden {

std::vector<uint8_t> volume_surface(const std::vector<uint8_t>& m, int w, int h, int d) {
  const size_t n = (size_t)w * h * d, plane = (size_t)w * h;
  if (w < 1 || h < 1 || d < 1 || m.size() != n) throw std::invalid_argument("golden::volume_surface: the mask must hold w * h * d voxels");
  auto in = [&](int x, int y, int z) { return x >= 0 && x < w && y >= 0 && y < h && z >= 0 && z < d && m[(size_t)z * plane + (size_t)y * w + x]; };
  std::vector<uint8_t> s(n, 0);
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        s[(size_t)z * plane + (size_t)y * w + x] =
            in(x, y, z) && !(in(x - 1, y, z) && in(x + 1, y, z) && in(x, y - 1, z) && in(x, y + 1, z) && in(x, y, z - 1) && in(x, y, z + 1));
  return s;
}

namespace {

VolumeCompareDirected directed(const std::vector<uint8_t>& from, const std::vector<uint8_t>& to, uint64_t n_from, uint64_t n_to, int w, int h,
                               int d, const uint32_t um[3]) {
  if (n_from == 0 || n_to == 0) return not_found();
  const std::vector<int64_t> D = volume_distance(to, w, h, d, um, false, -1);
  VolumeCompareDirected r = not_found();
  std::vector<uint32_t> s;
  s.reserve((size_t)n_from);
  for (size_t p = 0; p < from.size(); ++p) {
    if (!from[p]) continue;
    uint64_t q = (uint64_t)std::sqrt((long double)D[p]);  // an integer square root of its own, by search around the estimate
    while (q * q > (uint64_t)D[p]) --q;
    while ((q + 1) * (q + 1) <= (uint64_t)D[p]) ++q;
    s.push_back((uint32_t)q);
    r.sum_um += q;
    if (!r.found || (uint64_t)D[p] > r.max_um2) {  // raster order: the first one at the maximum stays
      r.max_um2 = (uint64_t)D[p];
      set_worst(r, (uint64_t)p, w, h);
      r.found = 1;
    }
  }
  std::sort(s.begin(), s.end());
  r.n = (uint32_t)s.size();
  r.p95_um = s[(size_t)((95ull * s.size() + 99ull) / 100ull) - 1];
  return r;
}

}  // namespace

VolumeCompare compare_volumes(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int w, int h, int d, const uint32_t um[3]) {
  check_args("golden::compare_volumes", w, h, d, um);
  const size_t n = (size_t)w * h * d;
  if (a.size() != n || b.size() != n) throw std::invalid_argument("golden::compare_volumes: both masks must hold w * h * d voxels");
  VolumeCompare c{};
  for (size_t i = 0; i < n; ++i) {
    const bool ia = a[i] != 0, ib = b[i] != 0;
    c.a_vox += ia, c.b_vox += ib, c.tp_vox += ia && ib, c.fp_vox += ia && !ib, c.fn_vox += ib && !ia;
  }
  const std::vector<uint8_t> sa = volume_surface(a, w, h, d), sb = volume_surface(b, w, h, d);
  for (size_t i = 0; i < n; ++i) c.surface_a += sa[i], c.surface_b += sb[i];
  c.ab = directed(sa, sb, c.surface_a, c.surface_b, w, h, d, um);
  c.ba = directed(sb, sa, c.surface_b, c.surface_a, w, h, d, um);
  return c;
}

}  // namespace golden
}  // namespace nm03
